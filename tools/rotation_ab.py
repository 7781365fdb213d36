"""Same-process A/B of the hoisted rotations against the composition of the
entry points they replace, on configs[4] (N = 2^17, Q = 48, P = 16, dnum = 3),
batch 1, R = 8 distinct keys, full level.

  (a) composition  Ext:     fast_core_ext + modmul_scalar / modadd_vv (addFirst)
                            + two automorphism calls, per rotation
                   non-Ext: fast_core_ext + two mod_down + modadd_vv
                            + two automorphism calls, per rotation
  (b) the new call ofhe_hip_ks_fast_rotation_ext / ofhe_hip_ks_fast_rotation

The outputs of (a) and (b) are checked for equality first.  Then, after a
warm-up, the contenders alternate (the order flips every round) for --repeats
rounds, each call timed with device events.

Writes medians and spread to profiles/rotation_ab.json (--out).
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "upmem--openfhe_amd"))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench  # noqa: E402
import ofhe_hip as H  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--log-n", type=int, default=17)
ap.add_argument("--q", type=int, default=48)
ap.add_argument("--p", type=int, default=16)
ap.add_argument("--dnum", type=int, default=3)
ap.add_argument("--rotations", type=int, default=8)
ap.add_argument("--repeats", type=int, default=11)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rotation_ab.json"))
a = ap.parse_args()
log_n, sq, sp, dnum, R = a.log_n, a.q, a.p, a.dnum, a.rotations
n, l, B = 1 << log_n, sq, 1
allq, allr = bench.moduli_chain(log_n, sq + sp)
q, p = allq[:sq], allq[sq:]
g = torch.Generator(device="cuda")
g.manual_seed(11)


def uniform(shape, moduli):
    x = torch.empty(shape, dtype=torch.int64, device="cuda")
    for t, m in enumerate(moduli):
        x[..., t, :].random_(0, m, generator=g)
    return x


ctx = H.Context(0)
ks = H.KeySwitch(ctx, log_n, q, allr[:sq], p, allr[sq:], dnum)
plan_q = H.NTTPlan(ctx, log_n, q, allr[:sq])
plan_qp = H.NTTPlan(ctx, log_n, allq, allr)
beta = ks.digits(l)[1]
digits = uniform((B, beta, l + sp, n), allq)
c0 = uniform((B, l, n), q)
keys = [(uniform((dnum, sq + sp, n), allq), uniform((dnum, sq + sp, n), allq)) for _ in range(R)]
idx = [pow(5, r + 1, 2 * n) for r in range(R)]
kb, ka = [b.data_ptr() for b, _ in keys], [x.data_ptr() for _, x in keys]
P = 1
for m in p:
    P *= m
pmodq = [P % m for m in q]
ext = lambda: torch.empty((R, B, l + sp, n), dtype=torch.int64, device="cuda")  # noqa: E731
low = lambda: torch.empty((R, B, l, n), dtype=torch.int64, device="cuda")  # noqa: E731
ea0, ea1, eb0, eb1 = ext(), ext(), ext(), ext()
na0, na1, nb0, nb1 = low(), low(), low(), low()
ct0, ct1 = (torch.empty((B, l + sp, n), dtype=torch.int64, device="cuda") for _ in range(2))
cm, md0, md1 = (torch.empty((B, l, n), dtype=torch.int64, device="cuda") for _ in range(3))
s = torch.cuda.current_stream()
st = s.cuda_stream


def compose_ext():
    for r in range(R):
        ks.fast_core_ext(l, digits.data_ptr(), kb[r], ka[r], ct0.data_ptr(), ct1.data_ptr(), B, st)
        plan_q.mod_mul_scalar(c0.data_ptr(), pmodq, cm.data_ptr(), B, st)
        plan_q.mod_add(ct0.data_ptr(), cm.data_ptr(), ct0.data_ptr(), B, st)  # batch 1: the Q towers lead ct0
        plan_qp.automorphism(idx[r], True, ct0.data_ptr(), ea0[r].data_ptr(), B, st)
        plan_qp.automorphism(idx[r], True, ct1.data_ptr(), ea1[r].data_ptr(), B, st)


def new_ext():
    ks.fast_rotation_ext(l, digits.data_ptr(), c0.data_ptr(), idx, kb, ka, eb0.data_ptr(), eb1.data_ptr(), B, st)


def compose_plain():
    for r in range(R):
        ks.fast_core_ext(l, digits.data_ptr(), kb[r], ka[r], ct0.data_ptr(), ct1.data_ptr(), B, st)
        ks.mod_down(l, ct0.data_ptr(), md0.data_ptr(), 0, B, st)
        ks.mod_down(l, ct1.data_ptr(), md1.data_ptr(), 0, B, st)
        plan_q.mod_add(md0.data_ptr(), c0.data_ptr(), md0.data_ptr(), B, st)
        plan_q.automorphism(idx[r], True, md0.data_ptr(), na0[r].data_ptr(), B, st)
        plan_q.automorphism(idx[r], True, md1.data_ptr(), na1[r].data_ptr(), B, st)


def new_plain():
    ks.fast_rotation(l, digits.data_ptr(), c0.data_ptr(), idx, kb, ka, nb0.data_ptr(), nb1.data_ptr(), 0, B, st)


compose_ext(), new_ext(), compose_plain(), new_plain()
torch.cuda.synchronize()
assert torch.equal(ea0, eb0) and torch.equal(ea1, eb1), "Ext: the new call differs from the composition"
assert torch.equal(na0, nb0) and torch.equal(na1, nb1), "non-Ext: the new call differs from the composition"
print("outputs equal; timing", flush=True)

contenders = {"ext_composition": compose_ext, "ext_new": new_ext,
              "plain_composition": compose_plain, "plain_new": new_plain}
times = {k: [] for k in contenders}
for rnd in range(a.repeats + 1):  # round 0 is a second warm-up
    order = list(contenders.items())
    for name, fn in (order if rnd % 2 == 0 else order[::-1]):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        fn()
        e1.record(s)
        e1.synchronize()
        if rnd:
            times[name].append(e0.elapsed_time(e1))

res = {"shape": dict(log_n=log_n, Q=sq, P=sp, dnum=dnum, beta=beta, batch=B, rotations=R, level=l),
       "repeats": a.repeats, "unit": "ms per call (all rotations)", "contenders": {}}
for name, tt in times.items():
    res["contenders"][name] = dict(median=statistics.median(tt), min=min(tt), max=max(tt))
    print(f"{name:24s} median {statistics.median(tt):8.3f} ms  [min {min(tt):.3f}, max {max(tt):.3f}]", flush=True)
c = res["contenders"]
for kind in ("ext", "plain"):
    res[kind + "_ratio_new_over_composition"] = c[kind + "_new"]["median"] / c[kind + "_composition"]["median"]
    res[kind + "_spreads_overlap"] = c[kind + "_new"]["max"] >= c[kind + "_composition"]["min"]
print(json.dumps({k: v for k, v in res.items() if k.endswith(("ratio_new_over_composition", "overlap"))}), flush=True)
os.makedirs(os.path.dirname(a.out), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
