"""Same-process A/B of CKKS / BGV multiplication with relinearisation and one
rescaling (ofhe_hip_ks_eval_mult, levels = 1) against the composition of the
calls shipped before it, at full level, on

  ks17_b1, ks17_b8   N = 2^17, Q = 48, P = 16, dnum = 3 (the bench's key-switching shape), batch 1 and 8
  small_b8           N = 2^15, Q = 24, P = 8,  dnum = 3, batch 8; also with BGV (t = 65537)

  (a) composition   eval_mult_core, ks_core on the third element, 2 x modadd_vv,
                    2 x drop_last_and_scale (BGV: mod_reduce) with tables built here
  (b) eval_mult     ofhe_hip_ks_eval_mult
  (c) eval_square   the same call with d0 = d1 = NULL, against (a) with c = d

and, alone: ofhe_hip_ks_relinearize of three elements (the ModDown takes the
sums in its last pass) against ks_core + 2 x modadd_vv; ofhe_hip_ks_rescale of
two elements against two calls of one element; the product with levels = 0
against its square (they differ by k_tensor2 - k_square2) next to
eval_mult_core (k_tensor2 alone), with k_tensor2's achieved bytes/s from the
56 B it moves per coefficient (k_square2: 40 B).

The outputs of (a), (b) and (c) are checked for equality first.  Then, after a
warm-up, the contenders alternate (the order flips every round) for --repeats
rounds, each call timed with device events.  Writes medians and spread to
profiles/she_mult_ab.json (--out).
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

SHAPES = {"ks17_b1": (17, 48, 16, 3, 1, 0), "ks17_b8": (17, 48, 16, 3, 8, 0), "small_b8": (15, 24, 8, 3, 8, 0),
          "small_b8_bgv": (15, 24, 8, 3, 8, 65537)}
ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default=",".join(SHAPES))
ap.add_argument("--repeats", type=int, default=11)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "she_mult_ab.json"))
a = ap.parse_args()
assert a.repeats >= 11, "at least 11 rounds"
ctx = H.Context(0)
g = torch.Generator(device="cuda")
g.manual_seed(14)
s = torch.cuda.current_stream()
st = s.cuda_stream


def uniform(shape, moduli):
    x = torch.empty(shape, dtype=torch.int64, device="cuda")
    for t, m in enumerate(moduli):
        x[..., t, :].random_(0, m, generator=g)
    return x


def empty(*shape):
    return torch.empty(shape, dtype=torch.int64, device="cuda")


def run_shape(log_n, sq, sp, dnum, B, t, repeats):
    n, l = 1 << log_n, sq
    scheme = H.SHE_BGV if t else H.SHE_CKKS
    allq, allr = bench.moduli_chain(log_n, sq + sp)
    q, p = allq[:sq], allq[sq:]
    ks = H.KeySwitch(ctx, log_n, q, allr[:sq], p, allr[sq:], dnum)
    plan_q = H.NTTPlan(ctx, log_n, q, allr[:sq])
    c0, c1, d0, d1 = (uniform((B, l, n), q) for _ in range(4))
    kb, ka = uniform((dnum, sq + sp, n), allq), uniform((dnum, sq + sp, n), allq)
    # the tables the composition's caller builds (ckksrns-cryptoparameters.cpp:66-87, bgvrns-cryptoparameters.cpp:91-107)
    ql = q[l - 1]
    ql_inv = [pow(ql, -1, m) for m in q[:l - 1]]
    ckks_c = [m - v for m, v in zip(q[:l - 1], ql_inv)]
    neg_t_inv = (ql - pow(t % ql, -1, ql)) % ql if t else 0

    o0, o1, o2, k0, k1 = (empty(B, l, n) for _ in range(5))
    a0, a1, b0, b1, s0, s1, e0, e1 = (empty(B, l - 1, n) for _ in range(8))

    def rescale_one(x, out):
        if t:
            plan_q.mod_reduce(l, x.data_ptr(), l * n, out.data_ptr(), (l - 1) * n, True, t, neg_t_inv, ql_inv, B, st)
        else:
            plan_q.drop_last_and_scale(l, x.data_ptr(), l * n, out.data_ptr(), (l - 1) * n, True, ckks_c, ql_inv, B, st)

    def composition(x0=d0, x1=d1, r0=a0, r1=a1):
        plan_q.eval_mult_core(c0.data_ptr(), c1.data_ptr(), x0.data_ptr(), x1.data_ptr(), o0.data_ptr(),
                              o1.data_ptr(), o2.data_ptr(), B, st)
        ks.core(l, o2.data_ptr(), kb.data_ptr(), ka.data_ptr(), k0.data_ptr(), k1.data_ptr(), t, B, st)
        plan_q.mod_add(o0.data_ptr(), k0.data_ptr(), o0.data_ptr(), B, st)
        plan_q.mod_add(o1.data_ptr(), k1.data_ptr(), o1.data_ptr(), B, st)
        rescale_one(o0, r0)
        rescale_one(o1, r1)

    def composition_square():
        composition(c0, c1, e0, e1)

    def fused(levels=1, r0=b0, r1=b1):
        ks.eval_mult(l, c0.data_ptr(), c1.data_ptr(), d0.data_ptr(), d1.data_ptr(), kb.data_ptr(), ka.data_ptr(),
                     r0.data_ptr(), r1.data_ptr(), scheme, t, levels, B, st)

    def fused_square(levels=1, r0=s0, r1=s1):
        ks.eval_square(l, c0.data_ptr(), c1.data_ptr(), kb.data_ptr(), ka.data_ptr(), r0.data_ptr(), r1.data_ptr(),
                       scheme, t, levels, B, st)

    with torch.cuda.stream(s):
        composition(), fused(), composition_square(), fused_square()
    torch.cuda.synchronize()
    assert torch.equal(a0, b0) and torch.equal(a1, b1), "eval_mult differs from the composition"
    assert torch.equal(e0, s0) and torch.equal(e1, s1), "eval_square differs from the composition with c = d"
    print("outputs equal; timing", flush=True)

    # the pieces alone
    f0, f1, g0, g1 = (empty(B, l, n) for _ in range(4))
    x3 = [c0, c1, d0]

    def relinearize_fused():
        ks.relinearize(l, [x.data_ptr() for x in x3], [kb.data_ptr()], [ka.data_ptr()], f0.data_ptr(), f1.data_ptr(),
                       t, B, st)

    def relinearize_separate():
        ks.core(l, d0.data_ptr(), kb.data_ptr(), ka.data_ptr(), k0.data_ptr(), k1.data_ptr(), t, B, st)
        plan_q.mod_add(c0.data_ptr(), k0.data_ptr(), g0.data_ptr(), B, st)
        plan_q.mod_add(c1.data_ptr(), k1.data_ptr(), g1.data_ptr(), B, st)

    def rescale_pair():
        ks.rescale(l, [c0.data_ptr(), c1.data_ptr()], [a0.data_ptr(), a1.data_ptr()], scheme, t, 1, B, st)

    def rescale_twice():
        ks.rescale(l, [c0.data_ptr()], [a0.data_ptr()], scheme, t, 1, B, st)
        ks.rescale(l, [c1.data_ptr()], [a1.data_ptr()], scheme, t, 1, B, st)

    def tensor_alone():
        plan_q.eval_mult_core(c0.data_ptr(), c1.data_ptr(), d0.data_ptr(), d1.data_ptr(), o0.data_ptr(),
                              o1.data_ptr(), o2.data_ptr(), B, st)

    with torch.cuda.stream(s):
        relinearize_fused(), relinearize_separate()
    torch.cuda.synchronize()
    assert torch.equal(f0, g0) and torch.equal(f1, g1), "relinearize differs from ks_core + 2 additions"

    contenders = {"composition": composition, "eval_mult": fused, "composition_square": composition_square,
                  "eval_square": fused_square, "relinearize_fused_tail": relinearize_fused,
                  "relinearize_separate_adds": relinearize_separate, "rescale_two_elements": rescale_pair,
                  "rescale_one_element_twice": rescale_twice, "k_tensor2_alone": tensor_alone,
                  "eval_mult_levels0": lambda: fused(0, f0, f1), "eval_square_levels0": lambda: fused_square(0, g0, g1)}
    times = {k: [] for k in contenders}
    for rnd in range(repeats + 1):  # round 0 is a second warm-up
        order = list(contenders.items())
        for name, fn in (order if rnd % 2 == 0 else order[::-1]):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(s)
            fn()
            t1.record(s)
            t1.synchronize()
            if rnd:
                times[name].append(t0.elapsed_time(t1))
    res = {"shape": dict(log_n=log_n, Q=sq, P=sp, dnum=dnum, batch=B, level=l, t=t, levels=1),
           "repeats": repeats, "unit": "ms per call", "contenders": {}}
    for name, tt in times.items():
        res["contenders"][name] = dict(median=statistics.median(tt), min=min(tt), max=max(tt))
        print(f"{name:28s} median {statistics.median(tt):9.3f} ms  [min {min(tt):.3f}, max {max(tt):.3f}]", flush=True)
    c = res["contenders"]
    for new, old in (("eval_mult", "composition"), ("eval_square", "composition_square"),
                     ("relinearize_fused_tail", "relinearize_separate_adds"),
                     ("rescale_two_elements", "rescale_one_element_twice")):
        spread = c[old]["max"] - c[old]["min"]
        res[f"{new}_minus_{old}_ms"] = c[new]["median"] - c[old]["median"]
        res[f"{old}_spread_ms"] = spread
        res[f"{new}_within_bar"] = c[new]["median"] - c[old]["median"] <= spread
    # the traffic the fused tail removes: a write and a read of both key-switch results and the sums' own
    # read / write of the first two elements, 2 * 3 * size_ql * N words
    res["removed_bytes_two_additions"] = 2 * 3 * l * n * 8 * B
    coeffs = B * l * n
    c["k_tensor2_alone"].update(bytes=56 * coeffs, tb_per_s=56 * coeffs / (c["k_tensor2_alone"]["median"] * 1e-3) / 1e12)
    # k_square2 = k_tensor2 - (product - square) with levels = 0: the two calls differ by that kernel only
    sq_ms = c["k_tensor2_alone"]["median"] - (c["eval_mult_levels0"]["median"] - c["eval_square_levels0"]["median"])
    res["k_square2_derived"] = dict(median=sq_ms, bytes=40 * coeffs,
                                    tb_per_s=(40 * coeffs / (sq_ms * 1e-3) / 1e12) if sq_ms > 0 else None)
    print(f"k_tensor2 {c['k_tensor2_alone']['tb_per_s']:.2f} TB/s; k_square2 (derived) {sq_ms:.3f} ms", flush=True)
    ks.close(), plan_q.close()
    return res


out = {}
for name in a.shapes.split(","):
    print("shape", name, SHAPES[name], flush=True)
    out[name] = run_shape(*SHAPES[name], a.repeats)
    torch.cuda.empty_cache()
os.makedirs(os.path.dirname(a.out), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
