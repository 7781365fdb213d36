"""Same-process A/B of the BSGS linear transform (ofhe_hip_ks_bsgs_transform)
against the composition of the calls shipped before it, term by term as the
loop of FHECKKSRNS::EvalLinearTransform (ckksrns-fhe.cpp:1507-1552), batch 1,
full level, on

  configs[4]   N = 2^17, Q = 48, P = 16, dnum = 3, nbaby = ngiant = 8
  a small one  N = 2^15, Q = 24, P = 8,  dnum = 3, nbaby = ngiant = 4

  (a) composition  precompute + fast_rotation_ext (the babies, one call); per giant step
                   KeySwitchExt as modmul_scalar into a zeroed Ql|P polynomial,
                   modmul_vv / modadd_vv per term and element over Ql|P; then
                   mod_down (x2, or x1 at the identity giant), automorphism + modadd_vv
                   (first), precompute + fast_rotation_ext + 2 modadd_vv (outer);
                   at the end 2 mod_down + modadd_vv
  (b) the new call ofhe_hip_ks_bsgs_transform

Baby and giant step 0 are the identity, as in EvalLinearTransform; every
diagonal is present.  The outputs of (a) and (b) are checked for equality
first.  Then, after a warm-up, the contenders alternate (the order flips every
round) for --repeats rounds, each call timed with device events.  The two
accumulation stages are also timed alone through their stage calls
(ofhe_hip_ks_mult_ext_sum: k_lt_inner; ofhe_hip_ks_fast_rotation_ext_sum:
k_lt_outer) and their achieved bytes/s computed from the words each moves;
the rest of the fused call (its ModUp, ModDown and baby-rotation launch sets)
is timed through the earlier entry points at the batch sizes the call uses
(part_*), so that a loss can be placed.

Writes medians and spread to profiles/linear_transform_ab.json (--out).
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

SHAPES = {"configs4": (17, 48, 16, 3, 8, 8), "small": (15, 24, 8, 3, 4, 4)}
ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="configs4,small")
ap.add_argument("--repeats", type=int, default=11)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "linear_transform_ab.json"))
a = ap.parse_args()
assert a.repeats >= 11, "at least 11 rounds"
ctx = H.Context(0)
g = torch.Generator(device="cuda")
g.manual_seed(12)
s = torch.cuda.current_stream()
st = s.cuda_stream


def uniform(shape, moduli):
    x = torch.empty(shape, dtype=torch.int64, device="cuda")
    for t, m in enumerate(moduli):
        x[..., t, :].random_(0, m, generator=g)
    return x


def empty(*shape):
    return torch.empty(shape, dtype=torch.int64, device="cuda")


def run_shape(log_n, sq, sp, dnum, nb, ng, repeats):
    n, l, B = 1 << log_n, sq, 1
    allq, allr = bench.moduli_chain(log_n, sq + sp)
    q, p = allq[:sq], allq[sq:]
    ks = H.KeySwitch(ctx, log_n, q, allr[:sq], p, allr[sq:], dnum)
    plan_q = H.NTTPlan(ctx, log_n, q, allr[:sq])
    plan_qp = H.NTTPlan(ctx, log_n, allq, allr)
    beta = ks.digits(l)[1]
    c0, c1 = uniform((B, l, n), q), uniform((B, l, n), q)
    diag = uniform((ng * nb, l + sp, n), allq)
    baby = [1] + [pow(5, i, 2 * n) for i in range(1, nb)]
    giant = [1] + [pow(5, nb * j, 2 * n) for j in range(1, ng)]
    key = lambda: (uniform((dnum, sq + sp, n), allq), uniform((dnum, sq + sp, n), allq))  # noqa: E731
    bkeys, gkeys = [None] + [key() for _ in baby[1:]], [None] + [key() for _ in giant[1:]]
    kptr = lambda keys, e: [0 if k is None else k[e].data_ptr() for k in keys]  # noqa: E731
    P = 1
    for m in p:
        P *= m
    pmodq = [P % m for m in q]
    poly = (l + sp) * n

    # (a) the composition's buffers
    dg, dg2 = empty(B, beta, l + sp, n), empty(B, beta, l + sp, n)
    r0, r1 = empty(nb - 1, B, l + sp, n), empty(nb - 1, B, l + sp, n)
    x0, x1 = torch.zeros((B, l + sp, n), dtype=torch.int64, device="cuda"), torch.zeros(
        (B, l + sp, n), dtype=torch.int64, device="cuda")  # KeySwitchExt: the P towers stay zero
    in0, in1, tm0, tm1, ou0, ou1, e0, e1 = (empty(B, l + sp, n) for _ in range(8))
    m0, m1, rot, first, a0, a1 = (empty(B, l, n) for _ in range(6))
    b0, b1 = empty(B, l, n), empty(B, l, n)

    def composition():
        ks.precompute(l, c1.data_ptr(), dg.data_ptr(), B, st)
        ks.fast_rotation_ext(l, dg.data_ptr(), c0.data_ptr(), baby[1:], kptr(bkeys[1:], 0), kptr(bkeys[1:], 1),
                             r0.data_ptr(), r1.data_ptr(), B, st)
        for j in range(ng):
            # batch 1: the Q towers lead the Ql|P polynomial
            plan_q.mod_mul_scalar(c0.data_ptr(), pmodq, x0.data_ptr(), B, st)
            plan_q.mod_mul_scalar(c1.data_ptr(), pmodq, x1.data_ptr(), B, st)
            plan_qp.mod_mul(x0.data_ptr(), diag[j * nb].data_ptr(), in0.data_ptr(), B, st)
            plan_qp.mod_mul(x1.data_ptr(), diag[j * nb].data_ptr(), in1.data_ptr(), B, st)
            for i in range(1, nb):
                d = diag[j * nb + i].data_ptr()
                plan_qp.mod_mul(r0[i - 1].data_ptr(), d, tm0.data_ptr(), B, st)
                plan_qp.mod_mul(r1[i - 1].data_ptr(), d, tm1.data_ptr(), B, st)
                plan_qp.mod_add(in0.data_ptr(), tm0.data_ptr(), in0.data_ptr(), B, st)
                plan_qp.mod_add(in1.data_ptr(), tm1.data_ptr(), in1.data_ptr(), B, st)
            if j == 0:
                ks.mod_down(l, in0.data_ptr(), first.data_ptr(), 0, B, st)
                ou0.zero_()
                ou1.copy_(in1)
                continue
            ks.mod_down(l, in0.data_ptr(), m0.data_ptr(), 0, B, st)
            ks.mod_down(l, in1.data_ptr(), m1.data_ptr(), 0, B, st)
            plan_q.automorphism(giant[j], True, m0.data_ptr(), rot.data_ptr(), B, st)
            plan_q.mod_add(first.data_ptr(), rot.data_ptr(), first.data_ptr(), B, st)
            ks.precompute(l, m1.data_ptr(), dg2.data_ptr(), B, st)
            ks.fast_rotation_ext(l, dg2.data_ptr(), 0, [giant[j]], [gkeys[j][0].data_ptr()],
                                 [gkeys[j][1].data_ptr()], e0.data_ptr(), e1.data_ptr(), B, st)
            plan_qp.mod_add(ou0.data_ptr(), e0.data_ptr(), ou0.data_ptr(), B, st)
            plan_qp.mod_add(ou1.data_ptr(), e1.data_ptr(), ou1.data_ptr(), B, st)
        ks.mod_down(l, ou0.data_ptr(), a0.data_ptr(), 0, B, st)
        ks.mod_down(l, ou1.data_ptr(), a1.data_ptr(), 0, B, st)
        plan_q.mod_add(a0.data_ptr(), first.data_ptr(), a0.data_ptr(), B, st)

    def fused():
        ks.bsgs_transform(l, baby, giant, kptr(bkeys, 0), kptr(bkeys, 1), kptr(gkeys, 0), kptr(gkeys, 1),
                          diag.data_ptr(), poly, None, c0.data_ptr(), c1.data_ptr(), b0.data_ptr(), b1.data_ptr(),
                          0, B, st)

    with torch.cuda.stream(s):
        composition(), fused()
    torch.cuda.synchronize()
    assert torch.equal(a0, b0) and torch.equal(a1, b1), "the new call differs from the composition"
    print("outputs equal; timing", flush=True)

    # the stages alone, on buffers of the transform's sizes
    sx0, sx1 = uniform((nb, B, l + sp, n), allq), uniform((nb, B, l + sp, n), allq)
    so0, so1 = empty(ng, B, l + sp, n), empty(ng, B, l + sp, n)
    nset = ng - 1
    sdg = uniform((nset, B, beta, l + sp, n), allq)
    to0, to1 = empty(B, l + sp, n), empty(B, l + sp, n)

    def stage_inner():
        ks.mult_ext_sum(l, nb, sx0.data_ptr(), sx1.data_ptr(), B * poly, diag.data_ptr(), poly, None, ng,
                        so0.data_ptr(), so1.data_ptr(), B, st)

    def stage_outer():
        ks.fast_rotation_ext_sum(l, sdg.data_ptr(), giant[1:], kptr(gkeys[1:], 0), kptr(gkeys[1:], 1),
                                 so1[0].data_ptr(), 1, to0.data_ptr(), to1.data_ptr(), B, st)

    # the rest of the fused call through the earlier entry points, at the batch sizes it uses
    pm = uniform((nset, B, l, n), q)
    pdg = empty(nset, B, beta, l + sp, n)
    md_in, md_out = uniform((2 * nset, B, l + sp, n), allq), empty(2 * nset, B, l, n)
    parts = {
        "part_precompute_c1": lambda: ks.precompute(l, c1.data_ptr(), dg.data_ptr(), B, st),
        "part_baby_rotations": lambda: ks.fast_rotation_ext(
            l, dg.data_ptr(), c0.data_ptr(), baby[1:], kptr(bkeys[1:], 0), kptr(bkeys[1:], 1), r0.data_ptr(),
            r1.data_ptr(), B, st),
        "part_mod_down_giants": lambda: ks.mod_down(l, md_in.data_ptr(), md_out.data_ptr(), 0, 2 * nset * B, st),
        "part_precompute_giants": lambda: ks.precompute(l, pm.data_ptr(), pdg.data_ptr(), nset * B, st),
        # the two outer sums and the identity giant's first element
        "part_mod_down_last": lambda: ks.mod_down(l, md_in.data_ptr(), md_out.data_ptr(), 0, 3 * B, st),
    }
    # not a part of the fused call: the ModDown of one polynomial on its own, as the composition runs it
    single = {"single_mod_down": lambda: ks.mod_down(l, md_in.data_ptr(), md_out.data_ptr(), 0, B, st)}
    contenders = {"composition": composition, "bsgs_transform": fused, "stage_mult_ext_sum": stage_inner,
                  "stage_fast_rotation_ext_sum": stage_outer, **parts, **single}
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
    res = {"shape": dict(log_n=log_n, Q=sq, P=sp, dnum=dnum, beta=beta, batch=B, nbaby=nb, ngiant=ng, level=l),
           "repeats": repeats, "unit": "ms per call", "contenders": {}}
    for name, tt in times.items():
        res["contenders"][name] = dict(median=statistics.median(tt), min=min(tt), max=max(tt))
        print(f"{name:28s} median {statistics.median(tt):9.3f} ms  [min {min(tt):.3f}, max {max(tt):.3f}]", flush=True)
    c = res["contenders"]
    res["ratio_new_over_composition"] = c["bsgs_transform"]["median"] / c["composition"]["median"]
    res["spreads_overlap"] = c["bsgs_transform"]["max"] >= c["composition"]["min"]
    res["sum_of_parts_and_stages_median"] = sum(v["median"] for k, v in c.items() if k.startswith(("part_", "stage_")))
    print(f"sum of the parts' and stages' medians {res['sum_of_parts_and_stages_median']:.3f} ms", flush=True)
    # words per (tower, coefficient): k_lt_inner reads 2 nb term words and nb ng diagonal words and
    # writes 2 ng; k_lt_outer reads beta digit and 2 beta key words per set and one addend, writes 2
    words = {"stage_mult_ext_sum": 2 * nb + nb * ng + 2 * ng, "stage_fast_rotation_ext_sum": 3 * beta * nset + 1 + 2}
    for name, w in words.items():
        byts = 8 * w * B * poly
        res["contenders"][name].update(words_per_position=w, bytes=byts,
                                       tb_per_s=byts / (c[name]["median"] * 1e-3) / 1e12)
        print(f"{name:28s} {w} words per (tower, coefficient): {res['contenders'][name]['tb_per_s']:.2f} TB/s", flush=True)
    ks.close(), plan_q.close(), plan_qp.close()
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
