"""Same-process timings of the BFV (BEHZ) multiplication calls.

  (a) ofhe_hip_behz_q_to_bsk, ofhe_hip_behz_floor and ofhe_hip_behz_conv_sk, each
      against the bytes it has to move over 8 TB/s.
  (b) the fused floor -> SK launch (ofhe_hip_behz_floor_sk, fused = 1) against
      the two launches (ofhe_hip_behz_floor into a preallocated buffer, then
      ofhe_hip_behz_conv_sk).
  (c) ofhe_hip_bfv_eval_mult_behz against ofhe_hip_bfv_eval_mult (HPS, R = Q + 1
      towers) at the same N, Q and batch, with the BEHZ stages timed through
      the public calls they are made of.

B and msk are the 60-bit primes that follow q in the descending chain, which is
the reference's choice (bfvrns-cryptoparameters.cpp:674-703) when its msk loop
does not run; that is asserted.  Outputs are checked for equality first ((b):
fused equals two launches; (c): the staged calls equal the one call).  Then,
after a warm-up, the contenders alternate (the order flips every round) for
--repeats rounds; a sample is a short run of back-to-back calls between two
device events.  Writes medians and spread to profiles/behz_mult_ab.json (--out).
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
import bfv_tables as BT  # noqa: E402
import ofhe_hip as H  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="14:8:8,16:16:4", help="log_n:Q:batch, comma separated")
ap.add_argument("--repeats", type=int, default=11)
ap.add_argument("--inner-kernel", type=int, default=20, help="back-to-back calls per sample, single kernels")
ap.add_argument("--inner-mult", type=int, default=5, help="back-to-back calls per sample, eval_mult and its stages")
ap.add_argument("--t", type=int, default=65537)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "behz_mult_ab.json"))
a = ap.parse_args()
HBM = 8e12  # bytes / s
g = torch.Generator(device="cuda")
g.manual_seed(29)
s = torch.cuda.current_stream()
st = s.cuda_stream
ctx = H.Context(0)


def uniform(shape, moduli):
    x = torch.empty(shape, dtype=torch.int64, device="cuda")
    for t, m in enumerate(moduli):
        x[..., t, :].random_(0, m, generator=g)
    return x


def empty(*shape):
    return torch.empty(shape, dtype=torch.int64, device="cuda")


def race(contenders, repeats, inner):
    """{name: dict(median, min, max)} in ms per call; the contenders alternate, order flipped every
    round.  One sample is `inner` back-to-back calls between two device events, divided by inner."""
    times = {k: [] for k in contenders}
    for rnd in range(repeats + 1):  # round 0 is a second warm-up
        order = list(contenders.items())
        for name, fn in (order if rnd % 2 == 0 else order[::-1]):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            for _ in range(inner):
                fn()
            e1.record(s)
            e1.synchronize()
            if rnd:
                times[name].append(e0.elapsed_time(e1) / inner)
    return {k: dict(median=statistics.median(v), min=min(v), max=max(v)) for k, v in times.items()}


def hps_mult(log_n, sq, B, cts):
    """ofhe_hip_bfv_eval_mult (HPS, R = Q + 1) on the same Q towers and inputs: (call, handles)"""
    sr = sq + 1
    m, roots = bench.moduli_chain(log_n, sq + sr)
    q, r, rq, rr = m[:sq], m[sq:], roots[:sq], roots[sq:]
    T = BT.BfvTables(q, r, a.t, BT.HPS)
    pq, pr, pqr = H.NTTPlan(ctx, log_n, q, rq), H.NTTPlan(ctx, log_n, r, rr), H.NTTPlan(ctx, log_n, m, roots)
    q_to_r = H.BaseConverter(ctx, log_n, q, r, T.q_hat_inv_modq, T.flat(T.q_hat_modr))
    r_to_q = H.BaseConverter(ctx, log_n, r, q, T.r_hat_inv_modr, T.flat(T.r_hat_modq))
    sr_h = H.ScaleRound(ctx, log_n, q, r, T.out_is_q, T.sr_table, T.sr_frac)
    mult = H.BfvMult(ctx, H.BFV_HPS, pq, pr, pqr, q_to_r, r_to_q, None, sr_h)
    outs = [empty(B, sq, 1 << log_n) for _ in range(3)]

    def call():
        mult.eval_mult(*[t.data_ptr() for t in cts + outs], B, st)

    return call, [mult, sr_h, r_to_q, q_to_r, pqr, pr, pq]


def shape_ab(log_n, sq, B):
    n = 1 << log_n
    sb, K = sq, sq + 1
    m, roots = bench.moduli_chain(log_n, sq + K)
    q, b, msk = m[:sq], m[sq:sq + sb], m[sq + sb]
    assert BT.product(b) * msk >= (2 * n) * a.t * BT.product(q), "the reference would regrow msk here"
    T = BT.BehzTables(q, b, msk, a.t)
    bz = H.Behz(ctx, log_n, T)
    pq, pb, pqb = (H.NTTPlan(ctx, log_n, q, roots[:sq]), H.NTTPlan(ctx, log_n, T.bsk, roots[sq:]),
                   H.NTTPlan(ctx, log_n, m, roots))
    w = 8 * B * n  # bytes of one tower over the batch

    # (a), (b): the kernels alone
    xq, xqb, xb = uniform((B, sq, n), q), uniform((B, sq + K, n), m), uniform((B, K, n), T.bsk)
    o_bsk, o_floor, o_sk, o_fused, o_two = empty(B, K, n), empty(B, K, n), empty(B, sq, n), empty(B, sq, n), empty(B, sq, n)

    def two_launches():
        bz.floor(xqb.data_ptr(), o_floor.data_ptr(), B, st)
        bz.conv_sk(o_floor.data_ptr(), o_two.data_ptr(), B, st)

    kernels = {
        "q_to_bsk": lambda: bz.q_to_bsk(xq.data_ptr(), o_bsk.data_ptr(), B, st),
        "floor": lambda: bz.floor(xqb.data_ptr(), o_floor.data_ptr(), B, st),
        "conv_sk": lambda: bz.conv_sk(xb.data_ptr(), o_sk.data_ptr(), B, st),
        "floor_sk_fused": lambda: bz.floor_sk(xqb.data_ptr(), o_fused.data_ptr(), B, st, fused=H.BEHZ_FUSED),
        "floor_sk_two_launches": two_launches,
    }
    for fn in kernels.values():
        fn()
    torch.cuda.synchronize()
    assert torch.equal(o_fused, o_two), "fused floor -> SK differs from the two launches"
    kres = race(kernels, a.repeats, a.inner_kernel)
    kbytes = {"q_to_bsk": w * (sq + K), "floor": w * (sq + K + K), "conv_sk": w * (K + sq),
              "floor_sk_fused": w * (sq + K + sq), "floor_sk_two_launches": w * (sq + K + K + K + sq)}
    fused, two = kres["floor_sk_fused"], kres["floor_sk_two_launches"]
    kernels_out = dict(contenders=kres, bytes=kbytes, hbm_bound_ms={k: v / HBM * 1e3 for k, v in kbytes.items()},
                       over_bound={k: kres[k]["median"] / (v / HBM * 1e3) for k, v in kbytes.items()},
                       fused_over_two_launches=fused["median"] / two["median"],
                       fused_slower_beyond_spread=fused["min"] > two["max"],
                       fused_faster_beyond_spread=fused["max"] < two["min"])

    # (c): the multiplication, its stages, and HPS on the same Q towers
    cts = [uniform((B, sq, n), q) for _ in range(4)]
    outs, outs2 = [empty(B, sq, n) for _ in range(3)], [empty(B, sq, n) for _ in range(3)]
    E, Tp = [empty(B, sq + K, n) for _ in range(4)], empty(3, B, sq + K, n)

    def one_call():
        bz.eval_mult(pq, pb, pqb, *[t.data_ptr() for t in cts + outs], B, st)

    def expand():
        for k in range(4):
            bz.expand(pq, pb, True, cts[k].data_ptr(), E[k].data_ptr(), B, st)

    def tensor():
        pqb.eval_mult_core(*[e.data_ptr() for e in E], Tp[0].data_ptr(), Tp[1].data_ptr(), Tp[2].data_ptr(), B, st)

    def intt():
        pqb.inverse(Tp.data_ptr(), 3 * B, st)

    def floor_sk():
        for k in range(3):
            bz.floor_sk(Tp[k].data_ptr(), outs2[k].data_ptr(), B, st, fused=H.BEHZ_AUTO)

    stages = {"expand": expand, "tensor": tensor, "intt": intt, "floor_sk": floor_sk}
    hps_call, hps_handles = hps_mult(log_n, sq, B, cts)
    one_call()
    for fn in stages.values():
        fn()
    hps_call()
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(outs, outs2)), "eval_mult_behz differs from its staged calls"
    # the stages run in place on each other's buffers in whatever order the rounds take them: the
    # words stay canonical residues, and none of the timings depends on their values
    res = race({"eval_mult_behz": one_call, "eval_mult_hps": hps_call, **stages}, a.repeats, a.inner_mult)
    moved = {"expand": 4 * w * (2 * sq + K), "tensor": 7 * w * (sq + K), "intt": 6 * w * (sq + K),
             "floor_sk": 3 * w * (sq + K + sq)}
    total = sum(moved.values())
    behz, hps = res["eval_mult_behz"], res["eval_mult_hps"]
    mult_out = dict(contenders=res, stage_bytes=moved, stage_hbm_bound_ms={k: v / HBM * 1e3 for k, v in moved.items()},
                    total_bytes=total, hbm_bound_ms=total / HBM * 1e3,
                    eval_mult_over_bound=behz["median"] / (total / HBM * 1e3),
                    sum_of_stage_medians_ms=sum(res[k]["median"] for k in stages),
                    hps_towers=2 * sq + 1, behz_towers=2 * sq + 1, behz_over_hps=behz["median"] / hps["median"])
    for h in hps_handles + [bz, pqb, pb, pq]:
        h.close()
    return kernels_out, mult_out


result = {"repeats": a.repeats, "calls_per_sample": dict(kernel=a.inner_kernel, eval_mult=a.inner_mult),
          "unit": "ms per call", "t": a.t, "fused_max_b": H.BEHZ_FUSED_MAX_B, "shapes": []}
for spec in a.shapes.split(","):
    log_n, sq, B = (int(v) for v in spec.split(":"))
    kern, mult = shape_ab(log_n, sq, B)
    result["shapes"].append(dict(log_n=log_n, Q=sq, B=sq, batch=B, kernels=kern, eval_mult=mult))
    print(f"N=2^{log_n} Q={sq} batch={B}", flush=True)
    for k, v in kern["contenders"].items():
        print(f"  {k:22s} median {v['median']:8.4f} ms  [min {v['min']:.4f}, max {v['max']:.4f}]  "
              f"bound {kern['hbm_bound_ms'][k]:.4f} ms", flush=True)
    for k, v in mult["contenders"].items():
        print(f"  {k:22s} median {v['median']:8.4f} ms  [min {v['min']:.4f}, max {v['max']:.4f}]", flush=True)
    print(f"  eval_mult_behz bytes bound {mult['hbm_bound_ms']:.4f} ms, behz / hps {mult['behz_over_hps']:.3f}, "
          f"fused / two launches {kern['fused_over_two_launches']:.3f}", flush=True)
result["fused_kept"] = not any(e["kernels"]["fused_slower_beyond_spread"] for e in result["shapes"])
os.makedirs(os.path.dirname(a.out), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(result, f, indent=1)
    f.write("\n")
ctx.close()
