"""Same-process timings of the BFV (HPS family) multiplication calls.

  (a) ofhe_hip_switch_crt_basis against ofhe_hip_approx_switch_crt_basis at the
      same shape (Q -> R): the exact call adds size_q double multiply-adds and
      one select-and-subtract per output, and no algorithmic bytes.
  (b) ofhe_hip_switch_crt_basis against a composition of calls that existed
      before it: modmul_scalar for y_i = [x_i QHat_i^-1]_{q_i}, torch float64
      ops for nu / alpha (separate multiply and add kernels, tower order), the
      approximate switch on y with unit QHat^-1, and a gathered
      alphaQModp[alpha][j] subtracted with modsub_vv.
  (c) ofhe_hip_bfv_eval_mult per technique, with its stages timed through the
      public calls they are made of and the bytes each stage has to move over
      8 TB/s as its bound.

Outputs are checked for equality first ((b): the composition equals the fused
call; (c): the staged calls equal the one call).  Then, after a warm-up, the
contenders alternate (the order flips every round) for --repeats rounds; a
sample is a short run of back-to-back calls between two device events.  Writes
medians and spread to profiles/bfv_mult_ab.json (--out).
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
ap.add_argument("--shapes", default="14:8:9:8,16:16:17:4", help="log_n:Q:R:batch, comma separated")
ap.add_argument("--repeats", type=int, default=11)
ap.add_argument("--inner-switch", type=int, default=20, help="back-to-back calls per sample, switch contenders")
ap.add_argument("--inner-mult", type=int, default=5, help="back-to-back calls per sample, eval_mult and its stages")
ap.add_argument("--t", type=int, default=65537)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bfv_mult_ab.json"))
a = ap.parse_args()
HBM = 8e12  # bytes / s
g = torch.Generator(device="cuda")
g.manual_seed(23)
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
    round.  One sample is `inner` back-to-back calls between two device events, divided by inner: a
    single 10-30 us call would be measured together with the events' resolution and the launch gap."""
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


def switch_ab(log_n, sq, sr, B):
    n = 1 << log_n
    m, roots = bench.moduli_chain(log_n, sq + sr)
    q, r = m[:sq], m[sq:]
    hinv, hmod = BT.hat_inv(q), BT.BfvTables.flat(BT.hat_mod(q, r))
    exact = H.BaseConverter(ctx, log_n, q, r, hinv, hmod)
    unit = H.BaseConverter(ctx, log_n, q, r, [1] * sq, hmod)
    plan_q, plan_r = H.NTTPlan(ctx, log_n, q, roots[:sq]), H.NTTPlan(ctx, log_n, r, roots[sq:])
    qinv = BT.inv_doubles(q)
    aq = torch.tensor(BT.alpha_mod(q, r), dtype=torch.int64, device="cuda")  # [sq + 1][sr]
    x = uniform((B, sq, n), q)
    y, o_fused, o_comp, o_approx = empty(B, sq, n), empty(B, sr, n), empty(B, sr, n), empty(B, sr, n)

    def fused():
        exact.switch_exact(x.data_ptr(), o_fused.data_ptr(), B, st)

    def approx():
        exact.switch(x.data_ptr(), o_approx.data_ptr(), B, st)

    def composition():
        plan_q.mod_mul_scalar(x.data_ptr(), hinv, y.data_ptr(), B, st)
        nu = torch.full((B, n), 0.5, dtype=torch.float64, device="cuda")
        for i in range(sq):
            nu = nu + y[:, i, :].to(torch.float64) * qinv[i]
        sub = aq[nu.to(torch.int64)].permute(0, 2, 1).contiguous()  # [B][sr][n]
        unit.switch(y.data_ptr(), o_comp.data_ptr(), B, st)
        plan_r.mod_sub(o_comp.data_ptr(), sub.data_ptr(), o_comp.data_ptr(), B, st)

    fused(), approx(), composition()
    torch.cuda.synchronize()
    assert torch.equal(o_fused, o_comp), "exact switch: the fused call differs from the composition"
    res = race({"exact_fused": fused, "approx": approx, "exact_composition": composition}, a.repeats, a.inner_switch)
    byts = 8 * B * n * (sq + sr)
    out = dict(contenders=res, bytes=byts, hbm_bound_ms=byts / HBM * 1e3,
               exact_over_approx=res["exact_fused"]["median"] / res["approx"]["median"],
               fused_over_composition=res["exact_fused"]["median"] / res["exact_composition"]["median"],
               fused_faster_than_composition_beyond_spread=res["exact_fused"]["max"] < res["exact_composition"]["min"])
    for h in (exact, unit, plan_q, plan_r):
        h.close()
    return out


def mult_ab(tech, log_n, sq, sr, B):
    n = 1 << log_n
    m, roots = bench.moduli_chain(log_n, sq + sr)
    q, r, rq, rr = m[:sq], m[sq:], roots[:sq], roots[sq:]
    T = BT.BfvTables(q, r, a.t, tech)
    pq, pr, pqr = H.NTTPlan(ctx, log_n, q, rq), H.NTTPlan(ctx, log_n, r, rr), H.NTTPlan(ctx, log_n, m, roots)
    q_to_r = H.BaseConverter(ctx, log_n, q, r, T.q_hat_inv_modq, T.flat(T.q_hat_modr))
    r_to_q = H.BaseConverter(ctx, log_n, r, q, T.r_hat_inv_modr, T.flat(T.r_hat_modq))
    neg = None
    if tech == BT.HPSPOVERQ:
        neg = H.BaseConverter(ctx, log_n, q, r, T.neg_r_q_hat_inv_modq, T.flat(T.q_inv_modr))
    sr_h = H.ScaleRound(ctx, log_n, q, r, T.out_is_q, T.sr_table, T.sr_frac)
    mult = H.BfvMult(ctx, H.BFV_HPS if tech == BT.HPS else H.BFV_HPSPOVERQ, pq, pr, pqr, q_to_r, r_to_q, neg, sr_h)
    cts = [uniform((B, sq, n), q) for _ in range(4)]
    outs, outs2 = [empty(B, sq, n) for _ in range(3)], [empty(B, sq, n) for _ in range(3)]
    E, Tp = [empty(B, sq + sr, n) for _ in range(4)], empty(3, B, sq + sr, n)
    S, tmp_q, tmp_r = empty(3, B, sr, n), empty(B, sq, n), empty(B, sr, n)

    def one_call():
        mult.eval_mult(*[t.data_ptr() for t in cts + outs], B, st)

    def expand():
        for k in range(4):
            if tech == BT.HPS or k < 2:
                H.expand_crt_basis(pq, pr, q_to_r, True, cts[k].data_ptr(), E[k].data_ptr(), B, st)
                continue
            # FastExpandCRTBasisPloverQ through the public calls (dense buffers, then assembled)
            pq.inverse_range(0, sq, cts[k].data_ptr(), tmp_q.data_ptr(), sq * n, sq * n, B, st)
            neg.switch(tmp_q.data_ptr(), tmp_r.data_ptr(), B, st)
            r_to_q.switch_exact(tmp_r.data_ptr(), tmp_q.data_ptr(), B, st)
            E[k][:, :sq].copy_(tmp_q)
            E[k][:, sq:].copy_(tmp_r)
            pqr.forward(E[k].data_ptr(), B, st)

    def tensor():
        pqr.eval_mult_core(*[e.data_ptr() for e in E], Tp[0].data_ptr(), Tp[1].data_ptr(), Tp[2].data_ptr(), B, st)

    def intt():
        pqr.inverse(Tp.data_ptr(), 3 * B, st)

    def scale():
        if tech == BT.HPS:
            sr_h.run(Tp.data_ptr(), S.data_ptr(), 3 * B, st)
        else:
            for k in range(3):
                sr_h.run(Tp[k].data_ptr(), outs2[k].data_ptr(), B, st)

    def switch_back():
        for k in range(3):
            r_to_q.switch_exact(S[k].data_ptr(), outs2[k].data_ptr(), B, st)

    stages = {"expand": expand, "tensor": tensor, "intt": intt, "scale_and_round": scale}
    if tech == BT.HPS:
        stages["switch_r_to_q"] = switch_back
    one_call()
    for fn in stages.values():
        fn()
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(outs, outs2)), "eval_mult differs from its staged calls"
    # the stages run in place on each other's buffers in whatever order the rounds take them: the
    # words stay canonical residues, and none of the timings depends on their values
    res = race({"eval_mult": one_call, **stages}, a.repeats, a.inner_mult)
    w = 8 * B * n  # bytes of one tower over the batch
    moved = {"expand": 4 * w * (2 * sq + sr), "tensor": 7 * w * (sq + sr), "intt": 6 * w * (sq + sr),
             "scale_and_round": 3 * w * ((sq + sr) + (sq if T.out_is_q else sr))}
    if tech == BT.HPS:
        moved["switch_r_to_q"] = 3 * w * (sr + sq)
    total = sum(moved.values())
    out = dict(contenders=res, stage_bytes=moved, stage_hbm_bound_ms={k: v / HBM * 1e3 for k, v in moved.items()},
               total_bytes=total, hbm_bound_ms=total / HBM * 1e3,
               eval_mult_over_bound=res["eval_mult"]["median"] / (total / HBM * 1e3),
               sum_of_stage_medians_ms=sum(res[k]["median"] for k in stages))
    mult.close()
    for h in (sr_h, neg, r_to_q, q_to_r, pqr, pr, pq):
        if h is not None:
            h.close()
    return out


result = {"repeats": a.repeats, "calls_per_sample": dict(switch=a.inner_switch, eval_mult=a.inner_mult),
          "unit": "ms per call", "t": a.t, "shapes": []}
for spec in a.shapes.split(","):
    log_n, sq, sr, B = (int(v) for v in spec.split(":"))
    entry = dict(log_n=log_n, Q=sq, R=sr, batch=B)
    entry["switch"] = switch_ab(log_n, sq, sr, B)
    entry["eval_mult_hps"] = mult_ab(BT.HPS, log_n, sq, sr, B)
    entry["eval_mult_hpspoverq"] = dict(R=sq, **mult_ab(BT.HPSPOVERQ, log_n, sq, sq, B))
    result["shapes"].append(entry)
    sw = entry["switch"]["contenders"]
    print(f"N=2^{log_n} Q={sq} R={sr} batch={B}", flush=True)
    for k, v in sw.items():
        print(f"  switch {k:18s} median {v['median']:8.4f} ms  [min {v['min']:.4f}, max {v['max']:.4f}]", flush=True)
    for name in ("eval_mult_hps", "eval_mult_hpspoverq"):
        for k, v in entry[name]["contenders"].items():
            print(f"  {name} {k:16s} median {v['median']:8.4f} ms  [min {v['min']:.4f}, max {v['max']:.4f}]",
                  flush=True)
        print(f"  {name} bytes bound {entry[name]['hbm_bound_ms']:.4f} ms", flush=True)
os.makedirs(os.path.dirname(a.out), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(result, f, indent=1)
    f.write("\n")
ctx.close()
