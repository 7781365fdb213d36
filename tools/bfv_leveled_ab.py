"""Same-process timings of the HPSPOVERQLEVELED calls (BFV multiplication with dropped levels).

  (a) ofhe_hip_scale_round_expand_ql_hat (one launch) against ofhe_hip_scale_and_round followed by
      ofhe_hip_expand_ql_hat (two launches, l + 1 intermediate towers written and read back).
  (b) ofhe_hip_expand_ql_hat with an addend against the same result from the element-wise calls:
      modmul_scalar over Q_l, ofhe_hip_zero of a polynomial over Q, a strided copy, modadd_vv.
      Its bytes over its time are reported next to the element-wise ops' bandwidth.
  (c) ofhe_hip_bfv_eval_mult_leveled at level l against ofhe_hip_bfv_eval_mult (HPSPOVERQ) on the
      full chain, with the levelled call's stages timed through the public calls they are made of.
  (d) ofhe_hip_bfv_relinearize_leveled against the same steps through the earlier public calls.

Outputs are checked for equality first.  Then, after a warm-up, the contenders alternate (the order
flips every round) for --repeats rounds; a sample is a short run of back-to-back calls between two
device events.  Writes medians and spread to profiles/bfv_leveled_ab.json (--out).
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
ap.add_argument("--shapes", default="14:8:8:3:4:2,16:16:4:7:4:4", help="log_n:Q:batch:l:P:dnum, comma separated")
ap.add_argument("--repeats", type=int, default=11)
ap.add_argument("--inner-small", type=int, default=20, help="back-to-back calls per sample, (a) and (b)")
ap.add_argument("--inner-mult", type=int, default=5, help="back-to-back calls per sample, (c) and (d)")
ap.add_argument("--t", type=int, default=65537)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bfv_leveled_ab.json"))
a = ap.parse_args()
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


def below(x, y):
    """is x's whole range below y's?"""
    return x["max"] < y["min"]


def shape_ab(log_n, sq, B, l, sp, dnum):
    n, L = 1 << log_n, l + 1
    m, roots = bench.moduli_chain(log_n, 2 * sq + sp)
    q, rq, r, rr = m[:sq], roots[:sq], m[sq:2 * sq], roots[sq:2 * sq]
    p, rp = m[2 * sq:], roots[2 * sq:]
    T, F = BT.LeveledTables(q, r, a.t, l), BT.BfvTables(q, r, a.t, BT.HPSPOVERQ)
    flat = BT.BfvTables.flat
    plan = lambda mo, ro: H.NTTPlan(ctx, log_n, mo, ro)  # noqa: E731
    pq, pql, prl, pqlrl = plan(q, rq), plan(q[:L], rq[:L]), plan(r[:L], rr[:L]), plan(q[:L] + r[:L], rq[:L] + rr[:L])
    pr, pqr = plan(r, rr), plan(q + r, rq + rr)
    ql_to_rl = H.BaseConverter(ctx, log_n, T.ql, T.rl, T.q_hat_inv_modq, flat(T.q_hat_modr))
    rl_to_ql = H.BaseConverter(ctx, log_n, T.rl, T.ql, T.r_hat_inv_modr, flat(T.r_hat_modq))
    neg_l = H.BaseConverter(ctx, log_n, q, T.rl, T.neg_rl_q_hat_inv_modq, flat(T.q_inv_modr))
    drop = H.ScaleRound(ctx, log_n, T.ql, q[L:], True, T.drop_table, T.drop_frac)
    sr_l = H.ScaleRound(ctx, log_n, T.ql, T.rl, True, T.sr_table, T.sr_frac)
    level = H.BfvLevel(ctx, l, pq, pql, prl, pqlrl, ql_to_rl, rl_to_ql, neg_l, drop, sr_l, T.ql_hat_modq)
    q_to_r = H.BaseConverter(ctx, log_n, q, r, F.q_hat_inv_modq, flat(F.q_hat_modr))
    r_to_q = H.BaseConverter(ctx, log_n, r, q, F.r_hat_inv_modr, flat(F.r_hat_modq))
    neg_f = H.BaseConverter(ctx, log_n, q, r, F.neg_r_q_hat_inv_modq, flat(F.q_inv_modr))
    sr_f = H.ScaleRound(ctx, log_n, q, r, True, F.sr_table, F.sr_frac)
    full = H.BfvMult(ctx, H.BFV_HPSPOVERQ, pq, pr, pqr, q_to_r, r_to_q, neg_f, sr_f)
    ks = H.KeySwitch(ctx, log_n, q, rq, p, rp, dnum)
    w = 8 * B * n  # bytes of one tower over the batch
    out = {}

    # ---- (a) the fused scale-round-lift against the two launches
    x = uniform((B, 2 * L, n), T.ql + T.rl)
    o1, o2, mid = empty(B, sq, n), empty(B, sq, n), empty(B, L, n)

    def fused():
        level.scale_round_expand(x.data_ptr(), o1.data_ptr(), B, st)

    def two():
        sr_l.run(x.data_ptr(), mid.data_ptr(), B, st)
        level.expand_ql_hat(mid.data_ptr(), o2.data_ptr(), 0, B, st)

    fused(), two()
    torch.cuda.synchronize()
    assert torch.equal(o1, o2), "(a) the fused launch differs from the two launches"
    res = race({"fused": fused, "two_launches": two}, a.repeats, a.inner_small)
    out["scale_round_lift"] = dict(contenders=res, fused_bytes=w * (2 * L + sq), two_launch_bytes=w * (4 * L + sq),
                                   fused_wholly_below=below(res["fused"], res["two_launches"]))

    # ---- (b) expand_ql_hat with an addend against the element-wise calls
    xl, add = uniform((B, L, n), T.ql), uniform((B, sq, n), q)
    e1, e2, tmp = empty(B, sq, n), empty(B, sq, n), empty(B, L, n)

    def one():
        level.expand_ql_hat(xl.data_ptr(), e1.data_ptr(), add.data_ptr(), B, st)

    def eltwise():
        pql.mod_mul_scalar(xl.data_ptr(), T.ql_hat_modq, tmp.data_ptr(), B, st)
        ctx.zero(e2.data_ptr(), 8 * B * sq * n, st)
        e2[:, :L].copy_(tmp)
        pq.mod_add(e2.data_ptr(), add.data_ptr(), e2.data_ptr(), B, st)

    one(), eltwise()
    torch.cuda.synchronize()
    assert torch.equal(e1, e2), "(b) expand_ql_hat differs from the element-wise calls"
    res = race({"expand_ql_hat": one, "eltwise_calls": eltwise}, a.repeats, a.inner_small)
    byts = w * (L + 2 * sq)
    out["expand_ql_hat_addend"] = dict(contenders=res, bytes=byts,
                                       tb_per_s=byts / (res["expand_ql_hat"]["median"] * 1e-3) / 1e12,
                                       tb_per_s_range=[byts / (res["expand_ql_hat"]["max"] * 1e-3) / 1e12,
                                                       byts / (res["expand_ql_hat"]["min"] * 1e-3) / 1e12],
                                       wholly_below=below(res["expand_ql_hat"], res["eltwise_calls"]))

    # ---- (c) eval_mult_leveled against the full-chain HPSPOVERQ call, and its stages
    cts = [uniform((B, sq, n), q) for _ in range(4)]
    outs, outs_f, outs_s = ([empty(B, sq, n) for _ in range(3)] for _ in range(3))
    E, Tp = empty(4, B, 2 * L, n), empty(3, B, 2 * L, n)
    coef, xq, tq, tr = empty(B, sq, n), empty(B, L, n), empty(B, L, n), empty(B, L, n)

    def leveled():
        level.eval_mult(*[t.data_ptr() for t in cts + outs], B, st)

    def full_chain():
        full.eval_mult(*[t.data_ptr() for t in cts + outs_f], B, st)

    def expand_c():
        for k in range(2):
            pq.inverse_range(0, sq, cts[k].data_ptr(), coef.data_ptr(), sq * n, sq * n, B, st)
            drop.run(coef.data_ptr(), xq.data_ptr(), B, st)
            H.expand_crt_basis(pql, prl, ql_to_rl, False, xq.data_ptr(), E[k].data_ptr(), B, st)

    def expand_d():
        for k in range(2, 4):
            pq.inverse_range(0, sq, cts[k].data_ptr(), coef.data_ptr(), sq * n, sq * n, B, st)
            neg_l.switch(coef.data_ptr(), tr.data_ptr(), B, st)
            rl_to_ql.switch_exact(tr.data_ptr(), tq.data_ptr(), B, st)
            E[k][:, :L].copy_(tq)
            E[k][:, L:].copy_(tr)
            pqlrl.forward(E[k].data_ptr(), B, st)

    def tensor():
        pqlrl.eval_mult_core(*[E[k].data_ptr() for k in range(4)], *[Tp[k].data_ptr() for k in range(3)], B, st)

    def intt():
        pqlrl.inverse(Tp.data_ptr(), 3 * B, st)

    def scale_lift():
        for k in range(3):
            level.scale_round_expand(Tp[k].data_ptr(), outs_s[k].data_ptr(), B, st)

    stages = {"expand_c": expand_c, "expand_d": expand_d, "tensor": tensor, "intt": intt, "scale_round_lift": scale_lift}
    leveled(), full_chain()
    for fn in stages.values():
        fn()
    torch.cuda.synchronize()
    assert all(torch.equal(u, v) for u, v in zip(outs, outs_s)), "(c) eval_mult_leveled differs from its staged calls"
    res = race({"eval_mult_leveled": leveled, "eval_mult_hpspoverq_full": full_chain, **stages}, a.repeats, a.inner_mult)
    out["eval_mult"] = dict(contenders=res,
                            leveled_over_full=res["eval_mult_leveled"]["median"] / res["eval_mult_hpspoverq_full"]["median"],
                            leveled_wholly_below=below(res["eval_mult_leveled"], res["eval_mult_hpspoverq_full"]),
                            sum_of_stage_medians_ms=sum(res[k]["median"] for k in stages))

    # ---- (d) relinearize_leveled against the steps through the earlier public calls
    el = [uniform((B, sq, n), q) for _ in range(3)]
    kb, ka = uniform((dnum, sq + sp, n), q + p), uniform((dnum, sq + sp, n), q + p)
    r0, r1, s0, s1 = empty(B, sq, n), empty(B, sq, n), empty(B, sq, n), empty(B, sq, n)
    a0, a1 = empty(B, L, n), empty(B, L, n)

    def relin():
        level.relinearize(ks, [t.data_ptr() for t in el], True, kb.data_ptr(), ka.data_ptr(), r0.data_ptr(),
                          r1.data_ptr(), B, st)

    def relin_steps():
        pq.inverse_range(0, sq, el[2].data_ptr(), coef.data_ptr(), sq * n, sq * n, B, st)
        drop.run(coef.data_ptr(), xq.data_ptr(), B, st)
        pql.forward(xq.data_ptr(), B, st)
        ks.core(L, xq.data_ptr(), kb.data_ptr(), ka.data_ptr(), a0.data_ptr(), a1.data_ptr(), 0, B, st)
        for src, c, dst in ((a0, el[0], s0), (a1, el[1], s1)):
            pql.mod_mul_scalar(src.data_ptr(), T.ql_hat_modq, tmp.data_ptr(), B, st)
            ctx.zero(dst.data_ptr(), 8 * B * sq * n, st)
            dst[:, :L].copy_(tmp)
            pq.mod_add(dst.data_ptr(), c.data_ptr(), dst.data_ptr(), B, st)

    relin(), relin_steps()
    torch.cuda.synchronize()
    assert torch.equal(r0, s0) and torch.equal(r1, s1), "(d) relinearize_leveled differs from its steps"
    res = race({"relinearize_leveled": relin, "public_call_steps": relin_steps}, a.repeats, a.inner_mult)
    out["relinearize"] = dict(contenders=res, wholly_below=below(res["relinearize_leveled"], res["public_call_steps"]))

    torch.cuda.synchronize()
    for h in (ks, full, level, sr_f, neg_f, r_to_q, q_to_r, sr_l, drop, neg_l, rl_to_ql, ql_to_rl, pqr, pr, pqlrl, prl,
              pql, pq):
        h.close()
    return out


result = {"repeats": a.repeats, "calls_per_sample": dict(small=a.inner_small, mult=a.inner_mult),
          "unit": "ms per call", "t": a.t, "shapes": []}
for spec in a.shapes.split(","):
    log_n, sq, B, l, sp, dnum = (int(v) for v in spec.split(":"))
    entry = dict(log_n=log_n, Q=sq, batch=B, l=l, P=sp, dnum=dnum, **shape_ab(log_n, sq, B, l, sp, dnum))
    result["shapes"].append(entry)
    print(f"N=2^{log_n} Q={sq} batch={B} l={l}", flush=True)
    for part in ("scale_round_lift", "expand_ql_hat_addend", "eval_mult", "relinearize"):
        for k, v in entry[part]["contenders"].items():
            print(f"  {part:22s} {k:26s} median {v['median']:8.4f} ms  [min {v['min']:.4f}, max {v['max']:.4f}]",
                  flush=True)
    print(f"  expand_ql_hat with addend: {entry['expand_ql_hat_addend']['tb_per_s']:.2f} TB/s", flush=True)
os.makedirs(os.path.dirname(a.out), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(result, f, indent=1)
    f.write("\n")
ctx.close()
