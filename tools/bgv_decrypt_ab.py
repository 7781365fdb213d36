"""Same-process timings of the BGV decryption calls.

  (a) ofhe_hip_bgv_mod_reduce_chain (the fused ModReduce chain Q_l -> q_0, with the Mod t ending) against
      the calls that existed before it -- size_ql - 1 calls of ofhe_hip_mod_reduce in coefficient form, each
      reading and writing every surviving tower -- against the bytes the kernel has to move over 8 TB/s and
      its arithmetic (size_ql (size_ql - 1) / 2 ModReduce steps per coefficient), and against the
      device-to-host copy of the towers of one polynomial through ofhe_hip_copy_to_host (pinned memory): what
      a host-side decryption pays before it computes anything.
  (b) ofhe_hip_bgv_decrypt on 2 elements (what ofhe_hip_ks_eval_mult leaves) in both of the reference's
      branches against the composition of earlier calls for the evaluation-form branch (modmul, modadd,
      ofhe_hip_ntt_inv, size_ql - 1 x ofhe_hip_mod_reduce, the copy of the tower left) and against the copy of
      the two elements to the host.

Outputs are checked for equality first: the chain without its ending against the tower the mod_reduce calls
leave, the chain with it and the evaluation-form decrypt against NativeVectorT::Mod(t) of that tower written
with torch.  Then, after a warm-up, the contenders alternate (the order flips every round) for --repeats
rounds; a sample is a short run of back-to-back calls between two device events.  Writes medians and spread to
profiles/bgv_decrypt_ab.json (--out).
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
ap.add_argument("--shapes", default="14:8:8,16:16:4", help="log_n:Q:batch, comma separated")
ap.add_argument("--t", type=int, default=65537)
ap.add_argument("--repeats", type=int, default=11)
ap.add_argument("--inner-kernel", type=int, default=10, help="back-to-back calls per sample, the chain")
ap.add_argument("--inner-decrypt", type=int, default=5, help="back-to-back calls per sample, decrypt and its stages")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bgv_decrypt_ab.json"))
a = ap.parse_args()
HBM = 8e12  # bytes / s
K = H.BGV_CHAIN_K
g = torch.Generator(device="cuda")
g.manual_seed(31)
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


def mod_t(x, q0, t):
    """NativeVectorT::Mod(t), mubintvecnat.cpp:139-166, for 2 < t <= q0 < 2^60"""
    v = torch.where(x > (q0 >> 1), x + (t - q0 % t), x)
    return torch.where(v >= t, v % t, v)


def chain_words(L):
    """towers read and written by the passes of the chain kernel on L towers"""
    words, live = 0, L
    while True:
        k = min(live - 1, K)
        words += live + (live - k)
        live -= k
        if live == 1:
            return words


def shape_ab(log_n, sq, B, t):
    n = 1 << log_n
    q, rq = bench.moduli_chain(log_n, sq)
    assert 2 < t <= q[0]
    plan = H.NTTPlan(ctx, log_n, q, rq)
    dec = H.BgvDecrypt(ctx, log_n, q, t)
    nti = [0] + [m - pow(t % m, -1, m) for m in q[1:]]
    qli = [[pow(q[j], -1, q[i]) for i in range(j)] for j in range(sq)]
    w = 8 * B * n  # bytes of one tower over the batch
    x = uniform((B, sq, n), q)
    cts = [uniform((B, sq, n), q) for _ in range(2)]
    cts_coef = [c.clone() for c in cts]
    for c in cts_coef:
        plan.inverse(c.data_ptr(), B, st)
    sk = uniform((1, sq, n), q)
    sk_b = sk.expand(B, sq, n).contiguous()
    o_raw, o_plain, o_steps, o_eval, o_coef, o_staged = (empty(B, n) for _ in range(6))
    y, acc = empty(B, sq, n), empty(B, sq, n)
    pinned = ctx.host_alloc(2 * w * sq)

    def chain(plain=True, out=o_plain):
        dec.mod_reduce_chain(sq, x.data_ptr(), out.data_ptr(), plain, B, st)

    def steps(src=x, work=y, out=o_steps):
        """size_ql - 1 ofhe_hip_mod_reduce calls: the first out of src, the rest in place, the last packed"""
        cur = src
        for j in range(sq - 1, 0, -1):
            dst, ds = (out, n) if j == 1 else (work, sq * n)
            plan.mod_reduce(j + 1, cur.data_ptr(), sq * n, dst.data_ptr(), ds, False, t, nti[j], qli[j], B, st)
            cur = work

    def d2h_one():
        ctx.copy_to_host(pinned, x.data_ptr(), w * sq, st)

    def d2h_two():
        for k in range(2):
            ctx.copy_to_host(pinned + k * w * sq, cts[k].data_ptr(), w * sq, st)

    def decrypt_eval():
        dec.decrypt(plan, sq, [c.data_ptr() for c in cts], sk.data_ptr(), o_eval.data_ptr(), True, B, st)

    def decrypt_coef():
        dec.decrypt(plan, sq, [c.data_ptr() for c in cts_coef], sk.data_ptr(), o_coef.data_ptr(), False, B, st)

    def staged():
        plan.mod_mul(cts[1].data_ptr(), sk_b.data_ptr(), acc.data_ptr(), B, st)
        plan.mod_add(acc.data_ptr(), cts[0].data_ptr(), acc.data_ptr(), B, st)
        plan.inverse(acc.data_ptr(), B, st)
        steps(acc, acc, o_staged)
        ctx.copy_to_host(pinned, o_staged.data_ptr(), w, st)  # the host's Mod t follows

    chain(False, o_raw), chain(), steps(), decrypt_eval(), decrypt_coef(), staged(), d2h_one(), d2h_two()
    torch.cuda.synchronize()
    assert torch.equal(o_raw, o_steps), "the chain differs from the mod_reduce calls"
    assert torch.equal(o_plain, mod_t(o_steps, q[0], t)), "the chain's ending differs from Mod t"
    assert torch.equal(o_eval, mod_t(o_staged, q[0], t)), "decrypt differs from its staged calls"
    kern = race({"chain": chain, "mod_reduce_calls": steps, "copy_to_host_one_polynomial": d2h_one}, a.repeats,
                a.inner_kernel)
    whole = race({"decrypt_eval_form": decrypt_eval, "decrypt_coeff_form": decrypt_coef, "decrypt_staged": staged,
                  "copy_to_host_two_elements": d2h_two}, a.repeats, a.inner_decrypt)
    med = lambda r, k: r[k]["median"]  # noqa: E731
    kb = w * chain_words(sq)
    nsteps = sq * (sq - 1) // 2
    # the calls' traffic: call j reads j + 1 towers and writes j
    sb = w * sum(2 * j + 1 for j in range(1, sq))
    tc = med(kern, "chain") * 1e-3
    out = dict(chain_k=K, kernels=kern, kernel_launches=-(-(sq - 1) // K), kernel_bytes=kb,
               kernel_hbm_bound_ms=kb / HBM * 1e3, kernel_tb_per_s=kb / tc / 1e12,
               kernel_over_hbm_bound=tc / (kb / HBM),
               steps_per_coefficient=nsteps,
               gsteps_per_s=nsteps * B * n / tc / 1e9,
               bound="arithmetic" if tc > 2 * kb / HBM else "bytes",
               mod_reduce_calls_bytes=sb, mod_reduce_calls_hbm_bound_ms=sb / HBM * 1e3,
               chain_over_mod_reduce_calls=med(kern, "chain") / med(kern, "mod_reduce_calls"),
               copy_bytes_one_polynomial=w * sq,
               copy_gb_per_s=w * sq / (med(kern, "copy_to_host_one_polynomial") * 1e-3) / 1e9,
               chain_over_copy=med(kern, "chain") / med(kern, "copy_to_host_one_polynomial"),
               decrypt=whole,
               decrypt_eval_over_staged=med(whole, "decrypt_eval_form") / med(whole, "decrypt_staged"),
               decrypt_eval_over_copy=med(whole, "decrypt_eval_form") / med(whole, "copy_to_host_two_elements"),
               decrypt_coeff_over_copy=med(whole, "decrypt_coeff_form") / med(whole, "copy_to_host_two_elements"))
    ctx.host_free(pinned)
    for h in (dec, plan):
        h.close()
    return out


result = {"repeats": a.repeats, "calls_per_sample": dict(kernel=a.inner_kernel, decrypt=a.inner_decrypt),
          "unit": "ms per call", "hbm_bytes_per_s": HBM, "t": a.t, "shapes": []}
for spec in a.shapes.split(","):
    log_n, sq, B = (int(v) for v in spec.split(":"))
    entry = dict(log_n=log_n, Q=sq, batch=B, **shape_ab(log_n, sq, B, a.t))
    result["shapes"].append(entry)
    print(f"N=2^{log_n} Q={sq} batch={B}", flush=True)
    for k, v in list(entry["kernels"].items()) + list(entry["decrypt"].items()):
        print(f"  {k:30s} median {v['median']:8.4f} ms  [min {v['min']:.4f}, max {v['max']:.4f}]", flush=True)
    print(f"  chain bytes bound {entry['kernel_hbm_bound_ms']:.4f} ms ({entry['kernel_tb_per_s']:.2f} TB/s), "
          f"{entry['gsteps_per_s']:.1f} G steps/s, bound by {entry['bound']}; chain / calls "
          f"{entry['chain_over_mod_reduce_calls']:.3f}, eval decrypt / staged {entry['decrypt_eval_over_staged']:.3f}",
          flush=True)
os.makedirs(os.path.dirname(a.out), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(result, f, indent=1)
    f.write("\n")
ctx.close()
