"""Same-process timings of the BFV decryption calls.

  (a) ofhe_hip_bfv_decrypt_scale_round in one power-of-two split loop (t = 2^15:
      C), one non-power-of-two split loop (t = 65537: G or H with the tower
      count) and under BEHZ, each against the bytes it has to move,
      (size_q + 1) * 8 per coefficient, over 8 TB/s, and against the
      device-to-host copy of the Q towers of one polynomial through
      ofhe_hip_copy_to_host (pinned memory) -- what a host-side decryption has
      to pay before it computes anything.
  (b) ofhe_hip_bfv_decrypt on 3 coefficient-form elements (what
      ofhe_hip_bfv_eval_mult leaves) against its bytes, against the same steps
      through calls that existed before it plus the scale-round call (NTT x 3,
      modmul / modadd for c0 + c1 s + c2 s^2, INTT), and against the copy of the
      three elements to the host.

Outputs are checked for equality first.  (a): the two floating-point loops
against torch compositions with one float64 kernel per multiply and per add,
the BEHZ kernel against Python integers on the first 256 coefficients of every
batch entry.  (b): the one call against the staged calls, HPS and BEHZ; both
end in the scale-round kernel checked under (a).  Then, after a warm-up, the
contenders alternate (the order flips every round) for --repeats rounds; a
sample is a short run of back-to-back calls between two device events.  Writes
medians and spread to profiles/bfv_decrypt_ab.json (--out).
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
ap.add_argument("--inner-kernel", type=int, default=20, help="back-to-back calls per sample, scale-round kernels")
ap.add_argument("--inner-decrypt", type=int, default=5, help="back-to-back calls per sample, decrypt and its stages")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bfv_decrypt_ab.json"))
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


def pow2_composition(x, T):
    """the loops C / D with torch kernels: one float64 kernel per multiply and per add, tower order"""
    hf = T.q_msb_hf
    fs = torch.full((x.shape[0], x.shape[2]), 0.5, dtype=torch.float64, device="cuda")
    acc = torch.zeros((x.shape[0], x.shape[2]), dtype=torch.int64, device="cuda")
    for i in range(len(T.q)):
        hi = x[:, i, :] >> hf
        lo = x[:, i, :] - (hi << hf)
        fs = fs + lo.to(torch.float64) * T.tQHatInvModqDivqFrac[i]
        fs = fs + hi.to(torch.float64) * T.tQHatInvModqBDivqFrac[i]
        acc = acc + lo * T.tQHatInvModqDivqModt[i] + hi * T.tQHatInvModqBDivqModt[i]  # modulo 2^64
    return (acc + fs.to(torch.int64)) & (T.t - 1)


def non_pow2_composition(x, T):
    """the loops G / H with torch kernels (products below 2^47 before the reduction mod t of H)"""
    hf, t, reduced = T.q_msb_hf, T.t, bool(T.branch & 1)
    fs = torch.zeros((x.shape[0], x.shape[2]), dtype=torch.float64, device="cuda")
    acc = torch.zeros((x.shape[0], x.shape[2]), dtype=torch.int64, device="cuda")
    for i in range(len(T.q)):
        hi = x[:, i, :] >> hf
        lo = x[:, i, :] - (hi << hf)
        fs = fs + lo.to(torch.float64) * T.tQHatInvModqDivqFrac[i]
        fs = fs + hi.to(torch.float64) * T.tQHatInvModqBDivqFrac[i]
        pl, ph = lo * T.tQHatInvModqDivqModt[i], hi * T.tQHatInvModqBDivqModt[i]
        acc = acc + (pl % t + ph % t if reduced else pl + ph)
    fs = fs + acc.to(torch.float64)
    quot = (fs * (1.0 / float(t))).to(torch.int64)
    fs = fs - float(t) * quot.to(torch.float64)
    return (fs + 0.5).to(torch.int64)


def behz_integers(x, T, count=256):
    """dcrtpoly-impl.h:2005-2049 with Python integers on the first `count` coefficients of every batch entry"""
    xs = x[:, :, :count].cpu().tolist()
    out = []
    for entry in xs:
        row = []
        for k in range(len(entry[0])):
            s = 0
            for i, m in enumerate(T.q):
                y = entry[i][k] * T.tgammaQHatInvModq[i] % m
                s = (s + y * T.negInvqModtgamma[i] % T.tgamma) % T.tgamma
            row.append((s + (s & ((1 << BT.GAMMA_BITS) - 1))) >> BT.GAMMA_BITS)
        out.append(row)
    return torch.tensor(out, dtype=torch.int64, device="cuda")


def shape_ab(log_n, sq, B):
    n = 1 << log_n
    q, rq = bench.moduli_chain(log_n, sq)
    plan = H.NTTPlan(ctx, log_n, q, rq)
    T2, Tn = BT.DecryptTables(q, 1 << 15), BT.DecryptTables(q, 65537)
    assert T2.split and Tn.split and T2.branch < 4 <= Tn.branch
    d_pow2, d_np2 = H.BfvDecrypt(ctx, log_n, T2), H.BfvDecrypt(ctx, log_n, Tn)
    d_behz = H.BfvDecrypt(ctx, log_n, Tn, H.BFV_BEHZ)
    w = 8 * B * n  # bytes of one tower over the batch
    x = uniform((B, sq, n), q)
    cts = [uniform((B, sq, n), q) for _ in range(3)]
    sk = uniform((1, sq, n), q)
    sk_b = sk.expand(B, sq, n).contiguous()
    o2, on, ob, od, os_, odb, osb = (empty(B, n) for _ in range(7))
    E, tmp, acc = [empty(B, sq, n) for _ in range(3)], empty(B, sq, n), empty(B, sq, n)
    pinned = ctx.host_alloc(3 * w * sq)

    def k_pow2():
        d_pow2.scale_round(x.data_ptr(), o2.data_ptr(), B, st)

    def k_np2():
        d_np2.scale_round(x.data_ptr(), on.data_ptr(), B, st)

    def k_behz():
        d_behz.scale_round(x.data_ptr(), ob.data_ptr(), B, st)

    def d2h_one():
        ctx.copy_to_host(pinned, x.data_ptr(), w * sq, st)

    def d2h_three():
        for k in range(3):
            ctx.copy_to_host(pinned + k * w * sq, cts[k].data_ptr(), w * sq, st)

    def decrypt(dec=d_np2, out=od):
        dec.decrypt(plan, [c.data_ptr() for c in cts], sk.data_ptr(), out.data_ptr(), False, B, st)

    def staged(dec=d_np2, out=os_):
        for k in range(3):
            plan.forward_range(0, sq, cts[k].data_ptr(), E[k].data_ptr(), sq * n, sq * n, B, st)
        plan.mod_mul(E[1].data_ptr(), sk_b.data_ptr(), acc.data_ptr(), B, st)
        plan.mod_add(acc.data_ptr(), E[0].data_ptr(), acc.data_ptr(), B, st)
        plan.mod_mul(sk_b.data_ptr(), sk_b.data_ptr(), tmp.data_ptr(), B, st)
        plan.mod_mul(E[2].data_ptr(), tmp.data_ptr(), tmp.data_ptr(), B, st)
        plan.mod_add(acc.data_ptr(), tmp.data_ptr(), acc.data_ptr(), B, st)
        plan.inverse(acc.data_ptr(), B, st)
        dec.scale_round(acc.data_ptr(), out.data_ptr(), B, st)

    k_pow2(), k_np2(), k_behz(), decrypt(), staged(), decrypt(d_behz, odb), staged(d_behz, osb), d2h_one(), d2h_three()
    torch.cuda.synchronize()
    assert torch.equal(o2, pow2_composition(x, T2)), "scale-round (t = 2^15) differs from the torch composition"
    assert torch.equal(on, non_pow2_composition(x, Tn)), "scale-round (t = 65537) differs from the torch composition"
    assert torch.equal(ob[:, :256], behz_integers(x, Tn)), "scale-round (BEHZ) differs from the integer loop"
    assert torch.equal(od, os_) and torch.equal(odb, osb), "decrypt differs from its staged calls"
    kern = race({"scale_round_pow2": k_pow2, "scale_round_non_pow2": k_np2, "scale_round_behz": k_behz,
                 "copy_to_host_one_polynomial": d2h_one}, a.repeats, a.inner_kernel)
    whole = race({"decrypt": decrypt, "decrypt_staged": staged, "copy_to_host_three_elements": d2h_three}, a.repeats,
                 a.inner_decrypt)
    kb = w * (sq + 1)
    # every transform counted as one read and one write of its towers
    stage_bytes = {"ntt_x3": 6 * w * sq, "decrypt_core": 4 * w * sq + 8 * n * sq, "intt": 2 * w * sq, "scale_round": kb}
    db = sum(stage_bytes.values())
    med = lambda r, k: r[k]["median"]  # noqa: E731
    out = dict(branches=dict(pow2=BT.BRANCHES[d_pow2.branch], non_pow2=BT.BRANCHES[d_np2.branch]),
               kernels=kern, kernel_bytes=kb, kernel_hbm_bound_ms=kb / HBM * 1e3,
               kernel_tb_per_s={k: kb / (med(kern, k) * 1e-3) / 1e12 for k in kern if k.startswith("scale_round")},
               copy_bytes_one_polynomial=w * sq,
               copy_gb_per_s=w * sq / (med(kern, "copy_to_host_one_polynomial") * 1e-3) / 1e9,
               kernel_over_copy={k: med(kern, k) / med(kern, "copy_to_host_one_polynomial")
                                 for k in kern if k.startswith("scale_round")},
               decrypt=whole, decrypt_stage_bytes=stage_bytes, decrypt_bytes=db, decrypt_hbm_bound_ms=db / HBM * 1e3,
               decrypt_over_bound=med(whole, "decrypt") / (db / HBM * 1e3),
               decrypt_over_staged=med(whole, "decrypt") / med(whole, "decrypt_staged"),
               decrypt_over_copy=med(whole, "decrypt") / med(whole, "copy_to_host_three_elements"))
    ctx.host_free(pinned)
    for h in (d_behz, d_np2, d_pow2, plan):
        h.close()
    return out


result = {"repeats": a.repeats, "calls_per_sample": dict(kernel=a.inner_kernel, decrypt=a.inner_decrypt),
          "unit": "ms per call", "hbm_bytes_per_s": HBM, "shapes": []}
for spec in a.shapes.split(","):
    log_n, sq, B = (int(v) for v in spec.split(":"))
    entry = dict(log_n=log_n, Q=sq, batch=B, **shape_ab(log_n, sq, B))
    result["shapes"].append(entry)
    print(f"N=2^{log_n} Q={sq} batch={B}  loops {entry['branches']}", flush=True)
    for k, v in entry["kernels"].items():
        print(f"  {k:30s} median {v['median']:8.4f} ms  [min {v['min']:.4f}, max {v['max']:.4f}]", flush=True)
    print(f"  scale-round bytes bound {entry['kernel_hbm_bound_ms']:.4f} ms, TB/s {entry['kernel_tb_per_s']}", flush=True)
    for k, v in entry["decrypt"].items():
        print(f"  {k:30s} median {v['median']:8.4f} ms  [min {v['min']:.4f}, max {v['max']:.4f}]", flush=True)
    print(f"  decrypt bytes bound {entry['decrypt_hbm_bound_ms']:.4f} ms", flush=True)
os.makedirs(os.path.dirname(a.out), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(result, f, indent=1)
    f.write("\n")
ctx.close()
