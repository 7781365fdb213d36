"""Same-process A/B of BV key switching with a digit size on

  n14  N = 2^14,  8 towers, batch 8
  n16  N = 2^16, 16 towers, batch 4

for digit_size 0, 30, 20, 10:

  (a) separate   bv_precompute_digits + bv_core_digits + 2 x modadd_vv (the whole digit array in memory)
  (b) one_call   ofhe_hip_bv_key_switch with both addends, chunk_digits = 0 (the library's scratch bound)

At digit_size = 0 also the calls shipped before the digit size, bv_precompute +
bv_core (+ the two additions): the regression point of the new one-call path.
The HYBRID key switch on the same Q (dnum = 3, P of ceil(towers / 3) towers)
is timed next to them so that BV can be placed against it.

The inner product alone (bv_core_digits at digit_size = 20): the plain loop
(ofhe_hip_bv_tune(1)) against the key-stationary variants (2 and 4 batch
entries per thread) at batch 1, 4 and 8, with the bytes the sum needs -- every
digit word once, every key word once, the outputs -- over the time.

Outputs are checked for equality first.  Then, after a warm-up, the contenders
alternate (the order flips every round) for --repeats rounds, each call timed
with device events.  Every timed call follows an untimed call of the same
contender: the contenders take scratch blocks of different sizes from the
context's stream-ordered pool, and a call that follows another contender's
pays for the pool re-mapping its blocks (up to 0.8 ms here), which is a cost of
the alternation, not of either contender.  Writes medians and spread to
profiles/bv_digits_ab.json.
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

SHAPES = {"n14": (14, 8, 8), "n16": (16, 16, 4)}
DIGIT_SIZES = (0, 30, 20, 10)
INNER_R, INNER_BATCHES, INNER_NB = 20, (1, 4, 8), (1, 2, 4, 0)  # 0: the library's choice
ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default=",".join(SHAPES))
ap.add_argument("--repeats", type=int, default=11)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bv_digits_ab.json"))
a = ap.parse_args()
assert a.repeats >= 11, "at least 11 rounds"
assert torch.cuda.is_available(), "this tool measures on the GPU"
ctx = H.Context(0)
g = torch.Generator(device="cuda")
g.manual_seed(21)
s = torch.cuda.current_stream()
st = s.cuda_stream


def uniform(shape, moduli):
    x = torch.empty(shape, dtype=torch.int64, device="cuda")
    for t, m in enumerate(moduli):
        x[..., t, :].random_(0, m, generator=g)
    return x


def empty(*shape):
    return torch.empty(shape, dtype=torch.int64, device="cuda")


def alternate(contenders, repeats):
    """name -> dict(median, min, max) in ms per call."""
    times = {k: [] for k in contenders}
    for rnd in range(repeats + 1):  # round 0 is a second warm-up
        order = list(contenders.items())
        for name, fn in (order if rnd % 2 == 0 else order[::-1]):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            fn()  # untimed: the scratch pool then holds this contender's blocks (see the module docstring)
            t0.record(s)
            fn()
            t1.record(s)
            t1.synchronize()
            if rnd:
                times[name].append(t0.elapsed_time(t1))
    out = {}
    for name, tt in times.items():
        out[name] = dict(median=statistics.median(tt), min=min(tt), max=max(tt))
        print(f"  {name:34s} median {out[name]['median']:9.3f} ms  [min {min(tt):.3f}, max {max(tt):.3f}]", flush=True)
    return out


def run_shape(log_n, T, B, repeats):
    n = 1 << log_n
    sp = -(-T // 3)
    allq, allr = bench.moduli_chain(log_n, T + sp)
    q, rq = allq[:T], allr[:T]
    plan = H.NTTPlan(ctx, log_n, q, rq)
    ks = H.KeySwitch(ctx, log_n, q, rq, allq[T:], allr[T:], 3)
    c, add0, add1 = (uniform((B, T, n), q) for _ in range(3))
    res = {"shape": dict(log_n=log_n, towers=T, batch=B), "repeats": repeats, "unit": "ms per call", "digit_sizes": {}}
    hkb, hka = uniform((3, T + sp, n), allq), uniform((3, T + sp, n), allq)
    h0, h1 = empty(B, T, n), empty(B, T, n)

    def hybrid():
        ks.core(T, c.data_ptr(), hkb.data_ptr(), hka.data_ptr(), h0.data_ptr(), h1.data_ptr(), 0, B, st)

    for r in DIGIT_SIZES:
        nd = plan.bv_digit_count(T, r)
        print(f" digit_size {r}: {nd} digits", flush=True)
        kb, ka = uniform((nd, T, n), q), uniform((nd, T, n), q)
        dd = empty(B, nd, T, n)
        s0, s1, k0, k1, p0, p1 = (empty(B, T, n) for _ in range(6))

        def separate():
            plan.bv_precompute_digits(T, r, c.data_ptr(), dd.data_ptr(), B, st)
            plan.bv_core_digits(T, nd, dd.data_ptr(), kb.data_ptr(), ka.data_ptr(), T, s0.data_ptr(), s1.data_ptr(), B,
                                st)
            plan.mod_add(add0.data_ptr(), s0.data_ptr(), s0.data_ptr(), B, st)
            plan.mod_add(add1.data_ptr(), s1.data_ptr(), s1.data_ptr(), B, st)

        def one_call():
            plan.bv_key_switch(T, r, c.data_ptr(), kb.data_ptr(), ka.data_ptr(), T, add0.data_ptr(), add1.data_ptr(),
                               k0.data_ptr(), k1.data_ptr(), 0, B, st)

        def shipped_before():
            plan.bv_precompute(T, c.data_ptr(), dd.data_ptr(), B, st)
            plan.bv_core(T, dd.data_ptr(), kb.data_ptr(), ka.data_ptr(), T, p0.data_ptr(), p1.data_ptr(), B, st)
            plan.mod_add(add0.data_ptr(), p0.data_ptr(), p0.data_ptr(), B, st)
            plan.mod_add(add1.data_ptr(), p1.data_ptr(), p1.data_ptr(), B, st)

        contenders = {"separate": separate, "one_call": one_call, "hybrid_dnum3": hybrid}
        if r == 0:
            contenders["shipped_before_precompute_core"] = shipped_before
        with torch.cuda.stream(s):
            for fn in contenders.values():
                fn()
        torch.cuda.synchronize()
        assert torch.equal(s0, k0) and torch.equal(s1, k1), "the one call differs from the separate calls"
        if r == 0:
            assert torch.equal(p0, k0) and torch.equal(p1, k1), "digit_size 0 differs from bv_precompute + bv_core"
        tt = alternate(contenders, repeats)
        entry = {"n_digits": nd, "contenders": tt,
                 "one_call_minus_separate_ms": tt["one_call"]["median"] - tt["separate"]["median"]}
        if r == 0:
            old = tt["shipped_before_precompute_core"]
            entry["shipped_before_spread_ms"] = old["max"] - old["min"]
            entry["one_call_minus_shipped_before_ms"] = tt["one_call"]["median"] - old["median"]
            entry["one_call_within_spread"] = entry["one_call_minus_shipped_before_ms"] <= entry["shipped_before_spread_ms"]
        res["digit_sizes"][str(r)] = entry
        del kb, ka, dd
        torch.cuda.empty_cache()

    # the inner product alone, plain against key-stationary
    res["inner_product"] = {}
    nd = plan.bv_digit_count(T, INNER_R)
    kb, ka = uniform((nd, T, n), q), uniform((nd, T, n), q)
    for Bi in INNER_BATCHES:
        print(f" inner product, batch {Bi}, {nd} digits", flush=True)
        dd = uniform((Bi, nd, T, n), q)
        outs = {nb: (empty(Bi, T, n), empty(Bi, T, n)) for nb in INNER_NB}

        def inner(nb):
            def fn():
                H.bv_tune(nb)
                o0, o1 = outs[nb]
                plan.bv_core_digits(T, nd, dd.data_ptr(), kb.data_ptr(), ka.data_ptr(), T, o0.data_ptr(),
                                    o1.data_ptr(), Bi, st)
            return fn

        names = {0: "library_choice", 1: "plain", 2: "key_stationary_2", 4: "key_stationary_4"}
        contenders = {names[nb]: inner(nb) for nb in INNER_NB}
        with torch.cuda.stream(s):
            for fn in contenders.values():
                fn()
        torch.cuda.synchronize()
        for nb in INNER_NB[1:]:
            assert torch.equal(outs[1][0], outs[nb][0]) and torch.equal(outs[1][1], outs[nb][1]), nb
        tt = alternate(contenders, repeats)
        need = 8 * T * n * (Bi * nd + 2 * nd + 2 * Bi)  # digits, keys and outputs once each
        for v in tt.values():
            v.update(bytes_needed=need, tb_per_s=need / (v["median"] * 1e-3) / 1e12)
        res["inner_product"][f"batch{Bi}"] = {"n_digits": nd, "contenders": tt,
                                              "fastest": min((k for k in tt if k != "library_choice"),
                                                             key=lambda k: tt[k]["median"])}
        del dd, outs
        torch.cuda.empty_cache()
    H.bv_tune(0)
    ks.close(), plan.close()
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
