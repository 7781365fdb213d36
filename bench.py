#!/usr/bin/env python3
"""Headline benchmark: 64-bit coefficients/s for c = INTT(NTT(a) (.) b) on
N = 2^16, 16 towers, batch 1024 per GPU (BASELINE.json configs[2]).

  python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]

A plain run sets up, runs W untimed and K timed steps, writes the outputs of
the last timed step when --dump-outputs is given, and prints the result line
(`value`, `ms_per_step`: one timed step).  --full adds, after the timed
region, everything else the line can carry: the per-kernel times and the
pipeline's HBM- and VALU-roofline fractions, the power sample, the spot
check against the oracle, the secondary operations, configs[3] / [4] / [0],
the PCIe-inclusive rate and a CPU baseline on the host cores.

--gpus N > 1 without WORLD_SIZE in the environment starts N ranks itself
(torch.distributed.run, one process per GPU) before anything touches the GPU;
under an external launcher WORLD_SIZE must equal N.  Each rank runs its own
batch (weak scaling, no data-path collective); the only collective is the
RCCL evaluation-key broadcast at setup.  Secondary lines in
the same JSON object under --full: configs[3] (32 towers split over the ranks, strong
scaling), configs[4] (HYBRID key switching, one bounded sample), configs[0]
(CPU-only add / Hadamard, poly-benchmark semantics).

Rank 0 prints ONE JSON line.
"""
import argparse
import hashlib
import glob
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "upmem--openfhe_amd"))

METRIC = "64-bit coeffs/sec for NTT+Hadamard+INTT, N=2^16, 16 towers; % HBM roofline"
HBM_PEAK_GBS = 8000.0          # MI355X_MICROARCH.md: 8 TB/s
ALG_BYTES_PER_COEFF = 24       # read a, read b, write c
# per-launch algorithmic bytes per coefficient of the three pipeline kernels
KERNEL_BYTES = {"colpass<fwd>": 16, "k_block<fused>": 24, "colpass<inv>": 16}
STAGE_NAMES = {0: "colpass<fwd>", 1: "k_block<fused>", 2: "colpass<inv>"}  # colpass = k_tcols (2^16) or k_cols
SIMDS = 1024                   # 256 CUs x 4 SIMDs
VALU_ISSUE_CEILING = 0.25      # wave64 VALU instructions per SIMD per cycle (4-cycle issue)
REF_CPU_MS_1T = 41.1           # reference NTT+Hadamard+INTT, 2^16 x 16 towers, 1 thread
PMC_FILE = os.path.join(ROOT, "profiles", "pmc_current.json")
DUMP_MAX_WORDS = 1 << 20       # --dump-outputs: words per output (3 float64 arrays of 8 MiB each)
DUMP_SEED = 0x5EED             # --dump-outputs: seed of the sample of a larger output


def build_id() -> str:
    """Hash of the backend's sources: PMC summaries are used only for the build they measured."""
    h = hashlib.sha256()
    csrc = os.path.join(ROOT, "upmem--openfhe_amd", "csrc")
    for f in sorted(glob.glob(os.path.join(csrc, "*.hip")) + glob.glob(os.path.join(csrc, "*.hpp")) +
                    [os.path.join(csrc, "Makefile"), os.path.join(ROOT, "include", "ofhe_hip.h")]):
        h.update(os.path.basename(f).encode())
        h.update(open(f, "rb").read())
    return h.hexdigest()[:16]


def moduli_chain(log_n, towers, bits=60):
    """poly-benchmark modulus chain (benchmark/src/poly-benchmark-16k.cpp:89-96)
    and minimal primitive 2N-th roots (nbtheory-impl.h:183-231).  Product-side
    setup code (not the oracle): deterministic Miller-Rabin in Python ints."""
    m = 2 << log_n

    def is_prime(n):
        if n < 2:
            return False
        for p in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37):
            if n % p == 0:
                return n == p
        d, s = n - 1, 0
        while d % 2 == 0:
            d //= 2
            s += 1
        for a in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37):
            x = pow(a, d, n)
            if x in (1, n - 1):
                continue
            for _ in range(s - 1):
                x = x * x % n
                if x == n - 1:
                    break
            else:
                return False
        return True

    q = (1 << bits) + 1
    while not is_prime(q):
        q += m
    qs, roots = [], []
    for _ in range(towers):
        q -= m
        while not is_prime(q):
            q -= m
        qs.append(q)
        e = (q - 1) // m
        c = 2
        while True:
            x = pow(c, e, q)
            if pow(x, m // 2, q) == q - 1:
                break
            c += 1
        x2 = x * x % q
        best, y = x, x
        for _ in range(m // 2 - 1):
            y = y * x2 % q
            if y < best:
                best = y
        roots.append(best)
    return qs, roots


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--log-n", type=int, default=16)
    ap.add_argument("--towers", type=int, default=16)
    ap.add_argument("--batch", type=int, default=1024, help="polynomials per GPU")
    ap.add_argument("--full", action="store_true",
                    help="pipeline workload: after the timed steps also measure and check everything else the "
                         "line carries (per-kernel times and roofline, power, oracle spot check, secondary "
                         "operations, configs[3]/[4]/[0], PCIe and CPU legs); a plain run does none of it")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="pipeline workload: after the timed steps write what the last one computed to "
                         "DIR/<name>.npy (float64; a fixed seeded sample of a large output)")
    ap.add_argument("--cpu-seconds", type=float, default=10.0, help="--full: CPU baseline budget (0 = skip)")
    ap.add_argument("--no-check", action="store_true", help="--full: skip the oracle spot check")
    ap.add_argument("--no-extras", action="store_true",
                    help="--full: skip power, secondary operations, configs[3]/[4]/[0], PCIe and CPU legs")
    ap.add_argument("--workload", default="pipeline", choices=["pipeline", "keyswitch", "rescale", "bv_keyswitch"],
                    help="pipeline = the headline metric (configs[2]); keyswitch = configs[4] HYBRID "
                         "key switching as the main line; rescale / bv_keyswitch = callers outside SURVEY.md "
                         "§8's rows (CKKS rescaling, BV key switching), measured only on request")
    ap.add_argument("--shard", default="batch", choices=["batch", "towers"],
                    help="batch = every rank runs its own batch of --batch (weak scaling, the default line); "
                         "towers = configs[3] as the main line: --towers split across ranks (strong scaling)")
    ap.add_argument("--c3-towers", type=int, default=32, help="configs[3] towers (split over ranks)")
    ap.add_argument("--c3-batch", type=int, default=512, help="configs[3] polynomials (the same on every rank)")
    ap.add_argument("--ks-batch", type=int, default=8, help="ciphertext polynomials per GPU (keyswitch)")
    ap.add_argument("--ks-steps", type=int, default=10, help="keyswitch sample steps in the default run")
    ap.add_argument("--pcie-batch", type=int, default=32, help="polynomials per chunk of the PCIe-inclusive run")
    ap.add_argument("--pcie-chunks", type=int, default=16, help="chunks of the PCIe-inclusive run (0 = skip)")
    ap.add_argument("--dist-backend", default="nccl", choices=["nccl", "gloo"],
                    help="nccl (RCCL, one GPU per rank); gloo = rehearsal of the N-rank path on one GPU")
    ap.add_argument("--launch-check", action="store_true",
                    help="start the ranks and report them (gloo, no GPU): checks the --gpus launcher")
    ap.add_argument("--require-capi-comm", action="store_true",
                    help="at N > 1, exit 3 (after printing the JSON line) unless every evaluation-key broadcast "
                         "went through the C ABI's RCCL communicator (ofhe_hip_bcast_evalkey)")
    return ap.parse_args(argv)


# ---------------------------------------------------------------------------
# Launch: --gpus N starts N ranks itself unless an external launcher did
# ---------------------------------------------------------------------------
def _free_port() -> int:
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def launch_ranks(n: int) -> int:
    """One process per GPU through torch.distributed.run, started as a child
    (this process has not touched the GPU); returns the launcher's exit code."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.abspath(__file__)]
    cmd += sys.argv[1:]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    return subprocess.call(cmd, env=env)


def capi_status(records, world):
    """Top-level summary of how the evaluation keys travelled: capi is True only
    when every broadcast of the run used ofhe_hip_bcast_evalkey (None at N = 1:
    nothing is broadcast); reasons name each fallback, then every rank whose
    own C-ABI communicator failed (the records' "ranks", shard.key_broadcaster
    .per_rank); per_rank lists, per broadcast, the ranks whose communicator
    came up and those that did not."""
    recs = {k: v for k, v in records.items() if v}
    if world <= 1 or not recs:
        return {"capi": None, "reasons": [], "broadcasts": sorted(recs), "per_rank": {}}
    bad = {k: v.get("backend") for k, v in recs.items() if not v.get("capi")}
    reasons = [f"{k}: {why}" for k, why in sorted(bad.items())]
    per_rank = {}
    for k, v in sorted(recs.items()):
        ranks = v.get("ranks") or []
        per_rank[k] = {"comm_up": sorted(r["rank"] for r in ranks if r.get("comm")),
                       "comm_failed": sorted(r["rank"] for r in ranks if not r.get("comm"))}
        reasons += [f"{k}: rank {r['rank']}: {r.get('error')}" for r in sorted(ranks, key=lambda r: r["rank"])
                    if not r.get("comm")]
    return {"capi": not bad, "reasons": reasons, "broadcasts": sorted(recs), "per_rank": per_rank}


def capi_exit_code(status, require: bool) -> int:
    """--require-capi-comm: 3 when a broadcast fell back (the JSON is printed first)."""
    return 3 if require and status.get("capi") is False else 0


def launch_check(args):
    """Each rank joins a gloo group; rank 0 prints the ranks that came up and
    how the key broadcaster came up (no GPU: the C-ABI communicator cannot, so
    the ranks fall back together; --require-capi-comm then exits 3)."""
    import torch
    import torch.distributed as dist

    import shard

    dist.init_process_group("gloo")
    world, rank = dist.get_world_size(), dist.get_rank()
    info = [None] * world
    dist.all_gather_object(info, {"rank": rank, "pid": os.getpid(), "local_rank": int(os.environ["LOCAL_RANK"])})
    bfn, backend, comm = shard.key_broadcaster(None, rank, world)
    key = torch.arange(64, dtype=torch.int64) if rank == 0 else torch.zeros(64, dtype=torch.int64)
    bfn(key, 0)
    rec = {"backend": backend, "capi": comm is not None, "verified": shard.same_on_all_ranks(key),
           "ranks": bfn.per_rank}
    status = capi_status({"launch_check": rec}, world)
    if rank == 0:
        print(json.dumps({"launch_check": True, "n_gpus": world, "ranks": [i["rank"] for i in info],
                          "local_ranks": [i["local_rank"] for i in info], "pids": [i["pid"] for i in info],
                          "evalkey_broadcast": rec, "evalkey_broadcast_capi": status}), flush=True)
    if comm is not None:
        comm.close()
    dist.barrier()
    dist.destroy_process_group()
    return capi_exit_code(status, args.require_capi_comm)


def main():
    args = parse_args()
    env_world = os.environ.get("WORLD_SIZE")
    if env_world is None and args.gpus > 1:
        sys.exit(launch_ranks(args.gpus))
    if env_world is not None and int(env_world) != args.gpus:
        print(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={env_world}; they must agree", file=sys.stderr)
        sys.exit(2)
    if args.launch_check:
        if env_world is None:
            print(json.dumps({"launch_check": True, "n_gpus": 1, "ranks": [0], "pids": [os.getpid()]}))
            return
        sys.exit(launch_check(args))
    if args.dump_outputs and args.workload != "pipeline":
        print("bench.py: --dump-outputs writes the pipeline workload's outputs only", file=sys.stderr)
        sys.exit(2)
    if args.workload == "keyswitch":
        sys.exit(bench_keyswitch_main(args))
    if args.workload in ("rescale", "bv_keyswitch"):
        sys.exit(bench_extra_main(args))
    sys.exit(bench_pipeline(args))


# ---------------------------------------------------------------------------
# Headline: configs[2]
# ---------------------------------------------------------------------------
def _dist_setup(backend="nccl"):
    """One process per GPU: RCCL ("nccl") over the ranks' own devices.
    backend "gloo" is a rehearsal mode for a one-GPU box (every rank on
    cuda:0, host-staged collectives; the C-ABI communicator then fails to come
    up on a shared device and the ranks fall back together)."""
    import torch
    import torch.distributed as dist

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if backend == "gloo":
        local = 0
    if world > 1:
        torch.cuda.set_device(local)
        if backend == "gloo":
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=torch.device("cuda", local))
    dev = torch.device("cuda", local)
    torch.cuda.set_device(dev)
    return world, rank, local, dev


def _timed(step, steps, warmup, stream, world, dev):
    """W untimed steps, then K steps bracketed by barrier + synchronize; returns
    (max-over-ranks host seconds, launch-stream event ms per step)."""
    import torch
    import torch.distributed as dist

    import shard

    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record(stream)
    for _ in range(steps):
        step()
    e1.record(stream)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    if world > 1:
        elapsed = shard.max_over_ranks(elapsed, device=dev)
    return elapsed, e0.elapsed_time(e1) / steps


def load_pmc(log_n, towers, batch):
    """profiles/pmc_current.json (tools/pmc_round.sh) when it measured this build
    and this configuration; else None with the reason."""
    if not os.path.exists(PMC_FILE):
        return None, "no profiles/pmc_current.json"
    try:
        pm = json.load(open(PMC_FILE))
    except Exception as e:  # noqa: BLE001
        return None, f"unreadable pmc file: {e}"
    if pm.get("build_id") != build_id():
        return None, f"pmc file measured build {pm.get('build_id')}, this is {build_id()}"
    c = pm.get("config", {})
    if (c.get("log_n"), c.get("towers"), c.get("batch")) != (log_n, towers, batch):
        return None, f"pmc file measured {c}, this run is log_n={log_n} towers={towers} batch={batch}"
    return pm, None


def headline_config(shard_mode, world, log_n, T_total, B):
    """The line's config block.  batch: configs[2], every rank its own batch
    of B; towers: configs[3], T_total towers split in contiguous ranges over
    the ranks (rank 0's share is towers_rank0), the same B on every rank."""
    import shard

    if shard_mode == "batch":
        return {"workload": f"configs[2]: N=2^{log_n}, towers={T_total}, batch={B} per GPU, c = INTT(NTT(a) (.) b)",
                "log_n": log_n, "towers": T_total, "batch_per_gpu": B, "global_batch": B * world,
                "parallelism": f"batch-sharded x{world} (no data-path collective)"}
    return {"workload": f"configs[3]: N=2^{log_n}, towers={T_total} split over {world} GPUs, "
                        f"batch={B}, c = INTT(NTT(a) (.) b)",
            "log_n": log_n, "towers": T_total, "towers_rank0": shard.shard_towers(T_total, 0, world)[1],
            "global_batch": B, "parallelism": f"tower-sharded x{world} (no data-path collective)"}


def dump_sample_index(numel):
    """--dump-outputs: the flat indices written of an output of `numel` words:
    None (all of it) up to DUMP_MAX_WORDS, else DUMP_MAX_WORDS indices drawn
    with a fixed seed (the same for every run and build), ascending."""
    import numpy as np

    if numel <= DUMP_MAX_WORDS:
        return None
    return np.sort(np.random.default_rng(DUMP_SEED).integers(0, numel, size=DUMP_MAX_WORDS, dtype=np.int64))


def dump_arrays(name, words):
    """--dump-outputs: the float64 arrays one output of uint64 residues becomes.
    <name> holds the residues themselves (rounded to float64's 53 bits above
    2^53), <name>_lo32 / <name>_hi32 their low and high 32 bits, which float64
    holds exactly: residue = hi32 * 2^32 + lo32."""
    import numpy as np

    assert words.dtype == np.uint64
    return {name: words.astype(np.float64), name + "_lo32": (words & np.uint64(0xFFFFFFFF)).astype(np.float64),
            name + "_hi32": (words >> np.uint64(32)).astype(np.float64)}


def dump_outputs(dirname, outputs):
    """--dump-outputs DIR: every output tensor (int64 storage of uint64
    residues, on the device) as DIR/<name>.npy, DIR/<name>_lo32.npy and
    DIR/<name>_hi32.npy; whole and in its own shape when it has at most
    DUMP_MAX_WORDS words, else the 1-D sample of dump_sample_index.  Returns
    what was written, for the result line."""
    import numpy as np
    import torch

    os.makedirs(dirname, exist_ok=True)
    written = {}
    for name, t in outputs.items():
        idx = dump_sample_index(t.numel())
        sel = t if idx is None else t.reshape(-1)[torch.from_numpy(idx).to(t.device)]
        words = sel.cpu().numpy().view(np.uint64)
        for fname, arr in dump_arrays(name, words).items():
            np.save(os.path.join(dirname, fname + ".npy"), arr)
            written[fname] = {"shape": list(arr.shape), "dtype": str(arr.dtype)}
        written[name]["of_shape"] = list(t.shape)
        written[name]["sampled"] = idx is not None
    return written


def bench_pipeline(args):
    import torch
    import torch.distributed as dist

    world, rank, local, dev = _dist_setup(args.dist_backend)

    import ofhe_hip as H
    import shard

    log_n, T_total, B = args.log_n, args.towers, args.batch
    if args.shard == "batch":
        b0, B_rank = shard.shard_batch(args.batch * world, rank, world)
        assert B_rank == args.batch
        t_start, T = 0, T_total
    else:
        b0 = 0
        t_start, T = shard.shard_towers(T_total, rank, world)
        if T == 0:
            raise SystemExit(f"--shard towers needs at least one tower per rank ({T_total} over {world})")

    ctx = H.Context(local)
    n = 1 << log_n
    qs_all, roots_all = moduli_chain(log_n, T_total)
    qs, roots = qs_all[t_start:t_start + T], roots_all[t_start:t_start + T]
    plan = H.NTTPlan(ctx, log_n, qs, roots)
    stream = torch.cuda.current_stream(dev)
    sp = stream.cuda_stream

    # synthetic inputs, SURVEY.md §8(d): splitmix64 seed 0x5EED ^ (b<<20) ^ (t<<8) ^ operand,
    # mod q_t, generated on the device (global batch index b)
    a = torch.empty((B, T, n), dtype=torch.int64, device=dev)
    b = torch.empty((B, T, n), dtype=torch.int64, device=dev)
    plan.fill_uniform(a.data_ptr(), B, 1, b0, sp)
    plan.fill_uniform(b.data_ptr(), B, 2, b0, sp)
    c = torch.empty_like(a)

    # RCCL broadcast of a synthetic hybrid key-switching key (setup, outside the
    # timed loop -- the only collective the path has)
    bcast, comm = None, None
    if world > 1:
        key = torch.empty(shard.evalkey_words(T_total, log_n, 3), dtype=torch.int64, device=dev)
        if rank == 0:
            key.random_(0, qs[-1])
        bfn, backend, comm = shard.key_broadcaster(ctx, rank, world)
        dist.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        bfn(key, 0)
        torch.cuda.synchronize()
        bcast = {"bytes": key.numel() * 8, "ms": (time.perf_counter() - t0) * 1e3, "backend": backend,
                 "capi": comm is not None, "verified": shard.same_on_all_ranks(key), "ranks": bfn.per_rank}
        del key

    def step():
        plan.ntt_mul_intt(a.data_ptr(), b.data_ptr(), c.data_ptr(), B, sp)

    elapsed, pipe_ms = _timed(step, args.steps, args.warmup, stream, world, dev)
    coeffs_rank = B * T * n
    coeffs_per_step = coeffs_rank * world if args.shard == "batch" else B * T_total * n
    value = coeffs_per_step * args.steps / elapsed
    ms_per_step = elapsed / args.steps * 1e3

    # c is what the last timed step left: written before anything else runs on it
    dumped = dump_outputs(args.dump_outputs, {"c": c}) if (args.dump_outputs and rank == 0) else None

    # everything below the timed region that takes runs of its own: --full only
    kernels_ms, roofline, power, parity, secondary, extras = {}, None, None, None, None, {}
    if args.full:
        # per-kernel durations with HIP events on the launch stream (separate pass)
        reps = max(3, min(args.steps, 10))
        for st in (0, 1, 2):
            if log_n <= 12 and st != 1:
                continue
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            plan.ntt_mul_intt_stage(0, a.data_ptr(), b.data_ptr(), c.data_ptr(), B, sp)
            plan.ntt_mul_intt_stage(1, a.data_ptr(), b.data_ptr(), c.data_ptr(), B, sp)
            ev0.record(stream)
            for _ in range(reps):
                plan.ntt_mul_intt_stage(st, a.data_ptr(), b.data_ptr(), c.data_ptr(), B, sp)
            ev1.record(stream)
            ev1.synchronize()
            kernels_ms[STAGE_NAMES[st]] = ev0.elapsed_time(ev1) / reps

        roofline = make_roofline(pipe_ms, kernels_ms, coeffs_rank, log_n, T, B, ms_per_step=ms_per_step)
        power = power_sample(step, pipe_ms, local) if (rank == 0 and not args.no_extras) else None

        # spot parity check against the oracle (two (batch, tower) rows)
        if not args.no_check and rank == 0:
            sys.path.insert(0, os.path.join(ROOT, "oracle"))
            import numpy as np
            import oracle as O

            step()
            torch.cuda.synchronize()
            ok = True
            for bi, ti in ((0, 0), (B - 1, T - 1)):
                tb = O.Tables(n, [qs[ti]], [roots[ti]])
                aa = a[bi, ti].cpu().numpy().view(np.uint64).reshape(1, 1, n)
                bb = b[bi, ti].cpu().numpy().view(np.uint64).reshape(1, 1, n)
                cc = c[bi, ti].cpu().numpy().view(np.uint64).reshape(1, 1, n)
                want_a = O.splitmix_fill(n, qs[ti], O.U([0x5EED ^ ((b0 + bi) << 20) ^ ((t_start + ti) << 8) ^ 1]))
                ok = ok and bool(np.array_equal(aa.reshape(-1), want_a))
                ok = ok and bool(np.array_equal(cc, O.ntt_mul_intt(aa, bb, tb)))
            parity = ok

        if not args.no_extras:
            secondary = secondary_ops(plan, a, b, c, B, T, n, stream)
        del a, b, c
        torch.cuda.empty_cache()
        if not args.no_extras:
            extras["configs3"] = bench_configs3(args, ctx, world, rank, dev)
            extras["keyswitch"] = bench_keyswitch(args, ctx, world, rank, dev, steps=args.ks_steps, warmup=2,
                                                  with_stages=True)
            if rank == 0 and world == 1:
                extras["pcie_inclusive"] = (pcie_inclusive(plan, args.pcie_batch, args.pcie_chunks, dev)
                                            if args.pcie_chunks > 0 else None)
                extras["configs0"] = bench_configs0(ctx)
                extras["cpu_baseline"] = cpu_baseline(args, qs, roots, log_n, T) if args.cpu_seconds > 0 else None

    status = capi_status({"headline": bcast, "keyswitch": (extras.get("keyswitch") or {}).get("evalkey_broadcast")},
                         world)
    if rank == 0:
        out = {
            "metric": METRIC,
            "value": value,
            "unit": "coeffs/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": ms_per_step,
            "higher_is_better": True,
            "full": args.full,
            "outputs": dumped,
            "scaling": "weak" if args.shard == "batch" else "strong",
            "vs_baseline": None,
            "dtype": "u64",
            "data": "synthetic: splitmix64 residues mod q_t, seed 0x5EED^(b<<20)^(t<<8)^operand "
                    "(SURVEY.md §8(d)), generated on the device; a coefficient form, b evaluation form",
            "config": headline_config(args.shard, world, log_n, T_total, B),
            "roofline": roofline,
            "kernels_ms": kernels_ms,
            "cpu_baseline": extras.get("cpu_baseline"),
            "parity_spot_check": parity,
            "evalkey_broadcast": bcast,
            "evalkey_broadcast_capi": status,
            "power": power,
            "secondary_ops": secondary,
            "configs3": extras.get("configs3"),
            "keyswitch": extras.get("keyswitch"),
            "configs0": extras.get("configs0"),
            "pcie_inclusive": extras.get("pcie_inclusive"),
            "build_id": build_id(),
        }
        print(json.dumps(out), flush=True)
    if world > 1:
        torch.cuda.synchronize()
        if comm is not None:
            comm.close()
        dist.barrier()
        dist.destroy_process_group()
    return capi_exit_code(status, args.require_capi_comm)


def power_sample(step, ms_per_step, device, seconds=4.0):
    """Package power, power cap and sclk of this rank's GPU while the metric
    pipeline runs (outside the timed region): ~`seconds` of steps are queued,
    rocm-smi is read once the firmware has settled, then the queue drains.
    The pipeline runs at the package power cap on MI355X; the
    clock the cap allows is what the VALU-bound kernels scale with."""
    import re
    import subprocess

    import torch

    n = max(20, int(seconds * 1e3 / max(ms_per_step, 1e-3)))
    for _ in range(n):
        step()
    done = torch.cuda.Event()
    done.record()
    time.sleep(min(1.5, 0.35 * seconds))
    try:
        txt = subprocess.run(["rocm-smi", "-d", str(device), "--showpower", "--showmaxpower", "--showclocks"],
                             capture_output=True, text=True, timeout=20).stdout
    except Exception as e:  # no rocm-smi: report why, never fail the bench
        torch.cuda.synchronize()
        return {"error": f"{type(e).__name__}: {e}"}
    # the reading is valid only if the queued steps were still running when it returned
    busy = not done.query()
    torch.cuda.synchronize()

    def num(pat):
        m = re.search(pat, txt)
        return float(m.group(1)) if m else None

    return {"package_w": num(r"(?:Current Socket|Average) Graphics Package Power \(W\): ([0-9.]+)"), "cap_w": num(r"Max Graphics Package Power \(W\): ([0-9.]+)"),
            "sclk_mhz": num(r"sclk clock level: \d+: \((\d+)Mhz\)"), "steps_queued": n, "under_load": busy,
            "source": "rocm-smi during ~%.0f s of pipeline steps after the timed region" % seconds}


def secondary_ops(plan, a, b, c, B, T, n, stream, reps=3):
    """SURVEY.md §8(d)'s secondary figures at the headline shape, on the same
    device-resident buffers: the standalone forward / inverse NTT (16
    algorithmic B per coefficient: read, write) and the vector ModMul / ModAdd
    (24 B: two reads, one write), HIP events on the launch stream, after the
    timed region (they leave a and b unchanged: the transforms run on c)."""
    import torch

    sp = stream.cuda_stream
    coeffs = B * T * n
    ops = {
        "ntt_fwd": (16, lambda: plan.forward(c.data_ptr(), B, sp)),
        "ntt_inv": (16, lambda: plan.inverse(c.data_ptr(), B, sp)),
        "modmul": (24, lambda: plan.mod_mul(a.data_ptr(), b.data_ptr(), c.data_ptr(), B, sp)),
        "modadd": (24, lambda: plan.mod_add(a.data_ptr(), b.data_ptr(), c.data_ptr(), B, sp)),
    }
    out = {}
    for name, (bpc, fn) in ops.items():
        fn()
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record(stream)
        for _ in range(reps):
            fn()
        ev1.record(stream)
        ev1.synchronize()
        ms = ev0.elapsed_time(ev1) / reps
        gbs = bpc * coeffs / (ms * 1e-3) / 1e9
        out[name] = {"ms": ms, "coeffs_per_s": coeffs / (ms * 1e-3), "alg_bytes_per_coeff": bpc,
                     "achieved_gbs": gbs, "hbm_frac": gbs / HBM_PEAK_GBS}
    out["config"] = f"N=2^{n.bit_length() - 1}, towers={T}, batch={B} (the headline buffers)"
    return out


def make_roofline(pipe_ms, kernels_ms, coeffs_rank, log_n, T, B, ms_per_step=None):
    """Roofline of the metric op, the unit the north star's >= 0.40 target is
    stated on (schema 3, round 6): 24 algorithmic B per coefficient (read a,
    read b, write c) x the coefficients one GPU processes per
    step / ms_per_step (the timed region; HIP-event time of the same three
    launches when ms_per_step is not given).  The op is three launches back to
    back, so `traffic` is the three launches' PMC HBM bytes per step.  Beside
    it: the dominant kernel (its own algorithmic bytes per launch over its
    average launch duration, HIP events on the launch stream; schema 2's
    top-level figure, now `dominant_kernel_frac`), and every launch under
    "kernels".  VALU: the measured VALU instructions per coefficient
    (SQ_INSTS_VALU, profiles/pmc_current.json, same build and configuration)
    at the measured clock and the 0.25 wave64 instructions per SIMD per cycle
    issue ceiling give the VALU-bound time; its ratio to the measured time is
    the VALU fraction.  `bound` is the roof the counters put closer: "valu"
    for these kernels, which the task's "hbm" | "mfma" does not name (gfx950
    has no 64-bit integer multiplier and the path runs no matrix
    instructions)."""
    pm, why = load_pmc(log_n, T, B)
    pk = (pm or {}).get("kernels", {})
    kernels = {}
    valu_ms_total, valu_ok, traffic_total = 0.0, bool(pk), 0.0
    for name, ms in kernels_ms.items():
        alg = KERNEL_BYTES[name] * coeffs_rank
        ent = {"ms": ms, "alg_bytes": alg, "achieved_gbs": alg / (ms * 1e-3) / 1e9,
               "hbm_frac": alg / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, "traffic": None, "valu": None}
        p = pk.get(name)
        if p:
            ent["traffic"] = p.get("hbm_bytes_per_launch")
            if ent["traffic"] is not None:
                traffic_total += ent["traffic"]
            ipc = p.get("valu_insts_per_coeff")
            clk = p.get("clock_ghz")
            if ipc and clk:
                vms = ipc * coeffs_rank / 64 / (SIMDS * clk * 1e9 * VALU_ISSUE_CEILING) * 1e3
                ent["valu"] = {"lane_insts_per_coeff": ipc, "clock_ghz": clk, "valu_bound_ms": vms,
                               "valu_frac": vms / ms}
                valu_ms_total += vms
            else:
                valu_ok = False
        else:
            valu_ok = False
        ent["bound"] = (("valu" if ent["valu"]["valu_frac"] > ent["hbm_frac"] else "hbm")
                        if ent["valu"] else None)
        kernels[name] = ent
    step_ms = ms_per_step if ms_per_step else pipe_ms
    alg = ALG_BYTES_PER_COEFF * coeffs_rank
    achieved = alg / (step_ms * 1e-3) / 1e9
    hbm_frac = achieved / HBM_PEAK_GBS
    valu = None
    if valu_ok and valu_ms_total > 0:
        valu = {"valu_bound_ms": valu_ms_total, "frac": valu_ms_total / step_ms,
                "lane_insts_per_coeff": sum(kernels[k]["valu"]["lane_insts_per_coeff"] for k in kernels),
                "issue_ceiling": VALU_ISSUE_CEILING, "simds": SIMDS,
                "source": "profiles/pmc_current.json (tools/pmc_round.sh, SQ_INSTS_VALU + GRBM_GUI_ACTIVE)"}
    traffic = traffic_total if (pk and all(kernels[k]["traffic"] for k in kernels)) else None
    bound = ("valu" if valu["frac"] > hbm_frac else "hbm") if valu else None
    dominant = max(kernels_ms, key=kernels_ms.get)
    d = kernels[dominant]
    return {"schema": 3, "bound": bound, "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
            "frac": hbm_frac, "traffic": traffic,
            "scope": f"the metric op c = INTT(NTT(a) (.) b) on one GPU: {ALG_BYTES_PER_COEFF} algorithmic B per "
                     f"coefficient x {coeffs_rank} coefficients per step / ms per step (three launches: forward "
                     "column pass, fused block pass, inverse column pass; traffic = their PMC HBM bytes per step); "
                     "the north star's >= 0.40 target is stated on this",
            "alg_bytes_per_step": alg, "ms_per_step": step_ms, "ms_per_step_events": pipe_ms,
            "pipeline_frac": hbm_frac, "valu": valu,
            "dominant_kernel": dominant, "dominant_kernel_frac": d["hbm_frac"],
            "dominant_kernel_achieved": d["achieved_gbs"], "dominant_kernel_ms": d["ms"],
            "dominant_kernel_traffic": d["traffic"],
            "dominant_kernel_scope": f"{dominant}: {KERNEL_BYTES[dominant]} algorithmic B per coefficient x "
                                     f"{coeffs_rank} coefficients per launch / its average launch duration "
                                     "(HIP events on the launch stream)",
            "kernels": kernels, "counters": "matched" if pm else why}


# ---------------------------------------------------------------------------
# configs[3]: 32 towers split into contiguous ranges over the ranks (strong scaling)
# ---------------------------------------------------------------------------
def bench_configs3(args, ctx, world, rank, dev):
    import torch
    import torch.distributed as dist

    import ofhe_hip as H
    import shard

    log_n, T_total, B = 16, args.c3_towers, args.c3_batch
    t0, T = shard.shard_towers(T_total, rank, world)
    n = 1 << log_n
    qs, roots = moduli_chain(log_n, T_total)
    plan = H.NTTPlan(ctx, log_n, qs[t0:t0 + T], roots[t0:t0 + T])
    stream = torch.cuda.current_stream(dev)
    sp = stream.cuda_stream
    a = torch.empty((B, T, n), dtype=torch.int64, device=dev)
    b = torch.empty_like(a)
    plan.fill_uniform(a.data_ptr(), B, 3, 0, sp)
    plan.fill_uniform(b.data_ptr(), B, 4, 0, sp)
    c = torch.empty_like(a)

    def step():
        plan.ntt_mul_intt(a.data_ptr(), b.data_ptr(), c.data_ptr(), B, sp)

    steps = max(3, args.steps // 2)
    elapsed, ev_ms = _timed(step, steps, 2, stream, world, dev)
    del a, b, c
    plan.close()
    torch.cuda.empty_cache()
    if world > 1:
        dist.barrier()
    total = B * T_total * n
    return {"workload": f"configs[3]: N=2^16, {T_total} towers split over {world} GPU(s) "
                        f"({T} on rank 0), batch {B}, c = INTT(NTT(a) (.) b)",
            "value": total * steps / elapsed, "unit": "coeffs/s", "scaling": "strong", "steps": steps,
            "ms_per_step": elapsed / steps * 1e3, "hbm_frac_per_gpu": total / world * 24 / (elapsed / steps) / 8e12,
            "towers_per_rank": T}


# ---------------------------------------------------------------------------
# CKKS rescaling (DCRTPolyImpl::DropLastElementAndScale, evaluation form) on
# configs[4]'s ring: 48 -> 47 towers at N = 2^17, a batch of ciphertext
# polynomials per GPU (batch-sharded)
# ---------------------------------------------------------------------------
def bench_rescale(args, ctx, world, rank, dev, steps, warmup):
    import torch
    import torch.distributed as dist

    import ofhe_hip as H
    import shard

    log_n, T = 17, 48
    n = 1 << log_n
    q, rq = moduli_chain(log_n, T)
    B = args.ks_batch
    ql = q[-1]
    a = [pow(ql, -1, qi) for qi in q[:-1]]  # qlInvModq
    c = [qi - ai for qi, ai in zip(q[:-1], a)]  # QlQlInvModqlDivqlModq = -ql^-1 mod q_i
    plan = H.NTTPlan(ctx, log_n, q, rq)
    stream = torch.cuda.current_stream(dev)
    sptr = stream.cuda_stream
    b0, _ = shard.shard_batch(B * world, rank, world)
    x = torch.empty((B, T, n), dtype=torch.int64, device=dev)
    plan.fill_uniform(x.data_ptr(), B, 8, b0, sptr)
    out = torch.empty((B, T - 1, n), dtype=torch.int64, device=dev)

    def step():
        plan.drop_last_and_scale(T, x.data_ptr(), T * n, out.data_ptr(), (T - 1) * n, True, c, a, B, sptr)

    elapsed, ev_ms = _timed(step, steps, warmup, stream, world, dev)
    del x, out
    plan.close()
    torch.cuda.empty_cache()
    if world > 1:
        dist.barrier()
    per = elapsed / steps
    return {"workload": f"DropLastElementAndScale (CKKS rescale), N=2^17, {T} -> {T - 1} towers, evaluation form, "
                        f"batch {B} per GPU",
            "value": B * world / per, "unit": "rescales/s", "scaling": "weak", "steps": steps,
            "ms_per_step": per * 1e3, "ms_per_step_events": ev_ms,
            "alg_hbm_gbs": B * (2 * T - 1) * n * 8 / per / 1e9,
            "note": "algorithmic bytes: read T towers, write T - 1 (8 B per word)"}


# ---------------------------------------------------------------------------
# BV key switching (digitSize = 0) on configs[4]'s ring and Q: N = 2^17, 48
# towers, 48 digits; 2 ciphertext polynomials per GPU (digits: 2.4 GiB each)
# ---------------------------------------------------------------------------
def bench_bv(args, ctx, world, rank, dev, steps, warmup):
    import torch
    import torch.distributed as dist

    import ofhe_hip as H
    import shard

    log_n, T, B = 17, 48, 2
    n = 1 << log_n
    q, rq = moduli_chain(log_n, T)
    plan = H.NTTPlan(ctx, log_n, q, rq)
    stream = torch.cuda.current_stream(dev)
    sptr = stream.cuda_stream
    b0, _ = shard.shard_batch(B * world, rank, world)
    c = torch.empty((B, T, n), dtype=torch.int64, device=dev)
    plan.fill_uniform(c.data_ptr(), B, 9, b0, sptr)
    kb = torch.empty((T, T, n), dtype=torch.int64, device=dev)
    ka = torch.empty_like(kb)
    plan.fill_uniform(kb.data_ptr(), T, 10, 0, sptr)
    plan.fill_uniform(ka.data_ptr(), T, 11, 0, sptr)
    d = torch.empty((B, T, T, n), dtype=torch.int64, device=dev)
    o0 = torch.empty((B, T, n), dtype=torch.int64, device=dev)
    o1 = torch.empty_like(o0)

    def step():
        plan.bv_precompute(T, c.data_ptr(), d.data_ptr(), B, sptr)
        plan.bv_core(T, d.data_ptr(), kb.data_ptr(), ka.data_ptr(), T, o0.data_ptr(), o1.data_ptr(), B, sptr)

    elapsed, ev_ms = _timed(step, steps, warmup, stream, world, dev)
    del c, kb, ka, d, o0, o1
    plan.close()
    torch.cuda.empty_cache()
    if world > 1:
        dist.barrier()
    per = elapsed / steps
    return {"workload": f"KeySwitchBV core, digitSize 0 (CRTDecompose + key inner product), N=2^17, {T} towers, "
                        f"batch {B} per GPU",
            "value": B * world / per, "unit": "keyswitch/s", "scaling": "weak", "steps": steps,
            "ms_per_step": per * 1e3, "ms_per_step_events": ev_ms}


# ---------------------------------------------------------------------------
# configs[4]: HYBRID key switching, N = 2^17, Q = 48, P = 16, dnum = 3
# ---------------------------------------------------------------------------
def bench_keyswitch(args, ctx, world, rank, dev, steps, warmup, with_stages=False):
    import torch
    import torch.distributed as dist

    import ofhe_hip as H
    import shard

    log_n, sq, sp_, dnum = 17, 48, 16, 3
    n = 1 << log_n
    allq, allr = moduli_chain(log_n, sq + sp_)
    q, rq, p, rp = allq[:sq], allr[:sq], allq[sq:], allr[sq:]
    B = args.ks_batch
    # BENCH_KS_SINGLE_STREAM=1: every digit on one stream (serial kernels, for
    # per-kernel PMC passes, tools/pmc_ks.sh)
    kso = H.KsOptions()
    kso.single_stream = 1 if os.environ.get("BENCH_KS_SINGLE_STREAM") == "1" else 0
    ks = H.KeySwitch(ctx, log_n, q, rq, p, rp, dnum, kso)
    _, beta = ks.digits(sq)
    pq = H.NTTPlan(ctx, log_n, q, rq)
    pqp = H.NTTPlan(ctx, log_n, q + p, rq + rp)
    stream = torch.cuda.current_stream(dev)
    sptr = stream.cuda_stream
    b0, _ = shard.shard_batch(B * world, rank, world)
    c = torch.empty((B, sq, n), dtype=torch.int64, device=dev)
    pq.fill_uniform(c.data_ptr(), B, 5, b0, sptr)
    kb = torch.empty((dnum, sq + sp_, n), dtype=torch.int64, device=dev)
    ka = torch.empty_like(kb)
    pqp.fill_uniform(kb.data_ptr(), dnum, 6, 0, sptr)
    pqp.fill_uniform(ka.data_ptr(), dnum, 7, 0, sptr)
    key_bcast, comm = None, None
    if world > 1:  # the evaluation key comes from rank 0 over RCCL (configs[3]/[4])
        bfn, backend, comm = shard.key_broadcaster(ctx, rank, world)
        bfn(kb, 0)
        bfn(ka, 0)
        key_bcast = {"backend": backend, "capi": comm is not None,
                     "verified": shard.same_on_all_ranks(kb) and shard.same_on_all_ranks(ka), "ranks": bfn.per_rank}
    o0 = torch.empty((B, sq, n), dtype=torch.int64, device=dev)
    o1 = torch.empty_like(o0)

    def step():
        ks.core(sq, c.data_ptr(), kb.data_ptr(), ka.data_ptr(), o0.data_ptr(), o1.data_ptr(), 0, B, sptr)

    elapsed, ev_ms = _timed(step, steps, warmup, stream, world, dev)
    stages, roof = None, None
    if with_stages:
        digits = torch.empty((B, beta, sq + sp_, n), dtype=torch.int64, device=dev)
        ct = torch.empty((2, B, sq + sp_, n), dtype=torch.int64, device=dev)
        stages = {}
        reps = max(2, min(steps, 5))

        def ev_time(fn):
            fn()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(reps):
                fn()
            e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1) / reps

        calls = {
            "mod_up(precompute)": lambda: ks.precompute(sq, c.data_ptr(), digits.data_ptr(), B, sptr),
            "inner_product": lambda: ks.fast_core_ext(sq, digits.data_ptr(), kb.data_ptr(), ka.data_ptr(),
                                                      ct[0].data_ptr(), ct[1].data_ptr(), B, sptr),
            "mod_down(x2)": lambda: (ks.mod_down(sq, ct[0].data_ptr(), o0.data_ptr(), 0, B, sptr),
                                     ks.mod_down(sq, ct[1].data_ptr(), o1.data_ptr(), 0, B, sptr)),
        }
        for name, fn in calls.items():
            stages[name] = ev_time(fn)
        # the standalone transform rate at this ring (the Q|P plan over the
        # digits buffer: B * beta polynomials of Q + P towers), forward and inverse
        tw = B * beta * (sq + sp_) * n
        ntt_fwd_ms = ev_time(lambda: pqp.forward(digits.data_ptr(), B * beta, sptr))
        ntt_inv_ms = ev_time(lambda: pqp.inverse(digits.data_ptr(), B * beta, sptr))
        roof = keyswitch_roofline(sq, sp_, dnum, n, B, ev_ms, stages, tw / (ntt_fwd_ms * 1e-3),
                                  tw / (ntt_inv_ms * 1e-3))
        del digits, ct
    # minimum HBM words per ciphertext polynomial and tower-coefficient: read c
    # (Q), write + read the digits (2 beta (Q+P)), write ct0/ct1 (2 (Q+P)),
    # ModDown reads them (2 (Q+P)) and writes out0/out1 (2 Q); keys are shared
    # by the batch and not counted
    qp = sq + sp_
    alg_words = sq + 2 * beta * qp + 4 * qp + 2 * sq
    if comm is not None:
        torch.cuda.synchronize()
        comm.close()
    del c, kb, ka, o0, o1
    ks.close()
    pq.close()
    pqp.close()
    torch.cuda.empty_cache()
    if world > 1:
        dist.barrier()
    return {"metric": "HYBRID key switches/sec (KeySwitchCore), N=2^17, 48+16 towers, dnum=3",
            "value": B * world * steps / elapsed, "unit": "keyswitch/s", "steps": steps, "warmup": warmup,
            "ms_per_step": elapsed / steps * 1e3, "ms_per_step_events": ev_ms, "scaling": "weak",
            "config": {"workload": "configs[4]: N=2^17, Q=48, P=16, dnum=3, KeySwitchCore",
                       "batch_per_gpu": B, "global_batch": B * world,
                       "parallelism": f"ciphertext-batch-sharded x{world}, key broadcast over RCCL"},
            "alg_hbm_gbs": alg_words * 8 * n * B / (elapsed / steps) / 1e9, "stages_ms": stages,
            "roofline": roof, "evalkey_broadcast": key_bcast}


def keyswitch_roofline(sq, sp, dnum, n, B, step_ms, stages, fwd_rate, inv_rate):
    """configs[4]'s key switch against its own bound (round 6): the NTTs it
    must run, at the standalone transform rate measured at this ring on this
    GPU (the path is bound by integer VALU issue), plus the key
    inner product's words at the 8 TB/s HBM peak.  Per ciphertext polynomial
    at level l = sq (keyswitch-hybrid.cpp:330-482): digit j (cnt_j of alpha
    towers) -> INTT of its cnt_j towers, NTT of the l - cnt_j + P complement
    towers; each of the two ApproxModDowns -> INTT of P towers, NTT of l
    towers.  Inner product HBM bytes per step: the digits B*beta*(l+P) towers
    read, the keys 2*beta*(l+P) (shared by the batch) read, ct0/ct1 2*B*(l+P)
    written, N words of 8 B each."""
    alpha = -(-sq // dnum)
    beta = min(-(-sq // alpha), dnum)
    cnts = [min(alpha, sq - alpha * j) for j in range(beta)]
    n_inv = sum(cnts) + 2 * sp
    n_fwd = sum(sq - c + sp for c in cnts) + 2 * sq
    transforms_ms = B * n * (n_fwd / fwd_rate + n_inv / inv_rate) * 1e3
    ip_bytes = 8 * n * (sq + sp) * (B * beta + 2 * beta + 2 * B)
    ip_bound_ms = ip_bytes / (HBM_PEAK_GBS * 1e9) * 1e3
    bound_ms = transforms_ms + ip_bound_ms
    ip = stages.get("inner_product")
    return {"bound": "valu (transforms) + hbm (inner product)", "bound_ms": bound_ms, "ms_per_step": step_ms,
            "frac": bound_ms / step_ms,
            "transforms_per_keyswitch": {"ntt": n_fwd, "intt": n_inv, "total": n_fwd + n_inv},
            "ntt_rate_coeffs_per_s": {"fwd": fwd_rate, "inv": inv_rate},
            "transforms_ms": transforms_ms,
            "inner_product": {"alg_bytes": ip_bytes, "bound_ms": ip_bound_ms, "ms": ip,
                              "achieved_gbs": ip_bytes / (ip * 1e-3) / 1e9 if ip else None,
                              "hbm_frac": ip_bytes / (ip * 1e-3) / 1e9 / HBM_PEAK_GBS if ip else None},
            "scope": f"batch {B} ciphertext polynomials, N=2^{n.bit_length() - 1}, Q={sq}, P={sp}, dnum={dnum}: "
                     "the transforms at the standalone NTT rate measured here plus the inner product at 8 TB/s, "
                     "over the measured time per step (base conversion and element passes not in the bound)"}


def bench_keyswitch_main(args):
    """--workload keyswitch: configs[4] as the main JSON line (with the stage split)."""
    import torch
    import torch.distributed as dist

    world, rank, local, dev = _dist_setup(args.dist_backend)
    import ofhe_hip as H

    ctx = H.Context(local)
    out = bench_keyswitch(args, ctx, world, rank, dev, steps=args.steps, warmup=args.warmup, with_stages=True)
    status = capi_status({"keyswitch": out.get("evalkey_broadcast")}, world)
    if rank == 0:
        out.update({"n_gpus": world, "higher_is_better": True, "vs_baseline": None, "dtype": "u64",
                    "data": "synthetic: splitmix64 ciphertext and key residues (SURVEY.md §8(d) seeds)",
                    "evalkey_broadcast_capi": status})
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    return capi_exit_code(status, args.require_capi_comm)


def bench_extra_main(args):
    """--workload rescale | bv_keyswitch: one of the round-2 callers outside
    SURVEY.md §8's rows as its own JSON line (not part of the default run)."""
    import torch.distributed as dist

    world, rank, local, dev = _dist_setup(args.dist_backend)
    import ofhe_hip as H

    ctx = H.Context(local)
    if args.workload == "rescale":
        out = bench_rescale(args, ctx, world, rank, dev, steps=args.steps, warmup=args.warmup)
    else:
        out = bench_bv(args, ctx, world, rank, dev, steps=args.steps, warmup=args.warmup)
    if rank == 0:
        out.update({"metric": out["workload"], "n_gpus": world, "higher_is_better": True, "vs_baseline": None,
                    "dtype": "u64", "data": "synthetic: splitmix64 residues (SURVEY.md §8(d) seeds)"})
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    return 0


# ---------------------------------------------------------------------------
# configs[0]: CPU-only poly benchmark, N = 2^14, 2 towers, POLY_NUM = 2
# ---------------------------------------------------------------------------
def bench_configs0(ctx):
    """DCRT_add / DCRT_mul of two evaluation-form DCRTPolys (poly-benchmark-16k.cpp:
    195-222: c = a->Plus(*b), c = a->Times(*b)), N = 2^14, 2 towers, on the CPU
    oracle (one thread, as the reference's benchmark loop runs) and, for
    comparison, one launch of the backend's ModAdd / ModMul on the GPU."""
    import numpy as np
    import torch

    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import oracle as O

    import ofhe_hip as H

    log_n, T = 14, 2
    n = 1 << log_n
    q, r = moduli_chain(log_n, T)
    a, b = O.uniform_dcrt(1, T, n, q, 1), O.uniform_dcrt(1, T, n, q, 2)

    def per_op(fn, budget=0.5):
        fn()
        k, t0 = 0, time.perf_counter()
        while time.perf_counter() - t0 < budget:
            fn()
            k += 1
        return (time.perf_counter() - t0) / k * 1e6

    threads = int(O.lib().oracle_num_threads())
    O.lib().oracle_set_threads(1)
    try:
        cpu = {"dcrt_add_us": per_op(lambda: O.eltwise("add", a, b, q)),
               "dcrt_mul_us": per_op(lambda: O.eltwise("mul", a, b, q))}
    finally:
        O.lib().oracle_set_threads(threads)
    plan = H.NTTPlan(ctx, log_n, q, r)
    da = torch.from_numpy(a.view(np.int64)).cuda()
    db = torch.from_numpy(b.view(np.int64)).cuda()
    dc = torch.empty_like(da)
    s = torch.cuda.current_stream()
    gpu = {}
    for name, fn in (("dcrt_add_us", plan.mod_add), ("dcrt_mul_us", plan.mod_mul)):
        fn(da.data_ptr(), db.data_ptr(), dc.data_ptr(), 1, s.cuda_stream)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        for _ in range(50):
            fn(da.data_ptr(), db.data_ptr(), dc.data_ptr(), 1, s.cuda_stream)
        e1.record(s)
        e1.synchronize()
        gpu[name] = e0.elapsed_time(e1) / 50 * 1e3
    ok = bool(np.array_equal(dc.cpu().numpy().view(np.uint64), O.eltwise("mul", a, b, q)))
    plan.close()
    return {"workload": "configs[0]: N=2^14, towers=2, POLY_NUM=2, DCRT_add / DCRT_mul (evaluation form), "
                        "poly-benchmark-16k.cpp:195-222 semantics",
            "cpu_port_1thread": cpu, "gpu_one_launch": gpu, "gpu_matches_oracle": ok,
            "note": "CPU = the oracle's restatement (oracle/ofhe_oracle.c), the reference being unbuildable here; "
                    "GPU figures are single launches of 2^15 words, launch-latency bound"}


# ---------------------------------------------------------------------------
# CPU baseline: the oracle on the host cores (a bounded sample)
# ---------------------------------------------------------------------------
def host_cpu():
    """(physical cores available to this process, CPU model) from lscpu."""
    model, cores_per_socket, sockets, tpc = None, None, None, 1
    try:
        out = subprocess.run(["lscpu"], capture_output=True, text=True, timeout=10).stdout
        for line in out.splitlines():
            k, _, v = line.partition(":")
            v = v.strip()
            if k.strip() == "Model name":
                model = v
            elif k.strip() == "Core(s) per socket":
                cores_per_socket = int(v)
            elif k.strip() == "Socket(s)":
                sockets = int(v)
            elif k.strip() == "Thread(s) per core":
                tpc = int(v)
    except Exception:  # noqa: BLE001
        pass
    avail = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    phys = cores_per_socket * sockets if cores_per_socket and sockets else avail
    cap = int(os.environ.get("OMP_NUM_THREADS", "0") or 0) or avail
    # one thread per physical core among the CPUs this process may use, within OMP_NUM_THREADS
    cores = max(1, min(cap, avail // max(1, tpc), phys))
    return cores, model, phys, tpc, avail


def cpu_baseline(args, qs, roots, log_n, T):
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import oracle as O

    n = 1 << log_n
    cores, model, phys, tpc, avail = host_cpu()
    tbs = O.Tables(n, qs, roots)
    # single thread, one polynomial of all towers (the reference's 41.1 ms figure)
    O.lib().oracle_set_threads(1)
    a1, b1 = O.uniform_dcrt(1, T, n, qs, 1), O.uniform_dcrt(1, T, n, qs, 2)
    O.ntt_mul_intt(a1, b1, tbs)
    best = 1e9
    for _ in range(9):  # best of 9: the host is shared
        t0 = time.perf_counter()
        O.ntt_mul_intt(a1, b1, tbs)
        best = min(best, time.perf_counter() - t0)
    one_ms = best * 1e3
    # all physical cores, OpenMP over batch x towers
    O.lib().oracle_set_threads(cores)
    Bs = 4
    ca, cb = O.uniform_dcrt(Bs, T, n, qs, 1), O.uniform_dcrt(Bs, T, n, qs, 2)
    O.ntt_mul_intt(ca, cb, tbs)
    runs, t0 = 0, time.perf_counter()
    while True:
        O.ntt_mul_intt(ca, cb, tbs)
        runs += 1
        el = time.perf_counter() - t0
        if el >= args.cpu_seconds:
            break
    return {"value": runs * Bs * T * n / el, "unit": "coeffs/s", "cores": cores, "kind": "port",
            "sample": f"{runs} runs x {Bs} polys x {T} towers x N=2^{log_n} ({el:.1f} s), "
                      f"oracle/ofhe_oracle.c, OpenMP over batch x towers on {cores} threads",
            "cpu_model": model, "physical_cores_reported": phys, "threads_per_core": tpc,
            "threads_note": f"{cores} threads: one per physical core of the {avail} logical CPUs in this "
                            f"process's affinity ({tpc} per core), within OMP_NUM_THREADS "
                            f"{os.environ.get('OMP_NUM_THREADS', 'unset')}; the host has {phys} physical cores",
            "host": socket.gethostname(),
            "single_thread_ms_per_poly": one_ms, "single_thread_coeffs_per_s": T * n / (one_ms * 1e-3),
            "reference_single_thread_ms_per_poly": REF_CPU_MS_1T,
            "port_vs_reference_1thread": one_ms / REF_CPU_MS_1T,
            "note": "the reference's 41.1 ms (SURVEY.md §6) was measured on the survey container's 8-vCPU Xeon; "
                    "the port measures 39.9 ms (best of 40) on the same container type (DESIGN.md (d)); the "
                    "reference itself is unbuildable here (DESIGN.md (c)), so the port is what runs"}


# ---------------------------------------------------------------------------
# PCIe-inclusive rate (never `value`)
# ---------------------------------------------------------------------------
def pcie_inclusive(plan, bc, chunks, dev):
    """c = INTT(NTT(a) (.) b) with a, b in pinned host memory and c returned to
    it: chunk i's H2D, chunk i-1's pipeline and chunk i-2's D2H overlap on three
    streams over two device slots.  Returns coefficients/s over `chunks` chunks
    of `bc` polynomials."""
    import torch

    T, n = plan.towers, plan.n
    a = torch.empty((2 * bc, T, n), dtype=torch.int64, device=dev)
    b = torch.empty_like(a)
    c = torch.empty_like(a)
    ha, hb, hc = (torch.empty((bc, T, n), dtype=torch.int64, pin_memory=True) for _ in range(3))
    sp = torch.cuda.current_stream(dev).cuda_stream
    plan.fill_uniform(a.data_ptr(), bc, 1, 0, sp)
    plan.fill_uniform(b.data_ptr(), bc, 2, 0, sp)
    ha.copy_(a[:bc])
    hb.copy_(b[:bc])
    s_in, s_run, s_out = (torch.cuda.Stream(dev) for _ in range(3))
    ev = {k: [torch.cuda.Event() for _ in range(2)] for k in ("in", "run", "out")}
    for k in ev:
        for e in ev[k]:
            e.record(torch.cuda.current_stream(dev))

    def go():
        for i in range(chunks):
            sl = i % 2
            da, db, dc = a[sl * bc:(sl + 1) * bc], b[sl * bc:(sl + 1) * bc], c[sl * bc:(sl + 1) * bc]
            s_in.wait_event(ev["run"][sl])          # chunk i-2 no longer reads da, db
            with torch.cuda.stream(s_in):
                da.copy_(ha, non_blocking=True)
                db.copy_(hb, non_blocking=True)
            ev["in"][sl].record(s_in)
            s_run.wait_event(ev["in"][sl])
            s_run.wait_event(ev["out"][sl])         # chunk i-2's c has left the device
            plan.ntt_mul_intt(da.data_ptr(), db.data_ptr(), dc.data_ptr(), bc, s_run.cuda_stream)
            ev["run"][sl].record(s_run)
            s_out.wait_event(ev["run"][sl])
            with torch.cuda.stream(s_out):
                hc.copy_(dc, non_blocking=True)
            ev["out"][sl].record(s_out)
        torch.cuda.synchronize(dev)

    go()  # warm (first pinned transfers)
    t0 = time.perf_counter()
    go()
    el = time.perf_counter() - t0
    coeffs = chunks * bc * T * n
    del a, b, c
    torch.cuda.empty_cache()
    return {"value": coeffs / el, "unit": "coeffs/s", "chunk_batch": bc, "chunks": chunks,
            "pcie_bytes_per_coeff": 24, "pcie_gbs": coeffs * 24 / el / 1e9,
            "note": "a, b pinned host -> HBM, pipeline, c -> pinned host; 3 streams, double-buffered"}


if __name__ == "__main__":
    main()
