"""bench.py's plain run on the GPU at a small shape: the result line carries
the headline figures and none of the --full legs, and --dump-outputs writes
what the timed path computed in its last step, the same from run to run,
checked here bit for bit against the oracle."""
import json
import os

import numpy as np
import pytest

gpu = pytest.mark.gpu

LOG_N, TOWERS, BATCH = 13, 3, 5  # column pass + block pass (log_n > 12), odd towers and batch


def _run(capsys, *extra):
    import bench

    args = bench.parse_args(["--gpus", "1", "--steps", "3", "--warmup", "1", "--log-n", str(LOG_N),
                             "--towers", str(TOWERS), "--batch", str(BATCH), *extra])
    capsys.readouterr()
    assert bench.bench_pipeline(args) == 0
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def _residues(d, name):
    lo, hi = np.load(os.path.join(d, name + "_lo32.npy")), np.load(os.path.join(d, name + "_hi32.npy"))
    assert lo.dtype == hi.dtype == np.float64
    return (hi.astype(np.uint64) << np.uint64(32)) | lo.astype(np.uint64)


@pytest.fixture(scope="module")
def want(O):
    import bench

    n = 1 << LOG_N
    qs, rs = bench.moduli_chain(LOG_N, TOWERS)
    a, b = O.uniform_dcrt(BATCH, TOWERS, n, qs, 1), O.uniform_dcrt(BATCH, TOWERS, n, qs, 2)
    return O.ntt_mul_intt(a, b, O.Tables(n, qs, rs))


@gpu
def test_plain_run_dumps_the_last_steps_output(hip, want, tmp_path, capsys):
    d1, d2 = str(tmp_path / "one"), str(tmp_path / "two")
    out = _run(capsys, "--dump-outputs", d1)
    n = 1 << LOG_N
    assert out["steps"] == 3 and out["warmup"] == 1 and out["full"] is False
    assert out["unit"] == "coeffs/s" and out["higher_is_better"] is True and out["dtype"] == "u64"
    assert out["ms_per_step"] > 0
    # value is the coefficients of one step over the time of one step
    assert abs(out["value"] - BATCH * TOWERS * n / (out["ms_per_step"] * 1e-3)) <= 1e-9 * out["value"]
    # none of the legs that take runs of their own
    assert out["roofline"] is None and out["kernels_ms"] == {} and out["parity_spot_check"] is None
    assert all(out[k] is None for k in ("cpu_baseline", "power", "secondary_ops", "configs3", "keyswitch",
                                        "configs0", "pcie_inclusive"))
    assert sorted(os.listdir(d1)) == ["c.npy", "c_hi32.npy", "c_lo32.npy"]
    assert out["outputs"]["c"] == {"shape": [BATCH, TOWERS, n], "dtype": "float64", "of_shape": [BATCH, TOWERS, n],
                                   "sampled": False}
    got = _residues(d1, "c")
    assert got.shape == want.shape and np.array_equal(got, want)
    c = np.load(os.path.join(d1, "c.npy"))
    assert c.dtype == np.float64 and np.array_equal(c, want.astype(np.float64))
    # the same arguments again: the same inputs, the same files
    _run(capsys, "--dump-outputs", d2)
    for f in os.listdir(d1):
        assert np.array_equal(np.load(os.path.join(d1, f)), np.load(os.path.join(d2, f))), f


@gpu
def test_a_large_output_is_dumped_as_its_fixed_sample(hip, want, tmp_path, capsys, monkeypatch):
    import bench

    monkeypatch.setattr(bench, "DUMP_MAX_WORDS", 1000)
    d = str(tmp_path / "s")
    out = _run(capsys, "--dump-outputs", d)
    assert out["outputs"]["c"]["sampled"] is True and out["outputs"]["c"]["shape"] == [1000]
    idx = bench.dump_sample_index(want.size)
    assert np.array_equal(_residues(d, "c"), want.reshape(-1)[idx])


@gpu
def test_full_run_adds_its_legs_after_the_dump(hip, want, tmp_path, capsys):
    """--full --no-extras: the per-kernel pass, the roofline and the oracle
    spot check run (on c, after it was written out) and reach the line."""
    d = str(tmp_path / "f")
    out = _run(capsys, "--full", "--no-extras", "--dump-outputs", d)
    assert out["full"] is True and out["parity_spot_check"] is True
    assert sorted(out["kernels_ms"]) == ["colpass<fwd>", "colpass<inv>", "k_block<fused>"]
    assert out["roofline"]["schema"] == 3 and out["roofline"]["ms_per_step"] == out["ms_per_step"]
    assert np.array_equal(_residues(d, "c"), want)
