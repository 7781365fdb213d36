"""Runs tests/cpp_leveled/test_leveled.cpp: on the GPU, the adapter's HPSPOVERQLEVELED calls
(BfvLevel::EvalMult / EvalSquare / Relinearize / ScaleAndRoundExpand, BfvLevelCache and
DCRTPolyHip::ExpandCRTBasisQlHat in upmem--openfhe_amd/host/ofhe_dcrt.hpp) equal the same steps
through the earlier C ABI calls on the same device data, one sub-test per level; without a device,
the adapter's FindLevelsToDrop equals bfv_tables.levels_to_drop on a grid."""
import os
import subprocess

import pytest
from conftest import ROOT

import bfv_tables as BT


@pytest.fixture(scope="module")
def leveled_bin():
    d = os.path.join(ROOT, "tests", "cpp_leveled")
    subprocess.run(["make", "-s", "-C", d], check=True)
    return os.path.join(d, "test_leveled_bin")


def test_cpp_leveled_builds(leveled_bin):
    """The adapter members compile against the header (no device needed)."""
    assert os.access(leveled_bin, os.X_OK)


def test_levels_to_drop_python_and_cpp_agree(leveled_bin):
    """216 x 4 grid points: size_q, tower bits, ring size, plaintext modulus, HYBRID or BV noise,
    EvalMult or key-switch cushion, depth"""
    r = subprocess.run([leveled_bin, "levels"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = [line.split() for line in r.stdout.splitlines()]
    assert len(rows) == 3 * 3 * 3 * 2 * 2 * 2 * 4
    seen = set()
    for size_q, bits, log_n, t, hybrid, ks, depth, got in rows:
        want = BT.levels_to_drop(int(depth), int(size_q), float(bits), 1 << int(log_n), int(t), hybrid=hybrid == "1",
                                 num_per_part_q=2, num_part_q=3, key_switch=ks == "1")
        assert int(got) == want, (size_q, bits, log_n, t, hybrid, ks, depth, got, want)
        seen.add(want)
    assert len(seen) > 3  # the grid is not all clamped to one value


@pytest.mark.gpu
def test_cpp_leveled(leveled_bin):
    r = subprocess.run([leveled_bin], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "leveled: 0 failures" in r.stdout, r.stdout
