"""Runs tests/cpp_behz/test_behz.cpp on the GPU: the adapter's BFV (BEHZ)
multiplication (BehzBasis::FastBaseConvqToBskMontgomery, FastRNSFloorq,
FastBaseConvSK, BfvMultBehz in upmem--openfhe_amd/host/ofhe_dcrt.hpp) equals
the direct C ABI calls on the same device data, and the reference's N = 8 known
answer of FastBaseConvqToBskMontgomery holds through the adapter."""
import os
import subprocess

import pytest
from conftest import ROOT


@pytest.fixture(scope="module")
def behz_bin():
    d = os.path.join(ROOT, "tests", "cpp_behz")
    subprocess.run(["make", "-s", "-C", d], check=True)
    return os.path.join(d, "test_behz_bin")


def test_cpp_behz_builds(behz_bin):
    """The adapter members compile against the header (no device needed)."""
    assert os.access(behz_bin, os.X_OK)


@pytest.mark.gpu
def test_cpp_behz_mult(behz_bin):
    r = subprocess.run([behz_bin], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "behz: 0 failures" in r.stdout, r.stdout
