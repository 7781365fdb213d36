"""Runs tests/cpp_bfv/test_bfv.cpp on the GPU: the adapter's BFV (HPS family)
multiplication (BaseConverter::SwitchCRTBasis, ExpandCRTBasis, ScaleAndRound,
BfvMult::EvalMult in upmem--openfhe_amd/host/ofhe_dcrt.hpp) equals the direct
C ABI calls on the same device data, and the reference's N = 8 known answer of
SwitchCRTBasis holds through the adapter."""
import os
import subprocess

import pytest
from conftest import ROOT


@pytest.fixture(scope="module")
def bfv_bin():
    d = os.path.join(ROOT, "tests", "cpp_bfv")
    subprocess.run(["make", "-s", "-C", d], check=True)
    return os.path.join(d, "test_bfv_bin")


def test_cpp_bfv_builds(bfv_bin):
    """The adapter members compile against the header (no device needed)."""
    assert os.access(bfv_bin, os.X_OK)


@pytest.mark.gpu
def test_cpp_bfv_mult(bfv_bin):
    r = subprocess.run([bfv_bin], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "bfv: 0 failures" in r.stdout, r.stdout
