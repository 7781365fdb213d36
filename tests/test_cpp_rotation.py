"""Runs tests/cpp_rotation/test_rotation.cpp on the GPU: the adapter's hoisted
rotations (KeySwitchHybrid::FastRotationPrecompute / FastRotation /
FastRotationExt in upmem--openfhe_amd/host/ofhe_dcrt.hpp) equal the
step-by-step composition of the C ABI calls they replace."""
import os
import subprocess

import pytest
from conftest import ROOT


@pytest.fixture(scope="module")
def rotation_bin():
    d = os.path.join(ROOT, "tests", "cpp_rotation")
    subprocess.run(["make", "-s", "-C", d], check=True)
    return os.path.join(d, "test_rotation_bin")


def test_cpp_rotation_builds(rotation_bin):
    """The adapter members compile against the header (no device needed)."""
    assert os.access(rotation_bin, os.X_OK)


@pytest.mark.gpu
def test_cpp_hoisted_rotations(rotation_bin):
    r = subprocess.run([rotation_bin], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "rotation: 0 failures" in r.stdout, r.stdout
