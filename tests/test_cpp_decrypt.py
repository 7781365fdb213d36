"""Runs tests/cpp_decrypt/test_decrypt.cpp on the GPU: the adapter's BFV
decryption (BfvDecrypt::ScaleAndRound, Decrypt and DCRTPolyHip::TimesQovert in
upmem--openfhe_amd/host/ofhe_dcrt.hpp) equals the direct C ABI calls on the same
device data, under the HPS family and BEHZ and on one tower, and an encryption
made with TimesQovert decrypts through the adapter."""
import os
import subprocess

import pytest
from conftest import ROOT


@pytest.fixture(scope="module")
def decrypt_bin():
    d = os.path.join(ROOT, "tests", "cpp_decrypt")
    subprocess.run(["make", "-s", "-C", d], check=True)
    return os.path.join(d, "test_decrypt_bin")


def test_cpp_decrypt_builds(decrypt_bin):
    """The adapter members compile against the header (no device needed)."""
    assert os.access(decrypt_bin, os.X_OK)


@pytest.mark.gpu
def test_cpp_decrypt(decrypt_bin):
    r = subprocess.run([decrypt_bin], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "decrypt: 0 failures" in r.stdout, r.stdout
