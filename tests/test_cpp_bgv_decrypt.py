"""Runs tests/cpp_bgv_decrypt/test_bgv_decrypt.cpp, one sub-test per run: the adapter's BGV decryption
(BgvDecrypt::ModReduceChain and Decrypt, BgvDecryptCache and the free DecryptCore in
upmem--openfhe_amd/host/ofhe_dcrt.hpp) equals the direct C ABI calls on the same device data at the full chain
and one level down, an encryption of a known plaintext decrypts through the adapter in both formats, the
argument rules throw, and ScalingFactor agrees with its definition (on the host alone)."""
import os
import subprocess

import pytest
from conftest import ROOT


@pytest.fixture(scope="module")
def bgv_decrypt_bin():
    d = os.path.join(ROOT, "tests", "cpp_bgv_decrypt")
    subprocess.run(["make", "-s", "-C", d], check=True)
    return os.path.join(d, "test_bgv_decrypt_bin")


def run(binary, sub):
    r = subprocess.run([binary, sub], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"bgv_decrypt {sub}: 0 failures" in r.stdout, r.stdout


def test_cpp_bgv_decrypt_builds(bgv_decrypt_bin):
    """The adapter members compile against the header (no device needed)."""
    assert os.access(bgv_decrypt_bin, os.X_OK)


def test_cpp_scaling_factor(bgv_decrypt_bin):
    """host arithmetic only"""
    run(bgv_decrypt_bin, "scaling")


@pytest.mark.gpu
@pytest.mark.parametrize("sub", ["chain", "decrypt", "core", "message", "errors"])
def test_cpp_bgv_decrypt(bgv_decrypt_bin, sub):
    run(bgv_decrypt_bin, sub)
