"""Runs tests/cpp_adapter_errors/test_adapter_errors.cpp on the GPU: every refusal of the C++ adapter
(upmem--openfhe_amd/host/ofhe_dcrt.hpp, and hooks::converter / hooks::PutEvalKey) -- exception class, what() and,
where two checks could refuse a call, the one that wins -- is byte for byte tests/golden/adapter_messages.txt,
recorded from the headers before their rules were given one owner each."""
import os
import subprocess

import pytest
from conftest import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden", "adapter_messages.txt")


@pytest.fixture(scope="module")
def errors_bin():
    d = os.path.join(ROOT, "tests", "cpp_adapter_errors")
    subprocess.run(["make", "-s", "-C", d], check=True)
    return os.path.join(d, "test_adapter_errors_bin")


def test_cpp_adapter_errors_builds(errors_bin):
    """The program compiles against both headers (no device needed), and the golden file is one line per case:
    name, class, what(), none of them a case that did not throw."""
    assert os.access(errors_bin, os.X_OK)
    with open(GOLDEN, "rb") as f:
        lines = f.read().decode().splitlines()
    assert len(lines) > 300
    assert len({ln.split("\t")[0] for ln in lines}) == len(lines), "case names are unique"
    for ln in lines:
        name, cls, what = ln.split("\t")
        assert cls in ("math_error", "not_implemented_error", "deserialize_error"), ln
        assert name and what, ln


@pytest.mark.gpu
def test_cpp_adapter_errors(errors_bin):
    r = subprocess.run([errors_bin], capture_output=True, timeout=120)
    with open(GOLDEN, "rb") as f:
        want = f.read()
    if r.stdout != want:
        got, exp = r.stdout.decode(errors="replace").splitlines(), want.decode().splitlines()
        for g, e in zip(got, exp):
            if g != e:
                print("got     ", g)
                print("expected", e)
        print(len(got), "lines, expected", len(exp))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout == want
