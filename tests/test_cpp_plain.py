"""The C++ Evaluator's plaintext arithmetic (include/fhecore.hpp): tests/cpp/test_plain.cpp runs
lincomb (mixed levels, constant, rescale), mul_plain and drop_level and compares them with the C
entry points (fhe_lincomb_level, fhe_mul_plain_level) inside the program."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "test_plain")


def _build():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "gpu-fhe_amd"), "cpptest"], check=True)


def test_cpp_plain_compiles():
    _build()
    assert os.access(BIN, os.X_OK)


@pytest.mark.gpu
def test_cpp_plain_runs_on_gpu():
    if not os.access(BIN, os.X_OK):
        _build()
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "cpp plain ok" in r.stdout
