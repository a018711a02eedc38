"""The C++ Evaluator's sum of products with one relinearisation (include/fhecore.hpp):
tests/cpp/test_mulsum.cpp runs mul_sum_relin (mixed levels, a square, a shared operand, rescale on
and off) and compares it with the C entry point (fhe_mul_sum_relin_level) and, for one term, with
Evaluator::mul_relin inside the program."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "test_mulsum")


def _build():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "gpu-fhe_amd"), "cpptest"], check=True)


def test_cpp_mulsum_compiles():
    _build()
    assert os.access(BIN, os.X_OK)


@pytest.mark.gpu
def test_cpp_mulsum_runs_on_gpu():
    if not os.access(BIN, os.X_OK):
        _build()
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "cpp mulsum ok" in r.stdout
