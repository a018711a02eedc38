"""The C++ Evaluator (include/fhecore.hpp) below the top level: tests/cpp/test_levels.cpp chains two
mul_relin(rescale) calls and a rotation at fewer limbs and compares them with the C entry points
(fhe_mul_relin_level, fhe_rotate_level) inside the program."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "test_levels")


def _build():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "gpu-fhe_amd"), "cpptest"], check=True)


def test_cpp_levels_compiles():
    _build()
    assert os.access(BIN, os.X_OK)


@pytest.mark.gpu
def test_cpp_levels_runs_on_gpu():
    if not os.access(BIN, os.X_OK):
        _build()
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "cpp levels ok" in r.stdout
