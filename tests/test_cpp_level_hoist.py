"""The C++ Evaluator (include/fhecore.hpp) hoisting below the top level:
tests/cpp/test_level_hoist.cpp brings a ciphertext two limbs below L, runs rotate_hoisted and
rotate_sum there with the top-level keys and plaintexts and compares them with the C entry points
(fhe_rotate_hoisted_level, fhe_rotate_sum_hoisted_level) inside the program."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "test_level_hoist")


def _build():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "gpu-fhe_amd"), "cpptest"], check=True)


def test_cpp_level_hoist_compiles():
    _build()
    assert os.access(BIN, os.X_OK)


@pytest.mark.gpu
def test_cpp_level_hoist_runs_on_gpu():
    if not os.access(BIN, os.X_OK):
        _build()
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "cpp level hoist ok" in r.stdout
