"""The C++ Evaluator's batched encryption (include/fhecore.hpp): tests/cpp/test_encrypt.cpp runs
the encrypt / encrypt_sk overloads with a level and a batch and encrypt_slots, and compares them
with the C entry points (fhe_encrypt_level, fhe_encrypt_sk_level, fhe_encrypt_slots), with
Evaluator::encrypt for one top-level ciphertext and with encode then encrypt inside the program."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "test_encrypt")


def _build():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "gpu-fhe_amd"), "cpptest"], check=True)


def test_cpp_encrypt_compiles():
    _build()
    assert os.access(BIN, os.X_OK)


@pytest.mark.gpu
def test_cpp_encrypt_runs_on_gpu():
    if not os.access(BIN, os.X_OK):
        _build()
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "cpp encrypt ok" in r.stdout
