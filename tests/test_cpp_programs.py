"""The C++ test programs that need no case file: each compiles against the C ABI and, on a GPU, runs
its own checks and prints its ok line."""
import os
import subprocess

import pytest

from cpp_programs import binary, build

PROGRAMS = [
    # The header-only C++ Context/Ciphertext/Evaluator (include/fhecore.hpp) compiles against the C
    # ABI and, on a GPU, multiplies ciphertexts bit-exactly (checked inside the program against a
    # schoolbook negacyclic product).
    ("test_fhecore", "cpp api ok"),
    # The C++ Evaluator below the top level: tests/cpp/test_levels.cpp chains two mul_relin(rescale)
    # calls and a rotation at fewer limbs and compares them with the C entry points
    # (fhe_mul_relin_level, fhe_rotate_level) inside the program.
    ("test_levels", "cpp levels ok"),
    # The C++ Evaluator's plaintext arithmetic: tests/cpp/test_plain.cpp runs lincomb (mixed levels,
    # constant, rescale), mul_plain and drop_level and compares them with the C entry points
    # (fhe_lincomb_level, fhe_mul_plain_level) inside the program.
    ("test_plain", "cpp plain ok"),
    # The C++ Evaluator hoisting below the top level: tests/cpp/test_level_hoist.cpp brings a
    # ciphertext two limbs below L, runs rotate_hoisted and rotate_sum there with the top-level keys
    # and plaintexts and compares them with the C entry points (fhe_rotate_hoisted_level,
    # fhe_rotate_sum_hoisted_level) inside the program.
    ("test_level_hoist", "cpp level hoist ok"),
    # The C++ Evaluator's sum of products with one relinearisation: tests/cpp/test_mulsum.cpp runs
    # mul_sum_relin (mixed levels, a square, a shared operand, rescale on and off) and compares it
    # with the C entry point (fhe_mul_sum_relin_level) and, for one term, with Evaluator::mul_relin
    # inside the program.
    ("test_mulsum", "cpp mulsum ok"),
    # The C++ Evaluator's batched encryption: tests/cpp/test_encrypt.cpp runs the encrypt /
    # encrypt_sk overloads with a level and a batch and encrypt_slots, and compares them with the C
    # entry points (fhe_encrypt_level, fhe_encrypt_sk_level, fhe_encrypt_slots), with
    # Evaluator::encrypt for one top-level ciphertext and with encode then encrypt inside the
    # program.
    ("test_encrypt", "cpp encrypt ok"),
]


@pytest.mark.parametrize("name,ok", PROGRAMS)
def test_cpp_program_compiles(name, ok):
    build()
    assert os.access(binary(name), os.X_OK)


@pytest.mark.gpu
@pytest.mark.parametrize("name,ok", PROGRAMS)
def test_cpp_program_runs_on_gpu(name, ok):
    if not os.access(binary(name), os.X_OK):
        build()
    r = subprocess.run([binary(name)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert ok in r.stdout
