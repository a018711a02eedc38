"""The C++ Evaluator's ModRaise (include/fhecore.hpp): tests/cpp/test_modraise.cpp raises a
ciphertext this file wrote and compares it word for word with the residues computed here from
pyoracle.mod_raise."""
import os
import subprocess

import numpy as np
import pytest

import pyoracle
import refs
from cpp_programs import binary, build

BIN = binary("test_modraise")
LOG_N, L, K = 10, 4, 2  # fhe::Context::standard(10, 4, 2, 2) in the program


def test_cpp_modraise_compiles():
    build()
    assert os.access(BIN, os.X_OK)


@pytest.mark.gpu
@pytest.mark.parametrize("in_level,out_level", [(1, L), (3, 2)])
def test_cpp_modraise_runs_on_gpu(tmp_path, in_level, out_level):
    if not os.access(BIN, os.X_OK):
        build()
    qs = [int(q) for q in pyoracle.gen_moduli(LOG_N, L + K)][:L]
    rng = np.random.default_rng(23)
    ct = np.stack([rng.integers(0, q, (2, 1 << LOG_N), dtype=np.uint64) for q in qs[:in_level]],
                  axis=1)
    want = pyoracle.mod_raise(ct, qs, in_level, out_level, ntt=refs.c_ntt()).astype(np.uint64)
    path = tmp_path / "case.bin"
    with open(path, "wb") as f:
        f.write(np.ascontiguousarray(ct).astype("<u8").tobytes())
        f.write(np.ascontiguousarray(want).astype("<u8").tobytes())
    r = subprocess.run([BIN, str(path), str(in_level), str(out_level)], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "cpp modraise ok" in r.stdout
