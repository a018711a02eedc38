"""The C++ Evaluator's sparse encode / decode overloads (include/fhecore.hpp):
tests/cpp/test_sparse_pack.cpp encodes the slots this file wrote, decodes the result, and compares
both word for word with what tests/sparse_pack_ref.py computes here."""
import os
import subprocess

import numpy as np
import pytest

import encode_ref
import pyoracle
import sparse_pack_ref as sp
from cpp_programs import binary, build

BIN = binary("test_sparse_pack")
LOG_N, L, K = 10, 4, 2  # fhe::Context::standard(10, 4, 2, 2) in the program
DELTA = 2.0 ** 50


def test_cpp_sparse_pack_compiles():
    build()
    assert os.access(BIN, os.X_OK)


@pytest.mark.gpu
@pytest.mark.parametrize("ls,level,special", [(5, L, 1), (0, 2, 0), (8, 1, 0), (9, L, 0)])
def test_cpp_sparse_pack_runs_on_gpu(tmp_path, ls, level, special):
    if not os.access(BIN, os.X_OK):
        build()
    allm = [int(q) for q in pyoracle.gen_moduli(LOG_N, L + K)]
    qs = [allm[i] for i in encode_ref.rows_limbs(level, bool(special), L, K)]
    rng = np.random.default_rng(31 + ls)
    z = rng.uniform(-1, 1, 1 << ls) + 1j * rng.uniform(-1, 1, 1 << ls)
    want = sp.encode(z, DELTA, LOG_N, ls, qs)
    back = sp.decode(want, DELTA, LOG_N, ls, qs, level)
    path = tmp_path / "case.bin"
    with open(path, "wb") as f:
        f.write(np.ascontiguousarray(z).view(np.float64).astype("<f8").tobytes())
        f.write(np.ascontiguousarray(want).astype("<u8").tobytes())
        f.write(np.ascontiguousarray(back).view(np.float64).astype("<f8").tobytes())
    r = subprocess.run([BIN, str(path), str(ls), str(level), str(special)], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "cpp sparse pack ok" in r.stdout
