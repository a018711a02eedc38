"""The C++ Evaluator's encode / decode (include/fhecore.hpp): tests/cpp/test_encode.cpp encodes
the slots this file wrote, decodes the result, and compares both word for word with what
tests/encode_ref.py computes here."""
import os
import subprocess

import numpy as np
import pytest

import encode_ref
import pyoracle
from cpp_programs import binary, build

BIN = binary("test_encode")
LOG_N, L, K = 10, 4, 2  # fhe::Context::standard(10, 4, 2, 2) in the program
DELTA = 2.0 ** 50


def test_cpp_encode_compiles():
    build()
    assert os.access(BIN, os.X_OK)


@pytest.mark.gpu
@pytest.mark.parametrize("level,special", [(L, 1), (2, 0), (1, 0)])
def test_cpp_encode_runs_on_gpu(tmp_path, level, special):
    if not os.access(BIN, os.X_OK):
        build()
    allm = [int(q) for q in pyoracle.gen_moduli(LOG_N, L + K)]
    qs = [allm[i] for i in encode_ref.rows_limbs(level, bool(special), L, K)]
    rng = np.random.default_rng(29)
    ns = 1 << (LOG_N - 1)
    z = rng.uniform(-1, 1, ns) + 1j * rng.uniform(-1, 1, ns)
    want = encode_ref.encode(z, DELTA, LOG_N, qs)
    back = encode_ref.decode(want, DELTA, LOG_N, qs, level)
    path = tmp_path / "case.bin"
    with open(path, "wb") as f:
        f.write(np.ascontiguousarray(z).view(np.float64).astype("<f8").tobytes())
        f.write(np.ascontiguousarray(want).astype("<u8").tobytes())
        f.write(np.ascontiguousarray(back).view(np.float64).astype("<f8").tobytes())
    r = subprocess.run([BIN, str(path), str(level), str(special)], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "cpp encode ok" in r.stdout
