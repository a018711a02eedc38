"""The C++ Evaluator's decrypt_slots (include/fhecore.hpp): tests/cpp/test_decrypt_slots.cpp
encrypts the slots this file wrote under a secret key it makes from a fixed seed, decrypts them
straight to slots, full and sparse, and compares word for word with what tests/encrypt_ref.py and
the decoders' references compute here from the same seeds."""
import os
import subprocess

import numpy as np
import pytest

import encode_ref
import encrypt_ref
import pyoracle
import sparse_pack_ref
from cpp_programs import binary, build

BIN = binary("test_decrypt_slots")
LOG_N, L, K = 10, 4, 2  # fhe::Context::standard(10, 4, 2, 2) in the program
LEVEL, INDEX0, SPARSE = 3, 5, 3
SK_SEED, SEED = 42, 0x1234567887654321
DELTA = 2.0 ** 50


def test_cpp_decrypt_slots_compiles():
    build()
    assert os.access(BIN, os.X_OK)


@pytest.mark.gpu
def test_cpp_decrypt_slots_runs_on_gpu(tmp_path):
    if not os.access(BIN, os.X_OK):
        build()
    allm = [int(q) for q in pyoracle.gen_moduli(LOG_N, L + K)]
    qs = allm[:L]
    sk = pyoracle.keygen_secret(SK_SEED, allm, LOG_N).astype(np.uint64)
    rng = np.random.default_rng(37)
    parts, wants = [], []
    for ls in (LOG_N - 1, SPARSE):
        z = rng.uniform(-1, 1, 1 << ls) + 1j * rng.uniform(-1, 1, 1 << ls)
        pt = sparse_pack_ref.encode(z, DELTA, LOG_N, ls, qs[:LEVEL])
        ct = encrypt_ref.encrypt_sk(SEED, pt, sk, qs, LOG_N, level=LEVEL, batch=1, index0=INDEX0)
        dec = encrypt_ref.decrypt(ct[0], sk, qs)
        if ls == LOG_N - 1:
            back = encode_ref.decode(dec, DELTA, LOG_N, qs, LEVEL)
        else:
            back = sparse_pack_ref.decode(dec, DELTA, LOG_N, ls, qs, LEVEL)
        assert np.abs(back - z).max() < 2.0 ** -30
        parts.append(z)
        wants.append(back)
    path = tmp_path / "case.bin"
    with open(path, "wb") as f:
        for a in parts + wants:
            f.write(np.ascontiguousarray(a).view(np.float64).astype("<f8").tobytes())
    r = subprocess.run([BIN, str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "cpp decrypt_slots ok" in r.stdout
