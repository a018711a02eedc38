"""The C++ layer of the bootstrap's building blocks (include/fhecore.hpp): KeyGenerator with a
Hamming weight, Evaluator::conj_split and conj_merge.  tests/cpp/test_bootstrap_ops.cpp compares
them word for word with the residues computed here from pyoracle's keygen_secret_sparse, conj_split
and conj_merge and checks the three C entries' error codes."""
import os
import subprocess

import numpy as np
import pytest

import pyoracle
import refs
from cpp_programs import binary, build

BIN = binary("test_bootstrap_ops")
LOG_N, L, K = 10, 4, 2  # fhe::Context::standard(10, 4, 2, 2) in the program


def test_cpp_bootstrap_ops_compiles():
    build()
    assert os.access(BIN, os.X_OK)


@pytest.mark.gpu
@pytest.mark.parametrize("seed,h,level", [(17, 28, 3), (18, 1024, 4)])
def test_cpp_bootstrap_ops_run_on_gpu(tmp_path, seed, h, level):
    if not os.access(BIN, os.X_OK):
        build()
    m = [int(q) for q in pyoracle.gen_moduli(LOG_N, L + K)]
    qs = m[:L]
    sk = pyoracle.keygen_secret_sparse(seed, h, m, LOG_N)
    rng = np.random.default_rng(seed)
    ct, cc = (np.stack([rng.integers(0, q, (2, 1 << LOG_N), dtype=np.uint64) for q in qs[:level]],
                       axis=1) for _ in range(2))
    re, im = pyoracle.conj_split(ct, cc, qs, level=level, ntt=refs.c_ntt())
    parts = [sk, ct, cc, re, im, pyoracle.conj_merge(ct, cc, qs, level=level, ntt=refs.c_ntt())]
    path = tmp_path / "case.bin"
    with open(path, "wb") as f:
        for p in parts:
            f.write(np.ascontiguousarray(np.asarray(p).astype(np.uint64)).astype("<u8").tobytes())
    r = subprocess.run([BIN, str(path), str(seed), str(h), str(level)], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "cpp bootstrap ops ok" in r.stdout
