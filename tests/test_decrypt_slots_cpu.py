"""fhe_decrypt_slots without a GPU: the C surface and its first host-side refusal, and the
reference composition the GPU tests compare with (tests/encrypt_ref.py decrypt, then
tests/encode_ref.py / sparse_pack_ref.py decode) bringing back the slots of a reference
encryption."""
import ctypes
import os
import re

import numpy as np
import pytest

import encode_ref
import encrypt_ref
import pyoracle
import sparse_pack_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOG_N, L = 10, 3
N = 1 << LOG_N
ALLM = [int(q) for q in pyoracle.gen_moduli(LOG_N, L + 1)]
QS = ALLM[:L]
SEED = 0x1234_5678_9ABC_DEF0
D50 = 2.0 ** 50


def test_header_declares_and_library_exports():
    from fhecore import _capi

    header = open(os.path.join(ROOT, "include", "fhecore.h")).read()
    m = re.search(r"\bint fhe_decrypt_slots\(([^;]*)\);", header)
    assert m, "include/fhecore.h does not declare fhe_decrypt_slots"
    args = [a.strip() for a in " ".join(m.group(1).split()).split(",")]
    assert args == ["const fhe_ctx* ctx", "double* slots", "const uint64_t* ct",
                    "const uint64_t* sk", "double delta", "uint32_t log_slots", "uint32_t level",
                    "uint32_t batch", "void* workspace", "fhe_stream_t stream"]
    assert "fhe_decrypt_slots" in _capi.SIGNATURES
    assert hasattr(_capi.load(), "fhe_decrypt_slots")


def test_null_context_is_refused_by_name():
    from fhecore import _capi

    lib = _capi.load()
    buf = (ctypes.c_uint64 * 8)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.fhe_decrypt_slots(None, p, p, p, D50, 9, 1, 1, None, None) == -1
    err = lib.fhe_last_error()
    assert b"fhe_decrypt_slots" in err and b"null context" in err
    assert not any(buf)


@pytest.mark.parametrize("secret", [False, True])
def test_reference_composition_brings_the_slots_back(secret):
    """A fresh encryption's slot error is about sqrt(N) sigma / delta ~ 3e-12 at delta = 2^50;
    2^-30 is a wide sanity bound on the reference itself, at full packing and at 8 slots, at
    levels 1, 2 and L."""
    sk = pyoracle.keygen_secret(11, ALLM, LOG_N).astype(np.uint64)
    key = sk if secret else pyoracle.keygen_public(12, sk, QS, LOG_N).astype(np.uint64)
    enc = encrypt_ref.encrypt_sk if secret else encrypt_ref.encrypt
    rng = np.random.default_rng(7)
    for ls in (LOG_N - 1, 3):
        z = rng.uniform(-1, 1, (2, 1 << ls)) + 1j * rng.uniform(-1, 1, (2, 1 << ls))
        pt = sparse_pack_ref.encode(z, D50, LOG_N, ls, QS)
        for level in (1, 2, L):
            ct = enc(SEED, pt, key, QS, LOG_N, level=level, batch=2, index0=3)
            dec = encrypt_ref.decrypt(ct, sk, QS)[..., :level, :]
            back = sparse_pack_ref.decode(dec, D50, LOG_N, ls, QS, level)
            if ls == LOG_N - 1:
                full = encode_ref.decode(dec, D50, LOG_N, QS, level)
                assert (full.view(np.uint64) == back.view(np.uint64)).all()
            err = float(np.abs(back - z).max())
            print(f"secret={secret} log_slots {ls} level {level}: |decode - z| <= {err:.3e}")
            assert back.shape == z.shape and err < 2.0 ** -30
