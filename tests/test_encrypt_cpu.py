"""Batched encryption without a GPU: the C surface and its host-side refusals, the vectorised
Philox of tests/encrypt_ref.py against pyoracle's, the reference against pyoracle.encrypt /
encrypt_sk, its level and index properties, and that what it encrypts decrypts."""
import ctypes

import numpy as np
import pytest

import encrypt_ref
import pyoracle

LOG_N, L = 10, 3
N = 1 << LOG_N
QS = [int(q) for q in pyoracle.gen_moduli(LOG_N, L + 1)]
ALLM, QS = QS, QS[:L]
SEED = 0x1234_5678_9ABC_DEF0
NAMES = ("fhe_encrypt_workspace", "fhe_encrypt_level", "fhe_encrypt_sk_level", "fhe_encrypt_slots")


@pytest.fixture(scope="module")
def keys():
    """(sk [L + 1, N], pk [2, L, N], pt [L, N]) as uint64, from pyoracle's key generation."""
    sk = pyoracle.keygen_secret(11, ALLM, LOG_N)
    pk = pyoracle.keygen_public(12, sk, QS, LOG_N)
    rng = np.random.default_rng(5)
    pt = np.stack([rng.integers(0, q, N, dtype=np.uint64) for q in QS])
    return sk.astype(np.uint64), pk.astype(np.uint64), pt


def test_surface_and_null_context():
    from fhecore import _capi

    lib = _capi.load()
    for name in NAMES:
        assert name in _capi.SIGNATURES
        assert hasattr(lib, name)
    buf = (ctypes.c_uint64 * 8)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.fhe_encrypt_workspace(None, 1, 1) == 0
    assert lib.fhe_encrypt_level(None, p, p, 1, 1, p, 1, 1, 7, 0, None, None) == -1
    assert b"null context" in lib.fhe_last_error()
    assert lib.fhe_encrypt_sk_level(None, p, p, 1, 1, p, 1, 1, 7, 0, None, None) == -1
    assert b"null context" in lib.fhe_last_error()
    assert lib.fhe_encrypt_slots(None, p, p, 2.0 ** 40, 9, p, 0, 1, 1, 7, 0, None, None) == -1
    assert b"null context" in lib.fhe_last_error()


def test_vectorised_philox_is_pyoracle_philox():
    rng = np.random.default_rng(1)
    c = rng.integers(0, 1 << 32, (4, 64), dtype=np.uint64)
    k0, k1 = 0x9E3779B9, 0xDEADBEEF
    got = encrypt_ref.philox(c[0], c[1], c[2], c[3], k0, k1)
    for i in range(64):
        want = pyoracle.philox4x32_10(tuple(int(c[r, i]) for r in range(4)), k0, k1)
        assert tuple(int(g[i]) for g in got) == want


@pytest.mark.parametrize("poly", [0, 5])
@pytest.mark.parametrize("kind", ["uniform", "ternary", "error"])
def test_vectorised_sample_is_pyoracle_sample(kind, poly):
    n = 256
    limbs = [(0, QS[0]), (2, QS[2]), (3, ALLM[3])]
    for tag in (32, 35):
        want = pyoracle.sample(kind, SEED, tag, poly, limbs, n)
        got = encrypt_ref.sample(kind, SEED, tag, poly, limbs, n)
        assert got.dtype == np.uint64 and (got.astype(object) == want).all()


def test_reference_at_the_top_level_is_pyoracle(keys):
    """Property (i) for the reference: element 0, index0 = 0, level L."""
    sk, pk, pt = keys
    want = pyoracle.encrypt(SEED, pt.astype(object), pk.astype(object), QS, LOG_N)
    got = encrypt_ref.encrypt(SEED, pt, pk, QS, LOG_N)
    assert (got[0].astype(object) == want).all()
    want = pyoracle.encrypt_sk(SEED, pt.astype(object), sk.astype(object), QS, LOG_N)
    got = encrypt_ref.encrypt_sk(SEED, pt, sk, QS, LOG_N)
    assert (got[0].astype(object) == want).all()


@pytest.mark.parametrize("secret", [False, True])
def test_reference_levels_and_indices(keys, secret):
    """Properties (ii) and (iii): level l is rows 0 .. l-1 of the level-L result; element i of a
    call with index0 = k is element 0 of a call with index0 = k + i."""
    sk, pk, pt = keys
    enc = (lambda **kw: encrypt_ref.encrypt_sk(SEED, pt, sk, QS, LOG_N, **kw)) if secret else \
        (lambda **kw: encrypt_ref.encrypt(SEED, pt, pk, QS, LOG_N, **kw))
    top = enc(batch=3, index0=5)
    for level in (1, 2):
        assert (enc(level=level, batch=3, index0=5) == top[:, :, :level]).all()
    for i in range(3):
        assert (enc(batch=1, index0=5 + i)[0] == top[i]).all()
    assert not (top[0] == top[1]).all()
    # pt = None encrypts zero, and a batched pt gives each ciphertext its own
    zero = np.zeros_like(pt)
    key = sk if secret else pk
    f = encrypt_ref.encrypt_sk if secret else encrypt_ref.encrypt
    assert (f(SEED, None, key, QS, LOG_N, batch=2) == f(SEED, zero, key, QS, LOG_N, batch=2)).all()
    two = np.stack([pt, zero])
    both = f(SEED, two, key, QS, LOG_N, batch=2)
    assert (both[0] == f(SEED, pt, key, QS, LOG_N)[0]).all()
    assert (both[1] == f(SEED, None, key, QS, LOG_N, batch=1, index0=1)[0]).all()


@pytest.mark.parametrize("secret", [False, True])
def test_reference_decrypts(keys, secret):
    """The centred limb-0 coefficients of decrypt(encrypt(pt)) - pt: within 21 (2N + 1) for the
    public-key form (e0 + e_pk u + e1 s, eta = 21, ternary u and s) and 21 for the secret-key form
    (e alone), at every level."""
    sk, pk, pt = keys
    f, key = (encrypt_ref.encrypt_sk, sk) if secret else (encrypt_ref.encrypt, pk)
    bound = encrypt_ref.noise_bound(LOG_N, secret)
    assert bound == (21 if secret else 21 * (2 * N + 1))
    for level in (1, L):
        ct = f(SEED, pt, key, QS, LOG_N, level=level, batch=2, index0=3)
        noise = encrypt_ref.noise_limb0(ct, pt[:level], sk, QS)
        worst = int(np.abs(noise).max())
        print(f"secret={secret} level {level}: |noise| <= {worst} (bound {bound})")
        assert 0 < worst <= bound
