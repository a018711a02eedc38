"""The device encoder's reference (tests/encode_ref.py) without a GPU: against the host
fhecore.ckks.Encoder and a long-double direct sum, its round trip, the exact rounding cases, the
root table the library uploads (fhe_encode_roots) against math.cos / math.sin bit for bit, and the
C entry points' host-side refusals."""
import ctypes
import math

import numpy as np
import pytest

import encode_ref
import pyoracle
from fhecore import ckks

DELTA = 2.0 ** 50


def unit_square(n, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n)


def direct_sum(z, log_n):
    """delta m_k of the canonical embedding in long double, before rounding (float128 [N])."""
    n = 1 << log_n
    enc = ckks.Encoder(n)
    ld = np.longdouble
    ang = np.arange(2 * n).astype(ld) * (ld(np.pi) + ld(1.2246467991473532e-16)) / ld(n)
    cos, sin = np.cos(ang), np.sin(ang)
    idx = (enc.pos[:, None] * np.arange(n)[None, :]) % (2 * n)
    zr, zi = z.real.astype(ld)[:, None], z.imag.astype(ld)[:, None]
    return (zr * cos[idx] + zi * sin[idx]).sum(axis=0) * (ld(2.0) / ld(n)) * ld(DELTA)


@pytest.mark.parametrize("log_n", [10, 11])
def test_reference_against_the_host_encoder(log_n):
    """Every coefficient within 2 of Encoder.encode (each is the rounding of a value within float
    error of the exact one), and the reference's worst distance from a long-double direct sum at
    most twice the host encoder's."""
    n = 1 << log_n
    z = unit_square(n // 2, seed=log_n)
    host = ckks.Encoder(n).encode(z, DELTA)
    ref = encode_ref.encode_coeffs(z, DELTA, log_n)
    diff = int(np.abs(ref - host).max())
    exact = direct_sum(z, log_n)
    e_ref = float(np.abs(ref.astype(np.longdouble) - exact).max())
    e_host = float(np.abs(host.astype(np.longdouble) - exact).max())
    print(f"log_n {log_n}: |ref - host| <= {diff}; vs long double: ref {e_ref:.3f}, "
          f"host {e_host:.3f}")
    assert diff <= 2
    assert e_ref <= 2 * e_host


@pytest.mark.parametrize("log_n", [10, 11])
def test_round_trip(log_n):
    n = 1 << log_n
    z = unit_square(n // 2, seed=20 + log_n)
    enc = ckks.Encoder(n)
    e_host = np.abs(enc.decode(enc.encode(z, DELTA), DELTA) - z).max()
    c = encode_ref.encode_coeffs(z, DELTA, log_n)
    e_ref = np.abs(encode_ref.decode_coeffs(c.astype(np.float64), DELTA, log_n) - z).max()
    print(f"log_n {log_n}: round trip ref {e_ref:.3e}, host {e_host:.3e}")
    assert e_ref <= 2 * e_host
    # and through the residues: two limbs carry the coefficients exactly
    qs = [int(q) for q in pyoracle.gen_moduli(log_n, 3)]
    pt = encode_ref.encode(z, DELTA, log_n, qs)
    for level in (1, 2, 3):
        assert (encode_ref.centred(pt, qs, level) == c.astype(object)).all()
        back = encode_ref.decode(pt, DELTA, log_n, qs, level)
        assert np.abs(back - z).max() == e_ref


def test_exact_cases():
    log_n = 10
    n = 1 << log_n
    assert not encode_ref.encode_coeffs(np.zeros(n // 2), DELTA, log_n).any()
    # constant slots (2k + 1) / 2^51 give coefficient 0 = k + 1/2 exactly: ties go to even
    for k in (0, 1, 2, 3, 1000, 1001):
        for sign in (1, -1):
            v = sign * (2 * k + 1) / 2.0 ** 51
            c = encode_ref.encode_coeffs(np.full(n // 2, v, dtype=np.complex128), DELTA, log_n)
            want = sign * (k if k % 2 == 0 else k + 1)
            assert c[0] == want, (k, sign, c[0])
            assert not c[1:].any()


@pytest.mark.parametrize("log_n", [10, 17])
def test_root_table_is_libm_bit_for_bit(log_n):
    import fhecore

    n = 1 << log_n
    got = fhecore.encode_roots(log_n)
    assert got.shape == (2 * n, 2) and got.dtype == np.float64
    want = np.array([(math.cos(math.pi * k / n), math.sin(math.pi * k / n)) for k in range(2 * n)])
    assert (got.view(np.uint64) == want.view(np.uint64)).all()
    wc, ws = encode_ref.roots(log_n)
    assert (wc.view(np.uint64) == got[:, 0].view(np.uint64)).all()
    assert (ws.view(np.uint64) == got[:, 1].view(np.uint64)).all()


def test_surface_and_host_side_refusals():
    from fhecore import _capi

    for name in ("fhe_encode_roots", "fhe_encode_workspace", "fhe_encode", "fhe_decode_workspace",
                 "fhe_decode"):
        assert name in _capi.SIGNATURES
        assert hasattr(_capi.load(), name)
    lib = _capi.load()
    buf = (ctypes.c_uint64 * 8)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.fhe_encode_workspace(None, 1) == 0 and lib.fhe_decode_workspace(None, 1) == 0
    assert lib.fhe_encode(None, p, p, DELTA, 1, 0, 1, None, None) == -1
    assert b"null context" in lib.fhe_last_error()
    assert lib.fhe_decode(None, p, p, DELTA, 1, 1, 1, None, None) == -1
    assert b"null context" in lib.fhe_last_error()
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert lib.fhe_encode(None, p, p, bad, 1, 0, 1, None, None) == -1
        assert b"delta" in lib.fhe_last_error()
        assert lib.fhe_decode(None, p, p, bad, 1, 1, 1, None, None) == -1
        assert b"delta" in lib.fhe_last_error()
    assert lib.fhe_encode_roots(9, p) == -4 and lib.fhe_encode_roots(18, p) == -4
    assert lib.fhe_encode_roots(10, None) == -1
