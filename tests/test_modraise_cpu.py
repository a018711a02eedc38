"""ModRaise without a GPU: the C entry points exist and refuse a null context, the reference
(pyoracle.mod_raise) is checked against its own definition through the CRT, and the identity a
bootstrap relies on -- the raised ciphertext decrypts to m + q_0 I with a small integer polynomial
I -- holds on the reference under a real key."""
import random

import numpy as np

import coracle
import pyoracle
import refs

LOG_N = 10
N = 1 << LOG_N
NTT = refs.c_ntt()


def chains():
    """A 60-bit chain, and a 60-bit q_0 over 50-bit primes (q_l < q_0 / 2: the lift must reduce)."""
    uni = [int(q) for q in pyoracle.gen_moduli(LOG_N, 4)]
    mixed = uni[:1] + [int(q) for q in pyoracle.gen_moduli(LOG_N, 3, bits=50)]
    return [uni, mixed]


def test_surface():
    from fhecore import _capi

    for name in ("fhe_mod_raise_workspace", "fhe_mod_raise"):
        assert name in _capi.SIGNATURES
        assert hasattr(_capi.load(), name)


def test_mod_raise_refuses_a_null_context_and_bad_arguments():
    import ctypes

    from fhecore import _capi

    lib = _capi.load()
    buf = (ctypes.c_uint64 * 8)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.fhe_mod_raise_workspace(None, 1) == 0
    assert lib.fhe_mod_raise(None, p, p, 1, 1, 1, None, None) == -1
    assert b"null context" in lib.fhe_last_error()
    # whatever else is wrong with the call, a null context never gets past the entry point
    for in_level, out_level, batch in [(0, 1, 1), (1, 0, 1), (1 << 20, 1, 1), (1, 1 << 20, 1),
                                       (1, 1, 0)]:
        assert lib.fhe_mod_raise(None, None, None, in_level, out_level, batch, None, None) == -1


def test_reference_against_its_definition():
    rng = np.random.default_rng(17)
    for qs in chains():
        q0 = qs[0]
        for in_level in (1, len(qs)):
            ct = np.stack([rng.integers(0, q, (2, N), dtype=np.uint64) for q in qs[:in_level]],
                          axis=1)  # (2, in_level, N)
            for out_level in (1, 2, len(qs)):
                ql = qs[:out_level]
                out = pyoracle.mod_raise(ct, qs, in_level, out_level, ntt=NTT)
                assert out.shape == (2, out_level, N)
                assert (out[:, 0] == ct[:, 0].astype(object)).all()
                assert all((out[:, l] < ql[l]).all() and (out[:, l] >= 0).all()
                           for l in range(out_level))
                # across its limbs the result is one integer polynomial: the centred lift
                c = pyoracle.centred_lift(ct, qs, NTT)
                assert (abs(c) <= (q0 - 1) // 2).all()
                coef = coracle.ntt_inv(out.astype(np.uint64), ql)
                for h in range(2):
                    if out_level > 1:
                        assert (pyoracle.crt_centered(coef[h], ql) == c[h]).all()
                    assert (coef[h, 0].astype(object) == c[h] % q0).all()


def test_boundary_coefficients():
    """0, 1, h, h + 1, q_0 - 1 with h = (q_0 - 1) / 2: h stays, h + 1 becomes -h."""
    for qs in chains():
        q0 = qs[0]
        h = (q0 - 1) // 2
        vals = [0, 1, h, h + 1, q0 - 1]
        x = np.array([vals[i % 5] for i in range(N)], dtype=np.uint64)
        ct = coracle.ntt_fwd(np.stack([x, x[::-1].copy()])[:, None, :], [q0])
        c = pyoracle.centred_lift(ct, qs, NTT)
        want = {0: 0, 1: 1, h: h, h + 1: -h, q0 - 1: -1}
        assert all(c[0, i] == want[vals[i % 5]] for i in range(N))
        out = pyoracle.mod_raise(ct, qs, 1, len(qs), ntt=NTT)
        coef = coracle.ntt_inv(out.astype(np.uint64), qs)
        for l, q in enumerate(qs):
            assert all(int(coef[0, l, i]) == want[vals[i % 5]] % q for i in range(N))


def test_raised_ciphertext_decrypts_to_m_plus_q0_I():
    """Ternary secret s, encrypt_sk of a known plaintext, drop to level 1, raise to L, decrypt over
    all L limbs: the CRT-centred coefficients y satisfy y = m_1 (mod q_0) exactly, m_1 the centred
    level-1 decryption, and I = (y - m_1) / q_0 has |I| <= (||s||_1 + 2) / 2 coefficientwise: each
    coefficient of c_0 + c_1 s over the centred representatives is at most (q_0 / 2)(1 + ||s||_1),
    and |m_1| <= q_0 / 2."""
    for qs in chains():
        L, q0 = len(qs), qs[0]
        rng = random.Random(99)
        s = [rng.randrange(-1, 2) for _ in range(N)]
        s1 = sum(abs(v) for v in s)
        sk_ntt = pyoracle.rns_ntt_fwd(pyoracle._to_rns(s, qs), qs)
        m = [rng.randrange(-(1 << 40), (1 << 40) + 1) for _ in range(N)]
        pt = coracle.ntt_fwd(np.asarray(pyoracle._to_rns(m, qs), dtype=np.uint64), qs)
        ct = pyoracle.encrypt_sk(4242, pt, sk_ntt, qs, LOG_N)
        low = ct[:, :1]
        d1 = pyoracle.decrypt(low, sk_ntt, qs[:1])
        m1 = coracle.ntt_inv(np.asarray(d1, dtype=np.uint64), qs[:1])[0].astype(object)
        m1 = np.where(m1 > (q0 - 1) // 2, m1 - q0, m1)
        assert max(abs(a - b) for a, b in zip(m1, m)) <= 21  # the encryption error (eta = 21)
        up = pyoracle.mod_raise(low, qs, 1, L, ntt=NTT)
        dec = pyoracle.decrypt(up, sk_ntt, qs)
        y = pyoracle.crt_centered(coracle.ntt_inv(np.asarray(dec, dtype=np.uint64), qs), qs)
        assert ((y - m1) % q0 == 0).all()
        big_i = (y - m1) // q0
        bound = (s1 + 2) / 2
        assert (abs(big_i) <= bound).all()
        assert abs(big_i).max() >= 1  # the term EvalMod is there to remove
        print(f"max |I| = {abs(big_i).max()}, bound {bound}")
