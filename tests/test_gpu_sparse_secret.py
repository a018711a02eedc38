"""fhe_keygen_secret_sparse on the GPU (csrc/keygen.hip): the INTT of sk against
pyoracle.sparse_secret_coefficients bit for bit on every one of the L + K limbs, the refusals, and keygen_secret without the keyword
unchanged against pyoracle."""
import numpy as np
import pytest

import pyoracle

pytestmark = pytest.mark.gpu

SEEDS = (0x1234_5678_9ABC, 7)


@pytest.fixture(scope="module")
def fc():
    import fhecore

    return fhecore


@pytest.fixture(scope="module")
def ctxs(fc):
    return {10: fc.Context(10, L=3, K=2, dnum=3), 13: fc.Context(13, L=2, K=1, dnum=1)}


# log_n = 10: one coefficient per lane of the select; 13: eight
@pytest.mark.parametrize("log_n,h", [(10, 1), (10, 28), (10, 64), (10, 1023), (10, 1024),
                                     (13, 192)])
@pytest.mark.parametrize("seed", SEEDS)
def test_sparse_secret_matches_the_reference_on_every_limb(fc, ctxs, log_n, h, seed):
    ctx = ctxs[log_n]
    sk = ctx.keygen_secret(seed=seed, hamming_weight=h)
    assert tuple(sk.shape) == (ctx.L + ctx.K, 1 << log_n)
    coef = fc.to_host(ctx.intt(sk))
    want = pyoracle.sparse_secret_coefficients(seed, h, log_n)
    for limb, q in enumerate(ctx.all_moduli):
        assert (coef[limb] == (want % q).astype(np.uint64)).all(), limb
    assert np.count_nonzero(coef[0]) == h


def test_sparse_secret_ntt_form_matches_the_reference(fc, ctxs):
    ctx = ctxs[10]
    sk = fc.to_host(ctx.keygen_secret(seed=9, hamming_weight=28)).astype(object)
    assert (sk == pyoracle.keygen_secret_sparse(9, 28, ctx.all_moduli, 10)).all()


def test_bad_weights_are_refused(fc, ctxs):
    ctx = ctxs[10]
    for h in (0, ctx.n + 1):
        with pytest.raises(fc.FheError) as e:
            ctx.keygen_secret(seed=1, hamming_weight=h)
        assert "FHE_EINVAL" in str(e.value) and "Hamming weight" in str(e.value)
    lib = fc.load()
    assert lib.fhe_keygen_secret_sparse(ctx.handle, None, 28, 1, None) == -1


def test_keygen_secret_without_the_keyword_is_unchanged(fc, ctxs):
    ctx = ctxs[10]
    sk = fc.to_host(ctx.keygen_secret(11)).astype(object)
    assert (sk == pyoracle.keygen_secret(11, ctx.all_moduli, 10)).all()
    assert (fc.to_host(ctx.keygen_secret(seed=11, hamming_weight=None)).astype(object) == sk).all()
