"""fhecore.bootstrap.Bootstrapper on the GPU backend: the shared case of tests/cases.py (BOOTSTRAP) bit
for bit against the CPU backend, then the same slots under keys made on the device with a secret
of Hamming weight 28, from a ciphertext dropped to level 1, and a second bootstrap of the result."""
import numpy as np
import pytest

import bootstrap_ref as br
import cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fc():
    import fhecore

    return fhecore


@pytest.fixture(scope="module")
def ctx(fc):
    su = cases.setup(cases.BOOTSTRAP)
    c = fc.Context(br.LOG_N, moduli=su["qs"], special=su["ps"], dnum=br.DNUM)
    assert c.moduli == su["qs"] and c.special == su["ps"]
    return c


def u64(x):
    return np.asarray(x).astype(np.uint64)


def test_bootstrap_matches_the_cpu_backend_bit_for_bit(fc, ctx):
    """Both backends receive the same integers and the same float64 diagonals (fhe_encode is
    bit-exact against encode_ref), so data, level and scale are the same."""
    from fhecore import bootstrap as bs
    from fhecore.polyeval import Ct

    su = cases.setup(cases.BOOTSTRAP)
    d = lambda key: (fc.to_device(u64(key[0])), fc.to_device(u64(key[1])))  # noqa: E731
    be = bs.GpuBackend(ctx, relin_key=d(su["relin"]), rot_keys={k: d(v) for k, v in su["rot"].items()})
    boot = bs.Bootstrapper(be, **br.PARAMS)
    ct = fc.to_device(u64(np.asarray(su["ct"])[:, :1]))
    out = boot.bootstrap(Ct(ct, 1, br.DELTA))
    ref, err = cases.run_cpu(cases.BOOTSTRAP)
    assert (out.level, out.scale) == (ref.level, ref.scale)
    assert (fc.to_host(out.data) == u64(ref.data)).all()
    assert err < cases.MARGIN * cases.BOOTSTRAP_ERR


def test_bootstrap_under_device_keys(fc, ctx):
    """keygen_secret(hamming_weight=28), the rotation, conjugation and relinearisation keys and
    the encryption on the device.  The ciphertext dropped to level 1 comes back at level
    L - 3 - 9 - 3 = 3 and decodes to the input slots within 2 x BOOTSTRAP_ERR: the error is a
    maximum over 512 slots of a noise-dominated sum and varies between key draws, hence 2 and not
    the 1.05 of the bit-exact runs.  A second bootstrap of the result still decrypts (within the
    two errors added): the level and scale bookkeeping closes."""
    from fhecore import bootstrap as bs
    from fhecore.polyeval import Ct

    su = cases.setup(cases.BOOTSTRAP)
    sk = ctx.keygen_secret(seed=51, hamming_weight=br.HAMMING)
    be = bs.GpuBackend(ctx, sk=sk, seed=1000)
    boot = bs.Bootstrapper(be, **br.PARAMS)
    ct = ctx.encrypt_sk(fc.to_device(su["pt"]), sk, seed=52)
    low = ctx.drop_level(ct, 1)
    out = boot.bootstrap(Ct(low, 1, br.DELTA))
    assert sorted(be.rot_keys) == br.rotation_elements()  # every step's key and the conjugation's
    assert out.level == boot.out_level == br.OUT_LEVEL
    assert tuple(out.data.shape) == (2, br.OUT_LEVEL, 1 << br.LOG_N)

    def slots(c):
        return cases.decode(cases.BOOTSTRAP, fc.to_host(ctx.decrypt(c.data, sk)), c.level, c.scale)

    err = float(np.abs(slots(out) - su["z"]).max())
    print(f"bootstrap under device keys: max slot error {err:.4e} "
          f"(CPU run {cases.BOOTSTRAP_ERR:.4e}), scale / delta {float(out.scale) / br.DELTA:.12f}")
    assert err < 2 * cases.BOOTSTRAP_ERR
    again = boot.bootstrap(out)
    assert again.level == br.OUT_LEVEL
    err2 = float(np.abs(slots(again) - su["z"]).max())
    print(f"second bootstrap: max slot error {err2:.4e}")
    assert err2 < 4 * cases.BOOTSTRAP_ERR


def test_encode_strided_diagonals_matches_the_backend_encoding(fc, ctx):
    """encode_strided_diagonals (the public form) gives the plaintexts and Galois elements the
    Bootstrapper's backend loads for the same factor."""
    from fhecore import bootstrap as bs

    f = bs.dft_factors(br.LOG_N, 3, True)[1]
    n1, n2, stride, offset = bs.factor_layouts(br.LOG_N, 3, True)[1]
    delta = float(ctx.moduli[-1])
    baby, giant, pts = bs.encode_strided_diagonals(ctx, f, n1, n2, delta, stride, offset)
    assert baby == [ctx.galois_elt(stride * (b + offset)) for b in range(n1)]
    assert giant == [ctx.galois_elt(stride * g * n1) for g in range(n2)]
    z, _, _ = bs.place_strided_diagonals(f, ctx.n // 2, n1, n2, stride, offset)
    import encode_ref

    want = encode_ref.encode(z, delta, br.LOG_N, ctx.all_moduli)
    for g in range(n2):
        for b in range(n1):
            assert (fc.to_host(pts[g][b]) == want[g, b]).all()
