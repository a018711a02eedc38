"""fhecore.polyeval.eval_mod on the GPU backend: the shared case of tests/evalmod_ref.py bit for
bit against the CPU backend, and the same slots under keys made on the device, next to a
mod_raise of the ciphertext from the bottom of the chain."""
import numpy as np
import pytest

import evalmod_ref as er

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fc():
    import fhecore

    return fhecore


@pytest.fixture(scope="module")
def ctx(fc):
    su = er.setup()
    c = fc.Context(er.LOG_N, moduli=su["qs"], special=su["ps"], dnum=er.DNUM)
    assert c.moduli == su["qs"] and c.special == su["ps"]
    return c


def u64(x):
    return np.asarray(x).astype(np.uint64)


def test_eval_mod_matches_the_cpu_backend_bit_for_bit(fc, ctx):
    """Both backends receive the same integer scalars, so data, level and scale are the same."""
    from fhecore import polyeval

    su = er.setup()
    key = (fc.to_device(u64(su["evk_b"])), fc.to_device(u64(su["evk_a"])))
    be = polyeval.GpuBackend(ctx, key)
    ct = polyeval.Ct(fc.to_device(u64(su["ct"])), er.L, er.DELTA)
    out = polyeval.eval_mod(be, ct, er.K, er.DEGREE, er.DOUBLE_ANGLES)
    ref, err = er.evalmod_cpu()
    assert (out.level, out.scale) == (ref.level, ref.scale)
    assert (fc.to_host(out.data) == u64(ref.data)).all()
    assert err < er.MARGIN * er.EVALMOD_ERR


def test_eval_mod_under_device_keys(fc, ctx):
    """keygen_secret / keygen_relin / encrypt_sk on the device.  The ciphertext dropped to level 1
    is raised back to L with mod_raise (limb 0 kept, L limbs again); eval_mod on the fresh
    encryption of the shared slots decrypts and decodes within the constant of the CPU run."""
    from fhecore import polyeval

    su = er.setup()
    sk = ctx.keygen_secret(seed=21)
    key = ctx.keygen_relin(sk, seed=22)
    ct = ctx.encrypt_sk(fc.to_device(su["pt"]), sk, seed=23)
    up = ctx.mod_raise(ctx.drop_level(ct, 1))
    assert tuple(up.shape) == (2, er.L, 1 << er.LOG_N)
    assert (up[:, 0] == ct[:, 0]).all()
    out = polyeval.eval_mod(polyeval.GpuBackend(ctx, key), polyeval.Ct(ct, er.L, er.DELTA), er.K,
                            er.DEGREE, er.DOUBLE_ANGLES)
    assert out.level == 3
    got = er.decode(fc.to_host(ctx.decrypt(out.data, sk)), out.level, out.scale)
    err = float(np.abs(got - er.target(su["v"])).max())
    print(f"eval_mod under device keys: max slot error {err:.4e} "
          f"(CPU run {er.EVALMOD_ERR:.4e}, cap {er.CAP:.4e})")
    assert err < er.MARGIN * er.EVALMOD_ERR
    assert float(np.abs(got - su["eps"]).max()) <= er.CAP + er.MARGIN * er.EVALMOD_ERR
