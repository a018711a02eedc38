"""fhecore.polyeval.eval_mod on the GPU backend: the shared case of tests/cases.py (EVALMOD) bit for
bit against the CPU backend, and the same slots under keys made on the device, next to a
mod_raise of the ciphertext from the bottom of the chain."""
import numpy as np
import pytest

import cases

EM = cases.EVALMOD

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fc():
    import fhecore

    return fhecore


@pytest.fixture(scope="module")
def ctx(fc):
    su = cases.setup(EM)
    c = fc.Context(EM.log_n, moduli=su["qs"], special=su["ps"], dnum=EM.dnum)
    assert c.moduli == su["qs"] and c.special == su["ps"]
    return c


def u64(x):
    return np.asarray(x).astype(np.uint64)


def test_eval_mod_matches_the_cpu_backend_bit_for_bit(fc, ctx):
    """Both backends receive the same integer scalars, so data, level and scale are the same."""
    from fhecore import polyeval

    su = cases.setup(EM)
    key = (fc.to_device(u64(su["relin"][0])), fc.to_device(u64(su["relin"][1])))
    be = polyeval.GpuBackend(ctx, key)
    ct = polyeval.Ct(fc.to_device(u64(su["ct"])), EM.L, EM.delta)
    out = polyeval.eval_mod(be, ct, cases.K, cases.DEGREE, cases.DOUBLE_ANGLES)
    ref, err = cases.run_cpu(EM)
    assert (out.level, out.scale) == (ref.level, ref.scale)
    assert (fc.to_host(out.data) == u64(ref.data)).all()
    assert err < cases.MARGIN * cases.EVALMOD_ERR


def test_eval_mod_under_device_keys(fc, ctx):
    """keygen_secret / keygen_relin / encrypt_sk on the device.  The ciphertext dropped to level 1
    is raised back to L with mod_raise (limb 0 kept, L limbs again); eval_mod on the fresh
    encryption of the shared slots decrypts and decodes within the constant of the CPU run."""
    from fhecore import polyeval

    su = cases.setup(EM)
    sk = ctx.keygen_secret(seed=21)
    key = ctx.keygen_relin(sk, seed=22)
    ct = ctx.encrypt_sk(fc.to_device(su["pt"]), sk, seed=23)
    up = ctx.mod_raise(ctx.drop_level(ct, 1))
    assert tuple(up.shape) == (2, EM.L, 1 << EM.log_n)
    assert (up[:, 0] == ct[:, 0]).all()
    out = polyeval.eval_mod(polyeval.GpuBackend(ctx, key), polyeval.Ct(ct, EM.L, EM.delta), cases.K,
                            cases.DEGREE, cases.DOUBLE_ANGLES)
    assert out.level == 3
    got = cases.decode(EM, fc.to_host(ctx.decrypt(out.data, sk)), out.level, out.scale)
    err = float(np.abs(got - cases.evalmod_target(su["v"])).max())
    print(f"eval_mod under device keys: max slot error {err:.4e} "
          f"(CPU run {cases.EVALMOD_ERR:.4e}, cap {cases.CAP:.4e})")
    assert err < cases.MARGIN * cases.EVALMOD_ERR
    assert float(np.abs(got - su["eps"]).max()) <= cases.CAP + cases.MARGIN * cases.EVALMOD_ERR
