"""fhecore.polyeval.eval_mod without a GPU, on the CPU backend and the shared case of
tests/evalmod_ref.py: its error against sin(2 pi K v) / (2 pi), the cap that error must respect,
the distance to eps, level and scale, the refusals, and the delegation to chebyshev_eval."""
import math
from fractions import Fraction

import numpy as np
import pytest

import evalmod_ref as er
import plain_ref


def test_eval_mod_error_and_cap():
    """Maximum slot error of this run: 1.051e-08 (deterministic under the fixed seeds; the margin
    covers float differences between numpy builds in the decode only).  The cap
    (2 pi)^2 (2^-8)^3 / 6 = 3.9e-7 is the cubic term the choice of eps already accepts: past it
    EvalMod's own error would dominate."""
    out, err = er.evalmod_cpu()
    print(f"eval_mod: level {out.level}, max slot error {err:.4e}, cap {er.CAP:.4e}")
    assert err < er.MARGIN * er.EVALMOD_ERR
    assert err < er.CAP
    assert abs(er.CAP - 3.9e-7) < 0.05e-7


def test_eval_mod_removes_the_integer_part():
    """K v = I + eps: the result is eps within the cubic term plus the measured error."""
    out, err = er.evalmod_cpu()
    su = er.setup()
    got = er.decrypt_decode(out.data, out.level, out.scale)
    dist = float(np.abs(got - su["eps"]).max())
    print(f"eval_mod: max distance to eps {dist:.4e}")
    assert dist <= er.CAP + er.MARGIN * er.EVALMOD_ERR
    assert np.abs(su["v"] * er.K - np.round(su["v"] * er.K)).max() <= er.EPS_MAX
    assert np.abs(np.round(su["v"] * er.K)).max() == er.K - 1  # the whole range of I is used


def test_eval_mod_level_and_scale():
    from fhecore import polyeval

    assert polyeval.eval_mod_levels(31, 3) == 9
    assert polyeval.eval_mod_levels(31, 0) == polyeval.levels_needed(31) == 6
    out, _ = er.evalmod_cpu()
    assert out.level == er.L - 9 == 3
    assert np.asarray(out.data).shape == (2, 3, 1 << er.LOG_N)
    # the scale: chebyshev_eval ends at exactly delta; each double angle squares the scale and
    # divides by the prime it rescales by; then the factor 1 / (2 pi) as the float 2 pi
    qs = er.setup()["qs"]
    s = Fraction(er.DELTA)
    for level in (6, 5, 4):  # the levels of the three products' inputs
        s = s * s / qs[level - 1]
    assert out.scale == s * Fraction(2.0 * math.pi)


def test_eval_mod_refusals():
    from fhecore import polyeval

    su = er.setup()
    be = er.backend()
    # 9 levels consumed and one must remain: an input at level 9 is too low (nothing is computed)
    with pytest.raises(ValueError, match="too few levels"):
        polyeval.eval_mod(be, polyeval.Ct(su["ct"][:, :9], 9, er.DELTA), er.K, er.DEGREE,
                          er.DOUBLE_ANGLES)
    with pytest.raises(ValueError, match="K"):
        polyeval.eval_mod(be, polyeval.Ct(su["ct"], er.L, er.DELTA), 0)
    with pytest.raises(ValueError, match="degree"):  # chebyshev_eval's own error
        polyeval.eval_mod(be, polyeval.Ct(su["ct"], er.L, er.DELTA), er.K, degree=64)


def test_eval_mod_without_double_angles_is_chebyshev_eval():
    """double_angles = 0, degree 3: the series of cos(2 pi K v - pi / 2) through chebyshev_eval,
    bit for bit, with the declared scale times 2 pi."""
    from fhecore import polyeval

    su = er.setup()
    be = er.backend()
    ct = polyeval.Ct(su["ct"][:, :4], 4, er.DELTA)
    got = polyeval.eval_mod(be, ct, 1, degree=3, double_angles=0)
    c = np.polynomial.chebyshev.chebinterpolate(
        lambda v: np.cos((2.0 * math.pi * 1 * v - math.pi / 2) / 1.0), 3)
    want = polyeval.chebyshev_eval(be, ct, [Fraction(float(v)) for v in c])
    assert got.level == want.level == 4 - polyeval.levels_needed(3)
    assert got.scale == want.scale * Fraction(2.0 * math.pi)
    assert (np.asarray(got.data) == np.asarray(want.data)).all()
