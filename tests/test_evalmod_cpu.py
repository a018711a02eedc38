"""fhecore.polyeval.eval_mod without a GPU, on the CPU backend and the shared case of
tests/cases.py (EVALMOD): its error against sin(2 pi K v) / (2 pi), the cap that error must respect,
the distance to eps, level and scale, the refusals, and the delegation to chebyshev_eval."""
import math
from fractions import Fraction

import numpy as np
import pytest

import cases

EM = cases.EVALMOD


def test_eval_mod_error_and_cap():
    """Maximum slot error of this run: 1.051e-08 (deterministic under the fixed seeds; the margin
    covers float differences between numpy builds in the decode only).  The cap
    (2 pi)^2 (2^-8)^3 / 6 = 3.9e-7 is the cubic term the choice of eps already accepts: past it
    EvalMod's own error would dominate."""
    out, err = cases.run_cpu(EM)
    print(f"eval_mod: level {out.level}, max slot error {err:.4e}, cap {cases.CAP:.4e}")
    assert err < cases.MARGIN * cases.EVALMOD_ERR
    assert err < cases.CAP
    assert abs(cases.CAP - 3.9e-7) < 0.05e-7


def test_eval_mod_removes_the_integer_part():
    """K v = I + eps: the result is eps within the cubic term plus the measured error."""
    out, err = cases.run_cpu(EM)
    su = cases.setup(EM)
    got = cases.decrypt_decode(EM, out.data, out.level, out.scale)
    dist = float(np.abs(got - su["eps"]).max())
    print(f"eval_mod: max distance to eps {dist:.4e}")
    assert dist <= cases.CAP + cases.MARGIN * cases.EVALMOD_ERR
    assert np.abs(su["v"] * cases.K - np.round(su["v"] * cases.K)).max() <= cases.EPS_MAX
    assert np.abs(np.round(su["v"] * cases.K)).max() == cases.K - 1  # the whole range of I is used


def test_eval_mod_level_and_scale():
    from fhecore import polyeval

    assert polyeval.eval_mod_levels(31, 3) == 9
    assert polyeval.eval_mod_levels(31, 0) == polyeval.levels_needed(31) == 6
    out, _ = cases.run_cpu(EM)
    assert out.level == EM.L - 9 == 3
    assert np.asarray(out.data).shape == (2, 3, 1 << EM.log_n)
    # the scale: chebyshev_eval ends at exactly delta; each double angle squares the scale and
    # divides by the prime it rescales by; then the factor 1 / (2 pi) as the float 2 pi
    qs = cases.setup(EM)["qs"]
    s = Fraction(EM.delta)
    for level in (6, 5, 4):  # the levels of the three products' inputs
        s = s * s / qs[level - 1]
    assert out.scale == s * Fraction(2.0 * math.pi)


def test_eval_mod_refusals():
    from fhecore import polyeval

    su = cases.setup(EM)
    be = cases.backend(EM)
    # 9 levels consumed and one must remain: an input at level 9 is too low (nothing is computed)
    with pytest.raises(ValueError, match="too few levels"):
        polyeval.eval_mod(be, polyeval.Ct(su["ct"][:, :9], 9, EM.delta), cases.K, cases.DEGREE,
                          cases.DOUBLE_ANGLES)
    with pytest.raises(ValueError, match="K"):
        polyeval.eval_mod(be, polyeval.Ct(su["ct"], EM.L, EM.delta), 0)
    with pytest.raises(ValueError, match="degree"):  # chebyshev_eval's own error
        polyeval.eval_mod(be, polyeval.Ct(su["ct"], EM.L, EM.delta), cases.K, degree=64)


def test_eval_mod_without_double_angles_is_chebyshev_eval():
    """double_angles = 0, degree 3: the series of cos(2 pi K v - pi / 2) through chebyshev_eval,
    bit for bit, with the declared scale times 2 pi."""
    from fhecore import polyeval

    su = cases.setup(EM)
    be = cases.backend(EM)
    ct = polyeval.Ct(su["ct"][:, :4], 4, EM.delta)
    got = polyeval.eval_mod(be, ct, 1, degree=3, double_angles=0)
    c = np.polynomial.chebyshev.chebinterpolate(
        lambda v: np.cos((2.0 * math.pi * 1 * v - math.pi / 2) / 1.0), 3)
    want = polyeval.chebyshev_eval(be, ct, [Fraction(float(v)) for v in c])
    assert got.level == want.level == 4 - polyeval.levels_needed(3)
    assert got.scale == want.scale * Fraction(2.0 * math.pi)
    assert (np.asarray(got.data) == np.asarray(want.data)).all()
