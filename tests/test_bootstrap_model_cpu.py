"""The float64 plaintext model of the bootstrap pipeline (tests/bootstrap_ref.py model) with the
Bootstrapper's constants: slots uniform in [-1, 1]^2, I uniform in [-15, 15], the exact sine and
eval_mod's interpolant with its double angles; the result returns to the message.  The figures
are the ones bootstrap_ref.py's choice of q_0 rests on."""
import pytest

import bootstrap_ref as br
import cases


# (q_0 bits, exact sine, noise) -> the model's maximum slot error at log_n = 10, seed 3
FLOOR = {(60, True, 0.0): 2.61e-08, (55, True, 0.0): 2.67e-05,
         (60, True, 1e-8): 8.94e-04, (55, True, 1e-8): 4.02e-05,
         (55, False, 0.0): 2.68e-05, (55, False, 1e-8): 4.03e-05}


@pytest.mark.parametrize("bits,exact,noise", sorted(FLOOR))
def test_model_returns_to_the_message(bits, exact, noise):
    """The error is the cubic term (2 pi)^2 (m / q_0)^3 / 6 times q_0 / delta, plus the noise times
    q_0 / delta: within 5 % of the recorded figure (float differences between numpy builds; the
    draw is seeded)."""
    err = br.model(10, float(2 ** bits), exact_sine=exact, noise=noise)
    print(f"q_0 = 2^{bits}, exact sine {exact}, noise {noise:g}: max slot error {err:.3e}")
    want = FLOOR[(bits, exact, noise)]
    assert abs(err - want) < 0.05 * want


def test_the_choice_of_q0():
    """With the evaluator's noise the error is smallest at 55 bits over delta = 2^50; without it a
    larger q_0 is always better (4 per bit)."""
    noisy = {b: br.model(10, float(2 ** b), noise=1e-8) for b in (53, 54, 55, 56, 57, 60)}
    assert min(noisy, key=noisy.get) == br.Q0_BITS == 55
    clean = [br.model(10, float(2 ** b)) for b in (54, 55, 56)]
    assert 3.9 < clean[0] / clean[1] < 4.1 and 3.9 < clean[1] / clean[2] < 4.1
    q0 = br.moduli()[0][0]
    assert q0.bit_length() == 55 and all(q.bit_length() == 50 for q in br.moduli()[0][1:])


def test_the_model_at_the_shared_case():
    """The interpolant, no noise, at the shared case's own q_0 and parameters: the cubic floor the
    measured BOOTSTRAP_ERR sits on."""
    q0 = br.moduli()[0][0]
    err = br.model(br.LOG_N, float(q0), exact_sine=False)
    print(f"model at the shared case's q_0: {err:.3e}; BOOTSTRAP_ERR {cases.BOOTSTRAP_ERR:.3e}")
    assert 0.5 * cases.BOOTSTRAP_ERR < err < 2 * cases.BOOTSTRAP_ERR
