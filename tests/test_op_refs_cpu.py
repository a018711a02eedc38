"""tests/golden/op_refs.json holds the SHA-256 of every result of the plaintext-arithmetic, mul-sum,
ModRaise, split / merge and sparse-secret functions at every level on three seeded shapes, and of
every array of the five shared cases with their CPU results, computed by the reference modules and
setup() functions that pyoracle and tests/cases.py replaced (tests/golden/make_golden.py op_refs).
pyoracle and the case builder must reproduce each: the definitions and the fixtures are the same
bits, which passing GPU comparisons against them could not show."""
import json
import os

import cases
import pyoracle
import refs


def _pinned(prefix, keep):
    with open(os.path.join(os.path.dirname(__file__), "golden", "op_refs.json")) as f:
        return {k: v for k, v in json.load(f).items() if k.startswith(prefix) == keep}


def test_every_moved_operation_at_every_level_is_what_its_reference_module_computed():
    """With the C transforms everywhere, and at log_n = 6 with ntt=None as well, the pure-Python
    definition."""
    want = _pinned("case/", False)
    got = {}
    for shape in refs.PIN_OPS:
        w = refs.small_world(*shape)
        got.update(refs.op_digests(w, pyoracle, refs.c_ntt()))
        if shape in refs.PIN_SMALL:
            assert refs.op_digests(w, pyoracle, None) == {k: got[k] for k in got if k.startswith(
                f"n{shape[0]}_L{shape[1]}_")}, shape
    assert got.keys() == want.keys()
    assert [k for k in want if got[k] != want[k]] == []


def test_every_shared_case_is_what_its_setup_and_cpu_run_computed():
    want = _pinned("case/", True)
    got = cases.case_digests()
    assert got.keys() == want.keys()
    assert [k for k in want if got[k] != want[k]] == []
