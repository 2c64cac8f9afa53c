"""CPU proofs behind tests/test_hip_icp_lm.py, with the oracle alone: the NumPy restatement of the LM stage
(tests/icp_lm_ref.py) reproduces the oracle's damp and sig columns and its pose bit for bit from the oracle's own
err / new_err / xi; every case of tests/icp_lm_cases.py reaches the regime it is named for; and the cases marked
decisive clear their margin on every iteration, so that no accept / reject of theirs hangs on rounding noise."""
import numpy as np
import pytest

from oracle import oracle as o
from tests import icp_lm_cases as lc
from tests import icp_lm_ref as lm

CASE_IDS = [c["name"] for c in lc.CASES]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("n", lc.SIZES)
@pytest.mark.parametrize("case", lc.CASES, ids=CASE_IDS)
def test_replay_reproduces_the_oracle_bit_for_bit(case, n, mode):
    """damp, sig and T from the trace's err, new_err and xi alone.  libm's pow is what the restatement calls too, so no
    entry needs an ulp allowance: every comparison is on the bits."""
    T, tr = lc.oracle_run(case, n, mode)
    assert np.isfinite(T).all() and np.isfinite(tr).all(), "the oracle's pose and trace stay finite"
    r = lm.replay(tr, lc.params(case, n, mode))
    assert np.array_equal(bits(r["damp"]), bits(tr[:, 2])), (r["damp"], tr[:, 2])
    assert np.array_equal(bits(r["sig"]), bits(tr[:, 3])), (r["sig"], tr[:, 3])
    assert np.array_equal(bits(r["T"]), bits(T)), (r["T"], T)
    assert np.array_equal(tr[:, 10:], np.zeros((tr.shape[0], 2), np.float32))
    if mode == 0:
        assert np.array_equal(r["accept"], tr[:, 1] < tr[:, 0])
        for k in np.flatnonzero(~r["accept"]):
            assert np.array_equal(r["T_step"][k], np.eye(4, dtype=np.float32))


def test_se3_exp_restatement_equals_the_oracle():
    """both branches and both sides of (float)theta < 1e-6f, on the bits"""
    rng = np.random.default_rng(3)
    below = np.nextafter(np.float32(1e-6), np.float32(0))
    for th in [0.0, 1e-30, float(below), float(np.float32(1e-6)), 1e-4, 0.3, 1.0, 3.0, 50.0]:
        for _ in range(4):
            a = rng.normal(size=3)
            xi = np.concatenate([rng.normal(size=3), th * a / np.linalg.norm(a)]).astype(np.float32)
            assert np.array_equal(bits(lm.se3_exp(xi)), bits(o.se3_exp(xi))), xi


@pytest.mark.parametrize("n", lc.SIZES)
@pytest.mark.parametrize("case", lc.CASES, ids=CASE_IDS)
def test_every_witness_holds_on_the_oracle(case, n):
    for mode in case["witness_modes"]:
        _, tr = lc.oracle_run(case, n, mode)
        assert case["witness"](tr, lc.params(case, n, mode)), (case["name"], n, mode, lc.pattern(tr), tr[:, :4])


def test_some_decisive_scene_accepts_again_after_a_reject():
    for n in lc.SIZES:
        case = lc.BY_NAME["reaccept"]
        assert 0 in case["decisive"][n]
        assert "RA" in lc.pattern(lc.oracle_run(case, n, 0)[1])


@pytest.mark.parametrize("n", lc.SIZES)
@pytest.mark.parametrize("case", [c for c in lc.CASES if any(c["decisive"].values())],
                         ids=[c["name"] for c in lc.CASES if any(c["decisive"].values())])
def test_decisive_cases_clear_their_margin_on_every_iteration(case, n):
    """|new_err - err| >= 1e-3 err: a condition on the inputs, ten times what the kernels' err may differ by"""
    for mode in case["decisive"][n]:
        _, tr = lc.oracle_run(case, n, mode)
        m = lc.margins(tr)
        assert m.min() >= lc.DECISIVE_MARGIN, (case["name"], n, mode, m)


def test_saturate_overflows_to_lmin_and_stays_finite():
    """-B errdiff > 700 makes exp overflow float32: the damping factor is lmin exactly, sig is 0, the step the identity"""
    case = lc.BY_NAME["saturate"]
    for n in lc.SIZES:
        prm = lc.params(case, n, 1)
        T, tr = lc.oracle_run(case, n, 1)
        r = lm.replay(tr, prm)
        lmin, _ = lm.soft_constants(prm)
        d = np.clip(lc.errdiffs(tr), -70.0, 70.0)
        hit = np.flatnonzero(-float(np.float32(prm["B"])) * d.astype(np.float64) > 700.0)
        assert hit.size and np.all(r["factor"][hit] == lmin) and np.all(r["sig"][hit] == 0)
        assert np.isfinite(T).all()


def test_soft_formulas_are_monotone_in_errdiff():
    """what the interval check of the GPU test relies on: both float64 formulas do not decrease with errdiff"""
    for prm in (dict(lc.DEFAULT), dict(lc.SOFT), dict(lc.DEFAULT, B=20.0, B2=15.0)):
        d = np.linspace(-70.0, 70.0, 2801)
        f, s = np.array([lm.soft_formulas_f64(float(x), prm) for x in d]).T
        assert np.all(np.diff(f) >= 0) and np.all(np.diff(s) >= 0)
