"""The exact fixture of the standard shape (tests/golden/exact_std.json, made
by tests/golden/make_exact_std.py) checked on the CPU: the stored solutions
are solutions, the stored costs are their costs, the recorded oracle errors
are those of the oracle built here (a stale fixture shows), and the exact
solve behind it reproduces exact_linear.json."""
import functools
import json
import os
import sys
from fractions import Fraction as F

import numpy as np
import pytest

import helpers

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)


@functools.lru_cache(maxsize=None)
def _fixture():
    import make_exact_std as gen
    return gen.load_fixture()


def _cases():
    return _fixture()["cases"]


def _id(c):
    return f"S{c['S']}_{c['regime']}"


def test_case_table():
    """Every S and regime the generator lists is in the file, once; the
    gradients are there for S <= 7; resid_floor is the nominal maximum."""
    import make_exact_std as gen
    fx = _fixture()
    assert (fx["N"], fx["r"], fx["D"]) == (gen.N, gen.R_ORD, gen.D)
    want = [(S, reg) for S, regs in gen.CASES.items() for reg in regs]
    assert [(c["S"], c["regime"]) for c in fx["cases"]] == want
    for S in (2, 3, 11, 12):
        assert {"nominal", "edge_even", "edge_odd"} <= set(gen.CASES[S])
    for c in fx["cases"]:
        assert ("J" in c) == (c["S"] <= gen.TIME_COST_MAX_S)
        np.testing.assert_array_equal(
            c["times"], gen.regime_times(np.array(_nominal(c["S"])["times"]), c["regime"]))
    assert fx["resid_floor"] == max(c["oracle_resid"] for c in fx["cases"]
                                    if c["regime"] == "nominal")


def _nominal(S):
    return next(c for c in _cases() if c["S"] == S and c["regime"] == "nominal")


def _eval_exact(c, t, k):
    """(p^(k)(t), sum of the magnitudes of its terms) of the FP64
    coefficients c, in Fractions."""
    from make_exact import falling
    terms = [F(float(c[j])) * falling(k, j) * F(float(t)) ** (j - k) for j in range(k, len(c))]
    return sum(terms), sum(abs(x) for x in terms)


@pytest.mark.parametrize("case", _cases(), ids=_id)
def test_exact_solution_is_a_path(oracle, case):
    """Fixed constraints and C^4 continuity of the stored coefficients.

    The coefficients are the exact ones rounded once, so evaluated exactly
    they miss a constraint by at most 2^-53 of the sum of the magnitudes of
    the terms on either side; that is asserted for every case.  With a 0.1 s
    segment the neighbouring vertex derivatives are ~1e8 and those terms
    cancel by ~1e9, so no FP64 coefficients meet the constraints to
    helpers.check_path's 1e-9 of the constraint value there (the exact ones
    miss by up to 3e-7); check_path at 1e-9 is asserted where it can hold,
    on the nominal cases.  Also the stored d_p against the vertex derivatives
    of the coefficients."""
    import make_exact_std as gen
    v = gen.vertices_of(case)
    c, t = np.array(case["coeffs"]), np.array(case["times"])
    if case["regime"] == "nominal":
        helpers.check_path(v, c, t, gen.N, tol=1e-9)
    u = F(1, 2 ** 53)
    for s in range(v.S):
        for d in range(gen.D):
            for k in range(gen.M):
                for end, vi in ((0, s), (1, s + 1)):
                    if v.mask[vi, k]:
                        got, scale = _eval_exact(c[s, d], t[s] if end else 0.0, k)
                        assert abs(got - F(float(v.vals[vi, k, d]))) <= u * scale, (s, d, k, end)
                if s + 1 < v.S:
                    a, sa = _eval_exact(c[s, d], t[s], k)
                    b, sb = _eval_exact(c[s + 1, d], 0.0, k)
                    assert abs(a - b) <= u * (sa + sb), (s, d, k)
    dp = np.array(case["dp"])
    free = ~np.array(case["mask"], bool)
    for d in range(gen.D):
        # derivative k at the start of segment s; the last vertex is fixed
        got = np.array([[helpers.evaluate_poly(c[min(s, v.S - 1), d], 0.0, k)
                         for k in range(gen.M)] for s in range(v.S + 1)])
        np.testing.assert_allclose(got[:v.S][free[:v.S]], dp[d], rtol=1e-12, atol=0)


@pytest.mark.parametrize("case", _cases(), ids=_id)
def test_exact_cost_is_the_cost_of_the_coefficients(oracle, case):
    """1/2 sum c^T Q c (computeCost) of the stored coefficients to 1e-9, and J
    = cost + time_penalty (sum T)^2."""
    import make_exact_std as gen
    c, t = np.array(case["coeffs"]), np.array(case["times"])
    cost = 0.0
    for s in range(len(t)):
        Q = oracle.segment_matrices(gen.N, gen.R_ORD, t[s])[0]
        cost += 0.5 * np.einsum("da,ab,db->", c[s], Q, c[s])
    assert helpers.rel_err(cost, case["cost"]) <= 1e-9
    if "J" in case:
        assert helpers.rel_err(case["cost"] + gen.PENALTY * t.sum() ** 2, case["J"]) <= 1e-14


@pytest.mark.parametrize("case", _cases(), ids=_id)
def test_recorded_oracle_errors_reproduce(oracle, case):
    """The oracle built here shows the recorded errors within a factor 2
    (figures under 1e-14 are single roundings of the compared number and
    count as equal)."""
    import make_exact_std as gen
    now = gen.oracle_figures(case)
    assert set(now) == {k for k in case if k.startswith("oracle_")}
    for k, a in now.items():
        a, b = max(a, 1e-14), max(case[k], 1e-14)
        assert a <= 2.0 * b and b <= 2.0 * a, (k, now[k], case[k])


def test_exact_solve_reproduces_exact_linear():
    """The generator's exact solve at (N = 10, r = 4, D = 1, S = 6) gives the
    committed case of exact_linear.json digit for digit."""
    import make_exact as me
    import make_exact_std as gen
    with open(os.path.join(GOLDEN, "exact_linear.json")) as f:
        c = next(c for c in json.load(f)["cases"] if (c["N"], c["r"]) == (gen.N, gen.R_ORD))
    mask, vals, t = np.array(c["mask"], np.uint8), np.array(c["vals"]), np.array(c["times"])
    assert vals.shape[2] == 1 and len(t) == 6
    sol = gen.exact_solution(gen.N, gen.R_ORD, mask, vals, t)
    np.testing.assert_array_equal(gen.exact_coeffs(gen.N, sol), np.array(c["exact"]))
    np.testing.assert_array_equal(me.exact_solve(gen.N, gen.R_ORD, mask, vals, t),
                                  np.array(c["exact"]))
