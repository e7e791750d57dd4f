"""The tube QCQP's dual certificates on the CPU (tests/tube_cert.py,
tests/golden/tube_dual.json; no GPU).

  * The fixture is what its generator says: the cases of the issue, every
    multiplier >= 0, the stored d(lambda) reproduced in float64 and, for the
    cases with n <= 75, again in 50-digit arithmetic.
  * The oracle's tol 1e-10 solution passes the assertions the GPU rows get
    (tests/test_tube_dual_gpu.py uses the same tube_cert.check_row).
  * The certificate has teeth: a solve stopped at tol 1e-6 fails the upper
    side, and an x pushed 1e-6 r outside one active tube constraint fails the
    lower side.

On the second teeth check.  Weak duality holds for every x, feasible or not:
cost(x) >= lower - sum lam_k max(g_k(x), 0).  With the whole violation counted
in the slack no point can fail the lower side, however good lambda is.  A GPU
row passes only if it also meets max g <= 1e-8, so together the two assertions
say gap >= -slack_capped, the slack with every max(g_k, 0) counted up to 1e-8
only.  That is the form the pushed point has to fail: it is outside by
2 r x 1e-6 r = 4.5e-8 > 1e-8, its cost drops by lam_k x that, and the check
catches it only if lam_k is the true sensitivity, i.e. the certificate is tight.
"""
import functools
import os
import sys

import numpy as np
import pytest

import pyoracle
import tube_cert

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_tube_dual as gen  # noqa: E402

GROUPS = {"orders": 10, "s_kernels": 16, "runtime_s10": 2, "box": 8, "radii": 1}
NOMINAL = ("orders", "s_kernels", "runtime_s10", "radii")


@functools.lru_cache(maxsize=None)
def fixture():
    return tube_cert.load()


def all_cases():
    return [c for g in fixture()["groups"].values() for c in g["cases"]]


def case_ids():
    return [c["name"] for c in all_cases()]


def vertices(case):
    return pyoracle.random_vertices(case["N"] // 2 - 1, case["S"], 3, -10.0, 10.0, case["seed"])


@functools.lru_cache(maxsize=12)
def case_forms(name):
    """The assembled forms at the multipliers' indices (the last few cases kept)."""
    case = next(c for c in all_cases() if c["name"] == name)
    qp = pyoracle.tube_assemble(case["N"], case["r"], vertices(case), case["times"], case["radii"],
                                times_cp=case["times_cp"])
    assert qp["cst"].shape == (case["n_con"],) and qp["q"].shape == (case["n"],)
    return tube_cert.forms(qp, case["lam_idx"])


def oracle_solve(case, tol):
    return pyoracle.tube_solve(case["N"], case["r"], vertices(case), case["times"], case["radii"],
                               times_cp=case["times_cp"], tol=tol, max_iter=100)


def residuals(case, x):
    return pyoracle.tube_residuals(case["N"], case["r"], vertices(case), case["times"],
                                   case["radii"], x, times_cp=case["times_cp"])


def test_fixture_cases():
    """The groups and shapes of the issue; the oracle converged on every nominal
    case; the box corners (b) are the rows it did not converge on."""
    fx = fixture()
    assert {k: len(g["cases"]) for k, g in fx["groups"].items()} == GROUPS
    shapes = {(c["N"], c["r"], c["S"]) for c in fx["groups"]["orders"]["cases"]}
    assert shapes == {(4, 1, 3), (6, 2, 5), (8, 3, 4), (10, 4, 2), (12, 5, 6)}
    assert sorted({c["S"] for c in fx["groups"]["s_kernels"]["cases"]}) == [2, 3, 5, 7, 9, 11, 13, 16]
    assert {c["S"] for c in fx["groups"]["runtime_s10"]["cases"]} == {17}
    for name in NOMINAL:
        assert all(c["oracle_status"] == 0 for c in fx["groups"][name]["cases"]), name
    for c in fx["groups"]["box"]["cases"]:
        assert not np.array_equal(c["times"], c["times_cp"])      # stale control-point maps
        assert np.all(c["times"] >= 0.1) and np.all(c["times"] <= 2.0 * c["times_cp"])
        if c["kind"] == "box_b":
            assert np.all(c["times"][0::2] == 0.1) and np.all(c["times"][1::2] == 2 * c["times_cp"][1::2])
    for name, g in fx["groups"].items():
        conv = [c["oracle_gap_rel"] for c in g["cases"] if c["oracle_status"] == 0]
        assert g["gap_floor"] == max(conv), name
    assert os.path.getsize(tube_cert.FIXTURE) <= os.path.getsize(
        os.path.join(os.path.dirname(tube_cert.FIXTURE), "exact_std.json"))


@pytest.mark.parametrize("name", case_ids())
def test_multipliers_and_float64_dual(name):
    """lambda >= 0, and d(lambda) evaluated here in float64 agrees with the
    stored 50-digit value as closely as the generator's float64 evaluation
    did.  Another LAPACK rounds differently: 8 x the recorded deviation, and
    never below the rounding of n sums of n terms."""
    case = next(c for c in all_cases() if c["name"] == name)
    assert np.all(case["lam"] > 0.0) and len(case["lam"]) == len(case["lam_idx"])
    assert len(set(case["lam_idx"].tolist())) == len(case["lam_idx"])
    assert 0 <= case["lam_idx"].min() and case["lam_idx"].max() < case["n_con"]
    fm = case_forms(name)
    d64, _ = tube_cert.dual_value(fm, case["lam"])
    scale = max(abs(case["dual"]), 1.0)
    assert abs(case["dual_f64"] - case["dual"]) / scale <= case["dual_f64_dev"] + tube_cert.EPS
    assert abs(d64 - case["dual"]) / scale <= max(8.0 * case["dual_f64_dev"],
                                                  case["n"] ** 2 * tube_cert.EPS)
    # lower = 1/2 d + c0, rounded down
    assert abs(case["lower"] - (0.5 * case["dual"] + case["c0"])) <= 4 * tube_cert.EPS * (
        abs(0.5 * case["dual"]) + abs(case["c0"]))


@pytest.mark.parametrize("name", [c["name"] for c in all_cases() if c["n"] <= 75])
def test_dual_in_multiprecision(name):
    """d(lambda) again in 50-digit arithmetic on the assembled doubles: the
    stored value to its last bit, and A = P + sum lam_k Q_k positive definite."""
    pytest.importorskip("mpmath")
    case = next(c for c in all_cases() if c["name"] == name)
    d = gen.mp_dual(case_forms(name), case["lam"])
    assert d is not None
    assert float(d) == case["dual"]


@pytest.mark.parametrize("name", [c["name"] for c in all_cases() if c["oracle_status"] == 0])
def test_oracle_meets_the_gpu_assertions(name):
    case = next(c for c in all_cases() if c["name"] == name)
    floor = fixture()["groups"][case["group"]]["gap_floor"]
    sol = oracle_solve(case, 1e-10)
    assert sol["status"] == 0
    fig = tube_cert.assess(case, floor, sol["coeffs"], sol["x"], sol["cost"],
                           residuals(case, sol["x"]), case_forms(name))
    tube_cert.check_row(case, tube_cert.OK, fig)
    # the float64 integral against the generator's 50-digit one, at its own bound
    assert case["oracle_cost_int_f64_err"] * fig["cost_int"] <= fig["e_int"]


def first_cases():
    return [g["cases"][0]["name"] for g in fixture()["groups"].values()]


@pytest.mark.parametrize("name", first_cases())
def test_teeth_early_stop_fails_upper_side(name):
    """The oracle stopped at tol 1e-6, 1e4 x early, is outside the bound."""
    case = next(c for c in all_cases() if c["name"] == name)
    floor = fixture()["groups"][case["group"]]["gap_floor"]
    sol = oracle_solve(case, 1e-6)
    fig = tube_cert.assess(case, floor, sol["coeffs"], sol["x"], sol["cost"],
                           residuals(case, sol["x"]), case_forms(name))
    print(f"{name}: tol 1e-6 gap/cost {fig['gap'] / fig['cost_int']:.2e}, bound/cost "
          f"{fig['bound'] / fig['cost_int']:.2e}")
    assert fig["gap"] > fig["bound"]
    with pytest.raises(AssertionError):
        tube_cert.check_row(case, tube_cert.OK, fig)


@pytest.mark.parametrize("name", first_cases())
def test_teeth_infeasible_point_fails_lower_side(name):
    """x moved so that one active tube constraint is violated by 2 r x 1e-6 r
    (1e-6 r outside the tube) with the other active constraints held to first
    order.  cost = 1/2 f + c0, so the cost moves by 1/2 (grad f . dx +
    1/2 dx^T P dx), evaluated without cancellation."""
    case = next(c for c in all_cases() if c["name"] == name)
    fm = case_forms(name)
    sol = oracle_solve(case, 1e-10)
    x = sol["x"]
    tubes = set(tube_cert.tube_constraint_indices(case["N"], case["S"]).tolist())
    cand = [i for i, k in enumerate(case["lam_idx"]) if int(k) in tubes]
    assert cand, "no active tube constraint"
    k = max(cand, key=lambda i: case["lam"][i])
    # which radius: r1 of the constraint's segment
    per = [(1 if i < case["S"] - 1 else 0) + 3 * (case["N"] - 2) for i in range(case["S"])]
    seg = int(np.searchsorted(np.cumsum(per), case["lam_idx"][k], side="right"))
    r1 = case["radii"][seg, 0]
    delta = 2.0 * r1 * 1e-6 * r1
    J = np.einsum("kij,j->ki", 0.5 * (fm["quad"] + fm["quad"].transpose(0, 2, 1)), x) + fm["lin"]
    rhs = np.zeros(len(case["lam"]))
    rhs[k] = delta
    dx = np.linalg.lstsq(J, rhs, rcond=None)[0]
    xp = x + dx
    g0, _ = tube_cert.constraint_values(fm, x)
    g1, e1 = tube_cert.constraint_values(fm, xp)
    assert g1[k] - g0[k] == pytest.approx(delta, rel=1e-3)
    assert g1[k] > tube_cert.FEASIBILITY_BAR
    grad = fm["P"] @ x + fm["q"]
    cost0, e0 = tube_cert.cost_integral(sol["coeffs"], case["times"], case["r"])
    cost = cost0 + 0.5 * (grad @ dx + 0.5 * dx @ fm["P"] @ dx)
    gap, slack = tube_cert.gap_and_slack(case, cost, e0, g1, e1)
    _, capped = tube_cert.gap_and_slack(case, cost, e0, g1, e1, cap=tube_cert.FEASIBILITY_BAR)
    print(f"{name}: lam {case['lam'][k]:.3e} g {g1[k]:.2e} gap {gap:.3e} slack {slack:.3e} "
          f"capped {capped:.3e}")
    assert -slack <= gap                 # weak duality itself: no x can break it
    assert gap < -capped                 # with the feasibility bar: caught
