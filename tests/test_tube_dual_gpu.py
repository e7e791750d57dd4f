"""GPU tube QCQP results against dual certificates (tests/tube_cert.py,
tests/golden/tube_dual.json): mtg_tube_solve on every case of the fixture,
mtg_ragged_tube_solve on one mixed batch, and the J of mtg_tube_time_cost /
mtg_ragged_tube_time_cost on the box cases.

The other GPU tube tests compare the kernels with the oracle's interior-point
method, which is the same algorithm.  Here the reference is the weak-duality
bound lower <= cost, evaluated in 50-digit arithmetic from stored multipliers:
it depends on no solver.  A row is held to "within a certified distance of the
optimum", the distance being what the oracle itself reaches at tol 1e-10
(tube_cert.check_row states the assertions; the oracle passes the same ones in
tests/test_tube_dual_cpu.py).  The constraint values at the GPU's x come from
oracle.tube_residuals (assembly only, pinned by the geometric restatement in
tests/test_tube_oracle.py).

Each test prints one line per group (run with -s); the lines measured on MI355X
are in profiles/tube_dual_gpu.txt.
"""
import numpy as np
import pytest

import tube_cert
from test_tube_dual_cpu import all_cases, case_forms, fixture, residuals, vertices

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TIME_PENALTY = 500.0
GROUPS = ("orders", "s_kernels", "runtime_s10", "box", "radii")
# The ragged batch: the N = 10 cases of S = 2, 5, 9, 16 and the S = 17 cases.
RAGGED_S = (2, 5, 9, 16, 17)
RAGGED_S_MAX = 17


def _T(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def geometry(case):
    """positions [(S+1), 3] and fixed values [3, N] of a case's vertices."""
    v = vertices(case)
    m, S = case["N"] // 2, case["S"]
    fv = np.zeros((3, case["N"]))
    fv[:, :m] = v.vals[0, :m, :].T
    fv[:, m:] = v.vals[S, :m, :].T
    return v.vals[:, 0, :].copy(), fv


def uniform_inputs(dev, cases):
    pos, fv = zip(*(geometry(c) for c in cases))
    return (_T(dev, np.stack(pos)), _T(dev, np.stack(fv)),
            _T(dev, np.stack([c["times_cp"] for c in cases])),
            _T(dev, np.stack([c["times"] for c in cases])),
            _T(dev, np.stack([c["radii"] for c in cases])))


def ragged_inputs(dev, cases, S_max):
    """NaN-padded inputs of a ragged batch, times_cp and times apart."""
    import mav_tube_trajectory_generation_amd as mtg
    probs = [(*geometry(c), c["times"], c["radii"]) for c in cases]
    seg, pos, fv, t, radii = mtg.pack_ragged_tube(probs, cases[0]["N"], dev, S_max=S_max)
    tcp = np.full((len(cases), S_max), np.nan)
    for b, c in enumerate(cases):
        tcp[b, :c["S"]] = c["times_cp"]
    return seg, pos, fv, _T(dev, tcp), t, radii


def floor_of(case):
    return fixture()["groups"][case["group"]]["gap_floor"]


def row_figures(case, status, coeffs, x, cost):
    """tube_cert.assess for a row with a finite result, else None."""
    if not (np.isfinite(cost) and np.isfinite(coeffs).all() and np.isfinite(x).all()):
        assert status not in (tube_cert.OK, tube_cert.NEAR_OPTIMAL), (case["name"], status)
        return None
    return tube_cert.assess(case, floor_of(case), coeffs, x, cost, residuals(case, x),
                            case_forms(case["name"]))


def check_group(label, name, rows):
    """rows: (case, status, fig) of one group.  Prints the group's line, then
    the row assertions and the cap on rows that did not converge."""
    group = fixture()["groups"][name]
    print(tube_cert.group_line(label, group, rows))
    for case, status, fig in rows:
        if fig is not None:
            tube_cert.check_row(case, int(status), fig)
        if status not in (tube_cert.OK, tube_cert.NEAR_OPTIMAL):
            print(f"  {case['name']}: status {status} (oracle {case['oracle_status']}, "
                  f"{case['oracle_iters']} iterations)"
                  + ("" if fig is None else f" gap/cost {fig['gap'] / fig['cost_int']:.2e} "
                     f"slack/cost {fig['slack'] / fig['cost_int']:.2e}"))
    tube_cert.check_caps(group, [int(s) for _, s, _ in rows])


@pytest.fixture(scope="module")
def solved(ctx, dev):
    """mtg_tube_solve of every case, one launch per (N, r, S), computed once:
    {case name: (status, coeffs, x, cost)}."""
    import mav_tube_trajectory_generation_amd as mtg
    batches = {}
    for c in all_cases():
        batches.setdefault((c["N"], c["r"], c["S"]), []).append(c)
    out = {}
    for (n, r, S), cases in batches.items():
        pos, fv, tcp, t, radii = uniform_inputs(dev, cases)
        o = mtg.tube_solve(ctx, n, r, pos, fv, tcp, t, radii, tol=1e-10, max_iter=100)
        o = {k: v.cpu().numpy() for k, v in o.items()}
        for b, c in enumerate(cases):
            out[c["name"]] = (int(o["status"][b]), o["coeffs"][b], o["x"][b], float(o["cost"][b]))
    return out


@pytest.mark.parametrize("name", GROUPS)
def test_tube_solve_certified(solved, name):
    rows = []
    for case in fixture()["groups"][name]["cases"]:
        status, coeffs, x, cost = solved[case["name"]]
        rows.append((case, status, row_figures(case, status, coeffs, x, cost)))
    check_group(f"tube_solve {name}", name, rows)


def test_ragged_tube_solve_certified(ctx, dev):
    """One launch over rows of 2, 5, 9, 16 and 17 segments at S_max = 17, every
    input NaN beyond the row's own count."""
    import mav_tube_trajectory_generation_amd as mtg
    cases = [c for c in all_cases() if c["group"] in ("s_kernels", "runtime_s10")
             and c["S"] in RAGGED_S]
    assert sorted({c["S"] for c in cases}) == list(RAGGED_S)
    seg, pos, fv, tcp, t, radii = ragged_inputs(dev, cases, RAGGED_S_MAX)
    assert torch.isnan(t[0, cases[0]["S"]:]).all() and torch.isnan(tcp[0, cases[0]["S"]:]).all()
    o = mtg.ragged_tube_solve(ctx, 10, 4, seg, pos, fv, tcp, t, radii, tol=1e-10, max_iter=100)
    o = {k: v.cpu().numpy() for k, v in o.items()}
    rows = {"s_kernels": [], "runtime_s10": []}
    for b, c in enumerate(cases):
        S, m = c["S"], 5
        x = o["x"][b, :, :(S - 1) * m].reshape(-1)
        rows[c["group"]].append((c, int(o["status"][b]),
                                 row_figures(c, int(o["status"][b]), o["coeffs"][b, :S], x,
                                             float(o["cost"][b]))))
    for name, r in rows.items():
        check_group(f"ragged_tube_solve {name}", name, r)


def check_time_rows(label, cases, J, status):
    """J of the time objective at gradient mode 0 on the box cases: only J comes
    back, so cost = J - time_penalty (sum T)^2.  Rows with status OK:
    lower - sum lam_k 1e-8 - model_err cost <= cost <= lower + the OK bound."""
    group = fixture()["groups"]["box"]
    worst, low, hist = -np.inf, np.inf, {}
    for b, c in enumerate(cases):
        hist[int(status[b])] = hist.get(int(status[b]), 0) + 1
        if status[b] != tube_cert.OK:
            continue
        cost = J[b] - TIME_PENALTY * float(np.sum(c["times"])) ** 2
        gap = cost - c["lower"]
        worst, low = max(worst, gap / cost), min(low, gap / cost)
    print(f"{label:24s} rows {len(cases):2d} status {hist} gap/cost max {worst:.2e} min {low:.2e} "
          f"(oracle max {group['gap_floor']:.2e})")
    for b, c in enumerate(cases):
        if status[b] != tube_cert.OK:
            continue
        cost = J[b] - TIME_PENALTY * float(np.sum(c["times"])) ** 2
        lo = c["lower"] - float(np.sum(c["lam"])) * tube_cert.FEASIBILITY_BAR - c["model_err"] * cost
        hi = c["lower"] + tube_cert.ok_bound(c, group["gap_floor"], cost)
        assert lo <= cost, (c["name"], cost, c["lower"], lo)
        assert cost <= hi, (c["name"], cost, c["lower"], hi)
    tube_cert.check_caps(group, [int(s) for s in status])


def test_tube_time_cost_certified(ctx, dev):
    import mav_tube_trajectory_generation_amd as mtg
    cases = fixture()["groups"]["box"]["cases"]
    pos, fv, tcp, t, radii = uniform_inputs(dev, cases)
    out = mtg.tube_time_cost(ctx, 10, 4, pos, fv, tcp, t, radii, time_penalty=TIME_PENALTY)
    check_time_rows("tube_time_cost box", cases, out["cost"].cpu().numpy(),
                    out["status"].cpu().numpy())


def test_ragged_tube_time_cost_certified(ctx, dev):
    """The same rows in a ragged batch at S_max = 8, NaN beyond the 6 segments."""
    import mav_tube_trajectory_generation_amd as mtg
    cases = fixture()["groups"]["box"]["cases"]
    seg, pos, fv, tcp, t, radii = ragged_inputs(dev, cases, 8)
    out = mtg.ragged_tube_time_cost(ctx, 10, 4, seg, pos, fv, tcp, t, radii,
                                    time_penalty=TIME_PENALTY)
    check_time_rows("ragged_tube_time_cost box", cases, out["cost"].cpu().numpy(),
                    out["status"].cpu().numpy())
