"""Weak-duality certificate of a tube QCQP result (numpy and stdlib only).

The tube problem is  min f(x) = 1/2 x^T P x + q^T x  s.t.  g_k(x) <= 0  with
convex quadratics g_k.  For any multipliers lambda >= 0

    f(x) >= d(lambda) - sum_k lambda_k max(g_k(x), 0)        for every x,
    d(lambda) = min_y [f(y) + sum_k lambda_k g_k(y)]          (one Cholesky solve),

whatever solver produced x and however lambda was found.  The fixture
tests/golden/tube_dual.json (tests/golden/make_tube_dual.py) stores, per case,
multipliers and the bound they certify, evaluated in 50-digit arithmetic on the
assembled doubles.  The bound is stated on the cost the solvers report, the
integral of the squared r-th derivative: cost = 1/2 f(x) + c0 with c0 constant
per problem (P = 2 R_pp, qcqp_impl:497-502), so

    lower = 1/2 d(lambda) + c0 <= cost(x) + slack.

Helpers here: the cost integral from returned coefficients, the free variables
x read back from returned coefficients, the float64 d(lambda), and the gap of a
result with the slack its lower side is allowed.
"""
import json
import math
import os

import numpy as np

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tube_dual.json")
EPS = 2.0 ** -52
FEASIBILITY_BAR = 1e-8  # max g_k of an accepted solution (tests/test_tube_gpu.py)
_GL_NODES, _GL_WEIGHTS = np.polynomial.legendre.leggauss(8)  # exact to degree 15 >= 2 (N - 1 - r)


def hexes(a):
    return [float(v).hex() for v in np.asarray(a, dtype=np.float64).reshape(-1)]


def unhex(a):
    return np.array([float.fromhex(v) for v in a], dtype=np.float64)


def load(path=FIXTURE):
    """The fixture with its hex-float fields decoded: {"meta", "groups": {name:
    {"gap_floor", "cases": [case]}}}.  A case holds N, r, S, seed, times,
    times_cp [S], radii [S, 2], lam_idx, lam, lower, c0, model_err and the
    oracle's recorded figures."""
    with open(path) as fh:
        fx = json.load(fh)
    for g in fx["groups"].values():
        g["gap_floor"] = float.fromhex(g["gap_floor"])
        for c in g["cases"]:
            for k in ("times", "times_cp", "lam"):
                c[k] = unhex(c[k])
            c["radii"] = unhex(c["radii"]).reshape(c["S"], 2)
            c["lam_idx"] = np.array(c["lam_idx"], dtype=np.int64)
            for k in ("lower", "c0", "dual", "dual_f64", "oracle_cost"):
                c[k] = float.fromhex(c[k])
    return fx


def falling(i, k):
    """i (i-1) ... (i-k+1): the factor of t^(i-k) in the k-th derivative of t^i."""
    return math.prod(range(i - k + 1, i + 1))


def cost_integral(coeffs, times, r):
    """sum over segments and dimensions of int_0^T (p^(r)(t))^2 dt for coeffs
    [S, D, N] (ascending powers), exactly: the integrand is a polynomial of
    degree 2 (N - 1 - r) <= 12 and an 8-point Gauss-Legendre rule integrates it
    without truncation.  Every term w_k p^(r)(t_k)^2 is positive, so the sum does
    not cancel.  Returns (value, e): e bounds the float64 rounding, from
    |fl(p^(r)(t_k)) - p^(r)(t_k)| <= 2^-52 (4 deg + 4) sum_j |c_j| t_k^j (the
    evaluation and the rounding of the node) carried through the square and the
    weights."""
    coeffs = np.asarray(coeffs, dtype=np.float64)
    S, D, N = coeffs.shape
    assert 2 * (N - 1 - r) <= 15
    ff = np.array([falling(i, r) for i in range(r, N)], dtype=np.float64)
    deg = N - 1 - r
    total, err = [], []
    for s in range(S):
        T = float(times[s])
        t = 0.5 * T * (1.0 + _GL_NODES)
        pw = t[:, None] ** np.arange(deg + 1)[None, :]          # [nodes, deg + 1]
        w = 0.5 * T * _GL_WEIGHTS
        for d in range(D):
            c = coeffs[s, d, r:] * ff
            v = pw @ c
            va = pw @ np.abs(c)
            ev = EPS * (4 * deg + 4) * va
            total.extend(w * v * v)
            err.extend(w * (2.0 * np.abs(v) * ev + ev * ev))
    value = math.fsum(total)
    return value, math.fsum(err) + 8.0 * EPS * value


def x_from_coeffs(coeffs, times):
    """The free variables x[d][v][k] (derivative k = 0..M-1 of interior vertex
    v = 1..S-1, dimension d) read from coeffs [S, D, N]: once from the start of
    the following segment (k! a_k) and once from the end of the preceding one.
    Returns (x_start, x_end, disagreement): each [D, S-1, M]; disagreement is
    the largest |x_start - x_end| over the entries of one derivative order
    divided by that order's largest |x_start|, maximised over the orders."""
    coeffs = np.asarray(coeffs, dtype=np.float64)
    S, D, N = coeffs.shape
    M = N // 2
    xs = np.zeros((D, S - 1, M))
    xe = np.zeros((D, S - 1, M))
    for v in range(1, S):
        T = float(times[v - 1])
        for k in range(M):
            xs[:, v - 1, k] = math.factorial(k) * coeffs[v, :, k]
            terms = [coeffs[v - 1, :, i] * (falling(i, k) * T ** (i - k)) for i in range(k, N)]
            xe[:, v - 1, k] = [math.fsum(tt[d] for tt in terms) for d in range(D)]
    return xs, xe, scaled_mismatch(xs, xe)


def scaled_mismatch(ref, other):
    """max over derivative orders k of max |ref - other|[..., k] / max |ref|[..., k]."""
    ref = np.asarray(ref, dtype=np.float64)
    other = np.asarray(other, dtype=np.float64).reshape(ref.shape)
    worst = 0.0
    for k in range(ref.shape[-1]):
        scale = np.max(np.abs(ref[..., k]))
        diff = np.max(np.abs(ref[..., k] - other[..., k]))
        if diff > 0.0:
            worst = max(worst, diff / scale if scale > 0.0 else math.inf)
    return worst


def symmetrised(P):
    """1/2 (P + P^T), exact in float64 up to one rounding per entry: the
    assembled P is not symmetric (|P - P^T| up to 3e-7 on entries of 4e4), and
    the gradient and the Cholesky factor must see the matrix of 1/2 x^T P x."""
    P = np.asarray(P, dtype=np.float64)
    return 0.5 * (P + P.T)


def tube_constraint_indices(N, S):
    """Indices of the quadratic tube constraints in the reference's order
    (qcqp_impl:321-474): per segment i [sphere if i < S-1], tube j = 1..N-2,
    then 2 (N-2) half-spaces."""
    out, k = [], 0
    for i in range(S):
        k += 1 if i < S - 1 else 0
        out.extend(range(k, k + N - 2))
        k += 3 * (N - 2)
    return np.array(out, dtype=np.int64)


def forms(qp, idx):
    """What the certificate needs of an assembled problem (pyoracle.tube_assemble):
    the symmetrised P, q, and the constraint forms of the indices idx only."""
    idx = np.asarray(idx, dtype=np.int64)
    return dict(P=symmetrised(qp["P"]), q=np.asarray(qp["q"]), idx=idx,
                quad=np.ascontiguousarray(qp["quad"][idx]), lin=np.ascontiguousarray(qp["lin"][idx]),
                cst=np.ascontiguousarray(qp["cst"][idx]))


def constraint_values(fm, x):
    """g_k(x) = 1/2 x^T Q_k x + l_k^T x + c_k of the constraints held in fm, and
    e_k = 2^-52 x (number of terms) x (sum of |terms|), the float64 rounding
    bound of each."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    Q, l, c = fm["quad"], fm["lin"], fm["cst"]
    g = 0.5 * np.einsum("i,kij,j->k", x, Q, x) + l @ x + c
    ax = np.abs(x)
    mag = 0.5 * np.einsum("i,kij,j->k", ax, np.abs(Q), ax) + np.abs(l) @ ax + np.abs(c)
    count = np.count_nonzero(Q, axis=(1, 2)) + np.count_nonzero(l, axis=1) + 1
    return g, EPS * count * mag


def dual_value(fm, lam):
    """d(lambda) in float64 for multipliers lam of the constraints held in fm
    (the rest zero): A = P + sum lam_k Q_k, b = q + sum lam_k l_k,
    d = -1/2 b^T A^-1 b + lam^T c.  Returns (d, minimiser of the Lagrangian);
    (-inf, None) where A is not positive definite."""
    lam = np.asarray(lam, dtype=np.float64)
    A = fm["P"] + np.einsum("k,kij->ij", lam, fm["quad"])
    A = 0.5 * (A + A.T)
    b = fm["q"] + lam @ fm["lin"]
    try:
        L = np.linalg.cholesky(A)
    except np.linalg.LinAlgError:
        return -math.inf, None
    y = np.linalg.solve(L, b)
    return -0.5 * float(y @ y) + float(lam @ fm["cst"]), -np.linalg.solve(L.T, y)


def gap_and_slack(case, cost, e_cost, g_lam, e_lam, cap=None):
    """gap = cost - lower and the slack of its lower side,
    sum_k lam_k (max(g_k, 0) + e_k) + model_err cost + e_cost, for the
    constraint values g_lam and rounding bounds e_lam at the multipliers'
    indices.  cap: count max(g_k, 0) up to this value only (a row that also has
    to meet max g <= cap cannot use more).  The cost is 1/2 f, so half the
    multiplier term would already be valid; the whole term is what the checks
    were specified with, and the looser of two valid forms."""
    viol = np.maximum(np.asarray(g_lam, dtype=np.float64), 0.0)
    if cap is not None:
        viol = np.minimum(viol, cap)
    slack = float(case["lam"] @ (viol + e_lam)) + case["model_err"] * abs(cost) + e_cost
    return cost - case["lower"], slack


def certified_gap(case, coeffs, x, g, fm=None):
    """For a result (coeffs [S, D, N], x, constraint values g [n_con] at x):
    dict(gap, slack, slack_capped, cost_int, e_int).  gap = cost_integral(coeffs)
    - lower is the certified distance above the optimum, valid once
    -slack <= gap; slack is gap_and_slack's.  With the assembled forms fm
    (forms(qp, case["lam_idx"])) e_k is their rounding bound at x and g_k the
    larger of g's and theirs; without them e_k = 0.  slack_capped counts each
    max(g_k, 0) up to the feasibility bar 1e-8 only."""
    cost_int, e_int = cost_integral(coeffs, case["times"], case["r"])
    g_lam = np.asarray(g, dtype=np.float64).reshape(-1)[case["lam_idx"]]
    e_lam = np.zeros(len(g_lam))
    if fm is not None:
        # g may come from another restatement of the constraints (the oracle's
        # relative coordinates; its zero-snap moves values by ~1e-13): the
        # inequality is the assembled forms', so the larger of the two counts.
        g_asm, e_lam = constraint_values(fm, x)
        g_lam = np.maximum(g_lam, g_asm)
    gap, slack = gap_and_slack(case, cost_int, e_int, g_lam, e_lam)
    _, capped = gap_and_slack(case, cost_int, e_int, g_lam, e_lam, cap=FEASIBILITY_BAR)
    return dict(gap=gap, slack=slack, slack_capped=capped, cost_int=cost_int, e_int=e_int)


def ok_bound(case, gap_floor, cost):
    """The upper side of a converged row: 2 max(oracle_gap, gap_floor cost)."""
    return 2.0 * max(case["oracle_gap"], gap_floor * abs(cost))


# Row statuses (include/mtg_hip.h) and the oracle's codes for the same outcomes.
OK, NOT_SPD, NOT_CONVERGED, NEAR_OPTIMAL = 0, 2, 3, 4
FROM_ORACLE_STATUS = {0: OK, 1: NOT_CONVERGED, 3: NEAR_OPTIMAL}
CONSISTENCY_BAR = 1e-9  # the suite's kernel-to-kernel bar


def assess(case, gap_floor, coeffs, x, cost, g, fm):
    """Every figure the row checks use, for one result: certified_gap's, the
    upper bound of a converged row, cost against the integral of the returned
    coefficients, x against the vertex derivatives of the returned coefficients
    (both sides of every interior vertex) and the largest constraint value."""
    fig = certified_gap(case, coeffs, x, g, fm)
    xs, xe, _ = x_from_coeffs(coeffs, case["times"])
    xr = np.asarray(x, dtype=np.float64).reshape(xs.shape)
    fig.update(bound=ok_bound(case, gap_floor, fig["cost_int"]),
               cost_err=abs(cost - fig["cost_int"]) / fig["cost_int"],
               x_err=max(scaled_mismatch(xr, xs), scaled_mismatch(xr, xe)),
               g_max=float(np.max(g)))
    return fig


def check_row(case, status, fig):
    """The assertions on one row with a finite result.  Every status: cost, x
    and feasibility.  OK: -slack <= gap <= 2 max(oracle_gap, gap_floor cost).
    NEAR_OPTIMAL: the same lower side, and 1e3 x that upper bound (the tier's
    definition: every residual within 1e3 tol).  NOT_CONVERGED and NOT_SPD rows
    carry no gap assertion; the caller caps their number."""
    tag = (case["name"], status)
    assert fig["cost_err"] <= max(CONSISTENCY_BAR, 2.0 * case["oracle_cost_int_err"]), (tag, fig)
    assert fig["x_err"] <= max(CONSISTENCY_BAR, 2.0 * case["oracle_x_coeff_err"]), (tag, fig)
    assert fig["g_max"] <= FEASIBILITY_BAR, (tag, fig)
    if status in (OK, NEAR_OPTIMAL):
        assert -fig["slack"] <= fig["gap"], (tag, fig)
        factor = 1.0 if status == OK else 1e3
        assert fig["gap"] <= factor * fig["bound"], (tag, fig)


def check_caps(group, statuses):
    """Rows that did not converge may not outnumber the oracle's in the group
    (none where the oracle has none)."""
    bad = sum(1 for s in statuses if s not in (OK, NEAR_OPTIMAL))
    allowed = sum(1 for c in group["cases"] if c["oracle_status"] != 0)
    assert bad <= allowed, (bad, allowed, list(statuses))


def group_line(name, group, rows):
    """One line of the table: rows is a list of (case, status, fig or None)."""
    hist = {}
    for _, s, _ in rows:
        hist[int(s)] = hist.get(int(s), 0) + 1
    figs = [(c, f) for c, s, f in rows if f is not None]
    conv = [(c, f) for c, s, f in rows if f is not None and s in (OK, NEAR_OPTIMAL)]
    worst = max((f["gap"] / f["cost_int"] for _, f in conv), default=float("nan"))
    low = min((f["gap"] / f["cost_int"] for _, f in conv), default=float("nan"))
    orc = max((c["oracle_gap_rel"] for c in group["cases"] if c["oracle_status"] == 0))
    unconv = max((f["gap"] / f["cost_int"] for (c, s, f) in rows
                  if f is not None and s not in (OK, NEAR_OPTIMAL)), default=float("nan"))
    return (f"{name:24s} rows {len(rows):2d} status {hist} gap/cost max {worst:.2e} min {low:.2e} "
            f"(oracle max {orc:.2e}) unconverged gap/cost {unconv:.2e} "
            f"cost_err {max((f['cost_err'] for _, f in figs), default=float('nan')):.1e} "
            f"(oracle {max(c['oracle_cost_int_err'] for c in group['cases']):.1e}) "
            f"x_err {max((f['x_err'] for _, f in figs), default=float('nan')):.1e} "
            f"(oracle {max(c['oracle_x_coeff_err'] for c in group['cases']):.1e}) "
            f"g_max {max((f['g_max'] for _, f in figs), default=float('nan')):.1e}")
