"""Exact (rational-arithmetic) fixtures for the kernels of the standard shape:
N = 10, r = 4, D = 3, the standard pattern with moving end vertices.

make_exact.py covers every (N, r) at S = 6, D = 1, where AUTO never selects
wave::Solver<10, 4, 3, S>, `lane` or `lane_pair`.  The cases here are those
kernels' shape, one S per kernel path, at the times the time optimisers hand
them: the box [0.1, 2 T0] and its edges, where the reference algorithm in
FP64 (the oracle) drifts up to 4e-3 from the true minimiser and cannot serve
as the target.  Per case: the exact coefficients, free derivatives and cost;
for S <= 7 the exact time-allocation objective J and its two gradient forms;
and the oracle's own error on each, which sets the bound a kernel must meet
("at least as accurate as the reference algorithm in FP64").

The oracle's cost (<= 5e-9) and the backward error of its d_p (<= 6e-10; 4e-8
with one 0.15 s segment) stay sharp in every regime; only its coefficients
degrade with the conditioning.

Run: python tests/golden/make_exact_std.py   (under a minute on 8 cores, CPU only)
"""
import json
import multiprocessing
import os
import sys
from fractions import Fraction as F

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(HERE, "..", "..", "oracle"), os.path.join(HERE, ".."), HERE]
import helpers  # noqa: E402
import pyoracle  # noqa: E402
from make_exact import exact_R, exact_coeffs, exact_solution  # noqa: E402

N, R_ORD, D, M = 10, 4, 3, 5
INC, W_D, W_T, PENALTY = 0.1, 0.1, 1.0, 500.0
FIXTURE = os.path.join(HERE, "exact_std.json")
T_MIN = 0.1  # kOptimizationTimeLowerBound: the box is [T_MIN, 2 T0]

ALL_REGIMES = ("nominal", "edge_even", "edge_odd", "all_min", "geometric", "fd_low")
# S -> regimes.  Each S is a kernel path (see test_wave_solver_shapes_gpu.py):
# 2, 3 no forward step; 4 even; 7 odd; 11 the last S with the end terms in the
# assembly lanes; 12 end terms in their own pass and the last S of the lane
# kernels; 16 the last compile-time-S wave kernel; 17 the runtime-S kernel.
# fd_low matters to the time objective only (S <= 7).  To keep the file
# small, S = 11 and 12 share all_min and geometric between them (they differ
# in the end terms only) and S = 16, 17 keep the nominal and one edge regime.
CASES = {
    2: ALL_REGIMES, 3: ALL_REGIMES, 4: ALL_REGIMES, 7: ALL_REGIMES,
    11: ("nominal", "edge_even", "edge_odd", "geometric"),
    12: ("nominal", "edge_even", "edge_odd", "all_min"),
    16: ("nominal", "edge_even"), 17: ("nominal", "edge_odd"),
}
TIME_COST_MAX_S = 7


def vertices(S):
    """The standard pattern with derivatives 1..4 at the first and the last
    vertex drawn uniform in [-2, 2] (test_wave_solver_shapes_gpu._vertices)."""
    v = helpers.standard_vertices(N, S, D, 3100 + S)
    rng = np.random.default_rng(3100 + S)
    v.vals[0, 1:M, :] = rng.uniform(-2.0, 2.0, (M - 1, D))
    v.vals[S, 1:M, :] = rng.uniform(-2.0, 2.0, (M - 1, D))
    return v


def regime_times(T0, regime):
    S = len(T0)
    s = np.arange(S)
    if regime == "nominal":
        return T0.copy()
    if regime == "edge_even":
        return np.where(s % 2 == 0, T_MIN, 2.0 * T0)
    if regime == "edge_odd":
        return np.where(s % 2 == 1, T_MIN, 2.0 * T0)
    if regime == "all_min":
        return np.full(S, T_MIN)
    if regime == "geometric":  # 0.1 s .. 25 s
        return T_MIN * 250.0 ** (s / (S - 1))
    if regime == "fd_low":  # the lower central-difference point is 0.05
        t = T0.copy()
        t[S // 2] = 0.15
        return t
    raise ValueError(regime)


def fd_time(Tn, hi):
    """fd_time of mtg_time_device.h, in the FP64 the kernels evaluate it in."""
    return T_MIN if Tn <= T_MIN else (Tn + INC if hi else Tn - INC)


def vertices_of(case):
    """pyoracle.Vertices of a stored case (mask, compact d_f)."""
    mask = np.array(case["mask"], np.uint8)
    df = np.array(case["df"])
    vals = np.zeros(mask.shape + (D,))
    vals[mask.astype(bool)] = df.T
    return pyoracle.Vertices(mask, vals)


def all_derivs(mask, df, free):
    """Every vertex derivative [D][(S+1) M] as the Fractions of the FP64
    numbers given: compact d_f [D, n_f] and free values [D, n_p], both in
    (vertex, derivative) order."""
    fixed = np.asarray(mask).reshape(-1).astype(bool)
    xs = []
    for d in range(len(df)):
        x = np.zeros(fixed.size)
        x[fixed] = df[d]
        x[~fixed] = free[d]
        xs.append([F(float(a)) for a in x])
    return xs


def backward_error(Rm, fr, xs):
    """Scaled backward error of the free rows of R x = 0, evaluated exactly:
    max over (dimension, free row i) of |sum_j R_ij x_j| / sum_j |R_ij x_j|."""
    worst = F(0)
    for x in xs:
        for i in fr:
            terms = [Rm[i][j] * x[j] for j in range(len(x)) if Rm[i][j] != 0]
            den = sum(abs(t) for t in terms)
            if den:
                worst = max(worst, abs(sum(terms)) / den)
    return float(worst)


def free_indices(mask):
    return [i for i, f in enumerate(np.asarray(mask).reshape(-1)) if not f]


def exact_J(v, times, cache):
    """Exact objective cost + PENALTY (sum T)^2 at FP64 times."""
    key = tuple(map(float, times))
    if key not in cache:
        cost = exact_solution(N, R_ORD, v.mask, v.vals, times)["cost"]
        cache[key] = cost + F(PENALTY) * sum(F(t) for t in key) ** 2
    return cache[key]


def exact_time_cost(v, times, sol):
    """(J, grad_mode 2 gradient, grad_mode 1 gradient), exact, rounded once.
    Mode 2: central differences of the re-solved J.  Mode 1: the reference's
    w_d (d^T R(T+) d - d^T R(T-) d) / (2 inc) + w_t with d held at the exact
    solution; only segment n's block of R moves."""
    cache = {tuple(map(float, times)): sol["cost"] + F(PENALTY) * sum(F(float(t)) for t in times) ** 2}
    J = exact_J(v, times, cache)
    two_inc = 2 * F(INC)
    g2, g1 = [], []
    for n, Tn in enumerate(map(float, times)):
        lo, hi = np.array(times, float), np.array(times, float)
        lo[n], hi[n] = fd_time(Tn, 0), fd_time(Tn, 1)
        g2.append(float((exact_J(v, hi, cache) - exact_J(v, lo, cache)) / two_inc))
        Hlo, Hhi = exact_R(N, R_ORD, [lo[n]])[0], exact_R(N, R_ORD, [hi[n]])[0]
        dq = F(0)
        for x in sol["x"]:
            e = x[n * M:(n + 2) * M]
            dq += sum(e[a] * (Hhi[a][b] - Hlo[a][b]) * e[b] for a in range(N) for b in range(N))
        g1.append(float(F(W_D) * dq / two_inc + F(W_T)))
    return float(J), g2, g1


def grad_err(g, g_exact):
    g, g_exact = np.asarray(g), np.asarray(g_exact)
    num = float(np.max(np.abs(g - g_exact)))
    return num / max(float(np.max(np.abs(g_exact))), 1e-300) if num else 0.0


def oracle_figures(case, Rm=None):
    """The oracle's error on every stored quantity of a case."""
    v = vertices_of(case)
    t = np.array(case["times"])
    if Rm is None:
        Rm = exact_R(N, R_ORD, t)[0]
    o = pyoracle.linear_solve(N, R_ORD, v, t)
    fig = dict(
        oracle_err=helpers.rel_err_coeffs(o["coeffs"], np.array(case["coeffs"])),
        oracle_cost_err=helpers.rel_err(o["cost"], case["cost"]),
        oracle_dp_err=helpers.rel_err_coeffs(o["dp"], np.array(case["dp"])),
        oracle_resid=backward_error(Rm, free_indices(case["mask"]),
                                    all_derivs(case["mask"], np.array(case["df"]), o["dp"])))
    if "J" in case:
        kw = dict(time_penalty=PENALTY, increment=INC, w_d=W_D, w_t=W_T)
        J, g2 = pyoracle.time_cost(N, R_ORD, v, t, grad_mode=2, **kw)
        _, g1 = pyoracle.time_cost(N, R_ORD, v, t, grad_mode=1, **kw)
        fig.update(oracle_J_err=helpers.rel_err(J, case["J"]),
                   oracle_grad_err=grad_err(g2, case["grad2"]),
                   oracle_grad1_err=grad_err(g1, case["grad1"]))
    return fig


def make_case(S, regime):
    v = vertices(S)
    T0 = pyoracle.estimate_segment_times(v, 3.0, 5.0)
    t = regime_times(T0, regime)
    mask, df = helpers.compact_fixed(v, N)
    sol = exact_solution(N, R_ORD, v.mask, v.vals, t)
    case = dict(S=S, regime=regime, mask=mask.tolist(), df=df.tolist(),
                times=list(map(float, t)), coeffs=exact_coeffs(N, sol).tolist(),
                dp=[[float(x[i]) for i in sol["fr"]] for x in sol["x"]],
                cost=float(sol["cost"]))
    if S <= TIME_COST_MAX_S:
        case["J"], case["grad2"], case["grad1"] = exact_time_cost(v, t, sol)
    case.update(oracle_figures(case, sol["R"]))
    return case


def _make_case(args):
    return make_case(*args)


def main():
    todo = [(S, regime) for S, regimes in CASES.items() for regime in regimes]
    # the cases are independent and exact, so the pool changes no digit
    with multiprocessing.Pool(min(8, os.cpu_count() or 1)) as pool:
        cases = pool.map(_make_case, todo, chunksize=1)
    for c in cases:
        print(c["S"], c["regime"],
              *(f"{k[7:]}={c[k]:.1e}" for k in c if k.startswith("oracle_")), flush=True)
    floor = max(c["oracle_resid"] for c in cases if c["regime"] == "nominal")
    # the mask and d_f of an S are the same in every regime: stored once
    problems = {str(c["S"]): dict(mask=c["mask"], df=c["df"]) for c in cases}
    for c in cases:
        del c["mask"], c["df"]
    with open(FIXTURE, "w") as f:
        json.dump({"generator": "tests/golden/make_exact_std.py", "N": N, "r": R_ORD, "D": D,
                   "increment": INC, "w_d": W_D, "w_t": W_T, "time_penalty": PENALTY,
                   "resid_floor": floor, "problems": problems, "cases": cases}, f,
                  separators=(",", ":"))


def load_fixture():
    """exact_std.json with each case's mask and d_f put back."""
    with open(FIXTURE) as f:
        fx = json.load(f)
    for c in fx["cases"]:
        c.update(fx["problems"][str(c["S"])])
    return fx


if __name__ == "__main__":
    main()
