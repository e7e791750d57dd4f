"""Dual certificates for the tube QCQP (tests/tube_cert.py states the bound).

Every GPU tube test compares the kernel with the oracle's interior-point
method, the same algorithm.  This generator produces a reference that depends
on no solver: per case multipliers lambda >= 0 and the lower bound d(lambda)
they certify, evaluated in 50-digit arithmetic on the assembled doubles taken
as exact data.  How lambda was found (NNLS on the active set at the oracle's x,
then L-BFGS-B ascent on the concave d) does not enter the bound's validity.

Per case the file holds the inputs that are not regenerated at test time
(times, times_cp, radii as hex floats; the vertices come from
random_vertices(N/2-1, S, 3, -10, 10, seed)), the nonzero multipliers, the
bound `lower` on the cost (rounded down to a double), c0 and model_err of the
relation cost = 1/2 f + c0, and the oracle's own certified figures at tol
1e-10, which set the bound a kernel must meet.  Per group, gap_floor is the
largest oracle_gap / cost over the group's cases the oracle converged on.

Cases (the smallest shapes that reach every code path):
  orders       (N, r, S) = (4,1,3), (6,2,5), (8,3,4), (10,4,2), (12,5,6)
  s_kernels    N = 10, S = 2, 3, 5, 7, 9, 11, 13, 16 (compile-time S)
  runtime_s10  N = 10, S = 17 (the first S past the compile-time set)
  box          N = 10, S = 6, seeds 780..783, control-point maps at T0:
               (a) times = T0 u, u ~ U[0.5, 1.8] of default_rng(0) drawn seed
               after seed, clipped to [0.1, 2 T0]; (b) even segments 0.1 s,
               odd segments 2 T0 (the corners LN_SBPLX visits)
  radii        N = 10, S = 4, seed 11, r1 and r2 ~ U[0.1, 0.5] of default_rng(3)
Seeds 300 and 301 and radius 0.15 unless stated.

Run: python tests/golden/make_tube_dual.py   (under a minute on 8 cores, CPU only)
"""
import json
import math
import multiprocessing
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(HERE, "..", "..", "oracle"), os.path.join(HERE, "..")]
import pyoracle  # noqa: E402
import tube_cert  # noqa: E402

FIXTURE = os.path.join(HERE, "tube_dual.json")
DPS = 50
TOL, MAX_ITER = 1e-10, 100
RADIUS = 0.15
T_MIN = 0.1


def case_specs():
    specs = []
    for n, r, S in ((4, 1, 3), (6, 2, 5), (8, 3, 4), (10, 4, 2), (12, 5, 6)):
        for seed in (300, 301):
            specs.append(dict(group="orders", N=n, r=r, S=S, seed=seed, kind="nominal"))
    for S in (2, 3, 5, 7, 9, 11, 13, 16):
        for seed in (300, 301):
            specs.append(dict(group="s_kernels", N=10, r=4, S=S, seed=seed, kind="nominal"))
    for seed in (300, 301):
        specs.append(dict(group="runtime_s10", N=10, r=4, S=17, seed=seed, kind="nominal",
                          need_status0=True))
    rng = np.random.default_rng(0)
    for seed in range(780, 784):
        specs.append(dict(group="box", N=10, r=4, S=6, seed=seed, kind="box_a",
                          u=rng.uniform(0.5, 1.8, 6)))
        specs.append(dict(group="box", N=10, r=4, S=6, seed=seed, kind="box_b"))
    specs.append(dict(group="radii", N=10, r=4, S=4, seed=11, kind="radii"))
    return specs


def vertices(N, S, seed):
    return pyoracle.random_vertices(N // 2 - 1, S, 3, -10.0, 10.0, seed)


def inputs(spec, seed):
    """(v, times, times_cp, radii) of a case."""
    N, S = spec["N"], spec["S"]
    v = vertices(N, S, seed)
    t0 = pyoracle.estimate_segment_times(v, 3.0, 5.0)
    radii = np.full((S, 2), RADIUS)
    times = t0.copy()
    if spec["kind"] == "box_a":
        times = np.clip(t0 * spec["u"], T_MIN, 2.0 * t0)
    elif spec["kind"] == "box_b":
        times = np.where(np.arange(S) % 2 == 0, T_MIN, 2.0 * t0)
    elif spec["kind"] == "radii":
        rng = np.random.default_rng(3)
        radii = np.column_stack([rng.uniform(0.1, 0.5, S), rng.uniform(0.1, 0.5, S)])
    return v, times, t0, radii


def multipliers(qp, x):
    """lambda >= 0 [n_con]: NNLS of the stationarity equation on the active set
    g_k > -1e-4 max(1, |c_k|) at x, then L-BFGS-B ascent on d over the same
    set; the better of the two by d."""
    from scipy.optimize import minimize, nnls
    P, q = tube_cert.symmetrised(qp["P"]), qp["q"]
    Qk, lk, ck = qp["quad"], qp["lin"], qp["cst"]
    g = 0.5 * np.einsum("i,kij,j->k", x, Qk, x) + lk @ x + ck
    idx = np.where(g > -1e-4 * np.maximum(1.0, np.abs(ck)))[0]
    fm = tube_cert.forms(qp, idx)
    Jg = np.einsum("kij,j->ki", fm["quad"], x) + fm["lin"]
    lam0, _ = nnls(Jg.T, -(P @ x + q), maxiter=50 * len(idx) + 1000)
    best, d_best = lam0, tube_cert.dual_value(fm, lam0)[0]
    scale = max(1.0, abs(0.5 * x @ P @ x + q @ x))

    def neg(la):
        d, y = tube_cert.dual_value(fm, la)
        if y is None:
            return 1e300, np.zeros(len(la))
        gy = 0.5 * np.einsum("i,kij,j->k", y, fm["quad"], y) + fm["lin"] @ y + fm["cst"]
        return -d / scale, -gy / scale

    res = minimize(neg, lam0, jac=True, method="L-BFGS-B", bounds=[(0.0, None)] * len(idx),
                   options=dict(maxiter=500, ftol=1e-16, gtol=1e-14))
    d_res = tube_cert.dual_value(fm, res.x)[0]
    if d_res > d_best:
        best, d_best = np.maximum(res.x, 0.0), d_res
    lam = np.zeros(len(ck))
    lam[idx] = best
    return lam


def mp_objective(fm, x, dps=DPS):
    """f(x) = 1/2 x^T P x + q^T x in dps-digit arithmetic on the doubles."""
    import mpmath as mp
    mp.mp.dps = dps
    xv = [mp.mpf(float(v)) for v in x]
    n = len(xv)
    P = fm["P"]
    f = mp.mpf(0)
    for i in range(n):
        row = mp.fsum(mp.mpf(float(P[i, j])) * xv[j] for j in range(n) if P[i, j] != 0.0)
        f += xv[i] * (row / 2 + mp.mpf(float(fm["q"][i])))
    return f


def mp_dual(fm, lam, dps=DPS):
    """d(lambda) in dps-digit arithmetic on the doubles of fm and lam (the
    multipliers of fm's constraints), or None where A = P + sum lam_k Q_k is
    not positive definite (the Cholesky factorisation is the proof that the
    Lagrangian is bounded below)."""
    import mpmath as mp
    mp.mp.dps = dps
    n = len(fm["q"])
    A = mp.matrix(n, n)
    P = fm["P"]
    for i in range(n):
        for j in range(n):
            if P[i, j] != 0.0:
                A[i, j] = mp.mpf(float(P[i, j]))
    b = mp.matrix([mp.mpf(float(v)) for v in fm["q"]])
    cst = mp.mpf(0)
    for k, lk in enumerate(lam):
        if lk == 0.0:
            continue
        lm = mp.mpf(float(lk))
        Q = fm["quad"][k]
        # the quadratic form only sees the symmetric part of Q_k
        for i, j in zip(*np.nonzero(Q)):
            h = lm * mp.mpf(float(Q[i, j])) / 2
            A[int(i), int(j)] += h
            A[int(j), int(i)] += h
        for i in np.nonzero(fm["lin"][k])[0]:
            b[int(i)] += lm * mp.mpf(float(fm["lin"][k][i]))
        cst += lm * mp.mpf(float(fm["cst"][k]))
    try:
        L = mp.cholesky(A)
    except (ValueError, ZeroDivisionError):
        return None
    # forward substitution L y = b;  d = -1/2 |y|^2 + lam^T c
    y = mp.matrix(n, 1)
    for i in range(n):
        s = b[i] - mp.fsum(L[i, j] * y[j] for j in range(i))
        y[i] = s / L[i, i]
    return -mp.fsum(v * v for v in y) / 2 + cst


def mp_cost_integral(coeffs, times, r, dps=DPS):
    """The cost integral of double coefficients in dps-digit arithmetic."""
    import mpmath as mp
    mp.mp.dps = dps
    S, D, N = coeffs.shape
    total = mp.mpf(0)
    for s in range(S):
        T = mp.mpf(float(times[s]))
        for d in range(D):
            c = [mp.mpf(float(coeffs[s, d, i])) * tube_cert.falling(i, r) for i in range(r, N)]
            for i, ci in enumerate(c):
                for j, cj in enumerate(c):
                    total += ci * cj * T ** (i + j + 1) / (i + j + 1)
    return total


def down(v):
    """The largest double <= the multi-precision value v."""
    f = float(v)
    import mpmath as mp
    return math.nextafter(f, -math.inf) if mp.mpf(f) > v else f


def solve(spec, seed, tol):
    v, times, tcp, radii = inputs(spec, seed)
    return pyoracle.tube_solve(spec["N"], spec["r"], v, times, radii, times_cp=tcp, tol=tol,
                               max_iter=MAX_ITER)


def make_case(spec):
    import mpmath as mp
    mp.mp.dps = DPS
    pyoracle.lib()
    N, r, S = spec["N"], spec["r"], spec["S"]
    seed, tried = spec["seed"], []
    while True:
        sol = solve(spec, seed, TOL)
        tried.append(seed)
        if sol["status"] == 0 or not spec.get("need_status0"):
            break
        assert len(tried) < 5, f"no converged seed among {tried}"
        seed += 2  # the group's two cases start at 300 and 301: stay on one's own parity
    v, times, tcp, radii = inputs(spec, seed)
    qp = pyoracle.tube_assemble(N, r, v, times, radii, times_cp=tcp)
    asym = float(np.max(np.abs(qp["P"] - qp["P"].T)))
    x = sol["x"]
    lam = multipliers(qp, x)
    idx = np.nonzero(lam)[0]
    fm = tube_cert.forms(qp, idx)
    del qp
    d = mp_dual(fm, lam[idx])
    assert d is not None, (spec, "A is not positive definite")
    d64 = tube_cert.dual_value(fm, lam[idx])[0]
    # cost = 1/2 f + c0: c0 at the solution and at a second point
    cint = mp_cost_integral(sol["coeffs"], times, r)
    c0 = cint - mp_objective(fm, x) / 2
    sol2 = solve(spec, seed, 1e-4)
    c0_2 = mp_cost_integral(sol2["coeffs"], times, r) - mp_objective(fm, sol2["x"]) / 2
    model_err = float(abs(c0 - c0_2) / cint)
    lower = d / 2 + c0
    xs, xe, _ = tube_cert.x_from_coeffs(sol["coeffs"], times)
    ref = x.reshape(xs.shape)
    x_err = max(tube_cert.scaled_mismatch(ref, xs), tube_cert.scaled_mismatch(ref, xe))
    ci64, _ = tube_cert.cost_integral(sol["coeffs"], times, r)
    # the oracle's own result through the check the kernels get: its gap may be
    # negative only within the slack (a cap-stopped x sits 1e-13 outside)
    probe = dict(lam=lam[idx], lam_idx=idx, lower=down(lower), model_err=model_err, times=times, r=r)
    g_res = pyoracle.tube_residuals(N, r, v, times, radii, x, times_cp=tcp)
    chk = tube_cert.certified_gap(probe, sol["coeffs"], x, g_res, fm)
    assert -chk["slack"] <= chk["gap"], (spec, chk)
    name = f"{spec['group']}_N{N}_S{S}_seed{seed}" + {"box_a": "_a", "box_b": "_b"}.get(spec["kind"], "")
    out = dict(
        name=name, group=spec["group"], kind=spec["kind"], N=N, r=r, S=S, seed=seed,
        seeds_tried=tried, n=int(len(x)), n_con=int(len(lam)),
        times=tube_cert.hexes(times), times_cp=tube_cert.hexes(tcp), radii=tube_cert.hexes(radii),
        lam_idx=[int(k) for k in idx], lam=tube_cert.hexes(lam[idx]),
        dual=float(d).hex(), dual_f64=float(d64).hex(),
        dual_f64_dev=float(abs(mp.mpf(d64) - d) / max(abs(d), 1)),
        lower=down(lower).hex(), c0=float(c0).hex(), model_err=model_err,
        p_asymmetry=asym,
        oracle_status=int(sol["status"]), oracle_iters=int(sol["iters"]),
        oracle_cost=float(sol["cost"]).hex(),
        oracle_gap=float(cint - lower),
        oracle_gap_rel=float((cint - lower) / cint),
        oracle_cost_int_err=float(abs(mp.mpf(sol["cost"]) - cint) / cint),
        oracle_cost_int_f64_err=float(abs(mp.mpf(ci64) - cint) / cint),
        oracle_x_coeff_err=float(x_err), oracle_slack=float(chk["slack"]),
        oracle_g_max=float(g_res.max()),
    )
    print(f"{name:34s} st {sol['status']} it {sol['iters']:3d} n {len(x):3d} nlam {len(idx):3d} "
          f"cost {float(cint):.6e} gap/cost {out['oracle_gap_rel']:.2e} model {model_err:.1e} "
          f"d64dev {out['dual_f64_dev']:.1e} costerr {out['oracle_cost_int_err']:.1e} "
          f"xerr {x_err:.1e}", flush=True)
    return out


def main():
    specs = case_specs()
    pyoracle.lib()  # build before the workers start
    with multiprocessing.Pool(min(8, os.cpu_count() or 1)) as pool:
        cases = pool.map(make_case, specs, chunksize=1)
    groups = {}
    for c in cases:
        groups.setdefault(c["group"], dict(gap_floor=0.0, cases=[]))["cases"].append(c)
    for name, g in groups.items():
        conv = [c["oracle_gap_rel"] for c in g["cases"] if c["oracle_status"] == 0]
        assert conv, f"group {name}: the oracle converged on no case"
        g["gap_floor"] = float(max(conv)).hex()
    meta = dict(generator="tests/golden/make_tube_dual.py", dps=DPS, oracle_tol=TOL,
                oracle_max_iter=MAX_ITER,
                note="lower <= cost integral of any feasible x; see tests/tube_cert.py")
    enc = lambda o: json.dumps(o, separators=(",", ":"))  # noqa: E731
    with open(FIXTURE, "w") as fh:  # one case per line
        fh.write('{"meta":' + enc(meta) + ',\n"groups":{\n')
        for gi, (name, g) in enumerate(groups.items()):
            fh.write(f'"{name}":{{"gap_floor":{enc(g["gap_floor"])},"cases":[\n')
            fh.write(",\n".join(enc(c) for c in g["cases"]))
            fh.write("\n]}" + (",\n" if gi + 1 < len(groups) else "\n"))
        fh.write("}}\n")
    print(f"wrote {FIXTURE}: {len(cases)} cases, {os.path.getsize(FIXTURE)} bytes")


if __name__ == "__main__":
    main()
