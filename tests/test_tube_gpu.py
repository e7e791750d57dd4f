"""GPU tube QCQP (mtg_tube_residuals / mtg_tube_solve) against the oracle.

The reference solves this problem with MOSEK (qcqp_impl:476-788), which is
absent: parity of the solve is against the oracle's own interior-point method
("parity unpinned" vs MOSEK; the oracle IPM is cross-checked with SciPy in
tests/test_tube_oracle.py).  Constraint residuals are pinned to the oracle's
reference-faithful assembly of qcqp_impl:321-474.

The oracle's IPM is the kernel's own algorithm, and rows it does not converge
on are skipped below.  tests/test_tube_dual_gpu.py holds the same kernels to
a reference that depends on no solver: a weak-duality lower bound on the cost
from stored multipliers (tests/tube_cert.py, tests/golden/tube_dual.json), at
every order, every compile-time S named here, S = 17, the time box's edge
with stale control-point maps, ragged rows and the J of the time objectives.
"""
import numpy as np
import pytest

from helpers import rel_err, rel_err_coeffs

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

N, R = 10, 4
M = N // 2


def main_cpp_vertices(oracle):
    """The 4-segment geometry of src/main.cpp:26-53 (radii 0.15, :55-67)."""
    S, D = 4, 3
    mask = np.zeros((S + 1, M), np.uint8)
    vals = np.zeros((S + 1, M, D))
    pts = [(2.7, 9.5, 4.8), (3.50796, 4.34802, 4.56653), (3.95552, 3.23008, 4.75131),
           (5.06673, 2.31032, 4.79433), (7.0, 2.2, 4.8)]
    for v, p in enumerate(pts):
        mask[v, 0] = 1
        vals[v, 0] = p
    mask[0, :] = 1
    mask[S, :] = 1
    return oracle.Vertices(mask, vals)


def tube_inputs(v):
    """positions [(S+1), 3] and tube fixed values [3, N] (start derivatives
    then end derivatives, qcqp_impl:48-65)."""
    S = v.S
    pos = v.vals[:, 0, :].copy()
    fv = np.zeros((3, N))
    fv[:, :M] = v.vals[0, :M, :].T
    fv[:, M:] = v.vals[S, :M, :].T
    return pos, fv


def _gpu(ctx, dev, items, radius=0.15, times_cp=None, tol=1e-10):
    import mav_tube_trajectory_generation_amd as mtg
    B = len(items)
    S = items[0][0].S
    pos = np.stack([tube_inputs(v)[0] for v, _ in items])
    fv = np.stack([tube_inputs(v)[1] for v, _ in items])
    times = np.stack([t for _, t in items])
    tcp = times if times_cp is None else times_cp
    radii = np.full((B, S, 2), radius)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    out = mtg.tube_solve(ctx, N, R, T(pos), T(fv), T(tcp), T(times), T(radii), tol=tol,
                         max_iter=100)
    torch.cuda.synchronize()
    res = mtg.tube_residuals(ctx, N, R, T(pos), T(fv), T(tcp), T(times), T(radii), out["x"])
    o = {k: v.cpu().numpy() for k, v in out.items()}
    o["resid"] = res.cpu().numpy()
    return o


def test_main_cpp_fixture(ctx, dev, oracle):
    v = main_cpp_vertices(oracle)
    t = oracle.estimate_segment_times(v, 2.0, 2.0)  # main.cpp:73-74
    radii = np.full((4, 2), 0.15)
    ref = oracle.tube_solve(N, R, v, t, radii, tol=1e-10, max_iter=100)
    assert ref["status"] == 0
    out = _gpu(ctx, dev, [(v, t)])
    assert out["status"][0] == 0, out["status"]
    assert abs(int(out["iters"][0]) - ref["iters"]) <= 2
    assert rel_err_coeffs(out["x"][0], ref["x"]) <= 1e-6
    assert rel_err_coeffs(out["coeffs"][0], ref["coeffs"]) <= 1e-6
    assert rel_err(out["cost"][0], ref["cost"]) <= 1e-6
    # Feasible: every residual <= 0 up to the IPM tolerance.
    assert out["resid"][0].max() <= 1e-8


def test_residuals_match_oracle_assembly(ctx, dev, oracle):
    """g_k(x) of the GPU (control-point form) vs the oracle's reference-
    faithful quadratic forms (qcqp_impl:357-474) at arbitrary x."""
    import mav_tube_trajectory_generation_amd as mtg
    rng = np.random.default_rng(3)
    for S, seed in ((4, 11), (10, 105)):
        v = oracle.random_vertices(M - 1, S, 3, -10.0, 10.0, seed)
        t = oracle.estimate_segment_times(v, 3.0, 5.0)
        tcp = t * rng.uniform(0.8, 1.2, size=S)  # stale control-point map quirk
        radii = np.column_stack([rng.uniform(0.1, 0.5, S), rng.uniform(0.1, 0.5, S)])
        n = (S - 1) * M * 3
        x = rng.normal(size=n)
        ref = oracle.tube_residuals(N, R, v, t, radii, x, times_cp=tcp)
        pos, fv = tube_inputs(v)
        T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        got = mtg.tube_residuals(ctx, N, R, T(pos[None]), T(fv[None]), T(tcp[None]), T(t[None]),
                                 T(radii[None]), T(x[None])).cpu().numpy()[0]
        assert got.shape == ref.shape == (mtg.tube_num_constraints(N, S),)
        scale = np.maximum(1.0, np.abs(ref))
        assert np.max(np.abs(got - ref) / scale) <= 1e-10


def test_random_batch_vs_oracle(ctx, dev, oracle):
    """BASELINE config 3 shape (reduced batch for the oracle comparison)."""
    S, B = 10, 12
    items = []
    for b in range(B):
        v = oracle.random_vertices(M - 1, S, 3, -10.0, 10.0, 105 + b)
        items.append((v, oracle.estimate_segment_times(v, 3.0, 5.0)))
    out = _gpu(ctx, dev, items)
    radii = np.full((S, 2), 0.15)
    for b, (v, t) in enumerate(items):
        ref = oracle.tube_solve(N, R, v, t, radii, tol=1e-10, max_iter=100)
        assert out["status"][b] == ref["status"] == 0, b
        assert rel_err_coeffs(out["x"][b], ref["x"]) <= 1e-6, b
        assert rel_err_coeffs(out["coeffs"][b], ref["coeffs"]) <= 1e-6, b
        assert rel_err(out["cost"][b], ref["cost"]) <= 1e-6, b
        assert out["resid"][b].max() <= 1e-8, b


def test_stale_control_point_times(ctx, dev, oracle):
    """Inside objectiveFunctionTime the control-point maps keep the setup
    times (qcqp_impl:152-157 vs :183): times_cp != times."""
    S = 6
    v = oracle.random_vertices(M - 1, S, 3, -10.0, 10.0, 77)
    t0 = oracle.estimate_segment_times(v, 3.0, 5.0)
    t = t0 * 0.9
    radii = np.full((S, 2), 0.15)
    ref = oracle.tube_solve(N, R, v, t, radii, times_cp=t0, tol=1e-10, max_iter=100)
    out = _gpu(ctx, dev, [(v, t)], times_cp=t0[None])
    assert out["status"][0] == ref["status"] == 0
    assert rel_err_coeffs(out["coeffs"][0], ref["coeffs"]) <= 1e-6
    assert rel_err(out["cost"][0], ref["cost"]) <= 1e-6


@pytest.mark.parametrize("n,r,S", [(4, 1, 3), (6, 2, 5), (8, 3, 4), (10, 4, 2), (12, 5, 6)])
def test_polynomial_orders_vs_oracle(ctx, dev, oracle, n, r, S):
    """Every supported N: the kernel's lane organisation differs for BS =
    3 N / 2 <= 16 (row-split sums) and N = 12 (single group)."""
    import mav_tube_trajectory_generation_amd as mtg
    m = n // 2
    B = 6
    items = []
    for b in range(B):
        v = oracle.random_vertices(m - 1, S, 3, -10.0, 10.0, 300 + 7 * n + b)
        items.append((v, oracle.estimate_segment_times(v, 3.0, 5.0)))
    pos = np.stack([v.vals[:, 0, :] for v, _ in items])
    fv = np.zeros((B, 3, n))
    for b, (v, _) in enumerate(items):
        fv[b, :, :m] = v.vals[0, :m, :].T
        fv[b, :, m:] = v.vals[S, :m, :].T
    times = np.stack([t for _, t in items])
    radii = np.full((B, S, 2), 0.15)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    out = mtg.tube_solve(ctx, n, r, T(pos), T(fv), T(times), T(times), T(radii), tol=1e-10,
                         max_iter=100)
    o = {k: v.cpu().numpy() for k, v in out.items()}
    agree = 0
    for b, (v, t) in enumerate(items):
        ref = oracle.tube_solve(n, r, v, t, np.full((S, 2), 0.15), tol=1e-10, max_iter=100)
        # oracle 0 converged / 1 cap / 3 near-optimal = MTG_TRAJ_OK /
        # NOT_CONVERGED / NEAR_OPTIMAL
        assert o["status"][b] == {0: 0, 1: 3, 3: 4}[ref["status"]], b
        if ref["status"] != 0:
            continue
        agree += 1
        assert rel_err_coeffs(o["coeffs"][b], ref["coeffs"]) <= 1e-6, b
        assert rel_err(o["cost"][b], ref["cost"]) <= 1e-6, b
    assert agree >= B // 2


@pytest.mark.parametrize("S", [2, 3, 5, 7, 9, 11, 13, 16])
def test_compile_time_s_kernels_vs_oracle(ctx, dev, oracle, S):
    """tube_solve_s_kernel<10, S> (every S it is instantiated for is one of
    these or between them) against the oracle IPM on a small batch."""
    B = 3
    items = []
    for b in range(B):
        v = oracle.random_vertices(M - 1, S, 3, -10.0, 10.0, 300 + 7 * S + b)
        items.append((v, oracle.estimate_segment_times(v, 3.0, 5.0)))
    out = _gpu(ctx, dev, items)
    radii = np.full((S, 2), 0.15)
    for b, (v, t) in enumerate(items):
        ref = oracle.tube_solve(N, R, v, t, radii, tol=1e-10, max_iter=100)
        assert out["status"][b] == ref["status"], (S, b)
        if ref["status"] != 0:
            continue
        assert rel_err_coeffs(out["coeffs"][b], ref["coeffs"]) <= 1e-6, (S, b)
        assert rel_err(out["cost"][b], ref["cost"]) <= 1e-6, (S, b)


def _random_tube_batch(S, B, dev, seed0):
    """Device inputs of B random S-segment problems (the bench generator)."""
    import mav_tube_trajectory_generation_amd as mtg
    _, _, times, pos = mtg.generate_random_problems(N, 3, S, B, seed0=seed0)
    fv = np.zeros((B, 3, N))
    fv[:, :, 0] = pos[:, 0, :]
    fv[:, :, M] = pos[:, S, :]
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    return dict(positions=T(pos), fixed_vals=T(fv), times_cp=T(times), times=T(times),
                radii=torch.full((B, S, 2), 0.15, dtype=torch.float64, device=dev))


def test_two_segment_rows_ignore_stale_lds(ctx, dev):
    """An S = 2 solve does not depend on what the CU ran before.  With one
    free vertex the layout's coupling slot Po is written by nobody but the
    solve body's own zeroing (tube_solve_one, mtg_tube_device.h), and
    Tube::factor multiplies its words by 0.0: a NaN left there by an earlier
    workgroup used to become the pivot.

    The S = 2 batch is solved twice: after a benign S = 4 solve, and after an
    S = 4 solve whose vertex positions are NaN.  make_tube_layout(10, .), in
    doubles: at S = 2 Po is [144, 169) (bul 50, T 2, geo 38, fixv 30, pos 9,
    Pd 15 before it); at S = 4 the per-segment geometry is [104, 180) (bul
    100, T 4 before it), every word of it computed from the positions, so NaN
    in the second run.  LDS is not cleared between launches and B = 2048
    workgroups land on every CU several times.  The two launches allocate
    different amounts of LDS, so only a CU's first workgroup slot is certain
    to start where its predecessor's did (the ragged test of the same name has
    equal allocations); one such slot per CU is what the test needs.  The NaN batch takes the
    MTG_TRAJ_NOT_SPD path of any non-finite input (one iteration, NaN
    outputs)."""
    import mav_tube_trajectory_generation_amd as mtg
    B = 2048
    two = _random_tube_batch(2, B, dev, 9000)
    four = _random_tube_batch(4, B, dev, 9000)
    nan4 = dict(four, positions=torch.full_like(four["positions"], float("nan")))
    runs = []
    for before in (four, nan4):
        first = mtg.tube_solve(ctx, N, R, **before)
        out = mtg.tube_solve(ctx, N, R, **two)
        torch.cuda.synchronize()
        runs.append(({k: v.cpu().numpy() for k, v in first.items()},
                     {k: v.cpu().numpy() for k, v in out.items()}))
    (_, a), (poison, b) = runs
    assert (poison["status"] == 2).all() and np.isnan(poison["cost"]).all()
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    for k in ("x", "coeffs", "cost"):
        assert np.isfinite(b[k]).all(), k
