"""Every instantiation of wave::Solver<10, 4, 3, S> (mtg_wave_device.h), S =
2..16, with moving end vertices, against the oracle.

Each S is its own kernel.  The end-vertex terms ride in the assembly pass's
spare lanes up to S = 11 and keep a pass of their own from S = 12; the
backward chain adds its middle-vertex terms into the forward chain's slot in
the same step (S even) or one step later (S odd); S = 2 and 3 have no forward
step.  createRandomVertices fixes the end derivatives to zero, so the stock
generator never reaches the end terms: the cases here draw them at random, as
test_standard_kernels_nonzero_end_derivatives does.
"""
import functools

import numpy as np
import pytest

from helpers import REL_TOL, compact_fixed, rel_err, rel_err_coeffs, standard_vertices

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

N, D, R, M = 10, 3, 4, 5


def _vertices(S, B, seed0):
    """B standard-pattern vertex sets with random non-zero derivatives
    1..M-1 at the start and the end vertex."""
    rng = np.random.default_rng(seed0)
    vs = []
    for b in range(B):
        v = standard_vertices(N, S, D, seed0 + b)
        v.vals[0, 1:M, :] = rng.uniform(-2.0, 2.0, (M - 1, D))
        v.vals[S, 1:M, :] = rng.uniform(-2.0, 2.0, (M - 1, D))
        vs.append(v)
    return vs


@functools.lru_cache(maxsize=None)
def _linear_case(oracle, S):
    """(mask, d_f [B, D, n_fixed], times [B, S], oracle solutions), computed
    once per S and shared by the tests below (read-only)."""
    B = 5
    dfs, ts, refs = [], [], []
    mask = None
    for v in _vertices(S, B, 8100 + 16 * S):
        mask, df = compact_fixed(v, N)
        t = oracle.estimate_segment_times(v, 3.0, 5.0)
        dfs.append(df)
        ts.append(t)
        refs.append(oracle.linear_solve(N, R, v, t))
    return mask, np.ascontiguousarray(dfs), np.ascontiguousarray(ts), refs


def _check(out, refs, tag):
    assert (out["status"] == 0).all(), tag
    for b, ref in enumerate(refs):
        assert rel_err_coeffs(out["coeffs"][b], ref["coeffs"]) <= REL_TOL, (tag, b)
        assert rel_err(out["cost"][b], ref["cost"]) <= REL_TOL, (tag, b)
        assert rel_err_coeffs(out["free"][b], ref["dp"]) <= REL_TOL, (tag, b)


@pytest.mark.parametrize("S", range(2, 17))
def test_linear_every_s_moving_ends(ctx, dev, oracle, S):
    """linear_wave_kernel<10, 4, 3, S, false>: coefficients, cost and free
    derivatives against the oracle, REL_TOL."""
    import mav_tube_trajectory_generation_amd as mtg
    mask, df, t, refs = _linear_case(oracle, S)
    plan = mtg.LinearPlan(ctx, N, D, R, S, mask).set_kernel("standard")
    assert plan.kernel == "standard"
    out = plan.solve(torch.from_numpy(df).to(dev), torch.from_numpy(t).to(dev), free=True)
    torch.cuda.synchronize()
    _check({k: v.cpu().numpy() for k, v in out.items()}, refs, S)


@pytest.mark.parametrize("S", [10, 12])
def test_linear_select_prev_moving_ends(ctx, dev, oracle, S):
    """linear_wave_kernel<10, 4, 3, S, true> (the launch that carries the
    previous step's selection in an extra workgroup): the same solves, and the
    selection of the costs of a first launch."""
    import mav_tube_trajectory_generation_amd as mtg
    mask, df, t, refs = _linear_case(oracle, S)
    B = len(refs)
    plan = mtg.LinearPlan(ctx, N, D, R, S, mask).set_kernel("standard")
    assert plan.kernel == "standard"
    fd, td = torch.from_numpy(df).to(dev), torch.from_numpy(t).to(dev)
    first = plan.solve(fd, td, free=True)
    out = {"coeffs": torch.full_like(first["coeffs"], float("nan")),
           "cost": torch.full_like(first["cost"], float("nan")),
           "free": torch.full_like(first["free"], float("nan")),
           "status": torch.full_like(first["status"], -1)}
    triple = torch.full((3,), float("nan"), dtype=torch.float64, device=dev)
    plan.solve_select_prev(fd, td, out, prev_cost=first["cost"], prev_start=100, rank=3,
                           prev_triple=triple)
    torch.cuda.synchronize()
    _check({k: v.cpu().numpy() for k, v in out.items()}, refs, S)
    c = first["cost"].cpu().numpy()
    j = int(np.argmin(c))
    assert tuple(triple.cpu().numpy()) == (c[j], 100.0 + j, 3.0)
    assert B == c.shape[0]


@pytest.mark.parametrize("S", [3, 11, 12])
def test_time_cost_moving_ends(ctx, dev, oracle, S):
    """time_cost_wave_kernel<10, 4, 3, S> (the same Solver::solve inside the
    time-allocation objective): objective and mode-2 gradient against the
    oracle, the bounds of test_time_cost_wave_kernels_every_s."""
    import mav_tube_trajectory_generation_amd as mtg
    B = 4
    vs = _vertices(S, B, 9300 + 16 * S)
    dfs, ts = [], []
    mask = None
    for v in vs:
        mask, df = compact_fixed(v, N)
        dfs.append(df)
        ts.append(oracle.estimate_segment_times(v, 3.0, 5.0))
    df, t = np.ascontiguousarray(dfs), np.ascontiguousarray(ts)
    plan = mtg.LinearPlan(ctx, N, D, R, S, mask)
    out = plan.time_cost(torch.from_numpy(df).to(dev), torch.from_numpy(t).to(dev),
                         grad_mode=2, increment=0.1, w_d=0.1, w_t=1.0)
    cost = out["cost"].cpu().numpy()
    grad = out["grad"].cpu().numpy()
    assert (out["status"].cpu().numpy() == 0).all()
    for b, v in enumerate(vs):
        J, g = oracle.time_cost(N, R, v, t[b], grad_mode=2, increment=0.1, w_d=0.1, w_t=1.0)
        # oracle parity; badly scaled times are held to exact values in
        # test_linear_exact_gpu.py::test_time_cost_vs_exact
        tol = 1e-9 if t[b].min() > 0.5 else 1e-6
        assert rel_err(cost[b], J) <= tol, (S, b)
        assert np.max(np.abs(grad[b] - g)) <= 1e-5 * np.max(np.abs(g)) + 1e-9, (S, b)
