"""Ragged batches on the GPU (mtg_ragged_linear_solve / _time_cost /
_time_optimize, RaggedLinearPlan): trajectories of different segment counts
in one launch against the CPU oracle per trajectory.

Inputs are random_vertices(N/2-1, S_b, D, -10, 10, seed) with
estimate_segment_times(v, 3, 5); padded inputs are NaN (pack_ragged) and
outputs are pre-filled with a poison value, so a kernel reading or skipping
padding shows.  Tolerances: helpers.REL_TOL against the oracle, 1e-9 kernel
against kernel, 1e-6 time-cost value, 1e-4 gradients; Subplex
evaluation count and result code exact, its T and cost 1e-6.
"""
import ctypes
import functools

import numpy as np
import pytest

from helpers import REL_TOL, check_path, rel_err, rel_err_coeffs, standard_vertices

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

POISON = -7.25e77
OK, BAD_TIME, BAD_SEGMENTS = 0, 1, 5


@functools.lru_cache(maxsize=None)
def _problem(N, D, r, S, seed):
    """(vertices, times, oracle solve) of one standard-pattern trajectory;
    computed once and shared (callers do not modify it)."""
    import pyoracle
    v = standard_vertices(N, S, D, seed)
    t = pyoracle.estimate_segment_times(v, 3.0, 5.0)
    return v, t, pyoracle.linear_solve(N, r, v, t)


def _batch(N, D, r, counts, seed0, S_max, dev):
    import mav_tube_trajectory_generation_amd as mtg
    probs = [_problem(N, D, r, s, seed0 + b) for b, s in enumerate(counts)]
    seg, fixed, times = mtg.pack_ragged([(p[2]["df"], p[1]) for p in probs], N, dev, S_max=S_max)
    return probs, seg, fixed, times


def _poisoned_out(plan, B, dev):
    return {"coeffs": torch.full((B, plan.S_max, plan.D, plan.N), POISON, dtype=torch.float64,
                                 device=dev),
            "cost": torch.full((B,), POISON, dtype=torch.float64, device=dev),
            "free": torch.full((B, plan.D, plan.np_max), POISON, dtype=torch.float64,
                               device=dev),
            "status": torch.full((B,), -99, dtype=torch.int32, device=dev)}


def _check_rows(plan, probs, counts, out):
    """Every row against its oracle solve, padding exactly 0.0, no NaN."""
    N, MF = plan.N, plan.N // 2 - 1
    coeffs = out["coeffs"].cpu().numpy()
    cost = out["cost"].cpu().numpy()
    free = out["free"].cpu().numpy()
    status = out["status"].cpu().numpy()
    assert not np.isnan(coeffs).any() and not np.isnan(cost).any() and not np.isnan(free).any()
    for b, (s, (v, t, ref)) in enumerate(zip(counts, probs)):
        assert status[b] == OK, (b, status[b])
        err = rel_err_coeffs(coeffs[b, :s], ref["coeffs"])
        print(f"row {b} S={s}: coeff err {err:.3e} cost err {rel_err(cost[b], ref['cost']):.3e}")
        assert err <= REL_TOL, (b, s, err)
        assert rel_err(cost[b], ref["cost"]) <= REL_TOL, (b, s, cost[b], ref["cost"])
        check_path(v, coeffs[b, :s], t, N)
        assert np.all(coeffs[b, s:] == 0.0), (b, s)
        np_b = (s - 1) * MF
        assert ref["dp"].shape == (plan.D, np_b)
        if np_b:
            scale = np.max(np.abs(ref["dp"]))
            assert np.max(np.abs(free[b, :, :np_b] - ref["dp"])) <= REL_TOL * scale, (b, s)
        assert np.all(free[b, :, np_b:] == 0.0), (b, s)


MIXED = (10, 3, 4, 12, (1, 2, 3, 12, 2, 5, 1), 105)


@pytest.fixture(scope="module")
def mixed(ctx, dev):
    """Test 1's launch, shared with the selection test."""
    import mav_tube_trajectory_generation_amd as mtg
    N, D, r, S_max, counts, seed0 = MIXED
    probs, seg, fixed, times = _batch(N, D, r, counts, seed0, S_max, dev)
    plan = mtg.RaggedLinearPlan(ctx, N, D, r, S_max)
    out = plan.solve(seg, fixed, times, free=True, out=_poisoned_out(plan, len(counts), dev))
    torch.cuda.synchronize()
    return plan, probs, counts, out


def test_mixed_counts_vs_oracle(mixed):
    """S = 1 (no system), S = 2 (one middle vertex: the twisted elimination
    with no chain step), odd and even chains, a row without padding,
    neighbours of different length."""
    plan, probs, counts, out = mixed
    assert plan.nf_max == 10 + 12 - 1 and plan.np_max == 11 * 4
    _check_rows(plan, probs, counts, out)


@pytest.mark.parametrize("N,D,r,S_max,counts", [(8, 2, 3, 5, (5, 1, 4, 2)),
                                                (10, 1, 2, 6, (2, 6, 3)),
                                                (12, 3, 4, 4, (4, 1, 3))])
def test_other_instantiations(ctx, dev, N, D, r, S_max, counts):
    import mav_tube_trajectory_generation_amd as mtg
    probs, seg, fixed, times = _batch(N, D, r, counts, 300, S_max, dev)
    plan = mtg.RaggedLinearPlan(ctx, N, D, r, S_max)
    out = plan.solve(seg, fixed, times, free=True, out=_poisoned_out(plan, len(counts), dev))
    torch.cuda.synchronize()
    _check_rows(plan, probs, counts, out)


def test_more_than_one_pass_per_wave(ctx, dev):
    """S_max = 64: D * nf = 219 fixed values and 64 times per wave, the
    assembly rows beyond the first 64, LDS above the 64 KiB default."""
    import mav_tube_trajectory_generation_amd as mtg
    N, D, r, S_max, counts = 10, 3, 4, 64, (64, 1, 33)
    probs, seg, fixed, times = _batch(N, D, r, counts, 400, S_max, dev)
    plan = mtg.RaggedLinearPlan(ctx, N, D, r, S_max)
    out = plan.solve(seg, fixed, times, free=True, out=_poisoned_out(plan, len(counts), dev))
    torch.cuda.synchronize()
    _check_rows(plan, probs, counts, out)


@pytest.mark.parametrize("S", [2, 7, 12])
def test_agrees_with_uniform_kernel(ctx, dev, S):
    import mav_tube_trajectory_generation_amd as mtg
    N, D, r, B = 10, 3, 4, 5
    mask, fixed, times, _ = mtg.generate_random_problems(N, D, S, B, seed0=500)
    fd, td = torch.from_numpy(fixed).to(dev), torch.from_numpy(times).to(dev)
    uni = mtg.LinearPlan(ctx, N, D, r, S, mask).set_kernel("standard").solve(fd, td, free=True)
    plan = mtg.RaggedLinearPlan(ctx, N, D, r, S)
    seg = torch.full((B,), S, dtype=torch.int32, device=dev)
    rag = plan.solve(seg, fd, td, free=True)
    torch.cuda.synchronize()
    cu, cr = uni["coeffs"].cpu().numpy(), rag["coeffs"].cpu().numpy()
    for b in range(B):
        assert rel_err_coeffs(cr[b], cu[b]) <= 1e-9, (S, b)
        assert rel_err(rag["cost"][b].item(), uni["cost"][b].item()) <= 1e-9, (S, b)
    fu, fr = uni["free"].cpu().numpy(), rag["free"].cpu().numpy()
    assert np.max(np.abs(fr - fu)) <= 1e-9 * np.max(np.abs(fu))
    assert torch.equal(rag["status"], uni["status"])


def test_bad_rows_stay_in_their_row(ctx, dev):
    """Counts outside [1, S_max] and a zero time: NaN over the row's whole
    padded extent, the neighbours and the guard regions untouched."""
    import mav_tube_trajectory_generation_amd as mtg
    N, D, r, S_max = 10, 3, 4, 12
    counts = [3, 0, 13, 4, -1]
    B = len(counts)
    plan = mtg.RaggedLinearPlan(ctx, N, D, r, S_max)
    good = {0: _problem(N, D, r, 3, 600), 3: _problem(N, D, r, 4, 603)}
    fixed = np.full((B, D, plan.nf_max), np.nan)
    times = np.full((B, S_max), np.nan)
    for b, (v, t, ref) in good.items():
        fixed[b, :, :ref["df"].shape[1]] = ref["df"]
        times[b, :len(t)] = t
    times[3, 1] = 0.0
    seg = torch.tensor(counts, dtype=torch.int32, device=dev)
    G = 2  # guard rows after each buffer
    full = _poisoned_out(plan, B + G, dev)
    out = plan.solve(seg, torch.from_numpy(fixed).to(dev), torch.from_numpy(times).to(dev),
                     free=True, out={k: v[:B] for k, v in full.items()})
    torch.cuda.synchronize()
    status = out["status"].cpu().numpy()
    assert status.tolist() == [OK, BAD_SEGMENTS, BAD_SEGMENTS, BAD_TIME, BAD_SEGMENTS]
    coeffs, cost, free = (out[k].cpu().numpy() for k in ("coeffs", "cost", "free"))
    for b in (1, 2, 3, 4):
        assert np.isnan(coeffs[b]).all() and np.isnan(free[b]).all() and np.isnan(cost[b]), b
    v, t, ref = good[0]
    assert rel_err_coeffs(coeffs[0, :3], ref["coeffs"]) <= REL_TOL
    assert rel_err(cost[0], ref["cost"]) <= REL_TOL
    assert np.all(coeffs[0, 3:] == 0.0) and np.all(free[0, :, 8:] == 0.0)
    assert np.max(np.abs(free[0, :, :8] - ref["dp"])) <= REL_TOL * np.max(np.abs(ref["dp"]))
    for k in ("coeffs", "cost", "free"):
        assert torch.all(full[k][B:] == POISON), k
    assert torch.all(full["status"][B:] == -99)


def test_graph_replay_with_other_counts(ctx, dev):
    """The launch holds no host knowledge of the counts: captured once,
    replayed over another mix written in place."""
    import mav_tube_trajectory_generation_amd as mtg
    N, D, r, S_max = 10, 3, 4, 12
    first, second = (4, 9, 1, 12, 2), (12, 1, 6, 2, 11)
    _, seg, fixed, times = _batch(N, D, r, first, 700, S_max, dev)
    plan = mtg.RaggedLinearPlan(ctx, N, D, r, S_max)
    out = _poisoned_out(plan, len(first), dev)
    plan.solve(seg, fixed, times, free=True, out=out)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        plan.solve(seg, fixed, times, free=True, out=out)
    probs2, seg2, fixed2, times2 = _batch(N, D, r, second, 720, S_max, dev)
    seg.copy_(seg2)
    fixed.copy_(fixed2)
    times.copy_(times2)
    for v in out.values():
        v.fill_(POISON if v.dtype == torch.float64 else -99)
    g.replay()
    torch.cuda.synchronize()
    _check_rows(plan, probs2, second, out)


def test_selection_across_counts(mixed, dev):
    """mtg_select_local over the ragged cost vector, one row NaN: numpy's
    NaN-ignoring argmin."""
    from mav_tube_trajectory_generation_amd import lib
    from mav_tube_trajectory_generation_amd._abi import check
    _, _, _, out = mixed
    cost = torch.cat([out["cost"], torch.tensor([float("nan")], dtype=torch.float64, device=dev)])
    cost = cost[torch.tensor([0, 1, 7, 2, 3, 4, 5, 6], device=dev)].contiguous()  # NaN inside
    triple = torch.empty(3, dtype=torch.float64, device=dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    check(lib().mtg_select_local(ctypes.c_void_p(cost.data_ptr()), cost.numel(), 1000, 3,
                                 ctypes.c_void_p(triple.data_ptr()), stream), "mtg_select_local")
    c = cost.cpu().numpy()
    j = int(np.nanargmin(c))
    assert triple.cpu().tolist() == [c[j], 1000.0 + j, 3.0]


TIME_CASES = [(3, 4, 16, (2, 3, 7, 16, 4, 1), 800), (2, 3, 6, (5, 2), 850)]


@pytest.mark.parametrize("D,r,S_max,counts,seed0", TIME_CASES, ids=["D3r4", "D2r3"])
def test_time_cost_vs_oracle(ctx, dev, oracle, D, r, S_max, counts, seed0):
    import mav_tube_trajectory_generation_amd as mtg
    N = 10
    probs, seg, fixed, times = _batch(N, D, r, counts, seed0, S_max, dev)
    plan = mtg.RaggedLinearPlan(ctx, N, D, r, S_max)
    for grad_mode in (0, 1, 2):
        out = plan.time_cost(seg, fixed, times, grad_mode=grad_mode, increment=0.1, w_d=0.1,
                             w_t=1.0)
        cost, status = out["cost"].cpu().numpy(), out["status"].cpu().numpy()
        grad = out["grad"].cpu().numpy() if grad_mode else None
        for b, (s, (v, t, _)) in enumerate(zip(counts, probs)):
            if s == 1:
                assert status[b] == BAD_SEGMENTS and np.isnan(cost[b]), (b, status[b], cost[b])
                assert grad is None or np.isnan(grad[b]).all()
                continue
            J, g = oracle.time_cost(N, r, v, t, grad_mode=grad_mode, increment=0.1, w_d=0.1,
                                    w_t=1.0)
            assert status[b] == OK, (b, status[b])
            print(f"mode {grad_mode} row {b} S={s}: J err {rel_err(cost[b], J):.3e}")
            assert rel_err(cost[b], J) <= 1e-6, (grad_mode, b, cost[b], J)
            if grad_mode:
                gerr = np.max(np.abs(grad[b, :s] - g)) / np.max(np.abs(g))
                print(f"    grad err {gerr:.3e}")
                assert gerr <= 1e-4, (grad_mode, b, grad[b, :s], g)
                assert np.all(grad[b, s:] == 0.0), (grad_mode, b)


@pytest.mark.parametrize("D,r,S_max,counts,seed0", TIME_CASES, ids=["D3r4", "D2r3"])
@pytest.mark.parametrize("E", [30, 50])
def test_time_optimize_sbplx_vs_oracle(ctx, dev, oracle, D, r, S_max, counts, seed0, E):
    import mav_tube_trajectory_generation_amd as mtg
    N = 10
    probs, seg, fixed, times = _batch(N, D, r, counts, seed0, S_max, dev)
    plan = mtg.RaggedLinearPlan(ctx, N, D, r, S_max)
    out = plan.time_optimize(seg, fixed, times, max_evals=E, optimizer="sbplx")
    o = {k: v.cpu().numpy() for k, v in out.items()}
    t_in = times.cpu().numpy()
    for b, (s, (v, t, _)) in enumerate(zip(counts, probs)):
        # bit-identical padding (NaN payloads included)
        assert np.array_equal(o["times"][b, s:].view(np.int64), t_in[b, s:].view(np.int64)), b
        if s == 1:
            assert o["status"][b] == BAD_SEGMENTS and np.isnan(o["cost"][b])
            assert np.array_equal(o["times"][b].view(np.int64), t_in[b].view(np.int64))
            assert o["evals"][b] == 0 and o["solves"][b] == 0 and o["result"][b] == -1
            continue
        Tc, fc, ec, rc, _ = oracle.time_optimize_sbplx(N, r, v, t, E)
        print(f"E={E} row {b} S={s}: evals {o['evals'][b]}/{ec} result {o['result'][b]}/{rc} "
              f"T err {np.max(np.abs(o['times'][b, :s] - Tc) / Tc):.3e} "
              f"cost err {rel_err(o['cost'][b], fc):.3e}")
        assert o["status"][b] == OK
        assert o["evals"][b] == ec and o["result"][b] == rc, (b, o["evals"][b], ec, rc)
        assert o["solves"][b] == o["evals"][b]
        assert np.max(np.abs(o["times"][b, :s] - Tc) / Tc) <= 1e-6, (b, o["times"][b, :s], Tc)
        assert rel_err(o["cost"][b], fc) <= 1e-6, (b, o["cost"][b], fc)


def test_time_optimize_descent_vs_oracle(ctx, dev, oracle):
    import mav_tube_trajectory_generation_amd as mtg
    N, D, r, S_max, counts, E = 10, 3, 4, 16, (2, 5, 9), 20
    probs, seg, fixed, times = _batch(N, D, r, counts, 900, S_max, dev)
    plan = mtg.RaggedLinearPlan(ctx, N, D, r, S_max)
    out = plan.time_optimize(seg, fixed, times, max_evals=E)
    o = {k: v.cpu().numpy() for k, v in out.items()}
    t_in = times.cpu().numpy()
    for b, (s, (v, t, _)) in enumerate(zip(counts, probs)):
        Tc, fc, ec = oracle.time_optimize(N, r, v, t, E)
        assert o["status"][b] == OK
        assert o["evals"][b] == ec, (b, o["evals"][b], ec)
        assert o["result"][b] == (5 if ec >= E else 4)
        assert np.max(np.abs(o["times"][b, :s] - Tc) / Tc) <= 1e-6, (b, o["times"][b, :s], Tc)
        assert rel_err(o["cost"][b], fc) <= 1e-6, (b, o["cost"][b], fc)
        assert np.array_equal(o["times"][b, s:].view(np.int64), t_in[b, s:].view(np.int64)), b


def test_time_entries_unsupported(ctx, dev):
    """Soft and hard constraints, and N, r, D outside the time kernels, are
    MTG_ERR_UNSUPPORTED (-4); so is S_max = 65 with a live context."""
    import mav_tube_trajectory_generation_amd as mtg
    N, D, r, S_max, counts = 10, 3, 4, 6, (2, 6)
    _, seg, fixed, times = _batch(N, D, r, counts, 950, S_max, dev)
    plan = mtg.RaggedLinearPlan(ctx, N, D, r, S_max)
    with pytest.raises(mtg.MTGError, match=r"\(-4\)"):
        plan.time_optimize(seg, fixed, times, max_evals=10, soft=[(1, 3.0)])
    with pytest.raises(mtg.MTGError, match=r"\(-4\)"):
        plan.time_cost(seg, fixed, times, soft=[(1, 3.0)])
    with pytest.raises(mtg.MTGError, match=r"\(-4\)"):
        plan.time_cost(seg, fixed, times, soft=[(1, 3.0)], hard=True)
    _, seg8, fixed8, times8 = _batch(8, 2, 3, (2, 3), 960, 3, dev)
    with pytest.raises(mtg.MTGError, match=r"\(-4\)"):
        mtg.RaggedLinearPlan(ctx, 8, 2, 3, 3).time_cost(seg8, fixed8, times8)
    with pytest.raises(mtg.MTGError, match=r"\(-4\)"):
        mtg.RaggedLinearPlan(ctx, N, D, r, 65)
    with pytest.raises(mtg.MTGError, match=r"\(-1\)"):
        mtg.RaggedLinearPlan(ctx, N, D, r, 0)
    with pytest.raises(mtg.MTGError):
        plan.solve(seg.to(torch.int64), fixed, times)      # counts must be int32
    with pytest.raises(mtg.MTGError):
        plan.solve(seg, fixed[:, :, :-1].contiguous(), times)


def test_plan_outlives_context(dev):
    """The plan keeps a copy of the device id: destroying it after its
    context touches no freed memory (it owns nothing on the device)."""
    import mav_tube_trajectory_generation_amd as mtg
    c = mtg.Context(0)
    plan = mtg.RaggedLinearPlan(c, 10, 3, 4, 12)
    assert (plan.nf_max, plan.np_max) == (21, 44)
    c.close()
    plan.close()
