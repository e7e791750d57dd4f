"""The entry and the tail of linear_wave_kernel<10, 4, 3, S> (the `standard`
kernel): what the wave does before its first block solve and after its last.

The problem index and the row offsets are 32-bit scalar arithmetic, the input
stores carry no execution mask (spare lanes store to a junk area) and the
bad-time fills sit out of line; after the solve come the coefficient copy-out,
the cost's reduction, the status word and the optional free derivatives.  None
of that may show in a result:

  * batch sizes 1, 9 and 67 (one workgroup; remainders 1 and 3 of the
    eight-way problem index) against the oracle, and every row of the 67
    bit-equal to the same row solved alone;
  * every combination of the optional outputs gives the same bits in the
    outputs that remain;
  * rows with a bad time come out as NaN with status BAD_TIME and leave their
    neighbours' bits alone;
  * the launch that carries a deferred selection, and a captured and replayed
    launch, give the bits of the plain eager launch.

S = 2 and 3 have no forward step, 10 is the bench shape, 11 the largest S
whose end-vertex terms ride in the assembly pass and whose chains differ in
length, 12 the first with a pass of their own, 16 the largest (two fixed
values per lane).  End vertices move as in test_wave_solver_shapes_gpu.py.
"""
import functools
import itertools

import numpy as np
import pytest

from helpers import REL_TOL, compact_fixed, rel_err, rel_err_coeffs, standard_vertices

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

N, D, R, M = 10, 3, 4, 5
SHAPES = [2, 3, 10, 11, 12, 16]
BMAX = 67
OK, BAD_TIME = 0, 1


@functools.lru_cache(maxsize=None)
def _case(oracle, S):
    """(mask, d_f [67, D, n_fixed], times [67, S], oracle solutions): once
    per S, shared by the tests below (read-only)."""
    rng = np.random.default_rng(4400 + S)
    dfs, ts, refs = [], [], []
    mask = None
    for b in range(BMAX):
        v = standard_vertices(N, S, D, 4400 + 100 * S + b)
        v.vals[0, 1:M, :] = rng.uniform(-2.0, 2.0, (M - 1, D))
        v.vals[S, 1:M, :] = rng.uniform(-2.0, 2.0, (M - 1, D))
        mask, df = compact_fixed(v, N)
        t = oracle.estimate_segment_times(v, 3.0, 5.0)
        dfs.append(df)
        ts.append(t)
        refs.append(oracle.linear_solve(N, R, v, t))
    df, t = np.ascontiguousarray(dfs), np.ascontiguousarray(ts)
    df.setflags(write=False)
    t.setflags(write=False)
    return mask, df, t, refs


def _plan(ctx, S, mask):
    import mav_tube_trajectory_generation_amd as mtg
    plan = mtg.LinearPlan(ctx, N, D, R, S, mask).set_kernel("standard")
    assert plan.kernel == "standard"
    return plan


def _solve(plan, dev, df, t, **kw):
    out = plan.solve(torch.from_numpy(np.array(df)).to(dev), torch.from_numpy(np.array(t)).to(dev),
                     **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _same_bits(a, b):
    """Bit equality (NaN payloads included)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("S", SHAPES)
def test_batch_sizes(ctx, dev, oracle, S):
    mask, df, t, refs = _case(oracle, S)
    plan = _plan(ctx, S, mask)
    outs = {}
    for B in (1, 9, BMAX):
        out = outs[B] = _solve(plan, dev, df[:B], t[:B], free=True)
        assert (out["status"] == OK).all(), (S, B)
        for b in range(B):
            assert rel_err_coeffs(out["coeffs"][b], refs[b]["coeffs"]) <= REL_TOL, (S, B, b)
            assert rel_err(out["cost"][b], refs[b]["cost"]) <= REL_TOL, (S, B, b)
            assert rel_err_coeffs(out["free"][b], refs[b]["dp"]) <= REL_TOL, (S, B, b)
    full = outs[BMAX]
    for b in range(BMAX):
        one = _solve(plan, dev, df[b:b + 1], t[b:b + 1], free=True)
        for k in ("coeffs", "cost", "free", "status"):
            assert _same_bits(one[k][0], full[k][b]), (S, b, k)


@pytest.mark.parametrize("S", SHAPES)
def test_optional_outputs(ctx, dev, oracle, S):
    mask, df, t, _ = _case(oracle, S)
    plan = _plan(ctx, S, mask)
    B = 9
    full = _solve(plan, dev, df[:B], t[:B], cost=True, free=True, status=True)
    for cost, status, free in itertools.product((False, True), repeat=3):
        out = _solve(plan, dev, df[:B], t[:B], cost=cost, free=free, status=status)
        want = {"coeffs"} | {k for k, on in (("cost", cost), ("status", status), ("free", free))
                             if on}
        assert set(out) == want, (S, cost, status, free)
        for k in want:
            assert _same_bits(out[k], full[k]), (S, cost, status, free, k)


@pytest.mark.parametrize("S", SHAPES)
def test_bad_times(ctx, dev, oracle, S):
    mask, df, t, _ = _case(oracle, S)
    plan = _plan(ctx, S, mask)
    B = 9
    clean = _solve(plan, dev, df[:B], t[:B], free=True)
    assert (clean["status"] == OK).all()
    rows = {0: 0, 4: S // 2, 8: S - 1}  # row -> segment: the first, a middle, the last
    good = [b for b in range(B) if b not in rows]
    for value in (0.0, -1.5, float("nan"), float("inf")):
        tb = np.array(t[:B])
        for b, s in rows.items():
            tb[b, s] = value
        out = _solve(plan, dev, df[:B], tb, free=True)
        for b in rows:
            assert out["status"][b] == BAD_TIME, (S, value, b)
            assert np.isnan(out["coeffs"][b]).all(), (S, value, b)
            assert np.isnan(out["cost"][b]), (S, value, b)
            assert np.isnan(out["free"][b]).all(), (S, value, b)
        for k in ("coeffs", "cost", "free", "status"):
            assert _same_bits(out[k][good], clean[k][good]), (S, value, k)


def test_select_prev_same_solves(ctx, dev, oracle):
    S, B = 10, 9
    mask, df, t, _ = _case(oracle, S)
    plan = _plan(ctx, S, mask)
    fd, td = torch.from_numpy(np.array(df[:B])).to(dev), torch.from_numpy(np.array(t[:B])).to(dev)
    first = plan.solve(fd, td, free=True)
    out = {"coeffs": torch.full_like(first["coeffs"], float("nan")),
           "cost": torch.full_like(first["cost"], float("nan")),
           "free": torch.full_like(first["free"], float("nan")),
           "status": torch.full_like(first["status"], -1)}
    triple = torch.full((3,), float("nan"), dtype=torch.float64, device=dev)
    plan.solve_select_prev(fd, td, out, prev_cost=first["cost"], prev_start=40, rank=2,
                           prev_triple=triple)
    torch.cuda.synchronize()
    for k in first:
        assert _same_bits(out[k].cpu().numpy(), first[k].cpu().numpy()), k
    c = first["cost"].cpu().numpy()
    j = int(np.argmin(c))
    assert tuple(triple.cpu().numpy()) == (c[j], 40.0 + j, 2.0)


def test_graph_replay(ctx, dev, oracle):
    S, B = 10, 9
    mask, df, t, _ = _case(oracle, S)
    plan = _plan(ctx, S, mask)
    fd, td = torch.from_numpy(np.array(df[:B])).to(dev), torch.from_numpy(np.array(t[:B])).to(dev)
    eager = {k: v.clone() for k, v in plan.solve(fd, td, free=True).items()}
    torch.cuda.synchronize()
    out = {k: torch.zeros_like(v) for k, v in eager.items()}
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        plan.solve(fd, td, free=True, out=out)
    for _ in range(2):
        for v in out.values():
            v.fill_(0)
        g.replay()
        torch.cuda.synchronize()
        for k in eager:
            assert _same_bits(out[k].cpu().numpy(), eager[k].cpu().numpy()), k
