"""The status word of linear_wave_kernel<10, 4, 3, S> (the `standard` kernel)
at the edges of its pivot test.

The kernel reports NOT_SPD when some pivot of a block solve is <= 0 and not a
NaN.  It reads that off the signed minimum of the pivots' high words and looks
at the pivots themselves only when that minimum is not positive
(stdp::PivotWords); the time kernels keep the FP64 minimum.  What could go
wrong is the status, so that is what is pinned here, at the smallest shapes
that reach each path of Solver::solve:

  S = 2   no sweep step, the middle block only
  S = 3   odd: the forward chain is shorter than the backward chain (a lane
          that skips a step keeps that step's pivots at 1.0)
  S = 10  the bench instantiation
  S = 12  the end-vertex terms in a pass of their own

  * well-posed problems: status 0, coefficients and cost against the oracle;
  * a NaN or an infinity in a fixed value: the pivots depend on the times
    alone, so the row's status stays 0 while its cost and the coefficients the
    value enters are not finite, and the other rows keep their bits;
  * a segment time of 1e-3 or 1e3 (inside the accepted range, pivots spread
    over many orders of magnitude): the status, cost and coefficients of the
    generic kernel on the same input.  Both inputs were first solved on the
    CPU with the oracle alone, at all four S: it reports them solvable
    (status 0, every coefficient and the cost finite), which the test
    asserts again.  The extreme time sits in an end segment, whose far vertex
    is fully fixed: the free vertex's block is then H11(T) of that one
    segment up to a diagonal scaling, entries from 1e15 to 1e-3 at T = 1e-3,
    and well conditioned.  Between two free vertices a segment 1e3 times
    shorter than its neighbours gives the free-free system a condition
    number of about (1e3)^(2r-1) = 1e21, past FP64: there no two FP64
    algorithms agree (tried at S = 3 with 1e-3 in the middle segment: equal
    status 0, but the two kernels' coefficients 9e2 apart in relative terms),
    so that is not a case;
  * a zero, a negative and a NaN time: BAD_TIME, the pivot code is not
    reached, the other rows keep their bits;
  * a captured and twice replayed S = 10 launch gives the eager launch's bits.
"""
import functools

import numpy as np
import pytest

from helpers import REL_TOL, compact_fixed, rel_err, rel_err_coeffs, standard_vertices

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

N, D, R, M = 10, 3, 4, 5
SHAPES = [2, 3, 10, 12]
B = 8
OK, BAD_TIME = 0, 1
POISON_ROW, POISON_DIM, POISON_FIXED = 3, 1, M  # the position of vertex 1
SMALL_ROW, LARGE_ROW = 2, 5


@functools.lru_cache(maxsize=None)
def _case(oracle, S):
    """(mask, d_f [8, D, n_fixed], times [8, S], vertices, oracle solutions)
    of createRandomVertices, seeds 105.., once per S (read-only)."""
    dfs, ts, vs, refs = [], [], [], []
    mask = None
    for b in range(B):
        v = standard_vertices(N, S, D, 105 + b)
        mask, df = compact_fixed(v, N)
        t = oracle.estimate_segment_times(v, 3.0, 5.0)
        dfs.append(df)
        ts.append(t)
        vs.append(v)
        refs.append(oracle.linear_solve(N, R, v, t))
    df, t = np.ascontiguousarray(dfs), np.ascontiguousarray(ts)
    df.setflags(write=False)
    t.setflags(write=False)
    return mask, df, t, vs, refs


def edge_times(t, S):
    """The case's times with 1e-3 in the last segment of one row and 1e3 in
    the first segment of another."""
    te = np.array(t)
    te[SMALL_ROW, S - 1] = 1e-3
    te[LARGE_ROW, 0] = 1e3
    return te


def _plan(ctx, S, mask, kernel="standard"):
    import mav_tube_trajectory_generation_amd as mtg
    plan = mtg.LinearPlan(ctx, N, D, R, S, mask).set_kernel(kernel)
    assert plan.kernel == kernel
    return plan


def _solve(plan, dev, df, t):
    out = plan.solve(torch.from_numpy(np.array(df)).to(dev), torch.from_numpy(np.array(t)).to(dev))
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("S", SHAPES)
def test_well_posed(ctx, dev, oracle, S):
    mask, df, t, _, refs = _case(oracle, S)
    out = _solve(_plan(ctx, S, mask), dev, df, t)
    assert (out["status"] == OK).all(), (S, out["status"])
    for b, ref in enumerate(refs):
        assert rel_err_coeffs(out["coeffs"][b], ref["coeffs"]) <= REL_TOL, (S, b)
        assert rel_err(out["cost"][b], ref["cost"]) <= REL_TOL, (S, b)


@pytest.mark.parametrize("S", SHAPES)
def test_non_finite_fixed_value(ctx, dev, oracle, S):
    mask, df, t, _, _ = _case(oracle, S)
    plan = _plan(ctx, S, mask)
    clean = _solve(plan, dev, df, t)
    others = [b for b in range(B) if b != POISON_ROW]
    for value in (float("nan"), float("inf"), float("-inf")):
        dfp = np.array(df)
        dfp[POISON_ROW, POISON_DIM, POISON_FIXED] = value
        out = _solve(plan, dev, dfp, t)
        assert out["status"][POISON_ROW] == OK, (S, value)
        assert not np.isfinite(out["cost"][POISON_ROW]), (S, value)
        # segment 1 starts at vertex 1: its c_0 is the value itself, and the
        # free derivatives of the vertex carry it into the rest
        assert not np.isfinite(out["coeffs"][POISON_ROW, 1, POISON_DIM, 0]), (S, value)
        assert not np.isfinite(out["coeffs"][POISON_ROW, 0, POISON_DIM]).all(), (S, value)
        for k in ("coeffs", "cost", "status"):
            assert _same_bits(out[k][others], clean[k][others]), (S, value, k)


@pytest.mark.parametrize("S", SHAPES)
def test_edge_times(ctx, dev, oracle, S):
    mask, df, t, vs, _ = _case(oracle, S)
    te = edge_times(t, S)
    for b in (SMALL_ROW, LARGE_ROW):
        ref = oracle.linear_solve(N, R, vs[b], te[b])
        assert ref["status"] == 0 and np.isfinite(ref["coeffs"]).all() and np.isfinite(ref["cost"])
    wave = _solve(_plan(ctx, S, mask), dev, df, te)
    gen = _solve(_plan(ctx, S, mask, "generic"), dev, df, te)
    for b in range(B):
        ec = rel_err_coeffs(wave["coeffs"][b], gen["coeffs"][b])
        ej = rel_err(wave["cost"][b], gen["cost"][b])
        print(f"S={S} row {b}: status {wave['status'][b]} / {gen['status'][b]} "
              f"coeffs {ec:.3e} cost {ej:.3e}")
    assert (wave["status"] == gen["status"]).all(), (S, wave["status"], gen["status"])
    for b in range(B):
        assert rel_err_coeffs(wave["coeffs"][b], gen["coeffs"][b]) <= REL_TOL, (S, b)
        assert rel_err(wave["cost"][b], gen["cost"][b]) <= REL_TOL, (S, b)


@pytest.mark.parametrize("S", SHAPES)
def test_bad_times(ctx, dev, oracle, S):
    mask, df, t, _, _ = _case(oracle, S)
    plan = _plan(ctx, S, mask)
    clean = _solve(plan, dev, df, t)
    rows = {1: 0, 6: S - 1}  # row -> segment
    good = [b for b in range(B) if b not in rows]
    for value in (0.0, -1.5, float("nan")):
        tb = np.array(t)
        for b, s in rows.items():
            tb[b, s] = value
        out = _solve(plan, dev, df, tb)
        for b in rows:
            assert out["status"][b] == BAD_TIME, (S, value, b)
            assert np.isnan(out["coeffs"][b]).all() and np.isnan(out["cost"][b]), (S, value, b)
        for k in ("coeffs", "cost", "status"):
            assert _same_bits(out[k][good], clean[k][good]), (S, value, k)


def test_graph_replay(ctx, dev, oracle):
    S = 10
    mask, df, t, _, _ = _case(oracle, S)
    plan = _plan(ctx, S, mask)
    fd, td = torch.from_numpy(np.array(df)).to(dev), torch.from_numpy(np.array(t)).to(dev)
    eager = {k: v.clone() for k, v in plan.solve(fd, td).items()}
    torch.cuda.synchronize()
    assert (eager["status"] == OK).all()
    out = {k: torch.zeros_like(v) for k, v in eager.items()}
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        plan.solve(fd, td, out=out)
    for _ in range(2):
        for v in out.values():
            v.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        for k in eager:
            assert _same_bits(out[k].cpu().numpy(), eager[k].cpu().numpy()), k
