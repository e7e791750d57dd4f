"""The collision-driven objectives and their projected L-BFGS over ragged
batches (mtg_ragged_coll_cost / mtg_ragged_coll_optimize): rows of 2..6
segments (ragged_coll_fixture.py) in rows padded to S_max = 7, against the
oracle row by row, against the uniform entries per count, and for what the
ragged layout adds: independence of the padding, of the row order, of S_max,
of the workspace's contents and of the near field, bad rows between guard
rows, graph replay over other counts, and the device chain from the ragged
tube solve to the selection."""
import ctypes

import numpy as np
import pytest

import ragged_coll_fixture as F
from coll_fixture import coll_params, forest_map
from helpers import compact_fixed, rel_err
from ragged_coll_fixture import M, N, R
from test_coll_gpu import VARIANTS

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

S_MAX = 7
BAD_SEGMENTS, BAD_TIME = 5, 1


def _T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _prm(**kw):
    import mav_tube_trajectory_generation_amd as mtg
    return mtg.make_coll_params(**coll_params(**kw))


@pytest.fixture(scope="module")
def occ(dev):
    return _T(forest_map(), dev)


def _pack(dev, rows, S_max, mode, fill=np.nan, pk=None):
    pk = F.pack(rows, S_max, mode, fill) if pk is None else pk
    return {k: _T(v, dev) for k, v in pk.items()}


def _cost(ctx, t, occ, prm, mode, S_max, **kw):
    import mav_tube_trajectory_generation_amd as mtg
    out = mtg.ragged_coll_cost(ctx, kw.pop("N", N), kw.pop("R", R), t["seg_counts"],
                               t["fixed_vals"], t["x"], t["times"] if mode == 0 else None, occ,
                               prm, mode=mode, S_max=S_max, **kw)
    return {k: v.cpu().numpy() for k, v in out.items()}


def _opt(ctx, t, occ, prm, mode, S_max, **kw):
    import mav_tube_trajectory_generation_amd as mtg
    out = mtg.ragged_coll_optimize(ctx, N, R, t["seg_counts"], t["fixed_vals"], t["x"],
                                   t["times"] if mode == 0 else None, occ, prm, mode=mode,
                                   S_max=S_max, **kw)
    return {k: v.cpu().numpy() for k, v in out.items()}


def _bounds(dev, rows, S_max, mode, fill=np.nan):
    P = F.paths()
    return {name: _T(np.array([F.pad_x(a, P[i]["S"], S_max, mode, fill)
                               for (i, _), a in zip(rows, arrs)]), dev)
            for name, arrs in zip(("lower", "upper", "initial_step"), F.opt_bounds(rows, mode))}


def _check_cost_row(got, b, S, S_max, mode, ref, prm):
    """One row against (J, grad, terms, collision) with the tolerances of
    test_coll_gpu.test_coll_cost_vs_oracle; the grad padding is exactly 0.0."""
    J, g, terms, c = ref
    inc = prm.get("increment_time", 1e-6)
    tol_g = 1e-8 if inc >= 0.05 else 1e-6
    tol_t = 1e-3 if inc < 1e-3 else tol_g
    assert got["status"][b] == 0
    assert got["collision"][b] == c, b
    assert rel_err(got["cost"][b], J) <= 1e-9, (b, got["cost"][b], J)
    assert np.max(np.abs(got["terms"][b] - terms)) <= 1e-9 * max(np.max(np.abs(terms)), 1e-12)
    row = got["grad"][b].reshape(-1)
    assert np.all(row[F.padding_mask(S, S_max, mode)] == 0.0), b
    gg = F.unpad_x(row, S, S_max, mode)
    off = S if mode else 0
    dg = np.abs(gg - g)
    assert np.max(dg[off:]) <= tol_g * max(np.max(np.abs(g)), 1e-12), (b, dg)
    if off:
        assert np.max(dg[:off]) <= tol_t * max(np.max(np.abs(g[:off])), 1e-12), (b, dg[:off])


# ------------------------------------------------------------ cost vs oracle
@pytest.mark.parametrize("variant", ["main", "central", "soft", "raise_last"])
@pytest.mark.parametrize("mode", [0, 1])
def test_cost_vs_oracle(ctx, dev, oracle, occ, mode, variant):
    """Every row is oracle.coll_cost on the row's own path: J, gradient, terms
    and the collision flag, with a per-row raise reference."""
    P = F.paths()
    prm = coll_params(**VARIANTS[variant])
    rows = F.cost_rows(mode)
    B = len(rows)
    assert B <= 16
    raise_ref = np.linspace(1.0, 100.0, B)
    got = _cost(ctx, _pack(dev, rows, S_MAX, mode), occ, _prm(**VARIANTS[variant]), mode, S_MAX,
                raise_ref=_T(raise_ref, dev))
    n_coll = 0
    for b, (i, x) in enumerate(rows):
        ref = oracle.coll_cost(N, R, P[i]["vt"], P[i]["t"], mode, x, forest_map(), prm,
                               raise_ref=raise_ref[b])
        _check_cost_row(got, b, P[i]["S"], S_MAX, mode, ref, prm)
        n_coll += ref[3]
    assert 0 < n_coll < B, n_coll  # both outcomes are exercised


def test_cost_vs_oracle_order_8(ctx, dev, oracle, occ):
    """N = 8 (M = 4, r = 3), mode 1 with central differences: counts 2, 3, 4."""
    import pyoracle
    from coll_fixture import perturbed_starts
    n, r, m = 8, 3, 4
    prm = coll_params(**VARIANTS["central"])
    occ_np = forest_map()
    probs, n_coll = [], 0
    for pos in F.path_positions()[:3]:
        S = len(pos) - 1
        mask = np.zeros((S + 1, m), np.uint8)
        vals = np.zeros((S + 1, m, 3))
        mask[0, :] = mask[S, :] = 1
        mask[1:S, 0] = 1
        vals[:, 0, :] = pos
        v = pyoracle.Vertices(mask, vals)
        t = np.asarray(pyoracle.estimate_segment_times(v, 2.0, 2.0))
        x0 = pyoracle.tube_solve(n, r, v, t, np.full((S, 2), 0.15))["x"]
        tm = mask.copy()
        tm[1:S, :] = 0
        vt = pyoracle.Vertices(tm, vals)
        _, df = compact_fixed(vt, n)
        for k, x in enumerate([x0] + perturbed_starts(x0, 1, 0.02, seed=5 + S)):
            probs.append((S, vt, t, df, np.concatenate([t * (1.0 + 0.03 * k), x])))
    B, np_max = len(probs), (S_MAX - 1) * m
    X = np.full((B, S_MAX + 3 * np_max), np.nan)
    for b, (S, _, _, _, x) in enumerate(probs):
        X[b, :S] = x[:S]
        X[b, S_MAX:].reshape(3, np_max)[:, :(S - 1) * m] = x[S:].reshape(3, -1)
    t = dict(seg_counts=_T(np.array([p[0] for p in probs], np.int32), dev),
             fixed_vals=_T(np.array([p[3] for p in probs]), dev), x=_T(X, dev), times=None)
    import mav_tube_trajectory_generation_amd as mtg
    got = _cost(ctx, t, occ, mtg.make_coll_params(**prm), 1, S_MAX, N=n, R=r)
    for b, (S, vt, tt, _, x) in enumerate(probs):
        J, g, terms, c = oracle.coll_cost(n, r, vt, tt, 1, x, occ_np, prm)
        assert got["status"][b] == 0 and got["collision"][b] == c
        assert rel_err(got["cost"][b], J) <= 1e-9, (b, got["cost"][b], J)
        assert np.max(np.abs(got["terms"][b] - terms)) <= 1e-9 * max(np.max(np.abs(terms)), 1e-12)
        gg = np.concatenate([got["grad"][b][:S],
                             got["grad"][b][S_MAX:].reshape(3, np_max)[:, :(S - 1) * m].ravel()])
        assert np.max(np.abs(gg - g)) <= 1e-8 * max(np.max(np.abs(g)), 1e-12), b
        assert np.count_nonzero(got["grad"][b]) <= gg.size  # the padding is 0.0
        n_coll += c
    assert n_coll < B


# ----------------------------------------------------------- cost vs uniform
@pytest.mark.parametrize("variant", ["central", "soft"])
@pytest.mark.parametrize("mode", [0, 1])
def test_cost_vs_uniform(ctx, dev, occ, mode, variant):
    """Each group of rows of one count against LinearPlan.coll_cost at
    S = S_b: 1e-9 on cost and terms and 1e-8 on the gradient (the project's
    ragged-vs-uniform bar).  The state is compact in both, so every sum runs
    over the same lanes in the same order."""
    import mav_tube_trajectory_generation_amd as mtg
    P = F.paths()
    prm = _prm(**VARIANTS[variant])
    rows = F.cost_rows(mode)
    B = len(rows)
    raise_ref = np.linspace(1.0, 100.0, B)
    got = _cost(ctx, _pack(dev, rows, S_MAX, mode), occ, prm, mode, S_MAX,
                raise_ref=_T(raise_ref, dev))
    worst = dict(cost=0.0, terms=0.0, grad=0.0)
    for i, p in enumerate(P):
        idx = [b for b, (j, _) in enumerate(rows) if j == i]
        mask, df = compact_fixed(p["vt"], N)
        plan = mtg.LinearPlan(ctx, N, 3, R, p["S"], mask)
        nb = len(idx)
        uni = plan.coll_cost(_T(np.repeat(df[None], nb, 0), dev),
                             _T(np.array([rows[b][1] for b in idx]), dev),
                             _T(np.repeat(p["t"][None], nb, 0), dev), occ, prm, mode=mode,
                             raise_ref=_T(raise_ref[idx], dev))
        uni = {k: v.cpu().numpy() for k, v in uni.items()}
        for k, b in enumerate(idx):
            assert got["status"][b] == uni["status"][k] == 0
            assert got["collision"][b] == uni["collision"][k]
            g = F.unpad_x(got["grad"][b], p["S"], S_MAX, mode)
            sc = max(np.max(np.abs(uni["grad"][k])), 1e-12)
            worst["cost"] = max(worst["cost"], rel_err(got["cost"][b], uni["cost"][k]))
            worst["terms"] = max(worst["terms"], np.max(np.abs(got["terms"][b] - uni["terms"][k])) /
                                 max(np.max(np.abs(uni["terms"][k])), 1e-12))
            worst["grad"] = max(worst["grad"], np.max(np.abs(g - uni["grad"][k])) / sc)
    print(f"ragged vs uniform, mode {mode} {variant}: largest relative difference {worst}")
    assert worst["cost"] <= 1e-9 and worst["terms"] <= 1e-9 and worst["grad"] <= 1e-8, worst
    if variant == "central":
        # Without soft constraints both run the same bodies on the same
        # compact state: the results are the same bits.
        # With them the extremum search is another kernel, held to the bar.
        assert worst == dict(cost=0.0, terms=0.0, grad=0.0), worst


# ------------------------------------------------------- optimiser vs oracle
@pytest.mark.parametrize("mode,variant,n", [(0, "main", 6), (0, "central", 12), (1, "central", 6),
                                            (0, "soft", 6), (1, "soft", 6)])
def test_optimize_vs_oracle(ctx, dev, occ, mode, variant, n):
    """The device L-BFGS takes the oracle port's steps on every row's own
    path (the rule of test_coll_gpu.test_coll_optimize_vs_oracle): same
    evaluation count, stopping reason and final point to 1e-6, then cost and
    terms to 1e-5; at most one row in six may leave the oracle's path (the
    objective is not smooth).  Every row ends below its J0 and inside its
    bounds.  main.cpp's increment_time = 1e-6 makes the oracle's time gradient
    rounding noise, so `main` runs in mode 0 only."""
    P = F.paths()
    rows = F.opt_rows(mode, n)
    ref = F.oracle_optimize(mode, variant, n)
    E = 25
    t = _pack(dev, rows, S_MAX, mode)
    got = _opt(ctx, t, occ, _prm(**VARIANTS[variant]), mode, S_MAX, max_evals=E,
               **_bounds(dev, rows, S_MAX, mode))
    lo = F.opt_bounds(rows, mode)[0]
    agree = 0
    for b, (i, x0) in enumerate(rows):
        S, o = P[i]["S"], ref[b]
        assert got["status"][b] == 0
        x = F.unpad_x(got["x"][b], S, S_MAX, mode)
        assert np.all(x >= lo[b])
        assert got["cost"][b] < o["J0"], (b, got["cost"][b], o["J0"])
        pad = F.padding_mask(S, S_MAX, mode)
        assert np.all(np.isnan(got["x"][b].reshape(-1)[pad]))  # keeps the input's bits
        same = (got["evals"][b] == o["evals"] and got["result"][b] == o["result"] and
                np.linalg.norm(x - o["x"]) <= 1e-6 * np.linalg.norm(o["x"]))
        if same:
            assert rel_err(got["cost"][b], o["J"]) <= 1e-5
            assert np.max(np.abs(got["terms"][b] - o["terms"])) <= 1e-5 * abs(o["J"])
            agree += 1
    assert agree >= n - n // 6, (agree, n)


# --------------------------------------------------------------- independence
def _ind_rows(mode):
    return F.cost_rows(mode, per_path=2)  # 10 rows, both collision outcomes


def _ind_run(ctx, dev, occ, mode, rows, S_max=S_MAX, fill=np.nan, ws_fill=None, field=None):
    """Cost and optimiser (soft constraints, history) of rows; every result
    per row with the padding stripped."""
    import mav_tube_trajectory_generation_amd as mtg
    P = F.paths()
    prm = _prm(**VARIANTS["soft"])
    t = _pack(dev, rows, S_max, mode, fill)
    B, E = len(rows), 8
    kw_c, kw_o = {}, {}
    if ws_fill is not None:
        for kw, optimize in ((kw_c, False), (kw_o, True)):
            nb = mtg.ragged_coll_workspace_bytes(N, S_max, B, prm, mode, optimize)
            kw["workspace"] = torch.full((nb,), ws_fill, dtype=torch.uint8, device=dev)
    c = _cost(ctx, t, occ, prm, mode, S_max, near_field=field, **kw_c)
    o = _opt(ctx, t, occ, prm, mode, S_max, max_evals=E, history=True, near_field=field,
             **_bounds(dev, rows, S_max, mode, fill), **kw_o)
    out = []
    for b, (i, _) in enumerate(rows):
        S = P[i]["S"]
        pad = F.padding_mask(S, S_max, mode)
        assert np.all(c["grad"][b].reshape(-1)[pad] == 0.0)
        ev = int(o["evals"][b])
        assert np.all(o["x_history"][b, :ev][:, pad] == 0.0)
        assert np.all(np.isnan(o["x_history"][b, ev:]))  # rows past evals are unset
        xin = t["x"][b].cpu().numpy().reshape(-1)
        assert np.array_equal(o["x"][b].reshape(-1)[pad], xin[pad], equal_nan=True)
        out.append(dict(
            cost=c["cost"][b], grad=F.unpad_x(c["grad"][b], S, S_max, mode), terms=c["terms"][b],
            collision=c["collision"][b], status=c["status"][b],
            x=F.unpad_x(o["x"][b], S, S_max, mode), ocost=o["cost"][b], evals=ev,
            result=o["result"][b], ostatus=o["status"][b], oterms=o["terms"][b],
            hist=np.array([F.unpad_x(h, S, S_max, mode) for h in o["x_history"][b, :ev]])))
    return out


_IND_BASE = {}


def _ind_base(ctx, dev, occ, mode):
    if mode not in _IND_BASE:
        _IND_BASE[mode] = _ind_run(ctx, dev, occ, mode, _ind_rows(mode))
    return _IND_BASE[mode]


def _same_bits(a, b, what):
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True), (what, k)


@pytest.mark.parametrize("what", ["padding", "permutation", "s_max_9", "s_max_6", "workspace",
                                  "near_field"])
@pytest.mark.parametrize("mode", [0, 1])
def test_independence(ctx, dev, occ, mode, what):
    """Bit for bit, cost, gradient and the optimiser's whole path do not depend
    on the input padding (NaN against 0.0), the row order, S_max (7 against 9,
    and 6, where the longest row has no padding), the workspace's contents
    (0xFF against zeros) or the near field."""
    import mav_tube_trajectory_generation_amd as mtg
    rows = _ind_rows(mode)
    base = _ind_base(ctx, dev, occ, mode)
    assert 0 < sum(int(r["collision"]) for r in base) < len(base)
    assert max(r["evals"] for r in base) > 2
    if what == "padding":
        other = _ind_run(ctx, dev, occ, mode, rows, fill=0.0)
    elif what == "permutation":
        perm = np.random.default_rng(5).permutation(len(rows))
        res = _ind_run(ctx, dev, occ, mode, [rows[j] for j in perm])
        other = [None] * len(rows)
        for k, j in enumerate(perm):
            other[j] = res[k]
    elif what == "s_max_9":
        other = _ind_run(ctx, dev, occ, mode, rows, S_max=9)
    elif what == "s_max_6":
        other = _ind_run(ctx, dev, occ, mode, rows, S_max=6)
    elif what == "workspace":
        other = _ind_run(ctx, dev, occ, mode, rows, ws_fill=255)
        zero = _ind_run(ctx, dev, occ, mode, rows, ws_fill=0)
        for b in range(len(rows)):
            _same_bits(zero[b], other[b], (what, b))
    else:
        field = mtg.coll_field(occ, _prm(**VARIANTS["soft"]))
        other = _ind_run(ctx, dev, occ, mode, rows, field=field)
    for b in range(len(rows)):
        _same_bits(base[b], other[b], (what, b))


# ------------------------------------------------------------------- bad rows
@pytest.mark.parametrize("mode", [0, 1])
def test_bad_rows(ctx, dev, occ, mode):
    """Counts 1, 0 and S_max + 1 and a zero time between guard rows: the bad
    rows get their failure values, the optimiser leaves their x untouched, and
    the guards are bit-identical to a run without the bad rows."""
    P = F.paths()
    prm = _prm(**VARIANTS["central"])
    good = F.cost_rows(mode, per_path=1)  # the five tube starts
    rows = [good[0], good[1], good[1], good[2], good[2], good[0], good[3], good[3], good[4]]
    bad = {1: 1, 3: 0, 5: S_MAX + 1}  # row -> count
    zero_t = 7
    pk = F.pack(rows, S_MAX, mode)
    for b, cnt in bad.items():
        pk["seg_counts"][b] = cnt
    if mode == 0:
        pk["times"][zero_t, 1] = 0.0
    else:
        pk["x"][zero_t, 1] = 0.0
    t = _pack(dev, rows, S_MAX, mode, pk=pk)
    guards = [b for b in range(len(rows)) if b not in bad and b != zero_t]
    tg = _pack(dev, [rows[b] for b in guards], S_MAX, mode)
    E = 6
    c, cg = _cost(ctx, t, occ, prm, mode, S_MAX), _cost(ctx, tg, occ, prm, mode, S_MAX)
    o = _opt(ctx, t, occ, prm, mode, S_MAX, max_evals=E)  # unbounded: a zero time stays zero
    og = _opt(ctx, tg, occ, prm, mode, S_MAX, max_evals=E)
    xin = pk["x"]
    for b in bad:
        assert c["status"][b] == BAD_SEGMENTS and c["collision"][b] == -1
        assert np.isnan(c["cost"][b]) and np.all(np.isnan(c["terms"][b]))
        assert np.all(np.isnan(c["grad"][b]))  # the whole padded row
        assert o["status"][b] == BAD_SEGMENTS and o["evals"][b] == 0 and o["result"][b] == -1
        assert np.isnan(o["cost"][b])
        assert np.array_equal(o["x"][b].view(np.int64), xin[b].view(np.int64))
    b = zero_t
    S = P[rows[b][0]]["S"]
    pad = F.padding_mask(S, S_MAX, mode)
    assert c["status"][b] == BAD_TIME and np.isnan(c["cost"][b]) and c["collision"][b] == 0
    assert np.all(np.isnan(c["grad"][b].reshape(-1)[~pad]))
    assert np.all(c["grad"][b].reshape(-1)[pad] == 0.0)
    assert o["status"][b] == BAD_TIME and o["result"][b] == -1 and np.isnan(o["cost"][b])
    assert o["evals"][b] == 1
    assert np.array_equal(o["x"][b].view(np.int64), xin[b].view(np.int64))
    for k, b in enumerate(guards):
        for name in ("cost", "grad", "terms", "collision", "status"):
            assert np.array_equal(c[name][b], cg[name][k], equal_nan=True), (name, b)
        for name in ("x", "cost", "evals", "result", "status", "terms"):
            assert np.array_equal(o[name][b], og[name][k], equal_nan=True), (name, b)
        assert c["status"][b] == 0 and o["status"][b] == 0


# -------------------------------------------------------------- graph capture
def test_graph_replay_over_other_counts(ctx, dev, occ):
    """ragged_coll_optimize captured in a HIP graph replays to the eager
    result; after the counts, points and bounds are overwritten in place with
    another batch (other counts per row) the replay equals that batch's eager
    result."""
    import mav_tube_trajectory_generation_amd as mtg
    mode, E = 1, 8
    prm = _prm(**VARIANTS["soft"])
    first = F.opt_rows(mode, 5)
    other = [first[j] for j in (3, 4, 0, 2, 1)]
    batches = []
    for rows in (first, other):
        t = _pack(dev, rows, S_MAX, mode)
        t.update(_bounds(dev, rows, S_MAX, mode))
        batches.append(t)

    def call(t, **kw):
        return mtg.ragged_coll_optimize(ctx, N, R, t["seg_counts"], t["fixed_vals"], t["x"], None,
                                        occ, prm, mode=mode, max_evals=E, lower=t["lower"],
                                        upper=t["upper"], initial_step=t["initial_step"],
                                        S_max=S_MAX, **kw)
    eager = [call(t) for t in batches]
    torch.cuda.synchronize()
    ws = torch.empty(mtg.ragged_coll_workspace_bytes(N, S_MAX, 5, prm, mode, True),
                     dtype=torch.uint8, device=dev)
    live = {k: v.clone() for k, v in batches[0].items()}
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            out = call(live, workspace=ws)
    for k, t in enumerate(batches):
        for name, dst in live.items():
            dst.copy_(t[name])
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        for name in ("evals", "result", "status"):
            assert torch.equal(out[name], eager[k][name]), (k, name)
        for name in ("x", "cost", "terms"):
            assert torch.equal(out[name].view(torch.int64),
                               eager[k][name].view(torch.int64)), (k, name)
        assert (out["status"] == 0).all() and (out["evals"] > 1).all()
    assert not torch.equal(eager[0]["evals"], eager[1]["evals"]) or \
        not torch.equal(eager[0]["cost"], eager[1]["cost"])


# ---------------------------------------------------------------------- chain
def test_chain(ctx, dev, occ):
    """ragged_tube_solve's x -> ragged_coll_optimize -> coefficients -> the
    ragged collision gate -> mtg_select_local, one map, no host step between
    the calls.  No ragged coefficients-from-constraints entry exists, so the
    coefficients come from LinearPlan.coefficients per count (in this test
    only).  The selected row is collision-free and the cheapest such row."""
    import mav_tube_trajectory_generation_amd as mtg
    from mav_tube_trajectory_generation_amd._abi import check, lib
    P = F.paths()
    order = [0, 1, 2, 3, 4, 2, 1, 3]
    B = len(order)
    seg, pos, fv, times, radii = mtg.pack_ragged_tube(
        [(P[i]["pos"], P[i]["df"], P[i]["t"], P[i]["radii"]) for i in order], N, dev, S_max=S_MAX)
    sol = mtg.ragged_tube_solve(ctx, N, R, seg, pos, fv, times, times, radii)
    assert (sol["status"] == 0).all()
    for b, i in enumerate(order):  # the tube solve's x is the fixture's start
        x = F.unpad_x(sol["x"][b].cpu().numpy(), P[i]["S"], S_MAX, 0)
        assert np.linalg.norm(x - P[i]["x0"]) <= 1e-6 * np.linalg.norm(P[i]["x0"])
    prm = _prm()
    field = mtg.coll_field(occ, prm)
    opt = mtg.ragged_coll_optimize(ctx, N, R, seg, fv, sol["x"], times, occ, prm, mode=0,
                                   max_evals=15, near_field=field)
    coeffs = torch.zeros((B, S_MAX, 3, N), dtype=torch.float64, device=dev)
    for i in sorted(set(order)):
        S = P[i]["S"]
        idx = torch.tensor([b for b, j in enumerate(order) if j == i], device=dev)
        mask, _ = compact_fixed(P[i]["vt"], N)
        plan = mtg.LinearPlan(ctx, N, 3, R, S, mask)
        c, _, st = plan.coefficients(fv[idx].contiguous(),
                                     opt["x"][idx][:, :, :(S - 1) * M].contiguous(),
                                     times[idx][:, :S].contiguous())
        assert (st == 0).all()
        coeffs[idx, :S] = c
    # the tree next to the last segment makes the 6-segment rows collide at their start
    gate = mtg.ragged_collision_cost(seg, coeffs, times, occ, prm.coll, near_field=field,
                                     gate=opt["cost"])
    triple = torch.empty(3, dtype=torch.float64, device=dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    check(lib().mtg_select_local(ctypes.c_void_p(gate["gated"].data_ptr()), B, 0, 0,
                                 ctypes.c_void_p(triple.data_ptr()), stream), "mtg_select_local")
    cost = opt["cost"].cpu().numpy()
    free = gate["collision"].cpu().numpy() == 0
    assert free.any() and (opt["status"] == 0).all()
    want = int(np.nanargmin(np.where(free, cost, np.nan)))
    got = triple.cpu().numpy()
    assert (got[0], int(got[1]), int(got[2])) == (cost[want], want, 0)
    assert free[int(got[1])]
