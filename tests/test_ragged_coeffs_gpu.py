"""Coefficients and cost from given constraints over ragged batches
(mtg_ragged_coeffs_from_constraints, mtg_ragged_tube_coeffs): the standard
pattern against its own solve, the oracle's A^-1 M [d_f; d_p] and the uniform
entry per count; the tube pattern (ragged_coll_fixture.py, rows of 2..6
segments padded to S_max = 7) against the uniform entry and the tube solve;
what the ragged layout adds (mode-1 rows, independence of padding, S_max, row
order and the outputs' contents, bad rows between guard rows); and the device
chain tube solve -> collision optimiser -> coefficients -> gate -> selection
-> sampling with no host step, eagerly and as one graph replayed over other
counts.

Tolerances are those of test_linear_gpu.test_coefficients_from_constraints:
1e-12 normwise (helpers.rel_err_coeffs) where the same closed form is summed
in another order, 1e-9 against the oracle's matrices, 1e-9 on the cost (a
cancelling form)."""
import ctypes
import functools

import numpy as np
import pytest

import ragged_coll_fixture as F
from coll_fixture import coll_params, forest_map
from helpers import compact_fixed, rel_err_coeffs, standard_vertices
from ragged_coll_fixture import M, N, R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

POISON = -7.25e77
OK, BAD_TIME, BAD_SEGMENTS = 0, 1, 5
S_MAX = 7
COUNTS_1 = [1, 2, 12, 5, 7, 3, 9, 12, 1, 4, 6, 8, 10, 11, 2, 12,
            3, 5, 7, 9, 11, 1, 4, 6, 8, 10, 2, 12, 6, 3, 9, 5]   # B = 32, S_max = 12


def _T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bits(t):
    return t.contiguous().view(torch.int64) if t.dtype == torch.float64 else t


def _same_bits(a, b, what):
    assert torch.equal(_bits(a), _bits(b)), what


def _rel(got, ref):
    return np.abs(got - ref) / np.maximum(np.abs(ref), 1e-300)


# ------------------------------------------------------------ standard pattern
@functools.lru_cache(maxsize=None)
def _std_rows(N_, D, counts, seed0):
    """Per row (S, d_f [D, nf_b], times [S_b]) of createRandomVertices(seed0 + b)
    with S = counts[b] segments (generate_random_problems)."""
    import mav_tube_trajectory_generation_amd as mtg
    rows = []
    for b, S in enumerate(counts):
        _, fixed, times, _ = mtg.generate_random_problems(N_, D, S, 1, seed0=seed0 + b)
        rows.append((S, fixed[0], times[0]))
    return tuple(rows)


def _std_pack(N_, rows, S_max, dev):
    import mav_tube_trajectory_generation_amd as mtg
    return mtg.pack_ragged([(df, t) for _, df, t in rows], N_, dev, S_max=S_max)


def _pad_free(free, rows, MF, fill):
    """The ragged solve's free_vals with every entry past a row's
    (S_b - 1)(M - 1) set to `fill`."""
    free = free.clone()
    for b, (S, _, _) in enumerate(rows):
        free[b, :, (S - 1) * MF:] = fill
    return free


def _std_poison(plan, B, dev):
    return {"coeffs": torch.full((B, plan.S_max, plan.D, plan.N), float("nan"),
                                 dtype=torch.float64, device=dev),
            "cost": torch.full((B,), float("nan"), dtype=torch.float64, device=dev),
            "status": torch.full((B,), -99, dtype=torch.int32, device=dev)}


@pytest.fixture(scope="module")
def std1(ctx, dev):
    """Case 1's batch, its solve and the solved free values with NaN padding
    (shared, not modified)."""
    import mav_tube_trajectory_generation_amd as mtg
    D, r, S_max = 3, 4, 12
    rows = _std_rows(N, D, tuple(COUNTS_1), 105)
    seg, fixed, times = _std_pack(N, rows, S_max, dev)
    plan = mtg.RaggedLinearPlan(ctx, N, D, r, S_max)
    sol = plan.solve(seg, fixed, times, free=True)
    assert (sol["status"] == 0).all()
    free = _pad_free(sol["free"], rows, M - 1, float("nan"))
    return dict(D=D, r=r, S_max=S_max, rows=rows, seg=seg, fixed=fixed, times=times, plan=plan,
                sol=sol, free=free)


def test_standard_round_trip(dev, std1):
    """The solved free values give back the solve's coefficients (bit for bit
    on an MI355X) and cost (4.5e-11: the solve sums the form in another
    order); NaN input padding, NaN-filled outputs, output padding exactly 0.0."""
    s = std1
    B = len(s["rows"])
    assert {1, 2, 12} <= set(COUNTS_1) and B == 32
    assert torch.isnan(s["fixed"]).any() and torch.isnan(s["times"]).any()
    assert torch.isnan(s["free"]).any()
    c, cost, st = s["plan"].coefficients(s["seg"], s["fixed"], s["free"], s["times"],
                                         out=_std_poison(s["plan"], B, dev))
    assert (st == OK).all()
    c, cost = c.cpu().numpy(), cost.cpu().numpy()
    want, wcost = s["sol"]["coeffs"].cpu().numpy(), s["sol"]["cost"].cpu().numpy()
    for b, (S, _, _) in enumerate(s["rows"]):
        err = rel_err_coeffs(c[b, :S], want[b, :S])
        print(f"row {b} S {S}: coeffs {err:.3e} cost {_rel(cost[b], wcost[b]):.3e}")
        assert err <= 1e-12, (b, S)
        assert _rel(cost[b], wcost[b]) <= 1e-9, (b, S)
        assert (c[b, S:] == 0.0).all() and not np.signbit(c[b, S:]).any(), (b, S)
        assert np.isfinite(c[b, :S]).all()


def test_standard_vs_oracle(dev, oracle, std1):
    """Perturbed free values: the oracle's A^-1 M [d_f; d_p], the cost from
    those coefficients with the oracle's Q, and a cost above the optimum."""
    s = std1
    D, r, MF = s["D"], s["r"], M - 1
    rng = np.random.default_rng(3)
    free = s["sol"]["free"].cpu().numpy()
    dp = free + rng.normal(0.0, 0.3, free.shape)
    c, cost, st = s["plan"].coefficients(s["seg"], s["fixed"],
                                         _pad_free(_T(dp, dev), s["rows"], MF, float("nan")),
                                         s["times"])
    assert (st == OK).all()
    c, cost = c.cpu().numpy(), cost.cpu().numpy()
    solved = s["sol"]["cost"].cpu().numpy()
    counts = np.array(COUNTS_1)
    for b in np.nonzero(counts > 1)[0]:
        assert cost[b] > solved[b], b
    shortest = int(np.nonzero(counts == counts[counts >= 2].min())[0][0])
    middle = int(np.nonzero(counts == 6)[0][0])
    longest = int(np.nonzero(counts == counts.max())[0][0])
    for b in (shortest, middle, longest):
        S, df, t = s["rows"][b]
        v = standard_vertices(N, S, D, 105 + b)
        m = oracle.linear_matrices(N, r, v, t)
        J = 0.0
        for d in range(D):
            dall = np.concatenate([df[d], dp[b, d, :(S - 1) * MF]])
            want = (m["Ainv"] @ m["M"] @ dall).reshape(S, N)
            err = rel_err_coeffs(c[b, :S, d], want)
            print(f"row {b} S {S} d {d}: coeffs vs oracle {err:.3e}")
            assert err <= 1e-9, (b, d)
            for k in range(S):
                Q = oracle.segment_matrices(N, r, t[k])[0]
                J += 0.5 * want[k] @ Q @ want[k]
        print(f"row {b}: cost vs oracle {_rel(cost[b], J):.3e}")
        assert _rel(cost[b], J) <= 1e-9, b


def _vs_uniform(ctx, dev, N_, r, D, counts, S_max, seed0):
    """Ragged entry against LinearPlan.coefficients per count (the uniform
    entry's generic kernel) on perturbed solved free values."""
    import mav_tube_trajectory_generation_amd as mtg
    MF = N_ // 2 - 1
    rows = _std_rows(N_, D, tuple(counts), seed0)
    seg, fixed, times = _std_pack(N_, rows, S_max, dev)
    plan = mtg.RaggedLinearPlan(ctx, N_, D, r, S_max)
    sol = plan.solve(seg, fixed, times, free=True)
    rng = np.random.default_rng(11)
    dp = sol["free"].cpu().numpy()
    dp = dp + rng.normal(0.0, 0.3, dp.shape)
    free = _pad_free(_T(dp, dev), rows, MF, float("nan"))
    c, cost, st = plan.coefficients(seg, fixed, free, times, out=_std_poison(plan, len(rows), dev))
    assert (st == OK).all()
    figures = []
    for S in sorted(set(counts)):
        idx = [b for b, k in enumerate(counts) if k == S]
        mask, _, _, _ = mtg.generate_random_problems(N_, D, S, 1, seed0=1)
        uni = mtg.LinearPlan(ctx, N_, D, r, S, mask)
        cu, ju, su = uni.coefficients(fixed[idx][:, :, :N_ + S - 1].contiguous(),
                                      free[idx][:, :, :(S - 1) * MF].contiguous(),
                                      times[idx][:, :S].contiguous())
        assert (su == OK).all()
        cu, ju = cu.cpu().numpy(), ju.cpu().numpy()
        cr, jr = c[idx].cpu().numpy(), cost[idx].cpu().numpy()
        for k, b in enumerate(idx):
            err = rel_err_coeffs(cr[k, :S], cu[k])
            print(f"N {N_} r {r} D {D} S {S} row {b}: coeffs {err:.3e} "
                  f"cost {_rel(jr[k], ju[k]):.3e}")
            figures.append((S, b, err, _rel(jr[k], ju[k])))
            assert (cr[k, S:] == 0.0).all(), (S, b)
    for S, b, err, err_j in figures:   # every figure is printed before the first assertion
        assert err <= 1e-12, (S, b)
        assert err_j <= 1e-9, (S, b)


@pytest.mark.parametrize("N_,r,D", [(4, 1, 3), (6, 2, 3), (8, 3, 3), (12, 4, 3), (10, 2, 1),
                                    (10, 3, 4)])
def test_orders_and_dimensions_vs_uniform(ctx, dev, N_, r, D):
    """Every order, and D = 1 and 4, against LinearPlan.coefficients per count.

    The entry sums the cost operation for operation as the uniform entry does
    ("Cost"): measured on an MI355X the costs agree to
    2.7e-16 or better and the coefficients to 2.7e-15 on all six shapes.  An
    independent order of the same sum is 1.9e-9 to 3.4e-9 off at N = 12."""
    _vs_uniform(ctx, dev, N_, r, D, [1, 2, 3, 5, 5, 3, 2, 1], 5, 300)


def test_many_passes_vs_uniform(ctx, dev):
    """S_b D = 99 and 192 items: two and three passes of the 64 lanes."""
    _vs_uniform(ctx, dev, 10, 4, 3, [1, 33, 64, 64, 33, 1], 64, 400)


# ---------------------------------------------------------------- tube pattern
TUBE_ORDER = [0, 1, 2, 3, 4, 2, 1, 3]


@pytest.fixture(scope="module")
def occ(dev):
    return _T(forest_map(), dev)


@pytest.fixture(scope="module")
def tube(ctx, dev):
    """The fixture's paths through ragged_tube_solve (shared, not modified)."""
    import mav_tube_trajectory_generation_amd as mtg
    P = F.paths()
    seg, pos, fv, times, radii = mtg.pack_ragged_tube(
        [(P[i]["pos"], P[i]["df"], P[i]["t"], P[i]["radii"]) for i in TUBE_ORDER], N, dev,
        S_max=S_MAX)
    sol = mtg.ragged_tube_solve(ctx, N, R, seg, pos, fv, times, times, radii)
    assert (sol["status"] == 0).all()
    return dict(seg=seg, pos=pos, fv=fv, times=times, radii=radii, sol=sol)


def _nan_pad_x(x, order, S_max=S_MAX):
    """ragged_tube_solve's x (0.0 padding) with NaN padding."""
    x = x.clone()
    for b, i in enumerate(order):
        x[b, :, (F.paths()[i]["S"] - 1) * M:] = float("nan")
    return x


def _per_count(ctx, dev, order, fv, x, times):
    """LinearPlan.coefficients per count with the tube mask, scattered into
    the padded rectangle: the route of test_ragged_coll_opt_gpu.test_chain."""
    import mav_tube_trajectory_generation_amd as mtg
    P = F.paths()
    B = len(order)
    coeffs = torch.zeros((B, times.shape[1], 3, N), dtype=torch.float64, device=dev)
    cost = torch.zeros(B, dtype=torch.float64, device=dev)
    for i in sorted(set(order)):
        S = P[i]["S"]
        idx = torch.tensor([b for b, j in enumerate(order) if j == i], device=dev)
        mask, _ = compact_fixed(P[i]["vt"], N)
        plan = mtg.LinearPlan(ctx, N, 3, R, S, mask)
        c, j, st = plan.coefficients(fv[idx].contiguous(),
                                     x[idx][:, :, :(S - 1) * M].contiguous(),
                                     times[idx][:, :S].contiguous())
        assert (st == 0).all()
        coeffs[idx, :S] = c
        cost[idx] = j
    return coeffs, cost


def test_tube_round_trip_and_uniform(ctx, dev, tube):
    import mav_tube_trajectory_generation_amd as mtg
    t = tube
    x = _nan_pad_x(t["sol"]["x"], TUBE_ORDER)
    B = len(TUBE_ORDER)
    out = {"coeffs": torch.full((B, S_MAX, 3, N), float("nan"), dtype=torch.float64, device=dev),
           "cost": torch.full((B,), float("nan"), dtype=torch.float64, device=dev)}
    got = mtg.ragged_tube_coefficients(ctx, N, R, t["seg"], t["fv"], x, t["times"], out=out)
    assert (got["status"] == OK).all() and "times" not in got
    ref_c, ref_j = _per_count(ctx, dev, TUBE_ORDER, t["fv"], t["sol"]["x"], t["times"])
    c, j = got["coeffs"].cpu().numpy(), got["cost"].cpu().numpy()
    ref_c, ref_j = ref_c.cpu().numpy(), ref_j.cpu().numpy()
    sc, sj = t["sol"]["coeffs"].cpu().numpy(), t["sol"]["cost"].cpu().numpy()
    for b, i in enumerate(TUBE_ORDER):
        S = F.paths()[i]["S"]
        e_u, e_s = rel_err_coeffs(c[b, :S], ref_c[b, :S]), rel_err_coeffs(c[b, :S], sc[b, :S])
        print(f"row {b} S {S}: uniform {e_u:.3e} cost {_rel(j[b], ref_j[b]):.3e}; "
              f"tube solve {e_s:.3e} cost {_rel(j[b], sj[b]):.3e}")
        assert e_u <= 1e-12 and _rel(j[b], ref_j[b]) <= 1e-9, b
        assert e_s <= 1e-9, b
        assert (c[b, S:] == 0.0).all(), b


def _mode1_rows(t, order, dev, fill=np.nan, S_max=S_MAX):
    """[T; d_p] rows (pad_x mode 1) from the tube solve's x and the times."""
    P = F.paths()
    x = t["sol"]["x"].cpu().numpy()
    tt = t["times"].cpu().numpy()
    rows = []
    for b, i in enumerate(order):
        S = P[i]["S"]
        compact = np.concatenate([tt[b, :S], F.unpad_x(x[b], S, S_MAX, 0)])
        rows.append(F.pad_x(compact, S, S_max, 1, fill))
    return _T(np.array(rows), dev)


def test_tube_mode1_layout(ctx, dev, tube):
    import mav_tube_trajectory_generation_amd as mtg
    t = tube
    base = mtg.ragged_tube_coefficients(ctx, N, R, t["seg"], t["fv"],
                                        _nan_pad_x(t["sol"]["x"], TUBE_ORDER), t["times"])
    x1 = _mode1_rows(t, TUBE_ORDER, dev)
    got = mtg.ragged_tube_coefficients(ctx, N, R, t["seg"], t["fv"], x1, mode=1)
    assert tuple(got["times"].shape) == (len(TUBE_ORDER), S_MAX)     # S_max from the width
    assert (got["status"] == OK).all()
    _same_bits(got["coeffs"], base["coeffs"], "coeffs")
    _same_bits(got["cost"], base["cost"], "cost")
    tt, tin = got["times"].cpu().numpy(), t["times"].cpu().numpy()
    for b, i in enumerate(TUBE_ORDER):
        S = F.paths()[i]["S"]
        assert np.array_equal(tt[b, :S], tin[b, :S]) and (tt[b, S:] == 0.0).all(), b


# ---------------------------------------------------------------- independence
def _std_run(dev, plan, rows, S_max, fill, free_rows, poison=None):
    import mav_tube_trajectory_generation_amd as mtg
    Nn, MF = plan.N, plan.N // 2 - 1
    seg, fixed, times = mtg.pack_ragged([(df, t) for _, df, t in rows], Nn, dev, S_max=S_max)
    free = torch.full((len(rows), plan.D, (S_max - 1) * MF), fill, dtype=torch.float64, device=dev)
    for b, (S, _, _) in enumerate(rows):
        free[b, :, :(S - 1) * MF] = free_rows[b][:, :(S - 1) * MF]
    fixed = torch.nan_to_num(fixed, nan=fill) if fill == fill else fixed
    times = torch.nan_to_num(times, nan=fill) if fill == fill else times
    out = None
    if poison is not None:
        out = {"coeffs": torch.full((len(rows), S_max, plan.D, Nn), poison, dtype=torch.float64,
                                    device=dev),
               "cost": torch.full((len(rows),), poison, dtype=torch.float64, device=dev)}
    c, j, st = plan.coefficients(seg, fixed, free, times, out=out)
    assert (st == OK).all()
    return c, j


@pytest.mark.parametrize("what", ["padding", "s_max", "permutation", "poison"])
def test_independence_standard(ctx, dev, what):
    import mav_tube_trajectory_generation_amd as mtg
    D, r = 3, 4
    counts = (1, 2, 7, 4, 3, 7, 5, 6)
    rows = _std_rows(N, D, counts, 700)
    rng = np.random.default_rng(5)
    free_rows = [_T(rng.normal(0.0, 1.0, (D, 6 * (M - 1))), dev) for _ in rows]
    p7, p12 = (mtg.RaggedLinearPlan(ctx, N, D, r, s) for s in (7, 12))
    base_c, base_j = _std_run(dev, p7, rows, 7, float("nan"), free_rows)
    if what == "padding":
        c, j = _std_run(dev, p7, rows, 7, 0.0, free_rows)
    elif what == "poison":
        c, j = _std_run(dev, p7, rows, 7, float("nan"), free_rows, poison=POISON)
    elif what == "s_max":
        c, j = _std_run(dev, p12, rows, 12, float("nan"), free_rows)
        assert (c[:, 7:] == 0.0).all()
        c = c[:, :7]
    else:
        perm = [5, 2, 7, 0, 3, 6, 1, 4]
        c, j = _std_run(dev, p7, [rows[k] for k in perm], 7, float("nan"),
                        [free_rows[k] for k in perm])
        inv = torch.tensor(np.argsort(perm), device=dev)
        c, j = c[inv], j[inv]
    _same_bits(c, base_c, what)
    _same_bits(j, base_j, what)


def _tube_run(ctx, dev, tube, order_idx, S_max, fill, mode, poison=None):
    """Rows order_idx of the tube fixture's batch, repacked at S_max."""
    import mav_tube_trajectory_generation_amd as mtg
    P = F.paths()
    x = tube["sol"]["x"].cpu().numpy()
    tin = tube["times"].cpu().numpy()
    xs, ts = [], []
    for b in order_idx:
        S = P[TUBE_ORDER[b]]["S"]
        compact = F.unpad_x(x[b], S, S_MAX, 0)
        if mode:
            compact = np.concatenate([tin[b, :S], compact])
        xs.append(F.pad_x(compact, S, S_max, mode, fill))
        tr = np.full(S_max, fill)
        tr[:S] = tin[b, :S]
        ts.append(tr)
    idx = torch.tensor(order_idx, device=dev)
    B = len(order_idx)
    out = None
    if poison is not None:
        out = {"coeffs": torch.full((B, S_max, 3, N), poison, dtype=torch.float64, device=dev),
               "cost": torch.full((B,), poison, dtype=torch.float64, device=dev)}
        if mode:
            out["times"] = torch.full((B, S_max), poison, dtype=torch.float64, device=dev)
    got = mtg.ragged_tube_coefficients(ctx, N, R, tube["seg"][idx].contiguous(),
                                       tube["fv"][idx].contiguous(), _T(np.array(xs), dev),
                                       None if mode else _T(np.array(ts), dev), mode=mode,
                                       S_max=S_max, out=out)
    assert (got["status"] == OK).all()
    return got


@pytest.mark.parametrize("what", ["padding", "s_max", "permutation", "poison"])
@pytest.mark.parametrize("mode", [0, 1])
def test_independence_tube(ctx, dev, tube, mode, what):
    ident = list(range(len(TUBE_ORDER)))
    base = _tube_run(ctx, dev, tube, ident, S_MAX, np.nan, mode)
    names = ("coeffs", "cost") + (("times",) if mode else ())
    if what == "padding":
        got = _tube_run(ctx, dev, tube, ident, S_MAX, 0.0, mode)
    elif what == "poison":
        got = _tube_run(ctx, dev, tube, ident, S_MAX, np.nan, mode, poison=POISON)
    elif what == "s_max":
        got = _tube_run(ctx, dev, tube, ident, 12, np.nan, mode)
        assert (got["coeffs"][:, S_MAX:] == 0.0).all()
        got["coeffs"] = got["coeffs"][:, :S_MAX]
        if mode:
            assert (got["times"][:, S_MAX:] == 0.0).all()
            got["times"] = got["times"][:, :S_MAX]
    else:
        perm = [5, 2, 7, 0, 3, 6, 1, 4]
        got = _tube_run(ctx, dev, tube, perm, S_MAX, np.nan, mode)
        inv = torch.tensor(np.argsort(perm), device=dev)
        got = {k: got[k][inv] for k in names}
    for k in names:
        _same_bits(got[k], base[k], (what, k))


# -------------------------------------------------------------------- bad rows
def _check_bad(c, j, st, b, code, tt=None):
    assert st[b] == code, (b, st[b])
    assert np.isnan(c[b]).all() and np.isnan(j[b]), b
    if tt is not None:
        assert np.isnan(tt[b]).all(), b


def test_bad_rows_standard(ctx, dev):
    import mav_tube_trajectory_generation_amd as mtg
    D, r, S_max = 3, 4, 7
    counts = (3, 7, 5, 4, 6, 2, 7, 3, 5)   # guards at 0, 4, 8
    rows = _std_rows(N, D, counts, 800)
    plan = mtg.RaggedLinearPlan(ctx, N, D, r, S_max)
    seg, fixed, times = _std_pack(N, rows, S_max, dev)
    rng = np.random.default_rng(9)
    free = _T(rng.normal(0.0, 1.0, (len(rows), D, plan.np_max)), dev)
    free = _pad_free(free, rows, M - 1, float("nan"))
    guards = [0, 4, 8]
    gi = torch.tensor(guards, device=dev)
    ref_c, ref_j, ref_st = plan.coefficients(seg[gi].contiguous(), fixed[gi].contiguous(),
                                             free[gi].contiguous(), times[gi].contiguous())
    assert (ref_st == OK).all()
    seg2, times2 = seg.clone(), times.clone()
    seg2[1], seg2[2], seg2[3] = 0, -3, S_max + 1
    times2[5, 1] = 0.0          # inside S_b = 2
    times2[6, 6] = -1.0         # the last of S_b = 7
    times2[7, 0] = float("nan")
    times2[8, 6] = float("nan")  # behind S_b = 5: changes nothing
    out = {"coeffs": torch.full((len(rows), S_max, D, N), POISON, dtype=torch.float64, device=dev),
           "cost": torch.full((len(rows),), POISON, dtype=torch.float64, device=dev)}
    c, j, st = plan.coefficients(seg2, fixed, free, times2, out=out)
    cn, jn, sn = c.cpu().numpy(), j.cpu().numpy(), st.cpu().numpy()
    for b in (1, 2, 3):
        _check_bad(cn, jn, sn, b, BAD_SEGMENTS)
    for b in (5, 6, 7):
        _check_bad(cn, jn, sn, b, BAD_TIME)
    assert (sn[guards] == OK).all()
    _same_bits(c[gi], ref_c, "guard coeffs")
    _same_bits(j[gi], ref_j, "guard cost")


@pytest.mark.parametrize("mode", [0, 1])
def test_bad_rows_tube(ctx, dev, tube, mode):
    import mav_tube_trajectory_generation_amd as mtg
    P = F.paths()
    order = [0, 1, 2, 3, 4, 2, 1, 3, 4, 0, 2]   # guards at 0, 5, 10
    src = [TUBE_ORDER.index(i) for i in order]   # rows of the shared tube solve
    idx = torch.tensor(src, device=dev)
    seg, fv = tube["seg"][idx].contiguous(), tube["fv"][idx].contiguous()
    times = tube["times"][idx].contiguous()
    sub = dict(sol=dict(x=tube["sol"]["x"][idx].contiguous()), times=times)
    x = _mode1_rows(sub, order, dev) if mode else _nan_pad_x(sub["sol"]["x"], order)
    guards = [0, 5, 10]
    gi = torch.tensor(guards, device=dev)

    def run(seg_, fv_, x_, t_):
        B = seg_.shape[0]
        out = {"coeffs": torch.full((B, S_MAX, 3, N), POISON, dtype=torch.float64, device=dev),
               "cost": torch.full((B,), POISON, dtype=torch.float64, device=dev),
               "times": torch.full((B, S_MAX), POISON, dtype=torch.float64, device=dev)}
        return mtg.ragged_tube_coefficients(ctx, N, R, seg_, fv_, x_, None if mode else t_,
                                            mode=mode, S_max=S_MAX, out=out)

    ref = run(seg[gi].contiguous(), fv[gi].contiguous(), x[gi].contiguous(),
              times[gi].contiguous())
    assert (ref["status"] == OK).all()
    seg2, x2, t2 = seg.clone(), x.clone(), times.clone()
    seg2[1], seg2[2], seg2[3], seg2[4] = 0, -3, S_MAX + 1, 1

    def set_time(b, k, v):
        if mode:
            x2[b, k] = v
        else:
            t2[b, k] = v
    set_time(6, 1, 0.0)            # row 6: S_b = 3
    set_time(7, 4, -2.0)           # row 7: S_b = 5, its last time
    set_time(8, 0, float("nan"))   # row 8: S_b = 6
    set_time(10, 5, float("nan"))  # behind S_b = 4: changes nothing
    got = run(seg2, fv, x2, t2)
    c, j = got["coeffs"].cpu().numpy(), got["cost"].cpu().numpy()
    st, tt = got["status"].cpu().numpy(), got["times"].cpu().numpy()
    for b in (1, 2, 3, 4):
        _check_bad(c, j, st, b, BAD_SEGMENTS, tt)
    for b in (6, 7, 8):
        _check_bad(c, j, st, b, BAD_TIME, tt)
    assert (st[guards] == OK).all() and st[9] == OK
    for name in ("coeffs", "cost", "times"):
        _same_bits(got[name][gi], ref[name], ("guard", name))


# ----------------------------------------------------------------------- chain
N_SAMPLES = 256


def _chain(ctx, dev, occ, prm, field, t, mode, ws=None, out=None):
    """ragged_tube_solve -> ragged_coll_optimize -> ragged_tube_coefficients ->
    ragged_collision_cost gate -> mtg_select_local -> ragged_sample_trajectories
    on the current stream: no host read between the calls.  `out` holds the
    outputs of a previous call to write again (graph capture)."""
    import mav_tube_trajectory_generation_amd as mtg
    from mav_tube_trajectory_generation_amd._abi import check, lib
    B = t["seg"].shape[0]
    sol = mtg.ragged_tube_solve(ctx, N, R, t["seg"], t["pos"], t["fv"], t["times"], t["times"],
                                t["radii"])
    if mode == 0:
        x0, tm = sol["x"], t["times"]
    else:  # [T; d_p] rows: the times in front of the tube solve's x
        x0 = torch.cat([t["times"], sol["x"].reshape(B, -1)], dim=1)
        tm = None
    opt = mtg.ragged_coll_optimize(ctx, N, R, t["seg"], t["fv"], x0, tm, occ, prm, mode=mode,
                                   max_evals=15, near_field=field, workspace=ws, S_max=S_MAX)
    co = mtg.ragged_tube_coefficients(ctx, N, R, t["seg"], t["fv"], opt["x"], tm, mode=mode,
                                      S_max=S_MAX)
    gate_times = co["times"] if mode else t["times"]
    gate = mtg.ragged_collision_cost(t["seg"], co["coeffs"], gate_times, occ, prm.coll,
                                     near_field=field, gate=opt["cost"])
    triple = torch.empty(3, dtype=torch.float64, device=dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    check(lib().mtg_select_local(ctypes.c_void_p(gate["gated"].data_ptr()), B, 0, 0,
                                 ctypes.c_void_p(triple.data_ptr()), stream), "mtg_select_local")
    samples, stimes, count = mtg.ragged_sample_trajectories(t["seg"], co["coeffs"], gate_times,
                                                            0.05, n_max=N_SAMPLES)
    return dict(sol_status=sol["status"], x=opt["x"], opt_cost=opt["cost"],
                opt_status=opt["status"], coeffs=co["coeffs"], coeff_cost=co["cost"],
                coeff_status=co["status"], times=gate_times, collision=gate["collision"],
                gated=gate["gated"], triple=triple, samples=samples, n_samples=count)


def _chain_inputs(dev, order):
    import mav_tube_trajectory_generation_amd as mtg
    P = F.paths()
    seg, pos, fv, times, radii = mtg.pack_ragged_tube(
        [(P[i]["pos"], P[i]["df"], P[i]["t"], P[i]["radii"]) for i in order], N, dev, S_max=S_MAX)
    return dict(seg=seg, pos=pos, fv=fv, times=times, radii=radii)


def _prm():
    import mav_tube_trajectory_generation_amd as mtg
    return mtg.make_coll_params(**coll_params())


@pytest.mark.parametrize("mode", [0, 1])
def test_chain_without_host_step(ctx, dev, occ, mode):
    """The chain of test_ragged_coll_opt_gpu.test_chain with the coefficients
    from the ragged entry: they equal the per-count LinearPlan.coefficients
    route, the selection is that route's, and the selected row is free."""
    import mav_tube_trajectory_generation_amd as mtg
    from mav_tube_trajectory_generation_amd._abi import check, lib
    order = TUBE_ORDER
    B = len(order)
    prm = _prm()
    field = mtg.coll_field(occ, prm)
    t = _chain_inputs(dev, order)
    got = _chain(ctx, dev, occ, prm, field, t, mode)
    assert (got["sol_status"] == 0).all() and (got["opt_status"] == 0).all()
    assert (got["coeff_status"] == OK).all()
    # the per-count route from the same optimised point
    if mode == 0:
        xb, tb = got["x"], t["times"]
    else:
        xb = got["x"][:, S_MAX:].reshape(B, 3, (S_MAX - 1) * M).contiguous()
        tb = got["x"][:, :S_MAX].contiguous()
        for b, i in enumerate(order):
            S = F.paths()[i]["S"]
            assert torch.equal(got["times"][b, :S], tb[b, :S]), b
            assert (got["times"][b, S:] == 0.0).all(), b
    ref_c, _ = _per_count(ctx, dev, order, t["fv"], xb, tb)
    c, rc = got["coeffs"].cpu().numpy(), ref_c.cpu().numpy()
    for b, i in enumerate(order):
        S = F.paths()[i]["S"]
        err = rel_err_coeffs(c[b, :S], rc[b, :S])
        print(f"mode {mode} row {b} S {S}: coeffs vs per-count route {err:.3e}")
        assert err <= 1e-12, b
    gate_r = mtg.ragged_collision_cost(t["seg"], ref_c, got["times"], occ, prm.coll,
                                       near_field=field, gate=got["opt_cost"])
    triple_r = torch.empty(3, dtype=torch.float64, device=dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    check(lib().mtg_select_local(ctypes.c_void_p(gate_r["gated"].data_ptr()), B, 0, 0,
                                 ctypes.c_void_p(triple_r.data_ptr()), stream), "mtg_select_local")
    assert torch.equal(got["triple"], triple_r)
    assert torch.equal(got["collision"], gate_r["collision"])
    tr = got["triple"].cpu().numpy()
    free = got["collision"].cpu().numpy() == 0
    cost = got["opt_cost"].cpu().numpy()
    want = int(np.nanargmin(np.where(free, cost, np.nan)))
    assert free.any() and (tr[0], int(tr[1]), int(tr[2])) == (cost[want], want, 0)
    assert free[int(tr[1])]
    n = got["n_samples"].cpu().numpy()
    assert (n > 1).all() and (n <= N_SAMPLES).all()
    assert torch.isfinite(got["samples"][int(tr[1]), :, :int(n[int(tr[1])])]).all()


def test_chain_in_one_graph_replayed_over_other_counts(ctx, dev, occ):
    """The whole chain captured into one graph on a single stream; after
    another assignment of counts and paths is written into the same tensors
    the replay equals that batch's eager run bit for bit, and the two
    batches select different rows."""
    import mav_tube_trajectory_generation_amd as mtg
    mode = 0
    prm = _prm()
    field = mtg.coll_field(occ, prm)
    orders = (TUBE_ORDER, [3, 2, 1, 0, 3, 1, 2, 0])
    B = len(TUBE_ORDER)
    batches = [_chain_inputs(dev, o) for o in orders]
    eager = [_chain(ctx, dev, occ, prm, field, t, mode) for t in batches]
    torch.cuda.synchronize()
    ws = torch.empty(mtg.ragged_coll_workspace_bytes(N, S_MAX, B, prm, mode, True),
                     dtype=torch.uint8, device=dev)
    live = {k: v.clone() for k, v in batches[0].items()}
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            out = _chain(ctx, dev, occ, prm, field, live, mode, ws=ws)
    for k, t in enumerate(batches):
        for name, dst in live.items():
            dst.copy_(t[name])
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        n = out["n_samples"].cpu().numpy()
        assert (n > 1).all()
        for name, v in out.items():
            if name == "samples":   # columns past a row's count are not written
                for b in range(B):
                    assert torch.equal(_bits(v[b, :, :n[b]]),
                                       _bits(eager[k][name][b, :, :n[b]])), (k, name, b)
            else:
                assert torch.equal(_bits(v), _bits(eager[k][name])), (k, name)
        assert (out["coeff_status"] == OK).all() and (out["opt_status"] == 0).all()
    assert eager[0]["triple"][1].item() != eager[1]["triple"][1].item()
