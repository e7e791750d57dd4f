"""The ragged tube time entries on the GPU (mtg_ragged_tube_time_cost,
mtg_ragged_tube_time_optimize): per row the objective and the LN_SBPLX path
of the uniform entries at the row's own count, against the oracle per row
(orc_tube_time_cost, orc_tube_time_optimize_sbplx) and against the uniform
entries; bad rows that stay in their row; independence of the batch's order
and of S_max; the workspace and graph contracts; and the chain into the
ragged solve, the gated soft cost and the selection.

N = 10, r = 4, radius 0.15, vertices from oracle.random_vertices with
estimate_segment_times(v, 3.0, 5.0), as the uniform tests."""
import concurrent.futures as cf
import ctypes

import numpy as np
import pytest

from test_tube_gpu import tube_inputs

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

N, R = 10, 4
M = N // 2
H = 0.1
RADIUS = 0.15
SOFT = [(1, 3.0), (2, 5.0)]

# LN_SBPLX rows (test_sbplx_vs_oracle): row b has COUNTS[b % 4] segments and
# the vertices of seed SEED0 + b.
COUNTS = (2, 3, 7, 5)
SEED0 = 1100
BUDGETS = {"E30": (30, dict(f_rel=0.05)), "E80": (80, dict(f_rel=1e-6)),
           "E30soft": (30, dict(f_rel=0.05, soft=SOFT))}


def _T(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


class Row:
    def __init__(self, oracle, S, seed):
        self.S = S
        self.v = oracle.random_vertices(M - 1, S, 3, -10.0, 10.0, seed)
        self.t0 = oracle.estimate_segment_times(self.v, 3.0, 5.0)
        self.pos, self.fv = tube_inputs(self.v)
        self.radii = np.full((S, 2), RADIUS)


def _pack(dev, rows, S_max, times=None):
    """seg_counts, positions, fixed_vals, times, radii as pack_ragged_tube gives
    them (NaN padding); times: per-row arrays replacing the rows' T0."""
    import mav_tube_trajectory_generation_amd as mtg
    ts = [r.t0 for r in rows] if times is None else times
    return mtg.pack_ragged_tube([(r.pos, r.fv, t, r.radii) for r, t in zip(rows, ts)], N, dev,
                                S_max=S_max)


def _pad(dev, rows, arrays, S_max):
    out = np.full((len(rows), S_max), np.nan)
    for b, (r, a) in enumerate(zip(rows, arrays)):
        out[b, :r.S] = a
    return _T(dev, out)


def _np(out):
    return {k: (v.cpu().numpy() if v is not None else None) for k, v in out.items()}


def _pool(fn, items):
    with cf.ThreadPoolExecutor(max_workers=8) as ex:
        return list(ex.map(fn, items))


# --------------------------------------------------------------------- item 1
@pytest.fixture(scope="module")
def cost_rows(oracle):
    rows = [Row(oracle, S, 1200 + b) for b, S in enumerate((2, 3, 5, 8, 4, 2))]
    rng = np.random.default_rng(4)
    times = [r.t0 * rng.uniform(0.85, 1.15, size=r.S) for r in rows]  # stale maps
    return rows, times


def _check_cost_vs_oracle(oracle, rows, times, J, g, st, spec, picks):
    def ref(b):
        r = rows[b]
        Jr, gr = oracle.tube_time_cost(N, R, r.v, times[b], r.radii, times_cp=r.t0, grad_mode=2,
                                       soft=spec)
        qc = oracle.tube_solve(N, R, r.v, times[b], r.radii, times_cp=r.t0)["cost"]
        return b, Jr, gr, qc
    for b, Jr, gr, qc in _pool(ref, picks):
        S = rows[b].S
        assert st[b] == 0, b
        tolJ = 1e-6 * abs(qc) + 1e-9 * abs(Jr)
        if spec:
            tolJ += 1e-4 * abs(Jr - qc - 500.0 * times[b].sum() ** 2)  # soft amplifies by 100
        print(f"row {b} S {S}: |J - Jr| {abs(J[b] - Jr):.3e} tol {tolJ:.3e}")
        assert abs(J[b] - Jr) <= tolJ, (b, J[b], Jr)
        if g is not None:
            assert np.max(np.abs(g[b, :S] - gr)) <= 2 * tolJ / (2 * H) + \
                1e-9 * np.max(np.abs(gr)), b
            assert np.all(g[b, S:] == 0.0), b


@pytest.mark.parametrize("S_max", [8, 10])
def test_cost_vs_oracle(ctx, dev, oracle, cost_rows, S_max):
    """Counts (2, 3, 5, 8, 4, 2) at S_max = 8 and at S_max = 10 (above every
    count), times = T0 U(0.85, 1.15) with the maps at T0, NaN padding; the
    tolerance of test_tube_time_cost_vs_oracle."""
    import mav_tube_trajectory_generation_amd as mtg
    rows, times = cost_rows
    seg, pos, fv, t0, radii = _pack(dev, rows, S_max)
    t = _pad(dev, rows, times, S_max)
    out = _np(mtg.ragged_tube_time_cost(ctx, N, R, seg, pos, fv, t0, t, radii, grad=True))
    _check_cost_vs_oracle(oracle, rows, times, out["cost"], out["grad"], out["status"], None,
                          range(len(rows)))
    out0 = _np(mtg.ragged_tube_time_cost(ctx, N, R, seg, pos, fv, t0, t, radii))
    assert out0["grad"] is None
    assert np.array_equal(out0["cost"], out["cost"])      # bit for bit
    assert np.array_equal(out0["status"], out["status"])


def test_cost_soft_vs_oracle(ctx, dev, oracle, cost_rows):
    """Soft limits at 1.03 x a row's own maxima (the exponential regime): with
    row 0's limits every row is compared, with row b's limits row b."""
    import mav_tube_trajectory_generation_amd as mtg
    rows, times = cost_rows
    S_max = 8
    seg, pos, fv, t0, radii = _pack(dev, rows, S_max)
    t = _pad(dev, rows, times, S_max)
    for b, r in enumerate(rows):
        ref0 = oracle.tube_solve(N, R, r.v, times[b], r.radii, times_cp=r.t0)
        spec = [(k, 1.03 * oracle.max_magnitude(N, ref0["coeffs"], times[b], k)["value"])
                for k in (1, 2)]
        out = _np(mtg.ragged_tube_time_cost(ctx, N, R, seg, pos, fv, t0, t, radii, grad=True,
                                            soft=spec))
        _check_cost_vs_oracle(oracle, rows, times, out["cost"], out["grad"], out["status"], spec,
                              range(len(rows)) if b == 0 else [b])
        out0 = _np(mtg.ragged_tube_time_cost(ctx, N, R, seg, pos, fv, t0, t, radii, soft=spec))
        assert np.array_equal(out0["cost"], out["cost"])


# --------------------------------------------------------------------- item 3
@pytest.fixture(scope="module")
def sb_rows(oracle):
    return [Row(oracle, COUNTS[b % 4], SEED0 + b) for b in range(16)]


@pytest.fixture(scope="module")
def sb_runs(ctx, dev, sb_rows):
    """The ragged optimiser's outputs per budget, shared by the comparisons."""
    import mav_tube_trajectory_generation_amd as mtg
    S_max = 8
    seg, pos, fv, t0, radii = _pack(dev, sb_rows, S_max)
    runs = {}
    for name, (E, kw) in BUDGETS.items():
        out = mtg.ragged_tube_time_optimize(ctx, N, R, seg, pos, fv, radii, t0, E, **kw)
        runs[name] = _np(out)
    return (seg, pos, fv, t0, radii), runs


def _agrees(S, got, b, ref):
    """A row's agreement: evals and result equal, times within 1e-6 relative,
    cost within 1e-6."""
    return (ref["evals"] == got["evals"][b] and ref["result"] == got["result"][b]
            and np.max(np.abs(got["times"][b, :S] - ref["times"]) / ref["times"]) <= 1e-6
            and abs(got["cost"][b] - ref["cost"]) <= 1e-6 * abs(ref["cost"]))


@pytest.mark.parametrize("budget", list(BUDGETS))
def test_sbplx_vs_oracle(ctx, dev, oracle, sb_rows, sb_runs, budget):
    """B = 16, counts cycling over (2, 3, 7, 5) at S_max = 8: n = nsmin,
    n = nsmin + 1, n > nsmax and a count below S_max.  Agreement with
    orc_tube_time_optimize_sbplx on all but at most one row (Subplex compares
    objective values and the two IPMs differ by ~1e-9: the rule of
    test_tube_time_sbplx_gpu.py).

    Seeds: row b has seed 1100 + b.  Chosen on the CPU so that the cap is a
    condition and not slack: the oracle alone, run at tol 1e-10 and at tol
    1e-9, takes the same path (evals, result, times to 1e-6, cost to 1e-6) on
    all 16 rows for each of the three budgets (checked for the seeds 1100 to
    1147 with counts cycling the same way: all 48 are stable).

    Measured on MI355X: 16 of 16 rows agree on each of the three budgets
    (DESIGN.md 5.10.4)."""
    import mav_tube_trajectory_generation_amd as mtg
    E, kw = BUDGETS[budget]
    (seg, pos, fv, t0, radii), runs = sb_runs
    got = runs[budget]
    t0n = t0.cpu().numpy()
    soft = kw.get("soft")
    refs = _pool(lambda r: oracle.tube_time_optimize_sbplx(N, R, r.v, r.t0, r.radii, E, **kw),
                 sb_rows)
    agree = sum(_agrees(r.S, got, b, refs[b]) for b, r in enumerate(sb_rows))
    print(f"ragged LN_SBPLX {budget}: {agree} of 16 rows agree with the oracle")
    assert agree >= 15, agree
    # every row, no exceptions
    J0 = _np(mtg.ragged_tube_time_cost(ctx, N, R, seg, pos, fv, t0, t0, radii, soft=soft))
    Tt = _T(dev, got["times"])
    Jt = _np(mtg.ragged_tube_time_cost(ctx, N, R, seg, pos, fv, t0, Tt, radii, soft=soft))
    for b, r in enumerate(sb_rows):
        S = r.S
        assert got["status"][b] == 0, b
        assert 1 <= got["evals"][b] <= E, b
        assert got["result"][b] in (3, 4, 5), b
        T = got["times"][b, :S]
        assert np.all(T >= 0.1) and np.all(T <= 2 * r.t0), b
        assert got["cost"][b] <= J0["cost"][b], b
        assert abs(got["cost"][b] - Jt["cost"][b]) <= 1e-6 * abs(Jt["cost"][b]), b
        # the padding keeps its bits
        assert np.array_equal(got["times"][b, S:].view(np.int64), t0n[b, S:].view(np.int64)), b


# --------------------------------------------------------------------- item 2
def _uniform_groups(rows):
    groups = {}
    for b, r in enumerate(rows):
        groups.setdefault(r.S, []).append(b)
    return groups


def _uniform_geometry(dev, rows, idx):
    return (_T(dev, np.stack([rows[b].pos for b in idx])),
            _T(dev, np.stack([rows[b].fv for b in idx])),
            _T(dev, np.stack([rows[b].radii for b in idx])))


def test_cost_vs_uniform_entry(ctx, dev, cost_rows):
    """Each count's rows through tube_time_cost: 1e-6 on J and on the gradient
    (the routes run different bodies: the uniform one is compiled per S)."""
    import mav_tube_trajectory_generation_amd as mtg
    rows, times = cost_rows
    S_max = 8
    seg, pos, fv, t0, radii = _pack(dev, rows, S_max)
    t = _pad(dev, rows, times, S_max)
    for soft in (None, SOFT):
        out = _np(mtg.ragged_tube_time_cost(ctx, N, R, seg, pos, fv, t0, t, radii, grad=True,
                                            soft=soft))
        for S, idx in _uniform_groups(rows).items():
            upos, ufv, urad = _uniform_geometry(dev, rows, idx)
            ut0 = _T(dev, np.stack([rows[b].t0 for b in idx]))
            ut = _T(dev, np.stack([times[b] for b in idx]))
            ref = _np(mtg.tube_time_cost(ctx, N, R, upos, ufv, ut0, ut, urad, grad=True,
                                         soft=soft))
            for k, b in enumerate(idx):
                assert out["status"][b] == ref["status"][k] == 0
                assert abs(out["cost"][b] - ref["cost"][k]) <= 1e-6 * abs(ref["cost"][k]), b
                assert np.max(np.abs(out["grad"][b, :S] - ref["grad"][k])) <= \
                    1e-6 * np.max(np.abs(ref["grad"][k])), b


@pytest.mark.parametrize("budget", list(BUDGETS))
def test_sbplx_vs_uniform_entry(ctx, dev, sb_rows, sb_runs, budget):
    """Each count's rows through tube_time_optimize(optimizer="sbplx"): the
    agreement rule of test_sbplx_vs_oracle, all but at most one of the 16."""
    import mav_tube_trajectory_generation_amd as mtg
    E, kw = BUDGETS[budget]
    got = sb_runs[1][budget]
    agree = 0
    for S, idx in _uniform_groups(sb_rows).items():
        upos, ufv, urad = _uniform_geometry(dev, sb_rows, idx)
        ut0 = _T(dev, np.stack([sb_rows[b].t0 for b in idx]))
        ref = _np(mtg.tube_time_optimize(ctx, N, R, upos, ufv, urad, ut0, E, optimizer="sbplx",
                                         **kw))
        for k, b in enumerate(idx):
            assert ref["status"][k] == got["status"][b]
            one = dict(evals=ref["evals"][k], result=ref["result"][k], times=ref["times"][k],
                       cost=ref["cost"][k])
            agree += bool(_agrees(S, got, b, one))
    print(f"ragged LN_SBPLX {budget}: {agree} of 16 rows agree with the uniform entry")
    assert agree >= 15, agree


# --------------------------------------------------------------------- item 4
def _vp(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _raw_cost(ctx, dev, inp, t_cp, t, grad_mode, poison):
    """mtg_ragged_tube_time_cost into outputs filled beforehand."""
    import mav_tube_trajectory_generation_amd as mtg
    from mav_tube_trajectory_generation_amd._abi import check, lib, make_time_params
    seg, pos, fv, _, radii = inp
    B, S_max = t.shape
    p = make_time_params(grad_mode=grad_mode)
    cost = torch.full((B,), poison, dtype=torch.float64, device=dev)
    grad = torch.full((B, S_max), poison, dtype=torch.float64, device=dev)
    status = torch.full((B,), -77, dtype=torch.int32, device=dev)
    ws = torch.empty(mtg.ragged_tube_time_workspace_bytes(N, S_max, B, p, False),
                     dtype=torch.uint8, device=dev)
    check(lib().mtg_ragged_tube_time_cost(
        ctx.handle, N, R, S_max, B, _vp(seg), _vp(pos), _vp(fv), _vp(t_cp), _vp(t), _vp(radii),
        1e-10, 100, ctypes.byref(p), _vp(cost), _vp(grad), _vp(status), _vp(ws), ws.numel(),
        ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "cost")
    torch.cuda.synchronize()
    return dict(cost=cost.cpu().numpy(), grad=grad.cpu().numpy(), status=status.cpu().numpy())


def _raw_opt(ctx, dev, inp, t, E, poison):
    """mtg_ragged_tube_time_optimize into outputs filled beforehand."""
    import mav_tube_trajectory_generation_amd as mtg
    from mav_tube_trajectory_generation_amd._abi import check, lib, make_time_params
    seg, pos, fv, _, radii = inp
    B, S_max = t.shape
    p = make_time_params(optimizer="sbplx")
    tio = t.clone()
    cost = torch.full((B,), poison, dtype=torch.float64, device=dev)
    ints = [torch.full((B,), -77, dtype=torch.int32, device=dev) for _ in range(3)]
    ws = torch.empty(mtg.ragged_tube_time_workspace_bytes(N, S_max, B, p, True),
                     dtype=torch.uint8, device=dev)
    check(lib().mtg_ragged_tube_time_optimize(
        ctx.handle, N, R, S_max, B, _vp(seg), _vp(pos), _vp(fv), _vp(radii), _vp(tio), 1e-10,
        100, ctypes.byref(p), E, _vp(cost), _vp(ints[0]), _vp(ints[1]), _vp(ints[2]), _vp(ws),
        ws.numel(), ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "optimize")
    torch.cuda.synchronize()
    return dict(times=tio.cpu().numpy(), cost=cost.cpu().numpy(), evals=ints[0].cpu().numpy(),
                result=ints[1].cpu().numpy(), status=ints[2].cpu().numpy())


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def test_bad_rows_stay_in_their_row(ctx, dev, oracle):
    """Counts 0, 1, S_max + 1 and -3, an initial time of 0.08 and a NaN in a
    live time, among good rows, into poisoned outputs: the bad rows get their
    failure values, and every good row is bit-identical to the same batch
    without the bad rows."""
    import mav_tube_trajectory_generation_amd as mtg
    S_max, E = 6, 12
    counts = (3, 4, 6, 6, 5, 2, 4, 5, 5, 6, 4)
    rows = [Row(oracle, S, 1300 + b) for b, S in enumerate(counts)]
    bad_count = {1: 0, 3: 1, 4: S_max + 1, 8: -3}
    low, nan = 6, 9
    good = [b for b in range(len(rows)) if b not in bad_count and b not in (low, nan)]
    inp = list(_pack(dev, rows, S_max))
    seg = inp[0].cpu().numpy().copy()
    for b, c in bad_count.items():
        seg[b] = c
    inp[0] = _T(dev, seg)
    t = inp[3].cpu().numpy().copy()
    t[low, 1] = 0.08
    t[nan, 2] = np.nan
    # padding with a payload: it must come back bit for bit
    pay = np.array([0x7ff8dead0000beef], dtype=np.uint64).view(np.float64)[0]
    for b, r in enumerate(rows):
        t[b, r.S:] = pay
    t = _T(dev, t)
    tn = t.cpu().numpy()
    clean = list(_pack(dev, [rows[b] for b in good], S_max))
    tclean = _T(dev, tn[good])

    # the cost entry
    for grad_mode in (0, 2):
        out = _raw_cost(ctx, dev, inp, inp[3], t, grad_mode, 123.25)
        ref = _raw_cost(ctx, dev, clean, clean[3], tclean, grad_mode, 123.25)
        for b in bad_count:
            assert out["status"][b] == 5 and np.isnan(out["cost"][b]), b
            if grad_mode == 2:
                assert np.isnan(out["grad"][b]).all(), b
        assert out["status"][nan] == 1 and np.isnan(out["cost"][nan])
        if grad_mode == 0:
            assert np.all(out["grad"] == 123.25)          # not touched without a gradient
        for k, b in enumerate(good):
            assert out["status"][b] == ref["status"][k] == 0
            assert _bits(out["cost"])[b] == _bits(ref["cost"])[k], b
            assert np.array_equal(_bits(out["grad"][b]), _bits(ref["grad"][k])), b

    # the optimiser
    out = _raw_opt(ctx, dev, inp, t, E, 123.25)
    ref = _raw_opt(ctx, dev, clean, tclean, E, 123.25)
    for b in bad_count:
        assert out["status"][b] == 5 and np.isnan(out["cost"][b]), b
        assert out["evals"][b] == 0 and out["result"][b] == -1, b
        assert np.array_equal(_bits(out["times"][b]), _bits(tn[b])), b
    assert out["result"][low] == -1 and out["evals"][low] == 0 and np.isnan(out["cost"][low])
    assert np.array_equal(_bits(out["times"][low]), _bits(tn[low]))
    # a NaN time: the first evaluation reports it; the machine's path on an
    # objective that is NaN throughout is the uniform entry's
    r = rows[nan]
    uni = _np(mtg.tube_time_optimize(ctx, N, R, _T(dev, r.pos[None]), _T(dev, r.fv[None]),
                                     _T(dev, r.radii[None]), _T(dev, tn[nan:nan + 1, :r.S]), E,
                                     optimizer="sbplx"))
    assert out["status"][nan] == uni["status"][0] == 1
    assert out["evals"][nan] == uni["evals"][0] and out["result"][nan] == uni["result"][0]
    assert np.array_equal(out["times"][nan, :r.S], uni["times"][0], equal_nan=True)
    assert np.array_equal(out["cost"][nan:nan + 1], uni["cost"], equal_nan=True)
    assert np.array_equal(_bits(out["times"][nan, r.S:]), _bits(tn[nan, r.S:]))
    for k, b in enumerate(good):
        assert out["status"][b] == 0 and out["result"][b] in (3, 4, 5), b
        for name in ("times", "cost"):
            assert np.array_equal(_bits(out[name][b]), _bits(ref[name][k])), (name, b)
        for name in ("evals", "result", "status"):
            assert out[name][b] == ref[name][k], (name, b)
        assert np.array_equal(_bits(out["times"][b, rows[b].S:]), _bits(tn[b, rows[b].S:])), b


# --------------------------------------------------------------------- item 5
def test_independence(ctx, dev, oracle, sb_rows, sb_runs):
    """A permutation of the rows permutes every output, and the same rows at
    S_max = 8 and at S_max = 12 give the same results, bit for bit."""
    import mav_tube_trajectory_generation_amd as mtg
    rows = sb_rows
    E, kw = BUDGETS["E30soft"]
    base_opt = sb_runs[1]["E30soft"]
    rng = np.random.default_rng(11)
    times = [r.t0 * rng.uniform(0.9, 1.1, size=r.S) for r in rows]

    def run(order, S_max):
        sel = [rows[b] for b in order]
        seg, pos, fv, t0, radii = _pack(dev, sel, S_max)
        t = _pad(dev, sel, [times[b] for b in order], S_max)
        c = _np(mtg.ragged_tube_time_cost(ctx, N, R, seg, pos, fv, t0, t, radii, grad=True,
                                          soft=SOFT))
        o = _np(mtg.ragged_tube_time_optimize(ctx, N, R, seg, pos, fv, radii, t0, E, **kw))
        o["t0"] = t0.cpu().numpy()
        return c, o

    ident = list(range(len(rows)))
    base_c, base_o = run(ident, 8)
    for k in ("times", "cost", "evals", "result", "status"):
        assert np.array_equal(base_o[k], base_opt[k], equal_nan=True), k
    perm = list(np.random.default_rng(3).permutation(len(rows)))
    for order, S_max in ((perm, 8), (ident, 12)):
        c, o = run(order, S_max)
        for k, b in enumerate(order):
            S = rows[b].S
            assert _bits(c["cost"])[k] == _bits(base_c["cost"])[b], (S_max, b)
            assert np.array_equal(_bits(c["grad"][k, :S]), _bits(base_c["grad"][b, :S]))
            assert np.all(c["grad"][k, S:] == 0.0)
            assert c["status"][k] == base_c["status"][b]
            assert _bits(o["cost"])[k] == _bits(base_o["cost"])[b], (S_max, b)
            assert np.array_equal(_bits(o["times"][k, :S]), _bits(base_o["times"][b, :S]))
            assert np.array_equal(_bits(o["times"][k, S:]), _bits(o["t0"][k, S:]))
            for name in ("evals", "result", "status"):
                assert o[name][k] == base_o[name][b], (name, S_max, b)


# --------------------------------------------------------------------- item 6
def test_workspace_contents_do_not_matter(ctx, dev, oracle, sb_rows):
    """Every scratch word is written in the same call before it is read: a
    workspace of 0x00 bytes and one of 0xFF bytes (NaN doubles, int32 -1) give
    bit-identical results, for the cost and for the optimiser."""
    import mav_tube_trajectory_generation_amd as mtg
    from mav_tube_trajectory_generation_amd._abi import make_time_params
    rows = sb_rows[:8]
    S_max, B = 8, 8
    seg, pos, fv, t0, radii = _pack(dev, rows, S_max)
    t = t0 * 1.05
    for grad in (False, True):
        p = make_time_params(grad_mode=2 if grad else 0, soft=SOFT)
        nb = mtg.ragged_tube_time_workspace_bytes(N, S_max, B, p, False)
        outs = []
        for fill in (0x00, 0xFF):
            ws = torch.full((nb,), fill, dtype=torch.uint8, device=dev)
            outs.append(mtg.ragged_tube_time_cost(ctx, N, R, seg, pos, fv, t0, t, radii,
                                                  grad=grad, soft=SOFT, workspace=ws))
        for k in ("cost", "status") + (("grad",) if grad else ()):
            assert torch.equal(outs[0][k], outs[1][k]), (grad, k)
        assert torch.isfinite(outs[1]["cost"]).all()
    p = make_time_params(optimizer="sbplx", soft=SOFT)
    nb = mtg.ragged_tube_time_workspace_bytes(N, S_max, B, p, True)
    outs = []
    for fill in (0x00, 0xFF):
        ws = torch.full((nb,), fill, dtype=torch.uint8, device=dev)
        outs.append(mtg.ragged_tube_time_optimize(ctx, N, R, seg, pos, fv, radii, t0, 25,
                                                  soft=SOFT, workspace=ws))
    for k in ("cost", "evals", "result", "status"):
        assert torch.equal(outs[0][k], outs[1][k]), k
    assert torch.equal(outs[0]["times"].view(torch.int64), outs[1]["times"].view(torch.int64))
    # a workspace one byte short, or none, is refused
    short = torch.empty(nb - 1, dtype=torch.uint8, device=dev)
    with pytest.raises(mtg.MTGError):
        mtg.ragged_tube_time_optimize(ctx, N, R, seg, pos, fv, radii, t0, 25, soft=SOFT,
                                      workspace=short)
    with pytest.raises(mtg.MTGError, match=r"\(-4\)"):
        mtg.ragged_tube_time_optimize(ctx, N, R, seg, pos, fv, radii, t0, 25, optimizer="fd")


def test_graph_replay_over_another_batch(ctx, dev, oracle, sb_rows):
    """The optimise call captured in a HIP graph replays to the eager result;
    after seg_counts, times and geometry are overwritten in place with another
    batch (other counts), the replay equals that batch's eager result."""
    import mav_tube_trajectory_generation_amd as mtg
    from mav_tube_trajectory_generation_amd._abi import make_time_params
    S_max, B, E = 8, 6, 20
    first = list(_pack(dev, sb_rows[:B], S_max))
    other_rows = [Row(oracle, S, 1400 + b) for b, S in enumerate((8, 2, 4, 6, 3, 5))]
    other = _pack(dev, other_rows, S_max)
    eager = [mtg.ragged_tube_time_optimize(ctx, N, R, a[0], a[1], a[2], a[4], a[3], E)
             for a in (first, other)]
    p = make_time_params(optimizer="sbplx")
    ws = torch.empty(mtg.ragged_tube_time_workspace_bytes(N, S_max, B, p, True),
                     dtype=torch.uint8, device=dev)
    seg, pos, fv, t0, radii = (a.clone() for a in first)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            out = mtg.ragged_tube_time_optimize(ctx, N, R, seg, pos, fv, radii, t0, E,
                                                workspace=ws)
    for k, batch in enumerate((first, other)):
        for dst, src in zip((seg, pos, fv, t0, radii), batch):
            dst.copy_(src)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        for name in ("cost", "evals", "result", "status"):
            assert torch.equal(out[name], eager[k][name]), (k, name)
        assert torch.equal(out["times"].view(torch.int64),
                           eager[k]["times"].view(torch.int64)), k
        assert (out["status"] == 0).all() and (out["evals"] >= 1).all()


# --------------------------------------------------------------------- item 7
def test_chain(ctx, dev, sb_rows, sb_runs):
    """optimise -> ragged_tube_solve at the returned times with the maps at T0
    -> gated soft cost -> mtg_select_local: the selected row is the nanargmin
    of the gated costs computed on the host."""
    import mav_tube_trajectory_generation_amd as mtg
    from mav_tube_trajectory_generation_amd._abi import check, lib
    (seg, pos, fv, t0, radii), _ = sb_runs
    B = len(sb_rows)
    opt = mtg.ragged_tube_time_optimize(ctx, N, R, seg, pos, fv, radii, t0, 30)
    sol = mtg.ragged_tube_solve(ctx, N, R, seg, pos, fv, t0, opt["times"], radii)
    st = sol["status"].cpu().numpy()
    assert np.isin(st, (0, 4)).all(), st        # OK or NEAR_OPTIMAL: a usable solution
    assert torch.isfinite(sol["cost"]).all()
    vmax = mtg.ragged_max_magnitude(seg, sol["coeffs"], opt["times"], 1)["value"].cpu().numpy()
    srt = np.sort(vmax)
    limit = 0.5 * (srt[B // 2 - 1] + srt[B // 2])   # both classes, no maximum near the limit
    soft = mtg.ragged_soft_constraint_cost(seg, sol["coeffs"], opt["times"], [1], [limit],
                                           gate=sol["cost"])
    triple = torch.empty(3, dtype=torch.float64, device=dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    check(lib().mtg_select_local(_vp(soft["gated"]), B, 0, 0, _vp(triple), stream),
          "mtg_select_local")
    cost = sol["cost"].cpu().numpy()
    feasible = vmax <= limit
    assert feasible.any() and not feasible.all()
    gated = np.where(feasible, cost, np.nan)
    want = int(np.nanargmin(gated))
    got = triple.cpu().numpy()
    assert (got[0], int(got[1]), int(got[2])) == (cost[want], want, 0)
    assert np.array_equal(np.isinf(soft["gated"].cpu().numpy()), ~feasible)
