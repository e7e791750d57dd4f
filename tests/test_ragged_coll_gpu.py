"""The collision walk of a ragged batch on the GPU (mtg_ragged_collision_cost):
rows of different segment counts in one launch, each against the CPU oracle
on its own slice coeffs[b, :S_b], times[b, :S_b], with the hit location
against a NumPy walk, the gate, and the uniform kernel.

Geometry as tests/test_collision_gpu.py: standard_vertices shifted by +20
into a [0, 40)^3 map of resolution 0.25, estimate_segment_times(v, 3, 5),
coefficients from pyoracle.linear_solve.  times is NaN-padded as pack_ragged
pads it, the coefficient padding is NaN (or 0.0, what the ragged solve
writes), every output is pre-filled with a poison value.

Tolerances are test_collision_cost_vs_oracle's: collision flag exact, cost
1e-9 relative or 1e-12 absolute, grad_coeffs 1e-8 normwise.  hit_time is the
walk's repeated addition of dt from the segment's start, restated in
_walk_hit, so it is held bit for bit.  Which seeds collide was worked out on
the CPU with the oracle alone; every test asserts the mix it needs from the
oracle's flags before it looks at the kernel's.
"""
import ctypes
import functools

import numpy as np
import pytest

from helpers import compact_fixed, rel_err, standard_vertices

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

D = 3
OFFSET = 20.0
POISON = -7.25e77
PRM = dict(map_resolution=0.25, min_bound=(0.0,) * 3, max_bound=(40.0,) * 3, epsilon=0.5,
           robot_radius=0.1, coll_pot_multiplier=1.0, coll_check_time_increment=0.1)
ORDER_R = {8: 3, 10: 4, 12: 4}  # the derivative each order's solve minimises


def _prm(**kw):
    p = dict(PRM)
    p.update(kw)
    return p


def _key(prm):
    return tuple(sorted(prm.items()))


@functools.lru_cache(maxsize=None)
def _map(seed=5, n=160, n_obst=6000, n_blob=30):
    """test_collision_gpu._map: scattered occupied voxels and a few solid blocks."""
    rng = np.random.default_rng(seed)
    occ = np.full((n, n, n), -1.0, np.float32)
    idx = rng.integers(0, n, size=(n_obst, 3))
    occ[idx[:, 2], idx[:, 1], idx[:, 0]] = rng.uniform(0.0, 2.0, n_obst)
    for _ in range(n_blob):
        c = rng.integers(10, n - 10, size=3)
        occ[c[2] - 2:c[2] + 3, c[1] - 2:c[1] + 3, c[0] - 2:c[0] + 3] = 1.0
    occ.setflags(write=False)
    return occ


@functools.lru_cache(maxsize=None)
def _problem(N, S, seed):
    """(vertices, times, oracle solve) of one trajectory, computed once and
    shared (callers do not modify it)."""
    import pyoracle
    v = standard_vertices(N, S, D, seed)
    v.vals[:, 0, :] += OFFSET
    t = pyoracle.estimate_segment_times(v, 3.0, 5.0)
    return v, t, pyoracle.linear_solve(N, ORDER_R[N], v, t)


def _walk_hit(coeffs, times, occ, prm, side=20):
    """getCostAndGradientCollision's walk (nonlinear_impl:1667-1759) on a dense
    grid, after test_coll_oracle._walk_numpy, reduced to what decides where it
    stops: returns (collision, segment, t, by_bounds) of the first colliding
    evaluated sample, or (False, -1, nan, False)."""
    res, dt = prm["map_resolution"], prm["coll_check_time_increment"]
    mn, mx = np.array(prm["min_bound"]), np.array(prm["max_bound"])
    rad = prm["robot_radius"]
    nz, ny, nx = occ.shape
    N = coeffs.shape[2]

    def nearest(v):
        lo = v - side // 2  # findOccupiedVoxels: voxels overlapping [lo, lo + side]
        a = np.maximum(lo - 1, 0)
        b = np.minimum(lo + side, np.array([nx, ny, nz]) - 1)
        if np.any(a > b):
            return np.finfo(float).max * res
        sub = occ[a[2]:b[2] + 1, a[1]:b[1] + 1, a[0]:b[0] + 1]
        zz, yy, xx = np.nonzero(sub >= 0.0)
        if len(xx) == 0:
            return np.finfo(float).max * res
        pts = np.stack([xx + a[0], yy + a[1], zz + a[2]], axis=1).astype(float)
        return np.min(np.sqrt(np.sum((pts - v) ** 2, axis=1))) * res

    prev = np.zeros(3)
    time_sum, dist_sum = -1.0, 0.0
    for i in range(len(times)):
        t = 0.0
        while t < times[i]:
            Tv = np.array([t ** n for n in range(N)])
            pos = coeffs[i] @ Tv
            if time_sum < 0:
                time_sum = 0.0
                prev = pos
                t += dt
                continue
            time_sum += dt
            dist_sum += np.linalg.norm(pos - prev)
            prev = pos
            if dist_sum < res:
                t += dt
                continue
            valid = not (np.any(pos < mn + res) or np.any(pos > mx - res))
            d = nearest(np.trunc(pos / res).astype(int)) if valid else 0.0
            if d - rad <= 0.0:
                return True, i, t, not valid
            dist_sum = 0.0
            time_sum = 0.0
            t += dt
        time_sum += -dt + (times[i] - t)
    return False, -1, float("nan"), False


@functools.lru_cache(maxsize=None)
def _ref(N, S, seed, prm_key, map_key=()):
    """(J, collision, grad_coeffs) of the oracle on the row's own slice; a
    one-segment row has no free derivative, which the oracle takes as well."""
    import pyoracle
    v, t, sol = _problem(N, S, seed)
    J, c, gc, _ = pyoracle.collision_cost(N, ORDER_R[N], v, t, sol["dp"], _map(*map_key),
                                          dict(prm_key))
    return J, c, gc


@functools.lru_cache(maxsize=None)
def _ref_hit(N, S, seed, prm_key, map_key=()):
    _, t, sol = _problem(N, S, seed)
    return _walk_hit(sol["coeffs"], t, _map(*map_key), dict(prm_key))


def _pack(rows, N, S_max, dev, pad=np.nan):
    """seg_counts, coeffs [B, S_max, 3, N] padded with `pad`, times NaN-padded;
    rows: (S, seed)."""
    B = len(rows)
    c = np.full((B, S_max, D, N), pad)
    t = np.full((B, S_max), np.nan)
    for b, (S, seed) in enumerate(rows):
        _, tb, sol = _problem(N, S, seed)
        c[b, :S] = sol["coeffs"]
        t[b, :S] = tb
    seg = torch.tensor([S for S, _ in rows], dtype=torch.int32, device=dev)
    return seg, torch.from_numpy(c).to(dev), torch.from_numpy(t).to(dev)


def _out(B, S_max, N, dev, grad=True, gated=False, guard=0):
    f = lambda *shape: torch.full(shape, POISON, dtype=torch.float64, device=dev)  # noqa: E731
    i = lambda *shape: torch.full(shape, -99, dtype=torch.int32, device=dev)  # noqa: E731
    o = {"cost": f(B + guard), "collision": i(B + guard), "hit_segment": i(B + guard),
         "hit_time": f(B + guard)}
    if grad:
        o["grad_coeffs"] = f(B + guard, S_max, D, N)
    if gated:
        o["gated"] = f(B + guard)
    return o


def _head(o, B):
    return {k: v[:B] for k, v in o.items()}


def _np(o):
    return {k: v.cpu().numpy() for k, v in o.items()}


def _same(a, b):
    """Bit for bit, NaN included."""
    if a.dtype == torch.float64:
        a, b = a.contiguous().view(torch.int64), b.contiguous().view(torch.int64)
    return torch.equal(a, b)


class World:
    """A map on the device with its near field and parameters."""

    def __init__(self, dev, prm, map_key=()):
        import mav_tube_trajectory_generation_amd as mtg
        self.prm, self.map_key = prm, map_key
        self.occ_np = _map(*map_key)
        self.occ = torch.from_numpy(np.array(self.occ_np)).to(dev)
        self.params = mtg.make_collision_params(**prm)
        self.field = mtg.coll_field(self.occ, self.params)

    def run(self, seg, cd, td, field=True, grad=True, gate=None, out=None):
        import mav_tube_trajectory_generation_amd as mtg
        B, S_max, _, N = cd.shape
        if out is None:
            out = _out(B, S_max, N, cd.device, grad, gate is not None)
        return mtg.ragged_collision_cost(seg, cd, td, self.occ, self.params,
                                         near_field=self.field if field else None, grad=grad,
                                         gate=gate, out=out)


@pytest.fixture(scope="module")
def world(ctx, dev):
    return World(dev, PRM)


def _check_rows(N, S_max, rows, out, prm, map_key=()):
    """Every row against the oracle on its slice; returns the collision count."""
    o = _np(out)
    n_coll = 0
    for b, (S, seed) in enumerate(rows):
        J, c, gc = _ref(N, S, seed, _key(prm), map_key)
        err = rel_err(o["cost"][b], J)
        sc = max(np.max(np.abs(gc)), 1e-300)
        gerr = np.max(np.abs(o["grad_coeffs"][b, :S] - gc)) / sc
        print(f"N={N} row {b} S={S} seed {seed}: coll {c} cost err {err:.3e} grad err {gerr:.3e}")
        assert o["collision"][b] == c, (b, o["collision"][b], c)
        n_coll += c
        assert err <= 1e-9 or abs(o["cost"][b] - J) <= 1e-12, (b, o["cost"][b], J)
        assert gerr <= 1e-8, (b, gerr)
        assert np.all(o["grad_coeffs"][b, S:] == 0.0), b
        assert (o["hit_segment"][b] >= 0) == bool(c), b
    return n_coll


def _check_hits(N, rows, out, prm, map_key=()):
    """hit_segment and hit_time against the NumPy walk: exact, bit for bit."""
    o = _np(out)
    hits = []
    for b, (S, seed) in enumerate(rows):
        c, seg, t, by_bounds = _ref_hit(N, S, seed, _key(prm), map_key)
        print(f"row {b} S={S} seed {seed}: walk {(c, seg, t, by_bounds)} kernel "
              f"{(o['collision'][b], o['hit_segment'][b], o['hit_time'][b])}")
        assert o["collision"][b] == int(c), b
        assert o["hit_segment"][b] == seg, (b, o["hit_segment"][b], seg)
        if c:
            assert o["hit_time"][b] == t, (b, o["hit_time"][b], t)
        else:
            assert np.isnan(o["hit_time"][b]), b
        hits.append((c, seg, by_bounds))
    return hits


MIXED_N, MIXED_SMAX = 10, 12
MIXED = ((1, 105), (2, 106), (3, 107), (12, 108), (2, 109), (5, 110), (1, 111), (7, 112))


@pytest.fixture(scope="module")
def mixed(world, dev):
    """Test 1's launch (near field, gradient, NaN padding), shared."""
    seg, cd, td = _pack(MIXED, MIXED_N, MIXED_SMAX, dev)
    out = world.run(seg, cd, td)
    torch.cuda.synchronize()
    return seg, cd, td, out


def test_mixed_counts_vs_oracle(mixed):
    """S = 1, S = 2, odd and even counts, a row without padding, neighbours of
    different length, both outcomes."""
    n_ref = sum(_ref(MIXED_N, S, seed, _key(PRM))[1] for S, seed in MIXED)
    assert 0 < n_ref < len(MIXED), n_ref
    n_coll = _check_rows(MIXED_N, MIXED_SMAX, MIXED, mixed[3], PRM)
    assert 0 < n_coll < len(MIXED), n_coll


LAST_SEGMENT_ROW = (2, 204)  # collides in its last segment
TIGHT = dict(min_bound=(OFFSET - 9.0,) * 3, max_bound=(OFFSET + 9.0,) * 3)


def test_hit_location(world, mixed, dev):
    """Free rows -1 / NaN; colliding rows the walk's sample, among them one
    that collides in its last segment; under tight bounds a row that leaves
    them reports the sample at which it does."""
    hits = _check_hits(MIXED_N, MIXED, mixed[3], PRM)
    assert any(c for c, _, _ in hits) and not all(c for c, _, _ in hits)
    rows = (LAST_SEGMENT_ROW, (4, 121), (2, 122))
    seg, cd, td = _pack(rows, MIXED_N, 5, dev)
    out = world.run(seg, cd, td)
    torch.cuda.synchronize()
    hits = _check_hits(MIXED_N, rows, out, PRM)
    assert hits[0][0] and hits[0][1] == LAST_SEGMENT_ROW[0] - 1, hits[0]
    tight = World(dev, _prm(**TIGHT))
    out = tight.run(seg, cd, td)
    torch.cuda.synchronize()
    hits = _check_hits(MIXED_N, rows, out, tight.prm)
    assert any(c and by_bounds for c, _, by_bounds in hits), hits
    _check_rows(MIXED_N, 5, rows, out, tight.prm)


def test_segment_longer_than_one_chunk(ctx, dev):
    """dt = 0.02: every segment here lasts more than 64 dt, so the walk
    continues a segment across chunks inside a ragged row."""
    prm = _prm(coll_check_time_increment=0.02)
    rows = ((2, 131), (1, 132), (3, 133))
    for S, seed in rows:
        assert np.max(_problem(MIXED_N, S, seed)[1]) > 64 * 0.02
    w = World(dev, prm)
    seg, cd, td = _pack(rows, MIXED_N, 4, dev)
    out = w.run(seg, cd, td)
    torch.cuda.synchronize()
    _check_rows(MIXED_N, 4, rows, out, prm)
    _check_hits(MIXED_N, rows, out, prm)


SMALL_MAP = (7, 100)  # covers [0, 25)^3: the trajectories leave the grid, not the bounds
WIDE = dict(min_bound=(-100.0,) * 3, max_bound=(100.0,) * 3)


def test_with_and_without_near_field(world, mixed, dev):
    """Bit-identical outputs; on the small map the walks leave the grid, so
    the near-field launch falls back to the box scan there."""
    seg, cd, td, with_field = mixed
    without = world.run(seg, cd, td, field=False)
    torch.cuda.synchronize()
    for k in with_field:
        assert _same(with_field[k], without[k]), k
    prm = _prm(**WIDE)
    rows = MIXED[:6]
    # a free row with a vertex at least 1 m beyond the grid: it is walked
    # there, through the band in which the box still overlaps the grid
    outside = [np.max(_problem(MIXED_N, S, seed)[0].vals[:, 0, :]) >= 26.0 and
               not _ref(MIXED_N, S, seed, _key(prm), SMALL_MAP)[1] for S, seed in rows]
    assert any(outside), outside
    w = World(dev, prm, SMALL_MAP)
    seg, cd, td = _pack(rows, MIXED_N, MIXED_SMAX, dev)
    a = w.run(seg, cd, td)
    b = w.run(seg, cd, td, field=False)
    torch.cuda.synchronize()
    for k in a:
        assert _same(a[k], b[k]), k
    _check_rows(MIXED_N, MIXED_SMAX, rows, a, prm, SMALL_MAP)


@pytest.mark.parametrize("S,seeds", [(2, (106, 109, 122, 204, 141, 142)),
                                     (6, (140, 141, 142, 143, 144, 145))])
def test_against_uniform_kernel(ctx, world, dev, S, seeds):
    """Rows of one count against LinearPlan.collision_cost: flags exact, cost
    and gradient within 1e-9."""
    import mav_tube_trajectory_generation_amd as mtg
    N, S_max = MIXED_N, 7
    rows = tuple((S, seed) for seed in seeds)
    n_ref = sum(_ref(N, S, seed, _key(PRM))[1] for seed in seeds)
    assert 0 < n_ref < len(rows), n_ref
    seg, cd, td = _pack(rows, N, S_max, dev)
    out = world.run(seg, cd, td)
    mask, _ = compact_fixed(_problem(N, S, rows[0][1])[0], N)
    plan = mtg.LinearPlan(ctx, N, D, ORDER_R[N], S, mask)
    uni = plan.collision_cost(cd[:, :S].contiguous(), td[:, :S].contiguous(), world.occ,
                              world.params)
    torch.cuda.synchronize()
    assert torch.equal(out["collision"], uni["collision"])
    r, u = _np(out), _np(uni)
    for b in range(len(rows)):
        assert rel_err(r["cost"][b], u["cost"][b]) <= 1e-9 or r["cost"][b] == u["cost"][b], b
        sc = max(np.max(np.abs(u["grad_coeffs"][b])), 1e-300)
        assert np.max(np.abs(r["grad_coeffs"][b, :S] - u["grad_coeffs"][b])) <= 1e-9 * sc, b
        assert np.all(r["grad_coeffs"][b, S:] == 0.0), b


def test_padding_is_not_read(world, mixed, dev):
    """0.0 in the coefficient and time padding: bit for bit the NaN-padded
    results, which hold no NaN but the free rows' hit_time."""
    seg, cd, td, ref = mixed
    _, c0, _ = _pack(MIXED, MIXED_N, MIXED_SMAX, dev, pad=0.0)
    t0 = torch.nan_to_num(td, nan=0.0)
    assert torch.isnan(cd).any() and torch.isnan(td).any()
    out = world.run(seg, c0, t0)
    torch.cuda.synchronize()
    for k in ref:
        assert _same(ref[k], out[k]), k
    assert not torch.isnan(ref["cost"]).any() and not torch.isnan(ref["grad_coeffs"]).any()


def test_bad_rows_stay_in_their_row(world, dev):
    """Counts 0, S_max + 1 and -3 between good rows: the failure values in the
    row's own outputs, the good rows bit for bit a clean launch's, the guard
    rows behind every output untouched."""
    N, S_max, G = MIXED_N, MIXED_SMAX, 2
    good = {0: MIXED[2], 2: MIXED[5], 4: MIXED[1], 6: MIXED[3]}
    counts = [good[0][0], 0, good[2][0], S_max + 1, good[4][0], -3, good[6][0]]
    B = len(counts)
    seg_g, c_g, t_g = _pack(tuple(good.values()), N, S_max, dev)
    cd = torch.full((B, S_max, D, N), float("nan"), dtype=torch.float64, device=dev)
    td = torch.full((B, S_max), float("nan"), dtype=torch.float64, device=dev)
    for j, b in enumerate(good):
        cd[b], td[b] = c_g[j], t_g[j]
    seg = torch.tensor(counts, dtype=torch.int32, device=dev)
    gate = torch.arange(1.0, B + 1.0, dtype=torch.float64, device=dev)
    for field in (True, False):
        full = _out(B, S_max, N, dev, gated=True, guard=G)
        out = world.run(seg, cd, td, field=field, gate=gate, out=_head(full, B))
        clean = world.run(seg_g, c_g, t_g, field=field)
        torch.cuda.synchronize()
        for b in (1, 3, 5):
            assert torch.isnan(out["cost"][b]) and torch.isnan(out["hit_time"][b]), b
            assert int(out["collision"][b]) == -1 and int(out["hit_segment"][b]) == -1, b
            assert torch.isnan(out["grad_coeffs"][b]).all(), b
            assert float(out["gated"][b]) == float("inf"), b
        for j, b in enumerate(good):
            for k in clean:
                assert np.array_equal(_np(out)[k][b], _np(clean)[k][j], equal_nan=True), (b, k)
            want = float("inf") if int(clean["collision"][j]) else float(gate[b])
            assert float(out["gated"][b]) == want, b
        for k in ("cost", "hit_time", "grad_coeffs", "gated"):
            assert torch.all(full[k][B:] == POISON), k
        for k in ("collision", "hit_segment"):
            assert torch.all(full[k][B:] == -99), k


def _select(costs, dev, start=1000, rank=3):
    from mav_tube_trajectory_generation_amd import lib
    from mav_tube_trajectory_generation_amd._abi import check
    triple = torch.empty(3, dtype=torch.float64, device=dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    check(lib().mtg_select_local(ctypes.c_void_p(costs.data_ptr()), costs.numel(), start, rank,
                                 ctypes.c_void_p(triple.data_ptr()), stream), "mtg_select_local")
    return triple


def test_gate_and_selection(world, dev):
    """The solve's cost through the gate: +inf exactly on colliding and bad
    rows, a NaN gate passes through, the aliased form agrees, and
    mtg_select_local over gated is nanargmin over the free rows' costs."""
    N, S_max = MIXED_N, MIXED_SMAX
    rows = MIXED + ((4, 113), (9, 114))
    coll = np.array([_ref(N, S, seed, _key(PRM))[1] for S, seed in rows] + [1])  # + a bad row
    assert 2 <= (coll == 0).sum() and 2 <= coll.sum(), coll
    cost = np.array([_problem(N, S, seed)[2]["cost"] for S, seed in rows] + [0.5])
    seg, cd, td = _pack(rows + ((1, 105),), N, S_max, dev)
    seg[-1] = S_max + 1  # the bad row would win the selection on its gate
    B = len(coll)
    gate = torch.from_numpy(cost).to(dev)
    out = world.run(seg, cd, td, grad=False, gate=gate)
    torch.cuda.synchronize()
    want = np.where(coll == 0, cost, np.inf)
    assert np.array_equal(_np(out)["gated"], want)
    j = int(np.argmin(want))
    assert _select(out["gated"], dev).cpu().tolist() == [cost[j], 1000.0 + j, 3.0]
    g2 = gate.clone()
    g2[j] = float("nan")                       # the winner, a free row
    hit_row = int(np.flatnonzero(coll)[0])
    g2[hit_row] = float("nan")                 # a colliding row stays +inf
    want = np.where(coll == 0, g2.cpu().numpy(), np.inf)
    o2 = world.run(seg, cd, td, grad=False, gate=g2)
    got = _np(o2)["gated"]
    assert np.isnan(got[j]) and got[hit_row] == np.inf
    assert np.array_equal(got, want, equal_nan=True)
    alias = g2.clone()
    o3 = world.run(seg, cd, td, grad=False, gate=alias,
                   out=dict(_out(B, S_max, N, dev, grad=False), gated=alias))
    torch.cuda.synchronize()
    assert o3["gated"].data_ptr() == alias.data_ptr()
    assert np.array_equal(alias.cpu().numpy(), want, equal_nan=True)
    for k in ("cost", "collision", "hit_segment", "hit_time"):
        assert _same(o3[k], out[k]), k
    j2 = int(np.nanargmin(want))
    assert j2 != j
    assert _select(alias, dev).cpu().tolist() == [want[j2], 1000.0 + j2, 3.0]


def test_graph_replay_with_other_counts(ctx, world, dev):
    """ragged solve -> soft-constraint gate -> collision gate -> select
    captured as one chain, then replayed over another mix of counts written
    into the same buffers: the same as an eager run on those counts."""
    import pyoracle

    import mav_tube_trajectory_generation_amd as mtg
    N, r, S_max = MIXED_N, ORDER_R[MIXED_N], MIXED_SMAX
    first = ((4, 150), (9, 151), (1, 152), (12, 153), (2, 154), (6, 155))
    second = ((12, 108), (1, 111), (7, 112), (2, 109), (5, 110), (2, 204))
    ders = [1, 2]
    B = len(first)
    # limits between the second and third maxima of the replayed batch, so the
    # first gate decides rows of both classes, and so must the second
    ref = np.array([[pyoracle.max_magnitude(N, _problem(N, S, seed)[2]["coeffs"],
                                            _problem(N, S, seed)[1], k)["value"] for k in ders]
                    for S, seed in second])
    srt = np.sort(ref, axis=0)
    lims = (0.5 * (srt[-3] + srt[-2])).tolist()
    ok = np.all(ref <= lims, axis=1)
    coll = np.array([_ref(N, S, seed, _key(PRM))[1] for S, seed in second])
    assert np.all(np.abs(ref - lims) >= 1e-6 * np.array(lims))
    assert not ok.all() and (ok & (coll == 1)).any() and (ok & (coll == 0)).any(), (ok, coll)
    plan = mtg.RaggedLinearPlan(ctx, N, D, r, S_max)

    def inputs(rows):
        return mtg.pack_ragged([(_problem(N, S, seed)[2]["df"], _problem(N, S, seed)[1])
                                for S, seed in rows], N, dev, S_max=S_max)

    def fresh():
        f = lambda *shape: torch.full(shape, POISON, dtype=torch.float64, device=dev)  # noqa: E731
        return ({"coeffs": f(B, S_max, D, N), "cost": f(B)},
                {"cost": f(B), "maxima": f(B, 2), "gated": f(B)},
                _out(B, S_max, N, dev, grad=False, gated=True), f(3))

    def pipeline(seg, fixed, times, sol, soft, col, triple):
        from mav_tube_trajectory_generation_amd import lib
        from mav_tube_trajectory_generation_amd._abi import check
        plan.solve(seg, fixed, times, status=False, out=sol)
        mtg.ragged_soft_constraint_cost(seg, sol["coeffs"], times, ders, lims, gate=sol["cost"],
                                        out=soft)
        world.run(seg, sol["coeffs"], times, grad=False, gate=soft["gated"], out=col)
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        check(lib().mtg_select_local(ctypes.c_void_p(col["gated"].data_ptr()), B, 0, 0,
                                     ctypes.c_void_p(triple.data_ptr()), stream),
              "mtg_select_local")

    seg, fixed, times = inputs(first)
    bufs = fresh()
    pipeline(seg, fixed, times, *bufs)  # warm-up: LDS attributes, module load
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        pipeline(seg, fixed, times, *bufs)
    seg2, fixed2, times2 = inputs(second)
    seg.copy_(seg2)
    fixed.copy_(fixed2)
    times.copy_(times2)
    for o in bufs[:3]:
        for v in o.values():
            v.fill_(POISON if v.dtype == torch.float64 else -99)
    bufs[3].fill_(POISON)
    g.replay()
    torch.cuda.synchronize()
    eager = fresh()
    pipeline(seg2, fixed2, times2, *eager)
    torch.cuda.synchronize()
    for a, e in zip(bufs[:3], eager[:3]):
        for k in a:
            assert np.array_equal(_np(a)[k], _np(e)[k], equal_nan=True), k
    assert torch.equal(bufs[3], eager[3])
    gated = _np(bufs[2])["gated"]
    assert np.array_equal(np.isfinite(gated), ok & (coll == 0)), (gated, ok, coll)
    assert np.array_equal(_np(bufs[2])["collision"], coll)
    assert bufs[3].cpu().tolist() == [gated.min(), float(np.argmin(gated)), 0.0]


@pytest.mark.parametrize("N,S_max,rows", [(8, 5, ((5, 163), (1, 161), (4, 162), (2, 160))),
                                          (12, 4, ((4, 170), (1, 171), (3, 172), (2, 173)))])
def test_other_instantiations(world, dev, N, S_max, rows):
    seg, cd, td = _pack(rows, N, S_max, dev)
    out = world.run(seg, cd, td)
    torch.cuda.synchronize()
    n_coll = _check_rows(N, S_max, rows, out, PRM)
    assert 0 < n_coll < len(rows), n_coll
    _check_hits(N, rows, out, PRM)


def test_gate_only_launch(world, mixed, dev):
    """grad=False (no gradient in LDS, the walk without its gradient terms):
    the same cost, flags and hit location, with and without the near field."""
    seg, cd, td, ref = mixed
    for field in (True, False):
        out = world.run(seg, cd, td, field=field, grad=False)
        torch.cuda.synchronize()
        assert "grad_coeffs" not in out
        for k in ("cost", "collision", "hit_segment", "hit_time"):
            assert _same(out[k], ref[k]), (field, k)
