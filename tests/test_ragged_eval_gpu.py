"""The evaluators of a ragged batch on the GPU (mtg_ragged_max_magnitude,
mtg_ragged_soft_constraint_cost with its feasibility gate,
mtg_ragged_sample_trajectories): rows of different segment counts in one
launch, each against the CPU oracle on its own slice coeffs[b, :S_b],
times[b, :S_b], and against the uniform kernels.

Inputs are standard_vertices / estimate_segment_times(v, 3, 5) /
pyoracle.linear_solve as in test_ragged_gpu.py.  times is NaN-padded as
pack_ragged pads it, outputs are pre-filled with a poison value, and the
coefficient padding is 0.0 (what the ragged solve writes) or NaN: a kernel
that reads padding, or skips an output, shows.

Tolerances (the project's own): extrema values 1e-10 relative against the
oracle with the argmax rule of test_extrema_gpu._check_argmax; soft cost
1e-8; 1e-9 kernel against kernel; sample values 1e-9 (of max(1, |ref|), as
test_sample_gpu.py).  Sample counts are exact against the oracle.  Sample
times are held bit for bit to the rule both sampling kernels document,
(start of the first sampled segment) + k dt in FP64, restated here in
Python, and bit for bit to the uniform kernel.  The oracle restates the
reference's loop, which ADDS dt n times, so its times differ from k dt by
rounding: against it the bound is the accumulation's own worst case,
n 2^-53 (total time) for n samples (n additions, each rounded to half an
ulp of a sum below the total time).
"""
import ctypes
import functools

import numpy as np
import pytest

from helpers import rel_err, standard_vertices

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

POISON = -7.25e77


@functools.lru_cache(maxsize=None)
def _problem(N, D, r, S, seed):
    """(vertices, times, oracle solve) of one standard-pattern trajectory,
    computed once and shared (callers do not modify it)."""
    import pyoracle
    v = standard_vertices(N, S, D, seed)
    t = pyoracle.estimate_segment_times(v, 3.0, 5.0)
    return v, t, pyoracle.linear_solve(N, r, v, t)


@functools.lru_cache(maxsize=None)
def _ref_max(N, D, r, S, seed, k):
    import pyoracle
    _, t, sol = _problem(N, D, r, S, seed)
    return pyoracle.max_magnitude(N, sol["coeffs"], t, k)


def _probs(N, D, r, counts, seed0):
    return [_problem(N, D, r, s, seed0 + b) for b, s in enumerate(counts)]


def _pack(probs, N, D, S_max, dev, pad=0.0):
    """seg_counts, coeffs [B, S_max, D, N] padded with `pad`, times NaN-padded."""
    B = len(probs)
    c = np.full((B, S_max, D, N), pad)
    t = np.full((B, S_max), np.nan)
    for b, (_, tb, sol) in enumerate(probs):
        c[b, :len(tb)] = sol["coeffs"]
        t[b, :len(tb)] = tb
    seg = torch.tensor([len(p[1]) for p in probs], dtype=torch.int32, device=dev)
    return seg, torch.from_numpy(c).to(dev), torch.from_numpy(t).to(dev)


def _max_out(B, dev, guard=0):
    return {"time": torch.full((B + guard,), POISON, dtype=torch.float64, device=dev),
            "value": torch.full((B + guard,), POISON, dtype=torch.float64, device=dev),
            "segment": torch.full((B + guard,), -99, dtype=torch.int32, device=dev)}


def _soft_out(B, nc, dev, guard=0, gated=False):
    o = {"cost": torch.full((B + guard,), POISON, dtype=torch.float64, device=dev),
         "maxima": torch.full((B + guard, nc), POISON, dtype=torch.float64, device=dev)}
    if gated:
        o["gated"] = torch.full((B + guard,), POISON, dtype=torch.float64, device=dev)
    return o


def _head(o, B):
    return {k: v[:B] for k, v in o.items()}


def _np(o):
    return {k: v.cpu().numpy() for k, v in o.items()}


def _check_max_rows(N, D, r, counts, seed0, k, out):
    """ragged_max_magnitude's rows against the oracle on each slice."""
    from test_extrema_gpu import _check_argmax
    o = _np(out)
    for b, s in enumerate(counts):
        _, t, sol = _problem(N, D, r, s, seed0 + b)
        ref = _ref_max(N, D, r, s, seed0 + b, k)
        err = rel_err(o["value"][b], ref["value"])
        print(f"N={N} k={k} row {b} S={s}: value err {err:.3e} seg {o['segment'][b]}")
        assert err <= 1e-10, (k, b, o["value"][b], ref["value"])
        assert 0 <= o["segment"][b] < s, (k, b, o["segment"][b])
        _check_argmax(float(o["time"][b]), int(o["segment"][b]), ref, sol["coeffs"], t, k)


def _check_soft_rows(N, D, r, counts, seed0, ders, lims, out, weight=100.0):
    import pyoracle
    o = _np(out)
    for b, s in enumerate(counts):
        _, t, sol = _problem(N, D, r, s, seed0 + b)
        rc, rm = pyoracle.soft_constraint_cost(N, sol["coeffs"], t, ders, lims, weight)
        print(f"row {b} S={s}: maxima err {np.max(np.abs(o['maxima'][b] - rm) / rm):.3e} "
              f"cost err {rel_err(o['cost'][b], rc):.3e}")
        assert np.allclose(o["maxima"][b], rm, rtol=1e-10, atol=0), (b, o["maxima"][b], rm)
        assert abs(o["cost"][b] - rc) <= 1e-8 * rc, (b, o["cost"][b], rc)


def _run_all_max(seg, cd, td, B, ks, dev):
    import mav_tube_trajectory_generation_amd as mtg
    res = {}
    for k in ks:
        res[k] = mtg.ragged_max_magnitude(seg, cd, td, k, out=_max_out(B, dev))
    torch.cuda.synchronize()
    return res


MIXED = (10, 3, 4, 12, (1, 2, 3, 12, 2, 5, 1), 105)
SOFT = ([1, 2], [3.0, 1.5])


@pytest.fixture(scope="module")
def mixed(ctx, dev):
    """Test 1's launches on the zero-padded batch, shared with the padding,
    bad-row and end-to-end tests."""
    import mav_tube_trajectory_generation_amd as mtg
    N, D, r, S_max, counts, seed0 = MIXED
    probs = _probs(N, D, r, counts, seed0)
    seg, cd, td = _pack(probs, N, D, S_max, dev)
    B = len(counts)
    mx = _run_all_max(seg, cd, td, B, range(5), dev)
    soft = mtg.ragged_soft_constraint_cost(seg, cd, td, *SOFT, out=_soft_out(B, 2, dev))
    torch.cuda.synchronize()
    return probs, seg, cd, td, mx, soft


def test_mixed_counts_vs_oracle(mixed):
    """S = 1, S = 2, odd and even counts, a row without padding, neighbours
    of different length; one chunk per constraint (S_b * 8 <= 64) and two
    (S_b = 12)."""
    N, D, r, S_max, counts, seed0 = MIXED
    _, _, _, _, mx, soft = mixed
    for k in range(5):
        _check_max_rows(N, D, r, counts, seed0, k, mx[k])
    _check_soft_rows(N, D, r, counts, seed0, *SOFT, soft)


def test_padding_is_not_read(mixed, dev):
    """NaN in the coefficient padding as well as in the time padding: bit
    for bit the zero-padded results."""
    import mav_tube_trajectory_generation_amd as mtg
    N, D, r, S_max, counts, seed0 = MIXED
    probs, seg, _, td, mx, soft = mixed
    _, cn, _ = _pack(probs, N, D, S_max, dev, pad=np.nan)
    B = len(counts)
    mx2 = _run_all_max(seg, cn, td, B, range(5), dev)
    soft2 = mtg.ragged_soft_constraint_cost(seg, cn, td, *SOFT, out=_soft_out(B, 2, dev))
    torch.cuda.synchronize()
    for k in range(5):
        for key in ("time", "value", "segment"):
            assert torch.equal(mx2[k][key], mx[k][key]), (k, key)
    assert torch.equal(soft2["cost"], soft["cost"]) and torch.equal(soft2["maxima"], soft["maxima"])
    assert not torch.isnan(soft2["cost"]).any() and not torch.isnan(soft2["maxima"]).any()


def test_more_than_one_pass(ctx, dev):
    """S_max = 64: up to 512 items per constraint, eight chunks of one
    constraint and 24 in all for a four-wave workgroup, beside rows of one
    chunk.  Against the oracle, and against the uniform max_magnitude on each
    sliced row (four parts per segment at S = 64, so not bit for bit)."""
    import mav_tube_trajectory_generation_amd as mtg
    N, D, r, S_max, counts, seed0 = 10, 3, 4, 64, (64, 1, 33, 40), 400
    ders, lims = [1, 2, 3], [3.0, 1.5, 4.0]
    probs = _probs(N, D, r, counts, seed0)
    seg, cd, td = _pack(probs, N, D, S_max, dev)
    B = len(counts)
    mx = _run_all_max(seg, cd, td, B, ders, dev)
    soft = mtg.ragged_soft_constraint_cost(seg, cd, td, ders, lims, out=_soft_out(B, 3, dev))
    torch.cuda.synchronize()
    for k in ders:
        _check_max_rows(N, D, r, counts, seed0, k, mx[k])
    _check_soft_rows(N, D, r, counts, seed0, ders, lims, soft)
    for ci, k in enumerate(ders):  # one kernel: the soft maxima are max_magnitude's values
        assert torch.equal(soft["maxima"][:, ci], mx[k]["value"]), k
    for b, s in enumerate(counts):
        cu, tu = cd[b:b + 1, :s].contiguous(), td[b:b + 1, :s].contiguous()
        for k in ders:
            uni = mtg.max_magnitude(cu, tu, k)
            vu, vr = float(uni["value"][0]), float(mx[k]["value"][b])
            assert rel_err(vr, vu) <= 1e-9, (b, k, vr, vu)
            assert int(uni["segment"][0]) == int(mx[k]["segment"][b]), (b, k)


@pytest.mark.parametrize("N,D,r,S_max,counts", [(8, 2, 3, 5, (5, 1, 4, 2)),
                                                (12, 3, 4, 4, (4, 1, 3)),
                                                (4, 1, 1, 6, (2, 6, 3))])
def test_other_instantiations(ctx, dev, N, D, r, S_max, counts):
    probs = _probs(N, D, r, counts, 300)
    seg, cd, td = _pack(probs, N, D, S_max, dev)
    ks = range(0, min(4, N - 2) + 1)
    mx = _run_all_max(seg, cd, td, len(counts), ks, dev)
    for k in ks:
        _check_max_rows(N, D, r, counts, 300, k, mx[k])


def test_five_constraints(ctx, dev):
    """Five derivatives in one workgroup: five wave-uniform switches, more
    chunks (5 and 5 and 5) than waves."""
    import mav_tube_trajectory_generation_amd as mtg
    N, D, r, S_max, counts, seed0 = 10, 3, 4, 7, (2, 7, 1), 500
    ders, lims = [0, 1, 2, 3, 4], [20.0, 3.0, 1.5, 5.0, 9.0]
    probs = _probs(N, D, r, counts, seed0)
    seg, cd, td = _pack(probs, N, D, S_max, dev)
    soft = mtg.ragged_soft_constraint_cost(seg, cd, td, ders, lims,
                                           out=_soft_out(len(counts), 5, dev))
    torch.cuda.synchronize()
    _check_soft_rows(N, D, r, counts, seed0, ders, lims, soft)


def test_exact_fixture_ragged(ctx, dev):
    """tests/golden/extrema_exact.json (JSON only) packed into ragged
    batches per (N, D, K): every dyadic-maximum entry (F1: the maximum at
    t* = j T / 8, on a part boundary) as a one-segment row, rows of two and
    three of them, and for N = 10, D = 3 the multi-segment placements
    S3_first / middle / last / twice and S33_twice.  Value within the Horner
    bound 4 N 2^-53 sum |a_i| t^i, location within 1e-7 T
    (test_extrema_exact_gpu._check_extremum).  The two entries of DESIGN.md 3
    whose maximum the search once lost report the interior maximum."""
    import mav_tube_trajectory_generation_amd as mtg
    from test_extrema_exact_gpu import Failures, Stats, _check_extremum, _fixture
    fx = _fixture()
    named = {"F1_N10_K4_D3_T1.0_j6": 0.75, "F1_N4_K0_D3_T0.75_j3": 0.75 * 3 / 8}
    groups = {}
    for s in fx["segments"]:
        if s["name"].startswith("F1_"):
            for K in s["Ks"]:
                groups.setdefault((s["N"], s["D"], K), []).append(s)
    seen = set()
    stats, fails = Stats(), Failures()
    for (N, D, K), segs in sorted(groups.items()):
        rows = [[s] for s in segs]
        rows.append([segs[0], segs[-1]])
        rows.append([segs[-1], segs[0], segs[len(segs) // 2]])
        if (N, D) == (10, 3):
            for tr in fx["trajectories"]:
                if tr["name"] in ("S3_first", "S3_middle", "S3_last", "S3_twice", "S33_twice"):
                    rows.append([fx["segments"][i] for i in tr["segments"]])
        S_max = max(len(r) for r in rows)
        B = len(rows)
        c = np.full((B, S_max, D, N), np.nan)
        t = np.full((B, S_max), np.nan)
        for b, row in enumerate(rows):
            c[b, :len(row)] = np.stack([s["c"] for s in row])
            t[b, :len(row)] = [s["T"] for s in row]
        seg = torch.tensor([len(r) for r in rows], dtype=torch.int32, device=dev)
        out = _np(mtg.ragged_max_magnitude(seg, torch.from_numpy(c).to(dev),
                                           torch.from_numpy(t).to(dev), K,
                                           out=_max_out(B, dev)))
        for b, row in enumerate(rows):
            tag = ("+".join(s["name"] for s in row[:3]), len(row), K)
            assert 0 <= out["segment"][b] < len(row), tag
            fails.run(_check_extremum, row, K, float(out["value"][b]), float(out["time"][b]),
                      int(out["segment"][b]), True, stats, "ragged_max_magnitude", tag)
            if len(row) == 1 and row[0]["name"] in named:
                T, ts = row[0]["T"], named[row[0]["name"]]
                seen.add(row[0]["name"])
                assert abs(out["time"][b] - ts) <= 1e-7 * T, (tag, out["time"][b], ts)
    stats.dump()
    fails.check()
    assert seen == set(named)


def test_bad_rows_stay_in_their_row(ctx, dev):
    """Counts outside [1, S_max]: the failure values in the row's own
    outputs, the good rows bit for bit what a clean launch gives, the guard
    rows behind every output buffer untouched."""
    import mav_tube_trajectory_generation_amd as mtg
    N, D, r, S_max = 10, 3, 4, 12
    counts = [3, 0, 13, 4, -1]
    B, G = len(counts), 2
    good = {0: _problem(N, D, r, 3, 600), 3: _problem(N, D, r, 4, 603)}
    c = np.full((B, S_max, D, N), np.nan)
    t = np.full((B, S_max), np.nan)
    for b, (_, tb, sol) in good.items():
        c[b, :len(tb)] = sol["coeffs"]
        t[b, :len(tb)] = tb
    seg = torch.tensor(counts, dtype=torch.int32, device=dev)
    cd, td = torch.from_numpy(c).to(dev), torch.from_numpy(t).to(dev)
    gate = torch.arange(1.0, B + 1.0, dtype=torch.float64, device=dev)
    lims = [1.0e3, 1.0e3]  # every good row feasible
    fm, fs = _max_out(B, dev, G), _soft_out(B, 2, dev, G, gated=True)
    mx = mtg.ragged_max_magnitude(seg, cd, td, 1, out=_head(fm, B))
    soft = mtg.ragged_soft_constraint_cost(seg, cd, td, [1, 2], lims, gate=gate, out=_head(fs, B))
    n_max = 257
    smp, st, cnt = _sample_raw(seg, cd, td, 0.05, 0.0, -1.0, 1, n_max, dev, guard=G)
    torch.cuda.synchronize()
    for b in (1, 2, 4):
        assert torch.isnan(mx["value"][b]) and torch.isnan(mx["time"][b]), b
        assert int(mx["segment"][b]) == -1, b
        assert torch.isnan(soft["cost"][b]) and torch.isnan(soft["maxima"][b]).all(), b
        assert float(soft["gated"][b]) == float("inf"), b
        assert int(cnt[b]) == -1, b
        assert torch.all(smp[b] == POISON) and torch.all(st[b] == POISON), b
    # the good rows against a clean launch of the same two trajectories
    rows = [good[0], good[3]]
    seg2, c2, t2 = _pack(rows, N, D, S_max, dev, pad=np.nan)
    mx2 = mtg.ragged_max_magnitude(seg2, c2, t2, 1)
    soft2 = mtg.ragged_soft_constraint_cost(seg2, c2, t2, [1, 2], lims)
    smp2, st2, cnt2 = _sample_raw(seg2, c2, t2, 0.05, 0.0, -1.0, 1, n_max, dev)
    torch.cuda.synchronize()
    for j, b in enumerate((0, 3)):
        for key in ("time", "value", "segment"):
            assert torch.equal(mx[key][b], mx2[key][j]), (b, key)
        assert torch.equal(soft["cost"][b], soft2["cost"][j])
        assert torch.equal(soft["maxima"][b], soft2["maxima"][j])
        assert float(soft["gated"][b]) == float(gate[b])
        assert int(cnt[b]) == int(cnt2[j]) > 0
        assert torch.equal(smp[b], smp2[j]) and torch.equal(st[b], st2[j])
    for key in ("time", "value"):
        assert torch.all(fm[key][B:] == POISON), key
    assert torch.all(fm["segment"][B:] == -99)
    for key in ("cost", "maxima", "gated"):
        assert torch.all(fs[key][B:] == POISON), key
    assert torch.all(smp[B:] == POISON) and torch.all(st[B:] == POISON)
    assert torch.all(cnt[B:] == -99)


def _select(costs, dev, start=1000, rank=3):
    from mav_tube_trajectory_generation_amd import lib
    from mav_tube_trajectory_generation_amd._abi import check
    triple = torch.empty(3, dtype=torch.float64, device=dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    check(lib().mtg_select_local(ctypes.c_void_p(costs.data_ptr()), costs.numel(), start, rank,
                                 ctypes.c_void_p(triple.data_ptr()), stream), "mtg_select_local")
    return triple


def test_gate_and_selection(ctx, dev, oracle):
    """The feasibility gate feeds mtg_select_local without a host step:
    limits halfway between the two middle maxima of 16 rows, so both classes
    exist and no maximum is within rounding of its limit."""
    import mav_tube_trajectory_generation_amd as mtg
    N, D, r, S_max, seed0 = 10, 3, 4, 8, 800
    counts = tuple(2 + (5 * b) % 7 for b in range(16))
    ders = [1, 2]
    probs = _probs(N, D, r, counts, seed0)
    ref = np.array([[_ref_max(N, D, r, s, seed0 + b, k)["value"] for k in ders]
                    for b, s in enumerate(counts)])
    srt = np.sort(ref, axis=0)
    lims = (0.5 * (srt[7] + srt[8])).tolist()
    # conditions on the inputs, from the oracle's values alone
    assert np.all(np.abs(ref - lims) >= 1e-6 * np.array(lims)), (ref, lims)
    feasible = np.all(ref <= lims, axis=1)
    assert feasible.sum() >= 2 and not feasible.all(), feasible
    cost = np.array([p[2]["cost"] for p in probs])
    seg, cd, td = _pack(probs, N, D, S_max, dev)
    B = len(counts)
    gate = torch.from_numpy(cost).to(dev)
    out = mtg.ragged_soft_constraint_cost(seg, cd, td, ders, lims, gate=gate,
                                          out=_soft_out(B, 2, dev, gated=True))
    torch.cuda.synchronize()
    gated = out["gated"].cpu().numpy()
    assert np.array_equal(gated[feasible], cost[feasible])
    assert np.all(gated[~feasible] == np.inf)
    j = int(np.argmin(np.where(feasible, cost, np.inf)))
    assert _select(out["gated"], dev).cpu().tolist() == [cost[j], 1000.0 + j, 3.0]
    # a NaN gate passes through (and loses the selection); aliased call
    g2 = gate.clone()
    g2[j] = float("nan")
    infeasible_row = int(np.flatnonzero(~feasible)[0])
    g2[infeasible_row] = float("nan")
    want = np.where(feasible, g2.cpu().numpy(), np.inf)
    o2 = mtg.ragged_soft_constraint_cost(seg, cd, td, ders, lims, gate=g2)
    got = o2["gated"].cpu().numpy()
    assert np.isnan(got[j]) and got[infeasible_row] == np.inf
    assert np.array_equal(got, want, equal_nan=True)
    alias = g2.clone()
    o3 = mtg.ragged_soft_constraint_cost(seg, cd, td, ders, lims, gate=alias,
                                         out={"gated": alias})
    torch.cuda.synchronize()
    assert o3["gated"].data_ptr() == alias.data_ptr()
    assert np.array_equal(alias.cpu().numpy(), want, equal_nan=True)
    assert torch.equal(o3["cost"], out["cost"]) and torch.equal(o3["maxima"], out["maxima"])
    j2 = int(np.nanargmin(want))
    assert _select(alias, dev).cpu().tolist() == [want[j2], 1000.0 + j2, 3.0]


def _sample_raw(seg, cd, td, dt, t_start, t_end, K, n_max, dev, guard=0):
    """mtg_ragged_sample_trajectories into poisoned buffers (with guard rows)."""
    from mav_tube_trajectory_generation_amd import lib
    from mav_tube_trajectory_generation_amd._abi import check
    B, S_max, D, N = cd.shape
    smp = torch.full((B + guard, (K + 1) * D, n_max), POISON, dtype=torch.float64, device=dev)
    st = torch.full((B + guard, n_max), POISON, dtype=torch.float64, device=dev)
    cnt = torch.full((B + guard,), -99, dtype=torch.int32, device=dev)
    p = lambda x: ctypes.c_void_p(x.data_ptr())  # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    check(lib().mtg_ragged_sample_trajectories(N, D, S_max, B, p(seg), p(cd), p(td), t_start,
                                               t_end, dt, n_max, K, p(smp), p(st), p(cnt),
                                               stream), "mtg_ragged_sample_trajectories")
    return smp, st, cnt


def _rule_times(t, t_start, dt, n):
    """The documented sample times in FP64: start of the first sampled
    segment (found as the kernels find it) + k dt."""
    acc, i = 0.0, 0
    for i in range(len(t)):
        acc += float(t[i])
        if acc > t_start:
            break
    acc -= float(t[i])
    return acc + np.arange(n, dtype=np.float64) * dt


def _check_samples(N, D, probs, smp, st, cnt, dt, t_start, t_end, K, n_max):
    import pyoracle
    smp, st, cnt = smp.cpu().numpy(), st.cpu().numpy(), cnt.cpu().numpy()
    for b, (_, t, sol) in enumerate(probs):
        total = float(np.sum(t))
        te = total if t_end < 0 else t_end
        n = None
        for k in range(K + 1):
            ref, rt, n = pyoracle.evaluate_range(N, sol["coeffs"], t, t_start, te, dt, k)
            assert n <= n_max, "the test's n_max must hold every sample"
            assert cnt[b] == n, (b, k, cnt[b], n)
            got = smp[b, k * D:(k + 1) * D, :n].T
            scale = max(1.0, np.abs(ref).max()) if n else 1.0
            err = np.max(np.abs(got - ref)) / scale if n else 0.0
            assert err <= 1e-9, (b, k, err)
        want = _rule_times(t, t_start, dt, n)
        assert np.array_equal(st[b, :n], want), (b, np.max(np.abs(st[b, :n] - want)))
        terr = np.max(np.abs(st[b, :n] - rt)) if n else 0.0
        print(f"row {b} S={len(t)}: n {n} times vs oracle {terr:.3e} "
              f"(bound {n * 2.0 ** -53 * max(total, te):.3e})")
        assert terr <= n * 2.0 ** -53 * max(total, te), (b, terr)
        assert np.all(smp[b, :, n:] == POISON) and np.all(st[b, n:] == POISON), b


SAMPLE = (10, 3, 4, 12, (1, 2, 5, 12, 3), 900)
# 64 x 3 x 3 x 10 > 4096: the first row is sampled without the pre-scaled table
UNSCALED = (10, 3, 4, 64, (64, 1, 33), 400)


def _n_max(probs, dt, odd=False):
    """Room for the longest row's samples; even, or odd for the 8-byte stores."""
    n = int(max(float(np.sum(p[1])) for p in probs) / dt) + 3
    return n + (n % 2 != int(odd))


@pytest.mark.parametrize("t_start,t_end,K,odd", [
    (0.0, -1.0, 2, False),   # whole rows; even n_max: paired 16-byte stores
    (0.3, 2.0, 2, False),    # a window
    (0.0, -1.0, 2, True),    # odd n_max: 8-byte stores
    (0.0, -1.0, 4, False),   # five derivatives
], ids=["whole", "window", "odd", "deriv4"])
def test_sampling_vs_oracle(ctx, dev, t_start, t_end, K, odd):
    N, D, r, S_max, counts, seed0 = SAMPLE
    probs = _probs(N, D, r, counts, seed0)
    n_max = 256 + int(odd) if t_end > 0 else _n_max(probs, 0.01, odd)
    seg, cd, td = _pack(probs, N, D, S_max, dev, pad=np.nan)
    smp, st, cnt = _sample_raw(seg, cd, td, 0.01, t_start, t_end, K, n_max, dev)
    torch.cuda.synchronize()
    _check_samples(N, D, probs, smp, st, cnt, 0.01, t_start, t_end, K, n_max)


def test_sampling_unscaled_rows(ctx, dev):
    """S_b K D N above the pre-scaled table (64 x 3 x 3 x 10 > 4096) in one
    row, below it in its neighbours, inside one launch's LDS for S_max = 64
    (at S_max = 12, N = 10, D = 3 even five derivatives fit the table)."""
    N, D, r, S_max, counts, seed0 = UNSCALED
    probs = _probs(N, D, r, counts, seed0)
    dt = 0.05
    n_max = _n_max(probs, dt)
    seg, cd, td = _pack(probs, N, D, S_max, dev, pad=np.nan)
    smp, st, cnt = _sample_raw(seg, cd, td, dt, 0.0, -1.0, 2, n_max, dev)
    torch.cuda.synchronize()
    _check_samples(N, D, probs, smp, st, cnt, dt, 0.0, -1.0, 2, n_max)


@pytest.mark.parametrize("shape,dt,odd", [
    (SAMPLE, 0.01, False),    # paired 16-byte stores
    (SAMPLE, 0.01, True),     # 8-byte stores
    (UNSCALED, 0.05, False),  # the 64-segment row without the pre-scaled table
], ids=["even", "odd", "unscaled"])
def test_sampling_vs_uniform_kernel(ctx, dev, shape, dt, odd):
    """Every row as a uniform batch of one with the same n_max: counts, times
    and values bit for bit (both kernels run one sampling body, so a row's
    values are the same FMA sequence whichever of its paths the row takes)."""
    import mav_tube_trajectory_generation_amd as mtg
    N, D, r, S_max, counts, seed0 = shape
    probs = _probs(N, D, r, counts, seed0)
    n_max = _n_max(probs, dt, odd)
    seg, cd, td = _pack(probs, N, D, S_max, dev, pad=np.nan)
    smp, st, cnt = mtg.ragged_sample_trajectories(seg, cd, td, dt, max_derivative=2,
                                                  n_max=n_max)
    for b, s in enumerate(counts):
        us, ut, uc = mtg.sample_trajectories(cd[b:b + 1, :s].contiguous(),
                                             td[b:b + 1, :s].contiguous(), dt,
                                             max_derivative=2, n_max=n_max)
        n = int(uc[0])
        assert int(cnt[b]) == n > 0, (b, int(cnt[b]), n)
        assert torch.equal(st[b, :n], ut[0, :n]), b
        diff = float((smp[b, :, :n] - us[0, :, :n]).abs().max())
        print(f"row {b} S={s}: n {n} max |ragged - uniform| {diff:.3e}")
        assert torch.equal(smp[b, :, :n], us[0, :, :n]), (b, diff)


def test_default_n_max_from_masked_sums(ctx, dev):
    """The Python default reads the counts once: NaN padding must not reach
    the row sums."""
    import mav_tube_trajectory_generation_amd as mtg
    N, D, r, S_max, counts, seed0 = SAMPLE
    probs = _probs(N, D, r, counts, seed0)
    seg, cd, td = _pack(probs, N, D, S_max, dev)
    smp, st, cnt = mtg.ragged_sample_trajectories(seg, cd, td, 0.01)
    longest = max(float(np.sum(p[1])) for p in probs)
    assert smp.shape[2] % 64 == 0 and smp.shape[2] >= longest / 0.01 + 1
    assert int(longest / 0.01) <= int(cnt.max()) <= smp.shape[2] and int(cnt.min()) > 0
    assert st is not None and smp.shape[:2] == (len(counts), D)


def test_graph_replay_with_other_counts(ctx, dev):
    """solve -> soft cost with gate -> select captured on one stream, then
    replayed over another mix of counts written in place: no launch holds
    host knowledge of the counts."""
    import mav_tube_trajectory_generation_amd as mtg
    N, D, r, S_max = 10, 3, 4, 12
    first, second = (4, 9, 1, 12, 2), (12, 1, 6, 2, 11)
    ders = [1, 2]
    B = len(first)
    # limits between the third and fourth maxima of the replayed batch
    # (oracle values), so the gate has rows of both classes to decide
    ref = np.array([[_ref_max(N, D, r, s, 720 + b, k)["value"] for k in ders]
                    for b, s in enumerate(second)])
    srt = np.sort(ref, axis=0)
    lims = (0.5 * (srt[2] + srt[3])).tolist()
    ok = np.all(ref <= lims, axis=1)
    assert np.all(np.abs(ref - lims) >= 1e-6 * np.array(lims)) and ok.any() and not ok.all()
    plan = mtg.RaggedLinearPlan(ctx, N, D, r, S_max)

    def inputs(counts, seed0):
        probs = _probs(N, D, r, counts, seed0)
        return mtg.pack_ragged([(p[2]["df"], p[1]) for p in probs], N, dev, S_max=S_max)

    def fresh():
        return ({"coeffs": torch.full((B, S_max, D, N), POISON, dtype=torch.float64, device=dev),
                 "cost": torch.full((B,), POISON, dtype=torch.float64, device=dev)},
                _soft_out(B, 2, dev, gated=True),
                torch.full((3,), POISON, dtype=torch.float64, device=dev))

    def pipeline(seg, fixed, times, sol, soft, triple):
        from mav_tube_trajectory_generation_amd import lib
        from mav_tube_trajectory_generation_amd._abi import check
        plan.solve(seg, fixed, times, status=False, out=sol)
        mtg.ragged_soft_constraint_cost(seg, sol["coeffs"], times, ders, lims, gate=sol["cost"],
                                        out=soft)
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        check(lib().mtg_select_local(ctypes.c_void_p(soft["gated"].data_ptr()), B, 0, 0,
                                     ctypes.c_void_p(triple.data_ptr()), stream),
              "mtg_select_local")

    seg, fixed, times = inputs(first, 700)
    sol, soft, triple = fresh()
    pipeline(seg, fixed, times, sol, soft, triple)  # warm-up: LDS attributes, module load
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        pipeline(seg, fixed, times, sol, soft, triple)
    seg2, fixed2, times2 = inputs(second, 720)
    seg.copy_(seg2)
    fixed.copy_(fixed2)
    times.copy_(times2)
    for o in (sol, soft):
        for v in o.values():
            v.fill_(POISON)
    triple.fill_(POISON)
    g.replay()
    torch.cuda.synchronize()
    sol_e, soft_e, triple_e = fresh()
    pipeline(seg2, fixed2, times2, sol_e, soft_e, triple_e)
    torch.cuda.synchronize()
    for k in soft:
        assert torch.equal(soft[k], soft_e[k]), k
    assert torch.equal(sol["coeffs"], sol_e["coeffs"]) and torch.equal(sol["cost"], sol_e["cost"])
    assert torch.equal(triple, triple_e)
    gated = soft["gated"].cpu().numpy()
    assert np.isfinite(gated).any() and np.isinf(gated).any()  # the gate decided something
    assert triple.cpu().tolist() == [gated.min(), float(np.argmin(gated)), 0.0]


def test_end_to_end_from_ragged_solve(ctx, dev, mixed):
    """RaggedLinearPlan.solve's own coeffs (0.0 padding) and pack_ragged's
    NaN-padded times straight into the three calls.  The solve is held to
    helpers.REL_TOL = 1e-6 against the oracle's coefficients, and the
    evaluators are 1-Lipschitz in relative terms on them, so against the
    oracle-coefficient results: extrema, maxima and sample values 1e-6,
    segments equal, sample counts and times bit for bit (they depend on the
    times alone)."""
    import mav_tube_trajectory_generation_amd as mtg
    N, D, r, S_max, counts, seed0 = MIXED
    probs, seg0, cd0, td0, mx0, soft0 = mixed
    seg, fixed, times = mtg.pack_ragged([(p[2]["df"], p[1]) for p in probs], N, dev, S_max=S_max)
    plan = mtg.RaggedLinearPlan(ctx, N, D, r, S_max)
    sol = plan.solve(seg, fixed, times)
    B = len(counts)
    assert torch.isnan(times[0, 1:]).all() and torch.all(sol["coeffs"][0, 1:] == 0.0)
    for k in (0, 1, 2):
        mx = mtg.ragged_max_magnitude(seg, sol["coeffs"], times, k)
        a, b0 = mx["value"].cpu().numpy(), mx0[k]["value"].cpu().numpy()
        print(f"k={k}: value vs oracle-coefficient run {np.max(np.abs(a - b0) / b0):.3e}")
        assert np.all(np.abs(a - b0) <= 1e-6 * b0), (k, a, b0)
        assert torch.equal(mx["segment"], mx0[k]["segment"]), k
    soft = mtg.ragged_soft_constraint_cost(seg, sol["coeffs"], times, *SOFT, gate=sol["cost"])
    m, m0 = soft["maxima"].cpu().numpy(), soft0["maxima"].cpu().numpy()
    assert np.all(np.abs(m - m0) <= 1e-6 * m0)
    lim = np.array(SOFT[1])
    want = np.where(np.all(m <= lim, axis=1), sol["cost"].cpu().numpy(), np.inf)
    assert np.array_equal(soft["gated"].cpu().numpy(), want)
    n_max = _n_max(probs, 0.01)
    smp, st, cnt = mtg.ragged_sample_trajectories(seg, sol["coeffs"], times, 0.01,
                                                  max_derivative=2, n_max=n_max)
    smp0, st0, cnt0 = _sample_raw(seg0, cd0, td0, 0.01, 0.0, -1.0, 2, n_max, dev)
    torch.cuda.synchronize()
    assert torch.equal(cnt, cnt0) and int(cnt.min()) > 0
    for b in range(B):
        n = int(cnt[b])
        assert torch.equal(st[b, :n], st0[b, :n]), b
        scale = max(1.0, float(smp0[b, :, :n].abs().max()))
        assert float((smp[b, :, :n] - smp0[b, :, :n]).abs().max()) <= 1e-6 * scale, b
