"""The magnitude-extremum kernels (mtg_max_magnitude, mtg_min_max_magnitude,
mtg_magnitude_candidates, mtg_soft_constraint_cost) against the exact
fixture tests/golden/extrema_exact.json: adversarial polynomials whose real
roots of f = sum_d p_d^(K) p_d^(K+1) are certified in rational arithmetic
(tests/golden/make_extrema_exact.py describes the families).  Reads the JSON
only.

Value bound (derived, not tuned): the Horner sum of n = N - K terms has error
at most gamma_2n sum_i |a_i| t^i; the norm over the dimensions and the square
root add a factor below 2, so

    |v_dev - v_exact| <= 4 N 2^-53 sum_d sum_i |a_{d,i}| t^i

at the exact extremum's time t, a_{d,i} the coefficients of p_d^(K).  At an
interior extremum g is flat, so the time error enters squared; at 0 and T the
time is exact.  Location tolerance: 1e-7 T, as in
test_extrema_candidates_gpu.py.  Where several candidates tie to rounding
(the Chebyshev family: every extremum is 1, the Horner sum at t = 0 is exact
and at t near T it cancels by eight digits) the bound is taken at the time
of the candidate the device reports, and that candidate's exact value may
differ from the exact extremum by the two candidates' bounds at most; with
no tie this is the bound at the exact extremum's time.

What this file found (the figures are in DESIGN.md §3): max_magnitude and
min_max_magnitude lost a maximum that sits on a part boundary (two of the 37
F1 entries), and magnitude_candidates placed roots of strongly cancelling
polynomials (F3, D = 2) up to 1.5e-2 T off (N = 12: the middle of the
isolating node).  Both are fixed in the kernels; every check here passes.

The lines starting 'extrema' that the tests print (pytest -s) are
profiles/extrema_exact_gpu.txt: per family and entry point the largest value
error as a fraction of the bound and the largest root-location error as a
fraction of T.
"""
import functools
import json
import os
from fractions import Fraction as F

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "extrema_exact.json")
LOC_TOL = 1e-7


@functools.lru_cache(maxsize=None)
def _fixture():
    with open(PATH) as fh:
        fx = json.load(fh)
    for s in fx["segments"]:
        s["c"] = np.array([[float.fromhex(x) for x in row] for row in s["coeffs"]])
    return fx


def _falling(k, i):
    p = 1.0
    for m in range(k):
        p *= i - m
    return p


def _bound(seg, K, t):
    """4 N 2^-53 sum_d sum_i |a_{d,i}| t^i."""
    N = seg["N"]
    a = np.abs(seg["c"][:, K:]) * np.array([_falling(K, i) for i in range(K, N)])
    return 4 * N * 2.0 ** -53 * float(np.sum(a * float(t) ** np.arange(N - K)))


def _cands(seg, K, listed=False):
    """Exact candidates of one segment in the reference's order: (time,
    value as Fraction of the stored decimals)."""
    ref = seg["ref"][str(K)]
    t = [0.0, seg["T"]] + [float(r) for r in ref["roots"]]
    v = [F(x) for x in ref["values"]]
    keep = [True, True] + [bool(k) or not listed for k in ref["in_list"]]
    return [(tt, vv) for tt, vv, k in zip(t, v, keep) if k]


def _family(seg):
    return seg["name"].split("_")[0]


class Stats:
    """Largest value error / bound and location error / T per (family, entry point)."""

    def __init__(self):
        self.d = {}

    def add(self, fam, entry, verr, loc):
        k = (fam, entry)
        a, b = self.d.get(k, (0.0, 0.0))
        self.d[k] = (max(a, verr), max(b, loc))

    def dump(self):
        for (fam, entry), (v, l) in sorted(self.d.items()):
            print(f"extrema {fam:4s} {entry:22s} value/bound {v:.2e} location/T {l:.2e}")


def _check_extremum(segs, K, v_dev, t_dev, s_dev, want_max, stats, entry, tag, scale=1.0):
    """The device's extremum of a trajectory (list of fixture segments)
    against the exact one.  The reported time lies within 1e-7 T of an exact
    candidate c of the reported segment; the reported value is within the
    bound (at c's time) of c's exact value; c is the exact arg-extremum c*,
    or a near-tie: their exact values differ by no more than the two
    evaluation bounds, bound(c) + bound(c*), the most by which FP64 Horner
    sums can invert the comparison.  (Where the extrema tie, as the Chebyshev
    family's do, the candidates' bounds differ by orders of magnitude, so the
    bound belongs to the candidate evaluated; with c = c* this is the bound
    at the exact extremum's time.)"""
    best = None  # (value, segment, time), first strict extremum in order
    for si, seg in enumerate(segs):
        for t, v in _cands(seg, K):
            if best is None or (v > best[0] if want_max else v < best[0]):
                best = (v, si, t)
    if want_max and best[0] == 0:  # Extremum() = {0, 0, 0}
        best = (F(0), 0, 0.0)
    seg = segs[s_dev]
    T = seg["T"]
    assert 0.0 <= t_dev <= T, (tag, t_dev)
    d, t, v = min((abs(t - t_dev), t, v) for t, v in _cands(seg, K))
    assert d <= LOC_TOL * T, (tag, "time", s_dev, t_dev, best)
    bnd = _bound(seg, K, t)
    verr = abs(v_dev / scale - float(v))
    assert verr <= bnd, (tag, "value", v_dev / scale, float(v), verr / bnd)
    if (s_dev, t) != (best[1], best[2]):  # a near-tie
        assert abs(float(v - best[0])) <= bnd + _bound(segs[best[1]], K, best[2]), \
            (tag, "argument", s_dev, t_dev, best)
    stats.add(_family(segs[best[1]]), entry, verr / bnd if bnd else 0.0, d / T)


class Failures(list):
    """Collects assertion failures over the fixture's entries, so one run
    shows them all; check() raises if there were any."""

    def run(self, fn, *a, **k):
        try:
            fn(*a, **k)
        except AssertionError as e:
            self.append(str(e).split("\n")[0])

    def check(self):
        for x in self:
            print("FAIL", x)
        assert not self, f"{len(self)} failures, first: {self[0]}"


def _groups(segs_with_k):
    """(N, D, K) -> list of segments."""
    g = {}
    for seg, K in segs_with_k:
        g.setdefault((seg["N"], seg["D"], K), []).append(seg)
    return g


def _entries(prefixes=None):
    for s in _fixture()["segments"]:
        if prefixes is None or s["name"].startswith(prefixes):
            for K in s["Ks"]:
                yield s, K


def _stack(trajs, dev, scale=1.0):
    """Trajectories (lists of segments, equal S) -> device coeffs, times."""
    c = np.stack([np.stack([s["c"] for s in tr]) for tr in trajs]) * scale
    t = np.array([[s["T"] for s in tr] for tr in trajs])
    return torch.from_numpy(np.ascontiguousarray(c)).to(dev), torch.from_numpy(t).to(dev)


def _run_max_min(trajs, K, dev):
    import mav_tube_trajectory_generation_amd as mtg
    cd, td = _stack(trajs, dev)
    mx = {k: v.cpu().numpy() for k, v in mtg.max_magnitude(cd, td, K).items()}
    mm = {k: v.cpu().numpy() for k, v in mtg.min_max_magnitude(cd, td, K).items()}
    return mx, mm


def test_max_and_min_single_segments(ctx, dev):
    """Every fixture entry as a one-segment trajectory (eight parts per
    segment): max_magnitude and min_max_magnitude."""
    stats, fails = Stats(), Failures()
    for (N, D, K), segs in _groups(_entries()).items():
        mx, mm = _run_max_min([[s] for s in segs], K, dev)
        assert np.array_equal(mm["max_value"], mx["value"])
        assert np.array_equal(mm["max_time"], mx["time"])
        assert np.array_equal(mm["max_segment"], mx["segment"])
        for b, s in enumerate(segs):
            tag = (s["name"], K)
            fails.run(_check_extremum, [s], K, float(mx["value"][b]), float(mx["time"][b]),
                      int(mx["segment"][b]), True, stats, "max_magnitude", tag)
            fails.run(_check_extremum, [s], K, float(mm["min_value"][b]),
                      float(mm["min_time"][b]), int(mm["min_segment"][b]), False, stats,
                      "min_max_magnitude.min", tag)
    stats.dump()
    fails.check()


@pytest.mark.parametrize("S", [1, 3, 33, 65, 129])
def test_max_and_min_placement(ctx, dev, S):
    """F7: the hot segment first, in the middle, last and twice among
    fillers; 8 parts per segment for S = 1, 3; 4 for 33; 2 for 65; 1 for 129.
    B = 5 (several trajectories per 256-lane block, ragged last block) and
    B = 1; all K."""
    fx = _fixture()
    trs = [tr for tr in fx["trajectories"] if tr["S"] == S]
    trajs = [[fx["segments"][i] for i in tr["segments"]] for tr in trs]
    names = [tr["name"] for tr in trs]
    while len(trajs) < 5:
        trajs.append(trajs[len(trajs) % len(trs)])
        names.append(names[len(names) % len(trs)] + "_again")
    stats = Stats()
    for K in range(5):
        for batch, bn in ((trajs, names), (trajs[-2:-1], names[-2:-1])):
            mx, mm = _run_max_min(batch, K, dev)
            assert np.array_equal(mm["max_value"], mx["value"])
            assert np.array_equal(mm["max_time"], mx["time"])
            assert np.array_equal(mm["max_segment"], mx["segment"])
            for b, tr in enumerate(batch):
                tag = (bn[b], K, len(batch))
                _check_extremum(tr, K, float(mx["value"][b]), float(mx["time"][b]),
                                int(mx["segment"][b]), True, stats, f"max_magnitude S{S}", tag)
                _check_extremum(tr, K, float(mm["min_value"][b]), float(mm["min_time"][b]),
                                int(mm["min_segment"][b]), False, stats,
                                f"min_max_magnitude.min S{S}", tag)
                if K == 1 and "twice" in bn[b]:  # the first of two equal maxima wins
                    assert int(mx["segment"][b]) == 0, tag
    stats.dump()


def test_candidates(ctx, dev):
    """magnitude_candidates on every entry.  Strict entries: count, order and
    a one-to-one match with the exact roots within 1e-7 T.  Others: every
    device root within 1e-7 T of an exact root, no time outside [0, T], the
    list's maximum within the value bound, count no larger than exact."""
    import mav_tube_trajectory_generation_amd as mtg
    stats, fails = Stats(), Failures()
    for (N, D, K), segs in _groups(_entries()).items():
        cd, td = _stack([[s] for s in segs], dev)
        out = mtg.magnitude_candidates(cd, td, K)
        ct, cv, cn = (out[x].cpu().numpy() for x in ("time", "value", "count"))
        for b, s in enumerate(segs):
            fails.run(_check_list, s, K, ct[b, 0], cv[b, 0], int(cn[b, 0]), stats)
    stats.dump()
    fails.check()


def _check_list(s, K, ct, cv, n, stats):
    ref = s["ref"][str(K)]
    T = s["T"]
    tag = (s["name"], K)
    ex = _cands(s, K, listed=True)
    ex_roots = np.array([t for t, _ in ex[2:]])
    assert 2 <= n <= ct.shape[0], tag
    t, v = ct[:n], cv[:n]
    assert t[0] == 0.0 and t[1] == T, tag
    roots = t[2:]
    assert np.all((roots >= 0.0) & (roots <= T)), (tag, roots)
    assert np.all(np.diff(roots) > 0), (tag, roots)
    assert n <= len(ex), (tag, "count", roots, ex_roots)
    loc = 0.0
    for r in roots:  # every device root is an exact root
        assert ex_roots.size and np.min(np.abs(ex_roots - r)) <= LOC_TOL * T, \
            (tag, "not a root", r, ex_roots)
        loc = max(loc, float(np.min(np.abs(ex_roots - r))) / T)
    if ref["strict"]:
        assert n == len(ex), (tag, "count", roots, ex_roots)
        for r in ex_roots:
            assert np.min(np.abs(roots - r)) <= LOC_TOL * T, (tag, "missed", r, roots)
    # each listed value against the exact candidate it matches (bound at that
    # candidate's time); the list's maximum is the exact maximum or a near-tie
    # of it (exact values within the two evaluation bounds)
    verr = 0.0
    match = []
    for tt, vv in zip(t, v):
        d, te, ve = min((abs(te - tt), te, ve) for te, ve in ex)
        bnd = _bound(s, K, te)
        assert abs(vv - float(ve)) <= bnd, (tag, "value", tt, vv, float(ve))
        verr = max(verr, abs(vv - float(ve)) / bnd if bnd else 0.0)
        match.append((te, ve))
    vmax, imax = max((ve, -i) for i, (te, ve) in enumerate(ex))
    te, ve = match[int(np.argmax(v))]
    assert float(vmax - ve) <= _bound(s, K, te) + _bound(s, K, ex[-imax][0]), (tag, "maximum")
    stats.add(_family(s), "magnitude_candidates", verr, loc)


@pytest.mark.parametrize("S", [3, 33])
@pytest.mark.parametrize("ders", [[1], [1, 2], [3, 0, 2], [0, 1, 2, 3, 4], [0, 1, 2, 3, 4, 1, 2, 3]],
                         ids=lambda d: f"n{len(d)}")
def test_soft_constraint_maxima_one_launch(ctx, dev, S, ders):
    """soft_constraint_cost's maxima, one launch for all constraints: the
    part count falls 8 / 4 / 2 / 1 with n * group <= 512 (S = 33: 8 for one
    constraint, 4 for two, 2 for three, 1 for five and eight)."""
    import mav_tube_trajectory_generation_amd as mtg
    fx = _fixture()
    trs = [tr for tr in fx["trajectories"] if tr["S"] == S]
    trajs = [[fx["segments"][i] for i in tr["segments"]] for tr in trs]
    cd, td = _stack(trajs, dev)
    out = mtg.soft_constraint_cost(cd, td, ders, [1.0e3] * len(ders), weight=100.0)
    maxima = out["maxima"].cpu().numpy()
    stats = Stats()
    for b, tr in enumerate(trajs):
        for ci, K in enumerate(ders):
            _check_value_only(tr, K, float(maxima[b, ci]), stats, f"soft_cost S{S} n{len(ders)}",
                              (trs[b]["name"], K))
    stats.dump()


def _check_value_only(segs, K, v_dev, stats, entry, tag):
    best = max((v, -si, t) for si, seg in enumerate(segs) for t, v in _cands(seg, K))
    bnd = _bound(segs[-best[1]], K, best[2])
    verr = abs(v_dev - float(best[0]))
    assert verr <= bnd, (tag, v_dev, float(best[0]), verr / bnd)
    stats.add(_family(segs[-best[1]]), entry, verr / bnd if bnd else 0.0, 0.0)


def test_soft_constraint_maxima_per_constraint(ctx, dev):
    """B >= 4096 (one small trajectory tiled): one max_magnitude launch per
    constraint, the last forming the cost."""
    import mav_tube_trajectory_generation_amd as mtg
    fx = _fixture()
    tr = next(t for t in fx["trajectories"] if t["name"] == "S3_middle")
    segs = [fx["segments"][i] for i in tr["segments"]]
    B = 4100
    cd, td = _stack([segs], dev)
    cd, td = cd.repeat(B, 1, 1, 1).contiguous(), td.repeat(B, 1).contiguous()
    ders = [2, 1, 4]
    out = mtg.soft_constraint_cost(cd, td, ders, [1.0e3] * 3, weight=100.0)
    maxima = out["maxima"].cpu().numpy()
    assert np.all(maxima == maxima[0])
    stats = Stats()
    for ci, K in enumerate(ders):
        _check_value_only(segs, K, float(maxima[B - 1, ci]), stats, "soft_cost per-constraint",
                          ("S3_middle", K))
    stats.dump()


@pytest.mark.parametrize("e", [200, -200])
def test_power_of_two_scaling(ctx, dev, e):
    """F5: F1-F3 coefficients times 2^+-200.  Every operation of the search
    commutes with a power-of-two scale short of over/underflow (products and
    sums scale exactly; the Bernstein normalisation divides by the largest
    coefficient, whose reciprocal scales exactly; the pruning, sign and
    convergence tests compare quantities of equal scale), so times, segments
    and counts are bit-identical to the unscaled run and values scale
    exactly."""
    import mav_tube_trajectory_generation_amd as mtg
    sc = 2.0 ** e
    for (N, D, K), segs in _groups(_entries(("F1", "F2", "F3"))).items():
        trajs = [[s] for s in segs]
        c1, td = _stack(trajs, dev)
        c2, _ = _stack(trajs, dev, sc)
        for fn in (mtg.max_magnitude, mtg.min_max_magnitude, mtg.magnitude_candidates):
            a = {k: v.cpu().numpy() for k, v in fn(c1, td, K).items()}
            b = {k: v.cpu().numpy() for k, v in fn(c2, td, K).items()}
            if fn is mtg.magnitude_candidates:
                assert np.array_equal(a["count"], b["count"])
                m = np.arange(a["time"].shape[2])[None, None, :] < a["count"][..., None]
                assert np.array_equal(a["time"][m], b["time"][m]), (N, D, K)
                assert np.array_equal(a["value"][m] * sc, b["value"][m]), (N, D, K)
                continue
            for k in a:
                if "value" in k:
                    assert np.array_equal(a[k] * sc, b[k]), (N, D, K, k, [s["name"] for s in segs])
                else:
                    assert np.array_equal(a[k], b[k]), (N, D, K, k, [s["name"] for s in segs])
