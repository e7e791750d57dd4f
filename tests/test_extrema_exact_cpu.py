"""The exact extrema fixture (tests/golden/extrema_exact.json, made by
tests/golden/make_extrema_exact.py) checked on the CPU with fractions alone:
every stored root sits between two exact sign changes of f, the counts match
the stored Sturm counts, the stored extrema are the extrema of the stored
candidates, at least 80 % of the entries are strict, and the oracle (the
checker of smoke() and of the benchmark's baseline) is measured against the
exact values: 1e-10 relative in value on every strict entry, and everywhere
the fixture does not say 'oracle_misses'."""
import functools
import os
import sys
from fractions import Fraction as F

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)

import make_extrema_exact as gen  # noqa: E402


@functools.lru_cache(maxsize=None)
def _fixture():
    return gen.load_fixture()


def _entries():
    for s in _fixture()["segments"]:
        c = [[float.fromhex(x) for x in row] for row in s["coeffs"]]
        for K in s["Ks"]:
            yield s, c, K, s["ref"][str(K)]


def _f(c, K):
    f = []
    for row in c:
        a = gen.deriv_coeffs(row, K)
        f = gen.padd(f, gen.pmul(a, gen.pder(a)))
    return gen.trim(f)


def test_fixture_table():
    fx = _fixture()
    ents = list(_entries())
    assert len(ents) == fx["entries"]
    strict = sum(r["strict"] for _, _, _, r in ents)
    assert strict == fx["strict"] and strict >= 0.8 * len(ents)
    names = [s["name"] for s in fx["segments"]]
    assert len(set(names)) == len(names)
    for fam in ("F1", "F2", "F3", "F4", "F6", "F7"):
        ks = {K for s, _, K, _ in ents if s["name"].startswith(fam)}
        assert ks, fam
    assert {K for _, _, K, _ in ents} == {0, 1, 2, 3, 4}
    assert {s["N"] for s in fx["segments"]} == {4, 10, 12}
    # F1: every j = 1..7 at every T, both D
    f1 = [s["name"] for s in fx["segments"] if s["name"].startswith("F1_N10")]
    for T in gen.T_VALUES:
        for j in range(1, 8):
            assert any(n.endswith(f"_T{T}_j{j}") for n in f1), (T, j)
    for j in range(1, 8):
        assert {n.split("_")[3] for n in f1 if n.endswith(f"_j{j}")} == {"D1", "D3"}
    for tr in fx["trajectories"]:
        assert len(tr["segments"]) == tr["S"]
        assert len({(fx["segments"][i]["N"], fx["segments"][i]["D"]) for i in tr["segments"]}) == 1
    assert sorted({tr["S"] for tr in fx["trajectories"]}) == gen.F7_S


def test_roots_are_certified_and_counted():
    """Exact sign change of f across r +- T 2^-60 for every stored root (the
    stored decimals carry 28 digits); count equals the Sturm count; strictness
    as stored; roots ascending inside (0, T)."""
    for s, c, K, ref in _entries():
        T = F(s["T"])
        f = _f(c, K)
        roots = [F(r) for r in ref["roots"]]
        assert len(roots) == ref["count"] == len(ref["in_list"]), s["name"]
        assert len(ref["values"]) == ref["count"] + 2
        assert all(0 < r < T for r in roots) and roots == sorted(set(roots)), s["name"]
        h = T / 2 ** 60
        for r in roots:
            assert gen.sign(gen.peval(f, r - h)) * gen.sign(gen.peval(f, r + h)) < 0, (s["name"], K, r)
        # sign pattern between consecutive roots alternates: no root of odd
        # multiplicity between the stored ones at the midpoints
        pts = [F(0)] + roots + [T]
        mids = [gen.sign(gen.peval(f, (x + y) / 2)) for x, y in zip(pts, pts[1:])] if f else []
        assert all(x * y < 0 for x, y in zip(mids, mids[1:])), (s["name"], K)
        seps = [(y - x) / T for x, y in zip(roots, roots[1:])]
        ends = [min(r, T - r) / T for r in roots]
        strict = all(x >= gen.STRICT_SEP for x in seps + ends)
        assert strict == ref["strict"], (s["name"], K)
        if s["D"] > 1:
            assert all(ref["in_list"])
        else:  # the list's roots are the roots of p^(K+1)
            d = gen.pder(gen.deriv_coeffs(c[0], K))
            for r, keep in zip(roots, ref["in_list"]):
                ch = gen.sign(gen.peval(d, r - h)) * gen.sign(gen.peval(d, r + h)) < 0
                assert ch == bool(keep), (s["name"], K, r)


def test_stored_values_and_extrema():
    """values are |p^(K)| at 0, T and the roots (to the 28 stored digits),
    argmax / argmin the first strict extremum in that order."""
    for s, c, K, ref in _entries():
        T = F(s["T"])
        cand = [F(0), T] + [F(r) for r in ref["roots"]]
        vals = [F(v) for v in ref["values"]]
        g = [gen.mag2(c, K, t) for t in cand]
        for i, keep in enumerate(ref["in_list"]):  # a root of a one-dimensional p^(K)
            if not keep:
                assert g[2 + i] <= F(1, 10 ** 45) * max(g)
                g[2 + i] = F(0)
        for v, gg in zip(vals, g):
            assert abs(v * v - gg) <= F(1, 10 ** 25) * max(g), (s["name"], K)
        imax = imin = 0
        for i in range(1, len(cand)):
            if g[i] > g[imax]:
                imax = i
            if g[i] < g[imin]:
                imin = i
        assert (imax, imin) == (ref["argmax"], ref["argmin"]), (s["name"], K)


def test_oracle_against_exact(oracle):
    """The oracle's maximum and candidate list on every entry.  Strict
    entries: value within 1e-10 relative.  Entries not marked oracle_misses:
    value within 1e-10 and every exact list root within 1e-7 T of an oracle
    candidate.  Prints the largest errors (pytest -s)."""
    worst_v = worst_r = 0.0
    marked = []
    for s, c, K, ref in _entries():
        ca, ta = np.array([c]), np.array([s["T"]])
        want = float(ref["values"][ref["argmax"]])
        got = oracle.max_magnitude(s["N"], ca, ta, K)["value"]
        verr = abs(got - want) / want if want else abs(got)
        ot = oracle.magnitude_candidates(s["N"], ca, ta, K)[0][0]
        rerr = 0.0
        for r, keep in zip(ref["roots"], ref["in_list"]):
            if keep:
                rerr = max(rerr, float(np.min(np.abs(ot - float(r)))) / s["T"])
        if ref["strict"]:
            assert verr <= 1e-10, (s["name"], K, verr)
        if ref["oracle_misses"]:
            marked.append((s["name"], K, verr, rerr))
            continue
        assert verr <= 1e-10 and rerr <= 1e-7, (s["name"], K, verr, rerr)
        worst_v, worst_r = max(worst_v, verr), max(worst_r, rerr)
    print(f"oracle vs exact: value {worst_v:.2e} relative, roots {worst_r:.2e} T; "
          f"oracle_misses: {marked}")
