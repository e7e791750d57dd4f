"""Exact reference for the magnitude-extremum searches: writes
tests/golden/extrema_exact.json.  Run on the CPU (python
tests/golden/make_extrema_exact.py, a few minutes; needs mpmath and the built
oracle); no test runs it, the tests read the JSON only.

Every segment's coefficients are stored as hex floats, so the device gets
bit-identical doubles.  From those doubles, in exact rational arithmetic:

  a_d   = coefficients of p_d^(K) (falling factorials times the doubles),
  f     = sum_d a_d a_d'          (D = 1: the factors a and a' separately; the
                                   candidate list of a one-dimensional
                                   magnitude uses the roots of a' alone),
  count = distinct real roots of f in (0, T) by a Sturm chain of integer
          pseudo-remainders evaluated at 0 and T,
  roots = mpmath.polyroots at 100 digits, each certified by an exact sign
          change of f across r +- T 2^-60; the certified count must equal the
          Sturm count,
  g     = |p^(K)|^2 exactly at 0, T and the roots; the maximum and minimum in
          the reference's order (0, T, roots ascending; strict comparison).

An entry is strict when all roots of f in (0, T) are simple, pairwise at
least 1e-6 T apart and at least 1e-6 T from both ends; at least 80 % of the
entries are (asserted).

Families (the family a segment belongs to is in its name):
  F1  global maximum strictly inside, at T j / 8, j = 1..7, five T.
  F2  a local maximum and a local minimum eps T apart.  (A pair eps apart
      makes g monotone to third order around it, so the side g rises to
      holds larger values: the pair's maximum can be the global one only
      within about eps T of a segment end.  F2 'end' is that case; the
      others sit mid-segment beside a broad global maximum.)  'tang': an
      exact double root of f before rounding.
  F3  Chebyshev polynomials: every root of f real and inside.
  F4  extrema within 1e-9 T of the ends and beyond them.
  F6  degenerate: constant, linear through zero, low true degree, one
      dimension zero.
  F7  one hot segment and three low-magnitude fillers, analysed for
      K = 0..4: the tests build trajectories of 1..129 segments from them.
F5 (power-of-two scaling) is applied by the tests to F1-F3.

'oracle_misses' marks entries where the oracle (companion-matrix
eigenvalues with an |Im| > eps filter) drops a real root or misses the
maximum by more than 1e-10 relative; never set on a strict entry (asserted).
"""
import json
import math
import os
import sys
from fractions import Fraction as F

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "extrema_exact.json")
DIGITS = 28
STRICT_SEP = F(1, 10 ** 6)
T_VALUES = [0.1, 0.75, 1.0, 3.0, 7.3]


def load_fixture():
    with open(PATH) as fh:
        return json.load(fh)


# ---- polynomials as ascending lists of Fractions ---------------------------
def falling(k, i):
    p = 1
    for m in range(k):
        p *= i - m
    return p


def padd(a, b):
    n = max(len(a), len(b))
    return [(a[i] if i < len(a) else 0) + (b[i] if i < len(b) else 0) for i in range(n)]


def pmul(a, b):
    if not a or not b:
        return []
    r = [F(0)] * (len(a) + len(b) - 1)
    for i, x in enumerate(a):
        if x:
            for j, y in enumerate(b):
                r[i + j] += x * y
    return r


def pscale(a, s):
    return [x * s for x in a]


def pder(a):
    return [i * a[i] for i in range(1, len(a))]


def pint(a, c0=F(0)):
    return [c0] + [a[i] / (i + 1) for i in range(len(a))]


def peval(a, t):
    v = F(0)
    for x in reversed(a):
        v = v * t + x
    return v


def ppow(a, n):
    r = [F(1)]
    for _ in range(n):
        r = pmul(r, a)
    return r


def trim(a):
    a = list(a)
    while a and a[-1] == 0:
        a.pop()
    return a


def sign(x):
    return (x > 0) - (x < 0)


def deriv_coeffs(c, K):
    """Exact coefficients of p^(K) from one dimension's doubles c."""
    return [falling(K, i) * F(c[i]) for i in range(K, len(c))]


def mag2(coeffs, K, t):
    return sum(peval(deriv_coeffs(c, K), t) ** 2 for c in coeffs)


# ---- Sturm count and certified roots --------------------------------------
def _to_int(a):
    den = 1
    for x in a:
        den = den * x.denominator // math.gcd(den, x.denominator)
    v = [int(x * den) for x in a]
    g = 0
    for x in v:
        g = math.gcd(g, x)
    return [x // g for x in v]


def _neg_prem(a, b):
    """-(remainder of a by b) times a positive factor; integer lists."""
    r = list(a)
    lb, db = b[-1], len(b) - 1
    while len(r) - 1 >= db and any(r):
        k = len(r) - 1 - db
        lr = r[-1]
        r = [x * abs(lb) for x in r]
        s = lr * (1 if lb > 0 else -1)
        for i, y in enumerate(b):
            r[i + k] -= s * y
        assert r[-1] == 0
        r.pop()
        while r and r[-1] == 0:
            r.pop()
    if not r:
        return []
    g = 0
    for x in r:
        g = math.gcd(g, x)
    return [-x // g for x in r]


def sturm_count(f, T):
    """Distinct real roots of f (no root at 0 or T) in (0, T)."""
    chain = [_to_int(f)]
    chain.append([i * chain[0][i] for i in range(1, len(chain[0]))])
    while len(chain[-1]) > 1:
        nxt = _neg_prem(chain[-2], chain[-1])
        if not nxt:
            break
        chain.append(nxt)

    def var(t):
        sg = [sign(peval([F(x) for x in p], t)) for p in chain]
        sg = [s for s in sg if s]
        return sum(1 for x, y in zip(sg, sg[1:]) if x != y)

    return var(F(0)) - var(T)


def real_roots(f, T):
    """(certified roots of f in (0, T) as Fractions ascending, f stripped of
    its roots at exactly 0 and T).  f == 0 gives ([], [])."""
    import mpmath as mp
    f = trim(f)
    if not f:
        return [], []
    while f[0] == 0:
        f = f[1:]
    while peval(f, T) == 0:  # exact deflation by (t - T)
        q, acc = [], F(0)
        for x in reversed(f):
            acc = acc * T + x
            q.append(acc)
        assert q.pop() == 0
        f = q[::-1]
    if len(f) == 1:
        return [], f
    n = sturm_count(f, T)
    mp.mp.dps = 100
    top = f[-1]
    zs = mp.polyroots([mp.mpf(x.numerator) / mp.mpf(x.denominator) / (mp.mpf(top.numerator) / top.denominator)
                       for x in reversed(f)], maxsteps=400, extraprec=1000)
    h = T / 2 ** 60
    out = []
    for z in zs:
        if abs(mp.im(z)) > mp.mpf(10) ** -40 * float(T):
            continue
        re = mp.re(z)
        r = F(int(mp.floor(re * mp.mpf(2) ** 300)), 2 ** 300)
        if not (h < r < T - h):
            continue
        if sign(peval(f, r - h)) * sign(peval(f, r + h)) < 0:
            out.append(r)
    out.sort()
    assert len(out) == n, ("certified roots differ from the Sturm count", len(out), n)
    return out, f


def dec(x, sqrt=False):
    """A Fraction (or its square root) as a decimal string of DIGITS digits."""
    import mpmath as mp
    mp.mp.dps = 60
    v = mp.mpf(x.numerator) / mp.mpf(x.denominator)
    return mp.nstr(mp.sqrt(v) if sqrt else v, DIGITS) if v else "0.0"


def analyse(coeffs, T, K):
    """The reference data of one (segment, K)."""
    D = len(coeffs)
    T = F(T)
    a = [deriv_coeffs(c, K) for c in coeffs]
    if D == 1:
        rp, fp = real_roots(a[0], T)
        rd, fd = real_roots(pder(a[0]), T)
        assert not set(rp) & set(rd)
        roots = sorted(rp + rd)
        in_list = [r in rd for r in roots]
        f = pmul(fp, fd)
        if f:
            assert sturm_count(f, T) == len(roots)
    else:
        f = []
        for x in a:
            f = padd(f, pmul(x, pder(x)))
        roots, f = real_roots(f, T)
        in_list = [True] * len(roots)
    cand = [F(0), T] + roots
    g = [sum(peval(x, t) ** 2 for x in a) for t in cand]
    for i, keep in enumerate(in_list):  # D = 1: p^(K) is 0 at its own roots
        if not keep:
            g[2 + i] = F(0)
    imax = imin = 0
    for i in range(1, len(cand)):
        if g[i] > g[imax]:
            imax = i
        if g[i] < g[imin]:
            imin = i
    pts = [F(0)] + roots + [T]
    seps = [(y - x) / T for x, y in zip(roots, roots[1:])]
    ends = [min(r, T - r) / T for r in roots]
    minsep = min(seps) if seps else F(1)
    minend = min(ends) if ends else F(1)
    del pts
    return {
        "count": len(roots),
        "sign0": sign(peval(f, F(0))) if f else 0,
        "signT": sign(peval(f, T)) if f else 0,
        "roots": [dec(r) for r in roots],
        "in_list": [int(x) for x in in_list],
        "values": [dec(x, sqrt=True) for x in g],
        "argmax": imax,
        "argmin": imin,
        "min_sep": float(minsep),
        "min_end": float(minend),
        "strict": bool(minsep >= STRICT_SEP and minend >= STRICT_SEP),
    }


# ---- families ---------------------------------------------------------------
def segment(name, N, K, T, pk):
    """Coefficients (doubles) whose K-th derivative is pk (per dimension, a
    list of Fractions, ascending), integrated K times with arbitrary lower
    coefficients and rounded to double."""
    coeffs = []
    for d, a in enumerate(pk):
        a = list(a) + [F(0)] * (N - K - len(a))
        assert len(a) == N - K, name
        low = [float(F((-1) ** i * (i + 2 + d), 7)) for i in range(K)]
        coeffs.append(low + [float(a[j] / falling(K, j + K)) for j in range(N - K)])
    return {"name": name, "N": N, "D": len(pk), "T": T, "coeffs": coeffs, "Ks": [K]}


def lin(t0):
    return [-F(t0), F(1)]


def f1(N, K, D, T, j):
    Tq = F(T)
    ts = Tq * j / 8
    n = N - 1 - K
    amp = [F(3, 2), F(-2), F(5, 4)]
    pk = []
    for d in range(D):
        m = max(n - 2 - d, 0)
        s2 = pscale(ppow(lin(ts), 2), 1 / Tq ** 2)
        w = padd([F(1)], pscale(ppow([F(0), 1 / Tq], m), F(3, 10)))
        pk.append(pscale(padd([F(1)], pscale(pmul(s2, w), -1)), amp[d]))
    return segment(f"F1_N{N}_K{K}_D{D}_T{T}_j{j}", N, K, T, pk)


def f2(N, K, T, eps, kind):
    """h' = (t - t1)(t - t2)(tb - t) w(t): local maximum t1, local minimum
    t2 = t1 + eps T, broad global maximum tb.  'end': the segment ends
    0.4 eps T after t2, h' = (t - t1)(t - t2) w, so t1 is global.
    'tang': t1 = t2."""
    Tq = F(T)
    n = N - 1 - K
    e = F(eps)
    if kind == "end":
        t2 = Tq * (1 - F(4, 10) * e)
        t1 = t2 - Tq * e
        hp = pscale(pmul(lin(t1), lin(t2)), 1 / Tq ** 2)
        m = n - 3
    else:
        t1 = Tq * F(3, 8) if kind == "tang" else Tq * F(5, 16)
        t2 = t1 if kind == "tang" else t1 + Tq * e
        hp = pmul(pscale(pmul(lin(t1), lin(t2)), 1 / Tq ** 2), [F(7, 8), -1 / Tq]) if n >= 4 else \
            pscale(pmul(lin(t1), lin(t2)), 1 / Tq ** 2)
        m = n - 4
    if m > 0:
        hp = pmul(hp, padd([F(1)], pscale(ppow([F(0), 1 / Tq], m), F(1, 5))))
    h = pint(pscale(hp, 1 / Tq), F(2))  # h(0) = 2 keeps h > 0 on [0, T]
    return segment(f"F2_{kind}_N{N}_K{K}_T{T}_e{eps:g}", N, K, T, [h])


def cheb(n, T):
    x = [F(-1), 2 / F(T)]
    t0, t1 = [F(1)], x
    if n == 0:
        return t0
    for _ in range(n - 1):
        t0, t1 = t1, padd(pscale(pmul(x, t1), 2), pscale(t0, -1))
    return t1


def f3(N, K, D, T):
    n = N - 1 - K
    pk = [cheb(n, T)] + ([pscale(cheb(n - 1, T), F(1, 2))] if D == 2 else [])
    return segment(f"F3_N{N}_K{K}_D{D}_T{T}", N, K, T, pk)


def f4(N, K, T, where):
    """h = 1 - ((t - te) / T)^2 (1 + 0.2 (t / T)^m) in x, a constant in y:
    the extremum sits at te, on either side of an end."""
    Tq = F(T)
    te = {"T-": Tq * (1 - F(1, 10 ** 9)), "T+": Tq * (1 + F(1, 10 ** 9)),
          "0+": Tq * F(1, 10 ** 9), "0-": -Tq * F(1, 10 ** 9),
          "T-2^-31": Tq * (1 - F(1, 2 ** 31))}[where]
    n = N - 1 - K
    w = padd([F(1)], pscale(ppow([F(0), 1 / Tq], n - 2), F(1, 5)))
    h = padd([F(1)], pscale(pmul(pscale(ppow(lin(te), 2), 1 / Tq ** 2), w), -1))
    return segment(f"F4_N{N}_K{K}_T{T}_{where}", N, K, T, [h, [F(1, 4)]])


def f6(kind, N, K, T):
    Tq = F(T)
    if kind == "const":
        pk = [[F(3, 2)], [F(-1, 2)], [F(2)]]
    elif kind == "linzero":
        pk = [lin(Tq * F(3, 8))]
    elif kind == "deg3":
        pk = [pmul(lin(Tq * F(1, 4)), pmul(lin(Tq * F(5, 8)), lin(Tq * F(9, 8)))),
              pmul(lin(Tq * F(1, 2)), lin(-Tq))]
    else:  # one dimension identically zero
        pk = [f1(N, K, 1, T, 3)["coeffs"][0][K:], [], [F(1, 3), F(1, 5) / Tq]]
        pk[0] = [falling(K, i + K) * F(x) for i, x in enumerate(pk[0])]
    s = segment(f"F6_{kind}_N{N}_K{K}_T{T}", N, K, T, pk)
    if kind == "zerodim":
        s["coeffs"][1] = [0.0] * N
    return s


def f7_segments():
    """Hot segment (F1 shape at K = 1, maximum at T / 2: a boundary of every
    part count) and three fillers a tenth of its size, all N = 10, D = 3."""
    hot = f1(10, 1, 3, 0.75, 4)
    hot["name"] = "F7_hot"
    segs = [hot]
    for i in range(3):
        T = [1.0, 0.6, 2.5][i]
        pk = []
        for d in range(3):
            pk.append([F(((7 * i + 3 * d + 5 * j) % 11) - 5, 40 * (j + 1) ** 2) / F(T) ** j
                       for j in range(9)])
        s = segment(f"F7_fill{i}", 10, 1, T, pk)
        segs.append(s)
    for s in segs:
        s["Ks"] = [0, 1, 2, 3, 4]
    return segs


def build_segments():
    segs = []
    n = 0
    for ti, T in enumerate(T_VALUES):
        for j in range(1, 8):
            segs.append(f1(10, n % 5, 1 if (j + ti) % 2 else 3, T, j))
            n += 1
    segs.append(f1(4, 0, 3, 0.75, 3))
    segs.append(f1(12, 2, 1, 3.0, 5))
    for i, eps in enumerate([1e-2, 1e-4, 1e-6, 1e-8]):
        segs.append(f2(10, i + 1, T_VALUES[i + 1], eps, "pair"))
    segs.append(f2(10, 0, 1.0, 1e-2, "end"))
    segs.append(f2(10, 2, 0.75, 0, "tang"))
    segs.append(f2(4, 0, 1.0, 1e-2, "pair"))
    segs.append(f2(12, 3, 3.0, 1e-4, "pair"))
    for K in range(5):
        segs.append(f3(10, K, 1, [1.0, 3.0][K % 2]))
        segs.append(f3(10, K, 2, [0.75, 1.0][K % 2]))
    segs.append(f3(4, 1, 1, 1.0))
    segs.append(f3(12, 0, 2, 1.0))
    for i, where in enumerate(["T-", "T+", "0+", "0-", "T-2^-31"]):
        segs.append(f4(10, i, T_VALUES[i], where))
    segs.append(f6("const", 10, 1, 1.0))
    segs.append(f6("linzero", 10, 2, 0.75))
    segs.append(f6("deg3", 10, 0, 3.0))
    segs.append(f6("zerodim", 10, 1, 1.0))
    segs.extend(f7_segments())
    return segs


F7_S = [1, 3, 33, 65, 129]


def trajectories(segs):
    """F7: lists of segment indices.  The hot segment first, in the middle,
    last, and twice (first and last), among cycling fillers."""
    hot = next(i for i, s in enumerate(segs) if s["name"] == "F7_hot")
    fill = [i for i, s in enumerate(segs) if s["name"].startswith("F7_fill")]
    out = []
    for S in F7_S:
        places = {"first": [0], "middle": [S // 2], "last": [S - 1], "twice": [0, S - 1]}
        for name, pos in places.items():
            if S == 1 and name != "first":
                continue
            idx = [hot if s in pos else fill[s % 3] for s in range(S)]
            out.append({"name": f"S{S}_{name}", "S": S, "segments": idx})
    return out


def oracle_check(seg, K, ref):
    """(relative error of the oracle's maximum, largest distance / T of an
    exact list root from the oracle's list)."""
    sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))
    import numpy as np
    import pyoracle
    c = np.array([seg["coeffs"]])
    t = np.array([seg["T"]])
    mx = pyoracle.max_magnitude(seg["N"], c, t, K)
    vals = [float(v) for v in ref["values"]]
    want = vals[ref["argmax"]]
    verr = abs(mx["value"] - want) / want if want else abs(mx["value"])
    ot = pyoracle.magnitude_candidates(seg["N"], c, t, K)[0][0]
    rerr = 0.0
    for r, keep in zip(ref["roots"], ref["in_list"]):
        if keep:
            rerr = max(rerr, float(np.min(np.abs(ot - float(r)))) / seg["T"] if len(ot) else 1.0)
    return verr, rerr


def main():
    segs = build_segments()
    n_entries = n_strict = 0
    for s in segs:
        s["ref"] = {}
        for K in s["Ks"]:
            ref = analyse(s["coeffs"], s["T"], K)
            verr, rerr = oracle_check(s, K, ref)
            ref["oracle_misses"] = bool(verr > 1e-10 or rerr > 1e-7)
            assert not (ref["strict"] and verr > 1e-10), (s["name"], K, verr)
            s["ref"][str(K)] = ref
            n_entries += 1
            n_strict += ref["strict"]
            print(f"{s['name']:34s} K={K} roots={ref['count']:2d} strict={int(ref['strict'])} "
                  f"oracle: value {verr:.1e} roots {rerr:.1e}", flush=True)
        s["coeffs"] = [[float(x).hex() for x in row] for row in s["coeffs"]]
    assert n_strict >= 0.8 * n_entries, (n_strict, n_entries)
    fx = {"strict_sep": float(STRICT_SEP), "entries": n_entries, "strict": n_strict,
          "segments": segs, "trajectories": trajectories(segs)}
    with open(PATH, "w") as fh:
        json.dump(fx, fh, separators=(",", ":"))
        fh.write("\n")
    print(f"{n_entries} entries, {n_strict} strict, {os.path.getsize(PATH)} bytes")


if __name__ == "__main__":
    main()
