"""Fixtures of the ragged collision objectives (mtg_ragged_coll_cost /
mtg_ragged_coll_optimize): corridor paths of 2..6 segments cut from the
demo's vertices (coll_fixture.py) over its forest map, each with its tube QCQP
start, and the padded layouts of the ragged entries.

A row is (path index, compact x): x is what the oracle and the uniform entries
take for that path: d_p flattened D x np in mode 0, [T; d_p] in mode 1."""
import functools

import numpy as np

import pyoracle
from coll_fixture import (D, M, N, R, MAIN_POSITIONS, forest_map, perturbed_starts,  # noqa: F401
                          tube_pattern, vertices_with_positions)
from helpers import compact_fixed


def _with_midpoints(p, segments):
    out = []
    for i in range(len(p) - 1):
        out.append(p[i])
        if i in segments:
            out.append(0.5 * (p[i] + p[i + 1]))
    out.append(p[-1])
    return np.array(out)


def path_positions():
    """Counts 2, 3, 4 (prefixes of the demo path), 5 (a midpoint in its first
    segment) and 6 (midpoints in its first and last segments)."""
    p = MAIN_POSITIONS
    return [p[:3], p[:4], p[:5], _with_midpoints(p, {0}), _with_midpoints(p, {0, 3})]


@functools.lru_cache(maxsize=None)
def paths():
    """Per path: dict(S, v, vt (tube pattern), t, radii, x0 (the tube QCQP's
    d_p), df [D, 2M], sol (the oracle's tube solve))."""
    out = []
    for pos in path_positions():
        v = vertices_with_positions(pos)
        t = pyoracle.estimate_segment_times(v, 2.0, 2.0)
        radii = np.full((v.S, 2), 0.15)
        sol = pyoracle.tube_solve(N, R, v, t, radii)
        vt = tube_pattern(v)
        _, df = compact_fixed(vt, N)
        out.append(dict(S=v.S, v=v, vt=vt, t=np.asarray(t, dtype=np.float64), radii=radii,
                        x0=sol["x"], df=df, sol=sol, pos=np.asarray(pos)))
    return tuple(out)


def n_vars(S, mode):
    return (S if mode else 0) + D * (S - 1) * M


def pad_x(x, S, S_max, mode, fill=np.nan):
    """Compact x of a path of S segments into a padded row: [3, np_max] in mode
    0, [S_max + 3 np_max] in mode 1."""
    np_b, np_max = (S - 1) * M, (S_max - 1) * M
    x = np.asarray(x, dtype=np.float64)
    off = S if mode else 0
    blk = np.full((D, np_max), fill)
    blk[:, :np_b] = x[off:].reshape(D, np_b)
    if mode == 0:
        return blk
    tt = np.full(S_max, fill)
    tt[:S] = x[:S]
    return np.concatenate([tt, blk.reshape(-1)])


def unpad_x(row, S, S_max, mode):
    np_b, np_max = (S - 1) * M, (S_max - 1) * M
    row = np.asarray(row).reshape(-1)
    off = S_max if mode else 0
    blk = row[off:].reshape(D, np_max)[:, :np_b].reshape(-1)
    return np.concatenate([row[:S], blk]) if mode else blk


def padding_mask(S, S_max, mode):
    """True where a padded row (flattened) holds no variable of the path."""
    m = pad_x(np.zeros(n_vars(S, mode)), S, S_max, mode, fill=1.0)
    return m.reshape(-1) != 0.0


def pack(rows, S_max, mode, fill=np.nan):
    """rows: [(path index, compact x)].  Returns numpy dict(seg_counts [B] int32,
    fixed_vals [B, 3, N], x (padded), times [B, S_max])."""
    P = paths()
    B = len(rows)
    counts = np.array([P[i]["S"] for i, _ in rows], np.int32)
    fixed = np.array([P[i]["df"] for i, _ in rows]).reshape(B, D, N)
    times = np.full((B, S_max), fill)
    for b, (i, _) in enumerate(rows):
        times[b, :P[i]["S"]] = P[i]["t"]
    X = np.array([pad_x(x, P[i]["S"], S_max, mode, fill) for i, x in rows])
    return dict(seg_counts=counts, fixed_vals=fixed, x=X, times=times)


def start_of(i, mode, x=None, t=None):
    """The compact point of path i: x (default the tube start), with the times
    in front in mode 1."""
    p = paths()[i]
    x = p["x0"] if x is None else x
    t = p["t"] if t is None else t
    return np.concatenate([t, x]) if mode else np.asarray(x)


def cost_rows(mode, per_path=3, scale=0.02, seed=11):
    """The evaluation points of the cost tests: each path's tube start and
    per_path - 1 perturbed points (some hit a tree); in mode 1 with times
    scaled by up to +-10 %."""
    rng = np.random.default_rng(3)
    rows = []
    for i, p in enumerate(paths()):
        xs = [p["x0"]] + perturbed_starts(p["x0"], per_path - 1, scale, seed=seed + i)
        for x in xs:
            t = p["t"] * rng.uniform(0.9, 1.1, p["S"]) if mode else None
            rows.append((i, start_of(i, mode, x, t)))
    return rows


@functools.lru_cache(maxsize=None)
def free_starts(i, n, scale=0.01, seed=23):
    """The first n collision-free points of path i among its tube start and
    perturbed_starts(x0, 1, scale, seed + 100 i + j), j = 0, 1, ...: the
    optimiser can only descend from a start outside the trees (inside, J is the
    raise constant), and the 6-segment path's tube start itself grazes one."""
    from coll_fixture import coll_params
    p = paths()[i]
    occ = forest_map()
    out = []
    for j in range(-1, 200):
        x = p["x0"] if j < 0 else perturbed_starts(p["x0"], 1, scale, seed=seed + 100 * i + j)[0]
        if pyoracle.coll_cost(N, R, p["vt"], p["t"], 0, x, occ, coll_params())[3] == 0:
            out.append(x)
            if len(out) == n:
                return tuple(out)
    raise AssertionError(f"path {i}: fewer than {n} collision-free starts")


def opt_rows(mode, n):
    """n optimiser starts cycling over the paths, each collision-free."""
    P = paths()
    per = (n + len(P) - 1) // len(P)
    return [(k % len(P), start_of(k % len(P), mode, free_starts(k % len(P), per)[k // len(P)]))
            for k in range(n)]


def opt_bounds(rows, mode):
    """The reference's bounds (T >= 0.1 in the time variant) and steps
    (0.1 |x|), compact per row."""
    P = paths()
    lo, hi, step = [], [], []
    for i, x in rows:
        l = np.full(x.shape, -np.inf)
        if mode:
            l[:P[i]["S"]] = 0.1
        lo.append(l)
        hi.append(np.full(x.shape, np.inf))
        step.append(0.1 * np.abs(x))
    return lo, hi, step


@functools.lru_cache(maxsize=None)
def oracle_optimize(mode, variant, n, max_evals=25):
    """The oracle's optimiser on opt_rows(mode, n) with the parameters of
    test_coll_gpu.VARIANTS[variant]: per row dict(x, J, evals, result, terms,
    J0 (the start's cost)).  Computed once per (mode, variant, n)."""
    from coll_fixture import coll_params
    from test_coll_gpu import VARIANTS
    prm = coll_params(**VARIANTS[variant])
    P, occ = paths(), forest_map()
    rows = opt_rows(mode, n)
    lo, hi, step = opt_bounds(rows, mode)
    out = []
    for b, (i, x) in enumerate(rows):
        p = P[i]
        J0 = pyoracle.coll_cost(N, R, p["vt"], p["t"], mode, x, occ, prm)[0]
        xo, Jo, ev, res, terms = pyoracle.coll_optimize(N, R, p["vt"], p["t"], mode, x, occ, prm,
                                                        max_evals, lower=lo[b], upper=hi[b],
                                                        initial_step=step[b])
        out.append(dict(x=xo, J=Jo, evals=ev, result=res, terms=terms, J0=J0))
    return tuple(out)
