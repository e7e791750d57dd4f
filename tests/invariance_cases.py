"""Problems and exact transformations shared by the symmetry tests
(test_invariance_oracle.py on the CPU oracle, test_invariance_gpu.py on the
kernels).

The symmetries are properties of the problems themselves (a translated,
rotated or reversed tube problem is the same problem), so they hold whatever
the oracle computes.  Every transformation here is exact in FP64: positions
are rounded to multiples of 2^-20 and offsets are sums of a few powers of two,
so `pos + off`, the tube solve's origin `((pos_0 + off) + (pos_S + off)) / 2`
(a multiple of 2^-21 below 2^23) and `(pos + off) - origin` carry no
rounding, and the signed axis permutation and the reversal only move and
negate numbers.
"""
import numpy as np

# (N, r, S, seed): main.cpp's geometry is added by tube_problems().  The
# N = 10 cases are the reference sizes (S = 2 .. 16 are compile-time-S
# kernels); N = 6 and N = 12 are the kernel's other lane layouts, their seeds
# picked so that the oracle converges on the plain and on the shifted problem.
TUBE_RANDOM = [(10, 4, 2, 314), (10, 4, 3, 321), (10, 4, 5, 335), (10, 4, 10, 105),
               (10, 4, 16, 412), (6, 2, 5, 330), (12, 5, 6, 330)]

# Each component is a sum of powers of two below 2^23, so adding it to a
# multiple of 2^-20 of magnitude < 2^5 is exact (52 fraction bits).
OFFSETS = np.array([[128.0, -64.0, 32.0], [1024.0, -2048.0, 512.0],
                    [16384.0, 16384.0, 16384.0], [524288.0, 4194304.0, 256.0]])

TUBE_RADIUS = 0.15
TUBE_TOL, TUBE_MAX_ITER = 1e-10, 100


def quantise(a):
    return np.round(np.asarray(a, float) * 2.0 ** 20) / 2.0 ** 20


def main_cpp_vertices(oracle, M=5):
    """The 4-segment geometry of the reference's src/main.cpp:26-53."""
    S, D = 4, 3
    mask = np.zeros((S + 1, M), np.uint8)
    vals = np.zeros((S + 1, M, D))
    pts = [(2.7, 9.5, 4.8), (3.50796, 4.34802, 4.56653), (3.95552, 3.23008, 4.75131),
           (5.06673, 2.31032, 4.79433), (7.0, 2.2, 4.8)]
    for v, p in enumerate(pts):
        mask[v, 0] = 1
        vals[v, 0] = p
    mask[0, :] = 1
    mask[S, :] = 1
    return oracle.Vertices(mask, vals)


def tube_problems(oracle):
    """[(name, N, r, vertices, T0)]: positions on the 2^-20 grid, times from
    estimate_segment_times(3, 5) of the rounded positions (2, 2 for main.cpp,
    as main.cpp:73-74)."""
    out = []
    v = main_cpp_vertices(oracle)
    v.vals[:, 0, :] = quantise(v.vals[:, 0, :])
    out.append(("main_cpp", 10, 4, v, oracle.estimate_segment_times(v, 2.0, 2.0)))
    for N, r, S, seed in TUBE_RANDOM:
        v = oracle.random_vertices(N // 2 - 1, S, 3, -10.0, 10.0, seed)
        v.vals[:, 0, :] = quantise(v.vals[:, 0, :])
        out.append((f"N{N}_S{S}_seed{seed}", N, r, v,
                    oracle.estimate_segment_times(v, 3.0, 5.0)))
    return out


def translate(oracle, v, off):
    vals = v.vals.copy()
    vals[:, 0, :] += np.asarray(off, float)[None, :] * v.mask[:, 0, None]
    return oracle.Vertices(v.mask, vals)


def permute_axes(a):
    """(x, y, z) -> (z, -x, y) on the last axis: a proper rotation that maps
    axes to axes, so it commutes with every entrywise snap of the assembly."""
    a = np.asarray(a)
    return np.stack([a[..., 2], -a[..., 0], a[..., 1]], axis=-1)


def permute_vertices(oracle, v):
    return oracle.Vertices(v.mask, permute_axes(v.vals))


def reverse_vertices(oracle, v):
    """The same path flown backwards: vertices in reverse order, odd
    derivatives negated (d/d(-t))."""
    vals = v.vals[::-1].copy()
    vals[:, 1::2, :] *= -1.0
    return oracle.Vertices(v.mask[::-1].copy(), vals)


def x_translate(x, off, N, S):
    """Shift the position entries of a tube free-variable vector
    x[d][vertex 1..S-1][derivative 0..N/2-1]."""
    y = np.array(x, float).reshape(3, S - 1, N // 2).copy()
    y[:, :, 0] += np.asarray(off, float)[:, None]
    return y.reshape(np.shape(x))


def poly_derivatives(c, t, kmax):
    """Derivatives 0..kmax-1 at t of the polynomials c[..., N] (ascending
    powers): array [..., kmax]."""
    c = np.asarray(c, float)
    N = c.shape[-1]
    k = np.arange(N)
    out = []
    for d in range(kmax):
        f = np.ones(N)
        for m in range(d):
            f = f * np.maximum(k - m, 0)
        p = np.where(k >= d, np.asarray(t, float)[..., None] ** np.maximum(k - d, 0), 0.0)
        out.append(np.sum(c * f * p, axis=-1))
    return np.stack(out, axis=-1)


# ------------------------------------------------------------------ checks
# Shared by the oracle and the GPU file; a result is a dict with status,
# iters, cost, coeffs [S, 3, N] (and x where needed).  Each check returns the
# deviations it measured so the caller can print them.

def check_tube_translation(base, moved, off):
    """The moved problem is the same problem bit for bit once it is taken
    relative to the midpoint of its first and last vertex, so status and
    iteration count are equal; 1e-12 on the cost (relative) and on the
    non-constant coefficients (absolute) leaves room for another exact
    choice of origin.  Adding the origin back rounds the constant
    coefficient at the offset's magnitude: one ulp of the largest offset
    component."""
    assert moved["status"] == base["status"], (moved["status"], base["status"])
    assert moved["iters"] == base["iters"], (moved["iters"], base["iters"])
    dj = abs(moved["cost"] - base["cost"]) / abs(base["cost"])
    assert dj <= 1e-12, dj
    c, c0 = np.asarray(moved["coeffs"]), np.asarray(base["coeffs"])
    dc = float(np.max(np.abs(c[..., 1:] - c0[..., 1:])))
    assert dc <= 1e-12, dc
    d0 = float(np.max(np.abs((c[..., 0] - np.asarray(off)[None, :]) - c0[..., 0])))
    assert d0 <= np.spacing(np.max(np.abs(off))), (d0, np.spacing(np.max(np.abs(off))))
    return dj, dc, d0


def rel_coeffs(got, ref):
    """helpers.rel_err_coeffs: normwise per (segment, dimension)."""
    num = np.linalg.norm(np.asarray(got) - np.asarray(ref), axis=-1)
    den = np.linalg.norm(np.asarray(ref), axis=-1)
    return float(np.max(num / np.maximum(den, 1e-12)))


def check_tube_permutation(base, perm, cost_tol=1e-6):
    """The solver is not bitwise symmetric under a rotation (the block
    factorisation orders the dimensions), so this is held to the project's
    1e-6 tube parity bar and +-2 iterations."""
    assert perm["status"] == base["status"], (perm["status"], base["status"])
    assert abs(int(perm["iters"]) - int(base["iters"])) <= 2, (perm["iters"], base["iters"])
    dj = abs(perm["cost"] - base["cost"]) / abs(base["cost"])
    assert dj <= cost_tol, dj
    # coefficients [S, 3, N]: the dimension axis is permuted
    want = np.moveaxis(permute_axes(np.moveaxis(np.asarray(base["coeffs"]), 1, -1)), -1, 1)
    dc = rel_coeffs(perm["coeffs"], want)
    assert dc <= 1e-6, dc
    return dj, dc


def check_tube_reversal(base, rev, rev_resid, cost_tol=1e-6, iter_slack=2):
    assert rev["status"] == base["status"], (rev["status"], base["status"])
    assert abs(int(rev["iters"]) - int(base["iters"])) <= iter_slack, (rev["iters"], base["iters"])
    dj = abs(rev["cost"] - base["cost"]) / abs(base["cost"])
    assert dj <= cost_tol, dj
    assert np.max(rev_resid) <= 1e-8, np.max(rev_resid)
    return dj, float(np.max(rev_resid))
