"""Exact symmetries of the tube QCQP and of the linear minimum-derivative
solve on the GPU kernels.

Every other GPU test of these kernels compares with oracle/, our own
restatement, which shares the kernels' rules; what both share, parity cannot
see.  A translated, rotated, reversed or time-scaled problem is the same
problem whatever the oracle computes, so these properties hold on their own
(test_invariance_oracle.py runs the tube ones on the oracle).

Tube part: before the solve was moved to coordinates relative to the
midpoint of the first and last vertex (tube_origin(), mtg_tube_device.h) the
translation cases failed: the kernel built |b|^2 - r1^2, q, the cold start's
slack scale and the stopping test in world coordinates, and on an MI355X
every one of the eight problems stopped at the iteration cap (status 3, 100
iterations) at the offsets (1024, -2048, 512), (16384, 16384, 16384) and
(524288, 4194304, 256), with the cost off by up to 4.1 % at the last.  Now
status, iterations, cost, non-constant coefficients and residuals are equal
bit for bit at all four offsets; the axis permutation moves the cost by at
most 4.6e-13 and the reversal by 1.1e-13, both with equal iteration counts
(oracle: 1.7e-11 and 1.5e-11).

Linear part: the bound of a case is max(1e-9, 100 x the oracle's own deviation
under the same transformation of the same input): 1e-9 is the project's bar
for two elimination orders of one algorithm, the factor 100 allows for the
kernels' different summation order.  Measured worst deviations are listed in
test_linear_symmetries' docstring.
"""
import numpy as np
import pytest

import invariance_cases as ic
from helpers import compact_fixed, standard_vertices

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


def _T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# ------------------------------------------------------------------- tube

def _tube_arrays(variants, N):
    M = N // 2
    pos = np.stack([v.vals[:, 0, :] for v, _, _ in variants])
    fv = np.zeros((len(variants), 3, N))
    for b, (v, _, _) in enumerate(variants):
        fv[b, :, :M] = v.vals[0, :M, :].T
        fv[b, :, M:] = v.vals[v.S, :M, :].T
    times = np.stack([t for _, t, _ in variants])
    tcp = np.stack([c for _, _, c in variants])
    return pos, fv, tcp, times


_TUBE = {}
ADVICE_OFFSET = (1000.0, -1000.0, 1000.0)
NAMES = ["main_cpp"] + [f"N{N}_S{S}_seed{seed}" for N, _, S, seed in ic.TUBE_RANDOM]


def _tube(ctx, dev, oracle, name):
    """The problem `name` and all its transformed copies in one launch:
    {key: result}, keys "base", ("off", i), "1e3", "perm", "rev"; plus
    "resid_any": residuals of base and the four offsets at one arbitrary x
    (shifted with the problem).  Computed once per problem."""
    import mav_tube_trajectory_generation_amd as mtg
    if name in _TUBE:
        return _TUBE[name]
    _, N, r, v, t0 = next(p for p in ic.tube_problems(oracle) if p[0] == name)
    S = v.S
    keys = ["base"] + [("off", i) for i in range(len(ic.OFFSETS))] + ["1e3", "perm", "rev"]
    variants = [(v, t0, t0)] + [(ic.translate(oracle, v, off), t0, t0) for off in ic.OFFSETS]
    variants.append((ic.translate(oracle, v, ADVICE_OFFSET), t0, t0))
    variants.append((ic.permute_vertices(oracle, v), t0, t0))
    variants.append((ic.reverse_vertices(oracle, v), t0[::-1].copy(), t0[::-1].copy()))
    pos, fv, tcp, times = _tube_arrays(variants, N)
    radii = np.full((len(variants), S, 2), ic.TUBE_RADIUS)
    args = [_T(a, dev) for a in (pos, fv, tcp, times, radii)]
    out = mtg.tube_solve(ctx, N, r, *args, tol=ic.TUBE_TOL, max_iter=ic.TUBE_MAX_ITER)
    resid = mtg.tube_residuals(ctx, N, r, *args, out["x"]).cpu().numpy()
    o = {k: a.cpu().numpy() for k, a in out.items()}
    res = {}
    for b, key in enumerate(keys):
        res[key] = dict(status=int(o["status"][b]), iters=int(o["iters"][b]),
                        cost=float(o["cost"][b]), coeffs=o["coeffs"][b], x=o["x"][b],
                        resid=resid[b])
    # any x near the solution, on the 2^-20 grid so that x + offset is exact
    rng = np.random.default_rng(5)
    x_any = ic.quantise(o["x"][0] + rng.normal(scale=0.05, size=o["x"][0].shape))
    xs = np.stack([x_any] + [ic.x_translate(x_any, off, N, S) for off in ic.OFFSETS])
    n5 = 1 + len(ic.OFFSETS)
    res["resid_any"] = mtg.tube_residuals(ctx, N, r, *[a[:n5].contiguous() for a in args],
                                          _T(xs, dev)).cpu().numpy()
    res["v"] = v
    _TUBE[name] = res
    return res


@pytest.mark.parametrize("name", NAMES)
def test_tube_translation(ctx, dev, oracle, name):
    """Status and iteration count equal the unshifted solve's, cost and
    non-constant coefficients within 1e-12 (bit-equal in fact), constant
    coefficients within one ulp of the largest offset, residuals at a shifted
    x within the assembly bar 1e-10 max(1, |g|)."""
    res = _tube(ctx, dev, oracle, name)
    base = res["base"]
    assert base["status"] == 0, base["status"]
    g0 = res["resid_any"][0]
    for i, off in enumerate(ic.OFFSETS):
        moved = res[("off", i)]
        print(name, off, "status", moved["status"], "iters", moved["iters"], "base",
              base["status"], base["iters"])
        dev_ = ic.check_tube_translation(base, moved, off)
        dg = float(np.max(np.abs(res["resid_any"][1 + i] - g0) / np.maximum(1.0, np.abs(g0))))
        print("    dcost %.2e dcoeff %.2e dc0 %.2e" % dev_, "residuals %.2e" % dg)
        assert dg <= 1e-10, dg


def test_tube_offset_1e3_same_status_and_objective(ctx, dev, oracle):
    """The same tube problem offset by about 1e3 gives the same status and
    objective (finding 2)."""
    res = _tube(ctx, dev, oracle, "N10_S10_seed105")
    base, moved = res["base"], res["1e3"]
    assert moved["status"] == base["status"] == 0
    assert abs(moved["cost"] - base["cost"]) <= 1e-12 * abs(base["cost"])


@pytest.mark.parametrize("name", NAMES)
def test_tube_axis_permutation(ctx, dev, oracle, name):
    """(x, y, z) -> (z, -x, y): equal status, iterations within +-2, cost and
    permuted coefficients within the 1e-6 tube parity bar."""
    res = _tube(ctx, dev, oracle, name)
    dj, dc = ic.check_tube_permutation(res["base"], res["perm"])
    print(name, "iters", res["base"]["iters"], res["perm"]["iters"],
          "dcost %.2e dcoeff %.2e" % (dj, dc))


@pytest.mark.parametrize("name", NAMES)
def test_tube_reversal(ctx, dev, oracle, name):
    """Vertices and times reversed, odd end derivatives negated, uniform
    radii: equal status, iterations within +-2, cost within 1e-6, the
    reversed solution feasible to 1e-8."""
    res = _tube(ctx, dev, oracle, name)
    dj, gmax = ic.check_tube_reversal(res["base"], res["rev"], res["rev"]["resid"])
    print(name, "iters", res["base"]["iters"], res["rev"]["iters"],
          "dcost %.2e max g %.2e" % (dj, gmax))


@pytest.mark.parametrize("name", NAMES)
def test_tube_time_cost_translation(ctx, dev, oracle, name):
    """mtg_tube_time_cost at times 1.1 T0 with the control-point maps at T0
    and no time penalty (it would mask the cost), at the four offsets in one
    launch: J and the central-difference gradient within 1e-12 (absolute) of
    the unshifted ones.  Every problem, so that every lane layout and
    compile-time-S kernel goes through the shared-geometry path (2S + 1
    evaluation points per trajectory, bin = b / rep).  The QCQP objective has
    gradient modes 0 and 2 only (the ABI answers mode 1 with
    MTG_ERR_UNSUPPORTED); the optimisers' end points are not compared under
    translation: Subplex compares values and may branch."""
    import mav_tube_trajectory_generation_amd as mtg
    _, N, r, v, t0 = next(p for p in ic.tube_problems(oracle) if p[0] == name)
    S = v.S
    variants = [(v, 1.1 * t0, t0)] + [(ic.translate(oracle, v, off), 1.1 * t0, t0)
                                      for off in ic.OFFSETS]
    pos, fv, tcp, times = _tube_arrays(variants, N)
    radii = np.full((len(variants), S, 2), ic.TUBE_RADIUS)
    a = [_T(x, dev) for x in (pos, fv, tcp, times, radii)]
    plain = mtg.tube_time_cost(ctx, N, r, *a, time_penalty=0.0, grad=False, tol=ic.TUBE_TOL,
                               max_iter=ic.TUBE_MAX_ITER)
    fd = mtg.tube_time_cost(ctx, N, r, *a, time_penalty=0.0, grad=True, tol=ic.TUBE_TOL,
                            max_iter=ic.TUBE_MAX_ITER)
    for out in (plain, fd):
        J = out["cost"].cpu().numpy()
        st = out["status"].cpu().numpy()
        assert np.all(np.isfinite(J)) and np.all(st == st[0]) and st[0] == 0, (J, st)
        dj = np.max(np.abs(J[1:] - J[0]))
        print(name, "J", J[0], "dJ %.2e" % dj)
        assert dj <= 1e-12, (J, dj)
    g = fd["grad"].cpu().numpy()
    assert np.all(np.isfinite(g))
    dg = np.max(np.abs(g[1:] - g[0]))
    print(name, "dgrad %.2e" % dg)
    assert dg <= 1e-12, (g, dg)


# ----------------------------------------------------------------- linear

LINEAR_CASES = [
    (10, 4, 2, ("standard", "generic", "lane", "lane_pair")),
    (10, 4, 3, ("standard", "generic", "lane", "lane_pair")),
    (10, 4, 5, ("standard", "generic", "lane", "lane_pair")),
    (10, 4, 10, ("standard", "generic", "lane", "lane_pair")),
    (10, 4, 17, ("standard", "generic")),   # the wave kernel's runtime-S path
    (6, 2, 5, ("standard", "generic")),
    (12, 5, 5, ("standard", "generic")),
]
LIN_B, LIN_D = 24, 3   # 24 is not a multiple of the lane kernel's 21 per wave
LIN_OFFSETS = (1024.0, 131072.0)


def _linear_problems(N, S):
    """B problems on the standard pattern with random non-zero end
    derivatives (all-zero ones make reversal and scaling trivial), positions
    on the 2^-20 grid."""
    import pyoracle
    M = N // 2
    rng = np.random.default_rng(9100 + 10 * N + S)
    out = []
    for b in range(LIN_B):
        v = standard_vertices(N, S, LIN_D, 8000 + 31 * S + b)
        v.vals[:, 0, :] = ic.quantise(v.vals[:, 0, :])
        v.vals[0, 1:M, :] = rng.uniform(-2.0, 2.0, (M - 1, LIN_D))
        v.vals[S, 1:M, :] = rng.uniform(-2.0, 2.0, (M - 1, LIN_D))
        out.append((v, pyoracle.estimate_segment_times(v, 3.0, 5.0)))
    return out


def _time_scaled(oracle, v, t):
    vals = v.vals.copy()
    vals /= (2.0 ** np.arange(vals.shape[1]))[None, :, None]
    return oracle.Vertices(v.mask, vals), 2.0 * t


def _transformed(oracle, v, t):
    out = {"base": (v, t)}
    for off in LIN_OFFSETS:
        out[("off", off)] = (ic.translate(oracle, v, np.full(LIN_D, off)), t)
    out["rev"] = (ic.reverse_vertices(oracle, v), t[::-1].copy())
    out["scale"] = _time_scaled(oracle, v, t)
    out["perm"] = (ic.permute_vertices(oracle, v), t)
    return out


def _norm_dev(got, want):
    """max over (trajectory, segment, dimension) of ||got - want|| / ||want||."""
    num = np.linalg.norm(got - want, axis=-1)
    return float(np.max(num / np.maximum(np.linalg.norm(want, axis=-1), 1e-300)))


def _deviations(sol, times, N, r):
    """Deviation of each transformed solve from what the base solve implies.
    sol[key] = (coeffs [B, S, D, N], cost [B]); times [B, S]."""
    c0, J0 = sol["base"]
    dev = {}
    for off in LIN_OFFSETS:
        c, J = sol[("off", off)]
        dev[("off", off)] = (float(np.max(np.abs(J - J0) / J0)),
                             _norm_dev(c[..., 1:], c0[..., 1:]))
    # reversal: the reversed minimiser is p(T - t), so derivative k < 5 at the
    # start of reversed segment S-1-s is (-1)^k times the one at the end of
    # segment s (for every N: beyond the N/2 continuous ones too), and
    # likewise its end and the original start.
    c, J = sol["rev"]
    K = 5
    sign = (-1.0) ** np.arange(K)
    t = times[:, :, None]
    end0 = ic.poly_derivatives(c0, t, K)                   # [B, S, D, K]
    start0 = ic.poly_derivatives(c0, 0.0 * t, K)
    startr = ic.poly_derivatives(c, 0.0 * t, K)[:, ::-1]
    endr = ic.poly_derivatives(c, t[:, ::-1], K)[:, ::-1]
    dd = max(np.max(np.abs(startr - sign * end0) / np.maximum(1.0, np.abs(end0))),
             np.max(np.abs(endr - sign * start0) / np.maximum(1.0, np.abs(start0))))
    dev["rev"] = (float(np.max(np.abs(J - J0) / J0)), float(dd))
    # T -> 2 T, d_k -> d_k / 2^k: c_k -> c_k / 2^k, cost -> cost 2^(1 - 2 r)
    c, J = sol["scale"]
    dev["scale"] = (float(np.max(np.abs(J * 2.0 ** (2 * r - 1) - J0) / J0)),
                    _norm_dev(c * 2.0 ** np.arange(N), c0))
    return dev


_ORACLE_LIN = {}


def _oracle_linear(oracle, N, r, S):
    if (N, r, S) not in _ORACLE_LIN:
        probs = _linear_problems(N, S)
        sol = {}
        for key in _transformed(oracle, *probs[0]):
            cs, Js = [], []
            for v, t in probs:
                vt, tt = _transformed(oracle, v, t)[key]
                ref = oracle.linear_solve(N, r, vt, tt)
                cs.append(ref["coeffs"])
                Js.append(ref["cost"])
            sol[key] = (np.array(cs), np.array(Js))
        times = np.array([t for _, t in probs])
        _ORACLE_LIN[(N, r, S)] = (probs, times, _deviations(sol, times, N, r))
    return _ORACLE_LIN[(N, r, S)]


@pytest.mark.parametrize("N,r,S,kernels", LINEAR_CASES,
                         ids=[f"N{c[0]}_r{c[1]}_S{c[2]}" for c in LINEAR_CASES])
def test_linear_symmetries(ctx, dev, oracle, N, r, S, kernels):
    """Translation by 1024 and 131072 per axis (cost unchanged, coefficients
    unchanged apart from c0), reversal (cost unchanged, derivatives mirrored),
    time scaling x2 (c_k / 2^k, cost 2^(1-2r)) and the signed axis permutation
    (z, -x, y) on every kernel that accepts the case, B = 24.

    Bound per case and transformation: max(1e-9, 100 x ref), ref the oracle's
    own deviation on the same inputs (computed here).  The permutation is
    exact: dimensions are independent solves in every kernel, so per-dimension
    coefficients are bit-equal; the cost sums the dimensions in another order
    and is held to 1e-12.

    Worst measured on an MI355X, GPU over all kernels / oracle (cost;
    coefficients), N = 10 cases:
      translation 1024     6.8e-10 / 1.3e-10;  1.5e-9 / 2.0e-9
      translation 131072   3.8e-8 / 6.7e-8;    3.3e-7 / 2.5e-7
      reversal             2.0e-11 / 6.4e-11;  1.3e-10 / 1.1e-9 (derivatives)
      time scaling         0 / 2.9e-11;        0 / 5.6e-10 (bit-exact on the GPU)
      permutation          coefficients bit-equal, cost 3.2e-16
    N = 6: at most 4.0e-11 / 1.2e-10 (translation 131072), mirrored
    derivatives k < 5 under reversal 1.4e-13 / 3.0e-13; N = 12, r = 5:
    at most 2.4e-7 / 1.6e-7 (cost) and 3.7e-6 / 1.9e-6 (coefficients) under
    translation 131072, 2.9e-10 / 1.9e-7 under reversal.
    """
    import mav_tube_trajectory_generation_amd as mtg
    probs, times, ref = _oracle_linear(oracle, N, r, S)
    keys = list(_transformed(oracle, *probs[0]))
    for kernel in kernels:
        sol = {}
        for key in keys:
            dfs, ts = [], []
            mask = None
            for v, t in probs:
                vt, tt = _transformed(oracle, v, t)[key]
                mask, df = compact_fixed(vt, N)
                dfs.append(df)
                ts.append(tt)
            plan = mtg.LinearPlan(ctx, N, LIN_D, r, S, mask).set_kernel(kernel)
            assert plan.kernel == kernel
            out = plan.solve(_T(np.array(dfs), dev), _T(np.array(ts), dev))
            assert (out["status"].cpu().numpy() == 0).all(), (kernel, key)
            sol[key] = (out["coeffs"].cpu().numpy(), out["cost"].cpu().numpy())
        got = _deviations(sol, times, N, r)
        for key in got:
            for what, g, o in zip(("cost", "coeffs"), got[key], ref[key]):
                bound = max(1e-9, 100.0 * o)
                print(f"N{N} r{r} S{S} {kernel:9s} {str(key):18s} {what:6s} "
                      f"gpu {g:.2e} oracle {o:.2e} bound {bound:.2e}")
                assert g <= bound, (kernel, key, what, g, o)
        c0, J0 = sol["base"]
        c, J = sol["perm"]
        assert np.array_equal(c, np.moveaxis(ic.permute_axes(np.moveaxis(c0, 2, -1)), -1, 2)), kernel
        dj = float(np.max(np.abs(J - J0) / J0))
        print(f"N{N} r{r} S{S} {kernel:9s} perm cost {dj:.2e}")
        assert dj <= 1e-12, (kernel, dj)
