"""The extremum searches inside the time-allocation kernels (the soft
objective of mtg_time_cost: ExtSoft / ext_soft_maxima_wave on the standard
pattern, ext_trajectory_max_wave in the generic kernel), one maximum at a
time.

The maxima are not an output, but the objective reveals them.  With
time_penalty = 0 and grad_mode = 0, J is evaluated twice with the same
constraint list (same kernel instantiation, same part count P): every
constraint but the probed one, c, has limit 1e30 in both runs (its term is
e^-100); c has limit a in the first run and 1e30 in the second.  Then

    J_a - J_inf = exp(w (m_c - a) / a) - e^-100,  m_c = a (1 + ln(J_a - J_inf) / w),

with a the reference maximum, so the difference is about 1.  With w = 100 the
cancellation noise on m_c / a is about 2^-53 J / w; J < 1e4 w is asserted
first, which keeps it below 1e-12.

Reference for m_c: the coefficients plan.solve returns for the same fixed
values and times (segment times >= 0.5 s, where DESIGN.md §3 measures the
time kernels' own coefficients as agreeing to 3.7e-13), |p^(K)|^2 evaluated
in numpy.longdouble at 0, T, at the real parts of all complex roots of f
that fall in [0, T] (no imaginary-part filter) and at the local maxima of a
257-point grid, each polished by Newton steps on f in longdouble.  Every one
of these is a value g takes on the segment, so the reference never exceeds
the true maximum, and it falls short only by the square of a polished root's
error.  The assertion is |m_dev - m_ref| <= 1e-9 m_ref, the suite's parity
level for J and for the argmax value; a missed interior maximum shows orders
of magnitude above that.
"""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

N, D, R = 10, 3, 4
W = 100.0
BIG = 1.0e30
LD = np.longdouble


def _horner(a, t):
    v = np.zeros_like(t) + a[-1]
    for x in a[-2::-1]:
        v = v * t + x
    return v


def _der(a):
    return a[1:] * np.arange(1, len(a), dtype=LD) if len(a) > 1 else np.zeros(1, LD)


def _segment_max2(c, T, K):
    """max over [0, T] of |p^(K)|^2 for coefficients c [D, N] (longdouble)."""
    fall = np.array([math.prod(range(i - K + 1, i + 1)) for i in range(K, c.shape[1])], LD)
    a = [c[d, K:].astype(LD) * fall for d in range(c.shape[0])]
    a1 = [_der(x) for x in a]
    a2 = [_der(x) for x in a1]

    def g(t):
        return sum(_horner(x, t) ** 2 for x in a)

    def f(t):
        return sum(_horner(x, t) * _horner(y, t) for x, y in zip(a, a1))

    def fp(t):
        return sum(_horner(y, t) ** 2 + _horner(x, t) * _horner(z, t)
                   for x, y, z in zip(a, a1, a2))

    fc = np.zeros(2 * len(a[0]) - 2)
    for x, y in zip(a, a1):
        fc[:len(x) + len(y) - 1] += np.convolve(x.astype(float), y.astype(float))
    fc = np.trim_zeros(fc, "b")
    cand = [0.0, T]
    if fc.size > 1:
        z = np.roots(fc[::-1])
        cand += [float(x) for x in z.real if 0.0 <= x <= T]
    grid = np.linspace(0.0, T, 257)
    gg = g(grid.astype(LD))
    cand += [float(grid[i]) for i in range(1, 256) if gg[i] >= gg[i - 1] and gg[i] >= gg[i + 1]]
    t = np.array(cand, LD)
    pts = [t]
    for _ in range(12):
        d = fp(t)
        step = np.where(d != 0, f(t) / np.where(d != 0, d, 1), 0)
        t = np.clip(t - step, LD(0), LD(T))
        pts.append(t)
    return max(np.max(g(p)) for p in pts)


def _trajectory_max(coeffs, times, K):
    """max |p^(K)| over a trajectory, coeffs [S, D, N]."""
    best = LD(0)
    for s in range(coeffs.shape[0]):
        best = max(best, _segment_max2(coeffs[s], float(times[s]), K))
    return float(np.sqrt(best))


def _recover_maxima(plan, fd, td, ders, dev):
    """(device maxima [B, nc], reference maxima [B, nc]) for the constraint
    list ders, probed one constraint at a time."""
    B = td.shape[0]
    coeffs = plan.solve(fd, td)["coeffs"].cpu().numpy()
    times = td.cpu().numpy()
    nc = len(ders)
    ref = np.array([[_trajectory_max(coeffs[b], times[b], K) for K in ders] for b in range(B)])
    j_inf = plan.time_cost(fd, td, time_penalty=0.0, grad_mode=0, soft=[(K, BIG) for K in ders],
                           soft_weight=W)
    assert (j_inf["status"].cpu().numpy() == 0).all()
    j_inf = j_inf["cost"].cpu().numpy()
    assert np.all(j_inf < 1.0e4 * W), j_inf  # cancellation noise below 1e-12
    got = np.zeros((B, nc))
    for c in range(nc):
        for b in range(B):  # the limit is per launch: one row at a time
            soft = [(K, ref[b, c] if i == c else BIG) for i, K in enumerate(ders)]
            j_a = plan.time_cost(fd[b:b + 1], td[b:b + 1], time_penalty=0.0, grad_mode=0,
                                 soft=soft, soft_weight=W)["cost"].cpu().numpy()[0]
            dj = j_a - j_inf[b]
            assert dj > 0.0, (b, c, j_a, j_inf[b])
            got[b, c] = ref[b, c] * (1.0 + math.log(dj) / W)
    return got, ref


SHAPES = [
    (2, [1]),                        # P = 8 (clamped), KMIN = 1
    (2, [0]), (2, [3]), (2, [4]),    # KMIN = 0, 3, 4
    (3, [2, 1, 0]),                  # P = 7, unsorted, padding from KMIN = 0
    (5, [1, 2]),                     # P = 6
    (7, [1, 2, 3]),                  # P = 3
    (11, [0, 4]),                    # P = 2, widest padding
    (16, [1, 2]),                    # P = 2
    (16, [1, 2, 3, 4]),              # P = 1, exactly 64 items
    (16, [0, 1, 2, 3, 4]),           # 80 items: second round, partial
    (16, [0, 1, 2, 3, 4, 1, 2, 3]),  # 128 items: two full rounds, duplicates
    (17, [1, 2]),                    # runtime-S time_cost_std_kernel, P = 1
    (24, [1, 2, 3]),                 # runtime-S, 72 items: second round
]


@pytest.mark.parametrize("kernel", ["auto", "generic"])
@pytest.mark.parametrize("S,ders", SHAPES, ids=lambda x: "".join(map(str, x)) if isinstance(x, list) else f"S{x}")
def test_soft_maxima_random(ctx, dev, S, ders, kernel):
    import mav_tube_trajectory_generation_amd as mtg
    B = 4
    mask, fixed, times, _ = mtg.generate_random_problems(N, D, S, B, seed0=3100 + S)
    times = np.maximum(times, 0.5)
    plan = mtg.LinearPlan(ctx, N, D, R, S, mask).set_kernel(kernel)
    fd, td = torch.from_numpy(fixed).to(dev), torch.from_numpy(times).to(dev)
    got, ref = _recover_maxima(plan, fd, td, ders, dev)
    err = np.abs(got - ref) / ref
    print(f"soft_maxima S{S} {ders} {kernel}: max relative error {err.max():.2e}")
    assert np.all(err <= 1e-9), (S, ders, kernel, err)


def _line_problem(S, mirror):
    """Rest-to-rest straight line along x with equal segment times: the
    fixed values in (vertex, derivative) order, start and end with all
    N / 2 derivatives fixed (zero), positions in between."""
    M = N // 2
    x = 10.0 * np.arange(S + 1) / S
    if mirror:
        x = x[-1] - x
    fixed = np.zeros((1, D, 2 * M + S - 1))
    fixed[0, 0, 0] = x[0]
    fixed[0, 0, M:M + S - 1] = x[1:S]
    fixed[0, 0, M + S - 1] = x[S]
    return fixed, np.full((1, S), 1.25)


@pytest.mark.parametrize("kernel", ["auto", "generic"])
@pytest.mark.parametrize("S", [5, 8])
def test_soft_maxima_straight_line(ctx, dev, S, kernel):
    """Two dimensions identically zero, high-multiplicity roots of f at both
    ends, the velocity maximum by symmetry at the middle of the path: on a
    part boundary for even P, on a vertex for even S.  The mirror image's
    maxima equal the original's to 1e-12 relative."""
    import mav_tube_trajectory_generation_amd as mtg
    mask = mtg.generate_random_problems(N, D, S, 1, seed0=1)[0]
    plan = mtg.LinearPlan(ctx, N, D, R, S, mask).set_kernel(kernel)
    res = []
    for mirror in (False, True):
        fixed, times = _line_problem(S, mirror)
        fd, td = torch.from_numpy(fixed).to(dev), torch.from_numpy(times).to(dev)
        got, ref = _recover_maxima(plan, fd, td, [1, 2], dev)
        err = np.abs(got - ref) / ref
        print(f"soft_maxima line S{S} mirror={int(mirror)} {kernel}: max relative error "
              f"{err.max():.2e}")
        assert np.all(err <= 1e-9), (S, mirror, kernel, err)
        res.append(got)
    assert np.all(np.abs(res[0] - res[1]) <= 1e-12 * res[0]), (res[0], res[1])
