"""The linear-solve and time-cost kernels of the standard shape (N = 10, r = 4,
D = 3) against the exact rational minimiser (tests/golden/exact_std.json, made
by make_exact_std.py), not against the oracle.

The oracle is the reference algorithm in FP64; at the edge of the time
optimisers' box [0.1, 2 T0] its coefficients are wrong from the fourth digit
on, so parity with it says nothing there.  Each case of the fixture carries the
oracle's own error against the truth, and a kernel must be at least as
accurate: per row
  status      0 (no false NOT_SPD or BAD_TIME at the box edge);
  coefficients, d_p   rel_err_coeffs <= max(1e-9, 2 x the oracle's) (1e-9: the
              kernel-to-kernel bar of test_linear_lane_gpu.py);
  cost        rel_err <= max(1e-8, 2 x the oracle's) (1e-8: the bar of
              test_lane_kernels_match_wavefront_kernel for this cancelling form);
  backward error of the returned free values, |sum_j R_ij x_j| / sum_j |R_ij
              x_j| on the free rows with R(T) exact, evaluated in Fractions:
              <= 2 max(the oracle's, resid_floor).  It does not depend on the
              conditioning, so it discriminates where the coefficient bound
              is loose.
One batch per S holds every regime of that S, cycled to 24 rows (not a
multiple of the lane kernels' 21 trajectories per wave; neighbouring lanes hold
different regimes).  The table the tests print is profiles/exact_std_gpu.txt.

Worst measured on an MI355X over S and kernels, GPU / oracle:
  regime     coefficients        d_p                 cost                backward error
  nominal    3.7e-13 / 1.9e-10   1.8e-13 / 3.2e-10   2.1e-11 / 2.9e-11   7.5e-15 / 4.9e-11
  edge_even  2.4e-05 / 2.5e-03   3.9e-08 / 1.2e-07   7.7e-12 / 1.4e-11   9.1e-14 / 6.4e-10
  edge_odd   3.2e-05 / 4.4e-03   3.4e-06 / 1.4e-05   3.0e-09 / 4.6e-09   7.3e-13 / 8.2e-11
  all_min    1.5e-09 / 2.0e-05   3.7e-13 / 1.8e-08   9.5e-12 / 3.4e-12   7.5e-15 / 5.2e-10
  geometric  2.5e-12 / 8.7e-10   4.7e-13 / 4.5e-10   6.4e-12 / 1.3e-11   3.5e-15 / 1.8e-12
  fd_low     1.1e-06 / 1.9e-05   5.3e-08 / 6.4e-07   4.0e-10 / 3.6e-10   5.5e-15 / 4.1e-08
time_cost (S <= 7; gradients as a fraction of max |g_exact|):
  regime     J                   mode 1 gradient     mode 2 gradient
  nominal    7.4e-15 / 1.0e-14   2.4e-09 / 7.2e-09   8.9e-14 / 3.6e-13
  edge_even  7.7e-12 / 8.5e-12   1.5e-08 / 1.8e-07   1.4e-08 / 3.7e-08
  edge_odd   3.2e-12 / 5.5e-12   2.3e-06 / 1.9e-03   2.1e-08 / 8.0e-09
  all_min    9.5e-12 / 3.4e-12   0 / 0               0 / 0
  geometric  6.4e-12 / 1.3e-11   1.4e-11 / 1.7e-09   3.9e-09 / 1.7e-09
  fd_low     1.8e-11 / 1.3e-11   1.5e-11 / 2.5e-10   5.4e-09 / 1.9e-08
Every kernel returns status 0 on every row.  No bound is widened.

What these tests found: the generic kernel formed the cost as 0.5 e^T H e over
the vertex derivatives, which cancels by ten digits on a long segment next to
one at the lower time bound.  Its coefficients, d_p, backward error and mode-1
gradient were as good as the other kernels'; its cost was off, GPU / oracle:
  edge_odd   S3 2.1e-04 / 1.4e-09   S7 8.7e-05 / 4.1e-10   S11 9.6e-04 / 4.6e-09
             S17 1.5e-04 / 1.7e-09
  fd_low     S3 3.2e-07 / 2.9e-10   S4 2.0e-06 / 3.6e-10   S7 7.6e-07 / 2.4e-11
J by 4.1e-07 (bound 1e-9) and the mode-2 gradient by up to 4.6e-04 of max |g|
(bound 6.7e-08).  The generic linear-solve, coefficient and time kernels now
sum 0.5 c^T Q c from the coefficients as the reference and the other kernels
do (Traj::coeffs_and_cost, mtg_device.h); the figures above are with that.
The kernels of the soft-constraint objective, which these tests do not run,
still use the old form: DESIGN.md section 3.
"""
import functools
import os
import sys

import numpy as np
import pytest

from helpers import rel_err, rel_err_coeffs

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)

B = 24
LANE_MAX_S = 12


@functools.lru_cache(maxsize=None)
def _fixture():
    import make_exact_std as gen
    return gen.load_fixture()


def _s_values():
    return sorted({c["S"] for c in _fixture()["cases"]})


@functools.lru_cache(maxsize=None)
def _batch(S):
    """(mask, d_f [B, D, n_f], times [B, S], the case of each row): every
    regime of S, cycled to B rows.  Shared and read-only."""
    cases = [c for c in _fixture()["cases"] if c["S"] == S]
    rows = [cases[b % len(cases)] for b in range(B)]
    df = np.ascontiguousarray([c["df"] for c in rows], dtype=np.float64)
    t = np.ascontiguousarray([c["times"] for c in rows], dtype=np.float64)
    return np.array(rows[0]["mask"], np.uint8), df, t, rows


@functools.lru_cache(maxsize=None)
def _exact_R(S, regime):
    import make_exact_std as gen
    case = next(c for c in _fixture()["cases"] if (c["S"], c["regime"]) == (S, regime))
    return gen.exact_R(gen.N, gen.R_ORD, case["times"])[0]


def _kernels(S):
    return ["standard", "generic"] + (["lane", "lane_pair"] if S <= LANE_MAX_S else [])


def _linear_params():
    return [pytest.param(S, k, id=f"S{S}-{k}") for S in _s_values() for k in _kernels(S)]


@pytest.mark.parametrize("S,kernel", _linear_params())
def test_linear_vs_exact(ctx, dev, S, kernel):
    """plan.solve on every kernel that accepts the plan: status, coefficients,
    d_p, cost and backward error of every row against the fixture."""
    import make_exact_std as gen
    import mav_tube_trajectory_generation_amd as mtg
    fx = _fixture()
    mask, df, t, rows = _batch(S)
    plan = mtg.LinearPlan(ctx, gen.N, gen.D, gen.R_ORD, S, mask).set_kernel(kernel)
    assert plan.kernel == kernel
    assert plan.kernel_for_batch(B) == kernel
    out = plan.solve(torch.from_numpy(df).to(dev), torch.from_numpy(t).to(dev), free=True)
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in out.items()}
    fr = gen.free_indices(mask)
    worst, misses, resid_of = {}, [], {}
    for b, c in enumerate(rows):
        reg = c["regime"]
        if out["status"][b] != 0:
            misses.append((reg, b, "status", int(out["status"][b]), 0))
            continue
        key = (reg, out["free"][b].tobytes())  # rows of a regime usually agree bit for bit
        if key not in resid_of:
            resid_of[key] = gen.backward_error(_exact_R(S, reg), fr,
                                               gen.all_derivs(mask, df[b], out["free"][b]))
        got = dict(coeffs=rel_err_coeffs(out["coeffs"][b], np.array(c["coeffs"])),
                   dp=rel_err_coeffs(out["free"][b], np.array(c["dp"])),
                   cost=rel_err(out["cost"][b], c["cost"]),
                   resid=resid_of[key])
        bound = dict(coeffs=max(1e-9, 2.0 * c["oracle_err"]),
                     # d_p against its own oracle figure, never looser than the
                     # coefficients' bound
                     dp=max(1e-9, 2.0 * min(c["oracle_dp_err"], c["oracle_err"])),
                     cost=max(1e-8, 2.0 * c["oracle_cost_err"]),
                     resid=2.0 * max(c["oracle_resid"], fx["resid_floor"]))
        w = worst.setdefault(reg, dict.fromkeys(got, 0.0))
        for what, g in got.items():
            w[what] = max(w[what], g)
            if not g <= bound[what]:
                misses.append((reg, b, what, g, bound[what]))
    print()
    for c in {c["regime"]: c for c in rows}.values():
        w = worst.get(c["regime"])
        if w:
            print(f"linear S{S:<2d} {c['regime']:9s} {kernel:9s} gpu/oracle"
                  f" coeffs {w['coeffs']:.1e}/{c['oracle_err']:.1e}"
                  f" dp {w['dp']:.1e}/{c['oracle_dp_err']:.1e}"
                  f" cost {w['cost']:.1e}/{c['oracle_cost_err']:.1e}"
                  f" resid {w['resid']:.1e}/{c['oracle_resid']:.1e}")
    assert not misses, misses


def _time_params():
    import make_exact_std as gen
    return [pytest.param(S, k, id=f"S{S}-{k}") for S in _s_values() if S <= gen.TIME_COST_MAX_S
            for k in ("auto", "generic")]


@pytest.mark.parametrize("grad_mode", [0, 1, 2])
@pytest.mark.parametrize("S,kernel", _time_params())
def test_time_cost_vs_exact(ctx, dev, S, kernel, grad_mode):
    """plan.time_cost (AUTO: the standard-pattern wave kernel; and the generic
    kernel) against the exact J and the exact gradients.  J within e_J =
    max(1e-9, 2 x the oracle's), relative.  Gradient: max |g - g_exact| <=
    max(2 x the oracle's mode-2 error x max |g_exact|, 2 e_J |J| / (2 inc)),
    the second term being e_J carried through the difference of two J values;
    the same bound for mode 1, whose exact value holds d at the exact
    solution.  The fd_low rows (a lower central-difference point of 0.05,
    below the box) are among them: status 0 and a finite gradient."""
    import make_exact_std as gen
    import mav_tube_trajectory_generation_amd as mtg
    mask, df, t, rows = _batch(S)
    plan = mtg.LinearPlan(ctx, gen.N, gen.D, gen.R_ORD, S, mask).set_kernel(kernel)
    assert plan.kernel == ("standard" if kernel == "auto" else kernel)
    out = plan.time_cost(torch.from_numpy(df).to(dev), torch.from_numpy(t).to(dev),
                         time_penalty=gen.PENALTY, grad_mode=grad_mode, increment=gen.INC,
                         w_d=gen.W_D, w_t=gen.W_T)
    torch.cuda.synchronize()
    status = out["status"].cpu().numpy()
    J = out["cost"].cpu().numpy()
    grad = out["grad"].cpu().numpy() if grad_mode else None
    worst, misses = {}, []
    for b, c in enumerate(rows):
        reg = c["regime"]
        if status[b] != 0:
            misses.append((reg, b, "status", int(status[b]), 0))
            continue
        e_J = max(1e-9, 2.0 * c["oracle_J_err"])
        w = worst.setdefault(reg, dict(J=0.0, grad=0.0, gbound=0.0))
        g = rel_err(J[b], c["J"])
        w["J"] = max(w["J"], g)
        if not g <= e_J:
            misses.append((reg, b, "J", g, e_J))
        if grad_mode:
            ge = np.array(c["grad1" if grad_mode == 1 else "grad2"])
            gmax = float(np.max(np.abs(ge)))
            bound = max(2.0 * c["oracle_grad_err"] * gmax,
                        2.0 * e_J * abs(c["J"]) / (2.0 * gen.INC))
            if not np.isfinite(grad[b]).all():
                misses.append((reg, b, "grad not finite", grad[b].tolist(), bound))
                continue
            g = float(np.max(np.abs(grad[b] - ge)))
            w["grad"], w["gbound"] = max(w["grad"], g / max(gmax, 1e-300)), bound / max(gmax, 1e-300)
            if not g <= bound:
                misses.append((reg, b, "grad", g, bound))
    print()
    for c in {c["regime"]: c for c in rows}.values():
        w = worst.get(c["regime"])
        if w:
            og = c["oracle_grad1_err" if grad_mode == 1 else "oracle_grad_err"]
            print(f"time_cost S{S:<2d} {c['regime']:9s} {kernel:9s} mode {grad_mode} gpu/oracle"
                  f" J {w['J']:.1e}/{c['oracle_J_err']:.1e}"
                  + (f" grad {w['grad']:.1e}/{og:.1e} (bound {w['gbound']:.1e}, of max|g|)"
                     if grad_mode else ""))
    assert not misses, misses
