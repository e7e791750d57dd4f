"""Symmetries of the tube QCQP on the CPU oracle (no GPU needed).

The GPU tube kernels are compared with oracle/ only, and the oracle restates
the kernel's rules: whatever both share, parity cannot see.  A translated,
rotated or reversed tube problem is the same problem whatever the oracle
says, so these properties pin the oracle's half (test_invariance_gpu.py pins
the kernels') and tell later oracle edits what must not depend on the frame.

Before the solve was moved to coordinates relative to the midpoint of the
first and last vertex (setupTube) the translation cases failed: from
(1024, -2048, 512) on the solves ran to the iteration cap (status 1, 100
iterations) or stopped near-optimal, and at the UTM-like offset the cost was
off by percents.  Relative to the first vertex alone the reversal cases
failed: the reversed problem has another |q| and slack scale (seed 105,
S = 10: 26 iterations forwards, 22 backwards).

Measured on the oracle (worst over the eight problems): translation — status,
iterations, cost and non-constant coefficients equal bit for bit, constant
coefficients within 4.65e-10 (half an ulp of 4194304), residuals at a shifted
x equal; axis permutation — cost 1.7e-11, iterations equal; reversal — cost
1.5e-11, iterations equal.

The oracle is held to its own measured behaviour, tighter than the 1e-6
parity bar and +-2 iterations the kernels are held to in
test_invariance_gpu.py: cost within 5e-11 under the permutation, within 2e-11
and equal iteration counts under reversal.  The oracle's build is
deterministic (fixed flags, no FMA contraction), so these hold from machine
to machine, but the reversal bound sits close to the measured 1.5e-11: an
edit that reorders the oracle's arithmetic can trip it without being wrong.
Then re-measure; anything within the parity bar that keeps status and
iterations is rounding, anything larger is a frame dependence.
"""
import numpy as np
import pytest

import invariance_cases as ic

PROBLEMS = None


def _problems(oracle):
    """Every problem with its unshifted solve, computed once."""
    global PROBLEMS
    if PROBLEMS is None:
        PROBLEMS = {}
        for name, N, r, v, t0 in ic.tube_problems(oracle):
            radii = np.full((v.S, 2), ic.TUBE_RADIUS)
            PROBLEMS[name] = (N, r, v, t0, radii, _solve(oracle, N, r, v, t0, radii))
    return PROBLEMS


def _solve(oracle, N, r, v, t, radii):
    return oracle.tube_solve(N, r, v, t, radii, tol=ic.TUBE_TOL, max_iter=ic.TUBE_MAX_ITER)


NAMES = ["main_cpp"] + [f"N{N}_S{S}_seed{seed}" for N, _, S, seed in ic.TUBE_RANDOM]


@pytest.mark.parametrize("name", NAMES)
def test_tube_translation(oracle, name):
    N, r, v, t0, radii, base = _problems(oracle)[name]
    assert base["status"] == 0
    rng = np.random.default_rng(5)
    # any x near the solution, on the 2^-20 grid so that x + offset is exact
    x_any = ic.quantise(base["x"] + rng.normal(scale=0.05, size=base["x"].shape))
    g0 = oracle.tube_residuals(N, r, v, t0, radii, x_any)
    for off in ic.OFFSETS:
        vm = ic.translate(oracle, v, off)
        moved = _solve(oracle, N, r, vm, t0, radii)
        dev = ic.check_tube_translation(base, moved, off)
        print(name, off, "status", moved["status"], "iters", moved["iters"],
              "dcost %.2e dcoeff %.2e dc0 %.2e" % dev)
        g = oracle.tube_residuals(N, r, vm, t0, radii, ic.x_translate(x_any, off, N, v.S))
        dg = np.max(np.abs(g - g0) / np.maximum(1.0, np.abs(g0)))
        print("    residuals %.2e" % dg)
        assert dg <= 1e-10, dg


@pytest.mark.parametrize("name", [n for n in NAMES if n != "N10_S16_seed412"])
def test_tube_time_cost_translation(oracle, name):
    """J = QCQP cost at times 1.1 T0 with the control-point maps at T0, and
    its central-difference gradient, within 1e-12 (absolute) of the unshifted
    ones; no time penalty, which would mask the cost.  (The oracle has the
    plain and the finite-difference mode.)  S = 16 is left to the GPU file:
    here the objective is a loop of 2S + 1 separate solves per offset (6.5 s
    at S = 16) through the same setupTube that test_tube_translation covers
    at S = 16; the oracle has no shared-geometry path of its own."""
    N, r, v, t0, radii, _ = _problems(oracle)[name]
    kw = dict(times_cp=t0, time_penalty=0.0, tol=ic.TUBE_TOL, max_iter=ic.TUBE_MAX_ITER)
    J0, g0 = oracle.tube_time_cost(N, r, v, 1.1 * t0, radii, grad_mode=2, **kw)
    assert np.isfinite(J0) and np.all(np.isfinite(g0))
    for off in ic.OFFSETS:
        vm = ic.translate(oracle, v, off)
        for mode in (0, 2):
            J, g = oracle.tube_time_cost(N, r, vm, 1.1 * t0, radii, grad_mode=mode, **kw)
            assert abs(J - J0) <= 1e-12, (off, mode, J, J0)
            if mode == 2:
                assert np.max(np.abs(g - g0)) <= 1e-12, (off, g, g0)


@pytest.mark.parametrize("name", NAMES)
def test_tube_axis_permutation(oracle, name):
    N, r, v, t0, radii, base = _problems(oracle)[name]
    perm = _solve(oracle, N, r, ic.permute_vertices(oracle, v), t0, radii)
    dj, dc = ic.check_tube_permutation(base, perm, cost_tol=5e-11)
    print(name, "iters", base["iters"], perm["iters"], "dcost %.2e dcoeff %.2e" % (dj, dc))


@pytest.mark.parametrize("name", NAMES)
def test_tube_reversal(oracle, name):
    N, r, v, t0, radii, base = _problems(oracle)[name]
    vr, tr = ic.reverse_vertices(oracle, v), t0[::-1].copy()
    rev = _solve(oracle, N, r, vr, tr, radii)
    resid = oracle.tube_residuals(N, r, vr, tr, radii, rev["x"])
    dj, gmax = ic.check_tube_reversal(base, rev, resid, cost_tol=2e-11, iter_slack=0)
    print(name, "iters", base["iters"], rev["iters"], "dcost %.2e max g %.2e" % (dj, gmax))


def test_tube_offset_1e3_same_status_and_objective(oracle):
    """The same tube problem offset by about 1e3 gives the same status and
    objective (finding 2)."""
    N, r, v, t0, radii, base = _problems(oracle)["N10_S10_seed105"]
    moved = _solve(oracle, N, r, ic.translate(oracle, v, (1000.0, -1000.0, 1000.0)), t0, radii)
    assert moved["status"] == base["status"] == 0
    assert abs(moved["cost"] - base["cost"]) <= 1e-12 * abs(base["cost"])
