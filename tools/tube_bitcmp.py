"""Outputs of the six tube QCQP entry points of this build on small fixed
inputs, written to one .npz (run twice, with MTG_LIB_PATH pointing at two
builds, then compare): a bit-identity check for changes that must not alter
the arithmetic.

    python tools/tube_bitcmp.py out.npz            # write
    python tools/tube_bitcmp.py a.npz b.npz        # compare, array by array

Uniform (tube_solve, tube_time_cost with the central-difference gradient,
tube_time_optimize with LN_SBPLX): N = 10, r = 4, B = 64, S in 2, 3, 10, 16
(compile-time-S kernels) and 17 (run-time S); row 5 has a non-positive time.
Ragged (ragged_tube_solve with and without the dispatch order,
ragged_tube_time_cost, ragged_tube_time_optimize): counts cycling over
2, 3, 7, 5 at S_max = 8, B = 64; row 5 has a non-positive time, row 6 a count
of 1 and row 7 a count of S_max + 1.  The other orders (N = 4, 6, 8, 12) at
one shape each for the two solve entries.  The comparison prints, per array,
whether the bits agree, and for those that do not the rows that differ and
the largest relative difference.
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mav_tube_trajectory_generation_amd as mtg  # noqa: E402

B = 64
COUNTS = (2, 3, 7, 5)
S_MAX = 8
MAX_EVALS = 30


def uniform_inputs(N, S, dev, bad_row=True):
    M = N // 2
    _, _, times, pos = mtg.generate_random_problems(N, 3, S, B, seed0=105)
    fv = np.zeros((B, 3, N))
    fv[:, :, 0] = pos[:, 0, :]
    fv[:, :, M] = pos[:, S, :]
    times = times.copy()
    if bad_row:
        times[5, S // 2] = -1.0
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    return dict(positions=T(pos), fixed_vals=T(fv), times=T(times),
                radii=torch.full((B, S, 2), 0.15, dtype=torch.float64, device=dev))


def ragged_inputs(N, dev):
    """Padded rows (padding NaN) and their counts."""
    M = N // 2
    counts = np.array([COUNTS[b % len(COUNTS)] for b in range(B)], np.int32)
    pos = np.full((B, S_MAX + 1, 3), np.nan)
    fv = np.zeros((B, 3, N))
    times = np.full((B, S_MAX), np.nan)
    radii = np.full((B, S_MAX, 2), np.nan)
    for S in sorted(set(COUNTS)):
        _, _, t, p = mtg.generate_random_problems(N, 3, S, B, seed0=700)
        rows = np.nonzero(counts == S)[0]
        pos[rows, :S + 1] = p[rows]
        fv[rows, :, 0] = p[rows, 0, :]
        fv[rows, :, M] = p[rows, S, :]
        times[rows, :S] = t[rows]
        radii[rows, :S] = 0.15
    times[5, 0] = 0.0          # count 3: a non-positive time
    counts[6] = 1              # not a trajectory: too short
    counts[7] = S_MAX + 1      # not a trajectory: too long
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    return dict(seg_counts=T(counts), positions=T(pos), fixed_vals=T(fv), times=T(times),
                radii=T(radii))


def collect(dev):
    ctx = mtg.Context(0)
    res = {}

    def keep(tag, out):
        torch.cuda.synchronize()
        for k, v in out.items():
            if v is not None:
                res[f"{tag}/{k}"] = v.cpu().numpy()

    N, r = 10, 4
    for S in (2, 3, 10, 16, 17):
        u = uniform_inputs(N, S, dev)
        g = dict(positions=u["positions"], fixed_vals=u["fixed_vals"], radii=u["radii"])
        keep(f"tube_solve/S{S}", mtg.tube_solve(ctx, N, r, times_cp=u["times"].abs(),
                                                times=u["times"], **g))
        keep(f"tube_time_cost/S{S}", mtg.tube_time_cost(ctx, N, r, times_cp=u["times"].abs(),
                                                        times=u["times"], grad=True, **g))
        keep(f"tube_time_optimize/S{S}",
             mtg.tube_time_optimize(ctx, N, r, times=u["times"], max_evals=MAX_EVALS,
                                    optimizer="sbplx", **g))
    rg = ragged_inputs(N, dev)
    tcp = rg["times"].abs()
    for order in (True, False):
        keep(f"ragged_tube_solve/order{int(order)}",
             {k: v for k, v in mtg.ragged_tube_solve(ctx, N, r, times_cp=tcp, order=order,
                                                     **rg).items() if k != "order"})
    keep("ragged_tube_time_cost", mtg.ragged_tube_time_cost(ctx, N, r, times_cp=tcp, grad=True,
                                                            **rg))
    keep("ragged_tube_time_optimize",
         mtg.ragged_tube_time_optimize(ctx, N, r, max_evals=MAX_EVALS, **rg))
    for N, r, S in ((4, 1, 3), (6, 2, 5), (8, 3, 4), (12, 5, 6)):
        u = uniform_inputs(N, S, dev)
        keep(f"tube_solve/N{N}", mtg.tube_solve(ctx, N, r, times_cp=u["times"].abs(), **u))
        rg = ragged_inputs(N, dev)
        keep(f"ragged_tube_solve/N{N}",
             {k: v for k, v in mtg.ragged_tube_solve(ctx, N, r, times_cp=rg["times"].abs(),
                                                     **rg).items() if k != "order"})
    return res


def compare(pa, pb):
    a, b = np.load(pa), np.load(pb)
    assert sorted(a.files) == sorted(b.files), "the two files hold different arrays"
    differing = 0
    for k in sorted(a.files):
        x, y = a[k], b[k]
        if x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes():
            print(f"{k:44s} {str(x.shape):18s} identical bits")
            continue
        differing += 1
        xr, yr = x.reshape(x.shape[0], -1), y.reshape(y.shape[0], -1)
        rows = [i for i in range(x.shape[0]) if xr[i].tobytes() != yr[i].tobytes()]
        both = np.isfinite(xr) & np.isfinite(yr)
        rel = np.abs(xr - yr)[both] / np.maximum(np.abs(xr[both]), 1e-300)
        nanpos = bool((np.isnan(xr) == np.isnan(yr)).all())
        print(f"{k:44s} {str(x.shape):18s} DIFFERS in rows {rows}: max rel "
              f"{rel.max() if rel.size else 0.0:.3e}, NaN positions "
              f"{'agree' if nanpos else 'differ'}")
    print(f"{len(a.files)} arrays, {differing} differ")
    return differing


def main():
    if len(sys.argv) == 3:
        sys.exit(1 if compare(sys.argv[1], sys.argv[2]) else 0)
    np.savez(sys.argv[1], **collect(torch.device("cuda:0")))


if __name__ == "__main__":
    main()
