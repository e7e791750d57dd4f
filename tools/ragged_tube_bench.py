#!/usr/bin/env python3
"""The ragged tube QCQP solve against the per-S route, on the GPU.

    python tools/ragged_tube_bench.py [--batches 256,1024,4096] [--reps 5] [--rounds 5]

Workload: tools/ragged_bench.py's mixed-count batch (N = 10, r = 4, S_b
uniform over 2..12, S_max = 12, createRandomVertices(seed 105 + b) with
estimateSegmentTimes) as tube problems: the vertices' positions as the tube
geometry, radii 0.15, times_cp = times, tol 1e-10, at most 100 iterations.
Timed as ragged_bench.py times (device events around `reps` back-to-back
calls, eagerly and replayed from a HIP graph, the routes alternating for
`rounds` rounds, medians and min..max), per batch size:

  ragged_ordered  one mtg_ragged_tube_solve with order_ws (the order kernel,
                  then the solve dispatched longest rows first)
  ragged          the same call without order_ws
  per_s           what a caller has without the call: per S gather the group's
                  rows out of the padded batch, one mtg_tube_solve (the
                  compile-time-S kernels, LDS sized to that S), scatter
                  coeffs, cost, iters and status back into the padded outputs.
                  The grouping (a host sort of the counts) is done once,
                  outside the timed region.
  per_s_launches  the eleven launches alone, on rows gathered beforehand

The routes' results are compared first (statuses equal, cost and coeffs
1e-6, the tolerance of the tube tests: the routes run different bodies).
Prints one JSON line.
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

import ragged_bench as rb  # noqa: E402

RADIUS, TOL, MAX_ITER = 0.15, 1e-10, 100


def workload(mtg, B, dev):
    """Padded ragged tube inputs (NaN padding) and, per S, the rows that have it."""
    import torch
    N, M, S_MAX = rb.N, rb.N // 2, rb.S_MAX
    counts = np.random.default_rng(rb.SEED).integers(rb.S_MIN, S_MAX + 1, size=B).astype(np.int32)
    pos = np.full((B, S_MAX + 1, 3), np.nan)
    fv = np.full((B, 3, N), np.nan)
    times = np.full((B, S_MAX), np.nan)
    radii = np.full((B, S_MAX, 2), np.nan)
    groups = {}
    for S in range(rb.S_MIN, S_MAX + 1):
        _, f, t, p = mtg.generate_random_problems(N, 3, S, B, seed0=rb.SEED)
        idx = np.nonzero(counts == S)[0]
        if idx.size == 0:
            continue
        pos[idx, :S + 1] = np.asarray(p).reshape(B, S + 1, 3)[idx]
        fv[idx, :, :M] = f[idx, :, :M]             # start derivatives 0..M-1
        fv[idx, :, M:] = f[idx, :, N + S - 1 - M:]  # end derivatives 0..M-1
        times[idx, :S] = t[idx]
        radii[idx, :S] = RADIUS
        groups[S] = torch.from_numpy(idx).to(dev)
    T = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    return dict(seg_counts=T(counts), positions=T(pos), fixed_vals=T(fv), times_cp=T(times),
                times=T(times.copy()), radii=T(radii)), groups


def gather(inp, idx, S):
    return (inp["positions"][idx, :S + 1].contiguous(), inp["fixed_vals"][idx].contiguous(),
            inp["times_cp"][idx, :S].contiguous(), inp["times"][idx, :S].contiguous(),
            inp["radii"][idx, :S].contiguous())


def uniform_outputs(n, S, dev):
    import torch
    f64 = lambda *s: torch.empty(s, dtype=torch.float64, device=dev)  # noqa: E731
    i32 = lambda *s: torch.empty(s, dtype=torch.int32, device=dev)  # noqa: E731
    return dict(x=f64(n, 3 * (S - 1) * (rb.N // 2)), coeffs=f64(n, S, 3, rb.N), cost=f64(n),
                iters=i32(n), status=i32(n))


def tube_solve_into(mtg, ctx, S, rows, out, dev):
    """mtg_tube_solve into caller-owned outputs (the Python wrapper allocates)."""
    from mav_tube_trajectory_generation_amd.batch import _ptr, _stream
    p, f, tc, t, rd = rows
    mtg._abi.check(mtg.lib().mtg_tube_solve(
        ctx.handle, rb.N, rb.R, S, t.shape[0], _ptr(p), _ptr(f), _ptr(tc), _ptr(t), _ptr(rd),
        TOL, MAX_ITER, _ptr(out["x"]), _ptr(out["coeffs"]), _ptr(out["cost"]),
        _ptr(out["iters"]), _ptr(out["status"]), _stream(dev)), "mtg_tube_solve")


def measure(mtg, bench, ctx, dev, B, reps, rounds):
    import torch
    inp, groups = workload(mtg, B, dev)
    kw = dict(tol=TOL, max_iter=MAX_ITER)
    outs = {k: mtg.ragged_tube_solve(ctx, rb.N, rb.R, **inp, order=k == "ordered", **kw)
            for k in ("ordered", "plain")}
    s_out = {S: uniform_outputs(idx.numel(), S, dev) for S, idx in groups.items()}
    pre = {S: gather(inp, idx, S) for S, idx in groups.items()}
    all_ = dict(coeffs=torch.zeros((B, rb.S_MAX, 3, rb.N), dtype=torch.float64, device=dev),
                cost=torch.empty(B, dtype=torch.float64, device=dev),
                iters=torch.empty(B, dtype=torch.int32, device=dev),
                status=torch.empty(B, dtype=torch.int32, device=dev))

    def ragged_ordered():
        mtg.ragged_tube_solve(ctx, rb.N, rb.R, **inp, order=True, out=outs["ordered"], **kw)

    def ragged():
        mtg.ragged_tube_solve(ctx, rb.N, rb.R, **inp, order=False, out=outs["plain"], **kw)

    def per_s():
        for S, idx in groups.items():
            tube_solve_into(mtg, ctx, S, gather(inp, idx, S), s_out[S], dev)
            all_["coeffs"][idx, :S] = s_out[S]["coeffs"]
            for k in ("cost", "iters", "status"):
                all_[k][idx] = s_out[S][k]

    def per_s_launches():
        for S in groups:
            tube_solve_into(mtg, ctx, S, pre[S], s_out[S], dev)

    per_s()
    torch.cuda.synchronize()
    a, b = outs["ordered"], outs["plain"]
    for k in ("x", "coeffs", "cost", "iters", "status"):  # bit for bit
        v = (lambda t: t.view(torch.int64) if t.dtype == torch.float64 else t)
        assert torch.equal(v(a[k]), v(b[k])), k
    assert torch.equal(a["status"], all_["status"])
    ok = a["status"] == 0
    cerr = float(((a["cost"] - all_["cost"]).abs() / all_["cost"].abs().clamp_min(1e-300))[ok].max())
    num = (a["coeffs"] - all_["coeffs"]).norm(dim=3)
    den = all_["coeffs"].norm(dim=3).clamp_min(1e-12)
    kerr = float((num / den)[ok].max())
    assert cerr <= 1e-6 and kerr <= 1e-6, (cerr, kerr)
    m = rb.compare(bench, dict(ragged_ordered=ragged_ordered, ragged=ragged, per_s=per_s,
                               per_s_launches=per_s_launches), reps, rounds)
    m.update(batch=B, rows_status_ok=int(ok.sum().item()), cost_rel_diff=cerr,
             coeffs_rel_diff=kerr,
             iters_mean=round(float(a["iters"].double().mean().item()), 2),
             iters_max_abs_diff=int((a["iters"] - all_["iters"]).abs().max().item()))
    for route in ("ragged_ordered", "ragged"):
        for other in ("per_s", "per_s_launches"):
            m[f"ratio_{other}_over_{route}"] = {
                k: round(m[other][k]["median_us"] / m[route][k]["median_us"], 3)
                for k in ("eager", "graph")}
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="256,1024,4096")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("ragged_tube_bench.py needs a GPU: it measures, it does not fall back")
    import mav_tube_trajectory_generation_amd as mtg
    bench = rb.load_bench()
    dev = torch.device("cuda", 0)
    ctx = mtg.Context(0)
    res = dict(N=rb.N, r=rb.R, S_min=rb.S_MIN, S_max=rb.S_MAX, seed0=rb.SEED, radius=RADIUS,
               tol=TOL, max_iter=MAX_ITER, reps=a.reps, rounds=a.rounds, batches={})
    for B in (int(v) for v in a.batches.split(",")):
        res["batches"][str(B)] = measure(mtg, bench, ctx, dev, B, a.reps, a.rounds)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
