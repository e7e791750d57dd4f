#!/usr/bin/env python3
"""Ragged batch against the per-S route, on the GPU.

    python tools/ragged_bench.py [--batch 4096] [--opt-batch 1024] [--reps 200] [--rounds 5]

Workload: N = 10, D = 3, r = 4, trajectory b has S_b uniform over 2..12
(numpy default_rng(105)) and is createRandomVertices(seed 105 + b) with
estimateSegmentTimes, S_max = 12.  Timed, with device events around `reps`
back-to-back calls after a warm-up, eagerly (host enqueue included: what a
Python caller pays) and replayed from a HIP graph of the same calls (the
device's share), the routes alternating for `rounds` rounds (median and
min..max reported):

  ragged   one mtg_ragged_linear_solve over the padded batch
  per_s    what a caller has without it: eleven LinearPlans (one per S), per
           call the gathers of each group's rows out of the padded batch into
           per-S tensors, eleven mtg_linear_solve launches and the scatter of
           the costs back into one vector.  The grouping by S (a host sort of
           the counts) is done once, outside the timed region.
  per_s_launches  the eleven launches alone, on tensors gathered beforehand.

and the same for time_optimize (LN_SBPLX, 50 evaluations) at --opt-batch.
Both routes' costs are compared first (1e-9).  Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

N, D, R, S_MIN, S_MAX, SEED = 10, 3, 4, 2, 12, 105


def load_bench():
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(REPO, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def workload(mtg, B, dev):
    """Padded ragged inputs and, per S, the rows that have it."""
    import torch
    counts = np.random.default_rng(SEED).integers(S_MIN, S_MAX + 1, size=B).astype(np.int32)
    fixed = np.full((B, D, N + S_MAX - 1), np.nan)
    times = np.full((B, S_MAX), np.nan)
    masks, groups = {}, {}
    for S in range(S_MIN, S_MAX + 1):
        mask, f, t, _ = mtg.generate_random_problems(N, D, S, B, seed0=SEED)
        idx = np.nonzero(counts == S)[0]
        fixed[idx, :, :N + S - 1] = f[idx]
        times[idx, :S] = t[idx]
        masks[S] = mask
        groups[S] = torch.from_numpy(idx).to(dev)
    return (torch.from_numpy(counts).to(dev), torch.from_numpy(fixed).to(dev),
            torch.from_numpy(times).to(dev), masks, groups)


def timed(bench, fn, reps):
    import torch
    stream = torch.cuda.current_stream()
    ev = bench.TimingEvents("device")
    ev.record(0, stream)
    for _ in range(reps):
        fn()
    ev.record(1, stream)
    torch.cuda.synchronize()
    return ev.elapsed_ms() * 1e3 / reps  # us per call


def captured(fn, reps):
    """`reps` calls of fn captured in one HIP graph (one stream: a chain)."""
    import torch
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(reps):
            fn()
    g.replay()
    torch.cuda.synchronize()
    return g


def compare(bench, routes, reps, rounds):
    """Per route: eager calls (what a Python caller pays, host enqueue
    included) and the same calls replayed from a HIP graph (the device's
    share: bench.py's timed region is a replay too)."""
    import torch
    for fn in routes.values():  # warm-up: code objects, allocator
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    graphs = {k: captured(fn, reps) for k, fn in routes.items()}
    us = {k: [] for k in routes}
    us_g = {k: [] for k in routes}
    for _ in range(rounds):
        for k, fn in routes.items():
            us[k].append(timed(bench, fn, reps))
            us_g[k].append(timed(bench, graphs[k].replay, 1) / reps)

    def stats(v):
        return dict(median_us=round(statistics.median(v), 3), min_us=round(min(v), 3),
                    max_us=round(max(v), 3))
    return {k: dict(eager=stats(us[k]), graph=stats(us_g[k])) for k in routes}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--opt-batch", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--opt-reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("ragged_bench.py needs a GPU: it measures, it does not fall back")
    import mav_tube_trajectory_generation_amd as mtg
    bench = load_bench()
    dev = torch.device("cuda", 0)
    ctx = mtg.Context(0)
    res = dict(N=N, D=D, r=R, S_min=S_MIN, S_max=S_MAX, seed0=SEED, reps=a.reps,
               opt_reps=a.opt_reps, rounds=a.rounds)

    # -- linear solve ------------------------------------------------------
    B = a.batch
    seg, fixed, times, masks, groups = workload(mtg, B, dev)
    ragged = mtg.RaggedLinearPlan(ctx, N, D, R, S_MAX)
    plans = {S: mtg.LinearPlan(ctx, N, D, R, S, masks[S]) for S in groups}
    r_out = ragged.solve(seg, fixed, times)
    cost_all = torch.empty(B, dtype=torch.float64, device=dev)
    s_out = {S: plans[S].solve(fixed[idx, :, :N + S - 1].contiguous(),
                               times[idx, :S].contiguous()) for S, idx in groups.items()}
    pre = {S: (fixed[idx, :, :N + S - 1].contiguous(), times[idx, :S].contiguous())
           for S, idx in groups.items()}

    def run_ragged():
        ragged.solve(seg, fixed, times, out=r_out)

    def run_per_s():
        for S, idx in groups.items():
            f = fixed[idx, :, :N + S - 1].contiguous()
            t = times[idx, :S].contiguous()
            plans[S].solve(f, t, out=s_out[S])
            cost_all[idx] = s_out[S]["cost"]

    def run_launches():
        for S in groups:
            plans[S].solve(pre[S][0], pre[S][1], out=s_out[S])

    run_ragged()
    run_per_s()
    torch.cuda.synchronize()
    err = float(torch.max(torch.abs(r_out["cost"] - cost_all) / cost_all.abs()).item())
    assert err <= 1e-9 and int(r_out["status"].abs().sum().item()) == 0, err
    lin = compare(bench, dict(ragged=run_ragged, per_s=run_per_s, per_s_launches=run_launches),
                  a.reps, a.rounds)
    lin["batch"] = B
    lin["cost_rel_diff"] = err
    lin["ratio_per_s_over_ragged"] = {
        m: round(lin["per_s"][m]["median_us"] / lin["ragged"][m]["median_us"], 3)
        for m in ("eager", "graph")}
    res["linear"] = lin

    # -- time_optimize, LN_SBPLX, 50 evaluations ----------------------------
    B = a.opt_batch
    seg, fixed, times, masks, groups = workload(mtg, B, dev)
    plans = {S: mtg.LinearPlan(ctx, N, D, R, S, masks[S]) for S in groups}
    cost_opt = torch.empty(B, dtype=torch.float64, device=dev)
    kw = dict(max_evals=50, optimizer="sbplx")
    last = {}

    def opt_ragged():
        last["r"] = ragged.time_optimize(seg, fixed, times, **kw)

    def opt_per_s():
        for S, idx in groups.items():
            o = plans[S].time_optimize(fixed[idx, :, :N + S - 1].contiguous(),
                                       times[idx, :S].contiguous(), **kw)
            cost_opt[idx] = o["cost"]

    opt_ragged()
    opt_per_s()
    torch.cuda.synchronize()
    # Subplex compares values ~1e-12 apart between the two kernels, so a
    # near-tie may send a trajectory down another path: report the share.
    rel = torch.abs(last["r"]["cost"] - cost_opt) / cost_opt.abs()
    opt = compare(bench, dict(ragged=opt_ragged, per_s=opt_per_s), a.opt_reps, a.rounds)
    opt["batch"] = B
    opt["rows_within_1e-6"] = float((rel <= 1e-6).double().mean().item())
    opt["ratio_per_s_over_ragged"] = {
        m: round(opt["per_s"][m]["median_us"] / opt["ragged"][m]["median_us"], 3)
        for m in ("eager", "graph")}
    res["time_optimize_sbplx_50"] = opt
    print(json.dumps(res))


if __name__ == "__main__":
    main()
