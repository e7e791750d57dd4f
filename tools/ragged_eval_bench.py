#!/usr/bin/env python3
"""The ragged evaluators against the per-S route, on the GPU.

    python tools/ragged_eval_bench.py [--batch 4096] [--sample-batch 1024]
                                      [--reps 200] [--sample-reps 20] [--rounds 5]

Workload: tools/ragged_bench.py's mixed-count batch (N = 10, D = 3, r = 4,
S_b uniform over 2..12, S_max = 12), solved once by the ragged solve; its
coeffs [B, S_max, D, N] and the NaN-padded times are what both routes read.
Timed as ragged_bench.py times (device events around `reps` back-to-back
calls, eagerly and replayed from a HIP graph, the routes alternating for
`rounds` rounds, medians and min..max):

  soft-constraint cost, constraints (1, v_max = 3) and (2, a_max = 5)
    ragged          one mtg_ragged_soft_constraint_cost
    per_s           per S: gather the group's rows coeffs[idx, :S],
                    times[idx, :S], one mtg_soft_constraint_cost, scatter cost
                    and maxima back.  The grouping (a host sort of the
                    counts) is done once, outside the timed region.
    per_s_launches  the eleven launches alone, on rows gathered beforehand
  sampling, dt = 0.01, derivatives 0..2, n_max fixed beforehand
    ragged          one mtg_ragged_sample_trajectories
    per_s           per S: gather, one mtg_sample_trajectories, scatter
                    samples and counts back
    per_s_launches  the eleven launches alone

Both routes' results are compared first (1e-9; sample counts equal).  Prints
one JSON line.
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

import ragged_bench as rb  # noqa: E402

DERS, LIMS = [1, 2], [3.0, 5.0]
DT, KMAX = 0.01, 2


def solved(mtg, ctx, B, dev):
    seg, fixed, times, _, groups = rb.workload(mtg, B, dev)
    plan = mtg.RaggedLinearPlan(ctx, rb.N, rb.D, rb.R, rb.S_MAX)
    out = plan.solve(seg, fixed, times)
    assert int(out["status"].abs().sum().item()) == 0
    return seg, out["coeffs"], times, groups


def ratios(res):
    res["ratio_per_s_over_ragged"] = {
        m: round(res["per_s"][m]["median_us"] / res["ragged"][m]["median_us"], 3)
        for m in ("eager", "graph")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--sample-batch", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--sample-reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("ragged_eval_bench.py needs a GPU: it measures, it does not fall back")
    import mav_tube_trajectory_generation_amd as mtg
    bench = rb.load_bench()
    dev = torch.device("cuda", 0)
    ctx = mtg.Context(0)
    res = dict(N=rb.N, D=rb.D, r=rb.R, S_min=rb.S_MIN, S_max=rb.S_MAX, seed0=rb.SEED,
               reps=a.reps, sample_reps=a.sample_reps, rounds=a.rounds)

    # -- soft-constraint cost ------------------------------------------------
    B = a.batch
    seg, coeffs, times, groups = solved(mtg, ctx, B, dev)
    r_out = mtg.ragged_soft_constraint_cost(seg, coeffs, times, DERS, LIMS)
    cost_all = torch.empty(B, dtype=torch.float64, device=dev)
    maxima_all = torch.empty((B, len(DERS)), dtype=torch.float64, device=dev)
    pre = {S: (coeffs[idx, :S].contiguous(), times[idx, :S].contiguous())
           for S, idx in groups.items()}
    s_out = {S: mtg.soft_constraint_cost(c, t, DERS, LIMS) for S, (c, t) in pre.items()}

    def soft_ragged():
        mtg.ragged_soft_constraint_cost(seg, coeffs, times, DERS, LIMS, out=r_out)

    def soft_per_s():
        for S, idx in groups.items():
            c = coeffs[idx, :S].contiguous()
            t = times[idx, :S].contiguous()
            mtg.soft_constraint_cost(c, t, DERS, LIMS, out=s_out[S])
            cost_all[idx] = s_out[S]["cost"]
            maxima_all[idx] = s_out[S]["maxima"]

    def soft_launches():
        for S, (c, t) in pre.items():
            mtg.soft_constraint_cost(c, t, DERS, LIMS, out=s_out[S])

    soft_ragged()
    soft_per_s()
    torch.cuda.synchronize()
    err = float(torch.max(torch.abs(r_out["maxima"] - maxima_all) / maxima_all).item())
    cerr = float(torch.max(torch.abs(r_out["cost"] - cost_all) / cost_all).item())
    assert err <= 1e-9 and cerr <= 1e-7, (err, cerr)  # exp(100 x) amplifies by 100 / limit
    soft = rb.compare(bench, dict(ragged=soft_ragged, per_s=soft_per_s,
                                  per_s_launches=soft_launches), a.reps, a.rounds)
    soft.update(batch=B, maxima_rel_diff=err, cost_rel_diff=cerr)
    ratios(soft)
    res["soft_constraint_cost"] = soft

    # -- sampling ------------------------------------------------------------
    B = a.sample_batch
    seg, coeffs, times, groups = solved(mtg, ctx, B, dev)
    span = float(torch.nan_to_num(times, nan=0.0).sum(dim=1).max().item())
    n_max = (int(span / DT) + 2 + 63) // 64 * 64
    nch = (KMAX + 1) * rb.D
    smp_all = torch.empty((B, nch, n_max), dtype=torch.float64, device=dev)
    cnt_all = torch.empty(B, dtype=torch.int32, device=dev)
    pre = {S: (coeffs[idx, :S].contiguous(), times[idx, :S].contiguous())
           for S, idx in groups.items()}
    kw = dict(max_derivative=KMAX, n_max=n_max, with_times=False)
    last = {}

    def smp_ragged():
        last["r"] = mtg.ragged_sample_trajectories(seg, coeffs, times, DT, **kw)

    def smp_per_s():
        for S, idx in groups.items():
            c = coeffs[idx, :S].contiguous()
            t = times[idx, :S].contiguous()
            s, _, n = mtg.sample_trajectories(c, t, DT, **kw)
            smp_all[idx] = s
            cnt_all[idx] = n

    def smp_launches():
        for S, (c, t) in pre.items():
            last[S] = mtg.sample_trajectories(c, t, DT, **kw)

    smp_ragged()
    smp_per_s()
    torch.cuda.synchronize()
    rs, _, rn = last["r"]
    assert torch.equal(rn, cnt_all)
    valid = torch.arange(n_max, device=dev)[None, None, :] < rn[:, None, None]
    diff = torch.where(valid, (rs - smp_all).abs(), torch.zeros((), dtype=rs.dtype, device=dev))
    scale = torch.where(valid, smp_all.abs(), torch.zeros((), dtype=rs.dtype, device=dev)).max()
    serr = float((diff.max() / scale).item())
    assert serr <= 1e-9, serr
    last.clear()
    smp = rb.compare(bench, dict(ragged=smp_ragged, per_s=smp_per_s,
                                 per_s_launches=smp_launches), a.sample_reps, a.rounds)
    smp.update(batch=B, dt=DT, max_derivative=KMAX, n_max=n_max,
               samples_total=int(rn.sum().item()), sample_rel_diff=serr)
    ratios(smp)
    res["sample_trajectories"] = smp
    print(json.dumps(res))


if __name__ == "__main__":
    main()
