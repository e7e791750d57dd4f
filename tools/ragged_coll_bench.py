#!/usr/bin/env python3
"""The ragged collision walk against the per-S route, on the GPU.

    python tools/ragged_coll_bench.py [--batch 4096] [--reps 20] [--rounds 5]

Workload: tools/ragged_bench.py's mixed-count batch (N = 10, D = 3, r = 4,
S_b uniform over 2..12, S_max = 12), solved once by the ragged solve and
shifted by +20 m into the map of tests/test_ragged_coll_gpu.py (160^3 voxels
of 0.25 m, 6000 scattered occupied voxels and 30 solid blocks, bounds
[0, 40]^3, robot radius 0.1, dt = 0.1, box side 20).  The gate input is the
solve's cost.  Timed as ragged_bench.py times (device events around `reps`
back-to-back calls, eagerly and replayed from a HIP graph, the routes
alternating for `rounds` rounds, medians and min..max), gate-only
(grad_coeffs not asked for) and with the coefficient gradient:

  ragged_field  one mtg_ragged_collision_cost with the map's near field
                (computed once per map, outside the timed region)
  ragged_scan   the same call without it (a workgroup scans every box)
  per_s         what a caller has without the call: per S gather the group's
                rows coeffs[idx, :S], times[idx, :S], one mtg_collision_cost
                (which takes no near field) through that S's LinearPlan,
                scatter cost, flags (and gradient) back, then mask the gate
                where a row collides.  The grouping (a host sort of the
                counts) is done once, outside the timed region.
  per_s_launches  the eleven launches alone, on rows gathered beforehand

Both routes' results are compared first (flags and gate equal, cost and
gradient 1e-9).  Prints one JSON line.
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

OFFSET = 20.0
PRM = dict(map_resolution=0.25, min_bound=[0.0] * 3, max_bound=[40.0] * 3, epsilon=0.5,
           robot_radius=0.1, coll_pot_multiplier=1.0, coll_check_time_increment=0.1)


def test_map(seed=5, n=160, n_obst=6000, n_blob=30):
    rng = np.random.default_rng(seed)
    occ = np.full((n, n, n), -1.0, np.float32)
    idx = rng.integers(0, n, size=(n_obst, 3))
    occ[idx[:, 2], idx[:, 1], idx[:, 0]] = rng.uniform(0.0, 2.0, n_obst)
    for _ in range(n_blob):
        c = rng.integers(10, n - 10, size=3)
        occ[c[2] - 2:c[2] + 3, c[1] - 2:c[1] + 3, c[0] - 2:c[0] + 3] = 1.0
    return occ


def bits(t):
    import torch
    return t.view(torch.int64) if t.dtype == torch.float64 else t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("ragged_coll_bench.py needs a GPU: it measures, it does not fall back")
    import mav_tube_trajectory_generation_amd as mtg
    bench = rb.load_bench()
    dev = torch.device("cuda", 0)
    ctx = mtg.Context(0)
    B = a.batch
    seg, fixed, times, masks, groups = rb.workload(mtg, B, dev)
    sol = mtg.RaggedLinearPlan(ctx, rb.N, rb.D, rb.R, rb.S_MAX).solve(seg, fixed, times)
    assert int(sol["status"].abs().sum().item()) == 0
    coeffs, gate = sol["coeffs"], sol["cost"]
    coeffs[:, :, :, 0] += OFFSET  # the same trajectories, inside the map
    occ = torch.from_numpy(test_map()).to(dev)
    params = mtg.make_collision_params(**PRM)
    field = mtg.coll_field(occ, params)
    plans = {S: mtg.LinearPlan(ctx, rb.N, rb.D, rb.R, S, masks[S]) for S in groups}
    pre = {S: (coeffs[idx, :S].contiguous(), times[idx, :S].contiguous())
           for S, idx in groups.items()}
    inf = torch.full((), float("inf"), dtype=torch.float64, device=dev)
    res = dict(N=rb.N, D=rb.D, r=rb.R, S_min=rb.S_MIN, S_max=rb.S_MAX, seed0=rb.SEED, batch=B,
               reps=a.reps, rounds=a.rounds, params=PRM, box_side=int(params.box_side))

    for mode, grad in (("gate_only", False), ("with_gradient", True)):
        outs = {k: None for k in ("field", "scan")}
        cost_all = torch.empty(B, dtype=torch.float64, device=dev)
        coll_all = torch.empty(B, dtype=torch.int32, device=dev)
        gc_all = torch.zeros((B, rb.S_MAX, rb.D, rb.N), dtype=torch.float64, device=dev)
        last = {}

        def ragged_field():
            outs["field"] = mtg.ragged_collision_cost(seg, coeffs, times, occ, params,
                                                      near_field=field, grad=grad, gate=gate,
                                                      out=outs["field"])

        def ragged_scan():
            outs["scan"] = mtg.ragged_collision_cost(seg, coeffs, times, occ, params, grad=grad,
                                                     gate=gate, out=outs["scan"])

        def per_s():
            for S, idx in groups.items():
                c = coeffs[idx, :S].contiguous()
                t = times[idx, :S].contiguous()
                o = plans[S].collision_cost(c, t, occ, params, grad=grad)
                cost_all[idx] = o["cost"]
                coll_all[idx] = o["collision"]
                if grad:
                    gc_all[idx, :S] = o["grad_coeffs"]
            last["gated"] = torch.where(coll_all != 0, inf, gate)

        def per_s_launches():
            for S, (c, t) in pre.items():
                last[S] = plans[S].collision_cost(c, t, occ, params, grad=grad)

        ragged_field()
        ragged_scan()
        per_s()
        torch.cuda.synchronize()
        r = outs["field"]
        for k in r:  # bit for bit, NaN included
            assert torch.equal(bits(r[k]), bits(outs["scan"][k])), k
        assert torch.equal(r["collision"], coll_all)
        assert torch.equal(r["gated"], last["gated"])
        cerr = float(((r["cost"] - cost_all).abs() / cost_all.abs().clamp_min(1e-300)).max())
        assert cerr <= 1e-9, cerr
        gerr = 0.0
        if grad:
            gerr = float(((r["grad_coeffs"] - gc_all).abs().amax(dim=(1, 2, 3)) /
                          gc_all.abs().amax(dim=(1, 2, 3)).clamp_min(1e-300)).max())
            assert gerr <= 1e-9, gerr
        m = rb.compare(bench, dict(ragged_field=ragged_field, ragged_scan=ragged_scan,
                                   per_s=per_s, per_s_launches=per_s_launches), a.reps, a.rounds)
        m.update(rows_colliding=int((coll_all != 0).sum().item()), cost_rel_diff=cerr,
                 grad_rel_diff=gerr)
        for route in ("ragged_field", "ragged_scan"):
            m[f"ratio_per_s_over_{route}"] = {
                k: round(m["per_s"][k]["median_us"] / m[route][k]["median_us"], 3)
                for k in ("eager", "graph")}
        res[mode] = m
        last.clear()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
