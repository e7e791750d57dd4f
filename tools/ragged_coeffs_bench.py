#!/usr/bin/env python3
"""The ragged coefficients-from-constraints entries against the per-count
route, on the GPU.

    python tools/ragged_coeffs_bench.py [--batches 256,1024,4096] [--std-batch 1024]
                                        [--reps 20] [--rounds 5]

Workload: N = 10, r = 4, D = 3.  Tube pattern: S_b uniform over 2..10,
S_max = 10, B rows per --batches; one standard-pattern line with S_b uniform
over 1..12, S_max = 12.  The kernel's time does not depend on the values, so
the derivatives are N(0, 1) and the times uniform over [0.5, 3]; the padding
of every input is NaN.  Timed as ragged_bench.py times (device events around
`reps` back-to-back calls, eagerly and replayed from a HIP graph, the routes
alternating for `rounds` rounds, medians and min..max), per line:

  ragged     one mtg_ragged_tube_coeffs / mtg_ragged_coeffs_from_constraints
             over the padded batch
  per_count  what a caller has without the entry: per count gather the
             group's rows out of the padded batch, one
             mtg_coeffs_from_constraints on the group's LinearPlan, scatter
             the coefficients and the cost back into the padded outputs.  The
             grouping (a host sort of the counts), the plans, the index
             tensors and every output are made once, outside the timed region.

Both routes' results are compared first (1e-12 normwise per segment and
dimension, 1e-9 on the cost).  Also reports the ragged call's store bandwidth
(coefficient bytes written, padding included, over the replayed time).
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

N, R, D, M, SEED = 10, 4, 3, 5, 105


def workload(B, S_min, S_max, tube, dev):
    """Padded random inputs (NaN padding) and the rows per count."""
    import torch
    rng = np.random.default_rng(SEED)
    counts = rng.integers(S_min, S_max + 1, size=B).astype(np.int32)
    mf = M if tube else M - 1
    nf_max = N if tube else N + S_max - 1
    fixed = np.full((B, D, nf_max), np.nan)
    free = np.full((B, D, (S_max - 1) * mf), np.nan)
    times = np.full((B, S_max), np.nan)
    for b, S in enumerate(counts):
        fixed[b, :, :N if tube else N + S - 1] = rng.standard_normal((D, N if tube else N + S - 1))
        free[b, :, :(S - 1) * mf] = rng.standard_normal((D, (S - 1) * mf))
        times[b, :S] = rng.uniform(0.5, 3.0, S)
    groups = {int(S): torch.from_numpy(np.nonzero(counts == S)[0]).to(dev)
              for S in range(S_min, S_max + 1) if (counts == S).any()}
    T = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    return dict(seg=T(counts), fixed=T(fixed), free=T(free), times=T(times)), groups


def measure(mtg, bench, ctx, dev, B, S_min, S_max, tube, reps, rounds):
    import torch
    from mav_tube_trajectory_generation_amd._abi import check
    from mav_tube_trajectory_generation_amd.batch import _ptr, _stream
    inp, groups = workload(B, S_min, S_max, tube, dev)
    mf = M if tube else M - 1
    f64 = lambda *s: torch.zeros(s, dtype=torch.float64, device=dev)  # noqa: E731
    i32 = lambda *s: torch.zeros(s, dtype=torch.int32, device=dev)  # noqa: E731
    rag = dict(coeffs=f64(B, S_max, D, N), cost=f64(B), status=i32(B))
    all_ = dict(coeffs=f64(B, S_max, D, N), cost=f64(B))
    rplan = None if tube else mtg.RaggedLinearPlan(ctx, N, D, R, S_max)
    plans, uni = {}, {}
    for S, idx in groups.items():
        mask = np.zeros((S + 1, M), np.uint8)
        mask[0, :] = mask[S, :] = 1
        if not tube:
            mask[:, 0] = 1
        plans[S] = mtg.LinearPlan(ctx, N, D, R, S, mask)
        n = idx.numel()
        uni[S] = dict(coeffs=f64(n, S, D, N), cost=f64(n), status=i32(n))

    def ragged():
        if tube:
            check(mtg.lib().mtg_ragged_tube_coeffs(
                ctx.handle, N, D, R, S_max, B, 0, _ptr(inp["seg"]), _ptr(inp["fixed"]),
                _ptr(inp["free"]), _ptr(inp["times"]), _ptr(rag["coeffs"]), _ptr(rag["cost"]),
                None, _ptr(rag["status"]), _stream(dev)), "mtg_ragged_tube_coeffs")
        else:
            check(mtg.lib().mtg_ragged_coeffs_from_constraints(
                rplan._h, B, _ptr(inp["seg"]), _ptr(inp["fixed"]), _ptr(inp["free"]),
                _ptr(inp["times"]), _ptr(rag["coeffs"]), _ptr(rag["cost"]), _ptr(rag["status"]),
                _stream(dev)), "mtg_ragged_coeffs_from_constraints")

    def per_count():
        for S, idx in groups.items():
            o = uni[S]
            fv = inp["fixed"][idx] if tube else inp["fixed"][idx, :, :N + S - 1].contiguous()
            fr = inp["free"][idx, :, :(S - 1) * mf].contiguous()
            t = inp["times"][idx, :S].contiguous()
            check(mtg.lib().mtg_coeffs_from_constraints(
                plans[S]._h, idx.numel(), _ptr(fv), _ptr(fr), _ptr(t), _ptr(o["coeffs"]),
                _ptr(o["cost"]), _ptr(o["status"]), _stream(dev)), "mtg_coeffs_from_constraints")
            all_["coeffs"][idx, :S] = o["coeffs"]
            all_["cost"][idx] = o["cost"]

    ragged()
    per_count()
    torch.cuda.synchronize()
    assert bool((rag["status"] == 0).all())
    num = (rag["coeffs"] - all_["coeffs"]).norm(dim=-1)
    den = all_["coeffs"].norm(dim=-1).clamp_min(1e-12)
    err_c = float((num / den).max().item())
    err_j = float(((rag["cost"] - all_["cost"]).abs() / all_["cost"].abs()).max().item())
    assert err_c <= 1e-12 and err_j <= 1e-9, (err_c, err_j)
    m = rb.compare(bench, dict(ragged=ragged, per_count=per_count), reps, rounds)
    stored = B * S_max * D * N * 8
    m.update(batch=B, pattern="tube" if tube else "standard", S_min=S_min, S_max=S_max,
             counts=len(groups), max_rel_err_coeffs=err_c, max_rel_err_cost=err_j,
             coeff_bytes_stored=stored,
             ragged_store_GBps=round(stored / (m["ragged"]["graph"]["median_us"] * 1e-6) / 1e9, 1))
    m["ratio_per_count_over_ragged"] = {
        k: round(m["per_count"][k]["median_us"] / m["ragged"][k]["median_us"], 3)
        for k in ("eager", "graph")}
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="256,1024,4096")
    ap.add_argument("--std-batch", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("ragged_coeffs_bench.py needs a GPU: it measures, it does not fall back")
    import mav_tube_trajectory_generation_amd as mtg
    bench = rb.load_bench()
    dev = torch.device("cuda", 0)
    ctx = mtg.Context(0)
    res = dict(N=N, r=R, D=D, seed0=SEED, reps=a.reps, rounds=a.rounds, lines=[])
    lines = [(int(v), 2, 10, True) for v in a.batches.split(",")] + [(a.std_batch, 1, 12, False)]
    for B, S_min, S_max, tube in lines:
        res["lines"].append(measure(mtg, bench, ctx, dev, B, S_min, S_max, tube, a.reps,
                                    a.rounds))
        print(json.dumps(res["lines"][-1]), file=sys.stderr, flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
