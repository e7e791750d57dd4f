#!/usr/bin/env python3
"""The ragged collision optimiser against the per-count route, on the GPU.

    python tools/ragged_coll_opt_bench.py [--batches 256,1024] [--evals 25]
                                          [--reps 2] [--rounds 3]

Workload: corridor paths through the demo's forest map (demo.forest_map) with
S_b uniform over 2..10 segments, S_max = 10: the demo's vertex polyline
resampled by arc length to S_b + 1 waypoints with 5 cm of jitter on the
intermediate ones, estimateSegmentTimes(., 2, 2), radii 0.15, x0 from one
mtg_ragged_tube_solve over the whole batch (N = 10, r = 4).  Optimised in mode
0 (x = d_p) with main.cpp's parameters (demo.coll_params()), 25 evaluations,
the near field of the map.  Timed as ragged_bench.py times (device events
around `reps` back-to-back calls, eagerly and replayed from a HIP graph, the
routes alternating for `rounds` rounds, medians and min..max), per batch size:

  ragged     one mtg_ragged_coll_optimize over the padded batch
  per_count  what a caller has without the call: per count gather the group's
             rows out of the padded batch, one mtg_coll_optimize on the
             group's LinearPlan with its own workspace, scatter x, cost,
             evals, result, status and terms back.  The grouping (a host sort
             of the counts), the plans and the workspaces are made once,
             outside the timed region.

Both routes start every call from a copy of x0.  Their results are compared
first: without soft constraints the two run the same bodies on the same
compact state, so every row must agree bit for bit.  Prints one JSON line.
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

import ragged_bench as rb  # noqa: E402

N, R, M, S_MIN, S_MAX, SEED = 10, 4, 5, 2, 10, 105


def resample(poly, S, rng):
    """S + 1 waypoints at equal arc length along poly, the inner ones jittered."""
    seg = np.linalg.norm(np.diff(poly, axis=0), axis=1)
    cum = np.concatenate([[0.0], np.cumsum(seg)])
    out = np.array([[np.interp(s, cum, poly[:, d]) for d in range(3)]
                    for s in np.linspace(0.0, cum[-1], S + 1)])
    out[1:S] += 0.05 * rng.standard_normal((S - 1, 3))
    return out


def workload(mtg, ctx, B, dev):
    """Padded inputs with x0 from the ragged tube solve, and the rows per count."""
    import torch
    from mav_tube_trajectory_generation_amd import demo
    rng = np.random.default_rng(SEED)
    counts = rng.integers(S_MIN, S_MAX + 1, size=B)
    probs = []
    for S in counts:
        pos = resample(demo.MAIN_POSITIONS, int(S), rng)
        _, df = demo.tube_pattern(pos)
        probs.append((pos, df, demo.estimate_segment_times(pos, 2.0, 2.0), np.full((S, 2), 0.15)))
    seg, pos, fv, times, radii = mtg.pack_ragged_tube(probs, N, dev, S_max=S_MAX)
    sol = mtg.ragged_tube_solve(ctx, N, R, seg, pos, fv, times, times, radii)
    assert bool(torch.isin(sol["status"], torch.tensor([0, 4], device=dev)).all())
    groups = {int(S): torch.from_numpy(np.nonzero(counts == S)[0]).to(dev)
              for S in range(S_MIN, S_MAX + 1) if (counts == S).any()}
    return dict(seg_counts=seg, fixed_vals=fv, times=times, x0=sol["x"]), groups


def measure(mtg, bench, ctx, dev, B, E, reps, rounds):
    import torch
    from mav_tube_trajectory_generation_amd import demo
    from mav_tube_trajectory_generation_amd._abi import check
    from mav_tube_trajectory_generation_amd.batch import _ptr, _stream
    inp, groups = workload(mtg, ctx, B, dev)
    occ = torch.from_numpy(demo.forest_map()).to(dev)
    prm = mtg.make_coll_params(**demo.coll_params())
    pp = ctypes.byref(prm)
    field = mtg.coll_field(occ, prm)
    nz, ny, nx = occ.shape
    f64 = lambda *s: torch.empty(s, dtype=torch.float64, device=dev)  # noqa: E731
    i32 = lambda *s: torch.empty(s, dtype=torch.int32, device=dev)  # noqa: E731
    u8 = lambda n: torch.empty(n, dtype=torch.uint8, device=dev)  # noqa: E731

    def outputs(n, np_):
        return dict(x=f64(n, 3, np_), cost=f64(n), evals=i32(n), result=i32(n), status=i32(n),
                    terms=f64(n, 4))

    np_max = (S_MAX - 1) * M
    rag, all_ = outputs(B, np_max), outputs(B, np_max)
    rag_ws = u8(mtg.ragged_coll_workspace_bytes(N, S_MAX, B, prm, 0, True))
    plans, uni, uni_ws = {}, {}, {}
    for S, idx in groups.items():
        mask = np.zeros((S + 1, M), np.uint8)
        mask[0, :] = mask[S, :] = 1
        plans[S] = mtg.LinearPlan(ctx, N, 3, R, S, mask)
        uni[S] = outputs(idx.numel(), (S - 1) * M)
        uni_ws[S] = u8(plans[S].coll_workspace_bytes(idx.numel(), prm, 0, True))

    def ragged():
        rag["x"].copy_(inp["x0"])
        check(mtg.lib().mtg_ragged_coll_optimize(
            ctx.handle, N, R, S_MAX, B, 0, _ptr(inp["seg_counts"]), _ptr(inp["fixed_vals"]),
            _ptr(rag["x"]), _ptr(inp["times"]), None, None, None, _ptr(occ), nx, ny, nz,
            _ptr(field), pp, E, _ptr(rag["cost"]), _ptr(rag["evals"]), _ptr(rag["result"]),
            _ptr(rag["status"]), _ptr(rag["terms"]), None, _ptr(rag_ws), rag_ws.numel(),
            _stream(dev)), "mtg_ragged_coll_optimize")

    def per_count():
        all_["x"].copy_(inp["x0"])
        for S, idx in groups.items():
            o, ws, np_ = uni[S], uni_ws[S], (S - 1) * M
            fv = inp["fixed_vals"][idx]
            t = inp["times"][idx, :S].contiguous()
            o["x"].copy_(inp["x0"][idx, :, :np_])
            check(mtg.lib().mtg_coll_optimize(
                plans[S]._h, idx.numel(), 0, _ptr(fv), _ptr(o["x"]), _ptr(t), None, None, None,
                _ptr(occ), nx, ny, nz, _ptr(field), pp, E, _ptr(o["cost"]), _ptr(o["evals"]),
                _ptr(o["result"]), _ptr(o["status"]), _ptr(o["terms"]), _ptr(ws), ws.numel(),
                _stream(dev)), "mtg_coll_optimize")
            all_["x"][idx, :, :np_] = o["x"]
            for k in ("cost", "evals", "result", "status", "terms"):
                all_[k][idx] = o[k]

    ragged()
    per_count()
    torch.cuda.synchronize()
    for k in ("evals", "result", "status"):
        assert torch.equal(rag[k], all_[k]), k
    for k in ("x", "cost", "terms"):
        assert torch.equal(rag[k].view(torch.int64), all_[k].view(torch.int64)), k
    m = rb.compare(bench, dict(ragged=ragged, per_count=per_count), reps, rounds)
    m.update(batch=B, counts=len(groups), rows_status_ok=int((rag["status"] == 0).sum().item()),
             evals_mean=round(float(rag["evals"].double().mean().item()), 2),
             rows_descended=int((rag["evals"] > 1).sum().item()))
    m["ratio_per_count_over_ragged"] = {
        k: round(m["per_count"][k]["median_us"] / m["ragged"][k]["median_us"], 3)
        for k in ("eager", "graph")}
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="256,1024")
    ap.add_argument("--evals", type=int, default=25)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("ragged_coll_opt_bench.py needs a GPU: it measures, it does not fall back")
    import mav_tube_trajectory_generation_amd as mtg
    bench = rb.load_bench()
    dev = torch.device("cuda", 0)
    ctx = mtg.Context(0)
    res = dict(N=N, r=R, S_min=S_MIN, S_max=S_MAX, seed0=SEED, mode=0, near_field=True,
               max_evals=a.evals, reps=a.reps, rounds=a.rounds, batches={})
    for B in (int(v) for v in a.batches.split(",")):
        res["batches"][str(B)] = measure(mtg, bench, ctx, dev, B, a.evals, a.reps, a.rounds)
        print(json.dumps({str(B): res["batches"][str(B)]}), file=sys.stderr, flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
