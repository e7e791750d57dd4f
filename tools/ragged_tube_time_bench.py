#!/usr/bin/env python3
"""The ragged tube QCQP time optimiser against the per-S route, on the GPU.

    python tools/ragged_tube_time_bench.py [--batches 256,1024,4096] [--evals 50]
                                           [--reps 2] [--rounds 3]

Workload: tools/ragged_tube_bench.py's mixed-count tube batch (N = 10, r = 4,
S_b uniform over 2..12, S_max = 12, radii 0.15, tol 1e-10, at most 100 IPM
iterations), optimised with LN_SBPLX for E = 50 evaluations from the
estimateSegmentTimes start (time_penalty 500, f_rel 0.05, steps 0.1 T0).
Timed as ragged_bench.py times (device events around `reps` back-to-back
calls, eagerly and replayed from a HIP graph, the routes alternating for
`rounds` rounds, medians and min..max), per batch size:

  ragged  one mtg_ragged_tube_time_optimize over the padded batch
  per_s   what a caller has without the call: per S gather the group's rows
          out of the padded batch, one mtg_tube_time_optimize_ex with the
          group's own workspace (the compile-time-S kernels, LDS sized to that
          S, E rounds each), scatter times, cost, evals, result and status
          back.  The grouping (a host sort of the counts) and the workspaces
          are made once, outside the timed region.

Both routes start every call from a copy of the initial times.  The routes'
results are compared first by the agreement rule of the tests (a row agrees
when evals and result are equal, times within 1e-6 relative and cost within
1e-6; Subplex compares objective values and the routes run different
bodies): at least 15 of every 16 rows, the count is reported.
Prints one JSON line.
"""
import argparse
import ctypes
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

import ragged_bench as rb  # noqa: E402
import ragged_tube_bench as rtb  # noqa: E402


def measure(mtg, bench, ctx, dev, B, E, reps, rounds):
    import torch
    from mav_tube_trajectory_generation_amd._abi import check, make_time_params
    from mav_tube_trajectory_generation_amd.batch import _ptr, _stream
    N, R, S_MAX = rb.N, rb.R, rb.S_MAX
    inp, groups = rtb.workload(mtg, B, dev)
    p = make_time_params(optimizer="sbplx")
    pp = ctypes.byref(p)
    f64 = lambda *s: torch.empty(s, dtype=torch.float64, device=dev)  # noqa: E731
    i32 = lambda *s: torch.empty(s, dtype=torch.int32, device=dev)  # noqa: E731
    u8 = lambda n: torch.empty(n, dtype=torch.uint8, device=dev)  # noqa: E731

    def outputs(n, S):
        return dict(times=f64(n, S), cost=f64(n), evals=i32(n), result=i32(n), status=i32(n))

    t0 = inp["times"]
    rag = outputs(B, S_MAX)
    rag_ws = u8(mtg.ragged_tube_time_workspace_bytes(N, S_MAX, B, p, True))
    uni = {S: outputs(idx.numel(), S) for S, idx in groups.items()}
    uni_ws = {S: u8(mtg.tube_time_workspace_bytes(N, S, idx.numel(), p, True))
              for S, idx in groups.items()}
    all_ = outputs(B, S_MAX)

    def ragged():
        rag["times"].copy_(t0)
        check(mtg.lib().mtg_ragged_tube_time_optimize(
            ctx.handle, N, R, S_MAX, B, _ptr(inp["seg_counts"]), _ptr(inp["positions"]),
            _ptr(inp["fixed_vals"]), _ptr(inp["radii"]), _ptr(rag["times"]), rtb.TOL,
            rtb.MAX_ITER, pp, E, _ptr(rag["cost"]), _ptr(rag["evals"]), _ptr(rag["result"]),
            _ptr(rag["status"]), _ptr(rag_ws), rag_ws.numel(), _stream(dev)),
            "mtg_ragged_tube_time_optimize")

    def per_s():
        all_["times"].copy_(t0)
        for S, idx in groups.items():
            pos, fv, _, t, rd = rtb.gather(inp, idx, S)
            o, ws = uni[S], uni_ws[S]
            o["times"].copy_(t)
            check(mtg.lib().mtg_tube_time_optimize_ex(
                ctx.handle, N, R, S, idx.numel(), _ptr(pos), _ptr(fv), _ptr(rd), _ptr(o["times"]),
                rtb.TOL, rtb.MAX_ITER, pp, E, _ptr(o["cost"]), _ptr(o["evals"]),
                _ptr(o["result"]), _ptr(o["status"]), _ptr(ws), ws.numel(), _stream(dev)),
                "mtg_tube_time_optimize_ex")
            all_["times"][idx, :S] = o["times"]
            for k in ("cost", "evals", "result", "status"):
                all_[k][idx] = o[k]

    ragged()
    per_s()
    torch.cuda.synchronize()
    live = torch.arange(S_MAX, device=dev)[None, :] < inp["seg_counts"][:, None]
    rel = ((rag["times"] - all_["times"]).abs() / all_["times"].abs())
    terr = torch.where(live, rel, torch.zeros_like(rel)).max(dim=1).values
    cerr = (rag["cost"] - all_["cost"]).abs() / all_["cost"].abs()
    agree = ((rag["evals"] == all_["evals"]) & (rag["result"] == all_["result"])
             & (terr <= 1e-6) & (cerr <= 1e-6))
    n_agree = int(agree.sum().item())
    assert torch.equal(rag["status"], all_["status"])
    assert n_agree * 16 >= B * 15, (n_agree, B)
    m = rb.compare(bench, dict(ragged=ragged, per_s=per_s), reps, rounds)
    m.update(batch=B, rows_agree=n_agree, rows_status_ok=int((rag["status"] == 0).sum().item()),
             evals_mean=round(float(rag["evals"].double().mean().item()), 2),
             result_counts={str(c): int((rag["result"] == c).sum().item()) for c in (3, 4, 5)})
    m["ratio_per_s_over_ragged"] = {
        k: round(m["per_s"][k]["median_us"] / m["ragged"][k]["median_us"], 3)
        for k in ("eager", "graph")}
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="256,1024,4096")
    ap.add_argument("--evals", type=int, default=50)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("ragged_tube_time_bench.py needs a GPU: it measures, it does not fall back")
    import mav_tube_trajectory_generation_amd as mtg
    bench = rb.load_bench()
    dev = torch.device("cuda", 0)
    ctx = mtg.Context(0)
    res = dict(N=rb.N, r=rb.R, S_min=rb.S_MIN, S_max=rb.S_MAX, seed0=rb.SEED, radius=rtb.RADIUS,
               tol=rtb.TOL, max_iter=rtb.MAX_ITER, optimizer="LN_SBPLX", max_evals=a.evals,
               reps=a.reps, rounds=a.rounds, batches={})
    for B in (int(v) for v in a.batches.split(",")):
        res["batches"][str(B)] = measure(mtg, bench, ctx, dev, B, a.evals, a.reps, a.rounds)
        print(json.dumps({str(B): res["batches"][str(B)]}), file=sys.stderr, flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
