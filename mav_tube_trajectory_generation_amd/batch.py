"""Batched Python front end of libmtg_hip.so.

Device buffers are torch CUDA (HIP) tensors: PyTorch supplies HBM
allocations and the current stream only; every computation is a gfx950 kernel
of libmtg_hip.so.  Host-array entry points (numpy) copy through the library's
own host ABI.
"""
import ctypes

import numpy as np

from . import _abi
from ._abi import (MTGError, check, lib, make_coll_params, make_collision_params,  # noqa: F401
                   make_time_params)


def _ptr(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _stream(device=None):
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _require(t, shape, name):
    import torch
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise MTGError(f"{name} must be a CUDA tensor")
    if t.dtype != torch.float64:
        raise MTGError(f"{name} must be float64 (the path computes in FP64)")
    if tuple(t.shape) != tuple(shape):
        raise MTGError(f"{name} has shape {tuple(t.shape)}, expected {tuple(shape)}")
    if not t.is_contiguous():
        raise MTGError(f"{name} must be contiguous")


class Context:
    """One HIP device (mtg_ctx_create)."""

    def __init__(self, device=0):
        self._h = ctypes.c_void_p()
        check(lib().mtg_ctx_create(device, ctypes.byref(self._h)), "mtg_ctx_create")
        self.device = device

    @property
    def handle(self):
        return self._h

    def close(self):
        if self._h:
            lib().mtg_ctx_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class LinearPlan:
    """(N, D, r, S, constraint pattern) -> batched solves (mtg_plan_create)."""

    def __init__(self, ctx, N, D, r, S, fixed_mask):
        mask = np.ascontiguousarray(np.asarray(fixed_mask, dtype=np.uint8).reshape(-1))
        if mask.size != (S + 1) * (N // 2):
            raise MTGError(f"fixed_mask must have (S+1)*N/2 = {(S + 1) * (N // 2)} entries")
        self.ctx, self.N, self.D, self.r, self.S = ctx, N, D, r, S
        self.mask = mask.reshape(S + 1, N // 2).copy()
        self._h = ctypes.c_void_p()
        check(lib().mtg_plan_create(ctx.handle, N, D, r, S,
                                    mask.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
                                    ctypes.byref(self._h)), "mtg_plan_create")
        nf, np_ = ctypes.c_int(), ctypes.c_int()
        check(lib().mtg_plan_counts(self._h, ctypes.byref(nf), ctypes.byref(np_)), "counts")
        self.n_fixed, self.n_free = nf.value, np_.value

    KERNELS = {"auto": 0, "generic": 1, "standard": 2, "lane": 3, "lane_pair": 4}
    _NAMES = {v: k for k, v in KERNELS.items()}

    def set_kernel(self, which):
        """Select the linear-solve kernel: "auto" (default), "generic",
        "standard" (one wavefront per trajectory) or "lane" (one
        (trajectory, dimension) per lane); MTGError where the pattern or
        sizes do not allow it."""
        check(lib().mtg_plan_set_kernel(self._h, self.KERNELS[which]), "mtg_plan_set_kernel")
        return self

    @property
    def kernel(self):
        """The forced kernel, or for "auto" the wavefront kernel ("generic" or
        "standard"); see kernel_for_batch."""
        k = lib().mtg_plan_kernel(self._h)
        check(min(k, 0), "mtg_plan_kernel")
        return self._NAMES[k]

    def kernel_for_batch(self, B):
        """Kernel a solve of B trajectories runs."""
        k = lib().mtg_plan_kernel_for_batch(self._h, B)
        check(min(k, 0), "mtg_plan_kernel_for_batch")
        return self._NAMES[k]

    def close(self):
        if self._h:
            lib().mtg_plan_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- device (torch) API -------------------------------------------------
    def solve(self, fixed_vals, times, cost=True, free=False, status=True, out=None):
        """Batched solveLinear + computeCost on device tensors.

        fixed_vals [B, D, n_fixed], times [B, S] (float64, CUDA).  Returns a
        dict with coeffs [B, S, D, N] and optionally cost [B], free [B, D,
        n_free], status [B] (int32).
        """
        import torch
        B = times.shape[0]
        _require(times, (B, self.S), "times")
        _require(fixed_vals, (B, self.D, self.n_fixed), "fixed_vals")
        dev = times.device
        o = out or {}
        if "coeffs" not in o:
            o["coeffs"] = torch.empty((B, self.S, self.D, self.N), dtype=torch.float64, device=dev)
        if cost and "cost" not in o:
            o["cost"] = torch.empty(B, dtype=torch.float64, device=dev)
        if free and "free" not in o:
            o["free"] = torch.empty((B, self.D, self.n_free), dtype=torch.float64, device=dev)
        if status and "status" not in o:
            o["status"] = torch.empty(B, dtype=torch.int32, device=dev)
        check(lib().mtg_linear_solve(self._h, B, _ptr(fixed_vals), _ptr(times), _ptr(o["coeffs"]),
                                     _ptr(o.get("cost")), _ptr(o.get("free")),
                                     _ptr(o.get("status")), _stream(dev)), "mtg_linear_solve")
        return o

    def select_workspace(self, B, device):
        """Workspace of solve_select for B trajectories (per-workgroup
        partials of the lane kernels; empty for the wavefront kernels)."""
        import torch
        n = lib().mtg_select_workspace_bytes(self._h, B)
        if n < 0:
            check(int(n), "mtg_select_workspace_bytes")
        return torch.empty(int(n), dtype=torch.uint8, device=device)

    def solve_select(self, fixed_vals, times, start, rank, workspace, out=None, free=False,
                     status=True):
        """solve() followed by the shard's selection (mtg_linear_solve_select:
        lane kernels reduce per-workgroup partials written by the solve's
        epilogue): adds "triple" = (cost, start + index, rank), the
        select_local rule, as a float64 device tensor [3].
        workspace from select_workspace(B)."""
        import torch
        B = times.shape[0]
        _require(times, (B, self.S), "times")
        _require(fixed_vals, (B, self.D, self.n_fixed), "fixed_vals")
        dev = times.device
        o = out or {}
        if "coeffs" not in o:
            o["coeffs"] = torch.empty((B, self.S, self.D, self.N), dtype=torch.float64, device=dev)
        if "cost" not in o:
            o["cost"] = torch.empty(B, dtype=torch.float64, device=dev)
        if free and "free" not in o:
            o["free"] = torch.empty((B, self.D, self.n_free), dtype=torch.float64, device=dev)
        if status and "status" not in o:
            o["status"] = torch.empty(B, dtype=torch.int32, device=dev)
        if "triple" not in o:
            o["triple"] = torch.empty(3, dtype=torch.float64, device=dev)
        check(lib().mtg_linear_solve_select(
            self._h, B, _ptr(fixed_vals), _ptr(times), _ptr(o["coeffs"]), _ptr(o["cost"]),
            _ptr(o.get("free")), _ptr(o.get("status")), int(start), int(rank), _ptr(o["triple"]),
            _ptr(workspace), workspace.numel(), _stream(dev)), "mtg_linear_solve_select")
        return o

    def solve_select_prev(self, fixed_vals, times, out, prev_cost=None, prev_start=0, rank=0,
                          prev_triple=None):
        """solve() into the output set `out` (coeffs, cost, status) with the
        previous step's shard selection in the same launch
        (mtg_linear_solve_select_prev): prev_cost [n] (another output set's
        costs) reduced to prev_triple [3] = (cost, prev_start + index, rank).
        prev_cost None: the plain solve."""
        B = times.shape[0]
        _require(times, (B, self.S), "times")
        _require(fixed_vals, (B, self.D, self.n_fixed), "fixed_vals")
        n = 0 if prev_cost is None else prev_cost.numel()
        check(lib().mtg_linear_solve_select_prev(
            self._h, B, _ptr(fixed_vals), _ptr(times), _ptr(out["coeffs"]), _ptr(out.get("cost")),
            _ptr(out.get("free")), _ptr(out.get("status")), _ptr(prev_cost), n, int(prev_start),
            int(rank), _ptr(prev_triple), _stream(times.device)), "mtg_linear_solve_select_prev")
        return out

    def coefficients(self, fixed_vals, free_vals, times):
        """Coefficients and cost from given d_f and d_p, no solve
        (setFreeConstraints, linear_impl:497-506).  Returns (coeffs, cost,
        status)."""
        import torch
        B = times.shape[0]
        _require(times, (B, self.S), "times")
        _require(fixed_vals, (B, self.D, self.n_fixed), "fixed_vals")
        _require(free_vals, (B, self.D, self.n_free), "free_vals")
        dev = times.device
        coeffs = torch.empty((B, self.S, self.D, self.N), dtype=torch.float64, device=dev)
        cost = torch.empty(B, dtype=torch.float64, device=dev)
        status = torch.empty(B, dtype=torch.int32, device=dev)
        check(lib().mtg_coeffs_from_constraints(self._h, B, _ptr(fixed_vals), _ptr(free_vals),
                                                _ptr(times), _ptr(coeffs), _ptr(cost),
                                                _ptr(status), _stream(dev)),
              "mtg_coeffs_from_constraints")
        return coeffs, cost, status

    def time_cost(self, fixed_vals, times, time_penalty=500.0, grad_mode=0, increment=0.1,
                  w_d=0.1, w_t=1.0, soft=None, soft_weight=100.0, hard=False,
                  hard_tolerance=0.1):
        """objectiveFunctionTime per trajectory (mtg_time_cost); soft: list of
        (derivative, maximum_value) soft magnitude constraints."""
        import torch
        B = times.shape[0]
        _require(times, (B, self.S), "times")
        _require(fixed_vals, (B, self.D, self.n_fixed), "fixed_vals")
        dev = times.device
        cost = torch.empty(B, dtype=torch.float64, device=dev)
        grad = torch.empty((B, self.S), dtype=torch.float64, device=dev) if grad_mode else None
        status = torch.empty(B, dtype=torch.int32, device=dev)
        p = make_time_params(time_penalty, increment, w_d, w_t, grad_mode, soft, soft_weight,
                             hard=hard, hard_tolerance=hard_tolerance)
        check(lib().mtg_time_cost(self._h, B, _ptr(fixed_vals), _ptr(times), ctypes.byref(p),
                                  _ptr(cost), _ptr(grad), _ptr(status), _stream(dev)),
              "mtg_time_cost")
        return dict(cost=cost, grad=grad, status=status)

    def time_optimize(self, fixed_vals, times, max_evals=50, time_penalty=500.0, increment=0.1,
                      w_d=0.1, w_t=1.0, soft=None, soft_weight=100.0, hard=False,
                      hard_tolerance=0.1, optimizer="fd", f_rel=0.05, f_abs=-1.0,
                      initial_stepsize_rel=0.1):
        """Optimise segment times in place on a copy; returns dict(times, cost,
        evals, solves, result, status); solves = inner solves run (gradient
        points included), result = the nlopt_result stopping code
        (mtg_time_optimize_ex).  optimizer "fd" (projected central-difference
        descent) or "sbplx" (LN_SBPLX, the reference's default algorithm,
        with f_rel / f_abs / initial_stepsize_rel as
        NonlinearOptimizationParameters)."""
        import torch
        B = times.shape[0]
        _require(times, (B, self.S), "times")
        _require(fixed_vals, (B, self.D, self.n_fixed), "fixed_vals")
        dev = times.device
        t = times.clone()
        cost = torch.empty(B, dtype=torch.float64, device=dev)
        evals = torch.empty(B, dtype=torch.int32, device=dev)
        solves = torch.empty(B, dtype=torch.int32, device=dev)
        result = torch.empty(B, dtype=torch.int32, device=dev)
        status = torch.empty(B, dtype=torch.int32, device=dev)
        p = make_time_params(time_penalty, increment, w_d, w_t, 2, soft, soft_weight,
                             hard=hard, hard_tolerance=hard_tolerance, optimizer=optimizer,
                             f_rel=f_rel, f_abs=f_abs, initial_stepsize_rel=initial_stepsize_rel)
        check(lib().mtg_time_optimize_ex(self._h, B, _ptr(fixed_vals), _ptr(t), ctypes.byref(p),
                                         max_evals, _ptr(cost), _ptr(evals), _ptr(solves),
                                         _ptr(result), _ptr(status), _stream(dev)),
              "mtg_time_optimize_ex")
        return dict(times=t, cost=cost, evals=evals, solves=solves, result=result,
                    status=status)

    def free_cost(self, fixed_vals, free_vals, times, mode=0, time_penalty=500.0, soft=None,
                  soft_weight=100.0, grad=True):
        """Free-derivative objectives (mtg_free_cost): mode 0
        objectiveFunctionFreeConstraints (J_d [+ soft], gradient of J_d
        [B, D, n_free]); mode 1 objectiveFunctionTimeAndConstraints."""
        import torch
        B = times.shape[0]
        _require(times, (B, self.S), "times")
        _require(fixed_vals, (B, self.D, self.n_fixed), "fixed_vals")
        _require(free_vals, (B, self.D, self.n_free), "free_vals")
        dev = times.device
        cost = torch.empty(B, dtype=torch.float64, device=dev)
        g = (torch.empty((B, self.D, self.n_free), dtype=torch.float64, device=dev)
             if (grad and mode == 0) else None)
        status = torch.empty(B, dtype=torch.int32, device=dev)
        p = make_time_params(time_penalty, 0.1, 0.1, 1.0, 0, soft, soft_weight)
        check(lib().mtg_free_cost(self._h, B, _ptr(fixed_vals), _ptr(free_vals), _ptr(times),
                                  ctypes.byref(p), mode, _ptr(cost), _ptr(g), _ptr(status),
                                  _stream(dev)), "mtg_free_cost")
        return dict(cost=cost, grad=g, status=status)

    def free_optimize(self, fixed_vals, free_vals, times, max_evals=50, lower=None, upper=None,
                      soft=None, soft_weight=100.0):
        """Optimise the free derivatives (mtg_free_optimize) on a copy of
        free_vals; returns dict(free, cost, evals, status)."""
        import torch
        B = times.shape[0]
        _require(times, (B, self.S), "times")
        _require(fixed_vals, (B, self.D, self.n_fixed), "fixed_vals")
        _require(free_vals, (B, self.D, self.n_free), "free_vals")
        for name, a in (("lower", lower), ("upper", upper)):
            if a is not None:
                _require(a, (B, self.D, self.n_free), name)
        dev = times.device
        d = free_vals.clone()
        cost = torch.empty(B, dtype=torch.float64, device=dev)
        evals = torch.empty(B, dtype=torch.int32, device=dev)
        status = torch.empty(B, dtype=torch.int32, device=dev)
        p = make_time_params(500.0, 0.1, 0.1, 1.0, 0, soft, soft_weight)
        check(lib().mtg_free_optimize(self._h, B, _ptr(fixed_vals), _ptr(d), _ptr(times),
                                      _ptr(lower), _ptr(upper), ctypes.byref(p), max_evals,
                                      _ptr(cost), _ptr(evals), _ptr(status), _stream(dev)),
              "mtg_free_optimize")
        return dict(free=d, cost=cost, evals=evals, status=status)

    def time_free_optimize(self, fixed_vals, free_vals, times, max_evals=50, time_penalty=500.0,
                           increment=0.1, soft=None, soft_weight=100.0, optimizer="fd",
                           f_rel=0.05, f_abs=-1.0, initial_stepsize_rel=0.1):
        """Optimise segment times and free derivatives together
        (mtg_time_free_optimize_ex, optimizeTimeAndFreeConstraints) on copies;
        optimizer "sbplx" runs LN_SBPLX over [T; d_p] (the reference's
        algorithm), "fd" the block-alternating descent.  Returns dict(times,
        free, cost, evals, result, status)."""
        import torch
        B = times.shape[0]
        _require(times, (B, self.S), "times")
        _require(fixed_vals, (B, self.D, self.n_fixed), "fixed_vals")
        _require(free_vals, (B, self.D, self.n_free), "free_vals")
        dev = times.device
        t = times.clone()
        d = free_vals.clone()
        cost = torch.empty(B, dtype=torch.float64, device=dev)
        evals = torch.empty(B, dtype=torch.int32, device=dev)
        result = torch.full((B,), 0, dtype=torch.int32, device=dev)
        status = torch.empty(B, dtype=torch.int32, device=dev)
        p = make_time_params(time_penalty, increment, 0.1, 1.0, 0, soft, soft_weight,
                             optimizer=optimizer, f_rel=f_rel, f_abs=f_abs,
                             initial_stepsize_rel=initial_stepsize_rel)
        check(lib().mtg_time_free_optimize_ex(self._h, B, _ptr(fixed_vals), _ptr(d), _ptr(t),
                                              ctypes.byref(p), max_evals, _ptr(cost),
                                              _ptr(evals), _ptr(result), _ptr(status),
                                              _stream(dev)), "mtg_time_free_optimize_ex")
        return dict(times=t, free=d, cost=cost, evals=evals, result=result, status=status)

    def collision_cost(self, coeffs, times, occupancy, params, grad=True):
        """Collision cost over a dense occupancy grid (mtg_collision_cost,
        getCostAndGradientCollision): coeffs [B, S, 3, N], times [B, S],
        occupancy float32 CUDA tensor [nz, ny, nx] (occupied iff >= 0),
        params from make_collision_params.  Returns dict(cost, collision,
        grad_coeffs, grad_free)."""
        import torch
        B = times.shape[0]
        _require(times, (B, self.S), "times")
        _require(coeffs, (B, self.S, self.D, self.N), "coeffs")
        if not (isinstance(occupancy, torch.Tensor) and occupancy.is_cuda and
                occupancy.dtype == torch.float32 and occupancy.dim() == 3 and
                occupancy.is_contiguous()):
            raise MTGError("occupancy must be a contiguous float32 CUDA tensor [nz, ny, nx]")
        nz, ny, nx = occupancy.shape
        dev = times.device
        cost = torch.empty(B, dtype=torch.float64, device=dev)
        coll = torch.empty(B, dtype=torch.int32, device=dev)
        gc = torch.empty((B, self.S, self.D, self.N), dtype=torch.float64, device=dev) \
            if grad else None
        gf = torch.empty((B, self.D, self.n_free), dtype=torch.float64, device=dev) \
            if grad else None
        check(lib().mtg_collision_cost(self._h, B, _ptr(coeffs), _ptr(times), _ptr(occupancy),
                                       nx, ny, nz, ctypes.byref(params), _ptr(cost), _ptr(coll),
                                       _ptr(gc), _ptr(gf), _stream(dev)), "mtg_collision_cost")
        return dict(cost=cost, collision=coll, grad_coeffs=gc, grad_free=gf)

    # -- collision-driven objectives (mtg_coll_cost / mtg_coll_optimize) -----
    def _n_vars(self, mode):
        return (self.S if mode else 0) + self.D * self.n_free

    def coll_workspace_bytes(self, B, params, mode=0, optimize=False):
        n = lib().mtg_coll_workspace_bytes(self._h, B, mode, ctypes.byref(params),
                                           1 if optimize else 0)
        if n < 0:
            check(int(n), "mtg_coll_workspace_bytes")
        return int(n)

    def _coll_inputs(self, fixed_vals, x, times, occupancy, mode):
        import torch
        B = x.shape[0]
        _require(fixed_vals, (B, self.D, self.n_fixed), "fixed_vals")
        _require(x, (B, self._n_vars(mode)), "x")
        if mode == 0:
            _require(times, (B, self.S), "times")
        if not (isinstance(occupancy, torch.Tensor) and occupancy.is_cuda and
                occupancy.dtype == torch.float32 and occupancy.dim() == 3 and
                occupancy.is_contiguous()):
            raise MTGError("occupancy must be a contiguous float32 CUDA tensor [nz, ny, nx]")
        return B

    def coll_cost(self, fixed_vals, x, times, occupancy, params, mode=0, raise_ref=None,
                  grad=True, workspace=None, near_field=None):
        """objectiveFunctionFreeConstraintsAndCollision (mode 0, x = d_p
        [B, D*n_free]) or ...AndCollisionAndTime (mode 1, x = [T; d_p]
        [B, S + D*n_free]) on the device (mtg_coll_cost).  params from
        make_coll_params; raise_ref [B] the collision raise reference (None:
        0); near_field from coll_field(occupancy, params) (None: every
        sample's box is scanned).  Returns dict(cost, grad, terms [B, 4],
        collision, status)."""
        import torch
        B = self._coll_inputs(fixed_vals, x, times, occupancy, mode)
        _check_field(near_field, occupancy)
        dev = x.device
        nz, ny, nx = occupancy.shape
        cost = torch.empty(B, dtype=torch.float64, device=dev)
        g = torch.empty((B, self._n_vars(mode)), dtype=torch.float64, device=dev) if grad else None
        terms = torch.empty((B, 4), dtype=torch.float64, device=dev)
        coll = torch.empty(B, dtype=torch.int32, device=dev)
        st = torch.empty(B, dtype=torch.int32, device=dev)
        nb = self.coll_workspace_bytes(B, params, mode, False)
        ws = _workspace(workspace, nb, dev)
        check(lib().mtg_coll_cost(self._h, B, mode, _ptr(fixed_vals), _ptr(x),
                                  _ptr(times) if mode == 0 else None, _ptr(occupancy), nx, ny,
                                  nz, _ptr(near_field), ctypes.byref(params), _ptr(raise_ref),
                                  _ptr(cost), _ptr(g),
                                  _ptr(terms), _ptr(coll), _ptr(st), _ptr(ws), nb,
                                  _stream(dev)), "mtg_coll_cost")
        return dict(cost=cost, grad=g, terms=terms, collision=coll, status=st)

    def coll_optimize(self, fixed_vals, x0, times, occupancy, params, mode=0, max_evals=25,
                      lower=None, upper=None, initial_step=None, workspace=None,
                      near_field=None, history=False):
        """Device L-BFGS over the collision objective (mtg_coll_optimize;
        optimizeFreeConstraintsAndCollision / ...AndTime with NLopt
        replaced); near_field as coll_cost.  Returns dict(x, cost, evals,
        result, status, terms); with history=True also x_history
        (B x max_evals x nv, nv = the number of optimisation variables,
        _n_vars(mode): D * n_free in mode 0, S + D * n_free in mode 1; the
        evaluated points in order, rows past evals unset:
        mtg_coll_optimize_trace)."""
        import torch
        B = self._coll_inputs(fixed_vals, x0, times, occupancy, mode)
        _check_field(near_field, occupancy)
        dev = x0.device
        nv = self._n_vars(mode)
        for a, name in ((lower, "lower"), (upper, "upper"), (initial_step, "initial_step")):
            if a is not None:
                _require(a, (B, nv), name)
        nz, ny, nx = occupancy.shape
        x = x0.clone()
        cost = torch.empty(B, dtype=torch.float64, device=dev)
        ev = torch.empty(B, dtype=torch.int32, device=dev)
        res = torch.empty(B, dtype=torch.int32, device=dev)
        st = torch.empty(B, dtype=torch.int32, device=dev)
        terms = torch.empty((B, 4), dtype=torch.float64, device=dev)
        nb = self.coll_workspace_bytes(B, params, mode, True)
        ws = _workspace(workspace, nb, dev)
        hist = (torch.full((B, max_evals, nv), float("nan"), dtype=torch.float64, device=dev)
                if history else None)
        check(lib().mtg_coll_optimize_trace(self._h, B, mode, _ptr(fixed_vals), _ptr(x),
                                            _ptr(times) if mode == 0 else None, _ptr(lower),
                                            _ptr(upper), _ptr(initial_step), _ptr(occupancy), nx,
                                            ny, nz, _ptr(near_field), ctypes.byref(params),
                                            max_evals, _ptr(cost), _ptr(ev), _ptr(res), _ptr(st),
                                            _ptr(terms), _ptr(hist), _ptr(ws), nb, _stream(dev)),
              "mtg_coll_optimize_trace")
        out = dict(x=x, cost=cost, evals=ev, result=res, status=st, terms=terms)
        if history:
            out["x_history"] = hist
        return out

    # -- host (numpy) API ---------------------------------------------------
    def solve_host(self, fixed_vals, times):
        fixed_vals = np.ascontiguousarray(fixed_vals, dtype=np.float64)
        times = np.ascontiguousarray(times, dtype=np.float64)
        B = times.shape[0]
        coeffs = np.zeros((B, self.S, self.D, self.N))
        cost = np.zeros(B)
        free = np.zeros((B, self.D, self.n_free))
        status = np.zeros(B, dtype=np.int32)
        dp = ctypes.POINTER(ctypes.c_double)
        rc = lib().mtg_linear_solve_host(
            self._h, B, fixed_vals.ctypes.data_as(dp), times.ctypes.data_as(dp),
            coeffs.ctypes.data_as(dp), cost.ctypes.data_as(dp), free.ctypes.data_as(dp),
            status.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)))
        if rc not in (0, _abi_numeric()):
            check(rc, "mtg_linear_solve_host")
        return dict(coeffs=coeffs, cost=cost, free=free, status=status)


def _abi_numeric():
    return -5  # MTG_ERR_NUMERIC: per-trajectory status carries the detail


def _require_counts(t, B):
    import torch
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise MTGError("seg_counts must be a CUDA tensor")
    if t.dtype != torch.int32:
        raise MTGError("seg_counts must be int32")
    if tuple(t.shape) != (B,):
        raise MTGError(f"seg_counts has shape {tuple(t.shape)}, expected {(B,)}")
    if not t.is_contiguous():
        raise MTGError("seg_counts must be contiguous")


class RaggedLinearPlan:
    """(N, D, r, S_max) -> batched solves of standard-pattern trajectories
    with per-trajectory segment counts in one launch (mtg_ragged_plan_create).

    Every array is a padded rectangle (include/mtg_hip.h, "Ragged batches"):
    seg_counts [B] int32, fixed_vals [B, D, nf_max], times [B, S_max]; see
    pack_ragged.  The counts stay on the device: no method reads them."""

    def __init__(self, ctx, N, D, r, S_max):
        self.N, self.D, self.r, self.S_max = N, D, r, S_max
        self._h = ctypes.c_void_p()
        check(lib().mtg_ragged_plan_create(ctx.handle, N, D, r, S_max, ctypes.byref(self._h)),
              "mtg_ragged_plan_create")
        nf, np_ = ctypes.c_int(), ctypes.c_int()
        check(lib().mtg_ragged_plan_counts(self._h, ctypes.byref(nf), ctypes.byref(np_)),
              "mtg_ragged_plan_counts")
        self.nf_max, self.np_max = nf.value, np_.value

    def close(self):
        if self._h:
            lib().mtg_ragged_plan_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _inputs(self, seg_counts, fixed_vals, times):
        B = times.shape[0]
        _require(times, (B, self.S_max), "times")
        _require(fixed_vals, (B, self.D, self.nf_max), "fixed_vals")
        _require_counts(seg_counts, B)
        return B

    def solve(self, seg_counts, fixed_vals, times, cost=True, free=False, status=True, out=None):
        """Batched solveLinear + computeCost (mtg_ragged_linear_solve).
        Returns a dict with coeffs [B, S_max, D, N] (segments >= S_b are 0.0)
        and optionally cost [B], free [B, D, np_max] (0.0 past each row's
        (S_b - 1)(N/2 - 1) entries), status [B] (int32)."""
        import torch
        B = self._inputs(seg_counts, fixed_vals, times)
        dev = times.device
        o = out or {}
        if "coeffs" not in o:
            o["coeffs"] = torch.empty((B, self.S_max, self.D, self.N), dtype=torch.float64,
                                      device=dev)
        if cost and "cost" not in o:
            o["cost"] = torch.empty(B, dtype=torch.float64, device=dev)
        if free and "free" not in o:
            o["free"] = torch.empty((B, self.D, self.np_max), dtype=torch.float64, device=dev)
        if status and "status" not in o:
            o["status"] = torch.empty(B, dtype=torch.int32, device=dev)
        _require(o["coeffs"], (B, self.S_max, self.D, self.N), "coeffs")
        check(lib().mtg_ragged_linear_solve(self._h, B, _ptr(seg_counts), _ptr(fixed_vals),
                                            _ptr(times), _ptr(o["coeffs"]), _ptr(o.get("cost")),
                                            _ptr(o.get("free")), _ptr(o.get("status")),
                                            _stream(dev)), "mtg_ragged_linear_solve")
        return o

    def coefficients(self, seg_counts, fixed_vals, free_vals, times, cost=True, status=True,
                     out=None):
        """LinearPlan.coefficients over the ragged batch in one launch
        (mtg_ragged_coeffs_from_constraints): coefficients and cost from given
        d_f and d_p, no solve.  free_vals [B, D, np_max] as solve(free=True)
        returns it (None only where S_max == 1); the padding of the inputs is
        never read.  Returns (coeffs [B, S_max, D, N] with segments >= S_b
        0.0, cost [B] or None, status [B] int32 or None); out may supply
        "coeffs", "cost" and "status".  A row whose count is outside
        [1, S_max] (status 5) or with a non-positive time (status 1) has
        coeffs and cost NaN."""
        import torch
        B = self._inputs(seg_counts, fixed_vals, times)
        if free_vals is not None or self.S_max > 1:
            _require(free_vals, (B, self.D, self.np_max), "free_vals")
        dev = times.device
        o = out or {}
        if "coeffs" in o:
            _require(o["coeffs"], (B, self.S_max, self.D, self.N), "coeffs")
        if "cost" in o:
            _require(o["cost"], (B,), "cost")
        if "status" in o:
            _require_int32(o["status"], (B,), "status")
        if "coeffs" not in o:
            o["coeffs"] = torch.empty((B, self.S_max, self.D, self.N), dtype=torch.float64,
                                      device=dev)
        if cost and "cost" not in o:
            o["cost"] = torch.empty(B, dtype=torch.float64, device=dev)
        if status and "status" not in o:
            o["status"] = torch.empty(B, dtype=torch.int32, device=dev)
        check(lib().mtg_ragged_coeffs_from_constraints(
            self._h, B, _ptr(seg_counts), _ptr(fixed_vals), _ptr(free_vals), _ptr(times),
            _ptr(o["coeffs"]), _ptr(o.get("cost")), _ptr(o.get("status")), _stream(dev)),
            "mtg_ragged_coeffs_from_constraints")
        return o["coeffs"], o.get("cost"), o.get("status")

    def time_cost(self, seg_counts, fixed_vals, times, time_penalty=500.0, grad_mode=0,
                  increment=0.1, w_d=0.1, w_t=1.0, soft=None, soft_weight=100.0, hard=False,
                  hard_tolerance=0.1):
        """objectiveFunctionTime per trajectory (mtg_ragged_time_cost); rows
        need S_b >= 2; grad [B, S_max] is 0.0 past S_b.  Soft and hard
        constraints are not supported on ragged batches (MTGError)."""
        import torch
        B = self._inputs(seg_counts, fixed_vals, times)
        dev = times.device
        cost = torch.empty(B, dtype=torch.float64, device=dev)
        grad = (torch.empty((B, self.S_max), dtype=torch.float64, device=dev)
                if grad_mode else None)
        status = torch.empty(B, dtype=torch.int32, device=dev)
        p = make_time_params(time_penalty, increment, w_d, w_t, grad_mode, soft, soft_weight,
                             hard=hard, hard_tolerance=hard_tolerance)
        check(lib().mtg_ragged_time_cost(self._h, B, _ptr(seg_counts), _ptr(fixed_vals),
                                         _ptr(times), ctypes.byref(p), _ptr(cost), _ptr(grad),
                                         _ptr(status), _stream(dev)), "mtg_ragged_time_cost")
        return dict(cost=cost, grad=grad, status=status)

    def time_optimize(self, seg_counts, fixed_vals, times, max_evals=50, time_penalty=500.0,
                      increment=0.1, w_d=0.1, w_t=1.0, soft=None, soft_weight=100.0, hard=False,
                      hard_tolerance=0.1, optimizer="fd", f_rel=0.05, f_abs=-1.0,
                      initial_stepsize_rel=0.1):
        """Optimise segment times on a copy (mtg_ragged_time_optimize); returns
        dict(times, cost, evals, solves, result, status) as
        LinearPlan.time_optimize.  times entries past S_b keep their input
        bits; a row with S_b < 2 keeps all of them."""
        import torch
        B = self._inputs(seg_counts, fixed_vals, times)
        dev = times.device
        t = times.clone()
        cost = torch.empty(B, dtype=torch.float64, device=dev)
        evals = torch.empty(B, dtype=torch.int32, device=dev)
        solves = torch.empty(B, dtype=torch.int32, device=dev)
        result = torch.empty(B, dtype=torch.int32, device=dev)
        status = torch.empty(B, dtype=torch.int32, device=dev)
        p = make_time_params(time_penalty, increment, w_d, w_t, 2, soft, soft_weight,
                             hard=hard, hard_tolerance=hard_tolerance, optimizer=optimizer,
                             f_rel=f_rel, f_abs=f_abs, initial_stepsize_rel=initial_stepsize_rel)
        check(lib().mtg_ragged_time_optimize(self._h, B, _ptr(seg_counts), _ptr(fixed_vals),
                                             _ptr(t), ctypes.byref(p), max_evals, _ptr(cost),
                                             _ptr(evals), _ptr(solves), _ptr(result),
                                             _ptr(status), _stream(dev)),
              "mtg_ragged_time_optimize")
        return dict(times=t, cost=cost, evals=evals, solves=solves, result=result,
                    status=status)


def pack_ragged(problems, N, device, S_max=None):
    """Padded inputs of RaggedLinearPlan from a list of (d_f [D, nf_b],
    times [S_b]) with nf_b = N + S_b - 1 (the order of LinearPlan.solve's
    fixed_vals).  Returns seg_counts [B] int32, fixed_vals [B, D, nf_max],
    times [B, S_max] on `device` (S_max None: the longest count).  The padding of
    both float arrays is NaN: no kernel may read it, and one that does shows."""
    import torch
    if not problems:
        raise MTGError("pack_ragged needs at least one problem")
    probs = [(np.asarray(df, dtype=np.float64), np.asarray(t, dtype=np.float64).reshape(-1))
             for df, t in problems]
    D = probs[0][0].shape[0]
    counts = np.array([t.size for _, t in probs], dtype=np.int32)
    S_max = int(counts.max()) if S_max is None else int(S_max)
    if S_max < int(counts.max()):
        raise MTGError(f"S_max = {S_max} is below the longest count {int(counts.max())}")
    fixed = np.full((len(probs), D, N + S_max - 1), np.nan)
    times = np.full((len(probs), S_max), np.nan)
    for b, (df, t) in enumerate(probs):
        if t.size < 1 or df.shape != (D, N + t.size - 1):
            raise MTGError(f"problem {b}: d_f has shape {df.shape}, expected "
                           f"{(D, N + t.size - 1)} for {t.size} segments")
        fixed[b, :, :df.shape[1]] = df
        times[b, :t.size] = t
    return (torch.from_numpy(counts).to(device), torch.from_numpy(fixed).to(device),
            torch.from_numpy(times).to(device))


def _extremum_out(B, dev):
    """The Extremum outputs of max_magnitude / ragged_max_magnitude."""
    import torch
    return {"time": torch.empty(B, dtype=torch.float64, device=dev),
            "value": torch.empty(B, dtype=torch.float64, device=dev),
            "segment": torch.empty(B, dtype=torch.int32, device=dev)}


def _sample_outputs(B, D, dev, dt, t_end, max_derivative, n_max, with_times, whole_span):
    """n_max and the (samples, sample_times or None, n_samples) tuple a sampling
    call fills and returns.  The default n_max is the sample count of the span
    t_end, or of whole_span() (the longest trajectory, read on the host) where
    t_end < 0."""
    import torch
    if not dt > 0:
        raise MTGError("dt must be > 0")
    if n_max is None:
        span = float(whole_span()) if t_end < 0 else t_end
        n_max = int(span / dt) + 2
        n_max = (n_max + 63) // 64 * 64  # 512-byte aligned channel rows
    nch = (max_derivative + 1) * D
    samples = torch.empty((B, nch, n_max), dtype=torch.float64, device=dev)
    stimes = torch.empty((B, n_max), dtype=torch.float64, device=dev) if with_times else None
    count = torch.empty(B, dtype=torch.int32, device=dev)
    return n_max, (samples, stimes, count)


def _ragged_eval_inputs(seg_counts, coeffs, times):
    import torch
    if not isinstance(coeffs, torch.Tensor) or coeffs.dim() != 4:
        raise MTGError("coeffs must be a CUDA tensor [B, S_max, D, N]")
    B, S_max, D, N = coeffs.shape
    _require(coeffs, (B, S_max, D, N), "coeffs")
    _require(times, (B, S_max), "times")
    _require_counts(seg_counts, B)
    return B, S_max, D, N


def ragged_max_magnitude(seg_counts, coeffs, times, derivative, out=None):
    """max_magnitude over a ragged batch in one launch
    (mtg_ragged_max_magnitude): row b is the Extremum of |p^(derivative)| over
    coeffs[b, :S_b], times[b, :S_b], S_b = seg_counts[b].

    seg_counts [B] int32, coeffs [B, S_max, D, N], times [B, S_max] (CUDA), as
    RaggedLinearPlan.solve and pack_ragged give them; the padding is never
    read.  Returns a dict of time [B], value [B], segment [B] int32.  A row
    whose count is outside [1, S_max] gets NaN, NaN, -1.  The counts stay on
    the device."""
    import torch
    B, S_max, D, N = _ragged_eval_inputs(seg_counts, coeffs, times)
    dev = times.device
    if out is None:
        out = _extremum_out(B, dev)
    check(lib().mtg_ragged_max_magnitude(N, D, S_max, B, _ptr(seg_counts), _ptr(coeffs),
                                         _ptr(times), derivative, _ptr(out["time"]),
                                         _ptr(out["value"]), _ptr(out["segment"]), _stream(dev)),
          "mtg_ragged_max_magnitude")
    return out


def ragged_soft_constraint_cost(seg_counts, coeffs, times, derivatives, limits, weight=100.0,
                                maximum_cost=1.0e12, gate=None, out=None):
    """soft_constraint_cost over a ragged batch in one launch
    (mtg_ragged_soft_constraint_cost), inputs as ragged_max_magnitude.

    Returns a dict of cost [B] and maxima [B, n_constraints]; with gate [B]
    (typically the solve's cost) also gated [B]: gate[b] where every
    maxima[b, c] <= limits[c], +inf elsewhere (a NaN gate passes through), so
    a selection over gated picks the cheapest feasible row.  out["gated"] may
    be gate itself.  A row whose count is outside [1, S_max] gets NaN cost and
    maxima and gated +inf."""
    import torch
    B, S_max, D, N = _ragged_eval_inputs(seg_counts, coeffs, times)
    nc = len(derivatives)
    if len(limits) != nc:
        raise MTGError("derivatives and limits differ in length")
    if gate is not None:
        _require(gate, (B,), "gate")
    dev = times.device
    out = dict(out) if out is not None else {}
    if "cost" not in out:
        out["cost"] = torch.empty(B, dtype=torch.float64, device=dev)
    if "maxima" not in out:
        out["maxima"] = torch.empty((B, nc), dtype=torch.float64, device=dev)
    _require(out["cost"], (B,), "cost")
    _require(out["maxima"], (B, nc), "maxima")
    if gate is not None:
        if "gated" not in out:
            out["gated"] = torch.empty(B, dtype=torch.float64, device=dev)
        _require(out["gated"], (B,), "gated")
    der = (ctypes.c_int * max(nc, 1))(*[int(d) for d in derivatives])
    lim = (ctypes.c_double * max(nc, 1))(*[float(v) for v in limits])
    check(lib().mtg_ragged_soft_constraint_cost(
        N, D, S_max, B, _ptr(seg_counts), _ptr(coeffs), _ptr(times), nc, der, lim, float(weight),
        float(maximum_cost), _ptr(out["maxima"]), _ptr(out["cost"]), _ptr(gate),
        _ptr(out["gated"] if gate is not None else None), _stream(dev)),
        "mtg_ragged_soft_constraint_cost")
    return out


def ragged_collision_cost(seg_counts, coeffs, times, occupancy, params, near_field=None,
                          grad=False, gate=None, out=None):
    """LinearPlan.collision_cost over a ragged batch in one launch
    (mtg_ragged_collision_cost), inputs as ragged_max_magnitude with D = 3;
    occupancy float32 CUDA tensor [nz, ny, nx] (occupied iff >= 0), params
    from make_collision_params, near_field from coll_field(occupancy, params)
    (None: every evaluated sample's box is scanned; the results are the same
    bit for bit).

    Returns a dict of cost [B], collision [B] int32 (0 / 1), hit_segment [B]
    int32 and hit_time [B]: the first colliding sample's segment and its t
    within that segment (-1 and NaN on a free row); with grad also grad_coeffs
    [B, S_max, 3, N] (0.0 past each row's count); with gate [B] (typically the
    solve's cost, or ragged_soft_constraint_cost's gated) also gated [B]:
    gate[b] on a collision-free row, +inf elsewhere (a NaN gate passes
    through).  out["gated"] may be gate itself.  A row whose count is outside
    [1, S_max] gets cost NaN, collision -1, hit_segment -1, hit_time NaN,
    grad_coeffs NaN and gated +inf.  The counts stay on the device."""
    import torch
    B, S_max, D, N = _ragged_eval_inputs(seg_counts, coeffs, times)
    if D != 3:
        raise MTGError(f"coeffs has D = {D}; the collision walk needs D = 3")
    if not (isinstance(occupancy, torch.Tensor) and occupancy.is_cuda and
            occupancy.dtype == torch.float32 and occupancy.dim() == 3 and
            occupancy.is_contiguous()):
        raise MTGError("occupancy must be a contiguous float32 CUDA tensor [nz, ny, nx]")
    _check_field(near_field, occupancy)
    if gate is not None:
        _require(gate, (B,), "gate")
    nz, ny, nx = occupancy.shape
    dev = times.device
    out = dict(out) if out is not None else {}
    for key in ("cost", "hit_time"):
        if key not in out:
            out[key] = torch.empty(B, dtype=torch.float64, device=dev)
        _require(out[key], (B,), key)
    for key in ("collision", "hit_segment"):
        if key not in out:
            out[key] = torch.empty(B, dtype=torch.int32, device=dev)
        if not (isinstance(out[key], torch.Tensor) and out[key].is_cuda and
                out[key].dtype == torch.int32 and tuple(out[key].shape) == (B,) and
                out[key].is_contiguous()):
            raise MTGError(f"{key} must be a contiguous int32 CUDA tensor of shape {(B,)}")
    if grad:
        if "grad_coeffs" not in out:
            out["grad_coeffs"] = torch.empty((B, S_max, D, N), dtype=torch.float64, device=dev)
        _require(out["grad_coeffs"], (B, S_max, D, N), "grad_coeffs")
    if gate is not None:
        if "gated" not in out:
            out["gated"] = torch.empty(B, dtype=torch.float64, device=dev)
        _require(out["gated"], (B,), "gated")
    check(lib().mtg_ragged_collision_cost(
        N, S_max, B, _ptr(seg_counts), _ptr(coeffs), _ptr(times), _ptr(occupancy), nx, ny, nz,
        _ptr(near_field), ctypes.byref(params), _ptr(out["cost"]), _ptr(out["collision"]),
        _ptr(out["hit_segment"]), _ptr(out["hit_time"]),
        _ptr(out["grad_coeffs"] if grad else None), _ptr(gate),
        _ptr(out["gated"] if gate is not None else None), _stream(dev)),
        "mtg_ragged_collision_cost")
    return out


def ragged_sample_trajectories(seg_counts, coeffs, times, dt, t_start=0.0, t_end=-1.0,
                               max_derivative=0, n_max=None, with_times=True):
    """sample_trajectories over a ragged batch in one launch
    (mtg_ragged_sample_trajectories), inputs as ragged_max_magnitude; t_end < 0
    means each row's own total time.

    Returns (samples [B, (max_derivative+1)*D, n_max] channel-major,
    sample_times [B, n_max] or None, n_samples [B] int32).  A row whose count
    is outside [1, S_max] gets n_samples -1 and no samples.

    The default n_max is the longest row's sample count, from the row sums of
    times masked by the counts: that default is the one place a ragged call
    reads the counts on the host (a device-to-host copy and a
    synchronisation).  Pass n_max to keep the call free of host reads, e.g.
    under graph capture."""
    import torch
    B, S_max, D, N = _ragged_eval_inputs(seg_counts, coeffs, times)
    dev = times.device

    def longest_row():
        mask = torch.arange(S_max, device=dev)[None, :] < seg_counts[:, None]
        return torch.where(mask, times, torch.zeros_like(times)).sum(dim=1).max().item()

    n_max, res = _sample_outputs(B, D, dev, dt, t_end, max_derivative, n_max, with_times,
                                 longest_row)
    check(lib().mtg_ragged_sample_trajectories(N, D, S_max, B, _ptr(seg_counts), _ptr(coeffs),
                                               _ptr(times), t_start, t_end, dt, n_max,
                                               max_derivative, *map(_ptr, res), _stream(dev)),
          "mtg_ragged_sample_trajectories")
    return res


def segment_matrices(ctx, N, r, times):
    """Q, A, A^-1, H for each time in a CUDA float64 tensor [n] -> 4 x [n, N, N]."""
    import torch
    n = times.shape[0]
    _require(times, (n,), "times")
    outs = [torch.empty((n, N, N), dtype=torch.float64, device=times.device) for _ in range(4)]
    check(lib().mtg_segment_matrices(ctx.handle, N, r, n, _ptr(times), *[_ptr(o) for o in outs],
                                     _stream(times.device)), "mtg_segment_matrices")
    return outs


def generate_random_problems(N, D, S, B, seed0=105, pos_bound=10.0, v_max=3.0, a_max=5.0):
    """Standard-pattern batch (host): mask [(S+1), N/2], fixed_vals [B, D, n_f],
    times [B, S], positions [B, S+1, D] — createRandomVertices(seed0 + b) +
    estimateSegmentTimes, bit-identical to the reference generator."""
    M = N // 2
    nf = 2 * M + (S - 1)
    mask = np.zeros((S + 1, M), np.uint8)
    fixed = np.zeros((B, D, nf))
    times = np.zeros((B, S))
    pos = np.zeros((B, S + 1, D))
    dp = ctypes.POINTER(ctypes.c_double)
    check(lib().mtg_generate_random_problems(
        N, D, S, B, seed0, pos_bound, v_max, a_max,
        mask.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), fixed.ctypes.data_as(dp),
        times.ctypes.data_as(dp), pos.ctypes.data_as(dp)), "mtg_generate_random_problems")
    return mask, fixed, times, pos


def tube_num_constraints(N, S):
    return lib().mtg_tube_num_constraints(N, S)


def tube_residuals(ctx, N, r, positions, fixed_vals, times_cp, times, radii, x):
    import torch
    B, S = times.shape
    m = tube_num_constraints(N, S)
    resid = torch.empty((B, m), dtype=torch.float64, device=times.device)
    check(lib().mtg_tube_residuals(ctx.handle, N, r, S, B, _ptr(positions), _ptr(fixed_vals),
                                   _ptr(times_cp), _ptr(times), _ptr(radii), _ptr(x),
                                   _ptr(resid), _stream(times.device)), "mtg_tube_residuals")
    return resid


def tube_solve(ctx, N, r, positions, fixed_vals, times_cp, times, radii, tol=1e-10,
               max_iter=100):
    import torch
    B, S = times.shape
    dev = times.device
    for name, t, shp in (("positions", positions, (B, S + 1, 3)),
                         ("fixed_vals", fixed_vals, (B, 3, N)),
                         ("times_cp", times_cp, (B, S)), ("radii", radii, (B, S, 2))):
        _require(t, shp, name)
    n = 3 * (S - 1) * (N // 2)
    x = torch.empty((B, n), dtype=torch.float64, device=dev)
    coeffs = torch.empty((B, S, 3, N), dtype=torch.float64, device=dev)
    cost = torch.empty(B, dtype=torch.float64, device=dev)
    iters = torch.empty(B, dtype=torch.int32, device=dev)
    status = torch.empty(B, dtype=torch.int32, device=dev)
    check(lib().mtg_tube_solve(ctx.handle, N, r, S, B, _ptr(positions), _ptr(fixed_vals),
                               _ptr(times_cp), _ptr(times), _ptr(radii), tol, max_iter, _ptr(x),
                               _ptr(coeffs), _ptr(cost), _ptr(iters), _ptr(status),
                               _stream(dev)), "mtg_tube_solve")
    return dict(x=x, coeffs=coeffs, cost=cost, iters=iters, status=status)


def _require_int32(t, shape, name):
    import torch
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise MTGError(f"{name} must be a CUDA tensor")
    if t.dtype != torch.int32:
        raise MTGError(f"{name} must be int32")
    if tuple(t.shape) != tuple(shape):
        raise MTGError(f"{name} has shape {tuple(t.shape)}, expected {tuple(shape)}")
    if not t.is_contiguous():
        raise MTGError(f"{name} must be contiguous")


def _ragged_tube_inputs(N, seg_counts, positions, fixed_vals, times_cp, times, radii):
    import torch
    if not isinstance(times, torch.Tensor) or times.dim() != 2:
        raise MTGError("times must be a CUDA tensor [B, S_max]")
    B, S_max = times.shape
    for name, t, shp in (("times", times, (B, S_max)), ("times_cp", times_cp, (B, S_max)),
                         ("positions", positions, (B, S_max + 1, 3)),
                         ("fixed_vals", fixed_vals, (B, 3, N)),
                         ("radii", radii, (B, S_max, 2))):
        _require(t, shp, name)
    _require_counts(seg_counts, B)
    return B, S_max


def ragged_tube_num_constraints(N, S_max):
    return lib().mtg_ragged_tube_num_constraints(N, S_max)


def ragged_tube_residuals(ctx, N, r, seg_counts, positions, fixed_vals, times_cp, times, radii,
                          x):
    """tube_residuals over a ragged batch in one launch
    (mtg_ragged_tube_residuals): row b holds the residuals of the tube problem
    of its first S_b = seg_counts[b] segments at x[b].

    seg_counts [B] int32, positions [B, S_max + 1, 3], fixed_vals [B, 3, N],
    times_cp and times [B, S_max], radii [B, S_max, 2], x [B, 3, (S_max - 1) M]
    (CUDA), as pack_ragged_tube and ragged_tube_solve give them; the padding
    is never read.  Returns resid [B, n_con(S_max)]: the row's n_con(S_b)
    residuals, then -inf.  A row whose count is outside [2, S_max] or with a
    non-positive time is NaN.  The counts stay on the device."""
    import torch
    B, S_max = _ragged_tube_inputs(N, seg_counts, positions, fixed_vals, times_cp, times, radii)
    _require(x, (B, 3, (S_max - 1) * (N // 2)), "x")
    dev = times.device
    m = max(ragged_tube_num_constraints(N, S_max), 0)
    resid = torch.empty((B, m), dtype=torch.float64, device=dev)
    check(lib().mtg_ragged_tube_residuals(
        ctx.handle, N, r, S_max, B, _ptr(seg_counts), _ptr(positions), _ptr(fixed_vals),
        _ptr(times_cp), _ptr(times), _ptr(radii), _ptr(x), _ptr(resid), _stream(dev)),
        "mtg_ragged_tube_residuals")
    return resid


def ragged_tube_solve(ctx, N, r, seg_counts, positions, fixed_vals, times_cp, times, radii,
                      tol=1e-10, max_iter=100, order=True, out=None):
    """tube_solve over a ragged batch in one launch (mtg_ragged_tube_solve):
    row b is the tube QCQP of its first S_b = seg_counts[b] segments,
    2 <= S_b <= S_max.  Inputs as ragged_tube_residuals.

    Returns a dict of x [B, 3, (S_max - 1) M] (row d: (S_b - 1) M values, then
    0.0), coeffs [B, S_max, 3, N] (segments >= S_b are 0.0: what the ragged
    evaluators read), cost [B], iters [B] int32, status [B] int32; out may
    supply any of them.  order=True sorts the rows by count on the device and
    dispatches the longest first (the permutation is returned as order [B]
    int32); the results do not depend on it.  A row whose count is out of
    range (status 5) or with a non-positive time (status 1) has x, coeffs and
    cost NaN and iters 0.  The counts stay on the device: a captured call may
    be replayed over other counts."""
    import torch
    B, S_max = _ragged_tube_inputs(N, seg_counts, positions, fixed_vals, times_cp, times, radii)
    dev = times.device
    M = N // 2
    out = dict(out) if out is not None else {}
    shapes = {"x": (B, 3, (S_max - 1) * M), "coeffs": (B, S_max, 3, N), "cost": (B,)}
    ints = ("iters", "status") + (("order",) if order else ())
    for name, shp in shapes.items():  # the caller's outputs first, then the missing ones
        if name in out:
            _require(out[name], shp, name)
    for name in ints:
        if name in out:
            _require_int32(out[name], (B,), name)
    for name, shp in shapes.items():
        if name not in out:
            out[name] = torch.empty(shp, dtype=torch.float64, device=dev)
    for name in ints:
        if name not in out:
            out[name] = torch.empty(B, dtype=torch.int32, device=dev)
    check(lib().mtg_ragged_tube_solve(
        ctx.handle, N, r, S_max, B, _ptr(seg_counts), _ptr(positions), _ptr(fixed_vals),
        _ptr(times_cp), _ptr(times), _ptr(radii), float(tol), int(max_iter), _ptr(out["x"]),
        _ptr(out["coeffs"]), _ptr(out["cost"]), _ptr(out["iters"]), _ptr(out["status"]),
        _ptr(out["order"] if order else None), _stream(dev)), "mtg_ragged_tube_solve")
    return out


def pack_ragged_tube(problems, N, device, S_max=None):
    """Padded inputs of ragged_tube_solve from a list of (positions
    [S_b + 1, 3], fixed_vals [3, N], times [S_b], radii [S_b, 2]).  Returns
    seg_counts [B] int32, positions [B, S_max + 1, 3], fixed_vals [B, 3, N],
    times [B, S_max], radii [B, S_max, 2] on `device` (S_max None: the longest
    count).  The padding of the float arrays is NaN: no kernel may read it,
    and one that does shows."""
    import torch
    if not problems:
        raise MTGError("pack_ragged_tube needs at least one problem")
    probs = [(np.asarray(p, dtype=np.float64), np.asarray(f, dtype=np.float64),
              np.asarray(t, dtype=np.float64).reshape(-1), np.asarray(rd, dtype=np.float64))
             for p, f, t, rd in problems]
    counts = np.array([t.size for _, _, t, _ in probs], dtype=np.int32)
    S_max = int(counts.max()) if S_max is None else int(S_max)
    if S_max < int(counts.max()):
        raise MTGError(f"S_max = {S_max} is below the longest count {int(counts.max())}")
    B = len(probs)
    pos = np.full((B, S_max + 1, 3), np.nan)
    fixed = np.full((B, 3, N), np.nan)
    times = np.full((B, S_max), np.nan)
    radii = np.full((B, S_max, 2), np.nan)
    for b, (p, f, t, rd) in enumerate(probs):
        S = t.size
        if S < 2:
            raise MTGError(f"problem {b}: a tube problem needs at least 2 segments, got {S}")
        if p.shape != (S + 1, 3) or f.shape != (3, N) or rd.shape != (S, 2):
            raise MTGError(f"problem {b}: shapes {p.shape}, {f.shape}, {rd.shape}, expected "
                           f"{(S + 1, 3)}, {(3, N)}, {(S, 2)} for {S} segments")
        pos[b, :S + 1] = p
        fixed[b] = f
        times[b, :S] = t
        radii[b, :S] = rd
    return (torch.from_numpy(counts).to(device), torch.from_numpy(pos).to(device),
            torch.from_numpy(fixed).to(device), torch.from_numpy(times).to(device),
            torch.from_numpy(radii).to(device))


def _tube_geometry(N, positions, fixed_vals, radii, B, S):
    for name, t, shp in (("positions", positions, (B, S + 1, 3)),
                         ("fixed_vals", fixed_vals, (B, 3, N)), ("radii", radii, (B, S, 2))):
        _require(t, shp, name)


def tube_time_workspace_bytes(N, S, B, params, optimize):
    """Device scratch the QCQP time objective / optimiser needs
    (mtg_tube_time_workspace_bytes)."""
    n = lib().mtg_tube_time_workspace_bytes(N, S, B, ctypes.byref(params), 1 if optimize else 0)
    if n < 0:
        check(int(n), "mtg_tube_time_workspace_bytes")
    return int(n)


def _workspace(workspace, nbytes, dev):
    import torch
    if workspace is None:
        return torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    if not isinstance(workspace, torch.Tensor) or not workspace.is_cuda or \
            not workspace.is_contiguous() or workspace.numel() * workspace.element_size() < nbytes:
        raise MTGError(f"workspace must be a contiguous CUDA tensor of >= {nbytes} bytes")
    return workspace


def tube_time_cost(ctx, N, r, positions, fixed_vals, times_cp, times, radii, time_penalty=500.0,
                   grad=False, increment=0.1, soft=None, soft_weight=100.0, tol=1e-10,
                   max_iter=100, workspace=None):
    """objectiveFunctionTime with the QCQP inner solve (mtg_tube_time_cost):
    J = computeCost() of the tube QCQP at `times` + time_penalty (sum T)^2
    [+ soft]; grad=True adds the central-difference gradient (grad_mode 2).
    workspace: optional device tensor of >= tube_time_workspace_bytes bytes
    (allocated from torch's caching allocator when None).
    Returns dict(cost [B], grad [B, S] or None, status [B])."""
    import torch
    B, S = times.shape
    dev = times.device
    _tube_geometry(N, positions, fixed_vals, radii, B, S)
    _require(times_cp, (B, S), "times_cp")
    _require(times, (B, S), "times")
    p = make_time_params(time_penalty, increment, 0.1, 1.0, 2 if grad else 0, soft, soft_weight)
    cost = torch.empty(B, dtype=torch.float64, device=dev)
    g = torch.empty((B, S), dtype=torch.float64, device=dev) if grad else None
    status = torch.empty(B, dtype=torch.int32, device=dev)
    nbytes = tube_time_workspace_bytes(N, S, B, p, False)
    ws = _workspace(workspace, nbytes, dev)
    check(lib().mtg_tube_time_cost(ctx.handle, N, r, S, B, _ptr(positions), _ptr(fixed_vals),
                                   _ptr(times_cp), _ptr(times), _ptr(radii), tol, max_iter,
                                   ctypes.byref(p), _ptr(cost), _ptr(g), _ptr(status), _ptr(ws),
                                   ws.numel() * ws.element_size(), _stream(dev)),
          "mtg_tube_time_cost")
    return dict(cost=cost, grad=g, status=status)


def tube_time_optimize(ctx, N, r, positions, fixed_vals, radii, times, max_evals,
                       time_penalty=500.0, increment=0.1, soft=None, soft_weight=100.0,
                       tol=1e-10, max_iter=100, workspace=None, optimizer="fd", f_rel=0.05,
                       f_abs=-1.0, initial_stepsize_rel=0.1):
    """optimizeTime in the fork's QCQP form (mtg_tube_time_optimize_ex).  times
    [B, S] are the initial times (and the control-point times).  optimizer
    "sbplx" runs LN_SBPLX, the reference's default (one QCQP per evaluation,
    f_rel / f_abs / initial_stepsize_rel as NonlinearOptimizationParameters);
    "fd" the projected central-difference descent.  Returns dict(times, cost,
    evals, result, status) with new tensors; result is the nlopt_result code."""
    import torch
    B, S = times.shape
    dev = times.device
    _tube_geometry(N, positions, fixed_vals, radii, B, S)
    _require(times, (B, S), "times")
    p = make_time_params(time_penalty, increment, 0.1, 1.0, 2, soft, soft_weight,
                         optimizer=optimizer, f_rel=f_rel, f_abs=f_abs,
                         initial_stepsize_rel=initial_stepsize_rel)
    t = times.clone()
    cost = torch.empty(B, dtype=torch.float64, device=dev)
    evals = torch.empty(B, dtype=torch.int32, device=dev)
    result = torch.empty(B, dtype=torch.int32, device=dev)
    status = torch.empty(B, dtype=torch.int32, device=dev)
    nbytes = tube_time_workspace_bytes(N, S, B, p, True)
    ws = _workspace(workspace, nbytes, dev)
    check(lib().mtg_tube_time_optimize_ex(ctx.handle, N, r, S, B, _ptr(positions),
                                          _ptr(fixed_vals), _ptr(radii), _ptr(t), tol, max_iter,
                                          ctypes.byref(p), max_evals, _ptr(cost), _ptr(evals),
                                          _ptr(result), _ptr(status), _ptr(ws),
                                          ws.numel() * ws.element_size(), _stream(dev)),
          "mtg_tube_time_optimize_ex")
    return dict(times=t, cost=cost, evals=evals, result=result, status=status)


def ragged_tube_time_workspace_bytes(N, S_max, B, params, optimize):
    """Device scratch the ragged QCQP time objective / optimiser needs
    (mtg_ragged_tube_time_workspace_bytes)."""
    n = lib().mtg_ragged_tube_time_workspace_bytes(N, S_max, B, ctypes.byref(params),
                                                   1 if optimize else 0)
    if n < 0:
        check(int(n), "mtg_ragged_tube_time_workspace_bytes")
    return int(n)


def ragged_tube_time_cost(ctx, N, r, seg_counts, positions, fixed_vals, times_cp, times, radii,
                          time_penalty=500.0, grad=False, increment=0.1, soft=None,
                          soft_weight=100.0, tol=1e-10, max_iter=100, workspace=None):
    """tube_time_cost over a ragged batch in one call (mtg_ragged_tube_time_cost):
    row b is the objective of its first S_b = seg_counts[b] segments.  Inputs
    as pack_ragged_tube gives them (times_cp and times [B, S_max]; the padding
    is never read); keywords as tube_time_cost.  Returns dict(cost [B], grad
    [B, S_max] or None, status [B]); grad[b, S_b:] is 0.0.  A row whose count
    is outside [2, S_max] has status 5, cost NaN and its grad row NaN.  The
    counts stay on the device."""
    import torch
    B, S_max = _ragged_tube_inputs(N, seg_counts, positions, fixed_vals, times_cp, times, radii)
    dev = times.device
    p = make_time_params(time_penalty, increment, 0.1, 1.0, 2 if grad else 0, soft, soft_weight)
    cost = torch.empty(B, dtype=torch.float64, device=dev)
    g = torch.empty((B, S_max), dtype=torch.float64, device=dev) if grad else None
    status = torch.empty(B, dtype=torch.int32, device=dev)
    nbytes = ragged_tube_time_workspace_bytes(N, S_max, B, p, False)
    ws = _workspace(workspace, nbytes, dev)
    check(lib().mtg_ragged_tube_time_cost(
        ctx.handle, N, r, S_max, B, _ptr(seg_counts), _ptr(positions), _ptr(fixed_vals),
        _ptr(times_cp), _ptr(times), _ptr(radii), tol, max_iter, ctypes.byref(p), _ptr(cost),
        _ptr(g), _ptr(status), _ptr(ws), ws.numel() * ws.element_size(), _stream(dev)),
        "mtg_ragged_tube_time_cost")
    return dict(cost=cost, grad=g, status=status)


def ragged_tube_time_optimize(ctx, N, r, seg_counts, positions, fixed_vals, radii, times,
                              max_evals, time_penalty=500.0, increment=0.1, soft=None,
                              soft_weight=100.0, tol=1e-10, max_iter=100, workspace=None,
                              optimizer="sbplx", f_rel=0.05, f_abs=-1.0,
                              initial_stepsize_rel=0.1):
    """tube_time_optimize(optimizer="sbplx") over a ragged batch in one call
    (mtg_ragged_tube_time_optimize): row b runs LN_SBPLX over its first S_b
    times.  times [B, S_max] are the initial times (and the control-point
    times); inputs as pack_ragged_tube gives them, keywords as
    tube_time_optimize.  Returns dict(times, cost, evals, result, status) with
    new tensors; times[b, S_b:] keeps the input's bits.  A row whose count is
    outside [2, S_max] has status 5, cost NaN, evals 0, result -1 and its
    times unchanged.  optimizer="fd" is not available for ragged batches (the
    call fails with MTG_ERR_UNSUPPORTED)."""
    import torch
    B, S_max = _ragged_tube_inputs(N, seg_counts, positions, fixed_vals, times, times, radii)
    dev = times.device
    p = make_time_params(time_penalty, increment, 0.1, 1.0, 2, soft, soft_weight,
                         optimizer=optimizer, f_rel=f_rel, f_abs=f_abs,
                         initial_stepsize_rel=initial_stepsize_rel)
    nbytes = ragged_tube_time_workspace_bytes(N, S_max, B, p, True)
    t = times.clone()
    cost = torch.empty(B, dtype=torch.float64, device=dev)
    evals = torch.empty(B, dtype=torch.int32, device=dev)
    result = torch.empty(B, dtype=torch.int32, device=dev)
    status = torch.empty(B, dtype=torch.int32, device=dev)
    ws = _workspace(workspace, nbytes, dev)
    check(lib().mtg_ragged_tube_time_optimize(
        ctx.handle, N, r, S_max, B, _ptr(seg_counts), _ptr(positions), _ptr(fixed_vals),
        _ptr(radii), _ptr(t), tol, max_iter, ctypes.byref(p), max_evals, _ptr(cost),
        _ptr(evals), _ptr(result), _ptr(status), _ptr(ws), ws.numel() * ws.element_size(),
        _stream(dev)), "mtg_ragged_tube_time_optimize")
    return dict(times=t, cost=cost, evals=evals, result=result, status=status)


def ragged_coll_workspace_bytes(N, S_max, B, params, mode=0, optimize=False):
    """Device scratch the ragged collision objective / optimiser needs
    (mtg_ragged_coll_workspace_bytes)."""
    n = lib().mtg_ragged_coll_workspace_bytes(N, S_max, B, mode, ctypes.byref(params),
                                              1 if optimize else 0)
    if n < 0:
        check(int(n), "mtg_ragged_coll_workspace_bytes")
    return int(n)


def _ragged_coll_inputs(N, seg_counts, fixed_vals, x, times, occupancy, mode, S_max):
    """Shapes of the ragged collision entries.  Mode 0: x [B, 3, np_max] (as
    ragged_tube_solve's x) and times [B, S_max]; mode 1: x [B, S_max +
    3 np_max] and S_max given (times is not read)."""
    import torch
    M = N // 2
    if mode == 0:
        if not isinstance(times, torch.Tensor) or times.dim() != 2:
            raise MTGError("times must be a CUDA tensor [B, S_max]")
        B, S_max = times.shape
        _require(times, (B, S_max), "times")
        _require(x, (B, 3, (S_max - 1) * M), "x")
    else:
        if S_max is None:
            raise MTGError("mode 1 needs S_max")
        if not isinstance(x, torch.Tensor) or x.dim() != 2:
            raise MTGError("x must be a CUDA tensor [B, S_max + 3 (S_max - 1) M]")
        B = x.shape[0]
        _require(x, (B, S_max + 3 * (S_max - 1) * M), "x")
    _require(fixed_vals, (B, 3, N), "fixed_vals")
    _require_counts(seg_counts, B)
    if not (isinstance(occupancy, torch.Tensor) and occupancy.is_cuda and
            occupancy.dtype == torch.float32 and occupancy.dim() == 3 and
            occupancy.is_contiguous()):
        raise MTGError("occupancy must be a contiguous float32 CUDA tensor [nz, ny, nx]")
    return B, int(S_max)


def ragged_coll_cost(ctx, N, r, seg_counts, fixed_vals, x, times, occupancy, params, mode=0,
                     raise_ref=None, grad=True, workspace=None, near_field=None, S_max=None):
    """LinearPlan.coll_cost over a ragged batch of the tube pattern in one call
    (mtg_ragged_coll_cost): row b is the objective of its first S_b =
    seg_counts[b] segments, 2 <= S_b <= S_max.

    seg_counts [B] int32, fixed_vals [B, 3, N] (CUDA).  Mode 0: x [B, 3,
    (S_max - 1) M], exactly ragged_tube_solve's x, and times [B, S_max]; mode
    1: x [B, S_max + 3 (S_max - 1) M] (S_max times, then the mode-0 block),
    times unused and S_max given.  The padding is never read.  Returns
    dict(cost, grad (shaped as x; padding 0.0), terms [B, 4], collision,
    status).  A row whose count is out of range has status 5, cost, terms and
    its whole grad row NaN and collision -1.  The counts stay on the device."""
    import torch
    B, S_max = _ragged_coll_inputs(N, seg_counts, fixed_vals, x, times, occupancy, mode, S_max)
    _check_field(near_field, occupancy)
    if raise_ref is not None:
        _require(raise_ref, (B,), "raise_ref")
    dev = x.device
    nz, ny, nx = occupancy.shape
    cost = torch.empty(B, dtype=torch.float64, device=dev)
    g = torch.empty(x.shape, dtype=torch.float64, device=dev) if grad else None
    terms = torch.empty((B, 4), dtype=torch.float64, device=dev)
    coll = torch.empty(B, dtype=torch.int32, device=dev)
    st = torch.empty(B, dtype=torch.int32, device=dev)
    nb = ragged_coll_workspace_bytes(N, S_max, B, params, mode, False)
    ws = _workspace(workspace, nb, dev)
    check(lib().mtg_ragged_coll_cost(
        ctx.handle, N, r, S_max, B, mode, _ptr(seg_counts), _ptr(fixed_vals), _ptr(x),
        _ptr(times) if mode == 0 else None, _ptr(occupancy), nx, ny, nz, _ptr(near_field),
        ctypes.byref(params), _ptr(raise_ref), _ptr(cost), _ptr(g), _ptr(terms), _ptr(coll),
        _ptr(st), _ptr(ws), ws.numel() * ws.element_size(), _stream(dev)),
        "mtg_ragged_coll_cost")
    return dict(cost=cost, grad=g, terms=terms, collision=coll, status=st)


def ragged_coll_optimize(ctx, N, r, seg_counts, fixed_vals, x0, times, occupancy, params, mode=0,
                         max_evals=25, lower=None, upper=None, initial_step=None,
                         workspace=None, near_field=None, history=False, S_max=None):
    """LinearPlan.coll_optimize over a ragged batch of the tube pattern in one
    call (mtg_ragged_coll_optimize): row b runs the projected L-BFGS over the
    variables of its first S_b segments.  Inputs as ragged_coll_cost; lower,
    upper and initial_step are shaped as x0.  Returns dict(x, cost, evals,
    result, status, terms) with new tensors (the padding of x keeps x0's
    bits); with history=True also x_history [B, max_evals, nv_max], each row
    laid out as x0 flattened (the padding of a written row is 0.0, rows past
    evals are unset).  A row whose count is out of range has status 5, cost
    NaN, evals 0, result -1 and its x unchanged."""
    import torch
    B, S_max = _ragged_coll_inputs(N, seg_counts, fixed_vals, x0, times, occupancy, mode, S_max)
    _check_field(near_field, occupancy)
    for a, name in ((lower, "lower"), (upper, "upper"), (initial_step, "initial_step")):
        if a is not None:
            _require(a, tuple(x0.shape), name)
    dev = x0.device
    nv = x0[0].numel() if B else S_max * (mode != 0) + 3 * (S_max - 1) * (N // 2)
    nz, ny, nx = occupancy.shape
    x = x0.clone()
    cost = torch.empty(B, dtype=torch.float64, device=dev)
    ev = torch.empty(B, dtype=torch.int32, device=dev)
    res = torch.empty(B, dtype=torch.int32, device=dev)
    st = torch.empty(B, dtype=torch.int32, device=dev)
    terms = torch.empty((B, 4), dtype=torch.float64, device=dev)
    nb = ragged_coll_workspace_bytes(N, S_max, B, params, mode, True)
    ws = _workspace(workspace, nb, dev)
    hist = (torch.full((B, max_evals, nv), float("nan"), dtype=torch.float64, device=dev)
            if history else None)
    check(lib().mtg_ragged_coll_optimize(
        ctx.handle, N, r, S_max, B, mode, _ptr(seg_counts), _ptr(fixed_vals), _ptr(x),
        _ptr(times) if mode == 0 else None, _ptr(lower), _ptr(upper), _ptr(initial_step),
        _ptr(occupancy), nx, ny, nz, _ptr(near_field), ctypes.byref(params), max_evals,
        _ptr(cost), _ptr(ev), _ptr(res), _ptr(st), _ptr(terms), _ptr(hist), _ptr(ws),
        ws.numel() * ws.element_size(), _stream(dev)), "mtg_ragged_coll_optimize")
    out = dict(x=x, cost=cost, evals=ev, result=res, status=st, terms=terms)
    if history:
        out["x_history"] = hist
    return out


def ragged_tube_coefficients(ctx, N, r, seg_counts, fixed_vals, x, times=None, mode=0,
                             S_max=None, out=None):
    """Coefficients and cost of a ragged batch of the tube pattern from its
    free derivatives in one launch (mtg_ragged_tube_coeffs): what
    LinearPlan.coefficients gives per count, for row b over its first S_b =
    seg_counts[b] segments, 2 <= S_b <= S_max.

    seg_counts [B] int32, fixed_vals [B, D, N] (CUDA).  Mode 0: x [B, D,
    (S_max - 1) M], as ragged_tube_solve and ragged_coll_optimize return it,
    and times [B, S_max]; mode 1: x [B, S_max + D (S_max - 1) M], as
    ragged_coll_optimize(mode=1) returns it, and times None.  S_max is taken
    from the shapes (given, it must agree with them).  The padding is never
    read.  Returns dict(coeffs [B, S_max, D, N] with segments >= S_b 0.0,
    cost [B], status [B] int32) and in mode 1 also times [B, S_max]: each
    row's S_b times, then 0.0; out may supply any of them (a "times" in out
    is written in mode 0 as well).  A row whose count
    is out of range (status 5) or with a non-positive time (status 1) has
    coeffs, cost and times NaN.  The counts stay on the device."""
    import torch
    M = N // 2
    if mode not in (0, 1):
        raise MTGError("mode must be 0 or 1")
    if not isinstance(fixed_vals, torch.Tensor) or fixed_vals.dim() != 3:
        raise MTGError("fixed_vals must be a CUDA tensor [B, D, N]")
    B, D = fixed_vals.shape[0], fixed_vals.shape[1]
    _require(fixed_vals, (B, D, N), "fixed_vals")
    if mode == 0:
        if not isinstance(times, torch.Tensor) or times.dim() != 2:
            raise MTGError("times must be a CUDA tensor [B, S_max]")
        if S_max is not None and S_max != times.shape[1]:
            raise MTGError(f"S_max = {S_max} but times has shape {tuple(times.shape)}")
        S_max = times.shape[1]
        _require(times, (B, S_max), "times")
        _require(x, (B, D, (S_max - 1) * M), "x")
    else:
        if times is not None:
            raise MTGError("mode 1 takes the times from x: times must be None")
        if not isinstance(x, torch.Tensor) or x.dim() != 2:
            raise MTGError("x must be a CUDA tensor [B, S_max + D (S_max - 1) M]")
        if S_max is None:  # width = S_max (1 + D M) - D M
            S_max, rem = divmod(x.shape[1] + D * M, 1 + D * M)
            if rem:
                raise MTGError(f"x has shape {tuple(x.shape)}: no S_max gives that width")
        _require(x, (B, S_max + D * (S_max - 1) * M), "x")
    S_max = int(S_max)
    _require_counts(seg_counts, B)
    dev = x.device
    out = dict(out) if out is not None else {}
    shapes = {"coeffs": (B, S_max, D, N), "cost": (B,)}
    if mode == 1 or "times" in out:
        shapes["times"] = (B, S_max)
    for name, shp in shapes.items():  # the caller's outputs first, then the missing ones
        if name in out:
            _require(out[name], shp, name)
    if "status" in out:
        _require_int32(out["status"], (B,), "status")
    for name, shp in shapes.items():
        if name not in out:
            out[name] = torch.empty(shp, dtype=torch.float64, device=dev)
    if "status" not in out:
        out["status"] = torch.empty(B, dtype=torch.int32, device=dev)
    check(lib().mtg_ragged_tube_coeffs(
        ctx.handle, N, D, r, S_max, B, mode, _ptr(seg_counts), _ptr(fixed_vals), _ptr(x),
        _ptr(times) if mode == 0 else None, _ptr(out["coeffs"]), _ptr(out["cost"]),
        _ptr(out.get("times")), _ptr(out["status"]), _stream(dev)),
        "mtg_ragged_tube_coeffs")
    return out


def sample_trajectories(coeffs, times, dt, t_start=0.0, t_end=-1.0, max_derivative=0,
                        n_max=None, with_times=True):
    """Batched Trajectory::evaluateRange (trajectory.cpp:74-134) for derivatives
    0..max_derivative (mtg_sample_trajectories).

    coeffs [B, S, D, N], times [B, S] (float64, CUDA).  Returns (samples
    [B, (max_derivative+1)*D, n_max] channel-major, sample_times [B, n_max]
    or None, n_samples [B] int32).  n_max defaults to the longest trajectory's
    sample count.
    """
    import torch
    B, S, D, N = coeffs.shape
    _require(coeffs, (B, S, D, N), "coeffs")
    _require(times, (B, S), "times")
    dev = times.device
    n_max, res = _sample_outputs(B, D, dev, dt, t_end, max_derivative, n_max, with_times,
                                 lambda: times.sum(dim=1).max().item())
    check(lib().mtg_sample_trajectories(N, D, S, B, _ptr(coeffs), _ptr(times), t_start, t_end,
                                        dt, n_max, max_derivative, *map(_ptr, res), _stream(dev)),
          "mtg_sample_trajectories")
    return res


def max_magnitude(coeffs, times, derivative, out=None):
    """Batched PolynomialOptimization::computeMaximumOfMagnitude
    (linear_impl:455-487; mtg_max_magnitude).

    coeffs [B, S, D, N], times [B, S] (float64, CUDA).  Returns a dict of
    time [B] (relative to the segment start), value [B], segment [B] int32:
    the Extremum of |p^(derivative)| over the trajectory.
    """
    import torch
    B, S, D, N = coeffs.shape
    _require(coeffs, (B, S, D, N), "coeffs")
    _require(times, (B, S), "times")
    dev = times.device
    if out is None:
        out = _extremum_out(B, dev)
    check(lib().mtg_max_magnitude(N, D, S, B, _ptr(coeffs), _ptr(times), derivative,
                                  _ptr(out["time"]), _ptr(out["value"]), _ptr(out["segment"]),
                                  _stream(dev)), "mtg_max_magnitude")
    return out


def _check_field(field, occupancy):
    if field is None:
        return
    import torch
    nz, ny, nx = occupancy.shape
    if not (isinstance(field, torch.Tensor) and field.is_cuda and field.dtype == torch.int16 and
            field.is_contiguous() and field.numel() == nz * ny * nx * 8):
        raise MTGError("near_field must be coll_field()'s int16 CUDA tensor [nz, ny, nx, 8]")


def coll_field(occupancy, params):
    """Near field of an occupancy map for the collision walk (mtg_coll_field):
    per voxel the seven box minima the walk would scan for (uint16 bits in an
    int16 tensor [nz, ny, nx, 8]).  params: make_coll_params(...) or
    make_collision_params(...) (only box_side is read).  Compute once per map
    and pass as near_field to LinearPlan.coll_cost / coll_optimize."""
    import torch
    nz, ny, nx = occupancy.shape
    cp = getattr(params, "coll", params)
    field = torch.empty((nz, ny, nx, 8), dtype=torch.int16, device=occupancy.device)
    check(lib().mtg_coll_field(_ptr(occupancy), nx, ny, nz, ctypes.byref(cp), _ptr(field),
                               _stream(occupancy.device)), "mtg_coll_field")
    return field


def magnitude_candidates(coeffs, times, derivative, max_candidates=None):
    """Batched candidate lists of the magnitude extrema
    (Segment::computeMinMaxMagnitudeCandidates, segment.cpp:82-161, per
    segment over all D dimensions; mtg_magnitude_candidates).

    coeffs [B, S, D, N], times [B, S] (float64, CUDA).  Returns a dict of
    time / value [B, S, C] and count [B, S] int32: per segment t = 0, T and
    the real roots of d/dt |p^(derivative)|^2 in [0, T] ascending, with
    |p^(derivative)| at each.  C defaults to 2 (N - derivative) - 1, which
    always suffices.  count is the number of candidates the search found, as
    the C ABI returns it (a count above C means a smaller max_candidates
    truncated the list); stored [B, S] = min(count, C) is the number of
    valid entries, and entries past it are unset.  (Round 4 had briefly
    clamped count and moved the found number to a "found" key; that
    alias is kept for callers written against it.)
    """
    import torch
    B, S, D, N = coeffs.shape
    _require(coeffs, (B, S, D, N), "coeffs")
    _require(times, (B, S), "times")
    dev = times.device
    C = int(max_candidates or 2 * (N - derivative) - 1)
    out = {"time": torch.empty((B, S, C), dtype=torch.float64, device=dev),
           "value": torch.empty((B, S, C), dtype=torch.float64, device=dev),
           "count": torch.empty((B, S), dtype=torch.int32, device=dev)}
    check(lib().mtg_magnitude_candidates(N, D, S, B, _ptr(coeffs), _ptr(times), derivative, C,
                                         _ptr(out["time"]), _ptr(out["value"]),
                                         _ptr(out["count"]), _stream(dev)),
          "mtg_magnitude_candidates")
    out["stored"] = torch.clamp(out["count"], max=C)
    out["found"] = out["count"]
    return out


def min_max_magnitude(coeffs, times, derivative):
    """Batched Trajectory::computeMinMaxMagnitude (trajectory.cpp:184-220;
    mtg_min_max_magnitude) over all D dimensions of coeffs [B, S, D, N].
    Returns a dict of min_time, min_value, min_segment, max_time, max_value,
    max_segment [B]."""
    import torch
    B, S, D, N = coeffs.shape
    _require(coeffs, (B, S, D, N), "coeffs")
    _require(times, (B, S), "times")
    dev = times.device
    out = {k: torch.empty(B, dtype=torch.float64, device=dev)
           for k in ("min_time", "min_value", "max_time", "max_value")}
    out["min_segment"] = torch.empty(B, dtype=torch.int32, device=dev)
    out["max_segment"] = torch.empty(B, dtype=torch.int32, device=dev)
    check(lib().mtg_min_max_magnitude(N, D, S, B, _ptr(coeffs), _ptr(times), derivative,
                                      _ptr(out["min_time"]), _ptr(out["min_value"]),
                                      _ptr(out["min_segment"]), _ptr(out["max_time"]),
                                      _ptr(out["max_value"]), _ptr(out["max_segment"]),
                                      _stream(dev)), "mtg_min_max_magnitude")
    return out


def soft_constraint_cost(coeffs, times, derivatives, limits, weight=100.0, maximum_cost=1.0e12,
                         out=None):
    """Batched evaluateMaximumMagnitudeAsSoftConstraint (nonlinear_impl:
    2735-2766; mtg_soft_constraint_cost) for the constraints
    (derivatives[c], limits[c]) of addMaximumMagnitudeConstraint.

    Returns a dict of cost [B] and maxima [B, n_constraints].
    """
    import ctypes

    import torch
    B, S, D, N = coeffs.shape
    _require(coeffs, (B, S, D, N), "coeffs")
    _require(times, (B, S), "times")
    nc = len(derivatives)
    if len(limits) != nc:
        raise MTGError("derivatives and limits differ in length")
    dev = times.device
    if out is None:
        out = {"cost": torch.empty(B, dtype=torch.float64, device=dev),
               "maxima": torch.empty((B, nc), dtype=torch.float64, device=dev)}
    der = (ctypes.c_int * max(nc, 1))(*[int(d) for d in derivatives])
    lim = (ctypes.c_double * max(nc, 1))(*[float(v) for v in limits])
    check(lib().mtg_soft_constraint_cost(N, D, S, B, _ptr(coeffs), _ptr(times), nc, der, lim,
                                         float(weight), float(maximum_cost), _ptr(out["maxima"]),
                                         _ptr(out["cost"]), _stream(dev)),
          "mtg_soft_constraint_cost")
    return out
