// mtg_time_device.h — the drivers of the segment-time objective, once for
// every inner solver: the cost-and-gradient driver (objectiveFunctionTime /
// getCostAndGradientTime, nonlinear_impl:877-945, 2495-2584) and the batched
// optimiser (optimizeTime, nonlinear_impl:332-397).  One trajectory per
// 64-lane workgroup; every lane calls.  The kernels of mtg_kernels.hip
// (Traj<N>) and mtg_time_std.hip (stdp::Solver, wave::Solver) build an
// evaluator and call these; the objective itself stays with each solver.
//
// An evaluator Ev is the solver extended (by derivation) with
//   int lane;           the solver's
//   double* T();        S doubles (LDS): the evaluation point
//   double* state(S);   4S doubles (LDS): the driver's state
//   double eval(S, tab, cbuf, const mtg_time_params& p, double* viol);
//                       J at T(), wave-uniform; *viol: the hard-constraint
//                       violation (0 without hard constraints).  tab and cbuf
//                       are the kernel's table pointer and soft-constraint
//                       LDS, handed through.  Begins with a workgroup
//                       barrier, so writes to T() need none after.
//   bool bad();         sticky: some evaluated point held an invalid time
//   bool not_spd();     sticky: some solve met a non-positive pivot
//   void fixed_d_gradient(S, const double* Tb, const mtg_time_params& p,
//                         double* g, double* scratch);
//                       the grad_mode 1 gradient at the base times Tb, d held
//                       at the base solution, into g (S); scratch: 2S doubles.
// The global rows of trajectory b (times, grad, times_io) start at
// b * row_stride: S for the uniform kernels, S_max for the ragged ones
// (mtg_ragged.hip), whose rows are padded rectangles.
// Each driver calls eval from ONE call site (a loop over evaluation points),
// so the solver body is instantiated once per kernel and stays within the
// register file.  The hooks are always_inline and the evaluator is the
// kernel's one solver object, so a kernel compiles as if the driver were
// written out in it (same inlining decisions: tools/kernel_regs.py).
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

#include "mtg_device.h"
#include "mtg_sbplx_device.h"

namespace mtg {

// Central-difference time around T_n: T_n - inc (even gi) or T_n + inc (odd),
// both clamped to 0.1 when T_n <= 0.1 (nonlinear_impl:2529-2530).
__device__ __attribute__((always_inline)) inline double fd_time(double Tn, int gi, double inc) {
  return Tn <= 0.1 ? 0.1 : ((gi & 1) ? Tn + inc : Tn - inc);
}

// Central-difference point gi (0 .. 2S-1) around the base times Tb into T:
// segment n = gi / 2 at fd_time, the others at their base times.
__device__ inline void set_fd_point(double* T, const double* Tb, int S, int gi, double inc,
                                    int lane) {
  const int n = gi >> 1;
  for (int i = lane; i < S; i += kWave) {
    const double Tn = Tb[i];
    T[i] = i != n ? Tn : fd_time(Tn, gi, inc);
  }
}

__device__ __attribute__((always_inline)) inline int traj_status(bool bad, bool not_spd) {
  return bad ? MTG_TRAJ_BAD_TIME : (not_spd ? MTG_TRAJ_NOT_SPD : MTG_TRAJ_OK);
}

// J(T) with optional gradient: grad_mode 1 through the evaluator's hook,
// grad_mode 2 by central differences of J (2S further evaluations).  A point
// with an invalid time, the base or a central-difference one (increment >=
// T_n > 0.1), makes the row MTG_TRAJ_BAD_TIME with NaN cost and gradient.
template <class Ev>
__device__ __attribute__((always_inline)) void time_cost_drive(
    Ev& ev, int S, int row_stride, const double* __restrict__ tab, double* cbuf,
    const double* __restrict__ times, const mtg_time_params& p, double* __restrict__ cost,
    double* __restrict__ grad, int32_t* __restrict__ status) {
  const int64_t b = blockIdx.x;
  const int lane = ev.lane;
  double* T = ev.T();        // evaluation point
  double* Tb = ev.state(S);  // base times
  double* g = Tb + S;        // gradient, then 2S doubles for the grad_mode 1 hook
  for (int i = lane; i < S; i += kWave) T[i] = Tb[i] = times[b * row_stride + i];
  const bool fd = grad && p.grad_mode == 2;
  const int nevals = 1 + (fd ? 2 * S : 0);
  double J0 = 0.0, Jlo = 0.0;
  for (int e = 0; e < nevals; ++e) {
    if (e > 0) set_fd_point(T, Tb, S, e - 1, p.increment, lane);
    double viol;
    const double J = ev.eval(S, tab, cbuf, p, &viol);
    if (e == 0) {
      J0 = J;
      if (ev.bad()) break;
    } else if ((e - 1) & 1) {
      if (lane == 0) g[(e - 1) >> 1] = (J - Jlo) / (2.0 * p.increment);
    } else {
      Jlo = J;
    }
  }
  __syncthreads();
  if (grad && p.grad_mode == 1 && !ev.bad()) ev.fixed_d_gradient(S, Tb, p, g, g + S);
  const bool bad = ev.bad();
  if (lane == 0) {
    if (cost) cost[b] = bad ? NAN : J0;
    if (status) status[b] = traj_status(bad, ev.not_spd());
  }
  if (grad && p.grad_mode != 0)
    for (int i = lane; i < S; i += kWave) grad[b * row_stride + i] = bad ? NAN : g[i];
}

// Bounds [0.1, 2 T0]; p.optimizer 0: projected, scaled steepest descent on
// the grad_mode 2 gradient with an expand/backtrack step rule; `max_evals`
// objective evaluations (NLopt maxeval semantics, nonlinear_impl:101;
// gradient evaluations are not counted).  p.optimizer 1: LN_SBPLX
// (mtg_sbplx_device.h, state at sbs).  A state machine with one objective
// evaluation per loop trip.
template <class Ev>
__device__ __attribute__((always_inline)) void time_optimize_drive(
    Ev& ev, int S, int row_stride, const double* __restrict__ tab, double* cbuf,
    double* __restrict__ times_io, const mtg_time_params& p, int max_evals, double* __restrict__ cost,
    int32_t* __restrict__ evals_out, int32_t* __restrict__ solves_out,
    int32_t* __restrict__ result_out, int32_t* __restrict__ status, sbplx::State* sbs) {
  const int64_t b = blockIdx.x;
  const int lane = ev.lane;
  double* T = ev.T();         // evaluation point
  double* Tcur = ev.state(S);  // accepted times
  double* T0 = Tcur + S;      // initial times (bounds)
  double* g = T0 + S;         // gradient at Tcur
  double* gv = g + S;         // gradient of the violation at Tcur (hard constraints)
  for (int i = lane; i < S; i += kWave) T[i] = Tcur[i] = T0[i] = times_io[b * row_stride + i];
  constexpr double kLower = 0.1;  // kOptimizationTimeLowerBound (:370)
  enum { kBase, kGrad, kTrial, kDone };
  int phase = kBase, gi = 0, evals = 0, nsolve = 0, res = 0;
  double f = 0.0, fv = 0.0, Jlo = 0.0, vlo = 0.0;
  double alpha = 0.1;  // initial_stepsize_rel (polynomial_optimization_nonlinear.h:55)
  // LN_SBPLX (optimizer 1): the machine picks every point, lane 0 advances it
  const bool sb = p.optimizer == 1;
  sbplx::Machine mach{sbs};
  if (sb) {
    __syncthreads();
    if (lane == 0)
      mach.init(S, T, p.initial_stepsize_rel > 0.0 ? p.initial_stepsize_rel : 0.1, max_evals,
                p.f_rel, p.f_abs);
    __syncthreads();
    if (sbs->done) phase = kDone;  // start outside the bounds (NLopt: FAILURE)
  }
  MTG_STAMP(460);
  while (phase != kDone) {
    double viol;
    const double J = ev.eval(S, tab, cbuf, p, &viol);
    ++nsolve;
    if (sb) {
      if (ev.bad()) break;
      __syncthreads();
      if (lane == 0) mach.resume(J, T);
      __syncthreads();
      if (sbs->done) break;
      continue;
    }
    if (phase == kBase) {
      f = J;
      fv = viol;
      evals = 1;
      if (ev.bad()) break;
      phase = kGrad;
      gi = 0;
    } else if (phase == kGrad) {
      if (gi & 1) {
        if (lane == 0) {
          g[gi >> 1] = (J - Jlo) / (2.0 * p.increment);
          gv[gi >> 1] = (viol - vlo) / (2.0 * p.increment);
        }
      } else {
        Jlo = J;
        vlo = viol;
      }
      if (++gi == 2 * S) phase = kTrial;
    } else {  // trial point
      ++evals;
      // Feasibility first (hard constraints; viol is 0 otherwise).
      if (viol == 0.0 ? (fv > 0.0 || J < f) : viol < fv) {
        f = J;
        fv = viol;
        for (int i = lane; i < S; i += kWave) Tcur[i] = T[i];
        alpha = fmin(alpha * 1.5, 1.0);
        phase = kGrad;
        gi = 0;
      } else {
        alpha *= 0.5;
      }
    }
    __syncthreads();
    // Next evaluation point.
    if (phase == kGrad) {
      set_fd_point(T, Tcur, S, gi, p.increment, lane);
    } else if (phase == kTrial) {
      if (!(evals < max_evals && alpha > 1e-9)) break;
      // Scaled direction -g_n T0_n, normalised so the largest relative move
      // is alpha; from an infeasible incumbent (hard constraints) the
      // direction descends the violation instead.
      const double* dir = fv > 0.0 ? gv : g;
      double gmax = 0.0;
      for (int i = 0; i < S; ++i) gmax = fmax(gmax, fabs(dir[i] * T0[i]));
      if (!(gmax > 0.0)) break;
      int moved = 0;
      for (int i = 0; i < S; ++i) {
        const double step = alpha * T0[i] * (dir[i] * T0[i]) / gmax;
        double tn = Tcur[i] - step;
        tn = fmin(fmax(tn, kLower), 2.0 * T0[i]);
        if (tn != Tcur[i]) moved = 1;
        if (lane == 0) T[i] = tn;
      }
      __syncthreads();
      if (!moved) break;
    }
  }
  __syncthreads();
  MTG_STAMP(461);
  if (sb) {  // NLopt's x and opt_f: the best point and its value
    for (int i = lane; i < S; i += kWave) Tcur[i] = sbplx::best_x(sbs)[i];
    f = sbs->minf;
    evals = sbs->nevals;
    res = sbs->result;
    __syncthreads();
  } else {
    res = evals >= max_evals ? sbplx::kMaxEval : sbplx::kXtol;
  }
  for (int i = lane; i < S; i += kWave) times_io[b * row_stride + i] = Tcur[i];
  const bool bad = ev.bad();
  if (lane == 0) {
    if (cost) cost[b] = bad ? NAN : f;
    if (evals_out) evals_out[b] = evals;
    if (solves_out) solves_out[b] = nsolve;
    if (result_out) result_out[b] = res;
    if (status) status[b] = traj_status(bad, ev.not_spd());
  }
}

}  // namespace mtg
