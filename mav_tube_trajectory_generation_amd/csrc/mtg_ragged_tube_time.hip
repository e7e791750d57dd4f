// mtg_ragged_tube_time.hip — the segment-time objective with the tube QCQP as
// its inner solve and the LN_SBPLX optimiser over it (mtg_tube_time.hip) for
// ragged batches: trajectory b has its own segment count S_b = seg_counts[b]
// (device), 2 <= S_b <= S_max, in the padded rectangles of mtg_ragged_tube.hip
// (include/mtg_hip.h, "Ragged tube QCQP time objective"):
//   positions B x (S_max+1) x 3   fixed_vals B x 3 x N   radii B x S_max x 2
//   times_cp, times, times_io, grad B x S_max
// Per row the arithmetic is that of the uniform entries at S = S_b.  The
// structure is theirs too: every objective evaluation of a round is a problem
// q = b P + j of one QCQP launch (P = 1, or 2 S_max + 1 with the central
// differences, of which row b uses the first 2 S_b + 1), and small kernels
// around it build the points, form J and advance one Subplex machine
// (mtg_sbplx_device.h, n = S_b) per trajectory.
//
// What is live is decided on the device and carried by one array, pcount: the
// points kernel writes pcount[q] = S_b for a problem that is to be solved and
// 0 for one that is not (an unused gradient point, a finished trajectory, a
// row whose count is out of range).  The QCQP kernel returns at 0 without
// touching any output, the ragged extrema kernel (mtg_ragged_eval.hip) takes
// pcount as its count vector and returns NaN at 0 without searching, and the
// finish kernel never reads a problem whose pcount is 0.  The host never
// reads the counts; all scratch is the caller's workspace and every word of
// it is written in the same call before it is read.
#include <hip/hip_runtime.h>

#include <cmath>

#include "mtg_internal.h"
#include "mtg_sbplx_device.h"
#include "mtg_tube_time_shared.h"
#include "mtg_tube_device.h"

namespace mtg {

namespace {

constexpr double kLower = 0.1;  // kOptimizationTimeLowerBound (nonlinear_impl:370)

__device__ inline bool count_ok(int S, int S_max) { return S >= 2 && S <= S_max; }

// Row j of the evaluation points of trajectory b from its times T (stride
// S_max), as tube_time_points_kernel, and the live count of problem b P + j.
__global__ void ragged_tube_time_points_kernel(int S_max, int64_t B, int P,
                                               const int32_t* __restrict__ seg_counts,
                                               const double* __restrict__ T, double h,
                                               const int32_t* __restrict__ skip,
                                               double* __restrict__ pts,
                                               int32_t* __restrict__ pcount) {
  const int64_t idx = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (idx >= B * P * S_max) return;
  const int64_t q = idx / S_max, b = q / P;
  const int j = static_cast<int>(q % P), i = static_cast<int>(idx % S_max);
  const int S = seg_counts[b];
  const bool live = count_ok(S, S_max) && !(skip && skip[b]) && j < 2 * S + 1;
  if (i == 0) pcount[q] = live ? S : 0;
  if (!live || i >= S) return;
  double t = T[b * S_max + i];
  if (j > 0 && i == (j - 1) / 2) t = t <= kLower ? kLower : ((j & 1) ? t - h : t + h);
  pts[idx] = t;
}

// tube_time_finish_kernel with the row's own S.  A row whose count is out of
// range gets its failure values where the cost entry's outputs are given; a
// row that was not evaluated this round (pcount 0) is left alone.
__global__ void ragged_tube_time_finish_kernel(
    int S_max, int64_t B, int P, const int32_t* __restrict__ seg_counts,
    const int32_t* __restrict__ pcount, const double* __restrict__ pts,
    const double* __restrict__ qcost, const int32_t* __restrict__ qstatus,
    const double* __restrict__ soft, double time_penalty, double h, double* __restrict__ Jall,
    double* __restrict__ cost, double* __restrict__ grad, int32_t* __restrict__ status) {
  const int64_t b = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const int S = seg_counts[b];
  if (!count_ok(S, S_max)) {
    if (cost) cost[b] = NAN;
    if (grad)
      for (int i = 0; i < S_max; ++i) grad[b * S_max + i] = NAN;
    if (status) status[b] = MTG_TRAJ_BAD_SEGMENTS;
    return;
  }
  if (pcount[b * P] == 0) return;
  const int rows = P > 1 ? 2 * S + 1 : 1;
  double J0 = 0.0, Jprev = 0.0;
  for (int j = 0; j < rows; ++j) {
    const int64_t q = b * P + j;
    double total = 0.0;
    for (int i = 0; i < S; ++i) total += pts[q * S_max + i];  // nonlinear_impl:2768-2774
    const int st = qstatus[q];
    double J = qcost[q] + total * total * time_penalty;
    if (soft) J += soft[q];
    if (st == MTG_TRAJ_BAD_TIME || st == MTG_TRAJ_NOT_SPD) J = NAN;
    if (Jall) Jall[q] = J;
    if (j == 0) {
      J0 = J;
    } else if (j & 1) {
      Jprev = J;
    } else if (grad) {
      grad[b * S_max + (j - 1) / 2] = (J - Jprev) / (2.0 * h);
    }
  }
  if (grad)
    for (int i = S; i < S_max; ++i) grad[b * S_max + i] = 0.0;
  if (cost) cost[b] = J0;
  if (status) status[b] = qstatus[b * P];
}

// The optimiser's state per trajectory (rows of S_max where per segment).
struct OptState {
  double *T0, *Ttr;
  int32_t *done, *st;
  char* sb;  // one machine state per trajectory (sb_bytes each, sized for S_max)
  size_t sb_bytes;
  double* warm;  // the IPM warm-start state per trajectory (stride for S_max)
  int32_t* warm_ok;
  int32_t* iters;  // IPM iterations of each trajectory's last solve
  int32_t* order;  // the next round's dispatch order
};

// tube_time_sbplx_init_kernel with n = S_b.  A row whose count is out of
// range never starts: it is done from the outset and the final kernel writes
// its failure values.
__global__ void ragged_tube_time_sbplx_init_kernel(int S_max, int64_t B,
                                                   const int32_t* __restrict__ seg_counts,
                                                   const double* __restrict__ times,
                                                   double step_rel, int max_evals,
                                                   double ftol_rel, double ftol_abs, OptState s) {
  const int64_t b = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const int S = seg_counts[b];
  s.warm_ok[b] = 0;  // the first evaluation (T0) starts cold
  s.iters[b] = 0;
  if (!count_ok(S, S_max)) {
    s.done[b] = 1;
    s.st[b] = MTG_TRAJ_BAD_SEGMENTS;
    return;
  }
  for (int i = 0; i < S; ++i) {
    const double t = times[b * S_max + i];
    s.T0[b * S_max + i] = t;
    s.Ttr[b * S_max + i] = t;
  }
  sbplx::Machine m{sb_state(s, b)};
  m.init(S, s.Ttr + b * S_max, step_rel, max_evals, ftol_rel, ftol_abs);
  s.done[b] = m.s->done;  // a start outside the bounds: no evaluation
  s.st[b] = MTG_TRAJ_OK;
}

// The machine's step between rounds (tube_time_sbplx_step_body,
// mtg_tube_time_shared.h).
__global__ void ragged_tube_time_sbplx_step_kernel(int S_max, int64_t B, int first,
                                                   const double* __restrict__ Jall,
                                                   const int32_t* __restrict__ qstatus,
                                                   OptState s) {
  tube_time_sbplx_step_body(S_max, B, first, Jall, qstatus, s);
}

// tube_time_sbplx_final_kernel: the first S_b entries of times_io only.  A
// row whose count is out of range has no machine: its times stay untouched.
__global__ void ragged_tube_time_sbplx_final_kernel(int S_max, int64_t B,
                                                    const int32_t* __restrict__ seg_counts,
                                                    OptState s, double* __restrict__ times_io,
                                                    double* __restrict__ cost,
                                                    int32_t* __restrict__ evals,
                                                    int32_t* __restrict__ result,
                                                    int32_t* __restrict__ status) {
  const int64_t b = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const int S = seg_counts[b];
  if (!count_ok(S, S_max)) {
    if (cost) cost[b] = NAN;
    if (evals) evals[b] = 0;
    if (result) result[b] = sbplx::kFailure;
    if (status) status[b] = MTG_TRAJ_BAD_SEGMENTS;
    return;
  }
  const sbplx::State* st = sb_state(s, b);
  const double* x = sbplx::best_x(st);
  for (int i = 0; i < S; ++i) times_io[b * S_max + i] = x[i];
  if (cost) cost[b] = st->minf;
  if (evals) evals[b] = st->nevals;
  if (result) result[b] = st->result;
  if (status) status[b] = s.st[b];
}

// The next round's dispatch order (tube_time_order_body,
// mtg_tube_time_shared.h), keyed by the last solve's iterations; the rows that
// have finished or never started go last.
__global__ __launch_bounds__(1024) void ragged_tube_time_order_kernel(
    int64_t B, const int32_t* __restrict__ iters, const int32_t* __restrict__ done,
    int32_t* __restrict__ order) {
  tube_time_order_body(B, iters, done, order);
}

}  // namespace

// One QCQP per live problem: tube_solve_one (mtg_tube_device.h) with padded
// rows, the warm start and no x output.
// Problem q = b P + j takes its geometry and T0 maps from trajectory b = q / P
// at the padded strides, its times from row q of the points buffer, and its
// count from pcount[q]: S_b where the problem is live, 0 where it is to be
// skipped (the workgroup then returns without touching any output).  The
// warm-start state of problem q starts at q tube_warm_doubles(N, S_max) and is
// carved for S_b.  coeffs is the layout the ragged extrema kernel reads:
// segments >= S_b are written 0.0, or NaN like the rest of the row where the
// problem has a bad time (the extrema kernel reads the first S_b only).
template <int N>
__global__ __launch_bounds__(tube_threads<N>())
__attribute__((amdgpu_waves_per_eu(tube_threads<N>() / kWave,
                                   tube_threads<N>() / kWave)))
void ragged_tube_eval_kernel(
    int S_max, int r, int P, const int32_t* __restrict__ pcount, const double* __restrict__ tab,
    const double* __restrict__ positions, const double* __restrict__ fixed_vals,
    const double* __restrict__ times_cp, const double* __restrict__ pts,
    const double* __restrict__ radii, double tol, int max_iter, double* __restrict__ coeffs,
    double* __restrict__ qcost, int32_t* __restrict__ iters, int32_t* __restrict__ qstatus,
    double* __restrict__ warm, int32_t* __restrict__ warm_ok,
    const int32_t* __restrict__ order) {
  constexpr int M = N / 2;
  const int64_t q = order ? order[blockIdx.x] : xcd_problem(blockIdx.x, gridDim.x);
  // Workgroup-uniform.  Anything but a count the launch's LDS and the padded
  // rows were sized for is "skip", not only 0.
  const int S = __builtin_amdgcn_readfirstlane(pcount[q]);
  if (!count_ok(S, S_max)) return;
  const int64_t b = q / P;
  tube_solve_one<N>(
      S, S_max, true, r, tab, positions + b * (S_max + 1) * 3, fixed_vals + b * 3 * N,
      times_cp + b * S_max, pts + q * S_max, radii + b * S_max * 2, tol, max_iter, nullptr,
      coeffs + q * S_max * 3 * N, q, qcost, iters, qstatus,
      warm ? warm + q * (static_cast<int64_t>(S_max - 1) * 3 * M + 2 * tube_ncon(N, S_max))
           : nullptr,
      warm_ok, &Tube<N>::ipm);
}

namespace {

// Caller-owned workspace (mtg_ragged_tube_time_workspace_bytes), carved in a
// fixed order as mtg_tube_time.hip carves its own (Carver).
struct Workspace {
  double *coeffs, *pts, *qcost, *softc, *Jall, *maxima;
  int32_t *qstatus, *pcount;
  OptState s;  // optimiser only
};
size_t carve(void* base, int N, int S_max, int64_t B, int P, int n_soft, bool optimiser,
             Workspace* w) {
  Carver c{static_cast<char*>(base)};
  const int64_t BP = B * P;
  w->coeffs = c.take<double>(BP * S_max * 3 * N);
  w->pts = c.take<double>(BP * S_max);
  w->qcost = c.take<double>(BP);
  w->softc = c.take<double>(BP);
  w->Jall = c.take<double>(BP);
  w->maxima = c.take<double>(BP * (n_soft > 0 ? n_soft : 1));
  w->qstatus = c.take<int32_t>(BP);
  w->pcount = c.take<int32_t>(BP);
  w->s = OptState{};
  if (optimiser) {
    w->s.T0 = c.take<double>(B * S_max);
    w->s.Ttr = c.take<double>(B * S_max);
    w->s.done = c.take<int32_t>(B);
    w->s.st = c.take<int32_t>(B);
    w->s.sb_bytes = sbplx::state_bytes(S_max);
    w->s.sb = c.take<char>(B * static_cast<int64_t>(w->s.sb_bytes));
    w->s.warm = c.take<double>(B * tube_warm_doubles(N, S_max));
    w->s.warm_ok = c.take<int32_t>(B);
    w->s.iters = c.take<int32_t>(B);
    w->s.order = c.take<int32_t>(B);
  }
  return c.off;
}

// The optimiser is LN_SBPLX, which is gradient-free: one point per round.
int points_of(const mtg_time_params& p, int S_max, bool optimiser) {
  return (!optimiser && p.grad_mode == 2) ? 2 * S_max + 1 : 1;
}

// What one round needs beyond the trajectories' inputs.
struct Round {
  const double* T;       // B x S_max: the point of every trajectory
  const int32_t* skip;   // B, nullable: finished trajectories
  double* warm;          // nullable, with warm_ok and iters
  int32_t *warm_ok, *iters;
  const int32_t* order;  // nullable
};

// Points -> QCQP -> soft -> J for B trajectories x P rows.  pcount is written
// for every problem by the points kernel; every array the finish kernel reads
// for a live problem (pts, qcost, qstatus, softc) is written earlier in the
// same stream: the points, then qcost and qstatus by that problem's QCQP
// workgroup (also where it fails), softc by the extrema launch.
hipError_t evaluate_points(const RaggedTubeArgs& a, int P, const Round& rd, double tol,
                           int max_iter, const mtg_time_params& p, const Workspace& w,
                           double* Jall, double* cost, double* grad, int32_t* status,
                           hipStream_t st) {
  const int S_max = a.S_max;
  const int64_t BP = a.B * P;
  hipLaunchKernelGGL(ragged_tube_time_points_kernel, dim3(blocks_for(BP * S_max)), dim3(256), 0,
                     st, S_max, a.B, P, a.seg_counts, rd.T, p.increment, rd.skip, w.pts,
                     w.pcount);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  e = with_order(a.N, [&](auto n) {
    return launch(ragged_tube_eval_kernel<n()>, BP, tube_threads<n()>(),
                  ragged_tube_lds_bytes(a.N, S_max), st, S_max, a.r, P,
                  static_cast<const int32_t*>(w.pcount), a.tab, a.positions, a.fixed_vals,
                  a.times_cp, static_cast<const double*>(w.pts), a.radii, tol, max_iter,
                  w.coeffs, w.qcost, rd.iters, w.qstatus, rd.warm, rd.warm_ok, rd.order);
  });
  if (e != hipSuccess) return e;
  if (p.n_soft > 0) {
    SoftSpec spec{};
    spec.n = p.n_soft;
    for (int c = 0; c < p.n_soft; ++c) {
      spec.derivative[c] = p.soft_derivative[c];
      spec.limit[c] = p.soft_limit[c];
    }
    spec.weight = p.soft_weight;
    spec.maximum_cost = p.soft_maximum_cost;
    const RaggedEvalOut out{w.maxima, nullptr, nullptr, w.softc, nullptr, nullptr};
    e = launch_ragged_extrema(a.N, 3, S_max, BP, w.pcount, w.coeffs, w.pts, spec, out, st);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(ragged_tube_time_finish_kernel, dim3(blocks_for(a.B)), dim3(256), 0, st,
                     S_max, a.B, P, a.seg_counts, static_cast<const int32_t*>(w.pcount),
                     static_cast<const double*>(w.pts), static_cast<const double*>(w.qcost),
                     static_cast<const int32_t*>(w.qstatus),
                     static_cast<const double*>(p.n_soft > 0 ? w.softc : nullptr),
                     p.time_penalty, p.increment, Jall, cost, grad, status);
  return hipGetLastError();
}

}  // namespace

size_t ragged_tube_time_workspace_bytes(int N, int S_max, int64_t B, const mtg_time_params& p,
                                        bool optimiser) {
  Workspace w;
  return carve(nullptr, N, S_max, B, points_of(p, S_max, optimiser), p.n_soft, optimiser, &w) +
         256;
}

int64_t ragged_tube_time_problems(int S_max, int64_t B, const mtg_time_params& p,
                                  bool optimiser) {
  return B * points_of(p, S_max, optimiser);
}

int ragged_tube_time_cost(const RaggedTubeArgs& a, double tol, int max_iter,
                          const mtg_time_params& p, double* cost, double* grad, int32_t* status,
                          void* workspace, size_t workspace_bytes, hipStream_t st) {
  const int P = points_of(p, a.S_max, false);
  Workspace w;
  if (ragged_tube_time_workspace_bytes(a.N, a.S_max, a.B, p, false) > workspace_bytes)
    return MTG_ERR_INVALID_ARG;
  carve(workspace, a.N, a.S_max, a.B, P, p.n_soft, false, &w);
  const Round rd{a.times, nullptr, nullptr, nullptr, nullptr, nullptr};
  const hipError_t e = evaluate_points(a, P, rd, tol, max_iter, p, w, nullptr, cost,
                                       p.grad_mode == 2 ? grad : nullptr, status, st);
  return e == hipSuccess ? MTG_OK : MTG_ERR_HIP;
}

// max_evals rounds, all stream-ordered, as tube_time_optimize: a trajectory
// that has stopped (or never started) has its `done` flag set and is skipped
// by every later kernel, so the call needs no host round trip and can be
// captured in a graph.  The loop is bounded by max_evals.
int ragged_tube_time_optimize(const RaggedTubeArgs& a, double* times_io, double tol, int max_iter,
                              const mtg_time_params& p, int max_evals, double* cost,
                              int32_t* evals, int32_t* result, int32_t* status, void* workspace,
                              size_t workspace_bytes, hipStream_t st) {
  const int S_max = a.S_max;
  const int64_t B = a.B;
  Workspace w;
  if (ragged_tube_time_workspace_bytes(a.N, S_max, B, p, true) > workspace_bytes)
    return MTG_ERR_INVALID_ARG;
  carve(workspace, a.N, S_max, B, 1, p.n_soft, true, &w);
  const OptState& s = w.s;
  hipLaunchKernelGGL(ragged_tube_time_sbplx_init_kernel, dim3(blocks_for(B)), dim3(256), 0, st,
                     S_max, B, a.seg_counts, static_cast<const double*>(times_io),
                     p.initial_stepsize_rel > 0.0 ? p.initial_stepsize_rel : 0.1, max_evals,
                     p.f_rel, p.f_abs, s);
  if (hipGetLastError() != hipSuccess) return MTG_ERR_HIP;
  // Control-point maps stay at the initial times (built once at setup,
  // qcqp_impl:152-157); Q and A^-1 follow the evaluation points.
  RaggedTubeArgs q = a;
  q.times_cp = s.T0;
  for (int round = 0; round < max_evals; ++round) {
    // Each solve warm-starts from the trajectory's previous one; from the
    // second round on, the longest solves go first.
    const Round rd{s.Ttr, s.done, s.warm, s.warm_ok, s.iters, round > 0 ? s.order : nullptr};
    const hipError_t e = evaluate_points(q, 1, rd, tol, max_iter, p, w, w.Jall, nullptr, nullptr,
                                         nullptr, st);
    if (e != hipSuccess) return MTG_ERR_HIP;
    hipLaunchKernelGGL(ragged_tube_time_sbplx_step_kernel, dim3(blocks_for(B)), dim3(256), 0, st,
                       S_max, B, round == 0 ? 1 : 0, static_cast<const double*>(w.Jall),
                       static_cast<const int32_t*>(w.qstatus), s);
    if (round + 1 < max_evals)
      hipLaunchKernelGGL(ragged_tube_time_order_kernel, dim3(1), dim3(1024), 0, st, B,
                         static_cast<const int32_t*>(s.iters),
                         static_cast<const int32_t*>(s.done), s.order);
    if (hipGetLastError() != hipSuccess) return MTG_ERR_HIP;
  }
  hipLaunchKernelGGL(ragged_tube_time_sbplx_final_kernel, dim3(blocks_for(B)), dim3(256), 0, st,
                     S_max, B, a.seg_counts, s, times_io, cost, evals, result, status);
  return hipGetLastError() == hipSuccess ? MTG_OK : MTG_ERR_HIP;
}

}  // namespace mtg
