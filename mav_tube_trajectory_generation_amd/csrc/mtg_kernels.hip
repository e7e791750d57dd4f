// mtg_kernels.hip — gfx950 kernels of the linear-solve and time-allocation
// hot path.  One 64-lane workgroup per trajectory; all per-trajectory state in
// LDS (mtg_device.h).  The time kernels are the generic solver's objective
// (objective_at) under the shared cost driver and optimiser of
// mtg_time_device.h.  Launchers at the bottom are called by mtg_host.cpp.
#include <hip/hip_runtime.h>

#include <cmath>

#include "mtg_device.h"
#include "mtg_extrema_device.h"
#include "mtg_internal.h"
#include "mtg_sbplx_device.h"
#include "mtg_time_device.h"

namespace mtg {

// ---------------------------------------------------------------------------
// Batched linear solve (setupFromVertices' per-trajectory part +
// solveLinear + computeCost, linear_impl:277-379, 113-130).
template <int N>
__global__ __launch_bounds__(kWave) void linear_solve_kernel(
    PlanDev pl, const double* __restrict__ fixed_vals, const double* __restrict__ times,
    double* __restrict__ coeffs, double* __restrict__ cost, double* __restrict__ free_vals,
    int32_t* __restrict__ status) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int S = pl.S, D = pl.D, nf = pl.nf, np = pl.np;
  const Layout lay = make_layout(N, S, D);
  Traj<N> t{S, D, pl.r, &lay, smem, reinterpret_cast<int*>(smem + lay.ndouble),
            static_cast<int>(threadIdx.x), pl.fmask, pl.use_mask != 0};
  const int64_t b = blockIdx.x;
  MTG_STAMP(0);
  t.load_inputs(pl.tab, pl.slots, pl.fixed_map, times + b * S, fixed_vals + b * D * nf, nf);
  __syncthreads();
  MTG_STAMP(1);
  t.compute_powers();
  __syncthreads();
  MTG_STAMP(2);
  const int bad_time = t.flag()[0] & 1;
  if (!bad_time) t.solve();
  const int fl = t.flag()[0];
  const int st = (fl & 1) ? MTG_TRAJ_BAD_TIME : ((fl & 2) ? MTG_TRAJ_NOT_SPD : MTG_TRAJ_OK);
  const int64_t per = static_cast<int64_t>(S) * D * N;
  if (bad_time) {
    for (int i = t.lane; i < per; i += kWave) coeffs[b * per + i] = NAN;
    if (free_vals)  // as every linear kernel: NaN free values on a bad time
      for (int i = t.lane; i < D * np; i += kWave) free_vals[b * D * np + i] = NAN;
    if (cost && t.lane == 0) cost[b] = NAN;
  } else {
    const double J = t.template coeffs_and_cost<true>(pl.tab, coeffs + b * per);
    if (cost && t.lane == 0) cost[b] = J;
    if (free_vals) {
      const int M = N / 2;
      for (int i = t.lane; i < (S + 1) * M * D; i += kWave) {
        const int sl = t.slot()[i / D];
        if (sl < 0) free_vals[b * D * np + (i % D) * np + (-sl - 1)] = t.dv()[i];
      }
    }
  }
  if (status && t.lane == 0) status[b] = st;
  MTG_STAMP(6);
}

// ---------------------------------------------------------------------------
// Coefficients and cost from given fixed and free derivatives, no solve
// (setFreeConstraints -> updateSegmentsFromCompactConstraints, linear_impl:
// 254-275, 497-506, and computeCost, :113-130).
template <int N>
__global__ __launch_bounds__(kWave) void coeffs_from_constraints_kernel(
    PlanDev pl, const double* __restrict__ fixed_vals, const double* __restrict__ free_vals,
    const double* __restrict__ times, double* __restrict__ coeffs, double* __restrict__ cost,
    int32_t* __restrict__ status) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int S = pl.S, D = pl.D, nf = pl.nf, np = pl.np;
  const Layout lay = make_layout(N, S, D);
  Traj<N> t{S, D, pl.r, &lay, smem, reinterpret_cast<int*>(smem + lay.ndouble),
            static_cast<int>(threadIdx.x), pl.fmask, pl.use_mask != 0};
  const int64_t b = blockIdx.x;
  t.load_inputs(pl.tab, pl.slots, pl.fixed_map, times + b * S, fixed_vals + b * D * nf, nf);
  for (int i = t.lane; i < D * np; i += kWave)
    t.dv()[pl.free_map[i % np] * D + i / np] = free_vals[b * D * np + i];
  __syncthreads();
  t.compute_powers();
  __syncthreads();
  const int bad_time = t.flag()[0] & 1;
  const int64_t per = static_cast<int64_t>(S) * D * N;
  if (bad_time) {
    for (int i = t.lane; i < per; i += kWave) coeffs[b * per + i] = NAN;
    if (cost && t.lane == 0) cost[b] = NAN;
  } else {
    const double J = t.template coeffs_and_cost<true>(pl.tab, coeffs + b * per);
    if (cost && t.lane == 0) cost[b] = J;
  }
  if (status && t.lane == 0) status[b] = bad_time ? MTG_TRAJ_BAD_TIME : MTG_TRAJ_OK;
}

// ---------------------------------------------------------------------------
// Per-segment matrices Q, A, A^-1, H for a batch of times (accessor parity:
// linear_impl:101-111, 132-169, 557-573, 318).  One thread per entry.
__device__ inline double falling(int n, int i) {  // base(n, i) = i!/(i-n)!
  if (i < n) return 0.0;
  double p = 1.0;
  for (int m = 0; m < n; ++m) p *= static_cast<double>(i - m);
  return p;
}

__device__ inline double ipow(double t, int e) {
  const double base = e < 0 ? 1.0 / t : t;
  const int n = e < 0 ? -e : e;
  double p = 1.0;
  for (int q = 0; q < n; ++q) p *= base;
  return p;
}

__global__ void segment_matrices_kernel(int N, int r, int64_t n,
                                        const double* __restrict__ tab,
                                        const double* __restrict__ times,
                                        double* Q, double* A, double* Ainv,
                                        double* H) {
  const int64_t gid = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  const int NN = N * N;
  if (gid >= n * NN) return;
  const int64_t s = gid / NN;
  const int e = static_cast<int>(gid % NN);
  const int a = e / N, c = e % N;
  const int M = N / 2;
  const double T = times[s];
  if (Q) {
    double q = 0.0;
    if (a >= r && c >= r) {
      const int ex = a + c - 2 * r + 1;
      q = falling(r, a) * falling(r, c) * ipow(T, ex) * 2.0 / ex;
    }
    Q[gid] = q;
  }
  if (A) {
    const int l = a % M;
    double v;
    if (a < M)
      v = (c == l) ? falling(l, l) : 0.0;
    else
      v = c >= l ? falling(l, c) * ipow(T, c - l) : 0.0;
    A[gid] = v;
  }
  if (Ainv) Ainv[gid] = tab[NN + e] * ipow(T, (c % M) - a);
  if (H) H[gid] = tab[e] * ipow(T, 1 - 2 * r + (a % M) + (c % M));
}

// ---------------------------------------------------------------------------
// Time-allocation objective J(T) = computeCost() + time_penalty (sum T)^2
// (objectiveFunctionTime, nonlinear_impl:877-945) with optional gradient.
template <int N, bool kSoft>
__device__ double objective_at(Traj<N>& t, const double* __restrict__ tab,
                               const mtg_time_params& p, double* cbuf, double* viol) {
  *viol = 0.0;
  // Assumes T() holds the times; recomputes powers and re-solves.
  __syncthreads();
  t.compute_powers();
  __syncthreads();
  t.clear_free();
  __syncthreads();
  t.solve();
  double J;
  if constexpr (kSoft) {
    // 0.5 e^T H e as before (Traj::coeffs_and_cost); coefficients into LDS
    J = t.template coeffs_and_cost<true, true>(tab, cbuf);
  } else {
    J = t.cost(tab);
  }
  double tot = 0.0;
  for (int i = 0; i < t.S; ++i) tot += t.T()[i];  // nonlinear_impl:2768-2774
  J += tot * tot * p.time_penalty;
  if constexpr (kSoft) {
    // evaluateMaximumMagnitudeAsSoftConstraint (nonlinear_impl:2735-2766):
    // one extremum search per constraint over the wave, from one call site.
    __syncthreads();
    double soft = 0.0;
    for (int c = 0; c < p.n_soft; ++c) {
      int K = 0;
      double lim = 1.0;
#pragma unroll
      for (int cc = 0; cc < kMaxSoftConstraints; ++cc)  // compile-time indices
        if (cc == c) {
          K = p.soft_derivative[cc];
          lim = p.soft_limit[cc];
        }
      const double m = ext_trajectory_max_wave_k<N>(K, cbuf, t.T(), t.S, t.D, t.lane);
      if (p.hard_constraints) {  // evaluateMaximumMagnitudeConstraint (:2687-2733)
        *viol = fmax(*viol, m - lim - p.hard_tolerance);
      } else {
        const double relative_violation = (m - lim) / lim;
        soft += fmin(p.soft_maximum_cost, exp(relative_violation * p.soft_weight));
      }
    }
    J += soft;
  }
  __syncthreads();
  return J;
}

// LDS for the soft-constraint objective's coefficients, after the layout.
__host__ __device__ inline size_t soft_cbuf_offset(const Layout& lay) {
  return (lay.bytes() + 15) / 16 * 16;
}
// The optimiser's LN_SBPLX state (mtg_sbplx_device.h) after everything else.
__host__ __device__ inline size_t sbplx_state_offset(const Layout& lay, int S, int D, int N,
                                                     bool soft) {
  const size_t end = soft ? soft_cbuf_offset(lay) + sizeof(double) * S * D * N : lay.bytes();
  return (end + 15) / 16 * 16;
}

// The evaluator of the shared drivers (mtg_time_device.h): Traj<N> with the
// drivers' hooks.  The evaluation point is the solver's T(), the drivers'
// state the layout's aux region, the flags the solver's (compute_powers and
// solve set them, nothing clears them).
template <int N, bool kSoft>
struct TrajEval : Traj<N> {
  __device__ __attribute__((always_inline)) double* state(int) const {
    return this->sm + this->lay->aux;
  }
  __device__ __attribute__((always_inline)) double eval(int, const double* __restrict__ tab,
                                                        double* cbuf, const mtg_time_params& p,
                                                        double* viol) {
    return objective_at<N, kSoft>(*this, tab, p, cbuf, viol);
  }
  __device__ __attribute__((always_inline)) bool bad() const {
    return (this->flag()[0] & 1) != 0;
  }
  __device__ __attribute__((always_inline)) bool not_spd() const {
    return (this->flag()[0] & 2) != 0;
  }
  // The reference's getCostAndGradientTime: with d held at the base solution
  // (dv), J_d(T') differs from J_d(T) only in segment n's block
  // (nonlinear_impl:2495-2584).  No re-solve; the wave sums each energy.
  __device__ __attribute__((always_inline)) void fixed_d_gradient(
      int S, const double* Tb, const mtg_time_params& p, double* g, double* /*scratch*/) {
    const double inc = p.increment;
    for (int n = 0; n < S; ++n) {
      const double qs = this->seg_energy_at(n, fd_time(Tb[n], 0, inc));
      const double qb = this->seg_energy_at(n, fd_time(Tb[n], 1, inc));
      if (this->lane == 0) g[n] = p.w_d * (qb - qs) / (2.0 * inc) + p.w_t * 1.0;
    }
    __syncthreads();
  }
};

// objectiveFunctionTime / getCostAndGradientTime and optimizeTime on the
// generic solver: the drivers of mtg_time_device.h around objective_at.
template <int N, bool kSoft>
__global__ __launch_bounds__(kWave) void time_cost_kernel(
    PlanDev pl, const double* __restrict__ fixed_vals, const double* __restrict__ times,
    mtg_time_params p, double* __restrict__ cost, double* __restrict__ grad,
    int32_t* __restrict__ status) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int S = pl.S, D = pl.D, nf = pl.nf;
  const Layout lay = make_layout(N, S, D);
  TrajEval<N, kSoft> ev{{S, D, pl.r, &lay, smem, reinterpret_cast<int*>(smem + lay.ndouble),
                         static_cast<int>(threadIdx.x), pl.fmask, pl.use_mask != 0}};
  const int64_t b = blockIdx.x;
  double* cbuf = reinterpret_cast<double*>(reinterpret_cast<char*>(smem) + soft_cbuf_offset(lay));
  ev.load_inputs(pl.tab, pl.slots, pl.fixed_map, times + b * S, fixed_vals + b * D * nf, nf);
  time_cost_drive(ev, S, S, pl.tab, cbuf, times, p, cost, grad, status);
}

template <int N, bool kSoft>
__global__ __launch_bounds__(kWave) void time_optimize_kernel(
    PlanDev pl, const double* __restrict__ fixed_vals, double* __restrict__ times_io,
    mtg_time_params p, int max_evals, double* __restrict__ cost,
    int32_t* __restrict__ evals_out, int32_t* __restrict__ solves_out,
    int32_t* __restrict__ result_out, int32_t* __restrict__ status) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int S = pl.S, D = pl.D, nf = pl.nf;
  const Layout lay = make_layout(N, S, D);
  TrajEval<N, kSoft> ev{{S, D, pl.r, &lay, smem, reinterpret_cast<int*>(smem + lay.ndouble),
                         static_cast<int>(threadIdx.x), pl.fmask, pl.use_mask != 0}};
  const int64_t b = blockIdx.x;
  double* cbuf = reinterpret_cast<double*>(reinterpret_cast<char*>(smem) + soft_cbuf_offset(lay));
  auto* sbs = reinterpret_cast<sbplx::State*>(reinterpret_cast<char*>(smem) +
                                              sbplx_state_offset(lay, S, D, N, kSoft));
  ev.load_inputs(pl.tab, pl.slots, pl.fixed_map, times_io + b * S, fixed_vals + b * D * nf, nf);
  time_optimize_drive(ev, S, S, pl.tab, cbuf, times_io, p, max_evals, cost, evals_out, solves_out,
                      result_out, status, sbs);
}

// ---------------------------------------------------------------------------
// Launchers.
template <int N>
static hipError_t launch_linear_n(const PlanDev& pl, int64_t B, const double* df,
                                  const double* times, double* coeffs, double* cost,
                                  double* free_vals, int32_t* status, hipStream_t st) {
  return launch(linear_solve_kernel<N>, B, kWave, make_layout(N, pl.S, pl.D).bytes(), st, pl, df,
                times, coeffs, cost, free_vals, status);
}

template <int N>
static hipError_t launch_coeffs_n(const PlanDev& pl, int64_t B, const double* df,
                                  const double* dp, const double* times, double* coeffs,
                                  double* cost, int32_t* status, hipStream_t st) {
  return launch(coeffs_from_constraints_kernel<N>, B, kWave, make_layout(N, pl.S, pl.D).bytes(),
                st, pl, df, dp, times, coeffs, cost, status);
}

template <int N>
static hipError_t launch_time_cost_n(const PlanDev& pl, int64_t B, const double* df,
                                     const double* times, const mtg_time_params& p,
                                     double* cost, double* grad, int32_t* status,
                                     hipStream_t st) {
  const Layout lay = make_layout(N, pl.S, pl.D);
  return with_soft(p.n_soft > 0, [&](auto soft) {
    const size_t bytes =
        soft ? soft_cbuf_offset(lay) + sizeof(double) * pl.S * pl.D * N : lay.bytes();
    return launch(time_cost_kernel<N, decltype(soft)::value>, B, kWave, bytes, st, pl, df, times,
                  p, cost, grad, status);
  });
}

template <int N>
static hipError_t launch_time_opt_n(const PlanDev& pl, int64_t B, const double* df,
                                    double* times, const mtg_time_params& p,
                                    int max_evals, double* cost, int32_t* evals,
                                    int32_t* solves, int32_t* result, int32_t* status,
                                    hipStream_t st) {
  const Layout lay = make_layout(N, pl.S, pl.D);
  return with_soft(p.n_soft > 0, [&](auto soft) {
    const size_t bytes =
        sbplx_state_offset(lay, pl.S, pl.D, N, soft) + sbplx::state_bytes(pl.S);
    return launch(time_optimize_kernel<N, decltype(soft)::value>, B, kWave, bytes, st, pl, df,
                  times, p, max_evals, cost, evals, solves, result, status);
  });
}

int linear_kernel_for_batch(const PlanDev& pl, int64_t B) {
  if (pl.kernel != MTG_KERNEL_AUTO) return pl.kernel;
  if (!pl.std_pattern) return MTG_KERNEL_GENERIC;
  if (has_linear_lane(pl) && B >= kLaneMinBatch) return MTG_KERNEL_LANE_PAIR;
  // The same test launch_linear_solve applies (std_pattern already implies
  // S <= kMaxStdS), so the reported kernel is the one that runs.
  return use_std_kernel(pl) ? MTG_KERNEL_STANDARD : MTG_KERNEL_GENERIC;
}

int64_t select_partials(const PlanDev& pl, int64_t B) {
  const int k = linear_kernel_for_batch(pl, B);
  if (k == MTG_KERNEL_LANE) return lane_blocks(B);
  if (k == MTG_KERNEL_LANE_PAIR) return lane2_blocks(B);
  return 0;  // one trajectory per workgroup: the costs are the partials
}

hipError_t launch_linear_solve(const PlanDev& pl, int64_t B, const double* df,
                               const double* times, double* coeffs, double* cost,
                               double* free_vals, int32_t* status, hipStream_t st,
                               const SelectArgs& sel) {
  const int k = linear_kernel_for_batch(pl, B);
  // A deferred selection (the previous step's costs, SelectArgs::prev_*):
  // an extra workgroup of the wave and lane-pair launches; a launch of its
  // own before the other kernels.
  SelectArgs own = sel;
  const bool prev_inside = k == MTG_KERNEL_LANE_PAIR || (k == MTG_KERNEL_STANDARD);
  if (sel.prev_out && !prev_inside) {
    const hipError_t e = launch_select_local(sel.prev_cost, sel.prev_count, sel.prev_start,
                                             sel.rank, sel.prev_out, st);
    if (e != hipSuccess) return e;
    own.prev_out = nullptr;
  }
  // Lane kernels: per-workgroup partials in the epilogue, then one small
  // reduction launch.  Wavefront kernels (one trajectory per workgroup): the
  // reduction reads the costs.
  if (k == MTG_KERNEL_LANE || k == MTG_KERNEL_LANE_PAIR) {
    const hipError_t e =
        k == MTG_KERNEL_LANE
            ? launch_linear_solve_lane(pl, B, df, times, coeffs, cost, free_vals, status, st, own)
            : launch_linear_solve_lane2(pl, B, df, times, coeffs, cost, free_vals, status, st,
                                        own);
    if (e != hipSuccess || !sel.out) return e;
    const int64_t n = k == MTG_KERNEL_LANE ? lane_blocks(B) : lane2_blocks(B);
    return launch_select_reduce(sel.part_cost, sel.part_idx, n, B, sel.start, sel.rank, sel.out,
                                st);
  }
  hipError_t e;
  if (use_std_kernel(pl)) {
    e = launch_linear_solve_std(pl, B, df, times, coeffs, cost, free_vals, status, st, own);
    if (e != hipSuccess || !sel.out) return e;
    return launch_select_local(cost, B, sel.start, sel.rank, sel.out, st);
  }
  e = with_order(pl.N, [&](auto n) {
    return launch_linear_n<n()>(pl, B, df, times, coeffs, cost, free_vals, status, st);
  });
  if (e != hipSuccess || !sel.out) return e;
  return launch_select_local(cost, B, sel.start, sel.rank, sel.out, st);
}

hipError_t launch_coeffs_from_constraints(const PlanDev& pl, int64_t B, const double* df,
                                          const double* dp, const double* times,
                                          double* coeffs, double* cost, int32_t* status,
                                          hipStream_t st) {
  return with_order(pl.N, [&](auto n) {
    return launch_coeffs_n<n()>(pl, B, df, dp, times, coeffs, cost, status, st);
  });
}

hipError_t launch_time_cost(const PlanDev& pl, int64_t B, const double* df,
                            const double* times, const mtg_time_params& p,
                            double* cost, double* grad, int32_t* status,
                            hipStream_t st) {
  if (has_time_std(pl)) return launch_time_cost_std(pl, B, df, times, p, cost, grad, status, st);
  return with_order(pl.N, [&](auto n) {
    return launch_time_cost_n<n()>(pl, B, df, times, p, cost, grad, status, st);
  });
}

hipError_t launch_time_optimize(const PlanDev& pl, int64_t B, const double* df,
                                double* times, const mtg_time_params& p, int max_evals,
                                double* cost, int32_t* evals, int32_t* solves,
                                int32_t* result, int32_t* status, hipStream_t st) {
  if (has_time_std(pl))
    return launch_time_optimize_std(pl, B, df, times, p, max_evals, cost, evals, solves, result,
                                    status, st);
  return with_order(pl.N, [&](auto n) {
    return launch_time_opt_n<n()>(pl, B, df, times, p, max_evals, cost, evals, solves, result,
                                  status, st);
  });
}

hipError_t launch_segment_matrices(int N, int r, int64_t n, const double* tab,
                                   const double* times, double* Q, double* A,
                                   double* Ainv, double* H, hipStream_t st) {
  const int64_t total = n * N * N;
  const int threads = 256;
  const int64_t blocks = (total + threads - 1) / threads;
  hipLaunchKernelGGL(segment_matrices_kernel, dim3(static_cast<unsigned>(blocks)),
                     dim3(threads), 0, st, N, r, n, tab, times, Q, A, Ainv, H);
  return hipGetLastError();
}

size_t linear_lds_bytes(int N, int S, int D) { return make_layout(N, S, D).bytes(); }

#ifdef MTG_STAMPS
extern "C" int mtg_debug_stamps(unsigned long long* out, int n) {
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_mtg_stamps), sizeof(unsigned long long) * n) ==
                 hipSuccess ? 0 : -3;
}
#endif

}  // namespace mtg
