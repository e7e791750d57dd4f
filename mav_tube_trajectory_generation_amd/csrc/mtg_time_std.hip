// mtg_time_std.hip — the time-allocation objective and the batched
// segment-time optimiser (objectiveFunctionTime / getCostAndGradientTime /
// optimizeTime, nonlinear_impl:877-945, 2495-2584, 332-397) for the standard
// vertex pattern, on the standard-pattern solver (stdp::Solver,
// mtg_std_device.h) or its compile-time-S form (wave::Solver,
// mtg_wave_device.h).  The gradient modes and the optimiser are the shared
// drivers of mtg_time_device.h, which the generic kernels (mtg_kernels.hip:
// time_cost_kernel, time_optimize_kernel) run too; this file holds the
// objective and its evaluator.  Instantiated for N = 10, r = 2..4, D = 1..3
// (other combinations run the generic kernels).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdlib>

#include "mtg_extrema_device.h"
#include "mtg_sbplx_device.h"
#include "mtg_std_device.h"
#include "mtg_time_device.h"
#include "mtg_wave_device.h"

namespace mtg {

namespace {

template <int N, int R, int D>
using StdSv = stdp::Solver<N, R, D>;

// The inner solve and computeCost at the times T (LDS) on either solver:
// stdp::Solver (runtime S) or wave::Solver (compile-time S, the C2 design).
// Every lane calls; *bad is set (and NaN returned) when a time is invalid;
// with cbuf the coefficients go there (LDS, soft searches).
template <int N, int R, int D>
__device__ __attribute__((always_inline)) double solve_cost(
    stdp::Solver<N, R, D>& sv, const double* __restrict__ tab, const double* T, double* cbuf,
    bool reload_rows, bool* bad, bool* not_spd) {
  __syncthreads();
  const bool b = sv.powers_from(T);
  __syncthreads();
  if (b) {
    *bad = true;
    return NAN;
  }
  // soft: the H(1) rows are reloaded per evaluation (L2 hits), so they are
  // not live across the extremum searches.
  if (reload_rows) sv.load_first_rows(tab);
  sv.assemble(tab);
  __syncthreads();
  *not_spd = sv.solve() || *not_spd;
  return sv.coeff_cost(cbuf);
}

template <int N, int R, int D, int S>
__device__ __attribute__((always_inline)) double solve_cost(
    wave::Solver<N, R, D, S>& sv, const double* __restrict__ /*tab*/, const double* T,
    double* cbuf, bool /*reload_rows*/, bool* bad, bool* not_spd) {
  __syncthreads();
  const int l = sv.lane;
  const double t = T[l < S ? l : S - 1];
  if (__any(l < S && (!(t > 0.0) || !(t < 1e300)))) {
    *bad = true;
    return NAN;
  }
  *not_spd = sv.solve(T) || *not_spd;
  return sv.coeff_cost(T, cbuf);
}

// J(T) = computeCost() + time_penalty (sum T)^2 [+ soft constraints] at the
// times T (LDS, S values).  Every lane calls it; returns the wave-uniform J
// (NaN and *bad set when a time is invalid).  kSoft: the coefficients go to
// cbuf (LDS) and evaluateMaximumMagnitudeAsSoftConstraint
// (nonlinear_impl:2735-2766) runs one extremum search per constraint; with
// p.hard_constraints the searches give *viol = max(0, max_c (max_c - limit_c
// - tolerance)) (evaluateMaximumMagnitudeConstraint, :2687-2733) instead of
// a cost term.
template <int N, int D, bool kSoft, class SV>
__device__ __attribute__((always_inline)) double std_objective(SV& sv, const double* __restrict__ tab,
                                const double* T, int S, const mtg_time_params& p, double* cbuf,
                                bool* bad, bool* not_spd, double* viol) {
  *viol = 0.0;
  unsigned long long tt = 0;
  MTG_TACC(511, tt);
  double J = solve_cost(sv, tab, T, kSoft ? cbuf : nullptr, kSoft, bad, not_spd);
  if (*bad) return NAN;
  double tot = 0.0;
  for (int i = 0; i < S; ++i) tot += T[i];  // nonlinear_impl:2768-2774
  J += tot * tot * p.time_penalty;
  MTG_TACC(450, tt);  // diagnostic: solve + coefficients
  if constexpr (kSoft) {
    __syncthreads();
    // Every constraint's maximum in one pass (ext_soft_maxima_wave).
    int Ks[kMaxSoftConstraints];
    int kmin = 4;
#pragma unroll
    for (int cc = 0; cc < kMaxSoftConstraints; ++cc) {
      Ks[cc] = p.soft_derivative[cc];
      if (cc < p.n_soft && Ks[cc] < kmin) kmin = Ks[cc];
    }
    double* scratch = cbuf + S * D * N;
    double* maxima = scratch + kMaxSoftConstraints * (N + 1);
    ext_soft_maxima_wave_k<N>(kmin, cbuf, T, S, D, sv.lane, p.n_soft, Ks, scratch, maxima);
    double soft = 0.0;
    for (int c = 0; c < p.n_soft; ++c) {
      double lim = 1.0;
#pragma unroll
      for (int cc = 0; cc < kMaxSoftConstraints; ++cc)  // compile-time indices
        if (cc == c) lim = p.soft_limit[cc];
      const double m = maxima[c];
      if (p.hard_constraints) {
        *viol = fmax(*viol, m - lim - p.hard_tolerance);
      } else {
        const double relative_violation = (m - lim) / lim;
        soft += fmin(p.soft_maximum_cost, exp(relative_violation * p.soft_weight));
      }
      MTG_TACC(451 + c, tt);  // diagnostic
    }
    J += soft;
  }
  return J;
}

// Loads d_f (and, for wave::Solver, H(1)) into the solver (all lanes).
template <int N, int R, int D>
__device__ void std_load_fixed(StdSv<N, R, D>& sv, const double* __restrict__ /*tab*/,
                               const double* __restrict__ fb) {
  const int nf = sv.nf;
  for (int i = sv.lane; i < D * nf; i += kWave) sv.put_fixed(i, fb[i]);
}
template <int N, int R, int D, int S>
__device__ void std_load_fixed(wave::Solver<N, R, D, S>& sv, const double* __restrict__ tab,
                               const double* __restrict__ fb) {
  sv.load_constants(tab, fb);
  wave::lds_order();
}

// The evaluator of the shared drivers (mtg_time_device.h): either solver
// with the drivers' hooks.  The evaluation point and the drivers' state share
// the solver's aux() region.
template <int N, int D, bool kSoft, class SV>
struct StdEval : SV {
  bool bad_ = false, not_spd_ = false;
  __device__ __attribute__((always_inline)) double* T() const { return this->aux(); }
  __device__ __attribute__((always_inline)) double* state(int S) const {
    return this->aux() + S;
  }
  __device__ __attribute__((always_inline)) double eval(int S, const double* __restrict__ tab,
                                                        double* cbuf, const mtg_time_params& p,
                                                        double* viol) {
    SV& sv = *this;
    return std_objective<N, D, kSoft>(sv, tab, T(), S, p, cbuf, &bad_, &not_spd_, viol);
  }
  __device__ __attribute__((always_inline)) bool bad() const { return bad_; }
  __device__ __attribute__((always_inline)) bool not_spd() const { return not_spd_; }
  // getCostAndGradientTime (nonlinear_impl:2495-2584): d held at the base
  // solution, only segment n's block of J_d = d^T R d changes.  One lane per
  // segment energy, 2S of them into E.
  __device__ __attribute__((always_inline)) void fixed_d_gradient(
      int S, const double* Tb, const mtg_time_params& p, double* g, double* E) {
    const int lane = this->lane;
    const double inc = p.increment;
    for (int i = lane; i < 2 * S; i += kWave) {
      const int n = i >> 1;
      E[i] = this->seg_energy(n, fd_time(Tb[n], i, inc));
    }
    __syncthreads();
    for (int n = lane; n < S; n += kWave)
      g[n] = p.w_d * (E[2 * n + 1] - E[2 * n]) / (2.0 * inc) + p.w_t * 1.0;
    __syncthreads();
  }
};

}  // namespace

__host__ __device__ inline size_t time_std_bytes(int N, int S, int D, bool soft) {
  const size_t base = sizeof(double) * static_cast<size_t>(stdp::layout(N, S, D).n);
  // soft: the coefficients (S x D x N), then the soft searches' scratch and
  // maxima (ext_soft_maxima_wave).
  return soft ? (base + 15) / 16 * 16 +
                    sizeof(double) * (S * D * N + kMaxSoftConstraints * (N + 2))
              : base;
}
size_t time_std_lds_bytes(int N, int S, int D, bool soft) { return time_std_bytes(N, S, D, soft); }
// The optimiser kernels add the LN_SBPLX machine's state after that.
static size_t time_std_opt_lds_bytes(int N, int S, int D, bool soft) {
  return (time_std_bytes(N, S, D, soft) + 15) / 16 * 16 + sbplx::state_bytes(S);
}

// objectiveFunctionTime / getCostAndGradientTime on one trajectory per
// workgroup: time_cost_drive (mtg_time_device.h) around std_objective.
template <int N, int R, int D, bool kSoft>
__global__ __launch_bounds__(kWave) void time_cost_std_kernel(
    int S, const double* __restrict__ tab, const double* __restrict__ fixed_vals,
    const double* __restrict__ times, mtg_time_params p, double* __restrict__ cost,
    double* __restrict__ grad, int32_t* __restrict__ status) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  StdEval<N, D, kSoft, StdSv<N, R, D>> ev;
  ev.init(S, smem, tab);
  std_load_fixed(ev, tab, fixed_vals + static_cast<int64_t>(blockIdx.x) * D * (N + S - 1));
  time_cost_drive(ev, S, tab, smem + (ev.L.n + 1) / 2 * 2, times, p, cost, grad, status);
}

// The same on the compile-time-S solver (N = 10, r = 4, D = 3, S = 2..16).
template <int N, int R, int D, int S, bool kSoft>
__global__ __launch_bounds__(kWave) void time_cost_wave_kernel(
    const double* __restrict__ tab, const double* __restrict__ fixed_vals,
    const double* __restrict__ times, mtg_time_params p, double* __restrict__ cost,
    double* __restrict__ grad, int32_t* __restrict__ status) {
  using G = wave::Geo<N, R, D, S>;
  constexpr int CB = kSoft ? S * D * N + kMaxSoftConstraints * (N + 2) : 0;
  __shared__ __attribute__((aligned(16))) double sm[G::L_N + CB];
  StdEval<N, D, kSoft, wave::Solver<N, R, D, S>> ev;
  ev.init(sm);
  std_load_fixed(ev, tab, fixed_vals + static_cast<int64_t>(blockIdx.x) * D * (N + S - 1));
  time_cost_drive(ev, S, tab, sm + G::L_N, times, p, cost, grad, status);
}

// Batched segment-time optimisation (optimizeTime, nonlinear_impl:332-397):
// time_optimize_drive (mtg_time_device.h) around std_objective.
template <int N, int R, int D, bool kSoft>
__global__ __launch_bounds__(kWave) void time_optimize_std_kernel(
    int S, const double* __restrict__ tab, const double* __restrict__ fixed_vals,
    double* __restrict__ times_io, mtg_time_params p, int max_evals,
    double* __restrict__ cost, int32_t* __restrict__ evals_out, int32_t* __restrict__ solves_out,
    int32_t* __restrict__ result_out, int32_t* __restrict__ status) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  StdEval<N, D, kSoft, StdSv<N, R, D>> ev;
  ev.init(S, smem, tab);
  auto* sbs = reinterpret_cast<sbplx::State*>(
      reinterpret_cast<char*>(smem) + (time_std_bytes(N, S, D, kSoft) + 15) / 16 * 16);
  std_load_fixed(ev, tab, fixed_vals + static_cast<int64_t>(blockIdx.x) * D * (N + S - 1));
  time_optimize_drive(ev, S, tab, smem + (ev.L.n + 1) / 2 * 2, times_io, p, max_evals, cost,
                      evals_out, solves_out, result_out, status, sbs);
}

// The same on the compile-time-S solver (N = 10, r = 4, D = 3, S = 2..16).
template <int N, int R, int D, int S, bool kSoft>
__global__ __launch_bounds__(kWave) void time_optimize_wave_kernel(
    const double* __restrict__ tab, const double* __restrict__ fixed_vals,
    double* __restrict__ times_io, mtg_time_params p, int max_evals,
    double* __restrict__ cost, int32_t* __restrict__ evals_out, int32_t* __restrict__ solves_out,
    int32_t* __restrict__ result_out, int32_t* __restrict__ status) {
  using G = wave::Geo<N, R, D, S>;
  constexpr int CB = kSoft ? S * D * N + kMaxSoftConstraints * (N + 2) : 0;
  constexpr int SB = static_cast<int>(sbplx::state_bytes(S) / sizeof(double));
  __shared__ __attribute__((aligned(16))) double sm[(G::L_N + CB + 1) / 2 * 2 + SB];
  StdEval<N, D, kSoft, wave::Solver<N, R, D, S>> ev;
  ev.init(sm);
  std_load_fixed(ev, tab, fixed_vals + static_cast<int64_t>(blockIdx.x) * D * (N + S - 1));
  time_optimize_drive(ev, S, tab, sm + G::L_N, times_io, p, max_evals, cost, evals_out,
                      solves_out, result_out, status,
                      reinterpret_cast<sbplx::State*>(sm + (G::L_N + CB + 1) / 2 * 2));
}

namespace {
template <int N, int R, int D>
hipError_t time_cost_nrd(const PlanDev& pl, int64_t B, const double* df, const double* times,
                         const mtg_time_params& p, double* cost, double* grad, int32_t* status,
                         hipStream_t st) {
  return with_soft(p.n_soft > 0, [&](auto soft) {
    return launch(time_cost_std_kernel<N, R, D, decltype(soft)::value>, B, kWave,
                  time_std_lds_bytes(N, pl.S, D, soft), st, pl.S, pl.tab, df, times, p, cost, grad,
                  status);
  });
}

template <int N, int R, int D>
hipError_t time_opt_nrd(const PlanDev& pl, int64_t B, const double* df, double* times,
                        const mtg_time_params& p, int max_evals, double* cost, int32_t* evals,
                        int32_t* solves, int32_t* result, int32_t* status, hipStream_t st) {
  return with_soft(p.n_soft > 0, [&](auto soft) {
    return launch(time_optimize_std_kernel<N, R, D, decltype(soft)::value>, B, kWave,
                  time_std_opt_lds_bytes(N, pl.S, D, soft), st, pl.S, pl.tab, df, times, p,
                  max_evals, cost, evals, solves, result, status);
  });
}

// The compile-time-S kernels hold their LDS statically.
template <int S>
hipError_t time_cost_wave_s(const PlanDev& pl, int64_t B, const double* df, const double* times,
                            const mtg_time_params& p, double* cost, double* grad,
                            int32_t* status, hipStream_t st) {
  return with_soft(p.n_soft > 0, [&](auto soft) {
    return launch(time_cost_wave_kernel<10, 4, 3, S, decltype(soft)::value>, B, kWave, 0, st,
                  pl.tab, df, times, p, cost, grad, status);
  });
}

template <int S>
hipError_t time_opt_wave_s(const PlanDev& pl, int64_t B, const double* df, double* times,
                           const mtg_time_params& p, int max_evals, double* cost, int32_t* evals,
                           int32_t* solves, int32_t* result, int32_t* status, hipStream_t st) {
  return with_soft(p.n_soft > 0, [&](auto soft) {
    return launch(time_optimize_wave_kernel<10, 4, 3, S, decltype(soft)::value>, B, kWave, 0, st,
                  pl.tab, df, times, p, max_evals, cost, evals, solves, result, status);
  });
}

// The compile-time-S kernels where the C2 kernel exists (MTG_STD_RUNTIME_S=1
// forces the runtime-S ones, for A/B runs; launch_linear_solve_std reads the
// same switch).
bool use_time_wave(const PlanDev& pl) {
  static const bool forced = [] {
    const char* e = std::getenv("MTG_STD_RUNTIME_S");
    return e && e[0] == '1';
  }();
  return has_linear_wave(pl) && !forced;
}

#define MTG_TIME_WAVE_DISPATCH(FN, ...)                                                      \
  switch (pl.S) {                                                                            \
    case 2: return FN<2>(__VA_ARGS__);   case 3: return FN<3>(__VA_ARGS__);                   \
    case 4: return FN<4>(__VA_ARGS__);   case 5: return FN<5>(__VA_ARGS__);                   \
    case 6: return FN<6>(__VA_ARGS__);   case 7: return FN<7>(__VA_ARGS__);                   \
    case 8: return FN<8>(__VA_ARGS__);   case 9: return FN<9>(__VA_ARGS__);                   \
    case 10: return FN<10>(__VA_ARGS__); case 11: return FN<11>(__VA_ARGS__);                 \
    case 12: return FN<12>(__VA_ARGS__); case 13: return FN<13>(__VA_ARGS__);                 \
    case 14: return FN<14>(__VA_ARGS__); case 15: return FN<15>(__VA_ARGS__);                 \
    case 16: return FN<16>(__VA_ARGS__);                                                     \
    default: return hipErrorInvalidValue;                                                    \
  }
}  // namespace

bool has_time_std(const PlanDev& pl) {
  return use_std_kernel(pl) && pl.N == 10 && pl.r >= 2 && pl.r <= 4 && pl.D >= 1 && pl.D <= 3;
}

#define MTG_TIME_STD_DISPATCH(FN, ...)                          \
  switch (pl.r * 4 + pl.D) {                                    \
    case 2 * 4 + 1: return FN<10, 2, 1>(__VA_ARGS__);           \
    case 2 * 4 + 2: return FN<10, 2, 2>(__VA_ARGS__);           \
    case 2 * 4 + 3: return FN<10, 2, 3>(__VA_ARGS__);           \
    case 3 * 4 + 1: return FN<10, 3, 1>(__VA_ARGS__);           \
    case 3 * 4 + 2: return FN<10, 3, 2>(__VA_ARGS__);           \
    case 3 * 4 + 3: return FN<10, 3, 3>(__VA_ARGS__);           \
    case 4 * 4 + 1: return FN<10, 4, 1>(__VA_ARGS__);           \
    case 4 * 4 + 2: return FN<10, 4, 2>(__VA_ARGS__);           \
    case 4 * 4 + 3: return FN<10, 4, 3>(__VA_ARGS__);           \
    default: return hipErrorInvalidValue;                       \
  }

hipError_t launch_time_cost_std(const PlanDev& pl, int64_t B, const double* df,
                                const double* times, const mtg_time_params& p, double* cost,
                                double* grad, int32_t* status, hipStream_t st) {
  if (!has_time_std(pl)) return hipErrorInvalidValue;
  if (use_time_wave(pl))
    MTG_TIME_WAVE_DISPATCH(time_cost_wave_s, pl, B, df, times, p, cost, grad, status, st)
  MTG_TIME_STD_DISPATCH(time_cost_nrd, pl, B, df, times, p, cost, grad, status, st)
}

hipError_t launch_time_optimize_std(const PlanDev& pl, int64_t B, const double* df,
                                    double* times, const mtg_time_params& p, int max_evals,
                                    double* cost, int32_t* evals, int32_t* solves,
                                    int32_t* result, int32_t* status, hipStream_t st) {
  if (!has_time_std(pl)) return hipErrorInvalidValue;
  if (use_time_wave(pl))
    MTG_TIME_WAVE_DISPATCH(time_opt_wave_s, pl, B, df, times, p, max_evals, cost, evals, solves,
                           result, status, st)
  MTG_TIME_STD_DISPATCH(time_opt_nrd, pl, B, df, times, p, max_evals, cost, evals, solves, result,
                        status, st)
}

}  // namespace mtg

#ifdef MTG_STAMPS
// This translation unit's stamps (the soft searches' per-lane counters).
extern "C" int mtg_debug_stamps_time(unsigned long long* out, int n) {
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_mtg_stamps),
                             sizeof(unsigned long long) * n) == hipSuccess ? 0 : -3;
}
#endif
