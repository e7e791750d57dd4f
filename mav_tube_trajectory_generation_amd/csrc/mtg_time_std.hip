// mtg_time_std.hip — the time-allocation objective and the batched
// segment-time optimiser (objectiveFunctionTime / getCostAndGradientTime /
// optimizeTime, nonlinear_impl:877-945, 2495-2584, 332-397) for the standard
// vertex pattern, on the standard-pattern solver (stdp::Solver,
// mtg_std_device.h) or its compile-time-S form (wave::Solver,
// mtg_wave_device.h).  The gradient modes and the optimiser are the shared
// drivers of mtg_time_device.h, which the generic kernels (mtg_kernels.hip:
// time_cost_kernel, time_optimize_kernel) run too; the objective and its
// evaluator are in mtg_time_std_device.h, shared with the ragged kernels
// (mtg_ragged.hip).  Instantiated for N = 10, r = 2..4, D = 1..3 (other
// combinations run the generic kernels).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdlib>

#include "mtg_time_std_device.h"

namespace mtg {

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
  time_cost_drive(ev, S, S, tab, smem + (ev.L.n + 1) / 2 * 2, times, p, cost, grad, status);
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
  time_cost_drive(ev, S, S, tab, sm + G::L_N, times, p, cost, grad, status);
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
  time_optimize_drive(ev, S, S, tab, smem + (ev.L.n + 1) / 2 * 2, times_io, p, max_evals, cost,
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
  time_optimize_drive(ev, S, S, tab, sm + G::L_N, times_io, p, max_evals, cost, evals_out,
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
