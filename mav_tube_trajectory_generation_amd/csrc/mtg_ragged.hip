// mtg_ragged.hip — ragged batches of the standard vertex pattern: every
// trajectory b of one launch has its own segment count S_b = seg_counts[b]
// (device), 1 <= S_b <= S_max, in padded rectangles (include/mtg_hip.h,
// "Ragged batches"):
//   fixed_vals B x D x nf_max   row d: nf_b = 2M + S_b - 1 values at the front
//   times      B x S_max        the first S_b
//   coeffs     B x S_max x D x N   segments >= S_b written 0.0
//   free_vals  B x D x np_max   row d: (S_b - 1)(M - 1) values, then 0.0
// One 64-lane workgroup per trajectory running stdp::Solver
// (mtg_std_device.h) initialised with S_b: its LDS layout is carved for S_b
// inside the launch's allocation for S_max.  S_b is wave-uniform
// (readfirstlane), so every branch on it is.  The host never reads the
// counts: a row whose count is outside its range is reported per trajectory
// (MTG_TRAJ_BAD_SEGMENTS), its outputs NaN over the whole padded row.
// The time kernels are the drivers of mtg_time_device.h around the evaluator
// of mtg_time_std_device.h, as mtg_time_std.hip's, with row stride S_max.
#include <hip/hip_runtime.h>

#include <cmath>

#include "mtg_time_std_device.h"

namespace mtg {

namespace {

// Index of fixed value i (= d * nf + f, the order put_fixed takes) in a
// padded row of D x nf_max.
template <int D>
__device__ inline int padded_fixed_index(int i, int nf, int nf_max) {
  int d = 0;  // i / nf without an integer division (D <= 4)
#pragma unroll
  for (int d2 = 1; d2 < D; ++d2) d += i >= d2 * nf ? 1 : 0;
  return i + d * (nf_max - nf);
}

__device__ inline int load_count(const int32_t* __restrict__ seg_counts) {
  return __builtin_amdgcn_readfirstlane(seg_counts[blockIdx.x]);
}

}  // namespace

// updateSegmentTimes + solveLinear + computeCost (linear_std_kernel,
// mtg_linear_std.hip) with the trajectory's own S.
template <int N, int R, int D>
__global__ __launch_bounds__(kWave) void ragged_linear_kernel(
    int S_max, const int32_t* __restrict__ seg_counts, const double* __restrict__ tab,
    const double* __restrict__ fixed_vals, const double* __restrict__ times,
    double* __restrict__ coeffs, double* __restrict__ cost, double* __restrict__ free_vals,
    int32_t* __restrict__ status) {
  using Sv = stdp::Solver<N, R, D>;
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int64_t b = blockIdx.x;
  const int lane = threadIdx.x;
  const int nf_max = 2 * Sv::M + S_max - 1, np_max = (S_max - 1) * Sv::MF;
  const int64_t per = static_cast<int64_t>(S_max) * D * N;
  double* cb = coeffs + b * per;
  double* fv = free_vals ? free_vals + b * D * np_max : nullptr;
  const int S = load_count(seg_counts);
  // A row that is not a trajectory, or whose solve cannot run: NaN over the
  // whole padded row, nothing outside it.
  auto fail = [&](int code) {
    for (int64_t i = lane; i < per; i += kWave) cb[i] = NAN;
    if (fv)
      for (int i = lane; i < D * np_max; i += kWave) fv[i] = NAN;
    if (cost && lane == 0) cost[b] = NAN;
    if (status && lane == 0) status[b] = code;
  };
  if (S < 1 || S > S_max) {
    fail(MTG_TRAJ_BAD_SEGMENTS);
    return;
  }
  // Inputs: fixed values, times and the lane's two rows of H(1) are all
  // issued before the first use, as in linear_std_kernel.
  Sv sv;
  sv.init(S, smem, nullptr);
  const int nf = sv.nf;
  const double* tb = times + b * S_max;
  const double* fb = fixed_vals + b * D * nf_max;
  const double f_l = fb[padded_fixed_index<D>(lane < D * nf ? lane : D * nf - 1, nf, nf_max)];
  const double t_raw = tb[lane < S ? lane : S - 1];
  const double t_l = lane < S ? t_raw : 1.0;
  // S = 1: no intermediate vertex, so no system: the table rows, the middle
  // terms, assembly and elimination are all skipped.
  const bool chain = S > 1;
  if (chain) {
    sv.load_first_rows(tab);
    sv.clear_mid_terms();
  }
  if (lane < D * nf) sv.put_fixed(lane, f_l);
  for (int i = lane + kWave; i < D * nf; i += kWave)
    sv.put_fixed(i, fb[padded_fixed_index<D>(i, nf, nf_max)]);
  bool bad = lane < S ? sv.powers(lane, t_l) : false;
  for (int s = lane + kWave; s < S; s += kWave) bad = sv.powers(s, tb[s]) || bad;
  const bool bad_time = __any(bad);
  __syncthreads();
  if (bad_time) {
    fail(MTG_TRAJ_BAD_TIME);
    return;
  }
  bool not_spd = false;
  if (chain) {
    sv.assemble(tab);
    __syncthreads();
    not_spd = sv.solve();
  }
  // S = 1: both vertices are fixed, dv holds them from put_fixed.
  const double J = sv.coeff_cost(cb);
  for (int64_t i = static_cast<int64_t>(S) * D * N + lane; i < per; i += kWave) cb[i] = 0.0;
  if (cost && lane == 0) cost[b] = J;
  if (fv && np_max > 0) {
    const int np = (S - 1) * Sv::MF;
    for (int i = lane; i < D * np_max; i += kWave) {
      const int d = i / np_max, p = i % np_max;
      const int v = p / Sv::MF + 1, kk = p % Sv::MF + 1;
      fv[i] = p < np ? sv.dv()[(v * D + d) * Sv::MP + kk] : 0.0;
    }
  }
  if (status && lane == 0) status[b] = not_spd ? MTG_TRAJ_NOT_SPD : MTG_TRAJ_OK;
}

namespace {

// d_f of a padded row into the solver (all lanes).
template <int N, int R, int D>
__device__ void ragged_load_fixed(StdSv<N, R, D>& sv, const double* __restrict__ fb,
                                  int nf_max) {
  const int nf = sv.nf;
  for (int i = sv.lane; i < D * nf; i += kWave)
    sv.put_fixed(i, fb[padded_fixed_index<D>(i, nf, nf_max)]);
}

// The time entries take 2 <= S_b <= S_max (a one-variable LN_SBPLX run is
// not pinned to the oracle).
__device__ inline bool time_count_ok(int S, int S_max) { return S >= 2 && S <= S_max; }

}  // namespace

// objectiveFunctionTime / getCostAndGradientTime (time_cost_std_kernel,
// mtg_time_std.hip) with the trajectory's own S; grad rows padded with 0.0.
template <int N, int R, int D>
__global__ __launch_bounds__(kWave) void ragged_time_cost_kernel(
    int S_max, const int32_t* __restrict__ seg_counts, const double* __restrict__ tab,
    const double* __restrict__ fixed_vals, const double* __restrict__ times, mtg_time_params p,
    double* __restrict__ cost, double* __restrict__ grad, int32_t* __restrict__ status) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int64_t b = blockIdx.x;
  const int lane = threadIdx.x;
  const int S = load_count(seg_counts);
  double* gb = grad && p.grad_mode != 0 ? grad + b * S_max : nullptr;
  if (!time_count_ok(S, S_max)) {
    if (gb)
      for (int i = lane; i < S_max; i += kWave) gb[i] = NAN;
    if (cost && lane == 0) cost[b] = NAN;
    if (status && lane == 0) status[b] = MTG_TRAJ_BAD_SEGMENTS;
    return;
  }
  StdEval<N, D, false, StdSv<N, R, D>> ev;
  ev.init(S, smem, tab);
  ragged_load_fixed(ev, fixed_vals + b * D * (N + S_max - 1), N + S_max - 1);
  time_cost_drive(ev, S, S_max, tab, nullptr, times, p, cost, grad, status);
  if (gb)
    for (int i = S + lane; i < S_max; i += kWave) gb[i] = 0.0;
}

// optimizeTime (time_optimize_std_kernel, mtg_time_std.hip) with the
// trajectory's own S; times_io entries >= S_b are not written.
template <int N, int R, int D>
__global__ __launch_bounds__(kWave) void ragged_time_optimize_kernel(
    int S_max, const int32_t* __restrict__ seg_counts, const double* __restrict__ tab,
    const double* __restrict__ fixed_vals, double* __restrict__ times_io, mtg_time_params p,
    int max_evals, double* __restrict__ cost, int32_t* __restrict__ evals_out,
    int32_t* __restrict__ solves_out, int32_t* __restrict__ result_out,
    int32_t* __restrict__ status) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int64_t b = blockIdx.x;
  const int S = load_count(seg_counts);
  if (!time_count_ok(S, S_max)) {
    if (threadIdx.x == 0) {
      if (cost) cost[b] = NAN;
      if (evals_out) evals_out[b] = 0;
      if (solves_out) solves_out[b] = 0;
      if (result_out) result_out[b] = sbplx::kFailure;
      if (status) status[b] = MTG_TRAJ_BAD_SEGMENTS;
    }
    return;
  }
  StdEval<N, D, false, StdSv<N, R, D>> ev;
  ev.init(S, smem, tab);
  auto* sbs = reinterpret_cast<sbplx::State*>(
      reinterpret_cast<char*>(smem) + (time_std_bytes(N, S, D, false) + 15) / 16 * 16);
  ragged_load_fixed(ev, fixed_vals + b * D * (N + S_max - 1), N + S_max - 1);
  time_optimize_drive(ev, S, S_max, tab, nullptr, times_io, p, max_evals, cost, evals_out,
                      solves_out, result_out, status, sbs);
}

size_t ragged_linear_lds_bytes(int N, int S_max, int D) {
  return sizeof(double) * static_cast<size_t>(stdp::layout(N, S_max, D).n);
}

size_t ragged_time_lds_bytes(int N, int S_max, int D, bool optimiser) {
  const size_t base = time_std_bytes(N, S_max, D, false);
  return optimiser ? (base + 15) / 16 * 16 + sbplx::state_bytes(S_max) : base;
}

bool has_ragged_time(const RaggedDev& pl) {
  return pl.N == 10 && pl.r >= 2 && pl.r <= 4 && pl.D >= 1 && pl.D <= 3;
}

namespace {

template <int N, int R, int D>
hipError_t ragged_linear_nrd(const RaggedDev& pl, int64_t B, const int32_t* seg,
                             const double* df, const double* times, double* coeffs,
                             double* cost, double* free_vals, int32_t* status, hipStream_t st) {
  return launch(ragged_linear_kernel<N, R, D>, B, kWave,
                ragged_linear_lds_bytes(N, pl.S_max, D), st, pl.S_max, seg, pl.tab, df, times,
                coeffs, cost, free_vals, status);
}

template <int N, int R>
hipError_t ragged_linear_nr(const RaggedDev& pl, int64_t B, const int32_t* seg, const double* df,
                            const double* times, double* coeffs, double* cost,
                            double* free_vals, int32_t* status, hipStream_t st) {
  switch (pl.D) {
    case 1: return ragged_linear_nrd<N, R, 1>(pl, B, seg, df, times, coeffs, cost, free_vals, status, st);
    case 2: return ragged_linear_nrd<N, R, 2>(pl, B, seg, df, times, coeffs, cost, free_vals, status, st);
    case 3: return ragged_linear_nrd<N, R, 3>(pl, B, seg, df, times, coeffs, cost, free_vals, status, st);
    case 4: return ragged_linear_nrd<N, R, 4>(pl, B, seg, df, times, coeffs, cost, free_vals, status, st);
    default: return hipErrorInvalidValue;
  }
}

template <int N>
hipError_t ragged_linear_n(const RaggedDev& pl, int64_t B, const int32_t* seg, const double* df,
                           const double* times, double* coeffs, double* cost, double* free_vals,
                           int32_t* status, hipStream_t st) {
#define MTG_RAGGED_R(RR)                                                                  \
  case RR:                                                                               \
    if constexpr (RR < N / 2)                                                            \
      return ragged_linear_nr<N, RR>(pl, B, seg, df, times, coeffs, cost, free_vals,     \
                                     status, st);                                        \
    return hipErrorInvalidValue;
  switch (pl.r) {
    MTG_RAGGED_R(0)
    MTG_RAGGED_R(1)
    MTG_RAGGED_R(2)
    MTG_RAGGED_R(3)
    MTG_RAGGED_R(4)
    MTG_RAGGED_R(5)
    default: return hipErrorInvalidValue;
  }
#undef MTG_RAGGED_R
}

template <int N, int R, int D>
hipError_t ragged_time_cost_nrd(const RaggedDev& pl, int64_t B, const int32_t* seg,
                                const double* df, const double* times, const mtg_time_params& p,
                                double* cost, double* grad, int32_t* status, hipStream_t st) {
  return launch(ragged_time_cost_kernel<N, R, D>, B, kWave,
                ragged_time_lds_bytes(N, pl.S_max, D, false), st, pl.S_max, seg, pl.tab, df,
                times, p, cost, grad, status);
}

template <int N, int R, int D>
hipError_t ragged_time_opt_nrd(const RaggedDev& pl, int64_t B, const int32_t* seg,
                               const double* df, double* times, const mtg_time_params& p,
                               int max_evals, double* cost, int32_t* evals, int32_t* solves,
                               int32_t* result, int32_t* status, hipStream_t st) {
  return launch(ragged_time_optimize_kernel<N, R, D>, B, kWave,
                ragged_time_lds_bytes(N, pl.S_max, D, true), st, pl.S_max, seg, pl.tab, df,
                times, p, max_evals, cost, evals, solves, result, status);
}

#define MTG_RAGGED_TIME_DISPATCH(FN, ...)                       \
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

}  // namespace

hipError_t launch_ragged_linear_solve(const RaggedDev& pl, int64_t B, const int32_t* seg_counts,
                                      const double* df, const double* times, double* coeffs,
                                      double* cost, double* free_vals, int32_t* status,
                                      hipStream_t st) {
  return with_order(pl.N, [&](auto n) {
    return ragged_linear_n<n()>(pl, B, seg_counts, df, times, coeffs, cost, free_vals, status,
                                st);
  });
}

hipError_t launch_ragged_time_cost(const RaggedDev& pl, int64_t B, const int32_t* seg_counts,
                                   const double* df, const double* times,
                                   const mtg_time_params& p, double* cost, double* grad,
                                   int32_t* status, hipStream_t st) {
  if (!has_ragged_time(pl)) return hipErrorInvalidValue;
  MTG_RAGGED_TIME_DISPATCH(ragged_time_cost_nrd, pl, B, seg_counts, df, times, p, cost, grad,
                           status, st)
}

hipError_t launch_ragged_time_optimize(const RaggedDev& pl, int64_t B, const int32_t* seg_counts,
                                       const double* df, double* times,
                                       const mtg_time_params& p, int max_evals, double* cost,
                                       int32_t* evals, int32_t* solves, int32_t* result,
                                       int32_t* status, hipStream_t st) {
  if (!has_ragged_time(pl)) return hipErrorInvalidValue;
  MTG_RAGGED_TIME_DISPATCH(ragged_time_opt_nrd, pl, B, seg_counts, df, times, p, max_evals, cost,
                           evals, solves, result, status, st)
}

}  // namespace mtg
