// mtg_ragged_tube.hip — the tube QCQP (mtg_tube.hip) for ragged batches: every
// trajectory b of one launch has its own segment count S_b = seg_counts[b]
// (device), 2 <= S_b <= S_max, in padded rectangles (include/mtg_hip.h,
// "Ragged tube QCQP"):
//   positions B x (S_max+1) x 3    the first S_b + 1 vertices
//   times_cp, times B x S_max      the first S_b
//   radii     B x S_max x 2        the first S_b
//   x         B x 3 x (S_max-1)M   row d: (S_b - 1) M values, then 0.0
//   coeffs    B x S_max x 3 x N    segments >= S_b written 0.0
//   resid     B x ncon(S_max)      ncon(S_b) values, then -inf
// Tube<N> (mtg_tube_device.h) takes S at run time and indexes every input as
// row * f(S) + i: the kernels here hand it the row's own pointers with row
// index 0 and run its setup, IPM and output arithmetic unchanged.  The LDS
// layout is carved for S_b inside the launch's allocation (the maximum of
// the layouts of 2..S_max).  S_b is workgroup-uniform (readfirstlane), so
// every branch on it is.  The host never reads the counts: a row whose count
// is out of range is reported per trajectory (MTG_TRAJ_BAD_SEGMENTS), its
// outputs NaN over the whole padded row.
#include <hip/hip_runtime.h>

#include <cmath>

#include "mtg_internal.h"
#include "mtg_tube_device.h"

namespace mtg {

namespace {

// The inputs of row b, each at its padded stride.
struct RaggedTubeRow {
  const double *positions, *fixed_vals, *times_cp, *times, *radii;
};
__device__ inline RaggedTubeRow ragged_tube_row(int64_t b, int N, int S_max,
                                                const double* __restrict__ positions,
                                                const double* __restrict__ fixed_vals,
                                                const double* __restrict__ times_cp,
                                                const double* __restrict__ times,
                                                const double* __restrict__ radii) {
  return RaggedTubeRow{positions + b * (S_max + 1) * 3, fixed_vals + b * 3 * N,
                       times_cp + b * S_max, times + b * S_max, radii + b * S_max * 2};
}

constexpr int kRaggedOrderKeys = 256;

}  // namespace

// tube_residuals_kernel<N> (mtg_tube.hip) per row with the row's own S.
template <int N>
__global__ __launch_bounds__(kWave) void ragged_tube_residuals_kernel(
    int S_max, int r, const int32_t* __restrict__ seg_counts, const double* __restrict__ tab,
    const double* __restrict__ positions, const double* __restrict__ fixed_vals,
    const double* __restrict__ times_cp, const double* __restrict__ times,
    const double* __restrict__ radii, const double* __restrict__ x, double* __restrict__ resid) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  constexpr int M = N / 2;
  const int64_t b = blockIdx.x;
  const int tid = static_cast<int>(threadIdx.x);
  const int S = __builtin_amdgcn_readfirstlane(seg_counts[b]);
  const int nc_max = tube_ncon(N, S_max);
  double* rb = resid + b * nc_max;
  if (S < 2 || S > S_max) {
    for (int k = tid; k < nc_max; k += kWave) rb[k] = NAN;
    return;
  }
  const TubeLayout L = make_tube_layout(N, S);
  Tube<N> t = make_tube<N>(&L, smem, S, r, tab);
  int* bad = reinterpret_cast<int*>(smem + L.ndouble);
  const RaggedTubeRow in =
      ragged_tube_row(b, N, S_max, positions, fixed_vals, times_cp, times, radii);
  t.setup(tab, 0, 0, in.positions, in.fixed_vals, in.times_cp, in.times, in.radii, bad);
  if (*bad & 1) {  // workgroup-uniform: setup ends on a barrier
    for (int k = tid; k < nc_max; k += kWave) rb[k] = NAN;
    return;
  }
  const int row = (S - 1) * M, row_max = (S_max - 1) * M;
  const double* xb = x + b * 3 * row_max;
  for (int idx = tid; idx < 3 * row; idx += t.nthr) {
    // reference order d*(S-1)*M + (u-1)*M + m  ->  internal ((u-1)*3+d)*M + m
    const int d = idx / row, j = idx % row, a = j / M, m = j % M;
    // positions relative to tube_origin(), as Tube::setup holds them
    const double o = m == 0 ? tube_origin(in.positions, 0, S, d) : 0.0;
    smem[L.x + (a * 3 + d) * M + m] = xb[d * row_max + j] - o;
  }
  __syncthreads();
  t.control_points(smem + L.x, L.cp);
  __syncthreads();
  for (int k = tid; k < nc_max; k += t.nthr) {
    double w[3];
    rb[k] = k < t.nc ? t.con_eval(k, L.cp, w) : -INFINITY;
  }
}

// tube_solve_one (mtg_tube_device.h) per row with the row's own S, without
// the warm start.
template <int N>
__global__ __launch_bounds__(tube_threads<N>())
__attribute__((amdgpu_waves_per_eu(tube_threads<N>() / kWave,
                                   tube_threads<N>() / kWave)))
void ragged_tube_solve_kernel(
    int S_max, int r, const int32_t* __restrict__ seg_counts, const double* __restrict__ tab,
    const double* __restrict__ positions, const double* __restrict__ fixed_vals,
    const double* __restrict__ times_cp, const double* __restrict__ times,
    const double* __restrict__ radii, double tol, int max_iter, double* __restrict__ x_out,
    double* __restrict__ coeffs, double* __restrict__ cost, int32_t* __restrict__ iters,
    int32_t* __restrict__ status, const int32_t* __restrict__ order) {
  constexpr int M = N / 2;
  // The row of this workgroup: order[blockIdx.x] (the longest rows first:
  // ragged_tube_order_kernel), else the XCD-contiguous map (mtg_device.h).
  const int64_t b = order ? order[blockIdx.x] : xcd_problem(blockIdx.x, gridDim.x);
  // A row that is not a trajectory goes through the body as two segments
  // (inside its own padded row and the launch's LDS, S_max >= 2; the values
  // are never used) instead of returning here: see tube_solve_one.
  const int Sr = __builtin_amdgcn_readfirstlane(seg_counts[b]);
  const bool valid = Sr >= 2 && Sr <= S_max;
  const RaggedTubeRow in =
      ragged_tube_row(b, N, S_max, positions, fixed_vals, times_cp, times, radii);
  tube_solve_one<N>(valid ? Sr : 2, S_max, valid, r, tab, in.positions, in.fixed_vals,
                    in.times_cp, in.times, in.radii, tol, max_iter,
                    x_out ? x_out + b * 3 * (S_max - 1) * M : nullptr,
                    coeffs + b * S_max * 3 * N, b, cost, iters, status, nullptr, nullptr,
                    &Tube<N>::ipm);
}

// The dispatch order of ragged_tube_solve_kernel: a counting sort of the rows
// by S_b, longest first, the rows whose count is out of range last (as
// tube_time_order_kernel, mtg_tube_time.hip).  A workgroup's duration grows
// with S_b and workgroups are dispatched in blockIdx order, so the long rows
// go first instead of forming the launch's tail.  Counts beyond the key range
// share the top key; ties are placed in any order: results do not depend on
// the order.
__global__ __launch_bounds__(1024) void ragged_tube_order_kernel(
    int64_t B, int S_max, const int32_t* __restrict__ seg_counts, int32_t* __restrict__ order) {
  __shared__ int cnt[kRaggedOrderKeys], off[kRaggedOrderKeys];
  const int t = static_cast<int>(threadIdx.x);
  for (int k = t; k < kRaggedOrderKeys; k += blockDim.x) cnt[k] = 0;
  __syncthreads();
  auto key = [&](int64_t b) {
    const int S = seg_counts[b];
    if (S < 2 || S > S_max) return 0;
    return S - 1 < kRaggedOrderKeys - 1 ? S - 1 : kRaggedOrderKeys - 1;
  };
  for (int64_t b = t; b < B; b += blockDim.x) atomicAdd(&cnt[key(b)], 1);
  __syncthreads();
  if (t == 0) {
    int run = 0;
    for (int k = kRaggedOrderKeys - 1; k >= 0; --k) {
      off[k] = run;
      run += cnt[k];
    }
  }
  __syncthreads();
  for (int64_t b = t; b < B; b += blockDim.x)
    order[atomicAdd(&off[key(b)], 1)] = static_cast<int32_t>(b);
}

// The layout is not monotone in S (Wb has its own slot only while
// 2 ncon < BS^2): the maximum over every count a row may have.  Stops at the
// first S beyond the limit, so the result is non-decreasing in S_max and the
// loop short whatever S_max is.
size_t ragged_tube_lds_bytes(int N, int S_max) {
  size_t best = 0;
  for (int S = 2; S <= S_max; ++S) {
    const size_t n = tube_lds_bytes(N, S);
    if (n > best) best = n;
    if (best > static_cast<size_t>(kMaxLdsBytes)) break;
  }
  return best;
}

hipError_t launch_ragged_tube_residuals(const RaggedTubeArgs& a, const double* x, double* resid,
                                        hipStream_t st) {
  return with_order(a.N, [&](auto n) {
    return launch(ragged_tube_residuals_kernel<n()>, a.B, kWave,
                  ragged_tube_lds_bytes(a.N, a.S_max), st, a.S_max, a.r, a.seg_counts, a.tab,
                  a.positions, a.fixed_vals, a.times_cp, a.times, a.radii, x, resid);
  });
}

hipError_t launch_ragged_tube_solve(const RaggedTubeArgs& a, double tol, int max_iter, double* x,
                                    double* coeffs, double* cost, int32_t* iters,
                                    int32_t* status, int32_t* order_ws, hipStream_t st) {
  if (order_ws) {
    hipLaunchKernelGGL(ragged_tube_order_kernel, dim3(1), dim3(1024), 0, st, a.B, a.S_max,
                       a.seg_counts, order_ws);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return with_order(a.N, [&](auto n) {
    return launch(ragged_tube_solve_kernel<n()>, a.B, tube_threads<n()>(),
                  ragged_tube_lds_bytes(a.N, a.S_max), st, a.S_max, a.r, a.seg_counts, a.tab,
                  a.positions, a.fixed_vals, a.times_cp, a.times, a.radii, tol, max_iter, x,
                  coeffs, cost, iters, status, static_cast<const int32_t*>(order_ws));
  });
}

}  // namespace mtg
