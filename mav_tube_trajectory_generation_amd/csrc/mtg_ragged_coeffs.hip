// mtg_ragged_coeffs.hip — coefficients and cost from given constraints over a
// ragged batch (include/mtg_hip.h, "Ragged coefficients from constraints"):
// mtg_coeffs_from_constraints (setFreeConstraints ->
// updateSegmentsFromCompactConstraints, linear_impl:254-275, 497-506, and
// computeCost, :113-130) for rows with their own segment count
// S_b = seg_counts[b] (device), in the padded rectangles of the other ragged
// entries.  Two vertex patterns share the one kernel body:
//   standard  fixed_vals B x D x nf_max, free_vals B x D x np_max,
//             np_max = (S_max-1)(M-1): the layouts of mtg_ragged_linear_solve
//   tube      fixed_vals B x D x N, x B x D x np_max, np_max = (S_max-1) M:
//             the layouts of mtg_ragged_tube_solve / mtg_ragged_coll_optimize;
//             with layout 1 a row is [T (S_max); d_p (D x np_max)]
// Both have closed-form slot maps in S_b (vertex_ptr), so there is no plan
// view, no map array and no workspace.
//
// One 64-lane workgroup per row; lane l of pass p is item sd = 64 p + l =
// s * D + d.  An item reads e = [d(s); d(s+1)] and forms
//   f_j = e_j T^(j mod M),  h = A(1)^-1 f,  c_i = T^-i h_i
// as stdp::Solver::coeff_cost_sd does (A(1)^-1 the exact compile-time table,
// the same operations in the same order: fed the ragged solve's free values
// it returns that solve's coefficients bit for bit), and its share of
// computeCost, 0.5 c^T Q(T) c = T^(1-2r) sum_ij g_i g_j / (i + j - 2r + 1) with
// g_i = base(r, i) h_i, as Traj::coeffs_and_cost of the uniform entry does,
// operation for operation and from the same table (the context's).  At
// N = 12 that sum cancels by seven digits and its value moves by some 1e-9
// with the order of the operations and with the last bits of the table; summed
// this way a row's cost is the uniform entry's to the rounding of the final
// sum over (s, d).  A lane adds its items' costs in pass order and the wave
// reduces by DPP, so the order of a row's sum is fixed by S_b and D alone.
//
// Stores: a row's coefficients are one run of S_max D N doubles and pass p
// owns doubles [64 N p, 64 N (p + 1)) of it.  The lanes put their N
// coefficients into LDS (64 N doubles, whatever S_max is) and the wave copies
// the chunk out as consecutive double2: each store instruction of the wave
// covers 1 KiB of consecutive addresses, and the 0.0 behind segment S_b is the
// tail of the same copy.  S_b is wave-uniform (readfirstlane) and so is every
// branch on it; no input padding is read.
#include <hip/hip_runtime.h>

#include <cmath>

#include "mtg_std_device.h"

namespace mtg {

namespace {

// Where the derivatives of vertex v of one dimension are: derivative 0 at
// p0[0], derivative k >= 1 at pk[k].
struct VertexPtr {
  const double *p0, *pk;
};

// kTube: fx = the dimension's N fixed values, fr = its (S_max-1) M free ones.
// Standard: fx = the dimension's nf_max fixed values in mtg_linear_solve's
// order, fr = its (S_max-1)(M-1) free ones.
template <int M, bool kTube>
__device__ inline VertexPtr vertex_ptr(int v, int S, const double* __restrict__ fx,
                                       const double* __restrict__ fr) {
  if (v == 0) return VertexPtr{fx, fx};
  if constexpr (kTube) {
    if (v == S) return VertexPtr{fx + M, fx + M};
    return VertexPtr{fr + (v - 1) * M, fr + (v - 1) * M};
  } else {
    if (v == S) return VertexPtr{fx + M + S - 1, fx + M + S - 1};
    return VertexPtr{fx + M + v - 1, fr + (v - 1) * (M - 1) - 1};
  }
}

}  // namespace

template <int N, int R, bool kTube>
__global__ __launch_bounds__(kWave) void ragged_coeffs_kernel(
    int D, int S_max, int layout, const int32_t* __restrict__ seg_counts,
    const double* __restrict__ tab, const double* __restrict__ fixed_vals,
    const double* __restrict__ free_vals, const double* __restrict__ times, double* __restrict__ coeffs, double* __restrict__ cost,
    double* __restrict__ times_out, int32_t* __restrict__ status) {
  constexpr int M = N / 2, MFREE = kTube ? M : M - 1;
  __shared__ __attribute__((aligned(16))) double stage[kWave * N];
  __shared__ double T_s[kWave];
  const int64_t b = blockIdx.x;
  const int lane = threadIdx.x;
  const int S = __builtin_amdgcn_readfirstlane(seg_counts[b]);
  const int per = S_max * D * N;
  const int np_max = (S_max - 1) * MFREE;
  const int nf_max = kTube ? N : 2 * M + S_max - 1;
  double* cb = coeffs + b * per;
  double* to = times_out ? times_out + b * S_max : nullptr;
  // A row that is not a trajectory: NaN over its whole padded row.
  auto fail = [&](int code) {
    for (int i = lane; i < per; i += kWave) cb[i] = NAN;
    if (to && lane < S_max) to[lane] = NAN;
    if (cost && lane == 0) cost[b] = NAN;
    if (status && lane == 0) status[b] = code;
  };
  if (S < (kTube ? 2 : 1) || S > S_max) {
    fail(MTG_TRAJ_BAD_SEGMENTS);
    return;
  }
  // layout 1: the row is [T; d_p].
  const int64_t xrow = layout ? S_max + static_cast<int64_t>(D) * np_max
                              : static_cast<int64_t>(D) * np_max;
  const double* fr = free_vals + b * xrow + (layout ? S_max : 0);
  const double* tb = layout ? free_vals + b * xrow : times + b * S_max;
  const double* fx = fixed_vals + b * D * nf_max;
  const double t_l = lane < S ? tb[lane] : 1.0;  // S <= S_max <= 64: one time per lane
  T_s[lane] = t_l;
  if (__any(!(t_l > 0.0) || !(t_l < 1e300))) {
    fail(MTG_TRAJ_BAD_TIME);
    return;
  }
  if (to && lane < S_max) to[lane] = lane < S ? t_l : 0.0;
  __syncthreads();
  const int items = S * D;
  const int valid = items * N;
  double acc = 0.0;
  for (int base = 0; base < S_max * D; base += kWave) {  // wave-uniform
    const int sd = base + lane;
    if (base < items) {  // wave-uniform: a pass with work
      if (sd < items) {
        constexpr stdp::AInvTab<N> kA{};
        const int s = sd / D, d = sd - s * D;
        const VertexPtr v0 = vertex_ptr<M, kTube>(s, S, fx + d * nf_max, fr + d * np_max);
        const VertexPtr v1 = vertex_ptr<M, kTube>(s + 1, S, fx + d * nf_max, fr + d * np_max);
        double e[N];
        e[0] = v0.p0[0];
        e[M] = v1.p0[0];
#pragma unroll
        for (int k = 1; k < M; ++k) {
          e[k] = v0.pk[k];
          e[M + k] = v1.pk[k];
        }
        const double T = T_s[s];
        const double inv = rcp64(T);
        double up[N], dn[N];  // T^e, T^-e by the chains of stdp::Solver::powers
        up[0] = dn[0] = 1.0;
#pragma unroll
        for (int i = 1; i < N; ++i) {
          up[i] = up[i - 1] * T;
          dn[i] = dn[i - 1] * inv;
        }
        double f[N], h[N];
#pragma unroll
        for (int j = 0; j < N; ++j) f[j] = e[j] * up[j % M];
        // Rows k < M of A(1)^-1 are diagonal (A(0) = diag(k!)).
#pragma unroll
        for (int i = 0; i < M; ++i) h[i] = kA.v[i * N + i] * f[i];
#pragma unroll
        for (int i = M; i < N; ++i) {
          double t = 0.0;
#pragma unroll
          for (int j = 0; j < N; ++j)
            if (kA.v[i * N + j] != 0.0) t = fma(kA.v[i * N + j], f[j], t);
          h[i] = t;
        }
        double2* o2 = reinterpret_cast<double2*>(stage + lane * N);
#pragma unroll
        for (int i = 0; i < M; ++i)
          o2[i] = make_double2(h[2 * i] * dn[2 * i], h[2 * i + 1] * dn[2 * i + 1]);
        // The cost as Traj::coeffs_and_cost sums it, operation for operation:
        // rows r.. of the context's A(1)^-1 (uniform addresses: scalar loads)
        // in one fma chain each, g_i = base(r, i) h_i, then the Hilbert form
        // sum_ij g_i g_j / (i + j - 2r + 1) by rows.
        const double* tA = tab + N * N;
        double g[N - R];
#pragma unroll
        for (int ii = 0; ii < N - R; ++ii) {
          const int i = R + ii;
          double hi = 0.0, base = 1.0;
#pragma unroll
          for (int j = 0; j < N; ++j) hi = fma(tA[i * N + j], f[j], hi);
#pragma unroll
          for (int m = 0; m < R; ++m) base *= static_cast<double>(i - m);
          g[ii] = base * hi;
        }
        double q = 0.0;
#pragma unroll
        for (int ii = 0; ii < N - R; ++ii) {
          double t = g[ii] * (1.0 / (2 * ii + 1));
#pragma unroll
          for (int jj = ii + 1; jj < N - R; ++jj) t = fma(2.0 / (ii + jj + 1), g[jj], t);
          q = fma(t, g[ii], q);
        }
        constexpr int e_cost = 1 - 2 * R;  // T^(1-2r)
        acc += q * (e_cost < 0 ? dn[-e_cost] : up[e_cost]);
      }
      __syncthreads();
    }
    // This pass's chunk of the row: staged coefficients, then 0.0.
    const int start = base * N;
    const int n_here = min(per - start, kWave * N);
    const int n_valid = valid - start;  // may be <= 0
    double2* dst = reinterpret_cast<double2*>(cb + start);
    for (int i = 2 * lane; i < n_here; i += 2 * kWave) {
      double2 v = make_double2(0.0, 0.0);
      if (i < n_valid) v = *reinterpret_cast<const double2*>(stage + i);
      dst[i >> 1] = v;
    }
    if (base + kWave < items) __syncthreads();  // wave-uniform: stage is refilled
  }
  const double J = stdp::wave_sum_dpp(acc);
  if (cost && lane == 0) cost[b] = J;
  if (status && lane == 0) status[b] = MTG_TRAJ_OK;
}

namespace {

template <int N, int R>
hipError_t ragged_coeffs_nr(const RaggedCoeffsArgs& a, hipStream_t st) {
  if (a.tube)
    return launch(ragged_coeffs_kernel<N, R, true>, a.B, kWave, 0, st, a.D, a.S_max, a.layout,
                  a.seg_counts, a.tab, a.fixed_vals, a.free_vals, a.times, a.coeffs, a.cost,
                  a.times_out, a.status);
  return launch(ragged_coeffs_kernel<N, R, false>, a.B, kWave, 0, st, a.D, a.S_max, 0,
                a.seg_counts, a.tab, a.fixed_vals, a.free_vals, a.times, a.coeffs, a.cost,
                a.times_out, a.status);
}

template <int N>
hipError_t ragged_coeffs_n(const RaggedCoeffsArgs& a, hipStream_t st) {
#define MTG_RAGGED_COEFFS_R(RR) \
  case RR:                      \
    if constexpr (RR < N / 2) return ragged_coeffs_nr<N, RR>(a, st); \
    return hipErrorInvalidValue;
  switch (a.r) {
    MTG_RAGGED_COEFFS_R(0)
    MTG_RAGGED_COEFFS_R(1)
    MTG_RAGGED_COEFFS_R(2)
    MTG_RAGGED_COEFFS_R(3)
    MTG_RAGGED_COEFFS_R(4)
    MTG_RAGGED_COEFFS_R(5)
    default: return hipErrorInvalidValue;
  }
#undef MTG_RAGGED_COEFFS_R
}

}  // namespace

hipError_t launch_ragged_coeffs(const RaggedCoeffsArgs& a, hipStream_t st) {
  if (a.S_max < 1 || a.S_max > kMaxStdS || a.D < 1 || a.D > kMaxD || !a.tab)
    return hipErrorInvalidValue;
  return with_order(a.N, [&](auto n) { return ragged_coeffs_n<n()>(a, st); });
}

}  // namespace mtg
