// mtg_ragged_eval.hip — the evaluators of a ragged batch (include/mtg_hip.h,
// "Ragged evaluators"): magnitude extrema, soft-constraint cost with a
// feasibility gate, and sampling, over the padded rectangles the ragged solve
// writes (mtg_ragged.hip):
//   seg_counts B                  S_b (device), read by the kernels only
//   coeffs     B x S_max x D x N  the first S_b segments are read
//   times      B x S_max          the first S_b are read (the rest may be NaN)
// Each row computes what the uniform kernels (mtg_extrema.hip, mtg_sample.hip)
// compute for coeffs[b, :S_b], times[b, :S_b].  S_b is loaded once per
// workgroup and made wave-uniform (readfirstlane), so every branch on it is.
// A row whose count is outside [1, S_max] writes its failure values (NaN,
// segment -1, gate +inf, n_samples -1) before anything is staged and touches
// nothing outside its own row.
#include <hip/hip_runtime.h>

#include <cmath>

#include "mtg_extrema_device.h"
#include "mtg_sample_device.h"

namespace mtg {

namespace {

__device__ inline int load_row_count(const int32_t* __restrict__ seg_counts, int64_t b) {
  return __builtin_amdgcn_readfirstlane(seg_counts[b]);
}

}  // namespace

// ---------------------------------------------------------------------------
// Extrema.  One workgroup of 1..4 whole waves per trajectory.  The row's S_b
// segments and times are staged in LDS (allocated for S_max).  Work items are
// (constraint, segment, part) with kExtParts parts always; they are dealt to
// the waves in chunks of 64 items of ONE constraint, so the switch on the
// derivative is wave-uniform and the wave-wide pruning bound (the largest
// |p^(K)|^2 at the lanes' right part ends: a value the trajectory attains)
// is valid, as in soft_cost_kernel.  A wave loops over its chunks, so
// S_b * kExtParts may exceed the workgroup.  A chunk reduces in the wave by
// (value, item): the larger value wins, the lower item wins ties, i.e. the
// chunk's first maximum in candidate order (segment, then part ascending).
// One lane per constraint then scans that constraint's chunk results in
// order with strict '>' from Extremum() = {0, 0, 0} (extremum.h:35-36,
// linear_impl:474), so "first maximum wins" holds across passes and waves.
// Lane 0 forms the cost and the gate.
constexpr int kRagExtWavesMax = 4;
constexpr int kRagExtBlockMax = kRagExtWavesMax * 64;
constexpr int kRagExtChunksMax = kMaxSoftConstraints * (kMaxStdS * kExtParts / 64);

template <int N>
__global__ __launch_bounds__(kRagExtBlockMax) void ragged_extrema_kernel(
    int D, int S_max, const int32_t* __restrict__ seg_counts, const double* __restrict__ coeffs,
    const double* __restrict__ times, SoftSpec spec, RaggedEvalOut out) {
  extern __shared__ double sm_rag[];  // S_max * (D * N + 1)
  __shared__ double cval_s[kRagExtChunksMax];
  __shared__ double ctime_s[kRagExtChunksMax];
  __shared__ int citem_s[kRagExtChunksMax];
  __shared__ double max_s[kMaxSoftConstraints];
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x;
  const int S = load_row_count(seg_counts, b);
  if (S < 1 || S > S_max) {  // workgroup-uniform
    if (tid < spec.n && out.maxima) out.maxima[b * spec.n + tid] = NAN;
    if (tid == 0) {
      if (out.max_time) out.max_time[b] = NAN;
      if (out.max_segment) out.max_segment[b] = -1;
      if (out.cost) out.cost[b] = NAN;
      if (out.gate_out) out.gate_out[b] = HUGE_VAL;
    }
    return;
  }
  const int per = S * D * N;
  double* c_s = sm_rag;
  double* T_s = sm_rag + per;
  {
    const double* cb = coeffs + b * (static_cast<int64_t>(S_max) * D * N);
    const double* tb = times + b * S_max;
    for (int i = tid; i < per; i += blockDim.x) c_s[i] = cb[i];
    for (int i = tid; i < S; i += blockDim.x) T_s[i] = tb[i];
  }
  __syncthreads();
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nwaves = blockDim.x >> 6;
  const int items = S * kExtParts;
  const int cps = (items + 63) >> 6;  // chunks per constraint
  const int nchunks = spec.n * cps;
  for (int q = wave; q < nchunks; q += nwaves) {  // wave-uniform
    const int cidx = q / cps;
    const int item = (q - cidx * cps) * 64 + lane;
    const bool active = item < items;
    const int s = active ? item >> 3 : 0, part = item & (kExtParts - 1);
    const double* c = c_s + s * D * N;
    const double T = T_s[s];
    int K = 0;
#pragma unroll
    for (int k = 0; k < kMaxSoftConstraints; ++k)  // compile-time indices
      if (k == cidx) K = spec.derivative[k];
    double best_v = -1.0, best_t = 0.0;
    ext_search_wave_bound<N>(K, c, D, T, part, kExtParts, 3, active, best_v, best_t);
    int best_i = item;
    for (int off = 32; off > 0; off >>= 1) {
      const double ov = __shfl_xor(best_v, off, 64), ot = __shfl_xor(best_t, off, 64);
      const int oi = __shfl_xor(best_i, off, 64);
      if (ov > best_v || (ov == best_v && oi < best_i)) {
        best_v = ov;
        best_t = ot;
        best_i = oi;
      }
    }
    if (lane == 0) {
      cval_s[q] = best_v;
      ctime_s[q] = best_t;
      citem_s[q] = best_i;
    }
  }
  __syncthreads();
  if (tid < spec.n) {
    double v = 0.0, t = 0.0;
    int seg = 0;
    for (int j = 0; j < cps; ++j) {
      const double x = cval_s[tid * cps + j];
      if (x > v) {
        v = x;
        t = ctime_s[tid * cps + j];
        seg = citem_s[tid * cps + j] >> 3;
      }
    }
    const double m = sqrt(v);
    max_s[tid] = m;
    if (out.maxima) out.maxima[b * spec.n + tid] = m;
    if (tid == 0) {  // time and segment of constraint 0 (mtg_ragged_max_magnitude)
      if (out.max_time) out.max_time[b] = t;
      if (out.max_segment) out.max_segment[b] = seg;
    }
  }
  if (!out.cost) return;  // workgroup-uniform
  __syncthreads();
  if (tid == 0) {
    double total = 0.0;
    bool feasible = true;
#pragma unroll
    for (int k = 0; k < kMaxSoftConstraints; ++k) {
      if (k >= spec.n) break;
      const double m = max_s[k];
      total += soft_penalty(m, spec.limit[k], spec.weight, spec.maximum_cost);
      feasible = feasible && m <= spec.limit[k];
    }
    out.cost[b] = total;
    // gate_out may alias gate_in: one load, then one store, by this lane.
    if (out.gate_out) out.gate_out[b] = feasible ? out.gate_in[b] : HUGE_VAL;
  }
}

size_t ragged_extrema_lds_bytes(int N, int S_max, int D) {
  return sizeof(double) * static_cast<size_t>(S_max) * (D * N + 1);
}

hipError_t launch_ragged_extrema(int N, int D, int S_max, int64_t B, const int32_t* seg_counts,
                                 const double* coeffs, const double* times, const SoftSpec& spec,
                                 const RaggedEvalOut& out, hipStream_t st) {
  if (S_max < 1 || S_max > kMaxStdS || spec.n < 1 || spec.n > kMaxSoftConstraints)
    return hipErrorInvalidValue;
  // As many waves as the longest possible row has chunks, four at the most.
  const int chunks = spec.n * ((S_max * kExtParts + 63) / 64);
  const int threads = 64 * (chunks < kRagExtWavesMax ? chunks : kRagExtWavesMax);
  const size_t lds = ragged_extrema_lds_bytes(N, S_max, D);
  return with_order(N, [&](auto n) {
    return launch(ragged_extrema_kernel<n()>, B, threads, lds, st, D, S_max, seg_counts, coeffs,
                  times, spec, out);
  });
}

// ---------------------------------------------------------------------------
// Sampling: sample_row (mtg_sample_device.h), the body of sample_kernel, with
// the row's own S.  One workgroup = 1024 consecutive samples of one
// trajectory, grid (ceil(n_max / 1024), B); rows are S_max apart and the LDS
// is carved for S_max; whether the pre-scaled table is used is decided from
// S_b inside it.
template <int N>
__global__ __launch_bounds__(kSampleBlock) void ragged_sample_kernel(
    int D, int S_max, const int32_t* __restrict__ seg_counts, const double* __restrict__ coeffs,
    const double* __restrict__ times, double t_start, double t_end_in, double dt, int n_max,
    int max_deriv, double* __restrict__ samples, double* __restrict__ sample_times,
    int32_t* __restrict__ n_samples) {
  extern __shared__ double dyn_rag[];
  const int64_t b = blockIdx.y;
  const int S = load_row_count(seg_counts, b);
  if (S < 1 || S > S_max) {  // workgroup-uniform; nothing staged, no sample written
    if (n_samples && blockIdx.x == 0 && threadIdx.x == 0) n_samples[b] = -1;
    return;
  }
  sample_row<N>(D, S, S_max, coeffs + b * (static_cast<int64_t>(S_max) * D * N),
                times + b * S_max, b, t_start, t_end_in, dt, n_max, max_deriv, samples,
                sample_times, n_samples, dyn_rag);
}

size_t ragged_sample_lds_bytes(int N, int S_max, int D, int max_deriv) {
  return sample_lds_bytes(N, S_max, D, max_deriv, /*shorter_rows=*/true);
}

hipError_t launch_ragged_sample(int N, int D, int S_max, int64_t B, const int32_t* seg_counts,
                                const double* coeffs, const double* times, double t_start,
                                double t_end, double dt, int n_max, int max_deriv,
                                double* samples, double* sample_times, int32_t* n_samples,
                                hipStream_t st) {
  return with_order(N, [&](auto n) {
    return launch(ragged_sample_kernel<n()>, sample_grid(n_max, B), kSampleBlock,
                  ragged_sample_lds_bytes(N, S_max, D, max_deriv), st, D, S_max, seg_counts,
                  coeffs, times, t_start, t_end, dt, n_max, max_deriv, samples, sample_times,
                  n_samples);
  });
}

}  // namespace mtg
