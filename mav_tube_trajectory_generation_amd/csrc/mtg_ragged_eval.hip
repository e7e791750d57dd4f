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
    double best_v = -1.0, best_t = 0.0, mv = 0.0, mt = 0.0;
#define MTG_RAG_SEARCH(k)                                                                 \
  {                                                                                       \
    double lb = active ? ext_mag2<N, k>(c, D, ldexp(T * (part + 1), -3)) : 0.0;           \
    for (int off = 32; off > 0; off >>= 1) lb = fmax(lb, __shfl_xor(lb, off, 64));        \
    if (active) ext_segment_search<N, k>(c, D, T, part, kExtParts, 3, best_v, best_t, mv, mt, lb); \
  }
    switch (K) {
      case 0: MTG_RAG_SEARCH(0) break;
      case 1: MTG_RAG_SEARCH(1) break;
      case 2: MTG_RAG_SEARCH(2) break;
      case 3:
        if constexpr (N >= 5) MTG_RAG_SEARCH(3)
        break;
      case 4:
        if constexpr (N >= 6) MTG_RAG_SEARCH(4)
        break;
      default: break;
    }
#undef MTG_RAG_SEARCH
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
      const double relative_violation = (m - spec.limit[k]) / spec.limit[k];
      total += fmin(spec.maximum_cost, exp(relative_violation * spec.weight));
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
#define CALL(n)                                                                               \
  return launch(ragged_extrema_kernel<n>, B, threads, lds, st, D, S_max, seg_counts, coeffs, \
                times, spec, out)
  switch (N) {
    case 4: CALL(4);
    case 6: CALL(6);
    case 8: CALL(8);
    case 10: CALL(10);
    case 12: CALL(12);
    default: return hipErrorInvalidValue;
  }
#undef CALL
}

// ---------------------------------------------------------------------------
// Sampling: sample_kernel (mtg_sample.hip) with the row's own S.  One
// workgroup = 1024 consecutive samples of one trajectory, grid
// (ceil(n_max / 1024), B); rows are S_max apart; whether the pre-scaled
// table base(dv, j) * c[seg][d][j] is used is decided from S_b, inside the
// LDS allocated for S_max.
namespace {

constexpr int kRagSampleBlock = 256;
constexpr int kRagSamplesPerLane = 4;
constexpr int kRagScaledMax = 4096;  // doubles of pre-scaled coefficients in LDS
typedef double rag_v2d __attribute__((ext_vector_type(2)));  // 16-byte non-temporal stores

// base(n, i) = i! / (i-n)! (polynomial.cpp:145-161), i >= n.
__device__ inline double rag_falling(int n, int i) {
  double p = 1.0;
  for (int m = 0; m < n; ++m) p *= static_cast<double>(i - m);
  return p;
}

inline int rag_scaled_doubles(int N, int D, int S_max, int max_deriv) {
  const int64_t all = static_cast<int64_t>(S_max) * (max_deriv + 1) * D * N;
  return static_cast<int>(all < kRagScaledMax ? all : kRagScaledMax);
}

}  // namespace

template <int N>
__global__ __launch_bounds__(kRagSampleBlock) void ragged_sample_kernel(
    int D, int S_max, const int32_t* __restrict__ seg_counts, const double* __restrict__ coeffs,
    const double* __restrict__ times, double t_start, double t_end_in, double dt, int n_max,
    int max_deriv, double* __restrict__ samples, double* __restrict__ sample_times,
    int32_t* __restrict__ n_samples) {
  // Dynamic LDS carved for S_max: coefficients, segment times, base table,
  // pre-scaled table ([seg][dv][d][j], min(S_max nK D N, kRagScaledMax)).
  extern __shared__ double dyn_rag[];
  double* c_s = dyn_rag;
  double* T_s = c_s + S_max * D * N;
  double* base_s = T_s + S_max;
  double* cs_s = base_s + N * N;
  __shared__ double seg0_s[2];  // start segment's accumulated start, time in it
  __shared__ int i0_s;
  __shared__ int cnt_s;
  const int64_t b = blockIdx.y;
  const int tid = threadIdx.x;
  const int S = load_row_count(seg_counts, b);
  if (S < 1 || S > S_max) {  // workgroup-uniform; nothing staged, no sample written
    if (n_samples && blockIdx.x == 0 && tid == 0) n_samples[b] = -1;
    return;
  }
  const int per = S * D * N;
  {
    const double* cb = coeffs + b * (static_cast<int64_t>(S_max) * D * N);
    const double* tb = times + b * S_max;
    for (int i = tid; i < per; i += kRagSampleBlock) c_s[i] = cb[i];
    for (int i = tid; i < S; i += kRagSampleBlock) T_s[i] = tb[i];
  }
  for (int i = tid; i < N * N; i += kRagSampleBlock) {
    const int n = i / N, j = i % N;
    base_s[i] = j >= n ? rag_falling(n, j) : 0.0;
  }
  __syncthreads();
  const int nK = max_deriv + 1;
  const bool scaled = S * nK * D * N <= kRagScaledMax;
  if (scaled) {
    for (int i = tid; i < S * nK * D * N; i += kRagSampleBlock) {
      const int j = i % N, d = (i / N) % D, dv = (i / (N * D)) % nK, seg = i / (N * D * nK);
      cs_s[i] = base_s[dv * N + j] * c_s[(seg * D + d) * N + j];
    }
  }
  if (tid == 0) {
    cnt_s = 0;
    // Start segment: first i with accumulated end > t_start (:88-103).
    double acc = 0.0;
    int i = 0;
    for (i = 0; i < S; ++i) {
      acc += T_s[i];
      if (acc > t_start) break;
    }
    if (t_start > acc || i >= S) {
      i0_s = -1;
    } else {
      acc -= T_s[i];
      i0_s = i;
      seg0_s[0] = acc;            // accumulated_time of the first sample
      seg0_s[1] = t_start - acc;  // time_in_segment of the first sample
    }
  }
  __syncthreads();
  const int i0 = i0_s;
  double t_end = t_end_in;
  if (t_end < 0.0) {  // the row's whole trajectory
    t_end = 0.0;
    for (int i = 0; i < S; ++i) t_end += T_s[i];
  }
  const int nch = (max_deriv + 1) * D;
  const int64_t out0 = b * static_cast<int64_t>(nch) * n_max;
  int nvalid = 0;
  // Sample k's segment and time in it by the reference's rule (the valid
  // samples form a prefix of 0 .. n_max-1).
  auto locate = [&](int k, int* seg_o, double* tin_o, double* acc_o) {
    bool valid = false;
    int seg = 0;
    double tin = 0.0, acc = 0.0;
    if (i0 >= 0 && k < n_max) {
      acc = seg0_s[0] + static_cast<double>(k) * dt;
      tin = seg0_s[1] + static_cast<double>(k) * dt;
      seg = i0;
      while (seg < S && tin > T_s[seg]) {
        tin -= T_s[seg];
        ++seg;
      }
      valid = acc < t_end && seg < S;
    }
    *seg_o = seg;
    *tin_o = tin;
    *acc_o = acc;
    return valid;
  };
  if (scaled && (n_max & 1) == 0) {
    // Two consecutive samples per lane and 16-byte stores; rows start at
    // even sample offsets (n_max even).
    for (int rep = 0; rep < kRagSamplesPerLane / 2; ++rep) {
      const int k = blockIdx.x * kRagSamplesPerLane * kRagSampleBlock +
                    rep * 2 * kRagSampleBlock + 2 * tid;
      int sg0, sg1;
      double tn0, tn1, ac0, ac1;
      const bool v0 = locate(k, &sg0, &tn0, &ac0);
      const bool v1 = locate(k + 1, &sg1, &tn1, &ac1);
      if (v0) {
        const double* cs0 = cs_s + sg0 * nK * D * N;
        const double* cs1 = cs_s + (v1 ? sg1 : sg0) * nK * D * N;
        double* o_row = samples + out0 + k;
#pragma unroll
        for (int dv = 0; dv < N; ++dv) {
          if (dv >= nK) break;
#pragma unroll
          for (int d = 0; d < kMaxD; ++d) {
            if (d >= D) break;
            const double* c0 = cs0 + (dv * D + d) * N;
            const double* c1 = cs1 + (dv * D + d) * N;
            double a = c0[N - 1], c = c1[N - 1];
#pragma unroll
            for (int j = N - 2; j >= dv; --j) {
              a = fma(a, tn0, c0[j]);
              c = fma(c, tn1, c1[j]);
            }
            double* o = o_row + static_cast<int64_t>(dv * D + d) * n_max;
            if (v1)  // streamed once: non-temporal stores
              __builtin_nontemporal_store(rag_v2d{a, c}, reinterpret_cast<rag_v2d*>(o));
            else
              __builtin_nontemporal_store(a, o);
          }
        }
        if (sample_times) {
          double* o = sample_times + b * static_cast<int64_t>(n_max) + k;
          if (v1)
            __builtin_nontemporal_store(rag_v2d{ac0, ac1}, reinterpret_cast<rag_v2d*>(o));
          else
            __builtin_nontemporal_store(ac0, o);
        }
      }
      nvalid += (v0 ? 1 : 0) + (v1 ? 1 : 0);
    }
  } else {
    for (int rep = 0; rep < kRagSamplesPerLane; ++rep) {
      const int k = (blockIdx.x * kRagSamplesPerLane + rep) * kRagSampleBlock + tid;
      int seg;
      double tin, acc;
      const bool valid = locate(k, &seg, &tin, &acc);
      if (valid && scaled) {
        const double* cs = cs_s + seg * nK * D * N;
        double* o_row = samples + out0 + k;
#pragma unroll
        for (int dv = 0; dv < N; ++dv) {
          if (dv >= nK) break;
#pragma unroll
          for (int d = 0; d < kMaxD; ++d) {
            if (d >= D) break;
            const double* cd = cs + (dv * D + d) * N;
            double v = cd[N - 1];
#pragma unroll
            for (int j = N - 2; j >= dv; --j) v = fma(v, tin, cd[j]);
            __builtin_nontemporal_store(v, o_row + static_cast<int64_t>(dv * D + d) * n_max);
          }
        }
        if (sample_times)
          __builtin_nontemporal_store(acc, sample_times + b * static_cast<int64_t>(n_max) + k);
      } else if (valid) {
        const double* c = c_s + seg * D * N;
        for (int dv = 0; dv <= max_deriv; ++dv) {
          const double* bs = base_s + dv * N;
          for (int d = 0; d < D; ++d) {
            const double* cd = c + d * N;
            double v = bs[N - 1] * cd[N - 1];
#pragma unroll
            for (int j = N - 2; j >= 0; --j)
              if (j >= dv) v = fma(v, tin, bs[j] * cd[j]);
            samples[out0 + static_cast<int64_t>(dv * D + d) * n_max + k] = v;
          }
        }
        if (sample_times) sample_times[b * static_cast<int64_t>(n_max) + k] = acc;
      }
      nvalid += valid ? 1 : 0;
    }
  }
  // Count: the valid samples are a prefix of 0..n_max-1, so exactly one
  // workgroup sees the end of the prefix (or holds sample n_max-1 with all
  // valid, or is workgroup 0 with none valid) and writes the count.
  if (n_samples) {
    for (int off = 32; off > 0; off >>= 1) nvalid += __shfl_xor(nvalid, off, 64);
    if ((tid & 63) == 0 && nvalid) atomicAdd(&cnt_s, nvalid);
    __syncthreads();
    if (tid == 0) {
      const int k0 = blockIdx.x * kRagSamplesPerLane * kRagSampleBlock;
      const int kend = min(k0 + kRagSamplesPerLane * kRagSampleBlock, n_max);
      const int cnt = cnt_s;
      // Is sample k0-1 (last of the previous workgroup) valid?
      bool prev_valid = false;
      if (k0 > 0) {
        int seg;
        double tin, acc;
        prev_valid = locate(k0 - 1, &seg, &tin, &acc);
      }
      if (cnt < kend - k0) {
        if (cnt > 0 || k0 == 0 || prev_valid) n_samples[b] = k0 + cnt;
      } else if (kend == n_max) {
        n_samples[b] = n_max;
      }
    }
  }
}

size_t ragged_sample_lds_bytes(int N, int S_max, int D, int max_deriv) {
  return sizeof(double) * (static_cast<size_t>(S_max) * (D * N + 1) + N * N +
                           rag_scaled_doubles(N, D, S_max, max_deriv));
}

hipError_t launch_ragged_sample(int N, int D, int S_max, int64_t B, const int32_t* seg_counts,
                                const double* coeffs, const double* times, double t_start,
                                double t_end, double dt, int n_max, int max_deriv,
                                double* samples, double* sample_times, int32_t* n_samples,
                                hipStream_t st) {
  const int per_block = kRagSampleBlock * kRagSamplesPerLane;
  const dim3 grid(static_cast<unsigned>((n_max + per_block - 1) / per_block),
                  static_cast<unsigned>(B));
  const size_t bytes = ragged_sample_lds_bytes(N, S_max, D, max_deriv);
#define CALL(n)                                                                              \
  {                                                                                          \
    const hipError_t e = prepare_lds(ragged_sample_kernel<n>, bytes);                        \
    if (e != hipSuccess) return e;                                                           \
    hipLaunchKernelGGL(ragged_sample_kernel<n>, grid, dim3(kRagSampleBlock), bytes, st, D,   \
                       S_max, seg_counts, coeffs, times, t_start, t_end, dt, n_max, max_deriv, \
                       samples, sample_times, n_samples);                                    \
    return hipGetLastError();                                                                \
  }
  switch (N) {
    case 4: CALL(4)
    case 6: CALL(6)
    case 8: CALL(8)
    case 10: CALL(10)
    case 12: CALL(12)
    default: return hipErrorInvalidValue;
  }
#undef CALL
}

}  // namespace mtg
