// mtg_tube_time_shared.h — what the tube QCQP time optimisers of uniform and of
// ragged batches (mtg_tube_time.hip, mtg_ragged_tube_time.hip) share: the
// dispatch-order sort, the LN_SBPLX step, the workspace carver and the small
// kernels' grid size.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "mtg_sbplx_device.h"

namespace mtg {

// The next round's dispatch order (TubeArgs::order): a counting sort of the
// trajectories by their last solve's IPM iterations, most first, the
// finished ones last.  A solve's iteration count is the best predictor of
// the next one's (consecutive points of a trajectory are close and share
// their constraints), so dispatching longest-first keeps a round's few long
// solves (up to the 100-iteration cap) from starting last and forming its
// tail.  Ties are placed in any order: results do not depend on the order.
// The body of a one-workgroup kernel of up to 1024 threads.
constexpr int kOrderKeys = 128;
__device__ __attribute__((always_inline)) inline void tube_time_order_body(
    int64_t B, const int32_t* __restrict__ iters, const int32_t* __restrict__ done,
    int32_t* __restrict__ order) {
  __shared__ int cnt[kOrderKeys], off[kOrderKeys];
  const int t = static_cast<int>(threadIdx.x);
  for (int k = t; k < kOrderKeys; k += blockDim.x) cnt[k] = 0;
  __syncthreads();
  auto key = [&](int64_t b) {
    const int it = iters[b];
    return done[b] ? 0 : 1 + (it < 0 ? 0 : (it > kOrderKeys - 2 ? kOrderKeys - 2 : it));
  };
  for (int64_t b = t; b < B; b += blockDim.x) atomicAdd(&cnt[key(b)], 1);
  __syncthreads();
  if (t == 0) {
    int run = 0;
    for (int k = kOrderKeys - 1; k >= 0; --k) {
      off[k] = run;
      run += cnt[k];
    }
  }
  __syncthreads();
  for (int64_t b = t; b < B; b += blockDim.x)
    order[atomicAdd(&off[key(b)], 1)] = static_cast<int32_t>(b);
}

// The LN_SBPLX machine (mtg_sbplx_device.h) of trajectory b in the workspace;
// State is the file's OptState (sb: the machines, sb_bytes each).
template <typename State>
__device__ inline sbplx::State* sb_state(const State& s, int64_t b) {
  return reinterpret_cast<sbplx::State*>(s.sb + static_cast<size_t>(b) * s.sb_bytes);
}

// Hand the round's J to the machine; it writes the next point into Ttr (rows
// of `stride`) or finishes.  The QCQP status of the first evaluation (T0) is
// the one reported.  The body of a kernel of one thread per trajectory.
template <typename State>
__device__ __attribute__((always_inline)) inline void tube_time_sbplx_step_body(
    int stride, int64_t B, int first, const double* __restrict__ Jall,
    const int32_t* __restrict__ qstatus, const State& s) {
  const int64_t b = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (b >= B || s.done[b]) return;
  if (first) s.st[b] = qstatus[b];
  sbplx::Machine m{sb_state(s, b)};
  m.resume(Jall[b], s.Ttr + b * stride);
  if (m.s->done) s.done[b] = 1;
}

inline unsigned blocks_for(int64_t n) { return static_cast<unsigned>((n + 255) / 256); }

// Carves a caller-owned workspace in a fixed order; each array starts on a
// 256-byte boundary.  With base == nullptr only the size is computed.
struct Carver {
  char* base;
  size_t off = 0;
  template <typename T>
  T* take(int64_t n) {
    off = (off + 255) & ~size_t(255);
    T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
    off += sizeof(T) * static_cast<size_t>(n);
    return p;
  }
};

}  // namespace mtg
