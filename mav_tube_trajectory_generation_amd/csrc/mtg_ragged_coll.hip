// mtg_ragged_coll.hip — the collision walk over a ragged batch
// (include/mtg_hip.h, mtg_ragged_collision_cost), over the padded rectangles
// the ragged solve writes (mtg_ragged.hip):
//   seg_counts B                  S_b (device), read by the kernel only
//   coeffs     B x S_max x 3 x N  the first S_b segments are read
//   times      B x S_max          the first S_b are read (the rest may be NaN)
// Each row runs collision_walk (mtg_collision_device.h) with S = S_b, so its
// cost, flag and coefficient gradient are those of collision_cost_kernel for
// coeffs[b, :S_b], times[b, :S_b].  S_b is loaded once per workgroup and made
// wave-uniform (readfirstlane), so every branch on it is.  With a near field
// the workgroup is one wave (one load per evaluated sample); without it,
// kCollBlock threads scan every evaluated sample's box.  The walk also hands
// out the first colliding sample (kHitLoc), and lane 0 forms the gate.  A row
// whose count is outside [1, S_max] writes its failure values before anything
// is staged and touches nothing outside its own row.
//
// The kernel is compiled per (gradient, near field): the gate-only launch
// (grad_coeffs null) carries none of the walk's gradient code, and the
// workgroup size is a constant.
//
// LDS, sized by S_max: c_s S_max x 3 x N, T_s S_max, then with a gradient
// g_s S_max x 3 x N and the walk's whole scratch; a gate-only launch has
// neither g_s nor the scratch's gradient rows, which the walk touches under
// `grad` alone.  The collision parameters, the output pointers and the
// tail's two sizes wait in LDS as well (kStaticLds bytes): the walk keeps
// about a hundred wave-uniform values alive, and with these 40 more in SGPRs
// for its whole length the kernels spilled 12 to 20 SGPRs and took 144
// VGPRs.  Read from LDS where they are used, no kernel spills; the gate-only
// kernels take 110 VGPRs and the gradient ones 126 to 130 (tools/
// kernel_regs.py).
#include <hip/hip_runtime.h>

#include <cmath>

#include "mtg_collision_device.h"

namespace mtg {

constexpr size_t kStaticLds = sizeof(mtg_collision_params) + sizeof(RaggedCollOut) +
                              2 * sizeof(int);

// The walk's scratch without its gradient rows (the last kWave x (N + 6)).
__host__ __device__ constexpr int coll_scratch_doubles_no_grad(int N) {
  return coll_scratch_doubles(N) - kWave * (N + 6);
}

template <int N, bool kGrad, bool kField>
__global__ __launch_bounds__(kField ? kWave : kCollBlock) void ragged_collision_kernel(
    int S_max, const int32_t* __restrict__ seg_counts, const double* __restrict__ coeffs,
    const double* __restrict__ times, const float* __restrict__ occ, int nx, int ny, int nz,
    const uint16_t* __restrict__ field, mtg_collision_params p, RaggedCollOut out) {
  constexpr int D = 3;
  constexpr int nthr = kField ? kWave : kCollBlock;
  extern __shared__ __attribute__((aligned(16))) double sm_rc[];
  __shared__ mtg_collision_params p_s;
  __shared__ RaggedCollOut out_s;
  __shared__ int size_s[2];  // row, per for the tail
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x;
  const int row = S_max * D * N;
  const int S = __builtin_amdgcn_readfirstlane(seg_counts[b]);
  if (S < 1 || S > S_max) {  // workgroup-uniform
    if constexpr (kGrad)
      for (int i = tid; i < row; i += nthr) out.grad_coeffs[b * row + i] = NAN;
    if (tid == 0) {
      if (out.cost) out.cost[b] = NAN;
      if (out.collision) out.collision[b] = -1;
      if (out.hit_segment) out.hit_segment[b] = -1;
      if (out.hit_time) out.hit_time[b] = NAN;
      if (out.gate_out) out.gate_out[b] = HUGE_VAL;
    }
    return;
  }
  const int per = S * D * N;
  double* c_s = sm_rc;      // S_max x D x N, the first S staged
  double* T_s = c_s + row;  // S_max
  double* g_s = kGrad ? T_s + S_max : nullptr;  // S_max x D x N dJ/dc
  double* scratch = T_s + S_max + (kGrad ? row : 0);
  {
    const double* cb = coeffs + b * row;
    const double* tb = times + b * S_max;
    for (int i = tid; i < per; i += nthr) {
      c_s[i] = cb[i];
      if constexpr (kGrad) g_s[i] = 0.0;
    }
    for (int i = tid; i < S; i += nthr) T_s[i] = tb[i];
  }
  if (tid == 0) {  // field by field: a struct copy goes through private memory
    p_s.map_resolution = p.map_resolution;
    for (int k = 0; k < 3; ++k) {
      p_s.min_bound[k] = p.min_bound[k];
      p_s.max_bound[k] = p.max_bound[k];
    }
    p_s.epsilon = p.epsilon;
    p_s.robot_radius = p.robot_radius;
    p_s.coll_pot_multiplier = p.coll_pot_multiplier;
    p_s.coll_check_time_increment = p.coll_check_time_increment;
    p_s.box_side = p.box_side;
    size_s[0] = row;
    size_s[1] = per;
    out_s.cost = out.cost;
    out_s.collision = out.collision;
    out_s.hit_segment = out.hit_segment;
    out_s.hit_time = out.hit_time;
    out_s.grad_coeffs = out.grad_coeffs;
    out_s.gate_in = out.gate_in;
    out_s.gate_out = out.gate_out;
  }
  __syncthreads();
  double J;
  bool hit;
  collision_walk<N, true>(S, c_s, T_s, occ, nx, ny, nz, p_s, kGrad, g_s, scratch, &J, &hit,
                          kField ? field : nullptr);
  if (tid == 0) {
    if (out_s.cost) out_s.cost[b] = J;
    if (out_s.collision) out_s.collision[b] = hit ? 1 : 0;
    if (out_s.hit_segment) out_s.hit_segment[b] = hit ? static_cast<int32_t>(scratch[4]) : -1;
    if (out_s.hit_time) out_s.hit_time[b] = hit ? scratch[5] : NAN;
    // gate_out may alias gate_in: one load, then one store, by this lane.
    if (out_s.gate_out) out_s.gate_out[b] = hit ? HUGE_VAL : out_s.gate_in[b];
  }
  // On a collision the gradient keeps the terms accumulated before it, as
  // collision_cost_kernel; the padding segments are written 0.0.
  if constexpr (kGrad) {
    const int n_row = size_s[0], n_per = size_s[1];
    double* gb = out_s.grad_coeffs + b * n_row;
    for (int i = tid; i < n_row; i += nthr) gb[i] = i < n_per ? g_s[i] : 0.0;
  }
}

size_t ragged_collision_lds_bytes(int N, int S_max, bool grad) {
  const size_t row = static_cast<size_t>(S_max) * 3 * N;
  return sizeof(double) * (grad ? 2 * row + S_max + coll_scratch_doubles(N)
                                : row + S_max + coll_scratch_doubles_no_grad(N)) +
         kStaticLds;
}

hipError_t launch_ragged_collision(int N, int S_max, int64_t B, const int32_t* seg_counts,
                                   const double* coeffs, const double* times, const float* occ,
                                   int nx, int ny, int nz, const uint16_t* field,
                                   const mtg_collision_params& p, const RaggedCollOut& out,
                                   hipStream_t st) {
  if (S_max < 1 || S_max > kMaxStdS) return hipErrorInvalidValue;
  const bool grad = out.grad_coeffs != nullptr;
  const size_t lds = ragged_collision_lds_bytes(N, S_max, grad) - kStaticLds;  // the dynamic part
  // With the near field one thread walks alone: one wave per row.
  return with_order(N, [&](auto n) {  // with_soft: true_type / false_type by a flag
    return with_soft(grad, [&](auto g) {
      return with_soft(field != nullptr, [&](auto f) {
        constexpr bool kField = decltype(f)::value;
        return launch(ragged_collision_kernel<n(), decltype(g)::value, kField>, B,
                      kField ? kWave : kCollBlock, lds, st, S_max, seg_counts, coeffs, times, occ,
                      nx, ny, nz, field, p, out);
      });
    });
  });
}

}  // namespace mtg
