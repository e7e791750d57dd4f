// mtg_coll_opt.hip — the collision-driven objectives of
// PolynomialOptimizationNonLinear and a batched device optimiser over them:
// the reference demo's path (src/main.cpp:77, 104-105).
//   mode 0  objectiveFunctionFreeConstraintsAndCollision (nonlinear_impl:
//           1115-1272) over x = d_p, driver optimizeFreeConstraintsAnd
//           Collision (:495-607);
//   mode 1  objectiveFunctionFreeConstraintsAndCollisionAndTime (:1274-1535)
//           over x = [T; d_p], driver optimizeFreeConstraintsAndCollisionAnd
//           Time (:708-845).
// See include/mtg_hip.h (mtg_coll_cost / mtg_coll_optimize) for the exact
// objective, including the reference quirks it reproduces.
//
// One objective evaluation of a batch is a short chain of launches, each
// shaped for its work:
//   prep   one wave per trajectory (generic per-trajectory state,
//          mtg_device.h): times, coefficients A^-1(T) M d, J_d = 2 computeCost
//          and its gradient 2 (R_pf d_f + R_pp d_p) (no R assembled), J_t and
//          the d-fixed time differences of J_d (seg_energy_at, only segment n
//          changes);
//   walk   one 256-thread workgroup per (trajectory, walk): the collision
//          walk at T and, for the time gradient, at every perturbed T
//          (mtg_collision_device.h); the gradient walk maps dJ_c/dc to the
//          free derivatives;
//   soft   (soft constraints only) one wave per (trajectory, perturbation)
//          builds the coefficients of x +- h e_i (only the one or two
//          segments touching the perturbed vertex are recomputed), then the
//          batched extremum search of mtg_extrema.hip forms every soft cost;
//   combine one wave per trajectory: weights, the collision raise rule and
//          the gradient; in the optimiser also one step of the L-BFGS state
//          machine, which places the next evaluation point.
// The optimiser enqueues max_evals such rounds.  Every kernel first reads
// the trajectory's `done` flag, so finished trajectories cost one load per
// launch and nothing synchronises with the host.  All scratch lives in the
// caller's workspace.  The kernels' bodies are in mtg_coll_opt_device.h,
// shared with the ragged entries (mtg_ragged_coll_opt.hip).
#include <hip/hip_runtime.h>

#include <cmath>

#include "mtg_coll_opt_device.h"

namespace mtg {

namespace {

CollDims coll_dims(const PlanDev& pl, int mode, const mtg_coll_params& p) {
  return mtg::coll_dims(pl.S, pl.D, pl.np, mode, p);
}

size_t carve(void* base, const CollDims& c, int N, int64_t B, int n_soft, bool opt, CollWs* w) {
  CollCarver k{static_cast<char*>(base)};
  coll_carve(k, c, N, B, n_soft, opt, w);
  return k.off + 256;
}

// The kernels: the bodies of mtg_coll_opt_device.h on the uniform row view.
template <int N>
__global__ __launch_bounds__(kWave) void coll_prep_kernel(PlanDev pl, CollDims cd,
                                                          const double* __restrict__ fixed_vals,
                                                          const double* __restrict__ times_in,
                                                          const double* __restrict__ xsrc,
                                                          double inc, CollWs w) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int64_t b = blockIdx.x;
  if (skipped(w, b)) return;
  coll_prep_body<N>(pl, UniformRow{cd}, b, fixed_vals, times_in, xsrc, inc, w, smem);
}

template <int N>
__global__ __launch_bounds__(kCollBlock) void coll_walk_kernel(
    PlanDev pl, CollDims cd, const float* __restrict__ occ, int nx, int ny, int nz,
    const uint16_t* __restrict__ field, mtg_collision_params cp, double inc, CollWs w) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const int64_t prob = blockIdx.x;
  const int64_t b = prob / cd.P;
  const int q = static_cast<int>(prob - b * cd.P);
  if (skipped(w, b)) return;
  coll_walk_body<N>(pl, UniformRow{cd}, b, q, occ, nx, ny, nz, field, cp, inc, w, sm);
}

template <int N>
__global__ __launch_bounds__(kWave) void coll_soft_points_kernel(
    PlanDev pl, CollDims cd, const double* __restrict__ fixed_vals,
    const double* __restrict__ xsrc, double h, CollWs w) {
  const int64_t prob = blockIdx.x;
  const int64_t b = prob / cd.Q;
  const int q = static_cast<int>(prob - b * cd.Q);
  if (skipped(w, b)) return;
  coll_soft_points_body<N>(pl, UniformRow{cd}, b, q, fixed_vals, xsrc, h, w);
}

template <bool kOpt>
__global__ __launch_bounds__(kWave) void coll_combine_kernel(CollDims cd, mtg_coll_params p,
                                                             int max_evals, Bounds bd, CollWs w,
                                                             CombineOut o) {
  const int64_t b = blockIdx.x;
  if (skipped(w, b)) return;
  coll_combine_body<kOpt>(UniformRow{cd}, b, p, max_evals, bd, w, o);
}

__global__ void coll_opt_init_kernel(CollDims cd, const double* __restrict__ x0,
                                     const double* __restrict__ step, Bounds bd, CollWs w) {
  coll_opt_init_body(UniformRow{cd}, blockIdx.x, x0, step, bd, w);
}

__global__ void coll_opt_final_kernel(CollDims cd, CollWs w, double* __restrict__ x_io,
                                      double* __restrict__ cost, int32_t* __restrict__ evals,
                                      int32_t* __restrict__ result, int32_t* __restrict__ status,
                                      double* __restrict__ terms) {
  coll_opt_final_body(UniformRow{cd}, blockIdx.x, w, x_io, cost, evals, result, status, terms);
}

unsigned grid1(int64_t n) { return static_cast<unsigned>(n); }

// One objective evaluation of the batch at xsrc (B x nv) up to the combine.
template <int N>
hipError_t evaluate_n(const PlanDev& pl, const CollDims& cd, int64_t B, const double* df,
                      const double* xsrc, const double* times, const float* occ, int nx, int ny,
                      int nz, const uint16_t* field, const mtg_coll_params& p, const CollWs& w,
                      hipStream_t st) {
  const size_t lds_prep = free_lds(N, pl.S, pl.D, pl.np, false).bytes;
  hipError_t e = launch(coll_prep_kernel<N>, B, kWave, lds_prep, st, pl, cd, df, times, xsrc,
                        p.increment_time, w);
  if (e != hipSuccess) return e;
  const size_t lds_walk = collision_lds_bytes(N, pl.S);
  // With the near field one thread walks alone: one wave per walk.
  hipLaunchKernelGGL(coll_walk_kernel<N>, dim3(grid1(B * cd.P)),
                     dim3(field ? kWave : kCollBlock), lds_walk, st, pl, cd, occ, nx, ny, nz,
                     field, p.coll, p.increment_time, w);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if (cd.Q > 0) {
    hipLaunchKernelGGL(coll_soft_points_kernel<N>, dim3(grid1(B * cd.Q)), dim3(kWave), 0, st, pl,
                       cd, df, xsrc, p.coll.map_resolution, w);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    SoftSpec spec = coll_soft_spec(p);
    spec.skip = w.done;
    spec.skip_rep = cd.Q;
    e = launch_soft_cost_any(N, pl.D, pl.S, B * cd.Q, w.softc, w.softT, spec, w.softm, w.softJ,
                             st);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

hipError_t evaluate(const PlanDev& pl, const CollDims& cd, int64_t B, const double* df,
                    const double* xsrc, const double* times, const float* occ, int nx, int ny,
                    int nz, const uint16_t* field, const mtg_coll_params& p, const CollWs& w,
                    hipStream_t st) {
  return with_order(pl.N, [&](auto n) {
    return evaluate_n<n()>(pl, cd, B, df, xsrc, times, occ, nx, ny, nz, field, p, w, st);
  });
}

}  // namespace

size_t coll_workspace_bytes(const PlanDev& pl, int64_t B, int mode, const mtg_coll_params& p,
                            bool optimiser) {
  const CollDims cd = coll_dims(pl, mode, p);
  CollWs w;
  return carve(nullptr, cd, pl.N, B, p.n_soft, optimiser, &w);
}

int64_t coll_problems(const PlanDev& pl, int64_t B, int mode, const mtg_coll_params& p) {
  const CollDims cd = coll_dims(pl, mode, p);
  return B * (cd.P > cd.Q ? cd.P : cd.Q);
}

int coll_cost(const PlanDev& pl, int64_t B, int mode, const double* df, const double* x,
              const double* times, const float* occ, int nx, int ny, int nz,
              const uint16_t* field, const mtg_coll_params& p, const double* raise_ref, double* cost, double* grad,
              double* terms, int32_t* collision, int32_t* status, void* workspace,
              size_t workspace_bytes, hipStream_t st) {
  const CollDims cd = coll_dims(pl, mode, p);
  if (coll_workspace_bytes(pl, B, mode, p, false) > workspace_bytes) return MTG_ERR_INVALID_ARG;
  CollWs w;
  carve(workspace, cd, pl.N, B, p.n_soft, false, &w);
  if (evaluate(pl, cd, B, df, x, times, occ, nx, ny, nz, field, p, w, st) != hipSuccess)
    return MTG_ERR_HIP;
  const CombineOut o{raise_ref, cost, grad, terms, collision, status, nullptr};
  hipLaunchKernelGGL(coll_combine_kernel<false>, dim3(grid1(B)), dim3(kWave), 0, st, cd, p, 0,
                     Bounds{nullptr, nullptr}, w, o);
  return hipGetLastError() == hipSuccess ? MTG_OK : MTG_ERR_HIP;
}

int coll_optimize(const PlanDev& pl, int64_t B, int mode, const double* df, double* x_io,
                  const double* times, const double* lower, const double* upper,
                  const double* initial_step, const float* occ, int nx, int ny, int nz,
                  const uint16_t* field, const mtg_coll_params& p, int max_evals, double* cost, int32_t* evals,
                  int32_t* result, int32_t* status, double* terms, double* x_history,
                  void* workspace, size_t workspace_bytes, hipStream_t st) {
  const CollDims cd = coll_dims(pl, mode, p);
  if (coll_workspace_bytes(pl, B, mode, p, true) > workspace_bytes) return MTG_ERR_INVALID_ARG;
  CollWs w;
  carve(workspace, cd, pl.N, B, p.n_soft, true, &w);
  const Bounds bd{lower, upper};
  hipLaunchKernelGGL(coll_opt_init_kernel, dim3(grid1(B)), dim3(kWave), 0, st, cd, x_io,
                     initial_step, bd, w);
  if (hipGetLastError() != hipSuccess) return MTG_ERR_HIP;
  CombineOut hist{};
  hist.x_history = x_history;
  for (int round = 0; round < max_evals; ++round) {
    if (evaluate(pl, cd, B, df, w.xt, times, occ, nx, ny, nz, field, p, w, st) != hipSuccess)
      return MTG_ERR_HIP;
    hipLaunchKernelGGL(coll_combine_kernel<true>, dim3(grid1(B)), dim3(kWave), 0, st, cd, p,
                       max_evals, bd, w, hist);
    if (hipGetLastError() != hipSuccess) return MTG_ERR_HIP;
  }
  hipLaunchKernelGGL(coll_opt_final_kernel, dim3(grid1(B)), dim3(kWave), 0, st, cd, w,
                     x_io, cost, evals, result, status, terms);
  return hipGetLastError() == hipSuccess ? MTG_OK : MTG_ERR_HIP;
}

}  // namespace mtg
