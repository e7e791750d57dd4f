// mtg_ragged_coll_opt.hip — the collision-driven objectives and their projected
// L-BFGS (mtg_coll_opt.hip) for ragged batches of the tube pattern: trajectory
// b has its own segment count S_b = seg_counts[b] (device), 2 <= S_b <= S_max,
// its start and end vertex fix derivatives 0..M-1 and every intermediate
// derivative is free, the pattern whose free values mtg_ragged_tube_solve
// returns as x (include/mtg_hip.h, "Ragged collision objectives").
//
// The launch chain is that of mtg_coll_opt.hip and so is every body
// (mtg_coll_opt_device.h, on the RaggedRow view): prep, walk, soft points,
// extremum search, combine, and init / final around the optimiser's rounds.
// What differs is only where a row's data sits:
//   - each workgroup builds its row's CollDims from seg_counts[b]; the grids
//     are sized for S_max (B x P_max walks, B x Q_max soft problems) and a
//     workgroup past the row's own P_b or Q_b returns after one load;
//   - the state in the workspace is compact at the front of rows carved for
//     S_max (S_b times, then 3 np_b values), so the L-BFGS sums partition
//     over the lanes as in the uniform kernel; only the caller's arrays (x,
//     grad, bounds, steps, history) are padded, through RaggedRow::ext;
//   - the pattern's maps (slots, free_map, fixed_map) of every count
//     2..S_max are written into the workspace by the first kernel of a call;
//   - the soft-points kernel writes each problem's count beside its
//     coefficients (0 for a slot that is not live) and the ragged extremum
//     kernel (mtg_ragged_eval.hip) searches the live ones.
// The host never reads the counts, nothing allocates or synchronises, and
// every workspace word is written in the same call before it is read.
#include <hip/hip_runtime.h>

#include <cmath>

#include "mtg_coll_opt_device.h"

namespace mtg {

namespace {

// What every kernel of a call needs to build its row.
struct RaggedColl {
  int N, r, S_max;
  CollDims mx;                 // the dimensions at S_max: the rows of the workspace
  const int32_t* seg_counts;   // B (device)
  const double* tab;           // H(1), A(1)^-1 for (N, r)
  int32_t* maps;               // (S_max - 1) x map_ints(N, S_max), count S at S - 2
};

__host__ __device__ inline int map_ints(int N, int S_max) {
  const int M = N / 2;
  return (S_max + 1) * M + (S_max - 1) * M + N;  // slots, free_map, fixed_map
}

__device__ inline bool count_ok(int S, int S_max) { return S >= 2 && S <= S_max; }

__device__ inline int row_count(const RaggedColl& a, int64_t b) {
  return __builtin_amdgcn_readfirstlane(a.seg_counts[b]);
}

__device__ inline RaggedRow make_row(const RaggedColl& a, int S) {
  RaggedRow row{a.mx, a.mx};
  coll_dims_sizes(row.cd, S, (S - 1) * (a.N / 2));
  return row;
}

// The plan view of the tube pattern at S segments (nf = N fixed values per
// dimension, np = (S - 1) M free ones), its maps from the workspace.
__device__ inline PlanDev row_plan(const RaggedColl& a, int S) {
  const int M = a.N / 2;
  PlanDev pl{};
  pl.N = a.N;
  pl.D = 3;
  pl.r = a.r;
  pl.S = S;
  pl.nf = a.N;
  pl.np = (S - 1) * M;
  pl.tab = a.tab;
  const int32_t* mp = a.maps + (S - 2) * map_ints(a.N, a.S_max);
  pl.slots = mp;
  pl.free_map = mp + (a.S_max + 1) * M;
  pl.fixed_map = pl.free_map + (a.S_max - 1) * M;
  pl.use_mask = (S + 1) * M <= 64;
  const uint64_t ends = (uint64_t(1) << M) - 1;
  pl.fmask = pl.use_mask ? (ends | (ends << (S * M))) : 0;
  return pl;
}

// The maps of the tube pattern for S = 2 + blockIdx.x: free p <-> slot M + p,
// fixed f < M <-> slot f, fixed f >= M <-> slot S M + f - M.
__global__ void ragged_coll_maps_kernel(RaggedColl a) {
  const int M = a.N / 2;
  const int S = 2 + static_cast<int>(blockIdx.x);
  int32_t* slots = a.maps + (S - 2) * map_ints(a.N, a.S_max);
  int32_t* free_map = slots + (a.S_max + 1) * M;
  int32_t* fixed_map = free_map + (a.S_max - 1) * M;
  const int t = threadIdx.x, nt = blockDim.x;
  for (int i = t; i < (S + 1) * M; i += nt) {
    const int v = i / M, k = i - v * M;
    slots[i] = v == 0 ? k : (v == S ? M + k : -((v - 1) * M + k + 1));
  }
  for (int p = t; p < (S - 1) * M; p += nt) free_map[p] = M + p;
  for (int f = t; f < a.N; f += nt) fixed_map[f] = f < M ? f : S * M + f - M;
}

// The cost entry's point: the caller's padded row into the compact state.
__global__ __launch_bounds__(kWave) void ragged_coll_gather_kernel(RaggedColl a,
                                                                   const double* __restrict__ x,
                                                                   CollWs w) {
  const int64_t b = blockIdx.x;
  const int S = row_count(a, b);
  if (!count_ok(S, a.S_max)) return;
  const RaggedRow row = make_row(a, S);
  const int nv = row.cd.nv, rnv = row.mx.nv;
  for (int i = threadIdx.x; i < nv; i += kWave) w.xt[b * rnv + i] = x[b * rnv + row.ext(i)];
}

template <int N>
__global__ __launch_bounds__(kWave) void ragged_coll_prep_kernel(
    RaggedColl a, const double* __restrict__ fixed_vals, const double* __restrict__ times_in,
    double inc, CollWs w) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int64_t b = blockIdx.x;
  const int S = row_count(a, b);
  if (!count_ok(S, a.S_max) || skipped(w, b)) return;
  coll_prep_body<N>(row_plan(a, S), make_row(a, S), b, fixed_vals, times_in, w.xt, inc, w, smem);
}

template <int N>
__global__ __launch_bounds__(kCollBlock) void ragged_coll_walk_kernel(
    RaggedColl a, const float* __restrict__ occ, int nx, int ny, int nz,
    const uint16_t* __restrict__ field, mtg_collision_params cp, double inc, CollWs w) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const int64_t prob = blockIdx.x;
  const int64_t b = prob / a.mx.P;
  const int q = static_cast<int>(prob - b * a.mx.P);
  const int S = row_count(a, b);
  if (!count_ok(S, a.S_max)) return;
  const RaggedRow row = make_row(a, S);
  if (q >= row.cd.P || skipped(w, b)) return;
  coll_walk_body<N>(row_plan(a, S), row, b, q, occ, nx, ny, nz, field, cp, inc, w, sm);
}

// softn[b Q_max + q]: S_b where the problem's coefficients are written and are
// to be searched, 0 elsewhere (past the row's Q_b, a finished row, a bad count
// or a bad time), which the ragged extremum kernel turns away at once.
template <int N>
__global__ __launch_bounds__(kWave) void ragged_coll_soft_points_kernel(
    RaggedColl a, const double* __restrict__ fixed_vals, double h, CollWs w,
    int32_t* __restrict__ softn) {
  const int64_t prob = blockIdx.x;
  const int64_t b = prob / a.mx.Q;
  const int q = static_cast<int>(prob - b * a.mx.Q);
  const int S = row_count(a, b);
  bool live = count_ok(S, a.S_max) && !skipped(w, b);
  RaggedRow row{};
  if (live) {
    row = make_row(a, S);
    live = q < row.cd.Q && w.st[b] == MTG_TRAJ_OK;
  }
  if (threadIdx.x == 0) softn[prob] = live ? S : 0;
  if (!live) return;
  coll_soft_points_body<N>(row_plan(a, S), row, b, q, fixed_vals, w.xt, h, w);
}

template <bool kOpt>
__global__ __launch_bounds__(kWave) void ragged_coll_combine_kernel(RaggedColl a,
                                                                    mtg_coll_params p,
                                                                    int max_evals, Bounds bd,
                                                                    CollWs w, CombineOut o) {
  const int64_t b = blockIdx.x;
  const int lane = threadIdx.x;
  const int S = row_count(a, b);
  const int rnv = a.mx.nv;
  if (!count_ok(S, a.S_max)) {
    if constexpr (!kOpt) {
      if (o.grad)
        for (int j = lane; j < rnv; j += kWave) o.grad[b * rnv + j] = NAN;
      if (lane == 0) {
        if (o.cost) o.cost[b] = NAN;
        if (o.terms)
          for (int z = 0; z < 4; ++z) o.terms[b * 4 + z] = NAN;
        if (o.collision) o.collision[b] = -1;
        if (o.status) o.status[b] = MTG_TRAJ_BAD_SEGMENTS;
      }
    }
    return;
  }
  if (skipped(w, b)) return;
  const RaggedRow row = make_row(a, S);
  // The padding of the row this launch writes: 0.0.
  double* out_row = kOpt ? (o.x_history ? o.x_history + (b * max_evals + w.evals[b]) * rnv
                                        : nullptr)
                         : (o.grad ? o.grad + b * rnv : nullptr);
  if (out_row)
    for (int j = lane; j < rnv; j += kWave)
      if (row.padding(j)) out_row[j] = 0.0;
  coll_combine_body<kOpt>(row, b, p, max_evals, bd, w, o);
}

// A row whose count is out of range never starts: it is done from the outset
// and the final kernel writes its failure values.
__global__ __launch_bounds__(kWave) void ragged_coll_opt_init_kernel(
    RaggedColl a, const double* __restrict__ x0, const double* __restrict__ step, Bounds bd,
    CollWs w) {
  const int64_t b = blockIdx.x;
  const int S = row_count(a, b);
  if (!count_ok(S, a.S_max)) {
    if (threadIdx.x == 0) w.done[b] = 1;
    return;
  }
  coll_opt_init_body(make_row(a, S), b, x0, step, bd, w);
}

__global__ __launch_bounds__(kWave) void ragged_coll_opt_final_kernel(
    RaggedColl a, CollWs w, double* __restrict__ x_io, double* __restrict__ cost,
    int32_t* __restrict__ evals, int32_t* __restrict__ result, int32_t* __restrict__ status,
    double* __restrict__ terms) {
  const int64_t b = blockIdx.x;
  const int S = row_count(a, b);
  if (!count_ok(S, a.S_max)) {
    if (threadIdx.x == 0) {
      if (cost) cost[b] = NAN;
      if (evals) evals[b] = 0;
      if (result) result[b] = -1;  // FAILURE
      if (status) status[b] = MTG_TRAJ_BAD_SEGMENTS;
      if (terms)
        for (int z = 0; z < 4; ++z) terms[b * 4 + z] = NAN;
    }
    return;
  }
  coll_opt_final_body(make_row(a, S), b, w, x_io, cost, evals, result, status, terms);
}

struct Workspace {
  CollWs w;
  int32_t* softn;  // B x Q_max
  int32_t* maps;
};

size_t carve(void* base, const CollDims& mx, int N, int S_max, int64_t B, int n_soft, bool opt,
             Workspace* ws) {
  CollCarver k{static_cast<char*>(base)};
  coll_carve(k, mx, N, B, n_soft, opt, &ws->w);
  ws->softn = k.take<int32_t>(B * mx.Q);
  ws->maps = k.take<int32_t>(static_cast<int64_t>(S_max - 1) * map_ints(N, S_max));
  return k.off + 256;
}

CollDims max_dims(int N, int S_max, int mode, const mtg_coll_params& p) {
  return coll_dims(S_max, 3, (S_max - 1) * (N / 2), mode, p);
}

unsigned grid1(int64_t n) { return static_cast<unsigned>(n); }

// One objective evaluation of the batch at the compact points w.xt up to the
// combine.
template <int N>
hipError_t evaluate_n(const RaggedCollArgs& g, const RaggedColl& a, const mtg_coll_params& p,
                      const Workspace& ws, hipStream_t st) {
  const CollWs& w = ws.w;
  hipError_t e = launch(ragged_coll_prep_kernel<N>, g.B, kWave,
                        ragged_coll_prep_lds_bytes(N, a.S_max), st, a, g.fixed_vals, g.times,
                        p.increment_time, w);
  if (e != hipSuccess) return e;
  // With the near field one thread walks alone: one wave per walk.
  hipLaunchKernelGGL(ragged_coll_walk_kernel<N>, dim3(grid1(g.B * a.mx.P)),
                     dim3(g.field ? kWave : kCollBlock), collision_lds_bytes(N, a.S_max), st, a,
                     g.occ, g.nx, g.ny, g.nz, g.field, p.coll, p.increment_time, w);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if (a.mx.Q > 0) {
    const int64_t BQ = g.B * a.mx.Q;
    hipLaunchKernelGGL(ragged_coll_soft_points_kernel<N>, dim3(grid1(BQ)), dim3(kWave), 0, st, a,
                       g.fixed_vals, p.coll.map_resolution, w, ws.softn);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    const RaggedEvalOut out{w.softm, nullptr, nullptr, w.softJ, nullptr, nullptr};
    e = launch_ragged_extrema(N, 3, a.S_max, BQ, ws.softn, w.softc, w.softT, coll_soft_spec(p),
                              out, st);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

hipError_t evaluate(const RaggedCollArgs& g, const RaggedColl& a, const mtg_coll_params& p,
                    const Workspace& ws, hipStream_t st) {
  return with_order(g.N, [&](auto n) { return evaluate_n<n()>(g, a, p, ws, st); });
}

// Carves the workspace and enqueues the maps kernel.
int begin(const RaggedCollArgs& g, const mtg_coll_params& p, bool opt, void* workspace,
          size_t workspace_bytes, RaggedColl* a, Workspace* ws, hipStream_t st) {
  if (ragged_coll_workspace_bytes(g.N, g.S_max, g.B, g.mode, p, opt) > workspace_bytes)
    return MTG_ERR_INVALID_ARG;
  const CollDims mx = max_dims(g.N, g.S_max, g.mode, p);
  carve(workspace, mx, g.N, g.S_max, g.B, p.n_soft, opt, ws);
  *a = RaggedColl{g.N, g.r, g.S_max, mx, g.seg_counts, g.tab, ws->maps};
  hipLaunchKernelGGL(ragged_coll_maps_kernel, dim3(g.S_max - 1), dim3(kWave), 0, st, *a);
  return hipGetLastError() == hipSuccess ? MTG_OK : MTG_ERR_HIP;
}

}  // namespace

size_t ragged_coll_prep_lds_bytes(int N, int S_max) {
  size_t m = 0;
  for (int S = 2; S <= S_max; ++S) {
    const size_t b = free_lds(N, S, 3, (S - 1) * (N / 2), false).bytes;
    if (b > m) m = b;
  }
  return m;
}

size_t ragged_coll_workspace_bytes(int N, int S_max, int64_t B, int mode,
                                   const mtg_coll_params& p, bool optimiser) {
  Workspace ws;
  return carve(nullptr, max_dims(N, S_max, mode, p), N, S_max, B, p.n_soft, optimiser, &ws);
}

int64_t ragged_coll_problems(int N, int S_max, int64_t B, int mode, const mtg_coll_params& p) {
  const CollDims mx = max_dims(N, S_max, mode, p);
  return B * (mx.P > mx.Q ? mx.P : mx.Q);
}

int ragged_coll_cost(const RaggedCollArgs& g, const double* x, const mtg_coll_params& p,
                     const double* raise_ref, double* cost, double* grad, double* terms,
                     int32_t* collision, int32_t* status, void* workspace,
                     size_t workspace_bytes, hipStream_t st) {
  RaggedColl a;
  Workspace ws;
  const int rc = begin(g, p, false, workspace, workspace_bytes, &a, &ws, st);
  if (rc) return rc;
  hipLaunchKernelGGL(ragged_coll_gather_kernel, dim3(grid1(g.B)), dim3(kWave), 0, st, a, x, ws.w);
  if (hipGetLastError() != hipSuccess) return MTG_ERR_HIP;
  if (evaluate(g, a, p, ws, st) != hipSuccess) return MTG_ERR_HIP;
  const CombineOut o{raise_ref, cost, grad, terms, collision, status, nullptr};
  hipLaunchKernelGGL(ragged_coll_combine_kernel<false>, dim3(grid1(g.B)), dim3(kWave), 0, st, a,
                     p, 0, Bounds{nullptr, nullptr}, ws.w, o);
  return hipGetLastError() == hipSuccess ? MTG_OK : MTG_ERR_HIP;
}

// max_evals rounds, all stream-ordered, as coll_optimize: a finished row (or
// one that never started) is skipped by every later kernel.
int ragged_coll_optimize(const RaggedCollArgs& g, double* x_io, const double* lower,
                         const double* upper, const double* initial_step,
                         const mtg_coll_params& p, int max_evals, double* cost, int32_t* evals,
                         int32_t* result, int32_t* status, double* terms, double* x_history,
                         void* workspace, size_t workspace_bytes, hipStream_t st) {
  RaggedColl a;
  Workspace ws;
  const int rc = begin(g, p, true, workspace, workspace_bytes, &a, &ws, st);
  if (rc) return rc;
  const Bounds bd{lower, upper};
  hipLaunchKernelGGL(ragged_coll_opt_init_kernel, dim3(grid1(g.B)), dim3(kWave), 0, st, a, x_io,
                     initial_step, bd, ws.w);
  if (hipGetLastError() != hipSuccess) return MTG_ERR_HIP;
  CombineOut hist{};
  hist.x_history = x_history;
  for (int round = 0; round < max_evals; ++round) {
    if (evaluate(g, a, p, ws, st) != hipSuccess) return MTG_ERR_HIP;
    hipLaunchKernelGGL(ragged_coll_combine_kernel<true>, dim3(grid1(g.B)), dim3(kWave), 0, st, a,
                       p, max_evals, bd, ws.w, hist);
    if (hipGetLastError() != hipSuccess) return MTG_ERR_HIP;
  }
  hipLaunchKernelGGL(ragged_coll_opt_final_kernel, dim3(grid1(g.B)), dim3(kWave), 0, st, a, ws.w,
                     x_io, cost, evals, result, status, terms);
  return hipGetLastError() == hipSuccess ? MTG_OK : MTG_ERR_HIP;
}

}  // namespace mtg
