// mtg_coll_opt_device.h — what the collision-driven objectives of uniform and
// of ragged batches (mtg_coll_opt.hip, mtg_ragged_coll_opt.hip) share: the
// per-trajectory dimensions, the workspace and its carver, and the bodies of
// every kernel of the evaluation chain and of the projected L-BFGS.
//
// A body sees its trajectory through a row view:
//   dims()  the trajectory's own dimensions (its S, np, nv, P, Q);
//   rows()  the dimensions the workspace rows were carved for: row b of a
//           workspace array of n entries per trajectory starts at b rows().n;
//   ext(i)  where variable i of the compact state (first the S times in
//           mode 1, then D x np free derivatives) sits in a row of the
//           caller's arrays (x, grad, bounds, steps, history), whose rows
//           are rows().nv apart.
// UniformRow has dims() == rows() and ext(i) == i.  RaggedRow has the row's
// count in dims(), S_max in rows() and the padded layout of the ragged tube
// solve in ext().  The state in the workspace is compact at the front of its
// row in both, so every sum over the variables partitions over the lanes in
// the same way whatever the padding.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

#include "mtg_collision_device.h"
#include "mtg_free_device.h"
#include "mtg_internal.h"

namespace mtg {

constexpr double kLowerT = 0.1;  // the clamp of getCostAndGradientTime (:2529-2530)
constexpr int kMaxLbfgsMemory = 16;
constexpr double kArmijo = 1e-4;

struct CollDims {
  int mode, S, D, np;
  int nfr;   // D * np free variables
  int nv;    // variables per trajectory (mode 1: S + nfr)
  int off;   // offset of d_p in x (mode 1: S)
  int P;     // collision walks per trajectory (1, or 1 + S / 1 + 2S for the time gradient)
  int Q;     // soft-cost problems per trajectory (0 without soft constraints)
  int central_t, central_sc;
  int m;     // L-BFGS memory
  int soft;  // soft constraints present
};

// The sizes of a trajectory of S segments and np free derivatives per
// dimension; mode, D, the difference schemes, soft and m stay.
__host__ __device__ inline void coll_dims_sizes(CollDims& c, int S, int np) {
  c.S = S;
  c.np = np;
  c.nfr = c.D * np;
  c.off = c.mode ? S : 0;
  c.nv = c.off + c.nfr;
  c.P = c.mode ? (c.central_t ? 1 + 2 * S : 1 + S) : 1;
  c.Q = c.soft ? (c.central_sc ? 1 + 2 * c.nfr : 1 + c.nfr) : 0;
}

inline CollDims coll_dims(int S, int D, int np, int mode, const mtg_coll_params& p) {
  CollDims c{};
  c.mode = mode;
  c.D = D;
  c.central_t = !p.simple_numgrad_time;
  c.central_sc = mode == 0 || !p.simple_numgrad_constraints;
  c.m = p.lbfgs_memory;
  c.soft = p.n_soft > 0;
  coll_dims_sizes(c, S, np);
  return c;
}

struct UniformRow {
  const CollDims& cd;
  __device__ const CollDims& dims() const { return cd; }
  __device__ const CollDims& rows() const { return cd; }
  __device__ int ext(int i) const { return i; }
};

// Rows padded to S_max: the caller's row is [S_max times (mode 1)] then D rows
// of np_max, of which the first np of each are the trajectory's.
struct RaggedRow {
  CollDims cd, mx;
  __device__ const CollDims& dims() const { return cd; }
  __device__ const CollDims& rows() const { return mx; }
  __device__ int ext(int i) const {
    if (i < cd.off) return i;
    const int k = (i - cd.off) / cd.np;
    return mx.off + k * mx.np + (i - cd.off - k * cd.np);
  }
  // Whether entry j of a caller's row belongs to no variable of this row.
  __device__ bool padding(int j) const {
    if (j < mx.off) return j >= cd.off;
    return (j - mx.off) % mx.np >= cd.np;
  }
};

struct CollWs {
  double* xt;      // B x nv   evaluation point (optimiser)
  double* T;       // B x S    its segment times
  double* coeffs;  // B x S x D x N
  double* Jd;      // B        J_d (unweighted)
  double* Jt;      // B        sum T
  double* gd;      // B x nfr  dJ_d / dd_p
  double* dJd;     // B x S    dJ_d / dT_n (d held)
  double* Jc;      // B x P    J_c of every walk
  int32_t* coll;   // B x P
  double* gc;      // B x nfr  dJ_c / dd_p of the walk at T
  double* softc;   // B x Q x S x D x N
  double* softT;   // B x Q x S
  double* softJ;   // B x Q
  double* softm;   // B x Q x n_soft (per-constraint launches)
  int32_t* st;     // B        MTG_TRAJ_* of the evaluation point
  int32_t* done;   // B        (optimiser) trajectory finished
  // L-BFGS state (optimiser).
  double *x, *g, *G, *dir, *Sh, *Yh, *rho, *f, *alpha, *Jref0, *Jlast, *terms, *tterms, *step0;
  int32_t *hist, *evals, *result, *phase;
};

struct CollCarver {
  char* base;
  size_t off = 0;
  template <typename T>
  T* take(int64_t n) {
    off = (off + 255) & ~size_t(255);
    T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
    off += sizeof(T) * static_cast<size_t>(n > 0 ? n : 1);
    return p;
  }
};

// Carves B rows of the dimensions c (a row view's rows()).
inline void coll_carve(CollCarver& k, const CollDims& c, int N, int64_t B, int n_soft, bool opt,
                       CollWs* w) {
  const int S = c.S, D = c.D;
  *w = CollWs{};
  w->xt = k.take<double>(B * c.nv);
  w->T = k.take<double>(B * S);
  w->coeffs = k.take<double>(B * S * D * N);
  w->Jd = k.take<double>(B);
  w->Jt = k.take<double>(B);
  w->gd = k.take<double>(B * c.nfr);
  w->dJd = k.take<double>(B * S);
  w->Jc = k.take<double>(B * c.P);
  w->coll = k.take<int32_t>(B * c.P);
  w->gc = k.take<double>(B * c.nfr);
  if (c.Q > 0) {
    w->softc = k.take<double>(B * c.Q * S * D * N);
    w->softT = k.take<double>(B * c.Q * S);
    w->softJ = k.take<double>(B * c.Q);
    w->softm = k.take<double>(B * c.Q * n_soft);
  }
  w->st = k.take<int32_t>(B);
  if (opt) {
    w->done = k.take<int32_t>(B);
    w->x = k.take<double>(B * c.nv);
    w->g = k.take<double>(B * c.nv);
    w->G = k.take<double>(B * c.nv);
    w->dir = k.take<double>(B * c.nv);
    w->Sh = k.take<double>(B * c.m * c.nv);
    w->Yh = k.take<double>(B * c.m * c.nv);
    w->rho = k.take<double>(B * c.m);
    w->f = k.take<double>(B);
    w->alpha = k.take<double>(B);
    w->Jref0 = k.take<double>(B);
    w->Jlast = k.take<double>(B);
    w->terms = k.take<double>(B * 4);
    w->tterms = k.take<double>(B * 4);
    w->step0 = k.take<double>(B);
    w->hist = k.take<int32_t>(B * 2);
    w->evals = k.take<int32_t>(B);
    w->result = k.take<int32_t>(B);
    w->phase = k.take<int32_t>(B);
  }
}

__device__ inline bool skipped(const CollWs& w, int64_t b) { return w.done && w.done[b]; }

// Segment time n of the time-gradient walk q (q = 0: T itself): central
// differences lower / raise T_n by h (q = 1 + 2n / 2 + 2n), forward
// differences raise it (q = 1 + n); both clamp at 0.1 (:2529-2530, 2622-2623).
__device__ inline double walk_time(const CollDims& cd, const double* T, int q, int i, double h) {
  const double t = T[i];
  if (q == 0) return t;
  const int n = cd.central_t ? (q - 1) >> 1 : q - 1;
  if (i != n) return t;
  const bool up = !cd.central_t || ((q - 1) & 1);
  return t <= kLowerT ? kLowerT : (up ? t + h : t - h);
}

// ---------------------------------------------------------------------------
// prep: coefficients, J_d and its gradient, J_t and dJ_d/dT (d held).  The
// body of a one-wave workgroup; smem is free_lds(N, S, D, np, false).
template <int N, typename Row>
__device__ __attribute__((always_inline)) inline void coll_prep_body(
    const PlanDev& pl, const Row& row, int64_t b, const double* __restrict__ fixed_vals,
    const double* __restrict__ times_in, const double* __restrict__ xsrc, double inc,
    const CollWs& w, double* smem) {
  const CollDims& cd = row.dims();
  const CollDims& rs = row.rows();
  const int S = pl.S, D = pl.D, nf = pl.nf, np = pl.np;
  const Layout lay = make_layout(N, S, D);
  const FreeLds fl = free_lds(N, S, D, np, false);
  Traj<N> t{S, D, pl.r, &lay, smem, reinterpret_cast<int*>(smem + lay.ndouble),
            static_cast<int>(threadIdx.x), pl.fmask, pl.use_mask != 0};
  const double* xb = xsrc + b * rs.nv;
  const double* tb = cd.mode ? xb : times_in + b * rs.S;
  const bool bad = free_setup(t, pl, fixed_vals + b * D * nf, xb + cd.off, tb);
  for (int i = t.lane; i < S; i += kWave) w.T[b * rs.S + i] = t.T()[i];
  double Jd = NAN, Jt = NAN;
  if (!bad) {
    // J_d = sum_dim d^T R d = c^T Q c = 2 computeCost() (:1537-1606).
    Jd = 2.0 * t.template coeffs_and_cost<true>(pl.tab, w.coeffs + b * rs.S * D * N);
    double* gv = lds_at<double>(smem, fl.gv);
    free_rd(t, gv);
    for (int i = t.lane; i < D * np; i += kWave)
      w.gd[b * rs.nfr + i] = 2.0 * gv[pl.free_map[i % np] * D + i / np];
    if (cd.mode == 1) {
      double tot = 0.0;
      for (int i = 0; i < S; ++i) tot += t.T()[i];  // computeTotalTrajectoryTime (:2768-2774)
      Jt = tot;
      // getCostAndGradientTime: J_d at T_n +- h with d held (updateSegmentTimes
      // then getCostAndGradientDerivative, :2532-2537); only segment n's
      // energy changes.
      for (int n = 0; n < S; ++n) {
        const double Tn = t.T()[n];
        const double hi = Tn <= kLowerT ? kLowerT : Tn + inc;
        const double e_hi = t.seg_energy_at(n, hi);
        double dj;
        if (cd.central_t) {
          const double lo = Tn <= kLowerT ? kLowerT : Tn - inc;
          dj = (e_hi - t.seg_energy_at(n, lo)) / (2.0 * inc);
        } else {
          dj = (e_hi - t.seg_energy_at(n, Tn)) / inc;
        }
        if (t.lane == 0) w.dJd[b * rs.S + n] = dj;
      }
    }
  }
  if (t.lane == 0) {
    w.Jd[b] = Jd;
    w.Jt[b] = Jt;
    w.st[b] = bad ? MTG_TRAJ_BAD_TIME : MTG_TRAJ_OK;
  }
}

// walk: J_c of walk q of trajectory b; q = 0 also the gradient.  sm is
// collision_lds_bytes(N, S).
template <int N, typename Row>
__device__ __attribute__((always_inline)) inline void coll_walk_body(
    const PlanDev& pl, const Row& row, int64_t b, int q, const float* __restrict__ occ, int nx,
    int ny, int nz, const uint16_t* __restrict__ field, const mtg_collision_params& cp,
    double inc, const CollWs& w, double* sm) {
  constexpr int D = 3;
  const CollDims& cd = row.dims();
  const CollDims& rs = row.rows();
  const int S = pl.S;
  const int64_t prob = b * rs.P + q;
  const int tid = threadIdx.x;
  if (w.st[b] != MTG_TRAJ_OK) {
    if (tid == 0) {
      w.Jc[prob] = NAN;
      w.coll[prob] = 0;
    }
    if (q == 0)
      for (int i = tid; i < cd.nfr; i += static_cast<int>(blockDim.x)) w.gc[b * rs.nfr + i] = NAN;
    return;
  }
  double* c_s = sm;               // S x D x N
  double* T_s = c_s + S * D * N;  // S (walk times)
  double* g_s = T_s + S;          // S x D x N
  double* scratch = g_s + S * D * N;
  const bool grad = q == 0;
  for (int i = tid; i < S * D * N; i += static_cast<int>(blockDim.x)) {
    c_s[i] = w.coeffs[b * rs.S * D * N + i];
    if (grad) g_s[i] = 0.0;
  }
  for (int i = tid; i < S; i += static_cast<int>(blockDim.x))
    T_s[i] = walk_time(cd, w.T + b * rs.S, q, i, inc);
  __syncthreads();
  double J;
  bool hit;
  collision_walk<N>(S, c_s, T_s, occ, nx, ny, nz, cp, grad, g_s, scratch, &J, &hit, field);
  if (tid == 0) {
    w.Jc[prob] = J;
    w.coll[prob] = hit ? 1 : 0;
  }
  if (grad)  // T_s is T itself for q = 0
    for (int i = tid; i < cd.nfr; i += static_cast<int>(blockDim.x))
      w.gc[b * rs.nfr + i] =
          coll_grad_free<N>(S, D, pl.np, pl.tab + N * N, pl.free_map, T_s, g_s, i);
}

// soft points: coefficients of problem q of trajectory b.  q = 0 is x itself;
// q > 0 perturbs free variable i = (q-1)/2 by -h / +h (central) or i = q-1 by
// +h (forward) as setFreeConstraints(free_constraints -+ increment) does
// (:2396-2416, 2469-2479): only the segments meeting at the perturbed vertex
// change, and they are recomputed as c = A^-1(T) [d(s); d(s+1)] from the
// perturbed endpoint derivatives.  The body of a one-wave workgroup.
template <int N, typename Row>
__device__ __attribute__((always_inline)) inline void coll_soft_points_body(
    const PlanDev& pl, const Row& row, int64_t b, int q, const double* __restrict__ fixed_vals,
    const double* __restrict__ xsrc, double h, const CollWs& w) {
  constexpr int M = N / 2;
  const CollDims& cd = row.dims();
  const CollDims& rs = row.rows();
  const int S = pl.S, D = pl.D, per = S * D * N;
  const int64_t prob = b * rs.Q + q;
  const int lane = threadIdx.x;
  double* dst = w.softc + prob * (rs.S * D * N);
  if (w.st[b] != MTG_TRAJ_OK) {  // keep the search on finite data; J is NaN anyway
    for (int i = lane; i < per; i += kWave) dst[i] = 0.0;
    for (int i = lane; i < S; i += kWave) w.softT[prob * rs.S + i] = 1.0;
    return;
  }
  for (int i = lane; i < per; i += kWave) dst[i] = w.coeffs[b * (rs.S * D * N) + i];
  for (int i = lane; i < S; i += kWave) w.softT[prob * rs.S + i] = w.T[b * rs.S + i];
  if (q == 0) return;
  __syncthreads();
  const int iv = cd.central_sc ? (q - 1) >> 1 : q - 1;
  const double sgn = (!cd.central_sc || ((q - 1) & 1)) ? 1.0 : -1.0;
  const int k = iv / pl.np, pidx = iv % pl.np;
  const int slot = pl.free_map[pidx], v = slot / M, j = slot % M;
  const double* xb = xsrc + b * rs.nv + cd.off;
  const double xp = xb[iv];
  const double xpert = sgn > 0.0 ? xp + h : xp - h;
  // Lanes 0..N-1: segment v (v = its start vertex); lanes 32..32+N-1:
  // segment v-1 (v = its end vertex).
  const int half = lane >> 5, a = lane & 31;
  const int s = v - half;
  if (a >= N || s < 0 || s >= S) return;
  double e[N];
#pragma unroll
  for (int jj = 0; jj < N; ++jj) {
    const int vv = s + jj / M, kk = jj % M;
    const int sl = pl.slots[vv * M + kk];
    double val = sl >= 0 ? fixed_vals[(b * D + k) * pl.nf + sl] : xb[k * pl.np + (-sl - 1)];
    if (vv == v && kk == j) val = xpert;
    e[jj] = val;
  }
  // c_a = sum_jj A(1)^-1[a][jj] T^(jj mod M - a) e_jj (Traj::coeffs_and_cost),
  // the powers by the multiplication chains of Traj::compute_powers.
  const double T = w.T[b * rs.S + s];
  const double inv = rcp64(T);
  const double* tA = pl.tab + N * N;  // A(1)^-1
  double c = 0.0;
#pragma unroll
  for (int jj = 0; jj < N; ++jj) {
    const int ex = (jj % M) - a;
    const double base = ex >= 0 ? T : inv;
    double pw = 1.0;
    for (int z = 0; z < (ex >= 0 ? ex : -ex); ++z) pw *= base;
    c += tA[a * N + jj] * pw * e[jj];
  }
  dst[(s * D + k) * N + a] = c;
}

// NLopt's relstop (vold -> vnew within reltol or abstol; util/stop.c).
__device__ inline bool relstop(double vold, double vnew, double reltol, double abstol) {
  if (vold == vnew) return true;
  const double d = fabs(vnew - vold);
  return d < abstol || d < reltol * (fabs(vnew) + fabs(vold)) * 0.5;
}

__device__ inline double wave_sum64(double x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, kWave);
  return x;
}
__device__ inline double wave_max64(double x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x = fmax(x, __shfl_xor(x, off, kWave));
  return x;
}

// Outputs and bounds are the caller's arrays: rows of rows().nv, entry ext(i).
struct CombineOut {
  const double* raise_ref;
  double* cost;
  double* grad;
  double* terms;
  int32_t* collision;
  int32_t* status;
  // Optimiser only (nullable): B x max_evals x nv, row k = the point of the
  // (k+1)-th counted evaluation (all_trajectories_, nonlinear_impl:1244,1482).
  double* x_history;
};

struct Bounds {
  const double* lo;
  const double* hi;
};

// Projected L-BFGS direction at (x, g) of trajectory b into w.dir: two-loop
// recursion over the stored pairs on the free variables (a variable at a
// bound whose gradient pushes outward is held).  Returns max |q| (0: the
// projected gradient vanishes).
template <typename Row>
__device__ double lbfgs_direction(const Row& row, const CollWs& w, const Bounds& bd, int64_t b,
                                  int lane, bool reset) {
  const CollDims& cd = row.dims();
  const int nv = cd.nv, m = cd.m, rnv = row.rows().nv;
  double* x = w.x + b * rnv;
  double* g = w.g + b * rnv;
  double* d = w.dir + b * rnv;
  int32_t* hist = w.hist + b * 2;
  if (reset) {
    if (lane == 0) hist[0] = hist[1] = 0;
    __syncthreads();
  }
  const int cnt = hist[0], head = hist[1];
  auto held = [&](int i) {
    const double lo = bd.lo ? bd.lo[b * rnv + row.ext(i)] : -HUGE_VAL;
    const double hi = bd.hi ? bd.hi[b * rnv + row.ext(i)] : HUGE_VAL;
    return (x[i] <= lo && g[i] > 0.0) || (x[i] >= hi && g[i] < 0.0);
  };
  double qmax = 0.0;
  for (int i = lane; i < nv; i += kWave) {
    const double qi = held(i) ? 0.0 : g[i];
    d[i] = qi;  // q, then r
    qmax = fmax(qmax, fabs(qi));
  }
  qmax = wave_max64(qmax);
  if (!(qmax > 0.0)) return qmax;
  double a[kMaxLbfgsMemory];
  const double* Sh = w.Sh + b * m * rnv;
  const double* Yh = w.Yh + b * m * rnv;
  const double* rho = w.rho + b * m;
  __syncthreads();
  for (int c = 0; c < cnt; ++c) {  // newest to oldest
    const int k = (head - 1 - c + m) % m;
    double sq = 0.0;
    for (int i = lane; i < nv; i += kWave) sq += Sh[k * rnv + i] * d[i];
    const double ak = rho[k] * wave_sum64(sq);
#pragma unroll
    for (int z = 0; z < kMaxLbfgsMemory; ++z)
      if (z == c) a[z] = ak;
    for (int i = lane; i < nv; i += kWave) d[i] -= ak * Yh[k * rnv + i];
  }
  double gamma;
  if (cnt > 0) {
    const int k = (head - 1 + m) % m;
    double sy = 0.0, yy = 0.0;
    for (int i = lane; i < nv; i += kWave) {
      sy += Sh[k * rnv + i] * Yh[k * rnv + i];
      yy += Yh[k * rnv + i] * Yh[k * rnv + i];
    }
    gamma = wave_sum64(sy) / wave_sum64(yy);
  } else {
    const double step = w.step0[b];
    gamma = (step > 0.0 ? step : 1.0) / qmax;
  }
  for (int i = lane; i < nv; i += kWave) d[i] *= gamma;
  for (int c = cnt - 1; c >= 0; --c) {  // oldest to newest
    const int k = (head - 1 - c + m) % m;
    double yr = 0.0;
    for (int i = lane; i < nv; i += kWave) yr += Yh[k * rnv + i] * d[i];
    const double beta = rho[k] * wave_sum64(yr);
    double ak = 0.0;
#pragma unroll
    for (int z = 0; z < kMaxLbfgsMemory; ++z)
      if (z == c) ak = a[z];
    for (int i = lane; i < nv; i += kWave) d[i] += (ak - beta) * Sh[k * rnv + i];
  }
  double gp = 0.0;
  for (int i = lane; i < nv; i += kWave) {
    d[i] = held(i) ? 0.0 : -d[i];
    gp += g[i] * d[i];
  }
  gp = wave_sum64(gp);
  if (!(gp < 0.0)) {  // not a descent direction: restart from steepest descent
    if (lane == 0) hist[0] = hist[1] = 0;
    const double step = w.step0[b];
    const double g0 = (step > 0.0 ? step : 1.0) / qmax;
    for (int i = lane; i < nv; i += kWave) d[i] = held(i) ? 0.0 : -g0 * g[i];
  }
  __syncthreads();
  return qmax;
}

// combine: J and its gradient at the evaluation point; with kOpt also one
// step of the L-BFGS state machine.  The body of a one-wave workgroup.
template <bool kOpt, typename Row>
__device__ __attribute__((always_inline)) inline void coll_combine_body(
    const Row& row, int64_t b, const mtg_coll_params& p, int max_evals, const Bounds& bd,
    const CollWs& w, const CombineOut& o) {
  const CollDims& cd = row.dims();
  const CollDims& rs = row.rows();
  const int lane = threadIdx.x;
  const int Q = cd.Q, nv = cd.nv, off = cd.off;
  const int rS = rs.S, rP = rs.P, rQ = rs.Q, rnv = rs.nv, rnfr = rs.nfr;
  const int st = w.st[b];
  const bool bad = st != MTG_TRAJ_OK;
  const bool coll = !bad && w.coll[b * rP] != 0;
  const double Jc0 = bad ? NAN : w.Jc[b * rP];
  double Jd = 0.0, Jt = 0.0, Jsc = 0.0;
  if (bad) {
    Jd = Jt = Jsc = NAN;
  } else if (!coll) {  // :1171-1178, 1355-1386
    Jd = w.Jd[b];
    if (cd.mode == 1) Jt = w.Jt[b];
    if (Q > 0) Jsc = w.softJ[b * rQ];
  }
  const double ct = p.w_d * Jd, ctm = p.w_t * Jt, csc = p.w_sc * Jsc;
  double cc = p.w_c * Jc0;
  const double total = ct + cc + ctm + csc;
  if (p.is_collision_safe && coll) {  // :1207-1226, 1432-1452
    double ref;
    if constexpr (kOpt)
      ref = p.is_coll_raise_first_iter ? w.Jref0[b] : w.Jlast[b];
    else
      ref = o.raise_ref ? o.raise_ref[b] : 0.0;
    cc = ref - (total - cc) + p.add_coll_raise;
  }
  const double J = ct + cc + ctm + csc;
  const double h = p.coll.map_resolution, inc = p.increment_time;
  // The optimiser's gradient is state (compact); the cost entry's is the caller's.
  double* G = kOpt ? w.G + b * rnv : (o.grad ? o.grad + b * rnv : nullptr);
  if (G) {
    for (int i = lane; i < nv; i += kWave) {
      double gi;
      if (i < off) {  // getCostAndGradientTime (:2565-2571, 2638-2644)
        const int n = i;
        if (bad) {
          gi = NAN;
        } else if (coll) {
          gi = 0.0;
        } else {
          const double dJc = cd.central_t
                                 ? (w.Jc[b * rP + 2 + 2 * n] - w.Jc[b * rP + 1 + 2 * n]) / (2.0 * inc)
                                 : (w.Jc[b * rP + 1 + n] - Jc0) / inc;
          gi = p.w_d * w.dJd[b * rS + n] + p.w_c * dJc + p.w_sc * 0.0 + p.w_t * 1.0;
        }
      } else {  // :1263-1268, 1525-1531
        const int k = i - off;
        double gdd = 0.0, gsc = 0.0;
        if (bad) {
          gdd = NAN;
        } else if (!coll) {
          gdd = w.gd[b * rnfr + k];
          if (Q > 0)
            gsc = cd.central_sc ? (w.softJ[b * rQ + 2 + 2 * k] - w.softJ[b * rQ + 1 + 2 * k]) /
                                      (2.0 * h)
                                : (w.softJ[b * rQ + 1 + k] - w.softJ[b * rQ]) / h;
        }
        gi = p.w_d * gdd + p.w_c * w.gc[b * rnfr + k] + p.w_sc * gsc;
      }
      G[kOpt ? i : row.ext(i)] = gi;
    }
  }
  if constexpr (!kOpt) {
    if (lane == 0) {
      if (o.cost) o.cost[b] = J;
      if (o.terms) {
        o.terms[b * 4 + 0] = ct;
        o.terms[b * 4 + 1] = cc;
        o.terms[b * 4 + 2] = ctm;
        o.terms[b * 4 + 3] = csc;
      }
      if (o.collision) o.collision[b] = coll ? 1 : 0;
      if (o.status) o.status[b] = st;
    }
    return;
  } else {
    __syncthreads();
    // ---- L-BFGS state machine (one counted evaluation per round).
    const int m = cd.m;
    double* x = w.x + b * rnv;
    double* g = w.g + b * rnv;
    double* xt = w.xt + b * rnv;
    double* d = w.dir + b * rnv;
    const int phase = w.phase[b];
    const int evals = w.evals[b] + 1;
    double f = w.f[b], alpha = w.alpha[b];
    int result = 0;  // 0: continue
    bool place = false;
    if (o.x_history) {  // the evaluated point, before the state machine moves xt
      double* hrow = o.x_history + (b * max_evals + (evals - 1)) * rnv;
      for (int i = lane; i < nv; i += kWave) hrow[row.ext(i)] = xt[i];
    }
    if (lane == 0) {
      if (phase == 0) w.Jref0[b] = J;  // total_cost_iter0_ (:1253-1257)
      w.Jlast[b] = J;                  // optimization_info_ of this evaluation
      w.evals[b] = evals;
      w.tterms[b * 4 + 0] = ct;
      w.tterms[b * 4 + 1] = cc;
      w.tterms[b * 4 + 2] = ctm;
      w.tterms[b * 4 + 3] = csc;
    }
    auto accept_point = [&]() {
      for (int i = lane; i < nv; i += kWave) {
        x[i] = xt[i];
        g[i] = G[i];
      }
      if (lane == 0) {
        w.f[b] = J;
        for (int z = 0; z < 4; ++z) w.terms[b * 4 + z] = w.tterms[b * 4 + z];
      }
      f = J;
      __syncthreads();
    };
    if (phase == 0) {
      if (!std::isfinite(J)) {
        result = -1;  // FAILURE
        if (lane == 0) w.f[b] = J;
      } else {
        accept_point();
        if (!(lbfgs_direction(row, w, bd, b, lane, true) > 0.0)) result = 1;  // SUCCESS
        alpha = 1.0;
        place = true;
      }
      if (lane == 0) w.phase[b] = 1;
    } else {
      double dd = 0.0;
      for (int i = lane; i < nv; i += kWave) dd += g[i] * (xt[i] - x[i]);
      dd = wave_sum64(dd);
      if (std::isfinite(J) && J < f && J <= f + kArmijo * dd) {
        // Accept: store the pair, test NLopt's ftol / xtol, new direction.
        double sy = 0.0, ss = 0.0, yy = 0.0;
        bool xstop = true;
        for (int i = lane; i < nv; i += kWave) {
          const double s = xt[i] - x[i], y = G[i] - g[i];
          sy += s * y;
          ss += s * s;
          yy += y * y;
          xstop = xstop && relstop(x[i], xt[i], p.x_rel, p.x_abs);
        }
        sy = wave_sum64(sy);
        ss = wave_sum64(ss);
        yy = wave_sum64(yy);
        xstop = __all(xstop);
        const bool fstop = relstop(f, J, p.f_rel, p.f_abs);
        if (sy > 1e-12 * sqrt(ss * yy)) {
          int32_t* hist = w.hist + b * 2;
          const int head = hist[1], cnt = hist[0];
          for (int i = lane; i < nv; i += kWave) {
            w.Sh[(b * m + head) * rnv + i] = xt[i] - x[i];
            w.Yh[(b * m + head) * rnv + i] = G[i] - g[i];
          }
          __syncthreads();
          if (lane == 0) {
            w.rho[b * m + head] = 1.0 / sy;
            hist[1] = (head + 1) % m;
            hist[0] = cnt < m ? cnt + 1 : m;
          }
          __syncthreads();
        }
        accept_point();
        if (fstop) {
          result = 3;  // FTOL_REACHED
        } else if (xstop) {
          result = 4;  // XTOL_REACHED
        } else {
          if (!(lbfgs_direction(row, w, bd, b, lane, false) > 0.0)) result = 1;
          alpha = 1.0;
          place = true;
        }
      } else {
        // Backtrack: minimiser of the quadratic through f, the slope dd and
        // J, kept in [0.1, 0.5] alpha.
        double an = 0.5 * alpha;
        const double den = 2.0 * (J - f - dd);
        if (std::isfinite(J) && den > 0.0)
          an = fmin(fmax(-dd * alpha / den, 0.1 * alpha), 0.5 * alpha);
        alpha = an;
        place = true;
        if (alpha < 1e-10) {
          if (w.hist[b * 2] > 0) {  // drop the curvature pairs, steepest descent
            if (!(lbfgs_direction(row, w, bd, b, lane, true) > 0.0)) result = 1;
            alpha = 1.0;
          } else {
            result = 4;
            place = false;
          }
        }
      }
    }
    if (result == 0 && evals >= max_evals) result = 5;  // MAXEVAL_REACHED
    if (result == 0 && place) {
      bool moved = false;
      for (int i = lane; i < nv; i += kWave) {
        double v = x[i] + alpha * d[i];
        if (bd.lo) v = fmax(v, bd.lo[b * rnv + row.ext(i)]);
        if (bd.hi) v = fmin(v, bd.hi[b * rnv + row.ext(i)]);
        xt[i] = v;
        moved = moved || v != x[i];
      }
      if (!__any(moved)) result = 4;
    }
    if (lane == 0) {
      w.alpha[b] = alpha;
      if (result != 0) {
        w.result[b] = result;
        w.done[b] = 1;
      }
    }
  }
}

// Optimiser start: x0 clamped into the bounds, state reset.  The body of a
// one-wave workgroup.
template <typename Row>
__device__ __attribute__((always_inline)) inline void coll_opt_init_body(
    const Row& row, int64_t b, const double* __restrict__ x0, const double* __restrict__ step,
    const Bounds& bd, const CollWs& w) {
  const int nv = row.dims().nv, rnv = row.rows().nv;
  const int lane = threadIdx.x;
  double smax = 0.0;
  for (int i = lane; i < nv; i += kWave) {
    const int e = row.ext(i);
    double v = x0[b * rnv + e];
    if (bd.lo) v = fmax(v, bd.lo[b * rnv + e]);
    if (bd.hi) v = fmin(v, bd.hi[b * rnv + e]);
    w.xt[b * rnv + i] = v;
    w.x[b * rnv + i] = v;
    const double s = step ? step[b * rnv + e] : 0.1 * fabs(x0[b * rnv + e]);  // initial_stepsize_rel
    smax = fmax(smax, fabs(s));
  }
  smax = wave_max64(smax);
  if (lane == 0) {
    w.step0[b] = smax;
    w.done[b] = 0;
    w.phase[b] = 0;
    w.evals[b] = 0;
    w.result[b] = 5;
    w.hist[b * 2] = w.hist[b * 2 + 1] = 0;
    w.alpha[b] = 1.0;
    w.f[b] = NAN;
    w.Jref0[b] = 0.0;  // total_cost_iter0_{} (polynomial_optimization_nonlinear.h:672)
    w.Jlast[b] = 0.0;  // OptimizationInfo() zeros
    for (int z = 0; z < 4; ++z) w.terms[b * 4 + z] = NAN;
    w.st[b] = MTG_TRAJ_OK;
  }
}

template <typename Row>
__device__ __attribute__((always_inline)) inline void coll_opt_final_body(
    const Row& row, int64_t b, const CollWs& w, double* __restrict__ x_io,
    double* __restrict__ cost, int32_t* __restrict__ evals, int32_t* __restrict__ result,
    int32_t* __restrict__ status, double* __restrict__ terms) {
  const int nv = row.dims().nv, rnv = row.rows().nv;
  const int lane = threadIdx.x;
  const bool ok = w.phase[b] != 0 && std::isfinite(w.f[b]);
  for (int i = lane; i < nv; i += kWave)
    if (ok) x_io[b * rnv + row.ext(i)] = w.x[b * rnv + i];
  if (lane == 0) {
    if (cost) cost[b] = w.f[b];
    if (evals) evals[b] = w.evals[b];
    if (result) result[b] = w.result[b];
    if (status) status[b] = w.st[b] != MTG_TRAJ_OK && !ok ? w.st[b] : MTG_TRAJ_OK;
    if (terms)
      for (int z = 0; z < 4; ++z) terms[b * 4 + z] = w.terms[b * 4 + z];
  }
}

// The soft-constraint parameters as the extremum launchers take them.
inline SoftSpec coll_soft_spec(const mtg_coll_params& p) {
  SoftSpec spec{};
  spec.n = p.n_soft;
  for (int c = 0; c < p.n_soft; ++c) {
    spec.derivative[c] = p.soft_derivative[c];
    spec.limit[c] = p.soft_limit[c];
  }
  spec.weight = p.soft_weight;
  spec.maximum_cost = p.soft_maximum_cost;
  return spec;
}

}  // namespace mtg
