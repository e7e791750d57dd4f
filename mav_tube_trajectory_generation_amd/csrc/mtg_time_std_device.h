// mtg_time_std_device.h — the time-allocation objective of the standard
// vertex pattern and its evaluator for the shared drivers of
// mtg_time_device.h: J(T) = computeCost() + time_penalty (sum T)^2 [+ soft
// constraints] on the standard-pattern solver (stdp::Solver, runtime S) or
// its compile-time-S form (wave::Solver).  Included by the uniform kernels
// (mtg_time_std.hip) and the ragged ones (mtg_ragged.hip); every definition
// is local to the including translation unit.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

#include "mtg_extrema_device.h"
#include "mtg_sbplx_device.h"
#include "mtg_std_device.h"
#include "mtg_time_device.h"
#include "mtg_wave_device.h"

namespace mtg {

namespace {

template <int N, int R, int D>
using StdSv = stdp::Solver<N, R, D>;

// The inner solve and computeCost at the times T (LDS) on either solver:
// stdp::Solver (runtime S) or wave::Solver (compile-time S, the C2 design).
// Every lane calls; *bad is set (and NaN returned) when a time is invalid;
// with cbuf the coefficients go there (LDS, soft searches).
template <int N, int R, int D>
__device__ __attribute__((always_inline)) double solve_cost(
    stdp::Solver<N, R, D>& sv, const double* __restrict__ tab, const double* T, double* cbuf,
    bool reload_rows, bool* bad, bool* not_spd) {
  __syncthreads();
  const bool b = sv.powers_from(T);
  __syncthreads();
  if (b) {
    *bad = true;
    return NAN;
  }
  // soft: the H(1) rows are reloaded per evaluation (L2 hits), so they are
  // not live across the extremum searches.
  if (reload_rows) sv.load_first_rows(tab);
  sv.assemble(tab);
  __syncthreads();
  *not_spd = sv.solve() || *not_spd;
  return sv.coeff_cost(cbuf);
}

template <int N, int R, int D, int S>
__device__ __attribute__((always_inline)) double solve_cost(
    wave::Solver<N, R, D, S>& sv, const double* __restrict__ /*tab*/, const double* T,
    double* cbuf, bool /*reload_rows*/, bool* bad, bool* not_spd) {
  __syncthreads();
  const int l = sv.lane;
  const double t = T[l < S ? l : S - 1];
  if (__any(l < S && (!(t > 0.0) || !(t < 1e300)))) {
    *bad = true;
    return NAN;
  }
  *not_spd = sv.solve(T) || *not_spd;
  return sv.coeff_cost(T, cbuf);
}

// J(T) = computeCost() + time_penalty (sum T)^2 [+ soft constraints] at the
// times T (LDS, S values).  Every lane calls it; returns the wave-uniform J
// (NaN and *bad set when a time is invalid).  kSoft: the coefficients go to
// cbuf (LDS) and evaluateMaximumMagnitudeAsSoftConstraint
// (nonlinear_impl:2735-2766) runs one extremum search per constraint; with
// p.hard_constraints the searches give *viol = max(0, max_c (max_c - limit_c
// - tolerance)) (evaluateMaximumMagnitudeConstraint, :2687-2733) instead of
// a cost term.
template <int N, int D, bool kSoft, class SV>
__device__ __attribute__((always_inline)) double std_objective(SV& sv, const double* __restrict__ tab,
                                const double* T, int S, const mtg_time_params& p, double* cbuf,
                                bool* bad, bool* not_spd, double* viol) {
  *viol = 0.0;
  unsigned long long tt = 0;
  MTG_TACC(511, tt);
  double J = solve_cost(sv, tab, T, kSoft ? cbuf : nullptr, kSoft, bad, not_spd);
  if (*bad) return NAN;
  double tot = 0.0;
  for (int i = 0; i < S; ++i) tot += T[i];  // nonlinear_impl:2768-2774
  J += tot * tot * p.time_penalty;
  MTG_TACC(450, tt);  // diagnostic: solve + coefficients
  if constexpr (kSoft) {
    __syncthreads();
    // Every constraint's maximum in one pass (ext_soft_maxima_wave).
    int Ks[kMaxSoftConstraints];
    int kmin = 4;
#pragma unroll
    for (int cc = 0; cc < kMaxSoftConstraints; ++cc) {
      Ks[cc] = p.soft_derivative[cc];
      if (cc < p.n_soft && Ks[cc] < kmin) kmin = Ks[cc];
    }
    double* scratch = cbuf + S * D * N;
    double* maxima = scratch + kMaxSoftConstraints * (N + 1);
    ext_soft_maxima_wave_k<N>(kmin, cbuf, T, S, D, sv.lane, p.n_soft, Ks, scratch, maxima);
    double soft = 0.0;
    for (int c = 0; c < p.n_soft; ++c) {
      double lim = 1.0;
#pragma unroll
      for (int cc = 0; cc < kMaxSoftConstraints; ++cc)  // compile-time indices
        if (cc == c) lim = p.soft_limit[cc];
      const double m = maxima[c];
      if (p.hard_constraints) {
        *viol = fmax(*viol, m - lim - p.hard_tolerance);
      } else {
        soft += soft_penalty(m, lim, p.soft_weight, p.soft_maximum_cost);
      }
      MTG_TACC(451 + c, tt);  // diagnostic
    }
    J += soft;
  }
  return J;
}

// Loads d_f (and, for wave::Solver, H(1)) into the solver (all lanes).
template <int N, int R, int D>
__device__ void std_load_fixed(StdSv<N, R, D>& sv, const double* __restrict__ /*tab*/,
                               const double* __restrict__ fb) {
  const int nf = sv.nf;
  for (int i = sv.lane; i < D * nf; i += kWave) sv.put_fixed(i, fb[i]);
}
template <int N, int R, int D, int S>
__device__ void std_load_fixed(wave::Solver<N, R, D, S>& sv, const double* __restrict__ tab,
                               const double* __restrict__ fb) {
  sv.load_constants(tab, fb);
  wave::lds_order();
}

// The evaluator of the shared drivers (mtg_time_device.h): either solver
// with the drivers' hooks.  The evaluation point and the drivers' state share
// the solver's aux() region.
template <int N, int D, bool kSoft, class SV>
struct StdEval : SV {
  bool bad_ = false, not_spd_ = false;
  __device__ __attribute__((always_inline)) double* T() const { return this->aux(); }
  __device__ __attribute__((always_inline)) double* state(int S) const {
    return this->aux() + S;
  }
  __device__ __attribute__((always_inline)) double eval(int S, const double* __restrict__ tab,
                                                        double* cbuf, const mtg_time_params& p,
                                                        double* viol) {
    SV& sv = *this;
    return std_objective<N, D, kSoft>(sv, tab, T(), S, p, cbuf, &bad_, &not_spd_, viol);
  }
  __device__ __attribute__((always_inline)) bool bad() const { return bad_; }
  __device__ __attribute__((always_inline)) bool not_spd() const { return not_spd_; }
  // getCostAndGradientTime (nonlinear_impl:2495-2584): d held at the base
  // solution, only segment n's block of J_d = d^T R d changes.  One lane per
  // segment energy, 2S of them into E.
  __device__ __attribute__((always_inline)) void fixed_d_gradient(
      int S, const double* Tb, const mtg_time_params& p, double* g, double* E) {
    const int lane = this->lane;
    const double inc = p.increment;
    for (int i = lane; i < 2 * S; i += kWave) {
      const int n = i >> 1;
      E[i] = this->seg_energy(n, fd_time(Tb[n], i, inc));
    }
    __syncthreads();
    for (int n = lane; n < S; n += kWave)
      g[n] = p.w_d * (E[2 * n + 1] - E[2 * n]) / (2.0 * inc) + p.w_t * 1.0;
    __syncthreads();
  }
};

}  // namespace

// LDS bytes of the standard-pattern time kernels (without the optimiser's
// LN_SBPLX state).
__host__ __device__ inline size_t time_std_bytes(int N, int S, int D, bool soft) {
  const size_t base = sizeof(double) * static_cast<size_t>(stdp::layout(N, S, D).n);
  // soft: the coefficients (S x D x N), then the soft searches' scratch and
  // maxima (ext_soft_maxima_wave).
  return soft ? (base + 15) / 16 * 16 +
                    sizeof(double) * (S * D * N + kMaxSoftConstraints * (N + 2))
              : base;
}

}  // namespace mtg
