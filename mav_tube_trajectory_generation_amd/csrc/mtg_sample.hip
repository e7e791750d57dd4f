// mtg_sample.hip — batched trajectory sampling (Trajectory::evaluateRange,
// reference src/trajectory.cpp:74-134; the [t, p, v, a, j, s] rows of
// printMatlabSampledTrajectory, nonlinear_impl:2907-3003).  SURVEY.md §8f
// rank 3.
//
// The body is sample_row (mtg_sample_device.h), shared with the ragged
// kernel; here every row has S segments and rows are S apart.
#include <hip/hip_runtime.h>

#include "mtg_sample_device.h"

namespace mtg {

template <int N>
__global__ __launch_bounds__(kSampleBlock) void sample_kernel(
    int D, int S, const double* __restrict__ coeffs, const double* __restrict__ times,
    double t_start, double t_end_in, double dt, int n_max, int max_deriv,
    double* __restrict__ samples, double* __restrict__ sample_times,
    int32_t* __restrict__ n_samples) {
  extern __shared__ double dyn[];
  const int64_t b = blockIdx.y;
  sample_row<N>(D, S, S, coeffs + b * (S * D * N), times + b * S, b, t_start, t_end_in, dt, n_max,
                max_deriv, samples, sample_times, n_samples, dyn);
}

hipError_t launch_sample(int N, int D, int S, int64_t B, const double* coeffs,
                         const double* times, double t_start, double t_end, double dt,
                         int n_max, int max_deriv, double* samples, double* sample_times,
                         int32_t* n_samples, hipStream_t st) {
  return with_order(N, [&](auto n) {
    return launch(sample_kernel<n()>, sample_grid(n_max, B), kSampleBlock,
                  sample_lds_bytes(N, S, D, max_deriv), st, D, S, coeffs, times, t_start, t_end,
                  dt, n_max, max_deriv, samples, sample_times, n_samples);
  });
}

}  // namespace mtg
