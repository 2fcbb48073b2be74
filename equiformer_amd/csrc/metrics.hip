// Running evaluation metrics on the device [ref: engine.py:136-139 evaluate, main_md17.py:451-462 evaluate, the OC20
// trainer's _compute_metrics (energy_trainer_v2.py:445-459) with the evaluator's energy_mae / energy_mse /
// energy_within_threshold].  The reference reads two to four scalars back per batch (`.item()`) and keeps the running
// averages on the host; here one launch per batch folds the batch into ten fp64 sums at a fixed device address, nothing is
// read back until the loop is over, and the launch can be captured in a HIP graph (equiformer_amd/evaluate.py).
//   * a batch is a few hundred rows: the launch is latency-bound whatever its shape, so ONE workgroup strides over the
//     rows (as the DeNS loss does, dens.hip).  Differences, norms and sums in fp64 from the fp32 inputs.
//   * partial sums meet by wave shuffles, then in LDS in wave order; thread 0 adds the batch total into `acc`.  No atomics,
//     no workspace: two runs give the same bits.
//   * excluded rows (>= n_graphs, node_mask 0) are never read: a NaN there reaches nothing.
#include "common.h"

namespace {

constexpr int MT_THREADS = EQF_METRICS_THREADS;
constexpr int MT_WAVES = MT_THREADS / 64;
constexpr int MT_Q = EQF_METRICS_SUMS;

__device__ __forceinline__ double mt_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// grid 1 x MT_THREADS
__global__ __launch_bounds__(MT_THREADS) void metrics_accumulate_kernel(
    const float* __restrict__ pred_y, const float* __restrict__ y, int n_graphs, const float* __restrict__ pred_dy,
    const float* __restrict__ dy, const float* __restrict__ node_mask, int N, double mean, double std, double threshold,
    double* __restrict__ acc) {
  __shared__ double part[MT_WAVES][MT_Q];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double a[MT_Q];
#pragma unroll
  for (int q = 0; q < MT_Q; ++q) a[q] = 0.0;
  for (int b = threadIdx.x; b < n_graphs; b += MT_THREADS) {
    const double p = pred_y[b], t = y[b];
    const double e = p * std + mean - t;
    const double ae = fabs(e);
    a[0] += 1.0;
    a[1] += fabs(p - (t - mean) / std);
    a[2] += ae;
    a[3] += e * e;
    a[4] += ae < threshold ? 1.0 : 0.0;
  }
  if (pred_dy) {
    for (int i = threadIdx.x; i < N; i += MT_THREADS) {
      if (node_mask && node_mask[i] == 0.f) continue;  // a phantom row of a padded batch: never read
      double n2 = 0.0;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const double p = pred_dy[3 * (long)i + c], t = dy[3 * (long)i + c];
        const double d = p - t / std, r = p * std - t;
        n2 += d * d;
        a[7] += fabs(d);
        a[8] += fabs(r);
        a[9] += r * r;
      }
      a[5] += 1.0;
      a[6] += sqrt(n2);
    }
  }
#pragma unroll
  for (int q = 0; q < MT_Q; ++q) {
    const double v = mt_wave_sum(a[q]);
    if (lane == 0) part[wave][q] = v;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
#pragma unroll
  for (int q = 0; q < MT_Q; ++q) {
    double t = part[0][q];
    for (int w = 1; w < MT_WAVES; ++w) t += part[w][q];
    acc[q] += t;
  }
}

}  // namespace

extern "C" {

int eqf_metrics_accumulate(const float* pred_y, const float* y, int n_graphs, const float* pred_dy, const float* dy,
                           const float* node_mask, int N, double task_mean, double task_std, double threshold, double* acc,
                           void* stream) {
  if (!pred_y || !y || !acc || n_graphs < 0 || N < 0) return EQF_E_BADARG;
  if (!(task_std > 0.0)) return EQF_E_BADARG;
  if (pred_dy && !dy) return EQF_E_BADARG;
  const bool forces = pred_dy && N > 0;
  if (n_graphs == 0 && !forces) return 0;
  hipLaunchKernelGGL(metrics_accumulate_kernel, dim3(1), dim3(MT_THREADS), 0, (hipStream_t)stream, pred_y, y, n_graphs,
                     forces ? pred_dy : nullptr, dy, node_mask, N, task_mean, task_std, threshold, acc);
  EQF_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
