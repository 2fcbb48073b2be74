// The energy / force training loss of the QM9, MD17 and plain IS2RE recipes, fused with their running meters
// [ref: engine.py:58-92 train_one_epoch (QM9: criterion on the normalised target, the loss and MAE meters), main_md17.py:380-400
// train_one_epoch (one criterion on energies and forces, the four meters), energy_trainer_v2.py:413-459 (the energy term of
// _compute_loss, _compute_metrics)].  Written with ATen the loss is a handful of launches per term and the meters cost two to
// four `.item()` read-backs per step; here it is one launch for the loss + the batch's share of the ten running sums of
// metrics.hip, one launch for its gradient, and nothing is read back: both can be captured in a HIP graph.
//   * a batch is a few hundred rows: the launches are latency-bound whatever their shape, so ONE workgroup strides over the
//     rows (as dens.hip, is2rs.hip and metrics.hip do).  Differences, norms and sums in fp64 from the fp32 inputs; partials
//     meet by wave shuffles, then in LDS in wave order: no atomics, no workspace, two runs give the same bits.
//   * excluded rows (energies >= n_graphs, atoms whose row_mask is 0) are never read: a NaN there reaches nothing.
//   * the backward recomputes the atom count from row_mask (first pass of its one workgroup): it reads nothing the forward
//     wrote, so a forward of a later batch cannot change what an earlier batch's backward sees.
#include "common.h"

namespace {

constexpr int TL_THREADS = 256;
constexpr int TL_WAVES = TL_THREADS / 64;
constexpr int TL_Q = EQF_METRICS_SUMS + 2;  // the ten sums of metrics.hip, sum d_e^2, sum d_ic^2

__device__ __forceinline__ double tl_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// grid 1 x TL_THREADS
__global__ __launch_bounds__(TL_THREADS) void ef_loss_fwd_kernel(
    const float* __restrict__ pred_y, const float* __restrict__ y, int n_graphs, const float* __restrict__ pred_dy,
    const float* __restrict__ dy, const float* __restrict__ row_mask, int N, const float* __restrict__ weights,
    int criterion, double mean, double std, double threshold, float* __restrict__ loss, double* __restrict__ acc) {
  __shared__ double part[TL_WAVES][TL_Q];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double a[TL_Q];
#pragma unroll
  for (int q = 0; q < TL_Q; ++q) a[q] = 0.0;
  for (int b = threadIdx.x; b < n_graphs; b += TL_THREADS) {
    const double p = pred_y[b], t = y[b];
    const double d = p - (t - mean) / std;
    const double e = p * std + mean - t;
    const double ae = fabs(e);
    a[0] += 1.0;
    a[1] += fabs(d);
    a[2] += ae;
    a[3] += e * e;
    a[4] += ae < threshold ? 1.0 : 0.0;
    a[10] += d * d;
  }
  if (pred_dy) {
    for (int i = threadIdx.x; i < N; i += TL_THREADS) {
      if (row_mask && row_mask[i] == 0.f) continue;  // a phantom row of a padded batch: never read
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
      a[11] += n2;
    }
  }
#pragma unroll
  for (int q = 0; q < TL_Q; ++q) {
    const double v = tl_wave_sum(a[q]);
    if (lane == 0) part[wave][q] = v;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  double t[TL_Q];
#pragma unroll
  for (int q = 0; q < TL_Q; ++q) {
    t[q] = part[0][q];
    for (int w = 1; w < TL_WAVES; ++w) t[q] += part[w][q];
  }
  const double le = (criterion == EQF_LOSS_L2 ? t[10] : t[1]) / n_graphs;
  double total = (double)weights[0] * le;
  const double n = t[5];
  if (pred_dy && n > 0) {  // an empty atom set adds an exact 0
    const double lf = criterion == EQF_LOSS_L2MAE ? t[6] / n : (criterion == EQF_LOSS_L2 ? t[11] : t[7]) / (3.0 * n);
    total += (double)weights[1] * lf;
  }
  loss[0] = (float)total;
  if (acc) {
#pragma unroll
    for (int q = 0; q < EQF_METRICS_SUMS; ++q) acc[q] += t[q];
  }
}

// grid 1 x TL_THREADS: the atom count first (the forward's predicate on row_mask), then one row per lane
__global__ __launch_bounds__(TL_THREADS) void ef_loss_bwd_kernel(
    const float* __restrict__ d_loss, const float* __restrict__ pred_y, const float* __restrict__ y, int n_graphs,
    int n_rows_y, const float* __restrict__ pred_dy, const float* __restrict__ dy, const float* __restrict__ row_mask, int N,
    const float* __restrict__ weights, int criterion, double mean, double std, float* __restrict__ d_pred_y,
    float* __restrict__ d_pred_dy) {
  __shared__ double part[TL_WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const double g = d_loss[0];
  const double ce = g * (double)weights[0] / n_graphs;
  for (int b = threadIdx.x; b < n_rows_y; b += TL_THREADS) {
    float o = 0.f;  // rows past n_graphs (the phantom molecule): exact zeros
    if (b < n_graphs) {
      const double d = (double)pred_y[b] - ((double)y[b] - mean) / std;
      o = (float)(criterion == EQF_LOSS_L2 ? 2.0 * ce * d : (d > 0 ? ce : (d < 0 ? -ce : 0.0)));
    }
    d_pred_y[b] = o;
  }
  if (!pred_dy) return;
  double n = N;
  if (row_mask) {
    double c = 0.0;
    for (int i = threadIdx.x; i < N; i += TL_THREADS) c += row_mask[i] == 0.f ? 0.0 : 1.0;
    c = tl_wave_sum(c);
    if (lane == 0) part[wave] = c;
    __syncthreads();
    n = part[0];
    for (int w = 1; w < TL_WAVES; ++w) n += part[w];
  }
  const double cf = n > 0 ? g * (double)weights[1] / (criterion == EQF_LOSS_L2MAE ? n : 3.0 * n) : 0.0;
  for (int i = threadIdx.x; i < N; i += TL_THREADS) {
    float o[3] = {0.f, 0.f, 0.f};  // phantom rows and (l2mae) rows whose difference vanishes: exact zeros
    if (!(row_mask && row_mask[i] == 0.f)) {
      double d[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) d[c] = (double)pred_dy[3 * (long)i + c] - (double)dy[3 * (long)i + c] / std;
      if (criterion == EQF_LOSS_L2MAE) {
        const double nrm = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
        if (nrm > 0) {
#pragma unroll
          for (int c = 0; c < 3; ++c) o[c] = (float)(cf / nrm * d[c]);
        }
      } else {
#pragma unroll
        for (int c = 0; c < 3; ++c)
          o[c] = (float)(criterion == EQF_LOSS_L2 ? 2.0 * cf * d[c] : (d[c] > 0 ? cf : (d[c] < 0 ? -cf : 0.0)));
      }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) d_pred_dy[3 * (long)i + c] = o[c];
  }
}

bool bad_criterion(int c) { return c != EQF_LOSS_L1 && c != EQF_LOSS_L2 && c != EQF_LOSS_L2MAE; }

}  // namespace

extern "C" {

int eqf_ef_loss_fwd(const float* pred_y, const float* y, int n_graphs, const float* pred_dy, const float* dy,
                    const float* row_mask, int N, const float* weights, int criterion, double task_mean, double task_std,
                    double threshold, float* loss, double* acc, void* stream) {
  if (!pred_y || !y || !weights || !loss || n_graphs < 1 || N < 0 || bad_criterion(criterion)) return EQF_E_BADARG;
  if (!(task_std > 0.0)) return EQF_E_BADARG;
  if (pred_dy && !dy) return EQF_E_BADARG;
  hipLaunchKernelGGL(ef_loss_fwd_kernel, dim3(1), dim3(TL_THREADS), 0, (hipStream_t)stream, pred_y, y, n_graphs, pred_dy,
                     dy, row_mask, N, weights, criterion, task_mean, task_std, threshold, loss, acc);
  EQF_CHECK_LAUNCH();
  return 0;
}

int eqf_ef_loss_bwd(const float* d_loss, const float* pred_y, const float* y, int n_graphs, int n_rows_y,
                    const float* pred_dy, const float* dy, const float* row_mask, int N, const float* weights, int criterion,
                    double task_mean, double task_std, float* d_pred_y, float* d_pred_dy, void* stream) {
  if (!d_loss || !pred_y || !y || !weights || !d_pred_y || n_graphs < 1 || n_rows_y < n_graphs || N < 0 ||
      bad_criterion(criterion))
    return EQF_E_BADARG;
  if (!(task_std > 0.0)) return EQF_E_BADARG;
  if (pred_dy && (!dy || !d_pred_dy)) return EQF_E_BADARG;
  hipLaunchKernelGGL(ef_loss_bwd_kernel, dim3(1), dim3(TL_THREADS), 0, (hipStream_t)stream, d_loss, pred_y, y, n_graphs,
                     n_rows_y, pred_dy, dy, row_mask, N, weights, criterion, task_mean, task_std, d_pred_y, d_pred_dy);
  EQF_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
