// The running meters of the DeNS and IS2RE + IS2RS training loops, folded on the device one step at a time
// [ref: engine.py:23-27 AverageMeter.update(val, n); main_md17_dens.py:361-427 (three loss and three MAE meters, each weighted
// by a per-step count and skipped when that count is 0); energy_trainer_v2.py:247-317 (avg_metric_dict, one update per step)].
// The reference reads every step's means back with `.item()` and adds them on the host.  Here the loss kernels leave the means
// in their fp32 stats buffer and this launch adds them to fp64 (sum, count) pairs that stay on the device.
//   * at most 16 meters: ONE wave, lane i owns meter i and is the only writer of acc[2i], acc[2i+1].  No atomics, no LDS.
//   * an fp32 value times an fp32 weight (a count in stats) or an integer constant below 2^29 has at most 24 + 29 significant
//     bits: the product is exact in fp64, so a contracted multiply-add rounds as the separate multiply and add do, and the
//     sums equal the host's AverageMeter fed the same fp32 values, bit for bit.
//   * a meter whose weight is 0 does not read its value: a NaN mean of an empty atom set reaches nothing.
#include "common.h"

namespace {

constexpr int MF_THREADS = 64;

// the meter tables of one launch, copied from the caller's host arrays into the kernel arguments
struct MeterTables {
  int value[EQF_METERS_MAX];
  int weight[EQF_METERS_MAX];
  double weight_const[EQF_METERS_MAX];
};

// grid 1 x MF_THREADS
__global__ __launch_bounds__(MF_THREADS) void meter_fold_kernel(const float* __restrict__ stats, const float* __restrict__ loss,
                                                               int M, MeterTables t, double* __restrict__ acc) {
  const int i = threadIdx.x;
  if (i >= M) return;
  const int wi = t.weight[i], vi = t.value[i];
  const double w = wi >= 0 ? (double)stats[wi] : t.weight_const[i];
  if (w == 0.0) return;  // the reference's `if not loss_f.isnan()`: the meter is not updated
  const double v = vi >= 0 ? (double)stats[vi] : (double)loss[0];
  acc[2 * i] += v * w;
  acc[2 * i + 1] += w;
}

}  // namespace

extern "C" {

int eqf_meter_fold(const float* stats, int n_stats, const float* loss, int M, const int* value_index,
                   const int* weight_index, const double* weight_const, double* acc, void* stream) {
  if (!acc || !value_index || !weight_index || M < 1 || M > EQF_METERS_MAX || n_stats < 0) return EQF_E_BADARG;
  MeterTables t;
  for (int i = 0; i < M; ++i) {
    const int v = value_index[i], w = weight_index[i];
    if (v < -1 || v >= n_stats || w < -1 || w >= n_stats) return EQF_E_BADARG;
    if ((v >= 0 || w >= 0) && !stats) return EQF_E_BADARG;
    if (v == -1 && !loss) return EQF_E_BADARG;
    double c = 0.0;
    if (w == -1) {
      if (!weight_const) return EQF_E_BADARG;
      c = weight_const[i];
      // an integer in [0, 2^29): the product with an fp32 value stays exact in fp64 (NaN fails both tests)
      if (!(c >= 0.0 && c < 536870912.0) || c != (double)(long long)c) return EQF_E_BADARG;
    }
    t.value[i] = v;
    t.weight[i] = w;
    t.weight_const[i] = c;
  }
  for (int i = M; i < EQF_METERS_MAX; ++i) {
    t.value[i] = t.weight[i] = 0;
    t.weight_const[i] = 0.0;
  }
  hipLaunchKernelGGL(meter_fold_kernel, dim3(1), dim3(MF_THREADS), 0, (hipStream_t)stream, stats, loss, M, t, acc);
  EQF_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
