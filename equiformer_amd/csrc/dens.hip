// The DeNS training step around the model (denoising non-equilibrium structures): the corruption of a batch and the
// three-term loss with its metrics [ref: main_md17_dens.py:379-427 train_one_epoch, :514-548
// add_masked_gaussian_noise_to_pos].  Written with ATen the step is ~15 launches for the corruption and ~45 for the
// losses and meters, with a host read-back behind every boolean index, `isnan` test and `.item()`; here it is one launch
// for the corruption, one for the loss + metrics and one for the loss gradient, none of which reads anything back -- the
// loss launches can be captured in a HIP graph (equiformer_amd/capture.py).
//   * corruption: every random number is a pure function of (seed, stream tag, index) (rng.h), so the atoms of a molecule
//     recompute their molecule's draw instead of reducing over it, and the result does not depend on the grid.
//   * loss: a DeNS batch is a few hundred rows -- the launch is latency-bound whatever its shape, so ONE workgroup
//     grid-strides over the rows.  Differences, norms and sums in fp64 from the fp32 inputs; partials meet by wave
//     shuffles, then in LDS in wave order (no atomics, no workspace: two calls give the same bits).
#include <algorithm>
#include "common.h"
#include "rng.h"

namespace {

// stream tags of the corruption's three families of draws
constexpr unsigned long long DENS_TAG_MOL = 0, DENS_TAG_ATOM = 1, DENS_TAG_NOISE = 2;

constexpr int DL_THREADS = 256;
constexpr int DL_WAVES = DL_THREADS / 64;
constexpr int DL_Q = 8;  // quantities reduced by the forward

// one row per lane, grid-stride.  pos_out may alias pos (a lane reads its row before it writes it).
__global__ __launch_bounds__(256) void dens_corrupt_kernel(
    const float* __restrict__ pos, const float* __restrict__ dy, const int* __restrict__ batch, int N, float std,
    float prob, float corrupt_ratio, unsigned long long seed, float* pos_out, float* __restrict__ force,
    float* __restrict__ noise_vec, unsigned char* __restrict__ noise_mask, unsigned char* __restrict__ denoising_pos_mask) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (long)gridDim.x * blockDim.x) {
    const bool mol = eqf_rand_uniform(seed, DENS_TAG_MOL, (unsigned long long)(long long)batch[i]) < prob;
    bool m = mol;
    if (corrupt_ratio >= 0.f) m = m && (eqf_rand_uniform(seed, DENS_TAG_ATOM, (unsigned long long)i) < corrupt_ratio);
    denoising_pos_mask[i] = mol ? 1 : 0;
    noise_mask[i] = m ? 1 : 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const long e = 3 * i + c;
      // (separately rounded product and sum: pos_out is bit-for-bit the fp32 `pos + noise_vec` of the stored noise)
      const float nv = __fmul_rn(std, eqf_rand_normal(seed, DENS_TAG_NOISE, (unsigned long long)e));
      const float p = pos[e];
      noise_vec[e] = nv;
      pos_out[e] = m ? __fadd_rn(p, nv) : p;
      force[e] = m ? dy[e] : 0.f;
    }
  }
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// the row's target and scale by its own set: the denoising target on corrupted rows, the force elsewhere
struct DensRow {
  double dx, dy, dz;  // pred - target / scale
  double nrm;         // |d|
  double abs_err;     // sum_c |pred_c * scale - target_c|
};

__device__ __forceinline__ DensRow dens_row(const float* __restrict__ pred_dy, const float* __restrict__ dy,
                                            const float* __restrict__ noise_vec, long i, bool masked, double std,
                                            double noise_std) {
  const float* __restrict__ t = masked ? noise_vec : dy;
  const double s = masked ? noise_std : std;
  const double px = pred_dy[3 * i], py = pred_dy[3 * i + 1], pz = pred_dy[3 * i + 2];
  const double tx = t[3 * i], ty = t[3 * i + 1], tz = t[3 * i + 2];
  DensRow r;
  r.dx = px - tx / s, r.dy = py - ty / s, r.dz = pz - tz / s;
  r.nrm = sqrt(r.dx * r.dx + r.dy * r.dy + r.dz * r.dz);
  r.abs_err = fabs(px * s - tx) + fabs(py * s - ty) + fabs(pz * s - tz);
  return r;
}

// grid 1 x DL_THREADS
__global__ __launch_bounds__(DL_THREADS) void dens_loss_fwd_kernel(
    const float* __restrict__ pred_y, const float* __restrict__ y, const float* __restrict__ pred_dy,
    const float* __restrict__ dy, const float* __restrict__ noise_vec, const unsigned char* __restrict__ noise_mask,
    const float* __restrict__ row_mask, const float* __restrict__ weights, int N, int nB, double mean, double std,
    double noise_std, float* __restrict__ loss, float* __restrict__ stats) {
  __shared__ double part[DL_WAVES][DL_Q];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // 0 sum |e|, 1 sum |e| in the target's units, 2 / 3 sum of norms (force / denoising rows), 4 / 5 sum of absolute
  // component errors, 6 / 7 rows
  double a[DL_Q] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int b = threadIdx.x; b < nB; b += DL_THREADS) {
    const double p = pred_y[b], t = y[b];
    a[0] += fabs(p - (t - mean) / std);
    a[1] += fabs(p * std + mean - t);
  }
  for (int i = threadIdx.x; i < N; i += DL_THREADS) {
    if (row_mask && row_mask[i] == 0.f) continue;  // a phantom row of a padded batch: never read
    const bool masked = noise_mask[i] != 0;
    const DensRow r = dens_row(pred_dy, dy, noise_vec, i, masked, std, noise_std);
    a[2] += masked ? 0.0 : r.nrm;
    a[3] += masked ? r.nrm : 0.0;
    a[4] += masked ? 0.0 : r.abs_err;
    a[5] += masked ? r.abs_err : 0.0;
    a[6] += masked ? 0.0 : 1.0;
    a[7] += masked ? 1.0 : 0.0;
  }
#pragma unroll
  for (int q = 0; q < DL_Q; ++q) {
    const double v = wave_sum_f64(a[q]);
    if (lane == 0) part[wave][q] = v;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  double t[DL_Q];
#pragma unroll
  for (int q = 0; q < DL_Q; ++q) {
    t[q] = part[0][q];
    for (int w = 1; w < DL_WAVES; ++w) t[q] += part[w][q];
  }
  const double nf = t[6], nd = t[7];
  // an empty row set contributes an exact zero (the reference gets NaN from the empty mean and skips the term)
  const double le = t[0] / nB, lf = nf > 0 ? t[2] / nf : 0.0, ld = nd > 0 ? t[3] / nd : 0.0;
  double total = (double)weights[0] * le;
  if (nf > 0) total += (double)weights[1] * lf;
  if (nd > 0) total += (double)weights[2] * ld;
  loss[0] = (float)total;
  stats[0] = (float)le;
  stats[1] = (float)lf;
  stats[2] = (float)ld;
  stats[3] = (float)nf;
  stats[4] = (float)nd;
  stats[5] = (float)(t[1] / nB);
  stats[6] = nf > 0 ? (float)(t[4] / (3.0 * nf)) : 0.f;
  stats[7] = nd > 0 ? (float)(t[5] / (3.0 * nd)) : 0.f;
}

// one row per lane, grid-stride over max(N, nB)
__global__ __launch_bounds__(DL_THREADS) void dens_loss_bwd_kernel(
    const float* __restrict__ d_loss, const float* __restrict__ pred_y, const float* __restrict__ y,
    const float* __restrict__ pred_dy, const float* __restrict__ dy, const float* __restrict__ noise_vec,
    const unsigned char* __restrict__ noise_mask, const float* __restrict__ row_mask, const float* __restrict__ weights,
    const float* __restrict__ stats, int N, int nB, double mean, double std, double noise_std,
    float* __restrict__ d_pred_y, float* __restrict__ d_pred_dy) {
  const double g = d_loss[0];
  const double ce = g * (double)weights[0] / nB;
  const double nf = stats[3], nd = stats[4];
  const double cf = nf > 0 ? g * (double)weights[1] / nf : 0.0, cd = nd > 0 ? g * (double)weights[2] / nd : 0.0;
  const int rows = max(N, nB);
  for (int i = blockIdx.x * DL_THREADS + threadIdx.x; i < rows; i += gridDim.x * DL_THREADS) {
    if (i < nB) {
      const double e = (double)pred_y[i] - ((double)y[i] - mean) / std;
      d_pred_y[i] = (float)(e > 0 ? ce : (e < 0 ? -ce : 0.0));
    }
    if (i < N) {
      float ox = 0.f, oy = 0.f, oz = 0.f;  // phantom rows and rows whose difference vanishes: exact zeros
      if (!(row_mask && row_mask[i] == 0.f)) {
        const bool masked = noise_mask[i] != 0;
        const DensRow r = dens_row(pred_dy, dy, noise_vec, i, masked, std, noise_std);
        if (r.nrm > 0) {
          const double c = (masked ? cd : cf) / r.nrm;
          ox = (float)(c * r.dx), oy = (float)(c * r.dy), oz = (float)(c * r.dz);
        }
      }
      d_pred_dy[3 * (long)i] = ox, d_pred_dy[3 * (long)i + 1] = oy, d_pred_dy[3 * (long)i + 2] = oz;
    }
  }
}

}  // namespace

extern "C" {

int eqf_dens_corrupt(const float* pos, const float* dy, const int* batch, int N, float std, float prob,
                     float corrupt_ratio, unsigned long long seed, float* pos_out, float* force, float* noise_vec,
                     unsigned char* noise_mask, unsigned char* denoising_pos_mask, void* stream) {
  if (N < 0 || !(std >= 0.f)) return EQF_E_BADARG;
  if (N == 0) return 0;
  if (!pos || !dy || !batch || !pos_out || !force || !noise_vec || !noise_mask || !denoising_pos_mask) return EQF_E_BADARG;
  const int blocks = std::min(eqf_cdiv(N, 256), 1024);
  hipLaunchKernelGGL(dens_corrupt_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, pos, dy, batch, N, std, prob,
                     corrupt_ratio, seed, pos_out, force, noise_vec, noise_mask, denoising_pos_mask);
  EQF_CHECK_LAUNCH();
  return 0;
}

int eqf_dens_loss_fwd(const float* pred_y, const float* y, const float* pred_dy, const float* dy, const float* noise_vec,
                      const unsigned char* noise_mask, const float* row_mask, const float* weights, int N, int nB,
                      double task_mean, double task_std, double noise_std, float* loss, float* stats, void* stream) {
  if (N < 0 || nB <= 0 || !pred_y || !y || !weights || !loss || !stats) return EQF_E_BADARG;
  if (N > 0 && (!pred_dy || !dy || !noise_vec || !noise_mask)) return EQF_E_BADARG;
  if (!(task_std != 0.0) || !(noise_std != 0.0)) return EQF_E_BADARG;
  hipLaunchKernelGGL(dens_loss_fwd_kernel, dim3(1), dim3(DL_THREADS), 0, (hipStream_t)stream, pred_y, y, pred_dy, dy,
                     noise_vec, noise_mask, row_mask, weights, N, nB, task_mean, task_std, noise_std, loss, stats);
  EQF_CHECK_LAUNCH();
  return 0;
}

int eqf_dens_loss_bwd(const float* d_loss, const float* pred_y, const float* y, const float* pred_dy, const float* dy,
                      const float* noise_vec, const unsigned char* noise_mask, const float* row_mask, const float* weights,
                      const float* stats, int N, int nB, double task_mean, double task_std, double noise_std,
                      float* d_pred_y, float* d_pred_dy, void* stream) {
  if (N < 0 || nB <= 0 || !d_loss || !pred_y || !y || !weights || !stats || !d_pred_y) return EQF_E_BADARG;
  if (N > 0 && (!pred_dy || !dy || !noise_vec || !noise_mask || !d_pred_dy)) return EQF_E_BADARG;
  if (!(task_std != 0.0) || !(noise_std != 0.0)) return EQF_E_BADARG;
  const int blocks = std::min(eqf_cdiv(std::max(N, nB), DL_THREADS), 1024);
  hipLaunchKernelGGL(dens_loss_bwd_kernel, dim3(blocks), dim3(DL_THREADS), 0, (hipStream_t)stream, d_loss, pred_y, y,
                     pred_dy, dy, noise_vec, noise_mask, row_mask, weights, stats, N, nB, task_mean, task_std, noise_std,
                     d_pred_y, d_pred_dy);
  EQF_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
