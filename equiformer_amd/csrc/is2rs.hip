// The IS2RE + IS2RS training step around the OC20 model (relaxed energy + every free atom's displacement to its relaxed
// position): the Noisy-Nodes perturbation of a batch and the two-term loss with its metrics
// [ref: oc20/trainer/base_trainer_v2.py:81-126 interpolate_init_relaxed_pos, oc20/trainer/energy_trainer_v2.py:413-442
// _compute_loss, :445-459 _compute_metrics].  Written with ATen the step is ~30 launches with a host read-back behind each
// boolean index (`batch.pos[tags] = new_pos[tags]`, `_mask_input(out['pos'], tag_mask)`); here it is one launch for the
// perturbation, one for the loss + metrics and one for the loss gradient, none of which reads anything back -- the loss
// launches can be captured in a HIP graph (equiformer_amd/capture.py).  The structure is that of dens.hip:
//   * perturbation: every random number is a pure function of (seed, stream tag, index) (rng.h), so the atoms of a
//     structure recompute their structure's draw instead of reducing over it, and the result does not depend on the grid.
//   * loss: ONE workgroup grid-strides over the rows (a batch is a few thousand rows at most: latency-bound whatever its
//     shape).  Differences and sums in fp64 from the fp32 inputs; partials meet by wave shuffles, then in LDS in wave order
//     (no atomics, no workspace: two calls give the same bits).
// `tags` keeps the integer type of the caller (int64 from a loader, int32 elsewhere): the kernels are templated on it, so
// no conversion launch stands in front of them.
#include <algorithm>
#include "common.h"
#include "rng.h"

// No product of this file may be fused with the sum that follows it: the perturbed position is specified as separately
// rounded fp32 operations, which a test recomputes bit for bit with eager torch on the CPU.  HIP's __fmul_rn / __fadd_rn /
// __fsub_rn do not promise that (without OCML's rounded operations they are the plain operators, and the default
// -ffp-contract of hipcc may fuse those across the call), so the operations are written as operators under this pragma.
#pragma clang fp contract(off)

namespace {

// stream tags of the perturbation's three families of draws (apart from those of dens.hip)
constexpr unsigned long long IS2RS_TAG_STRUCT = 16, IS2RS_TAG_FACTOR = 17, IS2RS_TAG_NOISE = 18;

constexpr int IL_THREADS = 256;
constexpr int IL_WAVES = IL_THREADS / 64;
constexpr int IL_Q = 7;  // quantities reduced by the forward

// one row per lane, grid-stride.  pos_out may alias pos (a lane reads its row before it writes it).
template <typename TagT>
__global__ __launch_bounds__(256) void is2rs_perturb_kernel(
    const float* pos, const float* __restrict__ pos_relaxed, const TagT* __restrict__ tags, const int* __restrict__ batch,
    int N, float p_perturb, float f_min, float noise_std, unsigned long long seed, float* pos_out,
    float* __restrict__ factor, float* __restrict__ noise_vec, unsigned char* __restrict__ selected) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (long)gridDim.x * blockDim.x) {
    const bool sel = eqf_rand_uniform(seed, IS2RS_TAG_STRUCT, (unsigned long long)(long long)batch[i]) < p_perturb;
    // f_min + (1 - f_min) u with u in [0, 1): below 1 in exact arithmetic; the clamp keeps the rounded value there too
    const float u = eqf_rand_uniform(seed, IS2RS_TAG_FACTOR, (unsigned long long)i);
    const float f = fminf(f_min + (1.f - f_min) * u, 0x1.fffffep-1f);
    const bool move = sel && tags[i] > 0;
    selected[i] = sel ? 1 : 0;
    factor[i] = f;
    const float g = 1.f - f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const long e = 3 * i + c;
      const float nv = noise_std * eqf_rand_normal(seed, IS2RS_TAG_NOISE, (unsigned long long)e);
      const float p = pos[e];
      noise_vec[e] = nv;
      // (separately rounded, see the pragma above: pos_out is bit-for-bit the fp32 `pos * f + (1 - f) * pos_relaxed + noise`
      // of the stored factor and noise)
      const float t1 = p * f, t2 = g * pos_relaxed[e];
      const float moved = (t1 + t2) + nv;
      pos_out[e] = move ? moved : p;
    }
  }
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

struct Is2rsNorm {
  double e_mean, e_std;
  double p_mean[3], p_std[3];
};

// grid 1 x IL_THREADS
template <typename TagT>
__global__ __launch_bounds__(IL_THREADS) void is2rs_loss_fwd_kernel(
    const float* __restrict__ pred_y, const float* __restrict__ y, const float* __restrict__ pred_pos,
    const float* __restrict__ pos, const float* __restrict__ pos_relaxed, const TagT* __restrict__ tags,
    const float* __restrict__ row_mask, const float* __restrict__ weights, int N, int nB, Is2rsNorm nm, double threshold,
    float* __restrict__ loss, float* __restrict__ stats) {
  __shared__ double part[IL_WAVES][IL_Q];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // 0 sum |e| (normalised), 1 sum |e| / 2 sum e^2 / 3 structures with |e| < threshold (the target's units), 4 sum of
  // absolute component differences (normalised) / 5 the same in Angstrom, 6 free rows
  double a[IL_Q] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int b = threadIdx.x; b < nB; b += IL_THREADS) {
    const double p = pred_y[b], t = y[b];
    a[0] += fabs(p - (t - nm.e_mean) / nm.e_std);
    const double err = fabs(p * nm.e_std + nm.e_mean - t);
    a[1] += err;
    a[2] += err * err;
    a[3] += err < threshold ? 1.0 : 0.0;
  }
  for (int i = threadIdx.x; i < N; i += IL_THREADS) {
    if (row_mask && row_mask[i] == 0.f) continue;  // a phantom row of a padded batch: never read
    if (!(tags[i] > 0)) continue;                  // a fixed atom
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const long e = 3 * (long)i + c;
      const double p = pred_pos[e], delta = (double)pos_relaxed[e] - (double)pos[e];
      a[4] += fabs(p - (delta - nm.p_mean[c]) / nm.p_std[c]);
      a[5] += fabs(p * nm.p_std[c] + nm.p_mean[c] - delta);
    }
    a[6] += 1.0;
  }
#pragma unroll
  for (int q = 0; q < IL_Q; ++q) {
    const double v = wave_sum_f64(a[q]);
    if (lane == 0) part[wave][q] = v;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  double t[IL_Q];
#pragma unroll
  for (int q = 0; q < IL_Q; ++q) {
    t[q] = part[0][q];
    for (int w = 1; w < IL_WAVES; ++w) t[q] += part[w][q];
  }
  const double nf = t[6];
  // an empty free set contributes an exact zero (the reference gets NaN from the empty mean)
  const double le = t[0] / nB, la = nf > 0 ? t[4] / (3.0 * nf) : 0.0;
  double total = (double)weights[0] * le;
  if (nf > 0) total += (double)weights[1] * la;
  loss[0] = (float)total;
  stats[0] = (float)le;
  stats[1] = (float)la;
  stats[2] = (float)nf;
  stats[3] = (float)(t[1] / nB);
  stats[4] = (float)(t[2] / nB);
  stats[5] = (float)(t[3] / nB);
  stats[6] = nf > 0 ? (float)(t[5] / (3.0 * nf)) : 0.f;
  stats[7] = 0.f;
}

// one row per lane, grid-stride over max(N, nB)
template <typename TagT>
__global__ __launch_bounds__(IL_THREADS) void is2rs_loss_bwd_kernel(
    const float* __restrict__ d_loss, const float* __restrict__ pred_y, const float* __restrict__ y,
    const float* __restrict__ pred_pos, const float* __restrict__ pos, const float* __restrict__ pos_relaxed,
    const TagT* __restrict__ tags, const float* __restrict__ row_mask, const float* __restrict__ weights,
    const float* __restrict__ stats, int N, int nB, Is2rsNorm nm, float* __restrict__ d_pred_y,
    float* __restrict__ d_pred_pos) {
  const double g = d_loss[0];
  const double ce = g * (double)weights[0] / nB;
  const double nf = stats[2];
  const double ca = nf > 0 ? g * (double)weights[1] / (3.0 * nf) : 0.0;
  const int rows = max(N, nB);
  for (int i = blockIdx.x * IL_THREADS + threadIdx.x; i < rows; i += gridDim.x * IL_THREADS) {
    if (i < nB) {
      const double e = (double)pred_y[i] - ((double)y[i] - nm.e_mean) / nm.e_std;
      d_pred_y[i] = (float)(e > 0 ? ce : (e < 0 ? -ce : 0.0));
    }
    if (i < N) {
      float o[3] = {0.f, 0.f, 0.f};  // phantom rows, fixed atoms and components whose difference vanishes: exact zeros
      if (!(row_mask && row_mask[i] == 0.f) && tags[i] > 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const long e = 3 * (long)i + c;
          const double delta = (double)pos_relaxed[e] - (double)pos[e];
          const double d = (double)pred_pos[e] - (delta - nm.p_mean[c]) / nm.p_std[c];
          o[c] = (float)(d > 0 ? ca : (d < 0 ? -ca : 0.0));
        }
      }
      d_pred_pos[3 * (long)i] = o[0], d_pred_pos[3 * (long)i + 1] = o[1], d_pred_pos[3 * (long)i + 2] = o[2];
    }
  }
}

inline Is2rsNorm is2rs_norm(double e_mean, double e_std, double pmx, double pmy, double pmz, double psx, double psy,
                            double psz) {
  Is2rsNorm nm;
  nm.e_mean = e_mean, nm.e_std = e_std;
  nm.p_mean[0] = pmx, nm.p_mean[1] = pmy, nm.p_mean[2] = pmz;
  nm.p_std[0] = psx, nm.p_std[1] = psy, nm.p_std[2] = psz;
  return nm;
}

}  // namespace

extern "C" {

int eqf_is2rs_perturb(const float* pos, const float* pos_relaxed, const void* tags, int tags_is64, const int* batch, int N,
                      float p_perturb, float f_min, float noise_std, unsigned long long seed, float* pos_out,
                      float* factor, float* noise_vec, unsigned char* selected, void* stream) {
  if (N < 0 || !(noise_std >= 0.f) || !(f_min >= 0.f && f_min <= 1.f)) return EQF_E_BADARG;
  if (N == 0) return 0;
  if (!pos || !pos_relaxed || !tags || !batch || !pos_out || !factor || !noise_vec || !selected) return EQF_E_BADARG;
  const int blocks = std::min(eqf_cdiv(N, 256), 1024);
  if (tags_is64)
    hipLaunchKernelGGL(is2rs_perturb_kernel<long long>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, pos, pos_relaxed,
                       (const long long*)tags, batch, N, p_perturb, f_min, noise_std, seed, pos_out, factor, noise_vec,
                       selected);
  else
    hipLaunchKernelGGL(is2rs_perturb_kernel<int>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, pos, pos_relaxed,
                       (const int*)tags, batch, N, p_perturb, f_min, noise_std, seed, pos_out, factor, noise_vec, selected);
  EQF_CHECK_LAUNCH();
  return 0;
}

int eqf_is2rs_loss_fwd(const float* pred_y, const float* y, const float* pred_pos, const float* pos,
                       const float* pos_relaxed, const void* tags, int tags_is64, const float* row_mask,
                       const float* weights, int N, int nB, double e_mean, double e_std, double p_mean_x, double p_mean_y,
                       double p_mean_z, double p_std_x, double p_std_y, double p_std_z, double threshold, float* loss,
                       float* stats, void* stream) {
  if (N < 0 || nB <= 0 || !pred_y || !y || !weights || !loss || !stats) return EQF_E_BADARG;
  if (N > 0 && (!pred_pos || !pos || !pos_relaxed || !tags)) return EQF_E_BADARG;
  if (!(e_std != 0.0) || !(p_std_x != 0.0) || !(p_std_y != 0.0) || !(p_std_z != 0.0)) return EQF_E_BADARG;
  const Is2rsNorm nm = is2rs_norm(e_mean, e_std, p_mean_x, p_mean_y, p_mean_z, p_std_x, p_std_y, p_std_z);
  if (tags_is64)
    hipLaunchKernelGGL(is2rs_loss_fwd_kernel<long long>, dim3(1), dim3(IL_THREADS), 0, (hipStream_t)stream, pred_y, y,
                       pred_pos, pos, pos_relaxed, (const long long*)tags, row_mask, weights, N, nB, nm, threshold, loss,
                       stats);
  else
    hipLaunchKernelGGL(is2rs_loss_fwd_kernel<int>, dim3(1), dim3(IL_THREADS), 0, (hipStream_t)stream, pred_y, y, pred_pos,
                       pos, pos_relaxed, (const int*)tags, row_mask, weights, N, nB, nm, threshold, loss, stats);
  EQF_CHECK_LAUNCH();
  return 0;
}

int eqf_is2rs_loss_bwd(const float* d_loss, const float* pred_y, const float* y, const float* pred_pos, const float* pos,
                       const float* pos_relaxed, const void* tags, int tags_is64, const float* row_mask,
                       const float* weights, const float* stats, int N, int nB, double e_mean, double e_std,
                       double p_mean_x, double p_mean_y, double p_mean_z, double p_std_x, double p_std_y, double p_std_z,
                       float* d_pred_y, float* d_pred_pos, void* stream) {
  if (N < 0 || nB <= 0 || !d_loss || !pred_y || !y || !weights || !stats || !d_pred_y) return EQF_E_BADARG;
  if (N > 0 && (!pred_pos || !pos || !pos_relaxed || !tags || !d_pred_pos)) return EQF_E_BADARG;
  if (!(e_std != 0.0) || !(p_std_x != 0.0) || !(p_std_y != 0.0) || !(p_std_z != 0.0)) return EQF_E_BADARG;
  const Is2rsNorm nm = is2rs_norm(e_mean, e_std, p_mean_x, p_mean_y, p_mean_z, p_std_x, p_std_y, p_std_z);
  const int blocks = std::min(eqf_cdiv(std::max(N, nB), IL_THREADS), 1024);
  if (tags_is64)
    hipLaunchKernelGGL(is2rs_loss_bwd_kernel<long long>, dim3(blocks), dim3(IL_THREADS), 0, (hipStream_t)stream, d_loss,
                       pred_y, y, pred_pos, pos, pos_relaxed, (const long long*)tags, row_mask, weights, stats, N, nB, nm,
                       d_pred_y, d_pred_pos);
  else
    hipLaunchKernelGGL(is2rs_loss_bwd_kernel<int>, dim3(blocks), dim3(IL_THREADS), 0, (hipStream_t)stream, d_loss, pred_y,
                       y, pred_pos, pos, pos_relaxed, (const int*)tags, row_mask, weights, stats, N, nB, nm, d_pred_y,
                       d_pred_pos);
  EQF_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
