// Collapsed edge-degree embedding (C ABI eqf_edgedeg_*; include/equiformer_hip.h).
//
// EdgeDegreeEmbeddingNetwork feeds its SeparableFCTP with the SAME row for every edge, a row whose only non-zero
// columns are the C channels x0 of the 0e segment.  Of the depth-wise paths only those with l1 == 0 (one per output
// degree l, coupling block == the (2l+1) components of Y_l) see anything but zeros, and radial last layer, depth-wise
// product and projection collapse into one small matrix per forward:
//
//   At[z_off_b + n, j] = sum_u W_b[out_ch_b + u, n] * x0[u] * W3[w_off_b + u, j]        a[...] alike with the offset
//   z = h At^T + a                                                          (the existing dense GEMM, not in this file)
//   node[i, node_off_b + k N_b + n] = s * (sum_{e in seg(i)} coupling[e, m_off_b + k] * z[e, z_off_b + n]
//                                          + [l_b == 0] deg(i) bias[n])
//
// Four kernels: the fold (parameters -> At, a), its backward (dAt, da -> the five parameter gradients, the rows that the
// zeros never reach WRITTEN as zeros), the segmented scatter over the dst-sorted CSR and its backward.  Plain fp32 FMAs,
// no atomics, a fixed summation order everywhere: results are bit-reproducible.
#include "common.h"
#include "prof.h"

namespace {

constexpr int MAXD = 7;  // 2 l + 1 of the highest degree handled (l <= 3)
constexpr int BWD_EDGES = 8;  // edges per block of the scatter's backward

__device__ __forceinline__ int block_of_col(const eqf_edgedeg& P, int zc) {
  int b = 0;
  while (b + 1 < P.nblk && zc >= P.z_off[b + 1]) ++b;
  return b;
}

// grid = Z rows of At, block = 64: thread j < H writes At[row, j], thread H writes a[row]
__global__ __launch_bounds__(64) void edgedeg_fold_fwd_kernel(const float* __restrict__ W3, const float* __restrict__ offset,
                                                              const float* __restrict__ expw, const float* __restrict__ expb,
                                                              const float* __restrict__ W, eqf_edgedeg P,
                                                              float* __restrict__ At, float* __restrict__ a) {
  extern __shared__ float sw[];  // [C]: W_b[out_ch + u, n] * x0[u]
  const int row = blockIdx.x;
  const int b = block_of_col(P, row);
  const int n = row - P.z_off[b];
  const float* Wb = W + P.pw_off[b] + (long)P.out_ch[b] * P.N[b] + n;
  for (int u = threadIdx.x; u < P.C; u += blockDim.x)
    sw[u] = Wb[(long)u * P.N[b]] * (expw[u] + (expb ? expb[u] : 0.f));
  __syncthreads();
  for (int j = threadIdx.x; j <= P.H; j += blockDim.x) {
    float acc = 0.f;
    if (j < P.H) {
      const float* w3 = W3 + (long)P.w_off[b] * P.H + j;
#pragma unroll 8
      for (int u = 0; u < P.C; ++u) acc = fmaf(sw[u], w3[(long)u * P.H], acc);
      At[(long)row * P.H + j] = acc;
    } else {
      const float* of = offset + P.w_off[b];
      for (int u = 0; u < P.C; ++u) acc = fmaf(sw[u], of[u], acc);
      a[row] = acc;
    }
  }
}

// blocks [0, C): channel u of every block b -- dW rows, dW3 rows, doffset, dx0[u]; the blocks behind them write the zeros
__global__ __launch_bounds__(256) void edgedeg_fold_bwd_kernel(const float* __restrict__ W3, const float* __restrict__ offset,
                                                               const float* __restrict__ expw, const float* __restrict__ expb,
                                                               const float* __restrict__ W, eqf_edgedeg P,
                                                               const float* __restrict__ dAt, const float* __restrict__ da,
                                                               float* __restrict__ dW3, float* __restrict__ doffset,
                                                               float* __restrict__ dW, float* __restrict__ dx0) {
  extern __shared__ float sm[];  // per block b the [H + 1] row of W3 | offset, then [blockDim] partial sums
  const int tid = threadIdx.x;
  if ((int)blockIdx.x >= P.C) {
    // zero fill: rows of W3 / offset outside every [w_off_b, w_off_b + C), rows of W outside every used block
    const long t0 = (long)(blockIdx.x - P.C) * blockDim.x + tid, step = (long)(gridDim.x - P.C) * blockDim.x;
    const long n3 = (long)P.w_numel * (P.H + 1);
    for (long i = t0; i < n3; i += step) {
      const int r = (int)(i / (P.H + 1)), j = (int)(i - (long)r * (P.H + 1));
      bool used = false;
      for (int b = 0; b < P.nblk; ++b) used |= (r >= P.w_off[b] && r < P.w_off[b] + P.C);
      if (!used) {
        if (j < P.H) dW3[(long)r * P.H + j] = 0.f;
        else doffset[r] = 0.f;
      }
    }
    for (long i = t0; i < P.pw_numel; i += step) {
      bool used = false;
      for (int b = 0; b < P.nblk; ++b) {
        const long rel = i - P.pw_off[b];
        if (rel >= 0 && rel < (long)P.K[b] * P.N[b]) {
          const int r = (int)(rel / P.N[b]);
          used = (r >= P.out_ch[b] && r < P.out_ch[b] + P.C);
        }
      }
      if (!used) dW[i] = 0.f;
    }
    return;
  }
  const int u = blockIdx.x, HW = P.H + 1;
  float* red = sm + P.nblk * HW;
  const float x0 = expw[u] + (expb ? expb[u] : 0.f);
  for (int i = tid; i < P.nblk * HW; i += blockDim.x) {
    const int b = i / HW, j = i - b * HW;
    const long wr = (long)P.w_off[b] + u;
    sm[i] = (j < P.H) ? W3[wr * P.H + j] : offset[wr];
  }
  __syncthreads();
  float part = 0.f;
  // Q[u, n] = <W3 row, dAt row n> + offset da[n]: one thread per column of z
  for (int zc = tid; zc < P.Z; zc += blockDim.x) {
    const int b = block_of_col(P, zc);
    const int n = zc - P.z_off[b], N = P.N[b];
    const float* w3 = sm + b * HW;
    const float* g = dAt + (long)zc * P.H;
    float q = 0.f;
#pragma unroll 8
    for (int j = 0; j < P.H; ++j) q = fmaf(w3[j], g[j], q);
    q = fmaf(w3[P.H], da[zc], q);
    const long wi = P.pw_off[b] + (long)(P.out_ch[b] + u) * N + n;
    dW[wi] = x0 * q;
    part = fmaf(W[wi], q, part);
  }
  // dW3[w_off + u, j] = x0 sum_n W[u, n] dAt[n, j]; column H is doffset: one thread per (block, j)
  for (int i = tid; i < P.nblk * HW; i += blockDim.x) {
    const int b = i / HW, j = i - b * HW, N = P.N[b];
    const long wr = (long)P.w_off[b] + u;
    const float* Wrow = W + P.pw_off[b] + (long)(P.out_ch[b] + u) * N;
    float acc = 0.f;
    if (j < P.H) {
      const float* g = dAt + (long)P.z_off[b] * P.H + j;
#pragma unroll 8
      for (int n = 0; n < N; ++n) acc = fmaf(Wrow[n], g[(long)n * P.H], acc);
      dW3[wr * P.H + j] = x0 * acc;
    } else {
      for (int n = 0; n < N; ++n) acc = fmaf(Wrow[n], da[P.z_off[b] + n], acc);
      doffset[wr] = x0 * acc;
    }
  }
  red[tid] = part;
  __syncthreads();
  for (int o = blockDim.x >> 1; o > 0; o >>= 1) {  // fixed tree: the same sum on every run
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  if (tid == 0) dx0[u] = red[0];
}

// one block per destination node; thread t owns the columns t, t + blockDim, ... of z and the (2l+1) node columns they feed
__global__ __launch_bounds__(256) void edgedeg_scatter_fwd_kernel(const float* __restrict__ z, const float* __restrict__ coupling,
                                                                  const int* __restrict__ row_ptr,
                                                                  const float* __restrict__ bias, eqf_edgedeg P, float s,
                                                                  float* __restrict__ node) {
  const int i = blockIdx.x;
  const int beg = row_ptr[i], end = row_ptr[i + 1];
  for (int zc = threadIdx.x; zc < P.Z; zc += blockDim.x) {
    const int b = block_of_col(P, zc);
    const int n = zc - P.z_off[b], d = 2 * P.l[b] + 1, N = P.N[b];
    float acc[MAXD];
#pragma unroll
    for (int k = 0; k < MAXD; ++k) acc[k] = 0.f;
    const float* zp = z + zc;
    const float* cp = coupling + P.m_off[b];
    for (int e = beg; e < end; ++e) {
      const float zv = zp[(long)e * P.Z];
      const float* c = cp + (long)e * P.m_numel;
#pragma unroll
      for (int k = 0; k < MAXD; ++k)
        if (k < d) acc[k] = fmaf(c[k], zv, acc[k]);
    }
    if (P.l[b] == 0 && bias) acc[0] = fmaf((float)(end - beg), bias[n], acc[0]);
    float* out = node + (long)i * P.D + P.node_off[b] + n;
#pragma unroll
    for (int k = 0; k < MAXD; ++k)
      if (k < d) out[(long)k * N] = s * acc[k];
  }
}

// blocks [0, nb_bias): dbias (8 columns each, 32 row lanes, summed in a fixed order); the rest: BWD_EDGES edges each
__global__ __launch_bounds__(256) void edgedeg_scatter_bwd_kernel(const float* __restrict__ dnode,
                                                                  const float* __restrict__ coupling,
                                                                  const int* __restrict__ dst, const int* __restrict__ row_ptr,
                                                                  eqf_edgedeg P, float s, int nnodes, int E, int nb_bias,
                                                                  int b0, float* __restrict__ dz, float* __restrict__ dbias) {
  __shared__ float red[256];
  const int tid = threadIdx.x;
  if ((int)blockIdx.x < nb_bias) {
    const int col = blockIdx.x * 8 + (tid & 7), lane = tid >> 3;
    float acc = 0.f;
    if (col < P.N[b0])
      for (int i = lane; i < nnodes; i += 32)
        acc = fmaf((float)(row_ptr[i + 1] - row_ptr[i]), dnode[(long)i * P.D + P.node_off[b0] + col], acc);
    red[tid] = acc;
    __syncthreads();
    if (lane == 0 && col < P.N[b0]) {
      float t = 0.f;
      for (int r = 0; r < 32; ++r) t += red[r * 8 + (tid & 7)];
      dbias[col] = s * t;
    }
    return;
  }
  const int e0 = (blockIdx.x - nb_bias) * BWD_EDGES;
  const int e1 = e0 + BWD_EDGES < E ? e0 + BWD_EDGES : E;
  for (int zc = tid; zc < P.Z; zc += blockDim.x) {
    const int b = block_of_col(P, zc);
    const int n = zc - P.z_off[b], d = 2 * P.l[b] + 1, N = P.N[b];
    for (int e = e0; e < e1; ++e) {
      const float* c = coupling + (long)e * P.m_numel + P.m_off[b];
      const float* g = dnode + (long)dst[e] * P.D + P.node_off[b] + n;
      float acc = 0.f;
#pragma unroll
      for (int k = 0; k < MAXD; ++k)
        if (k < d) acc = fmaf(c[k], g[(long)k * N], acc);
      dz[(long)e * P.Z + zc] = s * acc;
    }
  }
}

bool desc_ok(const eqf_edgedeg* P) {
  if (!P || P->nblk < 1 || P->nblk > EQF_MAX_SEG || P->C < 1 || P->H < 1 || P->Z < 1 || P->D < 1) return false;
  int z = 0;
  for (int b = 0; b < P->nblk; ++b) {
    if (P->l[b] < 0 || P->N[b] < 1 || P->K[b] < P->out_ch[b] + P->C || P->out_ch[b] < 0 || P->z_off[b] != z) return false;
    if (P->w_off[b] < 0 || P->w_off[b] + P->C > P->w_numel) return false;
    if (P->pw_off[b] < 0 || P->pw_off[b] + (long)P->K[b] * P->N[b] > P->pw_numel) return false;
    if (P->m_off[b] < 0 || P->m_off[b] + 2 * P->l[b] + 1 > P->m_numel) return false;
    if (P->node_off[b] < 0 || P->node_off[b] + (2 * P->l[b] + 1) * P->N[b] > P->D) return false;
    z += P->N[b];
  }
  return z == P->Z;
}

bool degrees_ok(const eqf_edgedeg* P) {
  for (int b = 0; b < P->nblk; ++b)
    if (2 * P->l[b] + 1 > MAXD) return false;
  return true;
}

}  // namespace

extern "C" {

int eqf_edgedeg_fold_fwd(const float* W3, const float* offset, const float* exp_w, const float* exp_b, const float* W,
                         const eqf_edgedeg* desc, float* At, float* a, void* stream) {
  if (!W3 || !offset || !exp_w || !W || !At || !a || !desc_ok(desc)) return EQF_E_BADARG;
  const eqf_edgedeg& P = *desc;
  hipStream_t st = (hipStream_t)stream;
  const int pid = eqf_prof_begin("edgedeg_fold_fwd", st, 2.0 * P.Z * (double)P.C * (P.H + 1),
                                 4.0 * (P.nblk * (double)P.C * (P.H + 1) + 2.0 * P.Z * (double)P.C + P.Z * (double)(P.H + 1)));
  hipLaunchKernelGGL(edgedeg_fold_fwd_kernel, dim3(P.Z), dim3(64), P.C * sizeof(float), st, W3, offset, exp_w, exp_b, W, P,
                     At, a);
  eqf_prof_end(pid, st);
  EQF_CHECK_LAUNCH();
  return 0;
}

int eqf_edgedeg_fold_bwd(const float* W3, const float* offset, const float* exp_w, const float* exp_b, const float* W,
                         const eqf_edgedeg* desc, const float* dAt, const float* da, float* dW3, float* doffset, float* dW,
                         float* dx0, void* stream) {
  if (!W3 || !offset || !exp_w || !W || !dAt || !da || !dW3 || !doffset || !dW || !dx0 || !desc_ok(desc)) return EQF_E_BADARG;
  const eqf_edgedeg& P = *desc;
  hipStream_t st = (hipStream_t)stream;
  const int pid = eqf_prof_begin("edgedeg_fold_bwd", st, 4.0 * P.Z * (double)P.C * (P.H + 1),
                                 4.0 * ((double)P.w_numel * (P.H + 1) + 2.0 * P.pw_numel + P.Z * (double)(P.H + 1)));
  hipLaunchKernelGGL(edgedeg_fold_bwd_kernel, dim3(P.C + 64), dim3(256), (P.nblk * (P.H + 1) + 256) * sizeof(float), st, W3, offset,
                     exp_w, exp_b, W, P, dAt, da, dW3, doffset, dW, dx0);
  eqf_prof_end(pid, st);
  EQF_CHECK_LAUNCH();
  return 0;
}

int eqf_edgedeg_scatter_fwd(const float* z, const float* coupling, const int* row_ptr, const float* bias,
                            const eqf_edgedeg* desc, float scale, float* node, int nnodes, int E, void* stream) {
  if (!z || !coupling || !row_ptr || !node || !desc_ok(desc) || E < 0) return EQF_E_BADARG;
  if (!degrees_ok(desc)) return EQF_E_UNSUPPORTED;
  if (nnodes <= 0) return 0;
  const eqf_edgedeg& P = *desc;
  hipStream_t st = (hipStream_t)stream;
  const int pid = eqf_prof_begin("edgedeg_scatter_fwd", st, 2.0 * (double)E * P.D,
                                 4.0 * ((double)E * (P.Z + P.m_numel) + (double)nnodes * P.D));
  hipLaunchKernelGGL(edgedeg_scatter_fwd_kernel, dim3(nnodes), dim3(P.Z > 128 ? 256 : 128), 0, st, z, coupling, row_ptr, bias, P, scale, node);
  eqf_prof_end(pid, st);
  EQF_CHECK_LAUNCH();
  return 0;
}

int eqf_edgedeg_scatter_bwd(const float* dnode, const float* coupling, const int* dst, const int* row_ptr,
                            const eqf_edgedeg* desc, float scale, float* dz, float* dbias, int nnodes, int E, void* stream) {
  if (!dnode || !coupling || !dst || !row_ptr || !dz || !desc_ok(desc)) return EQF_E_BADARG;
  if (!degrees_ok(desc)) return EQF_E_UNSUPPORTED;
  const eqf_edgedeg& P = *desc;
  int b0 = -1;
  for (int b = 0; b < P.nblk; ++b)
    if (P.l[b] == 0) b0 = b;
  if (dbias && b0 < 0) return EQF_E_BADARG;
  if (nnodes <= 0 || E < 0) return 0;
  const int nb_bias = dbias ? eqf_cdiv(P.N[b0], 8) : 0;
  if (E == 0 && nb_bias == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  const int pid = eqf_prof_begin("edgedeg_scatter_bwd", st, 2.0 * (double)E * P.D,
                                 4.0 * ((double)E * (P.Z + P.D + P.m_numel) + (double)nnodes * P.D));
  hipLaunchKernelGGL(edgedeg_scatter_bwd_kernel, dim3(nb_bias + eqf_cdiv(E, BWD_EDGES)), dim3(256), 0, st, dnode, coupling,
                     dst, row_ptr, P, scale, nnodes, E, nb_bias, b0 < 0 ? 0 : b0, dz, dbias);
  eqf_prof_end(pid, st);
  EQF_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
