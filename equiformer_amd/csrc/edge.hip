// Edge-wise gather / scatter and attention kernels over the dst-sorted radius graph (HBM-bound).
//
// Edges are stored sorted by destination node (CSR row_ptr), so every "scatter" of the reference
// (torch_scatter atomics) becomes a segmented reduction: one workgroup / wavefront owns one destination
// row, reads its incoming edge rows coalesced (1920-byte rows for 480 channels) and writes the node row
// once -- no atomics, deterministic.  The softmax over incoming edges is reduced with wavefront shuffles.
#include "common.h"
#include "prof.h"
#include "rng.h"

namespace {

// ---------------------------------------------------------------------------------------------- gather
__global__ __launch_bounds__(256) void gather_add_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                         const int* __restrict__ src, const int* __restrict__ dst,
                                                         float* __restrict__ msg, long total4, int D4) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total4) return;
  const long e = idx / D4;
  const int c = (int)(idx - e * D4);
  float4 v = reinterpret_cast<const float4*>(a)[(long)src[e] * D4 + c];
  if (b) {
    const float4 w = reinterpret_cast<const float4*>(b)[(long)dst[e] * D4 + c];
    v.x += w.x, v.y += w.y, v.z += w.z, v.w += w.w;
  }
  reinterpret_cast<float4*>(msg)[idx] = v;
}

// Rows of at least GATHER_ROW_MIN_D4 float4 columns (QM9: 120).  The kernel above pays, per float4, a 64-bit division and
// two dependent round trips (src[e] / dst[e], then the node rows).  Here a wavefront owns GATHER_ROWS consecutive edges: the
// edge index is wave-uniform (readfirstlane), so the index loads of all its edges go out together on the scalar unit, and the
// lanes stride the float4 columns with the 2 x GATHER_ROWS row loads of a column step requested before the first is used.
// Edges past E are clamped to E - 1 and not stored.  msg = a[src] + b[dst], the same single add per element.
constexpr int GATHER_ROW_MIN_D4 = 32;
constexpr int GATHER_WAVES = 4, GATHER_ROWS = 4;

__global__ __launch_bounds__(64 * GATHER_WAVES) void gather_add_rows_kernel(
    const float* __restrict__ a, const float* __restrict__ b, const int* __restrict__ src, const int* __restrict__ dst,
    float* __restrict__ msg, int E, int D4) {
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int lane = (int)(threadIdx.x & 63);
  const int e0 = ((int)blockIdx.x * GATHER_WAVES + wave) * GATHER_ROWS;
  if (e0 >= E) return;
  const float4* ra[GATHER_ROWS];
  const float4* rb[GATHER_ROWS];
#pragma unroll
  for (int j = 0; j < GATHER_ROWS; ++j) {
    const int e = min(e0 + j, E - 1);
    ra[j] = reinterpret_cast<const float4*>(a) + (long)src[e] * D4;
    rb[j] = b ? reinterpret_cast<const float4*>(b) + (long)dst[e] * D4 : nullptr;
  }
  for (int c = lane; c < D4; c += 64) {
    float4 v[GATHER_ROWS], w[GATHER_ROWS];
#pragma unroll
    for (int j = 0; j < GATHER_ROWS; ++j) v[j] = ra[j][c];
    if (b) {
#pragma unroll
      for (int j = 0; j < GATHER_ROWS; ++j) w[j] = rb[j][c];
#pragma unroll
      for (int j = 0; j < GATHER_ROWS; ++j) v[j].x += w[j].x, v[j].y += w[j].y, v[j].z += w[j].z, v[j].w += w[j].w;
    }
#pragma unroll
    for (int j = 0; j < GATHER_ROWS; ++j)
      if (e0 + j < E) reinterpret_cast<float4*>(msg)[(long)(e0 + j) * D4 + c] = v[j];
  }
}

// segment n of one segmented sum; one workgroup of 128
__device__ __forceinline__ void segment_sum_block(const float* __restrict__ x, const int* __restrict__ ptr,
                                                  const int* __restrict__ perm, float* __restrict__ out, int D,
                                                  float scale, int accumulate, int n) {
  const int beg = ptr[n], end = ptr[n + 1];
  if ((D & 3) == 0) {
    const int D4 = D >> 2;
    for (int c = threadIdx.x; c < D4; c += blockDim.x) {
      float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
      // four rows per step, their index and value loads in flight together (a row is ~11 entries: one load per iteration of a
      // run-time loop made the kernel a chain of 2 x 11 dependent memory round trips); same summation order as before
      for (int q = beg; q < end; q += 4) {
        long row[4];
        float4 v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int qq = min(q + j, end - 1);
          row[j] = perm ? perm[qq] : qq;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = reinterpret_cast<const float4*>(x)[row[j] * D4 + c];
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (q + j < end) acc.x += v[j].x, acc.y += v[j].y, acc.z += v[j].z, acc.w += v[j].w;
      }
      acc.x *= scale, acc.y *= scale, acc.z *= scale, acc.w *= scale;
      float4* o = reinterpret_cast<float4*>(out) + (long)n * D4 + c;
      if (accumulate) {
        const float4 p = *o;
        acc.x += p.x, acc.y += p.y, acc.z += p.z, acc.w += p.w;
      }
      *o = acc;
    }
  } else {
    for (int c = threadIdx.x; c < D; c += blockDim.x) {
      float acc = 0.f;
      for (int q = beg; q < end; ++q) {
        const long row = perm ? perm[q] : q;
        acc += x[row * D + c];
      }
      acc *= scale;
      float* o = out + (long)n * D + c;
      *o = accumulate ? *o + acc : acc;
    }
  }
}

__global__ __launch_bounds__(128) void segment_sum_kernel(const float* __restrict__ x, const int* __restrict__ ptr,
                                                          const int* __restrict__ perm, float* __restrict__ out, int D,
                                                          float scale, int accumulate) {
  segment_sum_block(x, ptr, perm, out, D, scale, accumulate, (int)blockIdx.x);
}

// Both adjoints of gather_add read the same d_msg: workgroups [0, nseg) sum by one CSR, [nseg, 2 nseg) by the other -- one
// launch on the dependency chain instead of two, every segment summed as segment_sum_kernel sums it.
__global__ __launch_bounds__(128) void segment_sum_pair_kernel(const float* __restrict__ x, const int* __restrict__ ptr_a,
                                                               const int* __restrict__ perm_a, float* __restrict__ out_a,
                                                               const int* __restrict__ ptr_b,
                                                               const int* __restrict__ perm_b, float* __restrict__ out_b,
                                                               int nseg, int D) {
  const int b = (int)blockIdx.x;
  if (b < nseg) segment_sum_block(x, ptr_a, perm_a, out_a, D, 1.f, 0, b);
  else segment_sum_block(x, ptr_b, perm_b, out_b, D, 1.f, 0, b - nseg);
}

__global__ __launch_bounds__(256) void segment_bcast_kernel(const float* __restrict__ x, const int* __restrict__ seg_of,
                                                            float* __restrict__ out, long total, int D, float scale) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const long row = idx / D;
  const int c = (int)(idx - row * D);
  out[idx] = scale * x[(long)seg_of[row] * D + c];
}

// out[q,c] = s[seg_of[q]] * x[q,c]: per-graph stochastic depth (GraphDropPath).  Linear in x, so the same kernel is its
// own backward (on dy) and second-order term.
__global__ __launch_bounds__(256) void segment_scale_kernel(const float* __restrict__ x, const float* __restrict__ s,
                                                            const int* __restrict__ seg_of, float* __restrict__ out,
                                                            long total4, int D4) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total4) return;
  const long row = idx / D4;
  const float f = s[seg_of[row]];
  float4 v = reinterpret_cast<const float4*>(x)[idx];
  v.x *= f; v.y *= f; v.z *= f; v.w *= f;
  reinterpret_cast<float4*>(out)[idx] = v;
}

// out[q,c] = f(seg_of[q]) * x[q,c] with the factor of segment_scale_kernel DRAWN here: f = inv_keep where the uniform of
// (seed0 + *seed_word, tag 32, (call << 32) | graph) (rng.h) is >= drop_p, else 0 -- a pure function of its arguments, so
// a captured launch whose host advances the word between replays drops other graphs every replay, and its backward
// (the same launch on dy) redraws the mask of its forward.  One wavefront owns whole rows: the row index is wave-uniform
// (readfirstlane), so the index load, the two 64-bit hashes and the compare happen once per row on the scalar unit, not
// once per float4; the lanes stride the row's float4 columns (coalesced 1 KiB per step).  A multiply, not a select: a NaN
// in a dropped row stays NaN, the bits are those of segment_scale_kernel fed the same factor.
constexpr unsigned long long DROPPATH_TAG = 32;  // (dens.hip: 0-2, is2rs.hip: 16-18)
constexpr int DROPPATH_WAVES = 4;

__global__ __launch_bounds__(64 * DROPPATH_WAVES) void segment_droppath_kernel(
    const float* __restrict__ x, const int* __restrict__ seg_of, float* __restrict__ out, int rows, int D4, float drop_p,
    float inv_keep, unsigned long long seed0, const unsigned long long* __restrict__ seed_word, unsigned long long call) {
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int lane = (int)(threadIdx.x & 63);
  const unsigned long long seed = seed0 + (seed_word ? *seed_word : 0ull);
  const long stride = (long)gridDim.x * DROPPATH_WAVES;
  for (long row = (long)blockIdx.x * DROPPATH_WAVES + wave; row < rows; row += stride) {
    const unsigned long long graph = (unsigned int)seg_of[row];
    const float u = eqf_rand_uniform(seed, DROPPATH_TAG, (call << 32) | graph);
    const float f = u >= drop_p ? inv_keep : 0.f;
    const float4* xr = reinterpret_cast<const float4*>(x) + row * D4;
    float4* orow = reinterpret_cast<float4*>(out) + row * D4;
    for (int c = lane; c < D4; c += 64) {
      float4 v = xr[c];
      v.x *= f; v.y *= f; v.z *= f; v.w *= f;
      orow[c] = v;
    }
  }
}

// ---------------------------------------------------------------------------------------------- DTP coupling
__global__ __launch_bounds__(256) void coupling_fwd_kernel(const float* __restrict__ sh, const float* __restrict__ cg,
                                                           const eqf_dtp_paths P, float* __restrict__ M, long total) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const long e = idx / P.npaths;
  const int p = (int)(idx - e * P.npaths);
  const int d1 = 2 * P.l1[p] + 1, d2 = 2 * P.l2[p] + 1, d3 = 2 * path_l3(P, p) + 1;
  const float* y = sh + e * P.sh_dim + P.l2[p] * P.l2[p];
  const float* c = cg + P.cg_off[p];
  float* m = M + e * P.m_numel + P.m_off[p];
  for (int i = 0; i < d1; ++i)
    for (int k = 0; k < d3; ++k) {
      float acc = 0.f;
      for (int j = 0; j < d2; ++j) acc = fmaf(c[(i * d2 + j) * d3 + k], y[j], acc);
      m[i * d3 + k] = acc;
    }
}

__global__ __launch_bounds__(256) void coupling_bwd_kernel(const float* __restrict__ dM, const float* __restrict__ cg,
                                                           const eqf_dtp_paths P, float* __restrict__ d_sh, long total) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const long e = idx / P.sh_dim;
  const int s = (int)(idx - e * P.sh_dim);
  int l2 = 0;
  while ((l2 + 1) * (l2 + 1) <= s) ++l2;
  const int j = s - l2 * l2;
  float acc = 0.f;
  for (int p = 0; p < P.npaths; ++p) {
    if (P.l2[p] != l2) continue;
    const int d1 = 2 * P.l1[p] + 1, d2 = 2 * l2 + 1, d3 = 2 * path_l3(P, p) + 1;
    const float* c = cg + P.cg_off[p];
    const float* g = dM + e * P.m_numel + P.m_off[p];
    for (int i = 0; i < d1; ++i)
      for (int k = 0; k < d3; ++k) acc = fmaf(c[(i * d2 + j) * d3 + k], g[i * d3 + k], acc);
  }
  d_sh[idx] = acc;
}

// ---------------------------------------------------------------------------------------------- DTP (un-fused)
__global__ __launch_bounds__(256) void dtp_fwd_kernel(const float* __restrict__ x, const float* __restrict__ M,
                                                      const float* __restrict__ w, const eqf_dtp_paths P,
                                                      float* __restrict__ out) {
  const long e = blockIdx.x;
  const int item = blockIdx.y * blockDim.x + threadIdx.x;  // (path, channel) == index into the weight row
  if (item >= P.w_numel) return;
  int p = 0;
  while (p + 1 < P.npaths && item >= P.w_off[p + 1]) ++p;
  const int u = item - P.w_off[p];
  const int d1 = 2 * P.l1[p] + 1, d3 = 2 * path_l3(P, p) + 1;
  const float wv = w ? w[e * P.w_numel + item] : 1.f;
  const float* xp = x + e * P.in_dim + P.in_off[p] + u;
  const float* mp = M + e * P.m_numel + P.m_off[p];
  float* op = out + e * P.out_dim + P.out_off[p] + P.out_ch[p] + u;
  float xv[7];
#pragma unroll
  for (int i = 0; i < 7; ++i) xv[i] = (i < d1) ? xp[i * P.mul[p]] : 0.f;
  for (int k = 0; k < d3; ++k) {
    float acc = 0.f;
#pragma unroll
    for (int i = 0; i < 7; ++i)
      if (i < d1) acc = fmaf(mp[i * d3 + k], xv[i], acc);
    op[k * P.out_k[p]] = acc * wv;
  }
}

struct InSegs {
  int nseg;
  int off[EQF_MAX_SEG], mul[EQF_MAX_SEG], cum[EQF_MAX_SEG + 1];
};

// one thread per (edge, input channel): owns dx[e, seg, :, u]; loops over the paths fed by that segment
__global__ __launch_bounds__(256) void dtp_bwd_kernel(const float* __restrict__ x, const float* __restrict__ M,
                                                      const float* __restrict__ w, const eqf_dtp_paths P,
                                                      const InSegs S, const float* __restrict__ d_out,
                                                      float* __restrict__ dx, float* __restrict__ dw,
                                                      float* __restrict__ dM) {
  extern __shared__ float dM_s[];  // m_numel floats when dM != null
  const long e = blockIdx.x;
  if (dM) {
    for (int i = threadIdx.x; i < P.m_numel; i += blockDim.x) dM_s[i] = 0.f;
    __syncthreads();
  }
  for (int ch = threadIdx.x; ch < S.cum[S.nseg]; ch += blockDim.x) {
    int s = 0;
    while (s + 1 < S.nseg && ch >= S.cum[s + 1]) ++s;
    const int u = ch - S.cum[s];
    const int in_off = S.off[s], mul = S.mul[s];
    float xv[7], gx[7];
    int d1 = 1;
    for (int p = 0; p < P.npaths; ++p)
      if (P.in_off[p] == in_off) d1 = 2 * P.l1[p] + 1;
#pragma unroll
    for (int i = 0; i < 7; ++i) {
      xv[i] = (i < d1) ? x[e * P.in_dim + in_off + i * mul + u] : 0.f;
      gx[i] = 0.f;
    }
    for (int p = 0; p < P.npaths; ++p) {
      if (P.in_off[p] != in_off) continue;
      const int d3 = 2 * path_l3(P, p) + 1;
      const float wv = w ? w[e * P.w_numel + P.w_off[p] + u] : 1.f;
      const float* mp = M + e * P.m_numel + P.m_off[p];
      const float* gp = d_out + e * P.out_dim + P.out_off[p] + P.out_ch[p] + u;
      float gw = 0.f;
      for (int k = 0; k < d3; ++k) {
        const float g = gp[k * P.out_k[p]];
        float t = 0.f;
#pragma unroll
        for (int i = 0; i < 7; ++i)
          if (i < d1) {
            const float m = mp[i * d3 + k];
            t = fmaf(m, xv[i], t);
            gx[i] = fmaf(m * wv, g, gx[i]);
            if (dM) atomicAdd(&dM_s[P.m_off[p] + i * d3 + k], wv * xv[i] * g);
          }
        gw = fmaf(g, t, gw);
      }
      if (dw) dw[e * P.w_numel + P.w_off[p] + u] = gw;
    }
#pragma unroll
    for (int i = 0; i < 7; ++i)
      if (i < d1) dx[e * P.in_dim + in_off + i * mul + u] = gx[i];
  }
  if (dM) {
    __syncthreads();
    for (int i = threadIdx.x; i < P.m_numel; i += blockDim.x) dM[e * P.m_numel + i] = dM_s[i];
  }
}

// ---------------------------------------------------------------------------------------------- attention logits
__device__ __forceinline__ float slrelu(float x) { return 0.6f * x + 0.4f * x * (2.f * sigmoidf_(x) - 1.f); }
__device__ __forceinline__ float dslrelu(float x) {
  const float s = sigmoidf_(x);
  return 0.6f + 0.4f * (2.f * s - 1.f) + 0.8f * x * s * (1.f - s);
}

// Kh in {8,16,32,64}: Kh consecutive lanes share (edge, head).  A thread takes ALPHA_U elements 256 apart, all requested before
// the first is used; the 64-bit division idx / HK is done once per workgroup (on its first index, wave-uniform), a lane divides
// only its small offset from there.  Every (edge, head) is still summed by the same Kh lanes with the same butterfly.
constexpr int ALPHA_U = 4;

__global__ __launch_bounds__(256) void alpha_fwd_kernel(const float* __restrict__ a, const float* __restrict__ adot,
                                                        float* __restrict__ logit, long total, int HK, int Kh, float c) {
  const long base = (long)blockIdx.x * (256 * ALPHA_U);
  const long eb = base / HK;
  const unsigned r0 = (unsigned)(base - eb * HK) + threadIdx.x;  // < HK + 256
  const int sh = __builtin_ctz((unsigned)Kh);
  float av[ALPHA_U], dv[ALPHA_U];
  long e[ALPHA_U];
  int col[ALPHA_U];
#pragma unroll
  for (int u = 0; u < ALPHA_U; ++u) {
    const long idx = base + u * 256 + threadIdx.x;
    const unsigned r = r0 + u * 256, q = r / (unsigned)HK;
    e[u] = eb + q;
    col[u] = (int)(r - q * (unsigned)HK);
    av[u] = idx < total ? a[idx] : 0.f;
    dv[u] = idx < total ? adot[col[u]] : 0.f;
  }
#pragma unroll
  for (int u = 0; u < ALPHA_U; ++u) {
    const long idx = base + u * 256 + threadIdx.x;
    float v = idx < total ? c * slrelu(av[u]) * dv[u] : 0.f;
    for (int o = Kh >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if (idx < total && (col[u] & (Kh - 1)) == 0) logit[e[u] * (HK >> sh) + (col[u] >> sh)] = v;  // Kh is a power of two
  }
}

__global__ __launch_bounds__(256) void alpha_bwd_kernel(const float* __restrict__ a, const float* __restrict__ adot,
                                                        const float* __restrict__ d_logit, float* __restrict__ da,
                                                        float* __restrict__ d_adot, int E, int HK, int Kh, float c,
                                                        int CH) {
  const int col = blockIdx.x * blockDim.x + threadIdx.x;
  if (col >= HK) return;
  const int h = col / Kh, H = HK / Kh;
  const int e0 = blockIdx.y * CH, e1 = min(E, e0 + CH);
  const float ad = adot[col];
  // d_alpha_dot[col] is a sum of signed terms over all edges that often nearly cancels: the CH products of a thread are formed
  // and added in fp64 (16 adds per thread) and rounded once, so what the column loses is the rounding of its terms and of the
  // E / CH atomics, not a serial fp32 chain
  double acc = 0.0;
  for (int e = e0; e < e1; ++e) {
    const float g = d_logit[(long)e * H + h] * c;
    const float av = a[(long)e * HK + col];
    da[(long)e * HK + col] = g * ad * dslrelu(av);
    acc += (double)g * (double)slrelu(av);
  }
  atomicAdd(d_adot + col, (float)acc);
}

// float4 columns, RP = 256 / (HK / 4) edge rows per pass, ALPHA_BWD_U = 4 passes (their a rows and d_logit words) requested
// before the first is used; a workgroup walks its CH = 64 edges in CH / (4 RP) such steps and ends with one atomic per column:
// 17.4 us per launch at E = 25 354, HK = 256 (26 MB in, 26 MB out; 397 workgroups, four dependent steps each).  Measured and not
// kept: all 16 passes of a workgroup in flight (133 VGPRs) took 19.3 us -- the chain is not what bounds this kernel.  Fewer
// edges per workgroup would multiply the same-address atomics on d_adot, which is what CH = 64 keeps down.
// HK % 4 == 0, HK / 4 <= 256, Kh % 4 == 0; every other shape takes alpha_bwd_kernel above.
constexpr int ALPHA_BWD_U = 4;  // passes in flight

__global__ __launch_bounds__(256) void alpha_bwd4_kernel(const float* __restrict__ a, const float* __restrict__ adot,
                                                         const float* __restrict__ d_logit, float* __restrict__ da,
                                                         float* __restrict__ d_adot, int E, int HK, int Kh, float c,
                                                         int CH) {
  const int Q = HK >> 2;               // float4 columns per row
  const int RP = 256 / Q;              // rows per pass
  const int tx = threadIdx.x % Q, ty = threadIdx.x / Q;
  const int H = HK / Kh, h = (4 * tx) / Kh;
  const int e0 = blockIdx.x * CH, e1 = min(E, e0 + CH);
  __shared__ float red[4 * 256];
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  if (ty < RP) {
    const float4 ad = reinterpret_cast<const float4*>(adot)[tx];
    for (int eb = e0 + ty; eb < e1; eb += ALPHA_BWD_U * RP) {
      float4 av[ALPHA_BWD_U];
      float g[ALPHA_BWD_U];
#pragma unroll
      for (int u = 0; u < ALPHA_BWD_U; ++u) {
        const int e = eb + u * RP;
        const bool ok = e < e1;
        av[u] = ok ? reinterpret_cast<const float4*>(a)[(long)e * Q + tx] : make_float4(0.f, 0.f, 0.f, 0.f);
        g[u] = ok ? d_logit[(long)e * H + h] * c : 0.f;
      }
#pragma unroll
      for (int u = 0; u < ALPHA_BWD_U; ++u) {
        const int e = eb + u * RP;
        if (e < e1) {
          float4 o;
          o.x = g[u] * ad.x * dslrelu(av[u].x), o.y = g[u] * ad.y * dslrelu(av[u].y);
          o.z = g[u] * ad.z * dslrelu(av[u].z), o.w = g[u] * ad.w * dslrelu(av[u].w);
          reinterpret_cast<float4*>(da)[(long)e * Q + tx] = o;
          acc.x += g[u] * slrelu(av[u].x), acc.y += g[u] * slrelu(av[u].y);
          acc.z += g[u] * slrelu(av[u].z), acc.w += g[u] * slrelu(av[u].w);
        }
      }
    }
  }
  float* my = red + 4 * threadIdx.x;
  my[0] = acc.x, my[1] = acc.y, my[2] = acc.z, my[3] = acc.w;
  __syncthreads();
  if ((int)threadIdx.x < HK) {
    const int col = threadIdx.x, q = col >> 2, k = col & 3;
    float sum = 0.f;
    for (int r = 0; r < RP; ++r) sum += red[4 * (r * Q + q) + k];
    atomicAdd(d_adot + col, sum);
  }
}

// ---------------------------------------------------------------------------------------------- softmax + aggregate
struct HeadTab {
  int nseg, H, D, G;  // G = float4 groups per head
  int off[EQF_MAX_SEG], mul[EQF_MAX_SEG], d[EQF_MAX_SEG], gcum[EQF_MAX_SEG + 1];
};

__device__ __forceinline__ int head_col(const HeadTab& T, int h, int g) {
  int s = 0;
  while (s + 1 < T.nseg && g >= T.gcum[s + 1]) ++s;
  const int mh = T.mul[s] / T.H;  // channels of this head in segment s
  const int q4 = mh >> 2;
  const int j = g - T.gcum[s];
  const int m = j / q4, q = j - m * q4;
  return T.off[s] + m * T.mul[s] + h * mh + 4 * q;
}

__device__ __forceinline__ float keep_scale(unsigned long long seed, unsigned long long idx, float p) {
  if (p <= 0.f) return 1.f;
  unsigned long long z = seed + 0x9E3779B97F4A7C15ull * (idx + 1);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z = z ^ (z >> 31);
  const float u = (float)(z >> 40) * (1.0f / 16777216.0f);
  return (u >= p) ? 1.f / (1.f - p) : 0.f;
}

// v of lane `src` (a constant) as a wave-uniform value: v_readlane, no trip through the LDS crossbar
__device__ __forceinline__ float lane_value(float v, int src) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), src));
}

constexpr int MAX_SLOTS = 4;  // up to 256 float4 groups (1024 channels) per head

__global__ void attn_fwd_kernel(const float* __restrict__ logit, const float* __restrict__ value,
                                const int* __restrict__ row_ptr, float* __restrict__ alpha, float* __restrict__ out,
                                const HeadTab T, float drop_p, unsigned long long seed0,
    const unsigned long long* __restrict__ seed_off) {
  // (the mask seed of a launch captured in a HIP graph: host part + a device word the caller advances between replays)
  const unsigned long long seed = seed0 + (seed_off ? *seed_off : 0ull);
  const int n = blockIdx.x;
  const int h = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int beg = row_ptr[n], end = row_ptr[n + 1];
  const int H = T.H, D4 = T.D >> 2;
  int col4[MAX_SLOTS];
  float4 acc[MAX_SLOTS];
#pragma unroll
  for (int s = 0; s < MAX_SLOTS; ++s) {
    const int g = lane + 64 * s;
    col4[s] = (g < T.G) ? head_col(T, h, g) >> 2 : -1;
    acc[s] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  float mx = -INFINITY;
  for (int e = beg + lane; e < end; e += 64) mx = fmaxf(mx, logit[(long)e * H + h]);
  mx = wave_max(mx);
  float sm = 0.f;
  for (int e = beg + lane; e < end; e += 64) sm += __expf(logit[(long)e * H + h] - mx);
  sm = wave_sum(sm);
  const float inv = 1.f / (sm + 1e-16f);
  for (int e = beg; e < end; ++e) {
    const float a = __expf(logit[(long)e * H + h] - mx) * inv;
    if (lane == 0) alpha[(long)e * H + h] = a;
    const float ak = a * keep_scale(seed, (unsigned long long)e * H + h, drop_p);
#pragma unroll
    for (int s = 0; s < MAX_SLOTS; ++s)
      if (col4[s] >= 0) {
        const float4 v = reinterpret_cast<const float4*>(value)[(long)e * D4 + col4[s]];
        acc[s].x = fmaf(ak, v.x, acc[s].x), acc[s].y = fmaf(ak, v.y, acc[s].y);
        acc[s].z = fmaf(ak, v.z, acc[s].z), acc[s].w = fmaf(ak, v.w, acc[s].w);
      }
  }
#pragma unroll
  for (int s = 0; s < MAX_SLOTS; ++s)
    if (col4[s] >= 0) reinterpret_cast<float4*>(out)[(long)n * D4 + col4[s]] = acc[s];
}

// Heads of <= 32 float4 groups (QM9 / MD17: 30): a wave covers TWO edges per step (lanes 0-31 edge e, lanes 32-63 edge
// e+1) and two such steps are issued before the first FMA -- four independent 16-byte value loads per lane in flight
// instead of one with 30 of 64 lanes working; the halves are folded with one shuffle at the end.
__global__ void attn_fwd_half_kernel(const float* __restrict__ logit, const float* __restrict__ value,
                                     const int* __restrict__ row_ptr, float* __restrict__ alpha,
                                     float* __restrict__ out, const HeadTab T, float drop_p, unsigned long long seed0,
    const unsigned long long* __restrict__ seed_off) {
  // (the mask seed of a launch captured in a HIP graph: host part + a device word the caller advances between replays)
  const unsigned long long seed = seed0 + (seed_off ? *seed_off : 0ull);
  const int n = blockIdx.x;
  const int h = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int half = lane >> 5, gl = lane & 31;
  const int beg = row_ptr[n], end = row_ptr[n + 1];
  const int H = T.H, D4 = T.D >> 2;
  const int deg = end - beg;
  const int col4 = (gl < T.G) ? head_col(T, h, gl) >> 2 : -1;
  const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
  const float4* const V = reinterpret_cast<const float4*>(value);
  // A row is ~11 edges: the kernel is a chain of dependent memory round trips, not a stream.  Two of the three are
  // taken out of the chain: (1) the value rows of the first four edges depend on row_ptr only and are requested BEFORE
  // the softmax statistics; inside the loop the next four are requested before the current ones are used; (2) the
  // head's logits are read ONCE, lane j holding edge beg + j, and handed to the edge loop by lane shuffles (rows longer
  // than 64 edges re-read memory for the rest).
  float4 xa = (beg + half < end && col4 >= 0) ? V[(long)(beg + half) * D4 + col4] : z4;
  float4 xb = (beg + 2 + half < end && col4 >= 0) ? V[(long)(beg + 2 + half) * D4 + col4] : z4;
  const float lg = lane < deg ? logit[(long)(beg + lane) * H + h] : -INFINITY;
  float mx = lg;
  for (int e = beg + 64 + lane; e < end; e += 64) mx = fmaxf(mx, logit[(long)e * H + h]);
  mx = wave_max(mx);
  float sm = lane < deg ? __expf(lg - mx) : 0.f;
  for (int e = beg + 64 + lane; e < end; e += 64) sm += __expf(logit[(long)e * H + h] - mx);
  sm = wave_sum(sm);
  const float inv = 1.f / (sm + 1e-16f);
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int e0 = beg; e0 < end; e0 += 4) {
    const int ea = e0 + half, eb = e0 + 2 + half;
    const bool va = ea < end, vb = eb < end;
    const float4 xan = (ea + 4 < end && col4 >= 0) ? V[(long)(ea + 4) * D4 + col4] : z4;
    const float4 xbn = (eb + 4 < end && col4 >= 0) ? V[(long)(eb + 4) * D4 + col4] : z4;
    const int ia = ea - beg, ib = eb - beg;
    float la = __shfl(lg, ia & 63), lb = __shfl(lg, ib & 63);
    if (ia >= 64 && va) la = logit[(long)ea * H + h];
    if (ib >= 64 && vb) lb = logit[(long)eb * H + h];
    const float aa = va ? __expf(la - mx) * inv : 0.f, ab = vb ? __expf(lb - mx) * inv : 0.f;
    if (gl == 0) {
      if (va) alpha[(long)ea * H + h] = aa;
      if (vb) alpha[(long)eb * H + h] = ab;
    }
    const float ka = aa * keep_scale(seed, (unsigned long long)ea * H + h, drop_p);
    const float kb = ab * keep_scale(seed, (unsigned long long)eb * H + h, drop_p);
    acc.x = fmaf(ka, xa.x, acc.x), acc.y = fmaf(ka, xa.y, acc.y), acc.z = fmaf(ka, xa.z, acc.z), acc.w = fmaf(ka, xa.w, acc.w);
    acc.x = fmaf(kb, xb.x, acc.x), acc.y = fmaf(kb, xb.y, acc.y), acc.z = fmaf(kb, xb.z, acc.z), acc.w = fmaf(kb, xb.w, acc.w);
    xa = xan, xb = xbn;
  }
  acc.x += __shfl_xor(acc.x, 32), acc.y += __shfl_xor(acc.y, 32);
  acc.z += __shfl_xor(acc.z, 32), acc.w += __shfl_xor(acc.w, 32);
  if (half == 0 && col4 >= 0) reinterpret_cast<float4*>(out)[(long)n * D4 + col4] = acc;
}

// The backward of attn_fwd_half_kernel, with the same two cuts in its chain of memory round trips: (1) the value rows of the
// first four edges, the row's d_out and the head's alpha (lane j holding edge beg + j) depend on row_ptr only and are requested
// together; inside the loop the next four value rows are requested before the current ones are used, and alpha reaches the
// edge loop by lane shuffles; (2) d(alpha) of the row's first 64 edges stays in registers -- after the half-wave butterfly
// lanes 0 and 32 hold the figures of the step's four edges, and lane j keeps the one of edge beg + j -- so the softmax
// fix-up at the end needs no stash in d_logit, no fence and no re-read.  Only edges from the 65th on take the memory stash.
// Same terms, same order, same butterflies as before: the results are bit-identical.
__global__ void attn_bwd_half_kernel(const float* __restrict__ alpha, const float* __restrict__ value,
                                     const int* __restrict__ row_ptr, const float* __restrict__ d_out,
                                     float* __restrict__ d_value, float* __restrict__ d_logit, const HeadTab T,
                                     float drop_p, unsigned long long seed0,
    const unsigned long long* __restrict__ seed_off) {
  // (the mask seed of a launch captured in a HIP graph: host part + a device word the caller advances between replays)
  const unsigned long long seed = seed0 + (seed_off ? *seed_off : 0ull);
  const int n = blockIdx.x;
  const int h = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int half = lane >> 5, gl = lane & 31;
  const int beg = row_ptr[n], end = row_ptr[n + 1];
  const int H = T.H, D4 = T.D >> 2;
  const int deg = end - beg;
  const int col4 = (gl < T.G) ? head_col(T, h, gl) >> 2 : -1;
  const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
  const float4* const V = reinterpret_cast<const float4*>(value);
  float4 xa = (beg + half < end && col4 >= 0) ? V[(long)(beg + half) * D4 + col4] : z4;
  float4 xb = (beg + 2 + half < end && col4 >= 0) ? V[(long)(beg + 2 + half) * D4 + col4] : z4;
  const float al = lane < deg ? alpha[(long)(beg + lane) * H + h] : 0.f;
  const float4 go = (col4 >= 0) ? reinterpret_cast<const float4*>(d_out)[(long)n * D4 + col4] : z4;
  float s_acc = 0.f;
  float da_mine = 0.f;  // d(alpha) of edge beg + lane
  for (int e0 = beg; e0 < end; e0 += 4) {
    const int ea = e0 + half, eb = e0 + 2 + half;
    const bool va = ea < end, vb = eb < end;
    const float4 xan = (ea + 4 < end && col4 >= 0) ? V[(long)(ea + 4) * D4 + col4] : z4;
    const float4 xbn = (eb + 4 < end && col4 >= 0) ? V[(long)(eb + 4) * D4 + col4] : z4;
    const int base = e0 - beg;  // wave-uniform, a multiple of 4
    float aa = __shfl(al, (base + half) & 63), ab = __shfl(al, (base + 2 + half) & 63);
    if (base >= 64) {
      aa = va ? alpha[(long)ea * H + h] : 0.f;
      ab = vb ? alpha[(long)eb * H + h] : 0.f;
    }
    if (!va) aa = 0.f;
    if (!vb) ab = 0.f;
    const float keepa = keep_scale(seed, (unsigned long long)ea * H + h, drop_p);
    const float keepb = keep_scale(seed, (unsigned long long)eb * H + h, drop_p);
    float pa = xa.x * go.x + xa.y * go.y + xa.z * go.z + xa.w * go.w;
    float pb = xb.x * go.x + xb.y * go.y + xb.z * go.z + xb.w * go.w;
    if (va && col4 >= 0) {
      const float k = aa * keepa;
      reinterpret_cast<float4*>(d_value)[(long)ea * D4 + col4] = make_float4(k * go.x, k * go.y, k * go.z, k * go.w);
    }
    if (vb && col4 >= 0) {
      const float k = ab * keepb;
      reinterpret_cast<float4*>(d_value)[(long)eb * D4 + col4] = make_float4(k * go.x, k * go.y, k * go.z, k * go.w);
    }
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) pa += __shfl_xor(pa, o), pb += __shfl_xor(pb, o);  // sums inside each half
    const float da = pa * keepa, db = pb * keepb;
    float contrib = aa * da + ab * db;           // this half's two edges
    contrib += __shfl_xor(contrib, 32);          // + the other half's
    s_acc += contrib;
    if (base < 64) {
      // edges base .. base + 3 are (da, half 0), (da, half 1), (db, half 0), (db, half 1): lanes base .. base + 3 keep them
      const float d0 = lane_value(da, 0), d1 = lane_value(da, 32), d2 = lane_value(db, 0), d3 = lane_value(db, 32);
      if ((lane >> 2) == (base >> 2)) da_mine = (lane & 2) ? ((lane & 1) ? d3 : d2) : ((lane & 1) ? d1 : d0);
    } else if (gl == 0) {  // rows longer than a wavefront: stash d(alpha) of the further edges; fixed up below
      if (va) d_logit[(long)ea * H + h] = da;
      if (vb) d_logit[(long)eb * H + h] = db;
    }
    xa = xan, xb = xbn;
  }
  if (lane < deg) d_logit[(long)(beg + lane) * H + h] = al * (da_mine - s_acc);
  if (deg > 64) {
    // the stash above was written by lanes 0 / 32 of THIS wave and is re-read below by its other lanes: same wave, same CU,
    // so both accesses go through this CU's write-through L1; the workgroup fence (s_waitcnt vmcnt(0)) retires the stores
    // before the loads are issued.  No other wave touches these addresses.
    __threadfence_block();
    for (int e = beg + 64 + lane; e < end; e += 64) {
      const float da = d_logit[(long)e * H + h];
      d_logit[(long)e * H + h] = alpha[(long)e * H + h] * (da - s_acc);
    }
  }
}

__global__ void attn_bwd_kernel(const float* __restrict__ alpha, const float* __restrict__ value,
                                const int* __restrict__ row_ptr, const float* __restrict__ d_out,
                                float* __restrict__ d_value, float* __restrict__ d_logit, const HeadTab T, float drop_p,
                                unsigned long long seed0,
    const unsigned long long* __restrict__ seed_off) {
  // (the mask seed of a launch captured in a HIP graph: host part + a device word the caller advances between replays)
  const unsigned long long seed = seed0 + (seed_off ? *seed_off : 0ull);
  const int n = blockIdx.x;
  const int h = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int beg = row_ptr[n], end = row_ptr[n + 1];
  const int H = T.H, D4 = T.D >> 2;
  int col4[MAX_SLOTS];
  float4 go[MAX_SLOTS];
#pragma unroll
  for (int s = 0; s < MAX_SLOTS; ++s) {
    const int g = lane + 64 * s;
    col4[s] = (g < T.G) ? head_col(T, h, g) >> 2 : -1;
    go[s] = (col4[s] >= 0) ? reinterpret_cast<const float4*>(d_out)[(long)n * D4 + col4[s]]
                           : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  float s_acc = 0.f;
  for (int e = beg; e < end; ++e) {
    const float a = alpha[(long)e * H + h];
    const float keep = keep_scale(seed, (unsigned long long)e * H + h, drop_p);
    const float ak = a * keep;
    float part = 0.f;
#pragma unroll
    for (int s = 0; s < MAX_SLOTS; ++s)
      if (col4[s] >= 0) {
        const float4 v = reinterpret_cast<const float4*>(value)[(long)e * D4 + col4[s]];
        part += v.x * go[s].x + v.y * go[s].y + v.z * go[s].z + v.w * go[s].w;
        float4 dv;
        dv.x = ak * go[s].x, dv.y = ak * go[s].y, dv.z = ak * go[s].z, dv.w = ak * go[s].w;
        reinterpret_cast<float4*>(d_value)[(long)e * D4 + col4[s]] = dv;
      }
    const float da = wave_sum(part) * keep;
    s_acc = fmaf(a, da, s_acc);
    if (lane == 0) d_logit[(long)e * H + h] = da;  // stash d(alpha); fixed up below
  }
  __threadfence_block();
  for (int e = beg + lane; e < end; e += 64) {
    const float da = d_logit[(long)e * H + h];
    d_logit[(long)e * H + h] = alpha[(long)e * H + h] * (da - s_acc);
  }
}

HeadTab make_headtab(const eqf_irreps& ir, int H, int* err) {
  HeadTab T{};
  *err = 0;
  T.nseg = ir.nseg;
  T.H = H;
  int off = 0, g = 0;
  for (int s = 0; s < ir.nseg; ++s) {
    T.off[s] = off;
    T.mul[s] = ir.mul[s];
    T.d[s] = 2 * ir.l[s] + 1;
    T.gcum[s] = g;
    if (ir.mul[s] % (4 * H) != 0) *err = EQF_E_UNSUPPORTED;
    g += T.d[s] * (ir.mul[s] / H) / 4;
    off += ir.mul[s] * T.d[s];
  }
  T.gcum[ir.nseg] = g;
  T.G = g;
  T.D = off;
  if (g > 64 * MAX_SLOTS || H > 16) *err = EQF_E_UNSUPPORTED;
  return T;
}

}  // namespace

extern "C" {

int eqf_gather_add_fwd(const float* a, const float* b, const int* src, const int* dst, float* msg, int E, int D,
                       void* stream) {
  if (!a || !src || !msg || (b && !dst)) return EQF_E_BADARG;
  if (D % 4 != 0) return EQF_E_UNSUPPORTED;
  if (E <= 0) return 0;
  const long total4 = (long)E * (D / 4);
  if (D / 4 >= GATHER_ROW_MIN_D4)  // a wave's 64 lanes would idle over narrower rows: those keep one float4 per thread
    hipLaunchKernelGGL(gather_add_rows_kernel, dim3(eqf_cdiv(E, GATHER_WAVES * GATHER_ROWS)), dim3(64 * GATHER_WAVES), 0,
                       (hipStream_t)stream, a, b, src, dst, msg, E, D / 4);
  else
    hipLaunchKernelGGL(gather_add_kernel, dim3(eqf_cdiv(total4, 256)), dim3(256), 0, (hipStream_t)stream, a, b, src, dst,
                       msg, total4, D / 4);
  EQF_CHECK_LAUNCH();
  return 0;
}

int eqf_segment_sum(const float* x, const int* ptr, const int* perm, float* out, int nseg, int D, float scale,
                    int accumulate, void* stream) {
  if (!x || !ptr || !out) return EQF_E_BADARG;
  if (nseg <= 0 || D <= 0) return 0;
  hipLaunchKernelGGL(segment_sum_kernel, dim3(nseg), dim3(128), 0, (hipStream_t)stream, x, ptr, perm, out, D, scale,
                     accumulate);
  EQF_CHECK_LAUNCH();
  return 0;
}

int eqf_segment_sum_pair(const float* x, const int* ptr_a, const int* perm_a, float* out_a, const int* ptr_b,
                         const int* perm_b, float* out_b, int nseg, int D, void* stream) {
  if (!x || !ptr_a || !out_a || !ptr_b || !out_b || out_a == out_b) return EQF_E_BADARG;
  if (nseg <= 0 || D <= 0) return 0;
  hipLaunchKernelGGL(segment_sum_pair_kernel, dim3(2 * nseg), dim3(128), 0, (hipStream_t)stream, x, ptr_a, perm_a, out_a,
                     ptr_b, perm_b, out_b, nseg, D);
  EQF_CHECK_LAUNCH();
  return 0;
}

int eqf_segment_scale(const float* x, const float* s, const int* seg_of, float* out, int rows, int D, void* stream) {
  if (!x || !s || !seg_of || !out) return EQF_E_BADARG;
  if (D % 4) return EQF_E_UNSUPPORTED;
  if (rows <= 0 || D <= 0) return 0;
  const long total4 = (long)rows * (D / 4);
  hipLaunchKernelGGL(segment_scale_kernel, dim3(eqf_cdiv(total4, 256)), dim3(256), 0, (hipStream_t)stream, x, s, seg_of,
                     out, total4, D / 4);
  EQF_CHECK_LAUNCH();
  return 0;
}

int eqf_segment_droppath(const float* x, const int* seg_of, float* out, int rows, int D, float drop_p, float inv_keep,
                         unsigned long long seed, const unsigned long long* seed_word, unsigned long long call,
                         void* stream) {
  if (!x || !seg_of || !out) return EQF_E_BADARG;
  if (D % 4) return EQF_E_UNSUPPORTED;
  if (rows <= 0 || D <= 0) return 0;
  // one row per wavefront up to 2 048 workgroups (8 per CU), the rows beyond that by the kernel's grid stride
  const long blocks = eqf_cdiv((long)rows, (long)DROPPATH_WAVES);
  hipLaunchKernelGGL(segment_droppath_kernel, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(64 * DROPPATH_WAVES), 0,
                     (hipStream_t)stream, x, seg_of, out, rows, D / 4, drop_p, inv_keep, seed, seed_word, call);
  EQF_CHECK_LAUNCH();
  return 0;
}

int eqf_segment_bcast(const float* x, const int* seg_of, float* out, int rows, int D, float scale, void* stream) {
  if (!x || !seg_of || !out) return EQF_E_BADARG;
  if (rows <= 0 || D <= 0) return 0;
  const long total = (long)rows * D;
  hipLaunchKernelGGL(segment_bcast_kernel, dim3(eqf_cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, x, seg_of,
                     out, total, D, scale);
  EQF_CHECK_LAUNCH();
  return 0;
}

int eqf_dtp_coupling_fwd(const float* sh, const float* cg, const eqf_dtp_paths* paths, float* coupling, int E,
                         void* stream) {
  if (!sh || !cg || !paths || !coupling || paths->npaths < 1 || paths->npaths > EQF_MAX_PATHS) return EQF_E_BADARG;
  if (E <= 0) return 0;
  const long total = (long)E * paths->npaths;
  hipLaunchKernelGGL(coupling_fwd_kernel, dim3(eqf_cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, sh, cg, *paths,
                     coupling, total);
  EQF_CHECK_LAUNCH();
  return 0;
}

int eqf_dtp_coupling_bwd(const float* d_coupling, const float* cg, const eqf_dtp_paths* paths, float* d_sh, int E,
                         void* stream) {
  if (!d_coupling || !cg || !paths || !d_sh) return EQF_E_BADARG;
  if (E <= 0) return 0;
  const long total = (long)E * paths->sh_dim;
  hipLaunchKernelGGL(coupling_bwd_kernel, dim3(eqf_cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, d_coupling, cg,
                     *paths, d_sh, total);
  EQF_CHECK_LAUNCH();
  return 0;
}

int eqf_dtp_fwd(const float* x, const float* coupling, const float* w, const eqf_dtp_paths* paths, float* out, int E,
                void* stream) {
  if (!x || !coupling || !paths || !out) return EQF_E_BADARG;
  for (int p = 0; p < paths->npaths; ++p)
    if (paths->l1[p] > 3) return EQF_E_UNSUPPORTED;
  if (E <= 0) return 0;
  hipLaunchKernelGGL(dtp_fwd_kernel, dim3(E, eqf_cdiv(paths->w_numel, 256)), dim3(256), 0, (hipStream_t)stream, x,
                     coupling, w, *paths, out);
  EQF_CHECK_LAUNCH();
  return 0;
}

int eqf_dtp_bwd(const float* x, const float* coupling, const float* w, const eqf_dtp_paths* paths, const float* d_out,
                float* dx, float* dw, float* d_coupling, int E, void* stream) {
  if (!x || !coupling || !paths || !d_out || !dx) return EQF_E_BADARG;
  InSegs S{};
  for (int p = 0; p < paths->npaths; ++p) {
    if (paths->l1[p] > 3) return EQF_E_UNSUPPORTED;
    bool found = false;
    for (int s = 0; s < S.nseg; ++s) found |= (S.off[s] == paths->in_off[p]);
    if (!found) {
      if (S.nseg >= EQF_MAX_SEG) return EQF_E_UNSUPPORTED;
      S.off[S.nseg] = paths->in_off[p];
      S.mul[S.nseg] = paths->mul[p];
      S.nseg++;
    }
  }
  // input channels no path reads still need dx = 0: the caller zero-fills dx (see ops.py); here we cover fed segments
  S.cum[0] = 0;
  for (int s = 0; s < S.nseg; ++s) S.cum[s + 1] = S.cum[s] + S.mul[s];
  if (E <= 0) return 0;
  const size_t lds = d_coupling ? sizeof(float) * paths->m_numel : 0;
  hipLaunchKernelGGL(dtp_bwd_kernel, dim3(E), dim3(256), lds, (hipStream_t)stream, x, coupling, w, *paths, S, d_out, dx,
                     dw, d_coupling);
  EQF_CHECK_LAUNCH();
  return 0;
}

int eqf_alpha_fwd(const float* a, const float* alpha_dot, float* logit, int E, int H, int Kh, float c, void* stream) {
  if (!a || !alpha_dot || !logit) return EQF_E_BADARG;
  if (!(Kh == 8 || Kh == 16 || Kh == 32 || Kh == 64)) return EQF_E_UNSUPPORTED;
  if (E <= 0) return 0;
  const long total = (long)E * H * Kh;
  hipLaunchKernelGGL(alpha_fwd_kernel, dim3(eqf_cdiv(total, 256 * ALPHA_U)), dim3(256), 0, (hipStream_t)stream, a, alpha_dot,
                     logit, total, H * Kh, Kh, c);
  EQF_CHECK_LAUNCH();
  return 0;
}

int eqf_alpha_bwd(const float* a, const float* alpha_dot, const float* d_logit, float* da, float* d_alpha_dot, int E,
                  int H, int Kh, float c, void* stream) {
  if (!a || !alpha_dot || !d_logit || !da || !d_alpha_dot) return EQF_E_BADARG;
  if (E <= 0) return 0;
  if ((H * Kh) % 4 == 0 && Kh % 4 == 0 && H * Kh <= 256 && 256 % (H * Kh / 4) == 0) {
    const int CH4 = 64;
    hipLaunchKernelGGL(alpha_bwd4_kernel, dim3(eqf_cdiv(E, CH4)), dim3(256), 0, (hipStream_t)stream, a, alpha_dot, d_logit,
                       da, d_alpha_dot, E, H * Kh, Kh, c, CH4);
    EQF_CHECK_LAUNCH();
    return 0;
  }
  const int CH = 16;  // few edges per thread (serial loop), one atomic per column and workgroup
  hipLaunchKernelGGL(alpha_bwd_kernel, dim3(eqf_cdiv(H * Kh, 128), eqf_cdiv(E, CH)), dim3(128), 0, (hipStream_t)stream,
                     a, alpha_dot, d_logit, da, d_alpha_dot, E, H * Kh, Kh, c, CH);
  EQF_CHECK_LAUNCH();
  return 0;
}

static int attn_aggregate_fwd_impl(const float* logit, const float* value, const int* row_ptr, float* alpha, float* out, int N,
                                   int H, const eqf_irreps* irreps, float drop_p, unsigned long long seed,
                                   const unsigned long long* seed_off, void* stream) {
  if (!logit || !value || !row_ptr || !alpha || !out || !irreps || H < 1) return EQF_E_BADARG;
  int err;
  const HeadTab T = make_headtab(*irreps, H, &err);
  if (err) return err;
  if (N <= 0) return 0;
  // HBM-bound kernel: timed for the "HBM GB/s on the scatter" figure of bench.py (bytes are filled in there, the edge
  // count lives on the device)
  const int pid = eqf_prof_begin("attn_fwd", (hipStream_t)stream, 0.0, 0.0);
  if (T.G <= 32)
    hipLaunchKernelGGL(attn_fwd_half_kernel, dim3(N), dim3(64 * H), 0, (hipStream_t)stream, logit, value, row_ptr, alpha,
                       out, T, drop_p, seed, seed_off);
  else
    hipLaunchKernelGGL(attn_fwd_kernel, dim3(N), dim3(64 * H), 0, (hipStream_t)stream, logit, value, row_ptr, alpha, out,
                       T, drop_p, seed, seed_off);
  eqf_prof_end(pid, (hipStream_t)stream);
  EQF_CHECK_LAUNCH();
  return 0;
}

int eqf_attn_aggregate_fwd(const float* logit, const float* value, const int* row_ptr, float* alpha, float* out, int N,
                           int H, const eqf_irreps* irreps, float drop_p, unsigned long long seed, void* stream) {
  return attn_aggregate_fwd_impl(logit, value, row_ptr, alpha, out, N, H, irreps, drop_p, seed, nullptr, stream);
}
int eqf_attn_aggregate_fwd_dseed(const float* logit, const float* value, const int* row_ptr, float* alpha, float* out, int N,
                                 int H, const eqf_irreps* irreps, float drop_p, unsigned long long seed,
                                 const unsigned long long* seed_offset, void* stream) {
  return attn_aggregate_fwd_impl(logit, value, row_ptr, alpha, out, N, H, irreps, drop_p, seed, seed_offset, stream);
}

static int attn_aggregate_bwd_impl(const float* alpha, const float* value, const int* row_ptr, const float* d_out,
                                   float* d_value, float* d_logit, int N, int H, const eqf_irreps* irreps, float drop_p,
                                   unsigned long long seed, const unsigned long long* seed_off, void* stream) {
  if (!alpha || !value || !row_ptr || !d_out || !d_value || !d_logit || !irreps || H < 1) return EQF_E_BADARG;
  int err;
  const HeadTab T = make_headtab(*irreps, H, &err);
  if (err) return err;
  if (N <= 0) return 0;
  const int pid = eqf_prof_begin("attn_bwd", (hipStream_t)stream, 0.0, 0.0);
  if (T.G <= 32)
    hipLaunchKernelGGL(attn_bwd_half_kernel, dim3(N), dim3(64 * H), 0, (hipStream_t)stream, alpha, value, row_ptr, d_out,
                       d_value, d_logit, T, drop_p, seed, seed_off);
  else
    hipLaunchKernelGGL(attn_bwd_kernel, dim3(N), dim3(64 * H), 0, (hipStream_t)stream, alpha, value, row_ptr, d_out,
                       d_value, d_logit, T, drop_p, seed, seed_off);
  eqf_prof_end(pid, (hipStream_t)stream);
  EQF_CHECK_LAUNCH();
  return 0;
}
int eqf_attn_aggregate_bwd(const float* alpha, const float* value, const int* row_ptr, const float* d_out,
                           float* d_value, float* d_logit, int N, int H, const eqf_irreps* irreps, float drop_p,
                           unsigned long long seed, void* stream) {
  return attn_aggregate_bwd_impl(alpha, value, row_ptr, d_out, d_value, d_logit, N, H, irreps, drop_p, seed, nullptr, stream);
}
int eqf_attn_aggregate_bwd_dseed(const float* alpha, const float* value, const int* row_ptr, const float* d_out,
                                 float* d_value, float* d_logit, int N, int H, const eqf_irreps* irreps, float drop_p,
                                 unsigned long long seed, const unsigned long long* seed_offset, void* stream) {
  return attn_aggregate_bwd_impl(alpha, value, row_ptr, d_out, d_value, d_logit, N, H, irreps, drop_p, seed, seed_offset, stream);
}

}  // extern "C"
