// Equivariant graph norm and instance norm: the node-side norms whose statistics are taken per (graph, channel) ACROSS the
// nodes of a graph, not per row [ref: nets/graph_norm.py:9-134 EquivariantGraphNorm, nets/instance_norm.py:9-134
// EquivariantInstanceNorm; reduce='mean', normalization='component', affine=True].  For one channel u of a segment of
// dimension d = 2l+1, in one graph g with n nodes:
//   0e segments:  mu = (1/n) sum_nodes x,  c = x - mean_shift[u] * mu   (instance norm: mean_shift == 1)
//   the others:   c = x                                                  (0o included)
//   v = (1/(n d)) sum_nodes sum_m c^2,  y = c * (v + eps)^(-1/2) * weight[u]  (+ bias[u] on 0e)
// One kernel family serves both norms (mean_shift == NULL: instance norm).  Segmented reductions over mol_ptr: a
// workgroup owns (graph, 64 channels), lane = channel (loads coalesced over u), its waves split the nodes of the graph and
// combine in LDS in wave order -- no atomics anywhere in this file, every result is independent of launch order.  The
// sums run in fp64 (a handful of adds per loaded value; these kernels wait for HBM and launch latency, not for the ALUs).
#include "common.h"

namespace {

constexpr int GN_WAVES = 4;     // waves of a reduction workgroup = node (or graph) slices
constexpr int GN_ROW_WAVES = 4; // rows per workgroup of the row-wise kernels

struct GnTab {
  int nseg;
  int off[EQF_MAX_SEG];   // row offset
  int mul[EQF_MAX_SEG];
  int d[EQF_MAX_SEG];     // 2l+1
  int woff[EQF_MAX_SEG];  // first channel of the segment among all channels (affine_weight, rstd column)
  int boff[EQF_MAX_SEG];  // first channel among the 0e channels (affine_bias, mean_shift, mean column), else -1
  int D, K, C0;           // row length, channels, 0e channels
};

GnTab make_gntab(const eqf_irreps& ir) {
  GnTab t{};
  t.nseg = ir.nseg;
  int off = 0, w = 0, b = 0;
  for (int s = 0; s < ir.nseg; ++s) {
    const bool scalar = ir.l[s] == 0 && !ir.odd[s];  // `ir.l == 0 and ir.p == 1`: a pseudo-scalar (0o) is not centred
    t.off[s] = off;
    t.mul[s] = ir.mul[s];
    t.d[s] = 2 * ir.l[s] + 1;
    t.woff[s] = w;
    t.boff[s] = scalar ? b : -1;
    w += ir.mul[s];
    if (scalar) b += ir.mul[s];
    off += ir.mul[s] * t.d[s];
  }
  t.D = off;
  t.K = w;
  t.C0 = b;
  return t;
}

// channel k -> (segment, channel within the segment)
__device__ __forceinline__ void gn_channel(const GnTab& T, int k, int& s, int& u) {
  s = 0;
  while (s + 1 < T.nseg && k >= T.woff[s + 1]) ++s;
  u = k - T.woff[s];
}

// nodes [beg, end) of graph g, clamped to the rows that exist
__device__ __forceinline__ void gn_nodes(const int* __restrict__ mol_ptr, int g, int rows, int& beg, int& end) {
  beg = min(max(mol_ptr[g], 0), rows);
  end = min(max(mol_ptr[g + 1], beg), rows);
}

// sum over the waves of the workgroup in wave order (every thread gets the total of its lane)
__device__ __forceinline__ double gn_combine(double (*part)[64], double v, int wave, int lane) {
  __syncthreads();  // (the previous round's reads are done)
  part[wave][lane] = v;
  __syncthreads();
  double t = part[0][lane];
#pragma unroll
  for (int w = 1; w < GN_WAVES; ++w) t += part[w][lane];
  return t;
}

// ---------------------------------------------------------------------------------------------- forward statistics
// grid (num_graphs, ceil(K / 64)).  Two passes over the graph's nodes: the mean first, then the centred squares (inputs
// like randn + 100 cancel in a one-pass E[x^2] - E[x]^2).  x2 optional: x + x2 is what is normalised.
__global__ __launch_bounds__(64 * GN_WAVES) void graphnorm_stats_kernel(
    const float* __restrict__ x, const float* __restrict__ x2, const float* __restrict__ mean_shift,
    float* __restrict__ mean, float* __restrict__ rstd, const int* __restrict__ mol_ptr, int rows, GnTab T, float eps) {
  __shared__ double part[GN_WAVES][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = blockIdx.x, k = blockIdx.y * 64 + lane;
  const bool live = k < T.K;
  int s = 0, u = 0;
  if (live) gn_channel(T, k, s, u);
  const int mul = T.mul[s], d = T.d[s], b = T.boff[s] >= 0 ? T.boff[s] + u : -1;
  const bool is0 = live && b >= 0;
  int beg, end;
  gn_nodes(mol_ptr, g, rows, beg, end);
  const int n = end - beg;
  if (n <= 0) {  // an empty graph has no rows: nothing divides by n, the saved statistics are defined
    if (wave == 0 && live) rstd[(long)g * T.K + k] = 0.f;
    if (wave == 0 && is0) mean[(long)g * T.C0 + b] = 0.f;
    return;
  }
  const long col = T.off[s] + u;
  double acc = 0.0;
  if (is0)
    for (int i = beg + wave; i < end; i += GN_WAVES) {
      const long e = (long)i * T.D + col;
      acc += (double)(x2 ? x[e] + x2[e] : x[e]);
    }
  const float mu = (float)(gn_combine(part, acc, wave, lane) / n);
  const float shift = is0 ? __fmul_rn(mean_shift ? mean_shift[b] : 1.f, mu) : 0.f;
  acc = 0.0;
  if (live)
    for (int i = beg + wave; i < end; i += GN_WAVES)
      for (int m = 0; m < d; ++m) {
        const long e = (long)i * T.D + col + m * mul;
        const float c = (x2 ? x[e] + x2[e] : x[e]) - shift;
        acc += (double)c * (double)c;
      }
  const double v = gn_combine(part, acc, wave, lane) / ((double)n * d);
  if (wave == 0 && live) rstd[(long)g * T.K + k] = (float)(1.0 / sqrt(v + (double)eps));
  if (wave == 0 && is0) mean[(long)g * T.C0 + b] = mu;
}

// ---------------------------------------------------------------------------------------------- forward apply
// One wave per row, as layernorm_fwd_kernel; the statistics of the row's graph are looked up through batch[row].
__global__ __launch_bounds__(64 * GN_ROW_WAVES) void graphnorm_apply_kernel(
    const float* __restrict__ x, const float* __restrict__ x2, float* __restrict__ xsum,
    const float* __restrict__ mean_shift, const float* __restrict__ w, const float* __restrict__ bias,
    const float* __restrict__ mean, const float* __restrict__ rstd, const int* __restrict__ batch,
    float* __restrict__ y, int rows, int num_graphs, GnTab T) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * GN_ROW_WAVES + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int g = batch[row];
  const bool known = g >= 0 && g < num_graphs;  // a row of no graph is passed on (xsum) and normalised to zero
  const long r0 = (long)row * T.D;
  for (int s = 0; s < T.nseg; ++s) {
    const int off = T.off[s], len = T.mul[s] * T.d[s], mul = T.mul[s];
    for (int i = lane; i < len; i += 64) {
      const int u = i % mul, k = T.woff[s] + u;
      const long e = r0 + off + i;
      const float xv = x2 ? x[e] + x2[e] : x[e];
      if (xsum) xsum[e] = xv;
      float v = 0.f;
      if (known) {
        float c = xv, bv = 0.f;
        if (T.boff[s] >= 0) {
          const int b = T.boff[s] + u;
          c = xv - __fmul_rn(mean_shift ? mean_shift[b] : 1.f, mean[(long)g * T.C0 + b]);
          bv = bias[b];
        }
        v = c * rstd[(long)g * T.K + k] * w[k] + bv;
      }
      y[e] = v;
    }
  }
}

// ---------------------------------------------------------------------------------------------- backward
// With c_hat = c * rstd and N = n d, per (graph, channel):
//   S1 = sum dy c_hat,   S2 = sum dy,   S3 = sum c_hat        (S2, S3 on 0e only; S3 = rstd n mu (1 - mean_shift) != 0)
//   dc = w rstd (dy - c_hat S1 / N),   Tg = sum_nodes dc = w rstd (S2 - S1 S3 / N)
//   dx = dc - mean_shift Tg / n = w rstd [(dy - mean_shift S2 / n) - (c_hat - mean_shift S3 / n) S1 / N]
//   d_weight += S1,  d_bias += S2,  d_mean_shift += -mu Tg     (summed over graphs)
// dx is formed in the second way: in a one-node graph dy - S2 is then an exact zero, as it is in the definition (the first
// way leaves the rounding of the stored Tg, times rstd = eps^(-1/2)).  The reduction kernel leaves S1 [B, K], S2, S3 and Tg
// [B, C0] in the caller's workspace, in fp64: with mean_shift near 1 the factor c_hat - mean_shift S3 / n is itself a small
// difference.  Grid as the statistics kernel.
__global__ __launch_bounds__(64 * GN_WAVES) void graphnorm_bwd_reduce_kernel(
    const float* __restrict__ x, const float* __restrict__ mean_shift, const float* __restrict__ w,
    const float* __restrict__ dy, const float* __restrict__ mean, const float* __restrict__ rstd,
    const int* __restrict__ mol_ptr, double* __restrict__ S1, double* __restrict__ S2, double* __restrict__ S3,
    double* __restrict__ Tg, int rows, GnTab T) {
  __shared__ double part[GN_WAVES][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = blockIdx.x, k = blockIdx.y * 64 + lane;
  const bool live = k < T.K;
  int s = 0, u = 0;
  if (live) gn_channel(T, k, s, u);
  const int mul = T.mul[s], d = T.d[s], b = T.boff[s] >= 0 ? T.boff[s] + u : -1;
  const bool is0 = live && b >= 0;
  int beg, end;
  gn_nodes(mol_ptr, g, rows, beg, end);
  const int n = end - beg;
  if (n <= 0) {  // the partials of an empty graph are zeros: the parameter gradients sum over every graph
    if (wave == 0 && live) S1[(long)g * T.K + k] = 0.0;
    if (wave == 0 && is0) S2[(long)g * T.C0 + b] = S3[(long)g * T.C0 + b] = Tg[(long)g * T.C0 + b] = 0.0;
    return;
  }
  const long col = T.off[s] + u;
  const float rs = live ? rstd[(long)g * T.K + k] : 0.f;
  const float shift = is0 ? __fmul_rn(mean_shift ? mean_shift[b] : 1.f, mean[(long)g * T.C0 + b]) : 0.f;
  double a1 = 0.0, a2 = 0.0, a3 = 0.0;
  if (live)
    for (int i = beg + wave; i < end; i += GN_WAVES)
      for (int m = 0; m < d; ++m) {
        const long e = (long)i * T.D + col + m * mul;
        const double ch = (double)(x[e] - shift) * (double)rs;
        const double gv = dy[e];
        a1 += gv * ch;
        a2 += gv;
        a3 += ch;
      }
  a1 = gn_combine(part, a1, wave, lane);
  a2 = gn_combine(part, a2, wave, lane);
  a3 = gn_combine(part, a3, wave, lane);
  if (wave == 0 && live) S1[(long)g * T.K + k] = a1;
  if (wave == 0 && is0) {
    S2[(long)g * T.C0 + b] = a2;
    S3[(long)g * T.C0 + b] = a3;
    Tg[(long)g * T.C0 + b] = (double)w[k] * (double)rs * (a2 - a1 * a3 / ((double)n * d));
  }
}

// dx, one wave per row (+ dres, the gradient arriving at the normalised sum from the residual branch)
__global__ __launch_bounds__(64 * GN_ROW_WAVES) void graphnorm_bwd_dx_kernel(
    const float* __restrict__ x, const float* __restrict__ mean_shift, const float* __restrict__ w,
    const float* __restrict__ dy, const float* __restrict__ dres, const float* __restrict__ mean,
    const float* __restrict__ rstd, const int* __restrict__ mol_ptr, const int* __restrict__ batch,
    const double* __restrict__ S1, const double* __restrict__ S2, const double* __restrict__ S3,
    float* __restrict__ dx, int rows, int num_graphs, GnTab T) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * GN_ROW_WAVES + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int g = batch[row];
  const bool known = g >= 0 && g < num_graphs;
  const int n = known ? max(mol_ptr[g + 1] - mol_ptr[g], 1) : 1;
  const double inv_n = 1.0 / (double)n;
  const long r0 = (long)row * T.D;
  for (int s = 0; s < T.nseg; ++s) {
    const int off = T.off[s], len = T.mul[s] * T.d[s], mul = T.mul[s];
    const double inv_N = inv_n / (double)T.d[s];
    for (int i = lane; i < len; i += 64) {
      const int u = i % mul, k = T.woff[s] + u;
      const long e = r0 + off + i;
      // In a graph of one to three nodes the 0e terms below cancel, to an exact zero or to a residue of order eps: they are
      // combined in fp64, so that the rounding of this kernel does not add to that of the saved statistics.
      double v = 0.0;
      if (known) {
        const double rs = rstd[(long)g * T.K + k];
        float shift = 0.f;
        double m2 = 0.0, m3 = 0.0;  // mean_shift * (mean over the nodes of dy, of c_hat)
        if (T.boff[s] >= 0) {
          const int b = T.boff[s] + u;
          const float a = mean_shift ? mean_shift[b] : 1.f;
          shift = __fmul_rn(a, mean[(long)g * T.C0 + b]);
          m2 = (double)a * (S2[(long)g * T.C0 + b] * inv_n);
          m3 = (double)a * (S3[(long)g * T.C0 + b] * inv_n);
        }
        const double ch = (double)(x[e] - shift) * rs;
        v = (double)w[k] * rs * (((double)dy[e] - m2) - (ch - m3) * (S1[(long)g * T.K + k] * inv_N));
      }
      if (dres) v += (double)dres[e];
      dx[e] = (float)v;
    }
  }
}

// Parameter gradients from the per-graph partials: grid ceil(K / 64), lane = channel, the waves split the graphs and
// combine in wave order; one thread adds the total to the caller's accumulator (nobody else writes that element).
__global__ __launch_bounds__(64 * GN_WAVES) void graphnorm_param_grad_kernel(
    const double* __restrict__ S1, const double* __restrict__ S2, const double* __restrict__ Tg,
    const float* __restrict__ mean, float* __restrict__ d_weight, float* __restrict__ d_bias,
    float* __restrict__ d_mean_shift, int num_graphs, GnTab T) {
  __shared__ double part[GN_WAVES][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int k = blockIdx.x * 64 + lane;
  const bool live = k < T.K;
  int s = 0, u = 0;
  if (live) gn_channel(T, k, s, u);
  const int b = T.boff[s] >= 0 ? T.boff[s] + u : -1;
  const bool is0 = live && b >= 0;
  double a1 = 0.0, a2 = 0.0, a3 = 0.0;
  if (live)
    for (int g = wave; g < num_graphs; g += GN_WAVES) {
      a1 += S1[(long)g * T.K + k];
      if (is0) {
        a2 += S2[(long)g * T.C0 + b];
        a3 -= (double)mean[(long)g * T.C0 + b] * Tg[(long)g * T.C0 + b];
      }
    }
  a1 = gn_combine(part, a1, wave, lane);
  a2 = gn_combine(part, a2, wave, lane);
  a3 = gn_combine(part, a3, wave, lane);
  if (wave != 0) return;
  if (live) d_weight[k] += (float)a1;
  if (is0) {
    d_bias[b] += (float)a2;
    if (d_mean_shift) d_mean_shift[b] += (float)a3;
  }
}

}  // namespace

extern "C" {

int eqf_graphnorm_fwd(const float* x, const float* x2, float* xsum, const float* mean_shift, const float* weight,
                      const float* bias, float* y, float* mean, float* rstd, const int* mol_ptr, const int* batch, int rows,
                      int num_graphs, const eqf_irreps* irreps, float eps, void* stream) {
  if (!x || !weight || !bias || !y || !mean || !rstd || !mol_ptr || !batch || !irreps || num_graphs <= 0)
    return EQF_E_BADARG;
  if (irreps->nseg < 1 || irreps->nseg > EQF_MAX_SEG) return EQF_E_BADARG;
  if ((x2 != nullptr) != (xsum != nullptr)) return EQF_E_BADARG;
  if (rows <= 0) return 0;
  const GnTab T = make_gntab(*irreps);
  hipLaunchKernelGGL(graphnorm_stats_kernel, dim3(num_graphs, eqf_cdiv(T.K, 64)), dim3(64 * GN_WAVES), 0,
                     (hipStream_t)stream, x, x2, mean_shift, mean, rstd, mol_ptr, rows, T, eps);
  EQF_CHECK_LAUNCH();
  hipLaunchKernelGGL(graphnorm_apply_kernel, dim3(eqf_cdiv(rows, GN_ROW_WAVES)), dim3(64 * GN_ROW_WAVES), 0,
                     (hipStream_t)stream, x, x2, xsum, mean_shift, weight, bias, mean, rstd, batch, y, rows, num_graphs, T);
  EQF_CHECK_LAUNCH();
  return 0;
}

int eqf_graphnorm_bwd(const float* x, const float* mean_shift, const float* weight, const float* dy, const float* dres,
                      const float* mean, const float* rstd, const int* mol_ptr, const int* batch, float* dx,
                      float* d_weight, float* d_bias, float* d_mean_shift, double* workspace, int rows, int num_graphs,
                      const eqf_irreps* irreps, void* stream) {
  if (!x || !weight || !dy || !mean || !rstd || !mol_ptr || !batch || !dx || !workspace || !irreps || num_graphs <= 0)
    return EQF_E_BADARG;
  if (irreps->nseg < 1 || irreps->nseg > EQF_MAX_SEG) return EQF_E_BADARG;
  if ((d_weight != nullptr) != (d_bias != nullptr)) return EQF_E_BADARG;
  if (d_mean_shift && (!mean_shift || !d_weight)) return EQF_E_BADARG;
  if (rows <= 0) return 0;
  const GnTab T = make_gntab(*irreps);
  double* S1 = workspace;
  double* S2 = S1 + (long)num_graphs * T.K;
  double* S3 = S2 + (long)num_graphs * T.C0;
  double* Tg = S3 + (long)num_graphs * T.C0;
  hipLaunchKernelGGL(graphnorm_bwd_reduce_kernel, dim3(num_graphs, eqf_cdiv(T.K, 64)), dim3(64 * GN_WAVES), 0,
                     (hipStream_t)stream, x, mean_shift, weight, dy, mean, rstd, mol_ptr, S1, S2, S3, Tg, rows, T);
  EQF_CHECK_LAUNCH();
  hipLaunchKernelGGL(graphnorm_bwd_dx_kernel, dim3(eqf_cdiv(rows, GN_ROW_WAVES)), dim3(64 * GN_ROW_WAVES), 0,
                     (hipStream_t)stream, x, mean_shift, weight, dy, dres, mean, rstd, mol_ptr, batch, S1, S2, S3, dx,
                     rows, num_graphs, T);
  EQF_CHECK_LAUNCH();
  if (d_weight) {
    hipLaunchKernelGGL(graphnorm_param_grad_kernel, dim3(eqf_cdiv(T.K, 64)), dim3(64 * GN_WAVES), 0, (hipStream_t)stream,
                       S1, S2, Tg, mean, d_weight, d_bias, d_mean_shift, num_graphs, T);
    EQF_CHECK_LAUNCH();
  }
  return 0;
}

}  // extern "C"
