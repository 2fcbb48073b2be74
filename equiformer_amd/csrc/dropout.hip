// Equivariant dropout drawn in the kernel (HBM-bound: one read and one write per element).
//
// out[row, s, m, u] = f(row, c) * x[row, s, m, u] with ONE factor per irrep instance (segment s, channel u), shared by its
// 2l+1 components m -- the sharing is what keeps the operator equivariant [ref: nets/drop.py:68-86 EquivariantDropout; with
// scalars_only the factor applies to the 0e segments alone and every other segment is copied, :89-108
// EquivariantScalarsDropout].  c = (channels of the segments before s) + u counts the irrep instances of the row, and
//   f(row, c) = u01 >= drop_p ? inv_keep : 0,   u01 = the uniform of rng.h for seed0 + *seed_word, tag 33,
//                                               index (call << 48) | (row << 16) | c
// -- a pure function of its arguments: it depends neither on the launch geometry nor on the number of rows, so a padded batch
// drops on its real rows what the unpadded batch drops, a captured launch whose host advances the word between replays draws a
// fresh mask every replay, and the backward (the same launch on dy) redraws the mask of its forward.
//
// One wavefront owns whole rows (grid stride beyond the grid).  A lane's work item is a channel quad of one segment: it
// makes the quad's four draws once, then walks the 2l+1 components at stride mul -- one 16-byte load and one 16-byte store
// each, neighbouring lanes on neighbouring quads (coalesced), no hash per component.  The key of (seed, tag) and the segment
// table are wave-uniform.  A multiply, not a select: a NaN in a dropped entry stays NaN, a dropped entry is +-0.
// What the kernel costs beyond a launch is the draws: one 64-bit hash per dropped irrep, three 64-bit integer multiplies
// each, at a quarter of the VALU rate.  A wavefront per 64-quad chunk of a row instead of per row -- three times the
// wavefronts at the OC20 feature, the loads requested before the draws -- measured the same time per launch and triples
// the wavefronts that draw on narrow rows (QM9: 56 quads in three segments); it was not kept.
#include "common.h"
#include "rng.h"

namespace {

constexpr unsigned long long DROPOUT_TAG = 33;  // (dens.hip: 0-2, is2rs.hip: 16-18, edge.hip stochastic depth: 32)
constexpr int DROPOUT_WAVES = 4;
constexpr int DROPOUT_MAX_BLOCKS = 2048;  // 8 per CU; the rows beyond 4 x 2048 by the grid stride

struct DropTab {
  int nseg;
  int off4[EQF_MAX_SEG];   // row offset of the segment, in float4
  int mul4[EQF_MAX_SEG];   // channel quads
  int comps[EQF_MAX_SEG];  // 2l+1
  int ch[EQF_MAX_SEG];     // irrep instances in front of the segment
  int drop[EQF_MAX_SEG];   // 0: the segment is copied through
  int D4;
};

__device__ __forceinline__ float keep_factor(unsigned long long key, unsigned long long idx, float drop_p, float inv_keep) {
  return eqf_rand_uniform_keyed(key, idx) >= drop_p ? inv_keep : 0.f;
}

__global__ __launch_bounds__(64 * DROPOUT_WAVES) void irreps_dropout_kernel(
    const float* __restrict__ x, float* __restrict__ out, int rows, const DropTab T, float drop_p, float inv_keep,
    unsigned long long seed0, const unsigned long long* __restrict__ seed_word, unsigned long long call) {
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int lane = (int)(threadIdx.x & 63);
  const unsigned long long key = eqf_rand_key(seed0 + (seed_word ? *seed_word : 0ull), DROPOUT_TAG);
  const long stride = (long)gridDim.x * DROPOUT_WAVES;
  for (long row = (long)blockIdx.x * DROPOUT_WAVES + wave; row < rows; row += stride) {
    const float4* xr = reinterpret_cast<const float4*>(x) + row * T.D4;
    float4* orow = reinterpret_cast<float4*>(out) + row * T.D4;
    const unsigned long long base = (call << 48) | ((unsigned long long)row << 16);
    for (int s = 0; s < T.nseg; ++s) {
      const int mul4 = T.mul4[s], comps = T.comps[s], drop = T.drop[s];
      const float4* xs = xr + T.off4[s];
      float4* os = orow + T.off4[s];
      for (int q = lane; q < mul4; q += 64) {
        float4 f = make_float4(1.f, 1.f, 1.f, 1.f);
        if (drop) {
          const unsigned long long c = (unsigned long long)(T.ch[s] + 4 * q);
          f.x = keep_factor(key, base | c, drop_p, inv_keep);
          f.y = keep_factor(key, base | (c + 1), drop_p, inv_keep);
          f.z = keep_factor(key, base | (c + 2), drop_p, inv_keep);
          f.w = keep_factor(key, base | (c + 3), drop_p, inv_keep);
        }
        // four components per step: their loads are in flight together before the first store
        for (int m0 = 0; m0 < comps; m0 += 4) {
          float4 v[4];
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (m0 + j < comps) v[j] = xs[(m0 + j) * mul4 + q];
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (m0 + j < comps) {
              if (drop) v[j].x *= f.x, v[j].y *= f.y, v[j].z *= f.z, v[j].w *= f.w;  // (else: the bits of x)
              os[(m0 + j) * mul4 + q] = v[j];
            }
        }
      }
    }
  }
}

}  // namespace

extern "C" {

int eqf_irreps_dropout(const float* x, float* out, int rows, const eqf_irreps* ir, int scalars_only, float drop_p,
                       float inv_keep, unsigned long long seed, const unsigned long long* seed_word,
                       unsigned long long call, void* stream) {
  if (!x || !out || !ir || ir->nseg < 0 || ir->nseg > EQF_MAX_SEG) return EQF_E_BADARG;
  DropTab T{};
  T.nseg = ir->nseg;
  long off = 0, ch = 0;
  for (int s = 0; s < ir->nseg; ++s) {
    if (ir->mul[s] < 0 || ir->l[s] < 0) return EQF_E_BADARG;
    if (ir->mul[s] % 4) return EQF_E_UNSUPPORTED;
    T.off4[s] = (int)(off / 4);
    T.mul4[s] = ir->mul[s] / 4;
    T.comps[s] = 2 * ir->l[s] + 1;
    T.ch[s] = (int)ch;
    T.drop[s] = !scalars_only || (ir->l[s] == 0 && !ir->odd[s]);
    off += (long)ir->mul[s] * (2 * ir->l[s] + 1);
    ch += ir->mul[s];
    if (off > INT32_MAX) return EQF_E_BADARG;
  }
  // the index of a draw packs (call, row, channel) into 16 + 32 + 16 bits
  if (ch >= (1 << 16) || call >= (1ull << 16)) return EQF_E_UNSUPPORTED;
  T.D4 = (int)(off / 4);
  if (rows <= 0 || off == 0) return 0;
  const long blocks = eqf_cdiv((long)rows, (long)DROPOUT_WAVES);
  hipLaunchKernelGGL(irreps_dropout_kernel, dim3((unsigned)(blocks < DROPOUT_MAX_BLOCKS ? blocks : DROPOUT_MAX_BLOCKS)),
                     dim3(64 * DROPOUT_WAVES), 0, (hipStream_t)stream, x, out, rows, T, drop_p, inv_keep, seed, seed_word,
                     call);
  EQF_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
