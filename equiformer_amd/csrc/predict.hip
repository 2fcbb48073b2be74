// The OC20 prediction pass, gathered on the device [ref: oc20/trainer/energy_trainer_v2.py:170-204 predict].  The reference
// denormalises every batch's energies with ATen and reads them back (`.tolist()`), and with write_pos adds the denormalised
// displacement to the free atoms through two boolean indices and copies the positions to the host (`.cpu()`): three host
// synchronisations per batch.  Here one launch per batch appends the batch to result buffers that stay on the device; nothing
// is read back until the pass is over, and the launch can be captured in a HIP graph (equiformer_amd/evaluate.py).
//   * where a batch lands is not an argument: the launch reads the two cursors, the capacities and the addresses of the
//     result buffers from a descriptor in device memory and advances the cursors itself, so a REPLAYED launch appends
//     behind the previous one, and buffers the host has grown in between are found at their new addresses.
//   * a batch is a few thousand floats: the launch is latency-bound whatever its shape, so ONE workgroup strides over the
//     rows (as metrics.hip does) and, after a barrier, one thread advances the cursors.  No atomics: launches that share a
//     descriptor are ordered by their stream.
//   * a batch is taken whole or not at all: one that does not fit a capacity writes nothing and is counted as dropped.
//   * excluded rows (the phantom structure, rows >= mol_ptr[B]) are never read: a NaN there reaches nothing.
#include <cstdint>
#include "common.h"

// Energies and positions are specified as separately rounded fp32 operations (what eager torch computes); see is2rs.hip.
#pragma clang fp contract(off)

namespace {

constexpr int PR_THREADS = EQF_PREDICT_THREADS;

struct PredictNorm {
  float e_mean, e_std;
  float pm0, pm1, pm2, ps0, ps1, ps2;
};

// grid 1 x PR_THREADS
template <typename TagT>
__global__ __launch_bounds__(PR_THREADS) void predict_append_kernel(
    const float* __restrict__ energy, const long long* __restrict__ sid, const int* __restrict__ mol_ptr, int B,
    const float* __restrict__ pos, const float* __restrict__ delta, const TagT* __restrict__ tags, PredictNorm nm,
    long long* desc) {
  const long long gc = desc[EQF_PREDICT_GRAPH_CURSOR], ac = desc[EQF_PREDICT_ATOM_CURSOR];
  const long long gcap = desc[EQF_PREDICT_GRAPH_CAP], acap = desc[EQF_PREDICT_ATOM_CAP];
  float* const e_out = (float*)(uintptr_t)desc[EQF_PREDICT_ENERGY_OUT];
  long long* const sid_out = (long long*)(uintptr_t)desc[EQF_PREDICT_SID_OUT];
  int* const natoms_out = (int*)(uintptr_t)desc[EQF_PREDICT_NATOMS_OUT];
  float* const pos_out = (float*)(uintptr_t)desc[EQF_PREDICT_POS_OUT];
  const int r0 = mol_ptr[0];
  const long long n = pos ? (long long)mol_ptr[B] - r0 : 0;  // real rows; without positions the atom part is left alone
  const bool fits = gc >= 0 && ac >= 0 && n >= 0 && e_out && sid_out && natoms_out && gc + B <= gcap &&
                    (!pos || (pos_out && ac + n <= acap));
  if (fits) {
    for (int b = threadIdx.x; b < B; b += PR_THREADS) {
      const float scaled = energy[b] * nm.e_std;
      e_out[gc + b] = scaled + nm.e_mean;
      sid_out[gc + b] = sid[b];
      natoms_out[gc + b] = mol_ptr[b + 1] - mol_ptr[b];
    }
    // one float per lane: consecutive lanes read and write consecutive addresses
    for (long long e = threadIdx.x; e < 3 * n; e += PR_THREADS) {
      const long long row = e / 3;
      const int c = (int)(e - 3 * row);
      const long long i = r0 + row, at = 3 * (long long)r0 + e;
      float p = pos[at];
      if (tags[i] > 0) {  // a free atom; a fixed one keeps the bits of pos
        const float scaled = delta[at] * (c == 0 ? nm.ps0 : c == 1 ? nm.ps1 : nm.ps2);
        const float d = scaled + (c == 0 ? nm.pm0 : c == 1 ? nm.pm1 : nm.pm2);
        p = p + d;
      }
      pos_out[3 * ac + e] = p;
    }
  }
  __syncthreads();  // every lane has read the cursors
  if (threadIdx.x != 0) return;
  if (fits) {
    desc[EQF_PREDICT_GRAPH_CURSOR] = gc + B;
    if (pos) desc[EQF_PREDICT_ATOM_CURSOR] = ac + n;
  } else {
    desc[EQF_PREDICT_DROPPED_GRAPHS] += B;
    desc[EQF_PREDICT_DROPPED_ATOMS] += n > 0 ? n : 0;
  }
}

}  // namespace

extern "C" {

int eqf_predict_append(const float* energy, const long long* sid, const int* mol_ptr, int B, const float* pos,
                       const float* delta, const void* tags, int tags_is64, float target_mean, float target_std,
                       float pos_mean_x, float pos_mean_y, float pos_mean_z, float pos_std_x, float pos_std_y,
                       float pos_std_z, long long* desc, void* stream) {
  if (!energy || !sid || !mol_ptr || !desc || B < 0) return EQF_E_BADARG;
  if (pos ? (!delta || !tags) : (delta || tags)) return EQF_E_BADARG;  // the atom part comes whole or not at all
  if (B == 0) return 0;
  PredictNorm nm;
  nm.e_mean = target_mean, nm.e_std = target_std;
  nm.pm0 = pos_mean_x, nm.pm1 = pos_mean_y, nm.pm2 = pos_mean_z;
  nm.ps0 = pos_std_x, nm.ps1 = pos_std_y, nm.ps2 = pos_std_z;
  if (tags_is64)
    hipLaunchKernelGGL(predict_append_kernel<long long>, dim3(1), dim3(PR_THREADS), 0, (hipStream_t)stream, energy, sid,
                       mol_ptr, B, pos, delta, (const long long*)tags, nm, desc);
  else
    hipLaunchKernelGGL(predict_append_kernel<int>, dim3(1), dim3(PR_THREADS), 0, (hipStream_t)stream, energy, sid, mol_ptr,
                       B, pos, delta, (const int*)tags, nm, desc);
  EQF_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
