// Counter-based random numbers: every draw is a pure function of (seed, stream tag, index) -- no state, no dependence on
// the launch geometry, the same bits on every run.  The mixer is the splitmix64 finaliser that keep_scale (edge.hip) and
// the second-order dropout (second.hip) carry as private copies.
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ unsigned long long eqf_mix64(unsigned long long z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// 64 random bits of draw `idx` of stream `tag`: the tag is mixed into the seed first, so that two streams of one seed are
// two different sequences, not one sequence at two offsets.
// The two halves are separate functions for kernels that make many draws of one stream: the key depends on (seed, tag)
// alone -- wave-uniform, formed once -- and a draw costs one mix of (key, idx).
__device__ __forceinline__ unsigned long long eqf_rand_key(unsigned long long seed, unsigned long long tag) {
  return eqf_mix64(seed + 0xD6E8FEB86659FD93ull * (tag + 1));
}
__device__ __forceinline__ unsigned long long eqf_rand_bits_keyed(unsigned long long key, unsigned long long idx) {
  return eqf_mix64(key + 0x9E3779B97F4A7C15ull * (idx + 1));
}
__device__ __forceinline__ unsigned long long eqf_rand_bits(unsigned long long seed, unsigned long long tag,
                                                           unsigned long long idx) {
  return eqf_rand_bits_keyed(eqf_rand_key(seed, tag), idx);
}
// eqf_rand_uniform(seed, tag, idx) from the key of (seed, tag)
__device__ __forceinline__ float eqf_rand_uniform_keyed(unsigned long long key, unsigned long long idx) {
  return (float)(eqf_rand_bits_keyed(key, idx) >> 40) * (1.0f / 16777216.0f);
}

// uniform in [0, 1) from the top 24 bits (every value is an exact float: `u < 1.f` always, `u < 0.f` never)
__device__ __forceinline__ float eqf_rand_uniform(unsigned long long seed, unsigned long long tag, unsigned long long idx) {
  return (float)(eqf_rand_bits(seed, tag, idx) >> 40) * (1.0f / 16777216.0f);
}

// standard normal by Box-Muller: the radial uniform from the top 24 bits shifted into (0, 1] (the logarithm is finite,
// |x| <= sqrt(48 ln 2) = 5.77), the angle from the low 24 bits in [0, 1)
__device__ __forceinline__ float eqf_rand_normal(unsigned long long seed, unsigned long long tag, unsigned long long idx) {
  const unsigned long long z = eqf_rand_bits(seed, tag, idx);
  const float u1 = (float)((z >> 40) + 1ull) * (1.0f / 16777216.0f);
  const float u2 = (float)(z & 0xFFFFFFull) * (1.0f / 16777216.0f);
  return sqrtf(-2.0f * logf(u1)) * cosf(6.283185307179586f * u2);
}
