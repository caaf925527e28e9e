// Philox4x64-10 (Random123; the generator numpy ships as np.random.Philox): counter (c0, c1, c2, c3), key (k0, 0).
// Shared by the VAE noise (vae.hip), the negative draw of the link-prediction feed (linkpred.hip) and the noise of the smooth
// attribution methods (igprep.hip, seq.hip), which also share the Box-Muller below.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace kgcn {

constexpr uint64_t kPhiloxM0 = 0xD2E7470EE14C6C93ull, kPhiloxM1 = 0xCA5A826395121157ull;
constexpr uint64_t kPhiloxW0 = 0x9E3779B97F4A7C15ull, kPhiloxW1 = 0xBB67AE8584CAA73Bull;

struct Philox4 { uint64_t v[4]; };

__device__ __forceinline__ Philox4 philox4x64_10(uint64_t c0, uint64_t c1, uint64_t c2, uint64_t c3, uint64_t seed) {
  uint64_t x0 = c0, x1 = c1, x2 = c2, x3 = c3, k0 = seed, k1 = 0;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t lo0 = kPhiloxM0 * x0, hi0 = __umul64hi(kPhiloxM0, x0);
    const uint64_t lo1 = kPhiloxM1 * x2, hi1 = __umul64hi(kPhiloxM1, x2);
    x0 = hi1 ^ x1 ^ k0;
    x1 = lo1;
    x2 = hi0 ^ x3 ^ k1;
    x3 = lo0;
    k0 += kPhiloxW0;
    k1 += kPhiloxW1;
  }
  return Philox4{{x0, x1, x2, x3}};
}

__device__ __forceinline__ Philox4 philox4x64_10(uint64_t c0, uint64_t c1, uint64_t seed) {
  return philox4x64_10(c0, c1, 0, 0, seed);
}

// two 64-bit words -> two N(0, 1): u1 = (top 24 bits + 1) 2^-24 in (0, 1], u2 = top 24 bits 2^-24 in [0, 1)
__device__ __forceinline__ void box_muller(uint64_t w0, uint64_t w1, float& n0, float& n1) {
  const float u1 = (float)((w0 >> 40) + 1) * 0x1p-24f;
  const float u2 = (float)(w1 >> 40) * 0x1p-24f;
  const float r = sqrtf(-2.0f * logf(u1));
  float s, c;
  sincospif(2.0f * u2, &s, &c);
  n0 = r * c;
  n1 = r * s;
}

// Attribution noise (include/kgcn_hip.h, "noise of the smooth attribution methods"): the four normals of columns 4 q .. 4 q + 3
// of row r of a [R, W] array, stream s, compound g, sample k: block counter (r ceil(W / 4) + q, k, g, s), key (seed, 0)
__device__ __forceinline__ void ig_noise4(uint64_t seed, uint32_t s, uint32_t g, uint32_t k, uint64_t block, float z[4]) {
  const Philox4 p = philox4x64_10(block, (uint64_t)k, (uint64_t)g, (uint64_t)s, seed);
  box_muller(p.v[0], p.v[1], z[0], z[1]);
  box_muller(p.v[2], p.v[3], z[2], z[3]);
}

}  // namespace kgcn
