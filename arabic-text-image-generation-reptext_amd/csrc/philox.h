// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11; Random123's constants) and the standard normals
// the stochastic master step draws from it (norm_elem.hip). Plain C++: the same text compiles for the host and the device.
//
// One call of philox4x32_10 gives four 32-bit words, which cover one group of four consecutive elements of a sample:
//   counter = (g low, g high, step, subsequence)      g = (index inside the sample) / 4
//   key     = (seed low, seed high ^ RT_PHILOX_DOMAIN)
// The value of an element is a function of (seed, subsequence, step, index inside the sample) and of nothing else: not of the batch,
// the grid, or which of the kernel's two paths reaches it. RT_PHILOX_DOMAIN keeps the stream apart from torch's own Philox stream for
// the same seed (torch keys with the seed as it is), which the initial latents come from.
//
// Words to normals (Box–Muller, accurate logf / sqrtf / sincospif):
//   u  = ((w >> 8) + 0.5)·2^-24      the sum is rounded to fp32 (to even) once w >> 8 reaches 2^23; u lies in [2^-25, 1]
//   z0 = r·cos θ,  z1 = r·sin θ      r = sqrt(−2 ln u(w0)),  θ = 2π·u(w1), taken as sincospi(2·u): the doubling is exact
//   z2, z3 the same from w2, w3
// |z| <= sqrt(2 ln 2^25) = 5.887; u = 1 gives r = 0, a finite draw.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RT_PHILOX_FN __host__ __device__ __forceinline__
#else
#include <math.h>
#define RT_PHILOX_FN static inline
#endif

#define RT_PHILOX_M0 0xD2511F53u
#define RT_PHILOX_M1 0xCD9E8D57u
#define RT_PHILOX_W0 0x9E3779B9u
#define RT_PHILOX_W1 0xBB67AE85u
#define RT_PHILOX_DOMAIN 0x53544F43u      // "STOC": XORed into the high key word

struct rt_philox4 { uint32_t w[4]; };

RT_PHILOX_FN rt_philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const uint64_t p0 = (uint64_t)RT_PHILOX_M0 * c0, p1 = (uint64_t)RT_PHILOX_M1 * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
    k0 += RT_PHILOX_W0; k1 += RT_PHILOX_W1;
  }
  return rt_philox4{{c0, c1, c2, c3}};
}

// the words of group g of a sample's stream at one step
RT_PHILOX_FN rt_philox4 philox_group(int64_t seed, int64_t subsequence, uint32_t step, uint64_t g) {
  return philox4x32_10((uint32_t)g, (uint32_t)(g >> 32), step, (uint32_t)subsequence, (uint32_t)(uint64_t)seed,
                       (uint32_t)((uint64_t)seed >> 32) ^ RT_PHILOX_DOMAIN);
}

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RT_PHILOX_DEV __device__ __forceinline__
RT_PHILOX_DEV float philox_uniform(uint32_t w) { return ((float)(w >> 8) + 0.5f) * 5.9604644775390625e-8f; }      // 2^-24

// the two normals of a pair of words; every product is a single rounding (nothing here can be fused)
RT_PHILOX_DEV void philox_normal_pair(uint32_t wa, uint32_t wb, float& za, float& zb) {
  const float r = sqrtf(-2.0f * logf(philox_uniform(wa)));
  float sn, cs;
  sincospif(2.0f * philox_uniform(wb), &sn, &cs);
  za = r * cs;
  zb = r * sn;
}

// the four normals of a group
RT_PHILOX_DEV void philox_normal4(const rt_philox4& p, float z[4]) {
  philox_normal_pair(p.w[0], p.w[1], z[0], z[1]);
  philox_normal_pair(p.w[2], p.w[3], z[2], z[3]);
}

// element ``lane`` (0..3) of a group alone: its pair's two normals by the same text, one of them picked — the bits of philox_normal4
RT_PHILOX_DEV float philox_normal_lane(const rt_philox4& p, int lane) {
  float za, zb;
  philox_normal_pair(p.w[lane & 2], p.w[(lane & 2) + 1], za, zb);
  return (lane & 1) ? zb : za;
}
#endif
