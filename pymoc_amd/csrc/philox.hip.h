// philox.hip.h -- the Gaussian deviate xi(seed, id, j, stream) of include/pymoc_hip.h: the one
// definition noise.hip (K18) and surrogates.hip (K24) share.  Philox4x32-10 keyed by the seed and
// counted by the four coordinates, then the first Box-Muller half (the second stays unused).  Its
// host restatement is tests/noise_cases.py: deviate; tests/test_noise_gpu.py pins the bits.
#pragma once
#include "common.hip.h"

namespace pm {

__device__ __forceinline__ void philox_round(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
  const uint32_t hi0 = __umulhi(0xD2511F53u, c[0]), lo0 = 0xD2511F53u * c[0];
  const uint32_t hi1 = __umulhi(0xCD9E8D57u, c[2]), lo1 = 0xCD9E8D57u * c[2];
  c[0] = hi1 ^ c[1] ^ k0;
  c[1] = lo1;
  c[2] = hi0 ^ c[3] ^ k1;
  c[3] = lo0;
}

// xi(seed, id, j, stream) of include/pymoc_hip.h
__device__ __forceinline__ double noise_deviate(uint32_t key0, uint32_t key1, uint64_t id,
                                                uint32_t j, uint32_t stream) {
  uint32_t c[4] = {(uint32_t)id, (uint32_t)(id >> 32), j, stream};
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    philox_round(c, key0, key1);
    key0 += 0x9E3779B9u;
    key1 += 0xBB67AE85u;
  }
  const double d1 = ((double)(c[0] >> 5) * 67108864.0 + (double)(c[1] >> 6)) * 0x1p-53;
  const double d2 = ((double)(c[2] >> 5) * 67108864.0 + (double)(c[3] >> 6)) * 0x1p-53;
  const double R = sqrt(-2.0 * log(1.0 - d1));
  return R * cos(6.283185307179586 * d2);
}

}  // namespace pm
