// qsc_philox.cuh — the counter-based generator of the draws (qsc_draw.hip) and of the keep rule
// (qsc_obs_select.hip): include/qsc.h has the arithmetic and the known answer.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

// the generator's key: the two halves of the ABI's 64-bit seed
struct SeedKey { uint32_t lo, hi; };
inline SeedKey split_seed(int64_t seed) {
  return {(uint32_t)((uint64_t)seed & 0xFFFFFFFFu), (uint32_t)((uint64_t)seed >> 32)};
}

// Philox4x32-10 (Salmon et al., SC'11): the first word of the output block
__device__ __forceinline__ uint32_t philox4x32_10_x0(uint32_t c0, uint32_t c1, uint32_t c2,
                                                     uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return c0;
}

}  // namespace
