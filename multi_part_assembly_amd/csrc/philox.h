// Philox4x32-10 (Salmon et al., SC'11; the Random123 constants): the stateless generator behind every device-side draw of
// the library (csrc/mesh_sample.hip, csrc/match_sample.hip).  The counter / key layouts of the users are fixed in
// include/mpa_hip.h; they never overlap, so equal seeds give unrelated streams.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mpa {

struct U4 {
  uint32_t x, y, z, w;
};

__device__ __forceinline__ U4 philox4x32_10(U4 c, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c.x, p1 = (uint64_t)0xCD9E8D57u * c.z;
    c = U4{(uint32_t)(p1 >> 32) ^ c.y ^ k0, (uint32_t)p1, (uint32_t)(p0 >> 32) ^ c.w ^ k1, (uint32_t)p0};
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return c;
}

}  // namespace mpa
