// Device-side draw of the point sub-samples of the GT <-> prediction matching (semantic datasets).
//
// The reference draws `torch.randperm(N)[:n]` on the host for every existing group of every sample, in every one of the
// `sample_iter` loss evaluations of a step (multi_part_assembly/models/modules/base_model.py:163): a device sync for the
// group ids, B * groups Python calls, a pinned copy back.  Here one launch fills sample_idx [B, G, n] for all B * G group
// slots: row (b, g) = the first n entries of a uniformly random permutation of 0..N-1, by a partial Fisher-Yates shuffle
// on Philox4x32-10 words (the layout is fixed in include/mpa_hip.h).  One wave per slot: the 64 lanes fill iota(N) in LDS
// (it never exists in global memory) and draw the <= 32 Philox blocks, one lane walks the n dependent swaps (two LDS
// reads and one write each: position k is never read again, so its value goes straight to the output row).
#include "common.h"
#include "philox.h"

namespace {

constexpr int kMaxDraw = 128;        // n: kMaxN of csrc/match.hip
constexpr int kMaxPoints = 16384;    // N: iota(N) as 16-bit words is 32 KiB of LDS
constexpr uint32_t kPurpose = 0x6D610000u;  // counter word 1 = kPurpose | block: never one of the mesh sampler's 0..3

__global__ __launch_bounds__(64) void match_sample_kernel(int N, int n, uint32_t k0, uint32_t k1, uint64_t counter,
                                                          const uint64_t* __restrict__ counter_dev, uint64_t salt,
                                                          int* __restrict__ sample_idx) {
  __shared__ uint16_t perm[kMaxPoints];
  __shared__ uint32_t w[kMaxDraw];
  const int t = threadIdx.x;
  const uint32_t slot = blockIdx.x;
  const uint64_t c = (counter_dev != nullptr ? *counter_dev : counter) + salt;
  for (int i = t; i < N; i += 64) perm[i] = (uint16_t)i;
  if (4 * t < n) {
    const mpa::U4 r = mpa::philox4x32_10(mpa::U4{slot, kPurpose | (uint32_t)t, (uint32_t)c, (uint32_t)(c >> 32)}, k0, k1);
    w[4 * t + 0] = r.x;
    w[4 * t + 1] = r.y;
    w[4 * t + 2] = r.z;
    w[4 * t + 3] = r.w;
  }
  __syncthreads();
  if (t == 0) {
    for (int k = 0; k < n; ++k) {
      const int j = k + (int)__umulhi(w[k], (uint32_t)(N - k));  // k <= j < N
      const uint16_t a = perm[k], b = perm[j];
      perm[j] = a;
      w[k] = b;  // perm[k] = b: no later step reads position k
    }
  }
  __syncthreads();
  for (int k = t; k < n; k += 64) sample_idx[(long long)slot * n + k] = (int)w[k];
}

}  // namespace

extern "C" int mpa_match_sample_indices(int64_t B, int64_t G, int64_t N, int64_t n, uint64_t seed, uint64_t counter,
                                        const uint64_t* counter_dev, uint64_t salt, int32_t* sample_idx, void* stream) {
  MPA_REQUIRE(B >= 0 && G >= 1 && B * G <= (1LL << 24), "match_sample_indices: B=%lld G=%lld out of range (B >= 0, G >= 1, "
              "B * G <= 2^24)", (long long)B, (long long)G);
  MPA_REQUIRE(N >= 1 && N <= kMaxPoints, "match_sample_indices: N=%lld outside [1, %d] (the permutation lives in LDS)",
              (long long)N, kMaxPoints);
  MPA_REQUIRE(n >= 1 && n <= kMaxDraw && n <= N, "match_sample_indices: n=%lld outside [1, min(N, %d)]", (long long)n,
              kMaxDraw);
  if (B == 0) return MPA_OK;
  MPA_REQUIRE(sample_idx != nullptr, "match_sample_indices: null pointer");
  hipLaunchKernelGGL(match_sample_kernel, dim3((unsigned)(B * G)), dim3(64), 0, mpa::as_stream(stream), (int)N, (int)n,
                     (uint32_t)seed, (uint32_t)(seed >> 32), counter, counter_dev, salt, sample_idx);
  return mpa::check_launch("match_sample_indices");
}
