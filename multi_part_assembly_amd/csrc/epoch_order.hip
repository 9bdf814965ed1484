// The sample order of an epoch, drawn and sharded on the device: what `DistributedSampler(shuffle=True)` +
// `torch.randperm` do on the host in the reference's loaders (multi_part_assembly/datasets/geometry_data.py:226-248).
// include/mpa_hip.h has the definition; multi_part_assembly_amd/sampler_ref.py restates it in numpy.
//
// Two launches on the caller's stream:
//   1. epoch_keys_kernel: key_i = one Philox4x32-10 block per shape -> workspace [S] uint64.
//   2. epoch_rank_kernel: thread i counts rank_i = #{j : (key_j, j) < (key_i, i)} against key tiles staged in LDS (every
//      lane reads the same LDS address: a broadcast, no bank conflict) and writes i to where position rank_i of the padded,
//      strided order lands in this rank's shard.  A stable argsort by counting: S^2 comparisons, every output entry
//      written exactly once by exactly one thread, no atomics, nothing that depends on the dispatch order.
// A tile that lies wholly below (above) the block's own indices needs `<=` (`<`) on the key alone; only the tile that
// overlaps them compares the index too.
#include "common.h"
#include "philox.h"

namespace {

constexpr int kThreads = 256;
constexpr int kTile = 1024;                  // keys per LDS tile: 8 KiB
constexpr int64_t kMaxShapes = 1LL << 18;    // S^2 = 6.9e10 comparisons at the cap: a few milliseconds, once per epoch
constexpr uint32_t kPurpose = 0x65700000u;   // counter word 1: the mesh sampler's is < 4, the match sampler's 0x6D61xxxx,
                                             // the PartNet gather's 0x706Exxxx

__global__ __launch_bounds__(kThreads) void epoch_keys_kernel(int S, uint32_t k0, uint32_t k1, int64_t epoch,
                                                              const int64_t* __restrict__ epoch_dev,
                                                              uint64_t* __restrict__ keys) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= S) return;
  const uint64_t e = (uint64_t)(epoch_dev != nullptr ? *epoch_dev : epoch);
  const mpa::U4 r = mpa::philox4x32_10(mpa::U4{(uint32_t)i, kPurpose, (uint32_t)e, (uint32_t)(e >> 32)}, k0, k1);
  keys[i] = (uint64_t)r.x | ((uint64_t)r.y << 32);
}

// 0: every j of the tile is below every i of the block; 1: above; 2: they overlap
template <int kMode>
__device__ __forceinline__ int count_tile(const uint64_t* tile, int n, int j0, uint64_t ki, int i) {
  int cnt = 0;
#pragma unroll 8
  for (int j = 0; j < n; ++j) {
    const uint64_t kj = tile[j];
    if (kMode == 0) cnt += kj <= ki ? 1 : 0;
    else if (kMode == 1) cnt += kj < ki ? 1 : 0;
    else cnt += (kj < ki || (kj == ki && j0 + j < i)) ? 1 : 0;
  }
  return cnt;
}

__global__ __launch_bounds__(kThreads) void epoch_rank_kernel(int S, int64_t world, int64_t rank, int64_t total,
                                                              const uint64_t* __restrict__ keys,
                                                              int64_t* __restrict__ out) {
  __shared__ __align__(16) uint64_t tile[kTile];
  const int t = threadIdx.x, i0 = blockIdx.x * kThreads, i = i0 + t;
  const bool live = i < S;
  const uint64_t ki = live ? keys[i] : 0;
  int cnt = 0;
  for (int j0 = 0; j0 < S; j0 += kTile) {
    const int n = S - j0 < kTile ? S - j0 : kTile;
    __syncthreads();  // the previous tile has been read by every wave
    for (int j = t; j < n; j += kThreads) tile[j] = keys[j0 + j];
    __syncthreads();
    if (j0 + n <= i0) cnt += count_tile<0>(tile, n, j0, ki, i);
    else if (j0 >= i0 + kThreads) cnt += count_tile<1>(tile, n, j0, ki, i);
    else cnt += count_tile<2>(tile, n, j0, ki, i);
  }
  if (!live) return;
  // position cnt of the permutation; the padded order repeats it from the start (padded[q] = perm[q mod S]), and rank r
  // owns the positions q with q mod world == r, as entry q / world of its shard
  for (int64_t q = cnt; q < total; q += S)
    if (q % world == rank) out[q / world] = i;
}

}  // namespace

extern "C" int mpa_epoch_order_workspace(int64_t S, int64_t* bytes) {
  MPA_REQUIRE(bytes != nullptr, "epoch_order_workspace: null pointer");
  MPA_REQUIRE(S >= 1, "epoch_order_workspace: S=%lld must be positive", (long long)S);
  MPA_REQUIRE(S <= kMaxShapes, "epoch_order_workspace: S=%lld above the supported maximum %lld", (long long)S,
              (long long)kMaxShapes);
  *bytes = 8 * S;
  return MPA_OK;
}

extern "C" int mpa_epoch_order(int64_t S, int64_t world, int64_t rank, uint64_t seed, int64_t epoch,
                               const int64_t* epoch_dev, void* workspace, int64_t* out, void* stream) {
  MPA_REQUIRE(S >= 1, "epoch_order: S=%lld must be positive", (long long)S);
  MPA_REQUIRE(world >= 1 && world <= (1LL << 20), "epoch_order: world=%lld outside [1, 2^20]", (long long)world);
  MPA_REQUIRE(rank >= 0 && rank < world, "epoch_order: rank=%lld outside [0, %lld)", (long long)rank, (long long)world);
  MPA_REQUIRE(S <= kMaxShapes, "epoch_order: S=%lld above the supported maximum %lld", (long long)S,
              (long long)kMaxShapes);
  MPA_REQUIRE(workspace != nullptr && out != nullptr, "epoch_order: null pointer (workspace and out are always needed)");
  MPA_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7u) == 0, "epoch_order: workspace must be 8-byte aligned");
  const int64_t total = (S + world - 1) / world * world;
  const dim3 grid((unsigned)((S + kThreads - 1) / kThreads));
  uint64_t* keys = static_cast<uint64_t*>(workspace);
  hipLaunchKernelGGL(epoch_keys_kernel, grid, dim3(kThreads), 0, mpa::as_stream(stream), (int)S, (uint32_t)seed,
                     (uint32_t)(seed >> 32), epoch, epoch_dev, keys);
  hipLaunchKernelGGL(epoch_rank_kernel, grid, dim3(kThreads), 0, mpa::as_stream(stream), (int)S, world, rank, total,
                     keys, out);
  return mpa::check_launch("epoch_order");
}
