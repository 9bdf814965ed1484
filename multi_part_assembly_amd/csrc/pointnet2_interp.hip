// PointNet++ feature propagation operators: what the reference's CUDA-only `pointnet2_ops` extension provides to its
// `PointnetFPModule` (pointnet2_ops/_ext-src/src/interpolate_gpu.cu: three_nn, three_interpolate, three_interpolate_grad).
// include/mpa_hip.h has the definitions; multi_part_assembly_amd/pointnet2_ref.py restates them in numpy.
//
//   three_nn  a block takes 256 unknown points of one cloud, one per lane, and keeps each point's three running bests in
//     registers.  The known cloud goes through LDS in ascending tiles of 512 points, padded to 16 bytes: every lane reads
//     the same address (a broadcast, one ds_read_b128 per point), four points per trip so that their distances are
//     independent work in front of the dependent insertions.  Tiles ascend and are walked front to back: the scan order
//     of the definition, whatever m.  The kernel takes the square root itself.
//   three_interpolate forward  a block stages a tile of feature rows in LDS and walks a run of unknown points, one per
//     thread: three indices and weights once, then every staged channel; stores coalesced along the points.
//   three_interpolate backward  the per-cloud inverted index of pointnet2_index.h over the 3 n flat positions 3 j + k
//     (grouping's, with K = 3), then a block per (cloud, 8 channels) stages the gradient rows in LDS and every thread adds
//     the list of a (channel, known point) pair front to back, each term times its weight: the order of `np.add.at`, no
//     floating-point atomics, bit-reproducible.
#include "common.h"
#include "pointnet2_index.h"

#include <math.h>

namespace {

// ---- three_nn ----------------------------------------------------------------------------------------------------------
constexpr int kNnThreads = 256;
constexpr int kNnTile = 512;  // known points per LDS tile (8 KiB)
constexpr int kNnUnroll = 4;

// The strict `<` cascade best1 / best2 / best3.  b1 <= b2 <= b3 holds throughout, so d < b1 implies d < b2 implies
// d < b3 and the three tests select the branch of the cascade; a NaN d fails all three.
__device__ __forceinline__ void nn_insert(float d, int k, float& b1, float& b2, float& b3, int& i1, int& i2, int& i3) {
  const bool l1 = d < b1, l2 = d < b2, l3 = d < b3;
  b3 = l2 ? b2 : (l3 ? d : b3);
  i3 = l2 ? i2 : (l3 ? k : i3);
  b2 = l1 ? b1 : (l2 ? d : b2);
  i2 = l1 ? i1 : (l2 ? k : i2);
  b1 = l1 ? d : b1;
  i1 = l1 ? k : i1;
}

__global__ __launch_bounds__(kNnThreads) void three_nn_kernel(const float* __restrict__ unknown,
                                                              const float* __restrict__ known, int n, int m,
                                                              int blocks_per_cloud, float* __restrict__ dist,
                                                              int32_t* __restrict__ idx) {
  __shared__ float4 tile[kNnTile];
  const int t = threadIdx.x;
  const int b = blockIdx.x / blocks_per_cloud, j = (blockIdx.x % blocks_per_cloud) * kNnThreads + t;
  const float* kn = known + (int64_t)b * m * 3;
  const float* u = unknown + ((int64_t)b * n + (j < n ? j : n - 1)) * 3;  // a lane past the cloud repeats its last point
  const float ux = u[0], uy = u[1], uz = u[2];
  float b1 = INFINITY, b2 = INFINITY, b3 = INFINITY;
  int i1 = 0, i2 = 0, i3 = 0;
  for (int base = 0; base < m; base += kNnTile) {
    const int len = m - base < kNnTile ? m - base : kNnTile;
    __syncthreads();  // the tile before has been read by every wave
    for (int e = t; e < 3 * len; e += kNnThreads)
      reinterpret_cast<float*>(tile)[(e / 3) * 4 + e % 3] = kn[(int64_t)base * 3 + e];
    __syncthreads();
    int e = 0;
    for (; e + kNnUnroll <= len; e += kNnUnroll) {
      float d[kNnUnroll];
#pragma unroll
      for (int q = 0; q < kNnUnroll; ++q) {
        const float4 p = tile[e + q];
        const float dx = ux - p.x, dy = uy - p.y, dz = uz - p.z;
        d[q] = (dx * dx + dy * dy) + dz * dz;
      }
#pragma unroll
      for (int q = 0; q < kNnUnroll; ++q) nn_insert(d[q], base + e + q, b1, b2, b3, i1, i2, i3);
    }
    for (; e < len; ++e) {
      const float4 p = tile[e];
      const float dx = ux - p.x, dy = uy - p.y, dz = uz - p.z;
      nn_insert((dx * dx + dy * dy) + dz * dz, base + e, b1, b2, b3, i1, i2, i3);
    }
  }
  if (j < n) {
    float* dr = dist + ((int64_t)b * n + j) * 3;
    int32_t* ir = idx + ((int64_t)b * n + j) * 3;
    dr[0] = sqrtf(b1);
    dr[1] = sqrtf(b2);
    dr[2] = sqrtf(b3);
    ir[0] = i1;
    ir[1] = i2;
    ir[2] = i3;
  }
}

// ---- three_interpolate ---------------------------------------------------------------------------------------------------
constexpr int kIpThreads = 256;
constexpr int kIpChunk = 1024;       // unknown points per block
constexpr int kIpTileFloats = 8192;  // LDS of a staged tile of feature rows (32 KiB)
constexpr int kIpTileRows = 8;

template <bool kStaged>
__global__ __launch_bounds__(kIpThreads) void three_interpolate_forward_kernel(const float* __restrict__ feat,
                                                                               const int32_t* __restrict__ idx,
                                                                               const float* __restrict__ weight, int C,
                                                                               int m, int n, int ct, int tiles, int chunks,
                                                                               float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) float ip_lds[];
  const int t = threadIdx.x;
  const int chunk = blockIdx.x % chunks, tile = (blockIdx.x / chunks) % tiles, b = blockIdx.x / chunks / tiles;
  const int c0 = tile * ct, nc = C - c0 < ct ? C - c0 : ct;
  const float* rows = feat + ((int64_t)b * C + c0) * m;
  if (kStaged) {
    for (int e = t; e < nc * m; e += kIpThreads) ip_lds[e] = rows[e];
    __syncthreads();
  }
  const int j1 = n - chunk * kIpChunk < kIpChunk ? n : (chunk + 1) * kIpChunk;
  float* o = out + ((int64_t)b * C + c0) * n;
  for (int j = chunk * kIpChunk + t; j < j1; j += kIpThreads) {
    const int32_t* ix = idx + ((int64_t)b * n + j) * 3;
    const float* w = weight + ((int64_t)b * n + j) * 3;
    const int k1 = ix[0], k2 = ix[1], k3 = ix[2];
    const float w1 = w[0], w2 = w[1], w3 = w[2];
    // an index outside [0, m) is never dereferenced: it reads as 0
    const bool ok1 = (unsigned)k1 < (unsigned)m, ok2 = (unsigned)k2 < (unsigned)m, ok3 = (unsigned)k3 < (unsigned)m;
    for (int c = 0; c < nc; ++c) {
      float f1 = 0.f, f2 = 0.f, f3 = 0.f;
      if (kStaged) {
        if (ok1) f1 = ip_lds[c * m + k1];
        if (ok2) f2 = ip_lds[c * m + k2];
        if (ok3) f3 = ip_lds[c * m + k3];
      } else {
        if (ok1) f1 = rows[(int64_t)c * m + k1];
        if (ok2) f2 = rows[(int64_t)c * m + k2];
        if (ok3) f3 = rows[(int64_t)c * m + k3];
      }
      o[(int64_t)c * n + j] = (f1 * w1 + f2 * w2) + f3 * w3;
    }
  }
}

constexpr int kIbThreads = 256;
constexpr int kIbRows = 8;       // channels per block
constexpr int kIbChunk = 1024;   // unknown points whose gradients are staged at a time (8 rows: 32 KiB)

// One block per (cloud, tile of channels): the gradient rows go through LDS a chunk of unknown points at a time; a thread
// takes (channel, known point) pairs and adds the point's list front to back (ascending positions 3 j + k, so a chunk
// holds one contiguous piece of it), every term the gradient of its unknown point times the position's weight.
__global__ __launch_bounds__(kIbThreads) void three_interpolate_backward_kernel(
    const float* __restrict__ grad_out, const float* __restrict__ weight, const int* __restrict__ start,
    const int* __restrict__ list, int C, int n, int m, int ms, int ps, int tiles, float* __restrict__ grad_feat) {
  extern __shared__ __attribute__((aligned(16))) float ib_lds[];
  const int t = threadIdx.x;
  const int tile = blockIdx.x % tiles, b = blockIdx.x / tiles;
  const int c0 = tile * kIbRows, nc = C - c0 < kIbRows ? C - c0 : kIbRows;
  const float* g = grad_out + ((int64_t)b * C + c0) * n;
  float* out = grad_feat + ((int64_t)b * C + c0) * m;
  const float* w = weight + (int64_t)b * n * 3;
  const int* st = start + (int64_t)b * ms;
  const int* li = list + (int64_t)b * ps;
  for (int j0 = 0; j0 < n; j0 += kIbChunk) {
    const int len = n - j0 < kIbChunk ? n - j0 : kIbChunk;
    for (int e = t; e < nc * len; e += kIbThreads) ib_lds[e] = g[(int64_t)(e / len) * n + j0 + e % len];
    __syncthreads();
    const int p0 = 3 * j0, p1 = 3 * (j0 + len);
    for (int e = t; e < nc * m; e += kIbThreads) {
      const int c = e / m, k = e % m;
      int lo = st[k];
      const int hi = st[k + 1];
      float acc = 0.f;
      if (j0 > 0) {
        acc = out[(int64_t)c * m + k];
        int a = lo, z = hi;  // first entry >= p0
        while (a < z) {
          const int mid = (a + z) >> 1;
          if (li[mid] < p0) a = mid + 1;
          else z = mid;
        }
        lo = a;
      }
      const float* row = ib_lds + c * len;
      for (; lo < hi; ++lo) {
        const int p = li[lo];
        if (p >= p1) break;
        acc += row[p / 3 - j0] * w[p];
      }
      out[(int64_t)c * m + k] = acc;
    }
    __syncthreads();  // the chunk has been read by every wave
  }
}

constexpr int64_t kInt31 = 1LL << 31;

}  // namespace

extern "C" int mpa_three_nn(const float* unknown, const float* known, int64_t M, int64_t n, int64_t m, float* dist,
                            int32_t* idx, void* stream) {
  MPA_REQUIRE(M >= 0 && n >= 0 && m >= 0, "three_nn: negative size (M=%lld, n=%lld, m=%lld)", (long long)M, (long long)n,
              (long long)m);
  if (M == 0) return MPA_OK;
  MPA_REQUIRE(n >= 1 && m >= 1, "three_nn: a cloud without points has no neighbours (n=%lld, m=%lld)", (long long)n,
              (long long)m);
  MPA_REQUIRE(M * n * 3 < kInt31 && M * m * 3 < kInt31, "three_nn: 3 M n = %lld and 3 M m = %lld must stay below 2^31",
              (long long)(M * n * 3), (long long)(M * m * 3));
  MPA_REQUIRE(unknown != nullptr && known != nullptr && dist != nullptr && idx != nullptr, "three_nn: null pointer");
  const int per_cloud = (int)((n + kNnThreads - 1) / kNnThreads);
  hipLaunchKernelGGL(three_nn_kernel, dim3((unsigned)(M * per_cloud)), dim3(kNnThreads), 0, mpa::as_stream(stream), unknown,
                     known, (int)n, (int)m, per_cloud, dist, idx);
  return mpa::check_launch("three_nn");
}

extern "C" int mpa_three_interpolate_forward(const float* features, const int32_t* idx, const float* weight, int64_t M,
                                             int64_t C, int64_t m, int64_t n, float* out, void* stream) {
  MPA_REQUIRE(M >= 0 && C >= 0 && m >= 0 && n >= 0, "three_interpolate_forward: negative size (M=%lld, C=%lld, m=%lld, n=%lld)",
              (long long)M, (long long)C, (long long)m, (long long)n);
  if (M == 0 || C == 0 || n == 0) return MPA_OK;
  MPA_REQUIRE(M * C < kInt31 && M * C * n < kInt31 && M * C * m < kInt31 && M * n * 3 < kInt31,
              "three_interpolate_forward: M C n = %lld, M C m = %lld and 3 M n = %lld must stay below 2^31",
              (long long)(M * C * n), (long long)(M * C * m), (long long)(M * n * 3));
  MPA_REQUIRE(idx != nullptr && weight != nullptr && out != nullptr && (features != nullptr || m == 0),
              "three_interpolate_forward: null pointer");
  const bool staged = m >= 1 && m <= kIpTileFloats;
  int ct = staged ? (int)(kIpTileFloats / m) : kIpTileRows;
  ct = ct > kIpTileRows ? kIpTileRows : ct;
  const int tiles = (int)((C + ct - 1) / ct), chunks = (int)((n + kIpChunk - 1) / kIpChunk);
  MPA_REQUIRE(M * tiles * chunks < kInt31, "three_interpolate_forward: too many blocks");
  const dim3 grid((unsigned)(M * tiles * chunks)), block(kIpThreads);
  hipStream_t s = mpa::as_stream(stream);
  if (staged)
    hipLaunchKernelGGL(three_interpolate_forward_kernel<true>, grid, block, (size_t)ct * m * sizeof(float), s, features, idx,
                       weight, (int)C, (int)m, (int)n, ct, tiles, chunks, out);
  else
    hipLaunchKernelGGL(three_interpolate_forward_kernel<false>, grid, block, 0, s, features, idx, weight, (int)C, (int)m,
                       (int)n, ct, tiles, chunks, out);
  return mpa::check_launch("three_interpolate_forward");
}

extern "C" int mpa_three_interpolate_workspace(int64_t M, int64_t n, int64_t m, int64_t* bytes) {
  MPA_REQUIRE(bytes != nullptr, "three_interpolate_workspace: null pointer");
  MPA_REQUIRE(M >= 0 && n >= 0 && m >= 0, "three_interpolate_workspace: negative size (M=%lld, n=%lld, m=%lld)",
              (long long)M, (long long)n, (long long)m);
  MPA_REQUIRE(n * 3 < kInt31 && M * (m + 64) < kInt31 && M * (n * 3 + 64) < kInt31,
              "three_interpolate_workspace: M m = %lld and 3 M n = %lld must stay below 2^31", (long long)(M * m),
              (long long)(M * n * 3));
  mpa::Arena a(nullptr);
  carve_group(a, M, m, n * 3);
  *bytes = a.bytes();
  return MPA_OK;
}

extern "C" int mpa_three_interpolate_backward(const float* grad_out, const int32_t* idx, const float* weight, int64_t M,
                                              int64_t C, int64_t n, int64_t m, void* workspace, float* grad_features,
                                              void* stream) {
  MPA_REQUIRE(M >= 0 && C >= 0 && n >= 0 && m >= 0, "three_interpolate_backward: negative size (M=%lld, C=%lld, n=%lld, m=%lld)",
              (long long)M, (long long)C, (long long)n, (long long)m);
  if (M == 0 || C == 0 || m == 0) return MPA_OK;
  MPA_REQUIRE(n * 3 < kInt31 && M * C < kInt31 && M * C * n < kInt31 && M * C * m < kInt31 && M * (m + 64) < kInt31 &&
                  M * (n * 3 + 64) < kInt31,
              "three_interpolate_backward: M C n = %lld, M C m = %lld and 3 M n = %lld must stay below 2^31",
              (long long)(M * C * n), (long long)(M * C * m), (long long)(M * n * 3));
  MPA_REQUIRE(grad_features != nullptr, "three_interpolate_backward: null pointer");
  hipStream_t s = mpa::as_stream(stream);
  if (n == 0) {  // nothing contributes
    mpa::zero_words_async(grad_features, M * C * m, s);
    return mpa::check_launch("three_interpolate_backward");
  }
  MPA_REQUIRE(grad_out != nullptr && idx != nullptr && weight != nullptr && workspace != nullptr,
              "three_interpolate_backward: null pointer");
  MPA_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 255u) == 0,
              "three_interpolate_backward: workspace must be 256-byte aligned");
  const int P = (int)(n * 3), ms = round64(m + 1), ps = round64(P);
  mpa::Arena a(workspace);
  const GroupWorkspace w = carve_group(a, M, m, P);
  hipLaunchKernelGGL(group_index_kernel, dim3((unsigned)M), dim3(kGrpThreads), 0, s, idx, (int)m, P, ms, ps, w.start,
                     w.cursor, w.list);
  const int tiles = (int)((C + kIbRows - 1) / kIbRows);
  const size_t lds = (size_t)kIbRows * (size_t)(n < kIbChunk ? n : kIbChunk) * sizeof(float);
  hipLaunchKernelGGL(three_interpolate_backward_kernel, dim3((unsigned)(M * tiles)), dim3(kIbThreads), lds, s, grad_out, weight,
                     w.start, w.list, (int)C, (int)n, (int)m, ms, ps, tiles, grad_features);
  return mpa::check_launch("three_interpolate_backward");
}
