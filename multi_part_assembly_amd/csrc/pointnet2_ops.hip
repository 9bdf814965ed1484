// PointNet++ sampling and grouping operators: what the reference's CUDA-only `pointnet2_ops` extension provides to its
// set-abstraction modules (pointnet2_ops/_ext-src/src/sampling_gpu.cu, ball_query_gpu.cu, group_points_gpu.cu).
// include/mpa_hip.h has the definitions; multi_part_assembly_amd/pointnet2_ref.py restates them in numpy.
//
//   furthest point sampling  one block of 512 threads per cloud, npoint - 1 dependent rounds.  N <= 4096: every thread keeps
//     its <= 8 points and their running distances in registers, the coordinates also sit in LDS (SoA) so that the last
//     winner's are one broadcast read.  A candidate is ONE 64-bit integer, (bits of d2) << 32 | ~key, where key is the
//     reference's tie order (bit-reversed reference thread, then the order inside it): the round's winner is the maximum,
//     so the reference's answer comes out whatever block this kernel uses.  The maximum goes over the wave on the DPP
//     network and once through LDS (two slots, alternating, so one barrier per round).  Larger N: the same round over
//     global memory, the running distances in the caller's workspace.
//   ball query  one wave per centre, 64 candidates per step in ascending index: ballot + prefix pop-count hand out the
//     slots in index order, the walk stops when the row is full, the tail of the row is filled with the first hit.
//   grouping forward  a block stages a tile of (m, c) rows in LDS and stores coalesced along the (j, l) positions.
//   grouping backward  a per-cloud inverted index (for every source point the ascending list of the positions that name
//     it, built by one block with a stable counting placement; integer atomics for the counts only), then one block per
//     (m, c) row stages the gradient row in LDS and every thread adds its points' lists front to back: the order of
//     `np.add.at`, no floating-point atomics, bit-reproducible.
#include "common.h"
#include "pointnet2_index.h"  // group_index_kernel, carve_group: shared with pointnet2_interp.hip

namespace {

constexpr int kFpsThreads = 512;
constexpr int kFpsWaves = kFpsThreads / mpa::kWave;
constexpr int kFpsResident = 4096;  // points per cloud the register-resident kernel takes (8 per thread)

template <int kCtrl, int kRowMask, bool kBound>
__device__ __forceinline__ uint64_t dpp_u64(uint64_t v) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)v, kCtrl, kRowMask, 0xf, kBound);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(v >> 32), kCtrl, kRowMask, 0xf, kBound);
  return ((uint64_t)hi << 32) | lo;
}

__device__ __forceinline__ uint64_t max_u64(uint64_t a, uint64_t b) { return a > b ? a : b; }

// Maximum over the 64 lanes, returned to all of them: the steps of common.h's wave_sum_dpp (a lane that a step leaves
// out reads 0, the identity of an unsigned maximum as of a sum).
__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v) {
  v = max_u64(v, dpp_u64<0xB1, 0xf, true>(v));    // quad_perm [1,0,3,2]
  v = max_u64(v, dpp_u64<0x4E, 0xf, true>(v));    // quad_perm [2,3,0,1]
  v = max_u64(v, dpp_u64<0x141, 0xf, true>(v));   // row_half_mirror
  v = max_u64(v, dpp_u64<0x140, 0xf, true>(v));   // row_mirror
  v = max_u64(v, dpp_u64<0x142, 0xa, false>(v));  // row_bcast15 into rows 1, 3
  v = max_u64(v, dpp_u64<0x143, 0xc, false>(v));  // row_bcast31 into rows 2, 3
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, 63);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), 63);
  return ((uint64_t)hi << 32) | lo;
}

// The reference's tie order of point k under its block size T = 2^logT: (bit-reversed k mod T) << 22 | k div T.
__device__ __forceinline__ uint32_t fps_key(int k, int logT) {
  const uint32_t r = (uint32_t)k & ((1u << logT) - 1u);
  const uint32_t rev = logT == 0 ? 0u : __brev(r) >> (32 - logT);
  return (rev << 22) | ((uint32_t)k >> logT);
}

__device__ __forceinline__ int fps_point_of_key(uint32_t key, int logT) {
  const uint32_t rev = key >> 22;
  const uint32_t r = logT == 0 ? 0u : __brev(rev) >> (32 - logT);
  return (int)(((key & 0x3fffffu) << logT) | r);
}

// skipped by the reference: |p|^2 in float32, widened to double, <= 1e-3
__device__ __forceinline__ bool fps_live(float x, float y, float z) {
  const float mag = (x * x + y * y) + z * z;
  return !((double)mag <= 1e-3);
}

__device__ __forceinline__ uint64_t fps_candidate(float d2, uint32_t nkey) {
  return ((uint64_t)__float_as_uint(d2) << 32) | nkey;
}

// Block maximum of `best` -> the round's winner.  `red` has two rows of kFpsWaves slots; row j & 1 belongs to round j.
__device__ __forceinline__ int fps_block_winner(uint64_t best, uint64_t (*red)[kFpsWaves], int j, int logT) {
  best = wave_max_u64(best);
  if ((threadIdx.x & (mpa::kWave - 1)) == 0) red[j & 1][threadIdx.x / mpa::kWave] = best;
  __syncthreads();
  uint64_t w = red[j & 1][0];
#pragma unroll
  for (int u = 1; u < kFpsWaves; ++u) w = max_u64(w, red[j & 1][u]);
  return w == 0 ? 0 : fps_point_of_key(~(uint32_t)w, logT);  // 0: every point is skipped
}

template <int kPer>
__global__ __launch_bounds__(kFpsThreads) void fps_resident_kernel(const float* __restrict__ xyz, int N, int npoint,
                                                                   int logT, int32_t* __restrict__ idx) {
  __shared__ float sx[kPer * kFpsThreads], sy[kPer * kFpsThreads], sz[kPer * kFpsThreads];
  __shared__ uint64_t red[2][kFpsWaves];
  const int t = threadIdx.x;
  const float* p = xyz + (int64_t)blockIdx.x * N * 3;
  idx += (int64_t)blockIdx.x * npoint;
  float x[kPer], y[kPer], z[kPer], temp[kPer];
  uint32_t nkey[kPer];
  bool live[kPer];
#pragma unroll
  for (int u = 0; u < kPer; ++u) {
    const int k = t + u * kFpsThreads;
    const bool in = k < N;
    x[u] = in ? p[3 * k + 0] : 0.f;
    y[u] = in ? p[3 * k + 1] : 0.f;
    z[u] = in ? p[3 * k + 2] : 0.f;
    sx[k] = x[u];
    sy[k] = y[u];
    sz[k] = z[u];
    live[u] = in && fps_live(x[u], y[u], z[u]);
    nkey[u] = ~fps_key(k, logT);
    temp[u] = 1e10f;
  }
  if (t == 0) idx[0] = 0;
  __syncthreads();
  int old = 0;
  for (int j = 1; j < npoint; ++j) {
    const float x1 = sx[old], y1 = sy[old], z1 = sz[old];
    uint64_t best = 0;
#pragma unroll
    for (int u = 0; u < kPer; ++u) {
      const float dx = x[u] - x1, dy = y[u] - y1, dz = z[u] - z1;
      const float d = (dx * dx + dy * dy) + dz * dz;
      const float d2 = fminf(d, temp[u]);
      if (live[u]) {
        temp[u] = d2;
        best = max_u64(best, fps_candidate(d2, nkey[u]));
      }
    }
    old = fps_block_winner(best, red, j, logT);
    if (t == 0) idx[j] = old;
  }
}

// N > 4096: the reference's own mapping (T = 512, thread t owns the points k = t mod 512), distances in the workspace
__global__ __launch_bounds__(kFpsThreads) void fps_stream_kernel(const float* __restrict__ xyz, int N, int npoint,
                                                                 float* __restrict__ temp_all, int32_t* __restrict__ idx) {
  __shared__ uint64_t red[2][kFpsWaves];
  constexpr int logT = 9;
  const int t = threadIdx.x;
  const float* p = xyz + (int64_t)blockIdx.x * N * 3;
  float* temp = temp_all + (int64_t)blockIdx.x * N;
  idx += (int64_t)blockIdx.x * npoint;
  for (int k = t; k < N; k += kFpsThreads) temp[k] = 1e10f;  // read back by this thread only
  if (t == 0) idx[0] = 0;
  int old = 0;
  for (int j = 1; j < npoint; ++j) {
    const float x1 = p[3 * old + 0], y1 = p[3 * old + 1], z1 = p[3 * old + 2];
    uint64_t best = 0;
    for (int k = t; k < N; k += kFpsThreads) {
      const float x2 = p[3 * k + 0], y2 = p[3 * k + 1], z2 = p[3 * k + 2];
      if (!fps_live(x2, y2, z2)) continue;
      const float dx = x2 - x1, dy = y2 - y1, dz = z2 - z1;
      const float d = (dx * dx + dy * dy) + dz * dz;
      const float d2 = fminf(d, temp[k]);
      temp[k] = d2;
      best = max_u64(best, fps_candidate(d2, ~fps_key(k, logT)));
    }
    old = fps_block_winner(best, red, j, logT);
    if (t == 0) idx[j] = old;
  }
}

// ---- ball query ------------------------------------------------------------------------------------------------------------
constexpr int kBqThreads = 256;
constexpr int kBqWaves = kBqThreads / mpa::kWave;
constexpr int kBqCentres = 32;    // centres per block: the staged cloud is read 32 times
constexpr int kBqStaged = 4096;   // points per cloud that are staged in LDS (48 KiB)

template <bool kStaged>
__global__ __launch_bounds__(kBqThreads) void ball_query_kernel(const float* __restrict__ xyz,
                                                                const float* __restrict__ new_xyz, float r2, int N, int S,
                                                                int nsample, int blocks_per_cloud,
                                                                int32_t* __restrict__ idx) {
  extern __shared__ __attribute__((aligned(16))) float bq_lds[];
  const int t = threadIdx.x, lane = t & (mpa::kWave - 1), wave = t / mpa::kWave;
  const int m = blockIdx.x / blocks_per_cloud, j0 = (blockIdx.x % blocks_per_cloud) * kBqCentres;
  const float* p = xyz + (int64_t)m * N * 3;
  float *sx = bq_lds, *sy = bq_lds + N, *sz = bq_lds + 2 * N;
  if (kStaged) {
    for (int k = t; k < N; k += kBqThreads) {
      sx[k] = p[3 * k + 0];
      sy[k] = p[3 * k + 1];
      sz[k] = p[3 * k + 2];
    }
    __syncthreads();
  }
  for (int c = wave; c < kBqCentres; c += kBqWaves) {  // (no barrier below: a wave may leave early)
    const int j = j0 + c;
    if (j >= S) break;
    const float* q = new_xyz + ((int64_t)m * S + j) * 3;
    const float cx = q[0], cy = q[1], cz = q[2];
    int32_t* row = idx + ((int64_t)m * S + j) * nsample;
    int cnt = 0, first = 0;
    for (int base = 0; base < N && cnt < nsample; base += mpa::kWave) {
      const int k = base + lane;
      bool hit = false;
      if (k < N) {
        const float x = kStaged ? sx[k] : p[3 * k + 0];
        const float y = kStaged ? sy[k] : p[3 * k + 1];
        const float z = kStaged ? sz[k] : p[3 * k + 2];
        const float dx = cx - x, dy = cy - y, dz = cz - z;
        hit = ((dx * dx + dy * dy) + dz * dz) < r2;
      }
      const uint64_t mask = __ballot(hit);
      if (mask != 0) {
        if (cnt == 0) first = base + __ffsll((long long)mask) - 1;
        const int slot = cnt + __popcll(mask & ((1ull << lane) - 1ull));
        if (hit && slot < nsample) row[slot] = k;
        cnt += __popcll(mask);
      }
    }
    for (int s = (cnt < nsample ? cnt : nsample) + lane; s < nsample; s += mpa::kWave) row[s] = first;
  }
}

// ---- grouping --------------------------------------------------------------------------------------------------------------
constexpr int kGrpChunk = 8192;       // (j, l) positions per block
constexpr int kGrpTileFloats = 8192;  // LDS of a staged tile of feature rows (32 KiB)
constexpr int kGrpTileRows = 8;

template <bool kStaged>
__global__ __launch_bounds__(kGrpThreads) void group_forward_kernel(const float* __restrict__ feat,
                                                                   const int32_t* __restrict__ idx, int C, int N, int SK,
                                                                   int ct, int tiles, int chunks, float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) float grp_lds[];
  const int t = threadIdx.x;
  const int chunk = blockIdx.x % chunks, tile = (blockIdx.x / chunks) % tiles, m = blockIdx.x / chunks / tiles;
  const int c0 = tile * ct, nc = C - c0 < ct ? C - c0 : ct;
  const float* rows = feat + ((int64_t)m * C + c0) * N;
  if (kStaged) {
    for (int e = t; e < nc * N; e += kGrpThreads) grp_lds[e] = rows[e];
    __syncthreads();
  }
  const int p1 = SK - chunk * kGrpChunk < kGrpChunk ? SK : (chunk + 1) * kGrpChunk;
  const int32_t* ix = idx + (int64_t)m * SK;
  float* o = out + ((int64_t)m * C + c0) * SK;
  for (int p = chunk * kGrpChunk + t; p < p1; p += kGrpThreads) {
    const int i = ix[p];
    const bool ok = (unsigned)i < (unsigned)N;  // an index outside [0, N) is never dereferenced: it reads as 0
    for (int c = 0; c < nc; ++c) {
      float v = 0.f;
      if (ok) v = kStaged ? grp_lds[c * N + i] : rows[(int64_t)c * N + i];
      o[(int64_t)c * SK + p] = v;
    }
  }
}

// One block per (m, c) row: the gradient row goes through LDS a chunk at a time, every thread adds the lists of its
// points front to back (a list is ascending, so a chunk holds one contiguous piece of it).
__global__ __launch_bounds__(kGrpThreads) void group_backward_kernel(const float* __restrict__ grad_out,
                                                                    const int* __restrict__ start,
                                                                    const int* __restrict__ list, int C, int N, int SK,
                                                                    int Ns, int SKs, float* __restrict__ grad_feat) {
  extern __shared__ __attribute__((aligned(16))) float grp_lds[];
  const int t = threadIdx.x;
  const int m = blockIdx.x / C;
  const float* g = grad_out + (int64_t)blockIdx.x * SK;
  float* out = grad_feat + (int64_t)blockIdx.x * N;
  const int* st = start + (int64_t)m * Ns;
  const int* li = list + (int64_t)m * SKs;
  for (int c0 = 0; c0 < SK; c0 += kGrpChunk) {
    const int len = SK - c0 < kGrpChunk ? SK - c0 : kGrpChunk;
    for (int p = t; p < len; p += kGrpThreads) grp_lds[p] = g[c0 + p];
    __syncthreads();
    for (int k = t; k < N; k += kGrpThreads) {
      int lo = st[k];
      const int hi = st[k + 1];
      float acc = 0.f;
      if (c0 > 0) {
        acc = out[k];
        int a = lo, b = hi;  // first entry >= c0
        while (a < b) {
          const int mid = (a + b) >> 1;
          if (li[mid] < c0) a = mid + 1;
          else b = mid;
        }
        lo = a;
      }
      for (; lo < hi; ++lo) {
        const int p = li[lo] - c0;
        if (p >= len) break;
        acc += grp_lds[p];
      }
      out[k] = acc;
    }
    __syncthreads();  // the chunk has been read by every wave
  }
}

constexpr int64_t kInt31 = 1LL << 31;

float* carve_fps(mpa::Arena& a, int64_t M, int64_t N) { return a.take<float>(N > kFpsResident ? M * N : 0, 256); }

}  // namespace

extern "C" int mpa_furthest_point_sample_workspace(int64_t M, int64_t N, int64_t* bytes) {
  MPA_REQUIRE(bytes != nullptr, "furthest_point_sample_workspace: null pointer");
  MPA_REQUIRE(M >= 0 && N >= 0, "furthest_point_sample_workspace: negative size (M=%lld, N=%lld)", (long long)M,
              (long long)N);
  MPA_REQUIRE(M * N * 3 < kInt31, "furthest_point_sample_workspace: 3 M N = %lld must stay below 2^31",
              (long long)(M * N * 3));
  mpa::Arena a(nullptr);
  carve_fps(a, M, N);
  *bytes = a.bytes();
  return MPA_OK;
}

extern "C" int mpa_furthest_point_sample(const float* xyz, int64_t M, int64_t N, int64_t npoint, void* workspace,
                                         int32_t* idx, void* stream) {
  MPA_REQUIRE(M >= 0 && N >= 0 && npoint >= 0, "furthest_point_sample: negative size (M=%lld, N=%lld, npoint=%lld)",
              (long long)M, (long long)N, (long long)npoint);
  if (M == 0 || npoint == 0) return MPA_OK;
  MPA_REQUIRE(N >= 1, "furthest_point_sample: a cloud without points has no sample (N=0)");
  MPA_REQUIRE(M * N * 3 < kInt31 && M * npoint < kInt31,
              "furthest_point_sample: 3 M N = %lld and M npoint = %lld must stay below 2^31", (long long)(M * N * 3),
              (long long)(M * npoint));
  MPA_REQUIRE(xyz != nullptr && idx != nullptr, "furthest_point_sample: null pointer");
  mpa::Arena a(workspace);
  float* temp = carve_fps(a, M, N);
  MPA_REQUIRE(N <= kFpsResident || workspace != nullptr,
              "furthest_point_sample: null workspace (N=%lld needs mpa_furthest_point_sample_workspace bytes)", (long long)N);
  MPA_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 255u) == 0, "furthest_point_sample: workspace must be 256-byte aligned");
  int logT = 0;  // T = min(512, 2^floor(log2 N)), the reference's block size
  while (logT < 9 && (2LL << logT) <= N) ++logT;
  const dim3 grid((unsigned)M), block(kFpsThreads);
  hipStream_t s = mpa::as_stream(stream);
  if (N > kFpsResident) {
    hipLaunchKernelGGL(fps_stream_kernel, grid, block, 0, s, xyz, (int)N, (int)npoint, temp, idx);
  } else if (N <= kFpsThreads) {
    hipLaunchKernelGGL(fps_resident_kernel<1>, grid, block, 0, s, xyz, (int)N, (int)npoint, logT, idx);
  } else if (N <= 2 * kFpsThreads) {
    hipLaunchKernelGGL(fps_resident_kernel<2>, grid, block, 0, s, xyz, (int)N, (int)npoint, logT, idx);
  } else if (N <= 4 * kFpsThreads) {
    hipLaunchKernelGGL(fps_resident_kernel<4>, grid, block, 0, s, xyz, (int)N, (int)npoint, logT, idx);
  } else {
    hipLaunchKernelGGL(fps_resident_kernel<8>, grid, block, 0, s, xyz, (int)N, (int)npoint, logT, idx);
  }
  return mpa::check_launch("furthest_point_sample");
}

extern "C" int mpa_ball_query(const float* xyz, const float* new_xyz, float radius, int64_t M, int64_t N, int64_t S,
                              int64_t nsample, int32_t* idx, void* stream) {
  MPA_REQUIRE(M >= 0 && N >= 0 && S >= 0 && nsample >= 0, "ball_query: negative size (M=%lld, N=%lld, S=%lld, nsample=%lld)",
              (long long)M, (long long)N, (long long)S, (long long)nsample);
  if (M == 0 || S == 0 || nsample == 0) return MPA_OK;
  MPA_REQUIRE(M * N * 3 < kInt31 && M * S * nsample < kInt31 && M * ((S + kBqCentres - 1) / kBqCentres) < kInt31,
              "ball_query: 3 M N = %lld and M S nsample = %lld must stay below 2^31", (long long)(M * N * 3),
              (long long)(M * S * nsample));
  MPA_REQUIRE(new_xyz != nullptr && idx != nullptr && (xyz != nullptr || N == 0), "ball_query: null pointer");
  const float r2 = radius * radius;
  const int per_cloud = (int)((S + kBqCentres - 1) / kBqCentres);
  const dim3 grid((unsigned)(M * per_cloud)), block(kBqThreads);
  hipStream_t s = mpa::as_stream(stream);
  if (N <= kBqStaged)
    hipLaunchKernelGGL(ball_query_kernel<true>, grid, block, (size_t)(3 * N * sizeof(float)), s, xyz, new_xyz, r2, (int)N,
                       (int)S, (int)nsample, per_cloud, idx);
  else
    hipLaunchKernelGGL(ball_query_kernel<false>, grid, block, 0, s, xyz, new_xyz, r2, (int)N, (int)S, (int)nsample,
                       per_cloud, idx);
  return mpa::check_launch("ball_query");
}

extern "C" int mpa_group_points_forward(const float* features, const int32_t* idx, int64_t M, int64_t C, int64_t N,
                                        int64_t S, int64_t K, float* out, void* stream) {
  MPA_REQUIRE(M >= 0 && C >= 0 && N >= 0 && S >= 0 && K >= 0,
              "group_points_forward: negative size (M=%lld, C=%lld, N=%lld, S=%lld, K=%lld)", (long long)M, (long long)C,
              (long long)N, (long long)S, (long long)K);
  if (M == 0 || C == 0 || S == 0 || K == 0) return MPA_OK;
  MPA_REQUIRE(S * K < kInt31 && M * C < kInt31 && M * C * S * K < kInt31 && M * C * N < kInt31,
              "group_points_forward: M C S K = %lld and M C N = %lld must stay below 2^31", (long long)(M * C * S * K),
              (long long)(M * C * N));
  MPA_REQUIRE(idx != nullptr && out != nullptr && (features != nullptr || N == 0), "group_points_forward: null pointer");
  const int SK = (int)(S * K);
  const bool staged = N >= 1 && N <= kGrpTileFloats;
  int ct = staged ? (int)(kGrpTileFloats / N) : kGrpTileRows;
  ct = ct > kGrpTileRows ? kGrpTileRows : ct;
  const int tiles = (int)((C + ct - 1) / ct), chunks = (SK + kGrpChunk - 1) / kGrpChunk;
  MPA_REQUIRE(M * tiles * chunks < kInt31, "group_points_forward: too many blocks");
  const dim3 grid((unsigned)(M * tiles * chunks)), block(kGrpThreads);
  hipStream_t s = mpa::as_stream(stream);
  if (staged)
    hipLaunchKernelGGL(group_forward_kernel<true>, grid, block, (size_t)ct * N * sizeof(float), s, features, idx, (int)C,
                       (int)N, SK, ct, tiles, chunks, out);
  else
    hipLaunchKernelGGL(group_forward_kernel<false>, grid, block, 0, s, features, idx, (int)C, (int)N, SK, ct, tiles, chunks,
                       out);
  return mpa::check_launch("group_points_forward");
}

extern "C" int mpa_group_points_workspace(int64_t M, int64_t N, int64_t S, int64_t K, int64_t* bytes) {
  MPA_REQUIRE(bytes != nullptr, "group_points_workspace: null pointer");
  MPA_REQUIRE(M >= 0 && N >= 0 && S >= 0 && K >= 0, "group_points_workspace: negative size (M=%lld, N=%lld, S=%lld, K=%lld)",
              (long long)M, (long long)N, (long long)S, (long long)K);
  MPA_REQUIRE(S * K < kInt31 && M * (N + 64) < kInt31 && M * (S * K + 64) < kInt31,
              "group_points_workspace: M N = %lld and M S K = %lld must stay below 2^31", (long long)(M * N),
              (long long)(M * S * K));
  mpa::Arena a(nullptr);
  carve_group(a, M, N, S * K);
  *bytes = a.bytes();
  return MPA_OK;
}

extern "C" int mpa_group_points_backward(const float* grad_out, const int32_t* idx, int64_t M, int64_t C, int64_t N,
                                         int64_t S, int64_t K, void* workspace, float* grad_features, void* stream) {
  MPA_REQUIRE(M >= 0 && C >= 0 && N >= 0 && S >= 0 && K >= 0,
              "group_points_backward: negative size (M=%lld, C=%lld, N=%lld, S=%lld, K=%lld)", (long long)M, (long long)C,
              (long long)N, (long long)S, (long long)K);
  if (M == 0 || C == 0 || N == 0) return MPA_OK;
  MPA_REQUIRE(S * K < kInt31 && M * C < kInt31 && M * C * S * K < kInt31 && M * C * N < kInt31 && M * (N + 64) < kInt31 &&
                  M * (S * K + 64) < kInt31,
              "group_points_backward: M C S K = %lld and M C N = %lld must stay below 2^31", (long long)(M * C * S * K),
              (long long)(M * C * N));
  MPA_REQUIRE(grad_features != nullptr, "group_points_backward: null pointer");
  hipStream_t s = mpa::as_stream(stream);
  if (S == 0 || K == 0) {  // nothing contributes
    mpa::zero_words_async(grad_features, M * C * N, s);
    return mpa::check_launch("group_points_backward");
  }
  MPA_REQUIRE(grad_out != nullptr && idx != nullptr && workspace != nullptr, "group_points_backward: null pointer");
  MPA_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 255u) == 0, "group_points_backward: workspace must be 256-byte aligned");
  const int SK = (int)(S * K), Ns = round64(N + 1), SKs = round64(SK);
  mpa::Arena a(workspace);
  const GroupWorkspace w = carve_group(a, M, N, SK);
  hipLaunchKernelGGL(group_index_kernel, dim3((unsigned)M), dim3(kGrpThreads), 0, s, idx, (int)N, SK, Ns, SKs, w.start,
                     w.cursor, w.list);
  const size_t lds = (size_t)(SK < kGrpChunk ? SK : kGrpChunk) * sizeof(float);
  hipLaunchKernelGGL(group_backward_kernel, dim3((unsigned)(M * C)), dim3(kGrpThreads), lds, s, grad_out, w.start, w.list,
                     (int)C, (int)N, SK, Ns, SKs, grad_features);
  return mpa::check_launch("group_points_backward");
}
