// Repulsion loss of a batch: the Chamfer distance of every unordered pair of parts of a shape, hinged at `thre`
// (multi_part_assembly/utils/loss.py:205-225), without the two [B P P, N, 3] expansions of the composition.
//
//   loss_b = [nv thre + 2 sum_{i<j, both valid} max(0, thre - cd_ij)] / nv^2,   cd_ij = mean_n d1[n] + mean_m d2[m]
//
// include/mpa_hip.h defines the arithmetic; multi_part_assembly_amd/repulsion_ref.py restates it in numpy.
//
//   the pair kernel  one 256-thread block per (sample b, pair slot i < j).  A block with a padded member writes flag 0 and a
//                    zero hinge and leaves without having read a point (padded slots may hold NaN).  Otherwise both parts go
//                    to LDS (24 N bytes) as they are -- the operator takes posed points.  The block reduces the two bounding
//                    boxes and the gap g between them with the rounded formula of contact_points.hip (per axis
//                    max(lo_j - hi_i, lo_i - hi_j, 0), then (gx*gx + gy*gy) + gz*gz): fp32 subtraction, multiplication of
//                    non-negative values and addition are monotone, so g is a lower bound of every COMPUTED d of the pair.
//   the prune        g >= thre: the pair is not searched.  Every d >= g, so each of the two means is at least
//                    g (1 - N 2^-24) however its N <= 2048 terms are added, and cd >= 2 g (1 - N 2^-24) >= g >= thre: the
//                    factor of two is the margin over the rounding of the means.  thre - cd <= 0, the hinge is exactly
//                    zero and the pair carries no gradient: the prune never changes a result.  It is off when `cd` is
//                    requested (the caller wants the distance, not only the hinge).
//   the walk         both directions from the staged points, as contact_kernel walks: a thread holds up to four queries,
//                    the other part arrives through wave-uniform (broadcast) LDS reads, four targets make a chunk whose
//                    minimum is compared once with the query's running best (strict `<`, started at 1e32), and the winning
//                    chunk of every query is evaluated again for the first target attaining the minimum -- the same
//                    operations give the same bits, so (d, index) are those of mpa_chamfer_forward for the pair.
//   the means        a thread adds its distances in ascending query index, the 64 lanes of a wave in six xor-butterfly
//                    steps (32, 16, ..., 1), the four waves left to right: `ordered_sum` of repulsion_ref.py.
//   the finalize     a second launch of one block per sample adds the hinges in slot order and forms loss_b; it also writes
//                    the diagonal of cd.  Measured: 4.9 us per call in a kernel trace, under 1 % of the 0.6 - 1.05 ms
//                    forward at B = 32, P = 20, N = 1000.  The alternative, the last pair block of a sample behind a
//                    ticket, needs a counter that is zero before the call: in a caller-owned workspace that is a zeroing
//                    launch of the same cost, plus an atomic and a fence in every pair block.  The second launch stays.
//   the grad kernel  one block per (b, part i), over the partners j in ascending order whose pair is hinged.  Part j and the
//                    arg-min list of j's points go to LDS, where the block builds the list's inverted index as
//                    csrc/pointnet2_index.h does (counts by integer atomics, prefix sums, stable placement by rank inside
//                    tiles of 256).  A thread owns up to four points of part i at a time: it adds the term of its own
//                    minimum, then the minima of part j that land on the point, in ascending index.  No floating-point
//                    atomics, a fixed order of every sum.  (A first version walked the whole list per thread instead of
//                    building the index: 2.03 ms against 1.06 ms for the worst-case backward at B = 32, P = 20, N = 1000.)
//
// No atomics, no memset nodes, nothing read back on the host, grids that depend on the sizes only: capturable, and
// bit-identical from run to run.
#include "chamfer_core.h"
#include "common.h"

namespace {

using mpa::f32x2;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / mpa::kWave;
constexpr int kQ = 4;             // queries per thread and sweep of the other part
constexpr int kChunk = 4;         // targets per comparison: 12 floats = 3 broadcast ds_read_b128
constexpr int kMaxPoints = 2048;  // both parts in LDS: 24 * 2048 = 48 KB
constexpr int kMaxParts = 64;
constexpr float kFar = 1e32f;     // chamfer_kernel.cu:60
constexpr unsigned short kNone = 0xffff;  // index -1 in the 16-bit lists
constexpr unsigned char kNotSearched = 0, kSearched = 1, kHinged = 2;

struct Workspace {
  unsigned char* flag;    // [B, pairs]
  float* hinge;           // [B, pairs] max(0, thre - cd)
  unsigned short* idx1;   // [B, pairs, N] arg-min in part j of every point of part i
  unsigned short* idx2;   // [B, pairs, N] arg-min in part i of every point of part j
};
Workspace carve(mpa::Arena& a, int64_t B, int64_t P, int64_t N) {
  const int64_t slots = B * (P * (P - 1) / 2);
  Workspace w;
  w.flag = a.take<unsigned char>(slots, 256);
  w.hinge = a.take<float>(slots, 256);
  w.idx1 = a.take<unsigned short>(slots * N, 256);
  w.idx2 = a.take<unsigned short>(slots * N, 256);
  return w;
}

// Copies the N points of part slot m into `dst` (xyz interleaved); this thread's bounding box of what it copied.
__device__ __forceinline__ void stage_part(const float* __restrict__ pcs, long long m, int N, float* __restrict__ dst,
                                           float* lo, float* hi) {
  const float* __restrict__ src = pcs + 3 * m * N;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    lo[k] = __builtin_inff();
    hi[k] = -__builtin_inff();
  }
  for (int i = threadIdx.x; i < N; i += kThreads) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float o = src[3 * i + k];
      dst[3 * i + k] = o;
      lo[k] = o < lo[k] ? o : lo[k];
      hi[k] = o > hi[k] ? o : hi[k];
    }
  }
}

// Nearest target in `ct` of every point of `cq` (both in LDS, N points each): index list and, if asked, distances to
// global memory; returns this thread's sum of its queries' distances, added in ascending query index.
__device__ __forceinline__ float walk(const float* __restrict__ cq, const float* __restrict__ ct, int N,
                                      unsigned short* __restrict__ idx_out, float* __restrict__ dist_out) {
  const int t = threadIdx.x;
  float sum = 0.0f;
  const float4* __restrict__ t4 = reinterpret_cast<const float4*>(ct);
  for (int base = 0; base < N; base += kQ * kThreads) {
    f32x2 X[kQ / 2], Y[kQ / 2], Z[kQ / 2], best[kQ / 2];
    int pos[kQ];
#pragma unroll
    for (int q = 0; q < kQ; ++q) {
      const int a = base + q * kThreads + t;
      const int aa = a < N ? a : 0;
      X[q >> 1][q & 1] = cq[3 * aa + 0];
      Y[q >> 1][q & 1] = cq[3 * aa + 1];
      Z[q >> 1][q & 1] = cq[3 * aa + 2];
      best[q >> 1][q & 1] = kFar;
      pos[q] = -1;
    }
    int c = 0;
    for (; c + kChunk <= N; c += kChunk) {
      const float4 u = t4[3 * (c >> 2) + 0], v = t4[3 * (c >> 2) + 1], w = t4[3 * (c >> 2) + 2];
      const float tx[4] = {u.x, u.w, v.z, w.y}, ty[4] = {u.y, v.x, v.w, w.z}, tz[4] = {u.z, v.y, w.x, w.w};
#pragma unroll
      for (int h = 0; h < kQ / 2; ++h) {
        f32x2 m = mpa::dist_exact_v(X[h] - tx[0], Y[h] - ty[0], Z[h] - tz[0]);
#pragma unroll
        for (int e = 1; e < kChunk; ++e) {
          const f32x2 d = mpa::dist_exact_v(X[h] - tx[e], Y[h] - ty[e], Z[h] - tz[e]);
          m[0] = d[0] < m[0] ? d[0] : m[0];
          m[1] = d[1] < m[1] ? d[1] : m[1];
        }
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          const bool better = m[e] < best[h][e];
          best[h][e] = better ? m[e] : best[h][e];
          pos[2 * h + e] = better ? c : pos[2 * h + e];
        }
      }
    }
    for (; c < N; ++c) {  // the last N % 4 targets, one by one
      const float sx = ct[3 * c + 0], sy = ct[3 * c + 1], sz = ct[3 * c + 2];
#pragma unroll
      for (int h = 0; h < kQ / 2; ++h) {
        const f32x2 d = mpa::dist_exact_v(X[h] - sx, Y[h] - sy, Z[h] - sz);
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          const bool better = d[e] < best[h][e];
          best[h][e] = better ? d[e] : best[h][e];
          pos[2 * h + e] = better ? c : pos[2 * h + e];
        }
      }
    }
#pragma unroll
    for (int q = 0; q < kQ; ++q) {
      const int a = base + q * kThreads + t;
      if (a >= N) continue;
      const float d = best[q >> 1][q & 1];
      int cc = pos[q];  // -1: no target was closer than 1e32
      if (cc >= 0) {
        const float x = X[q >> 1][q & 1], y = Y[q >> 1][q & 1], z = Z[q >> 1][q & 1];
        const int end = cc + kChunk < N ? cc + kChunk : N;
        for (int e = cc; e < end; ++e) {  // the first target of the winning chunk that attains the minimum
          if (mpa::dist_exact_f(x - ct[3 * e + 0], y - ct[3 * e + 1], z - ct[3 * e + 2]) == d) {
            cc = e;
            break;
          }
        }
      }
      idx_out[a] = cc >= 0 ? (unsigned short)cc : kNone;
      if (dist_out != nullptr) dist_out[a] = d;
      sum = sum + d;
    }
  }
  return sum;
}

// `ordered_sum` of repulsion_ref.py over the threads' partial sums; the result in thread 0 (red: kWaves floats of LDS).
__device__ __forceinline__ float block_sum(float v, float* red) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = v + __shfl_xor(v, off, 64);
  __syncthreads();  // (red may still be read from the previous sum)
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float s = red[0];
#pragma unroll
  for (int w = 1; w < kWaves; ++w) s = s + red[w];
  return s;
}

__global__ __launch_bounds__(kThreads) void repulsion_pair_kernel(const float* __restrict__ pcs, const float* __restrict__ valids,
                                                        float thre, int P, int N, int pairs, bool prune,
                                                        unsigned char* __restrict__ flag, float* __restrict__ hinge,
                                                        unsigned short* __restrict__ idx1, unsigned short* __restrict__ idx2,
                                                        float* __restrict__ cd, float* __restrict__ dists) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  __shared__ float box[kWaves][12];
  __shared__ float red[kWaves];
  const long long b = blockIdx.x / pairs;
  int k = (int)(blockIdx.x - b * pairs);
  int i = 0;
  while (k >= P - 1 - i) {  // slot -> (i, j = i + 1 + k), i < j; at most P <= 64 steps, block-uniform
    k -= P - 1 - i;
    ++i;
  }
  const int j = i + 1 + k, t = threadIdx.x;
  const long long si = b * P + i, sj = b * P + j, slot = blockIdx.x;
  const long long eij = si * P + j, eji = sj * P + i;
  if (valids[si] != 1.0f || valids[sj] != 1.0f) {  // nothing of a padded slot but its flag is read
    if (t == 0) {
      flag[slot] = kNotSearched;
      hinge[slot] = 0.0f;
      if (cd != nullptr) cd[eij] = cd[eji] = 0.0f;
    }
    return;
  }
  const int n3 = (3 * N + 3) & ~3;  // the second part starts 16-byte aligned
  float* __restrict__ ci = lds;
  float* __restrict__ cj = lds + n3;
  float bx[12];  // lo_i, hi_i, lo_j, hi_j
  stage_part(pcs, si, N, ci, bx + 0, bx + 3);
  stage_part(pcs, sj, N, cj, bx + 6, bx + 9);
  if (prune) {
#pragma unroll
    for (int e = 0; e < 12; ++e) {
      const bool is_lo = (e / 3) % 2 == 0;
      float v = bx[e];
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        const float o = __shfl_xor(v, off, 64);
        v = is_lo ? (o < v ? o : v) : (o > v ? o : v);
      }
      if ((t & 63) == 0) box[t >> 6][e] = v;
    }
  }
  __syncthreads();
  if (prune) {
    float g[3];
#pragma unroll
    for (int e = 0; e < 3; ++e) {
      float lo_i = box[0][e], hi_i = box[0][3 + e], lo_j = box[0][6 + e], hi_j = box[0][9 + e];
#pragma unroll
      for (int w = 1; w < kWaves; ++w) {
        lo_i = box[w][e] < lo_i ? box[w][e] : lo_i;
        hi_i = box[w][3 + e] > hi_i ? box[w][3 + e] : hi_i;
        lo_j = box[w][6 + e] < lo_j ? box[w][6 + e] : lo_j;
        hi_j = box[w][9 + e] > hi_j ? box[w][9 + e] : hi_j;
      }
      const float g1 = lo_j - hi_i, g2 = lo_i - hi_j;  // at most one of them is positive
      const float m = g1 > g2 ? g1 : g2;
      g[e] = m > 0.0f ? m : 0.0f;
    }
    if (mpa::dist_exact_f(g[0], g[1], g[2]) >= thre) {  // block-uniform: every thread read the same LDS words
      if (t == 0) {
        flag[slot] = kNotSearched;
        hinge[slot] = 0.0f;
      }
      return;
    }
  }
  float* d1 = dists != nullptr ? dists + (2 * slot + 0) * N : nullptr;
  float* d2 = dists != nullptr ? dists + (2 * slot + 1) * N : nullptr;
  const float s1 = block_sum(walk(ci, cj, N, idx1 + slot * N, d1), red);
  const float s2 = block_sum(walk(cj, ci, N, idx2 + slot * N, d2), red);
  if (t != 0) return;
  const float c = s1 / (float)N + s2 / (float)N;
  const float h = thre - c;
  flag[slot] = h >= 0.0f ? kHinged : kSearched;  // (torch's clamp_min passes the gradient at equality)
  hinge[slot] = h > 0.0f ? h : 0.0f;
  if (cd != nullptr) cd[eij] = cd[eji] = c;
}

__global__ __launch_bounds__(kThreads) void repulsion_finalize_kernel(const float* __restrict__ valids, const float* __restrict__ hinge,
                                                            float thre, int P, int pairs, float* __restrict__ loss,
                                                            float* __restrict__ cd) {
  __shared__ float h[kMaxParts * (kMaxParts - 1) / 2];
  const long long b = blockIdx.x;
  const int t = threadIdx.x;
  for (int k = t; k < pairs; k += kThreads) h[k] = hinge[b * pairs + k];
  if (cd != nullptr && t < P) cd[(b * P + t) * P + t] = 0.0f;
  __syncthreads();
  if (t != 0) return;
  int nv = 0;
  for (int p = 0; p < P; ++p) nv += valids[b * P + p] == 1.0f ? 1 : 0;
  float s = 0.0f;
  for (int k = 0; k < pairs; ++k) s = s + h[k];  // slot order; the slots that were not searched hold zeros
  const float n = (float)nv;
  loss[b] = (n * thre + 2.0f * s) / (n * n);  // nv = 0: 0 / 0 = NaN, as the reference
}

__global__ __launch_bounds__(kThreads) void repulsion_grad_kernel(const float* __restrict__ grad_loss, const float* __restrict__ pcs,
                                                        const float* __restrict__ valids, int P, int N, int pairs,
                                                        const unsigned char* __restrict__ flag,
                                                        const unsigned short* __restrict__ idx1,
                                                        const unsigned short* __restrict__ idx2, float* __restrict__ grad) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const long long b = blockIdx.x / P;
  const int i = (int)(blockIdx.x - b * P), t = threadIdx.x;
  const long long si = b * P + i;
  const float* __restrict__ pi = pcs + 3 * si * N;
  float* __restrict__ out = grad + 3 * si * N;
  if (valids[si] != 1.0f) {  // nothing of a padded slot but its flag is read
    for (int e = t; e < 3 * N; e += kThreads) out[e] = 0.0f;
    return;
  }
  int nv = 0;
  for (int p = 0; p < P; ++p) nv += valids[b * P + p] == 1.0f ? 1 : 0;
  const float n = (float)nv;
  const float c = (-grad_loss[b] * 2.0f) / ((n * n) * (float)N);
  // LDS: part j; then, of the arg-min list of j's points (key[m] = the point of part i that m lands on), the inverted
  // index of csrc/pointnet2_index.h built in the block: start [N + 1], cursor [N] (the counts first), list [N]
  const int n3 = (3 * N + 3) & ~3, Nr = (N + kThreads - 1) & ~(kThreads - 1);
  float* __restrict__ cj = lds;
  int* __restrict__ key = reinterpret_cast<int*>(lds + n3);  // Nr entries, -1 past N and for "none"
  int* __restrict__ start = key + Nr;                          // N + 1 (Nr + 4 reserved)
  int* __restrict__ cursor = start + Nr + 4;
  int* __restrict__ list = cursor + Nr;
  __shared__ int part[kThreads];
  const int per = (N + kThreads - 1) / kThreads;
  const int k0 = t * per < N ? t * per : N, k1 = k0 + per < N ? k0 + per : N;
  for (int base = 0; base < N; base += kQ * kThreads) {
    float a[kQ][3], acc[kQ][3];
#pragma unroll
    for (int q = 0; q < kQ; ++q) {
      const int m = base + q * kThreads + t;
#pragma unroll
      for (int e = 0; e < 3; ++e) {
        a[q][e] = m < N ? pi[3 * m + e] : 0.0f;
        acc[q][e] = 0.0f;
      }
    }
    for (int j = 0; j < P; ++j) {
      if (j == i) continue;
      const int lo = i < j ? i : j, hi = i < j ? j : i;
      const long long slot = b * pairs + (lo * (2 * P - lo - 1) / 2 + (hi - lo - 1));
      if (flag[slot] != kHinged) continue;  // block-uniform
      const unsigned short* __restrict__ own = (i < j ? idx1 : idx2) + slot * N;
      const unsigned short* __restrict__ other = (i < j ? idx2 : idx1) + slot * N;
      const float* __restrict__ pj = pcs + 3 * (b * P + j) * N;
      __syncthreads();  // the previous partner's LDS has been read
      for (int e = t; e < 3 * N; e += kThreads) cj[e] = pj[e];
      for (int m = t; m < Nr; m += kThreads) {
        const int v = m < N ? (int)other[m] : (int)kNone;
        key[m] = v < N ? v : -1;
        cursor[m] = 0;
      }
      __syncthreads();
      for (int m = t; m < N; m += kThreads) {  // counts (integer LDS atomics: the order does not matter)
        const int v = key[m];
        if (v >= 0) atomicAdd(&cursor[v], 1);
      }
      __syncthreads();
      int sum = 0;
      for (int k = k0; k < k1; ++k) sum += cursor[k];
      part[t] = sum;
      __syncthreads();
      if (t < mpa::kWave) {  // exclusive prefix of the 256 partial counts, by the first wave: four per lane, a lane scan
        const int p0 = part[4 * t + 0], p1 = part[4 * t + 1], p2 = part[4 * t + 2], p3 = part[4 * t + 3];
        const int mine4 = ((p0 + p1) + p2) + p3;
        int incl = mine4;
#pragma unroll
        for (int off = 1; off < mpa::kWave; off <<= 1) {
          const int o = __shfl_up(incl, off, mpa::kWave);
          if (t >= off) incl += o;
        }
        const int excl = incl - mine4;
        part[4 * t + 0] = excl;
        part[4 * t + 1] = excl + p0;
        part[4 * t + 2] = excl + p0 + p1;
        part[4 * t + 3] = excl + p0 + p1 + p2;
        if (t == mpa::kWave - 1) start[N] = incl;
      }
      __syncthreads();
      int run = part[t];
      for (int k = k0; k < k1; ++k) {
        const int cnt = cursor[k];
        start[k] = run;
        cursor[k] = run;
        run += cnt;
      }
      __syncthreads();
      // stable placement, 256 positions at a time: a position's rank among the equal keys before it in the tile, on top
      // of the key's cursor; the last of a key in the tile moves the cursor on (csrc/pointnet2_index.h)
      for (int tile0 = 0; tile0 < N; tile0 += kThreads) {
        const int mk = key[tile0 + t];  // (-1 past N)
        int rank = 0, later = 0;
        const int4* __restrict__ tile4 = reinterpret_cast<const int4*>(key + tile0);
#pragma unroll 4
        for (int u = 0; u < kThreads; u += 4) {
          const int4 w = tile4[u >> 2];
          rank += (w.x == mk && u + 0 < t) + (w.y == mk && u + 1 < t) + (w.z == mk && u + 2 < t) + (w.w == mk && u + 3 < t);
          later += (w.x == mk && u + 0 > t) + (w.y == mk && u + 1 > t) + (w.z == mk && u + 2 > t) + (w.w == mk && u + 3 > t);
        }
        if (mk >= 0) list[cursor[mk] + rank] = tile0 + t;
        __syncthreads();  // every cursor of this tile has been read
        if (mk >= 0 && later == 0) cursor[mk] += rank + 1;
        __syncthreads();
      }
#pragma unroll
      for (int q = 0; q < kQ; ++q) {
        const int m = base + q * kThreads + t;
        if (m >= N) continue;
        const int o = (int)own[m];
        if (o < N) {  // this point's own minimum
#pragma unroll
          for (int e = 0; e < 3; ++e) acc[q][e] = acc[q][e] + c * (2.0f * (a[q][e] - cj[3 * o + e]));
        }
        const int p1 = start[m + 1];
        for (int p = start[m]; p < p1; ++p) {  // the minima of part j that land on it, in ascending index
          const int l = list[p];
#pragma unroll
          for (int e = 0; e < 3; ++e) acc[q][e] = acc[q][e] + c * (2.0f * (a[q][e] - cj[3 * l + e]));
        }
      }
    }
#pragma unroll
    for (int q = 0; q < kQ; ++q) {
      const int m = base + q * kThreads + t;
      if (m < N) {
#pragma unroll
        for (int e = 0; e < 3; ++e) out[3 * m + e] = acc[q][e];
      }
    }
  }
}

int check_sizes(int64_t B, int64_t P, int64_t N, const char* what) {
  MPA_REQUIRE(B >= 0, "%s: negative batch size", what);
  MPA_REQUIRE(P >= 1 && P <= kMaxParts, "%s: need 1 <= P <= %d part slots (P=%lld)", what, kMaxParts, (long long)P);
  MPA_REQUIRE(N >= 1 && N <= kMaxPoints, "%s: need 1 <= N <= %d points per part (N=%lld)", what, kMaxPoints, (long long)N);
  MPA_REQUIRE(B < (1LL << 31) && B * P * P * N < (1LL << 31), "%s: need B * P * P * N < 2^31", what);
  return MPA_OK;
}

}  // namespace

extern "C" int mpa_repulsion_cd_workspace(int64_t B, int64_t P, int64_t N, int64_t* bytes, int64_t* flag_offset,
                                          int64_t* idx1_offset, int64_t* idx2_offset) {
  if (const int st = check_sizes(B, P, N, "repulsion_cd_workspace")) return st;
  MPA_REQUIRE(bytes != nullptr, "repulsion_cd_workspace: null pointer");
  char* const origin = reinterpret_cast<char*>(256);  // any aligned non-null base: the offsets are differences
  mpa::Arena a(origin);
  const Workspace w = carve(a, B, P, N);
  *bytes = a.bytes();
  if (flag_offset) *flag_offset = reinterpret_cast<char*>(w.flag) - origin;
  if (idx1_offset) *idx1_offset = reinterpret_cast<char*>(w.idx1) - origin;
  if (idx2_offset) *idx2_offset = reinterpret_cast<char*>(w.idx2) - origin;
  return MPA_OK;
}

extern "C" int mpa_repulsion_cd_forward(const float* part_pcs, const float* valids, float thre, int64_t B, int64_t P,
                                        int64_t N, void* workspace, float* loss, float* cd, float* dists, void* stream) {
  const char* what = "repulsion_cd_forward";
  if (const int st = check_sizes(B, P, N, what)) return st;
  if (B == 0) return MPA_OK;
  MPA_REQUIRE(part_pcs && valids && loss, "%s: null pointer", what);
  const int64_t pairs = P * (P - 1) / 2;
  MPA_REQUIRE(workspace != nullptr || pairs == 0, "%s: null workspace", what);
  mpa::Arena arena(workspace);
  const Workspace w = carve(arena, B, P, N);
  hipStream_t s = mpa::as_stream(stream);
  if (pairs > 0) {
    const size_t lds = 2 * sizeof(float) * (size_t)((3 * N + 3) & ~3LL);
    hipLaunchKernelGGL(repulsion_pair_kernel, dim3((unsigned)(B * pairs)), dim3(kThreads), lds, s, part_pcs, valids, thre, (int)P,
                       (int)N, (int)pairs, cd == nullptr, w.flag, w.hinge, w.idx1, w.idx2, cd, dists);
    if (const int st = mpa::check_launch(what)) return st;
  }
  hipLaunchKernelGGL(repulsion_finalize_kernel, dim3((unsigned)B), dim3(kThreads), 0, s, valids, w.hinge, thre, (int)P, (int)pairs,
                     loss, cd);
  return mpa::check_launch(what);
}

extern "C" int mpa_repulsion_cd_backward(const float* grad_loss, const float* part_pcs, const float* valids, int64_t B,
                                         int64_t P, int64_t N, const void* workspace, float* grad_pcs, void* stream) {
  const char* what = "repulsion_cd_backward";
  if (const int st = check_sizes(B, P, N, what)) return st;
  if (B == 0) return MPA_OK;
  MPA_REQUIRE(grad_loss && part_pcs && valids && grad_pcs, "%s: null pointer", what);
  const int64_t pairs = P * (P - 1) / 2;
  MPA_REQUIRE(workspace != nullptr || pairs == 0, "%s: null workspace", what);
  mpa::Arena arena(const_cast<void*>(workspace));
  const Workspace w = carve(arena, B, P, N);
  const int64_t Nr = (N + kThreads - 1) / kThreads * kThreads;  // grad_kernel's carve: part j, key, start, cursor, list
  const size_t lds = sizeof(float) * (size_t)((3 * N + 3) & ~3LL) + sizeof(int) * (size_t)(4 * Nr + 4);
  hipLaunchKernelGGL(repulsion_grad_kernel, dim3((unsigned)(B * P)), dim3(kThreads), lds, mpa::as_stream(stream), grad_loss, part_pcs,
                     valids, (int)P, (int)N, (int)pairs, w.flag, w.idx1, w.idx2, grad_pcs);
  return mpa::check_launch(what);
}
