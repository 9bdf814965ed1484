// Contact points of a batch: the all-pairs closest-pair search between the posed parts of every shape, in one launch.
//
// The reference never computes the `contact_points [B, P, P, 4]` table that `calc_connectivity_acc` consumes: it loads
// it from the PartNet release's files (multi_part_assembly/datasets/partnet_data.py:210-222).  The table is determined
// by what a batch carries — the canonical part clouds and the ground-truth poses — and include/mpa_hip.h defines it.
//
//   contact_kernel   one 256-thread block per (sample b, pair i <= j).  A diagonal block, or one with a padded member,
//                    writes its zeros / 1e32 / -1 and leaves without having read a point or a pose.  Otherwise both
//                    parts are posed with the inline functions of quat.h / mat3.h (the arithmetic of pose.hip / rmat.hip,
//                    so the coordinates are those of `pose_apply`) into LDS (24 N bytes, 48 KB at N = 2048; six blocks a CU
//                    at N = 1000).  Every thread then holds up to four queries of part i at a time and walks part j
//                    through wave-uniform (broadcast) LDS reads with the distance form of chamfer_core.h,
//                    d = (dx*dx + dy*dy) + dz*dz, every operation rounded.  Four targets make a chunk: their minimum is
//                    compared once with the query's running best (strict `<`, chunks in index order), and only the
//                    winning chunk of a query is evaluated again, after the walk, for the first target attaining the
//                    minimum — the same operations give the same bits, so this is the strict-`<` scan in index order.
//                    A thread meets its queries in increasing index order and keeps the first minimum; the block reduces
//                    (d, a, c) lexicographically on (d, a) — xor butterflies inside a wave, the four waves in LDS.
//   the prune        when neither min_dist nor index is requested only the flag is wanted.  The block then also reduces
//                    the two posed bounding boxes and evaluates the gap between them with the same rounded formula
//                    (per axis max(lo_j - hi_i, lo_i - hi_j, 0), then (gx*gx + gy*gy) + gz*gz).  fp32 subtraction,
//                    multiplication of non-negative values and addition are monotone, so the computed gap is a lower
//                    bound of every pair's COMPUTED d; a gap >= thre_sq therefore decides "no contact" exactly, and the
//                    walk is skipped.
//
// No atomics, no memset nodes, nothing read back on the host, a grid that depends on the sizes only: capturable, and
// bit-identical from run to run.
#include "chamfer_core.h"
#include "common.h"
#include "mat3.h"
#include "quat.h"

namespace {

using mpa::f32x2;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / mpa::kWave;
constexpr int kQ = 4;             // queries per thread and sweep of the other part
constexpr int kChunk = 4;         // targets per comparison: 12 floats = 3 broadcast ds_read_b128
constexpr int kMaxPoints = 2048;  // both posed parts in LDS: 24 * 2048 = 48 KB
constexpr int kMaxParts = 64;
constexpr float kFar = 1e32f;     // min_dist of the diagonal and of padded slots (chamfer_kernel.cu:60)

// Poses the N points of part slot m into `dst` (xyz interleaved); returns this thread's bounding box of what it wrote.
template <bool kRmat>
__device__ __forceinline__ void stage_part(const float* __restrict__ pcs, const float* __restrict__ rot,
                                           const float* __restrict__ trans, long long m, int N, float* __restrict__ dst,
                                           float* lo, float* hi) {
  const float* __restrict__ src = pcs + 3 * m * N;
  const float tr[3] = {trans[3 * m + 0], trans[3 * m + 1], trans[3 * m + 2]};
  mpa::Mat3 mat;
  mpa::Quat q{1.0f, 0.0f, 0.0f, 0.0f};
  if constexpr (kRmat) {
    mat = mpa::load_mat3(rot + 9 * m);
  } else {
    const float* r = rot + 4 * m;
    // Rotation3D's constructor rule (mpa_quat_sanitize): norm <= 0.5 (zero padding) -> identity
    if (__builtin_sqrtf(((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]) + r[3] * r[3]) > 0.5f) q = mpa::Quat{r[0], r[1], r[2], r[3]};
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    lo[k] = __builtin_inff();
    hi[k] = -__builtin_inff();
  }
  for (int i = threadIdx.x; i < N; i += kThreads) {
    const float px = src[3 * i + 0], py = src[3 * i + 1], pz = src[3 * i + 2];
    float o[3];
    if constexpr (kRmat) {
      mpa::mat3_rotate(mat, px, py, pz, o[0], o[1], o[2]);
    } else {
      mpa::quat_rotate(q, px, py, pz, o[0], o[1], o[2]);
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      o[k] = o[k] + tr[k];
      dst[3 * i + k] = o[k];
      lo[k] = o[k] < lo[k] ? o[k] : lo[k];
      hi[k] = o[k] > hi[k] ? o[k] : hi[k];
    }
  }
}

// The rows of a pair without a contact search: zeros in both rows (one row on the diagonal), 1e32 and -1 beside them.
__device__ __forceinline__ void write_empty(long long eij, long long eji, bool far_too, float* __restrict__ contact,
                                            float* __restrict__ min_dist, int* __restrict__ index) {
  const int t = threadIdx.x;
  if (t < 4) contact[4 * eij + t] = 0.0f;
  else if (t < 8 && eji != eij) contact[4 * eji + (t - 4)] = 0.0f;
  if (far_too && t == 8) {
    if (min_dist != nullptr) min_dist[eij] = min_dist[eji] = kFar;
    if (index != nullptr) index[eij] = index[eji] = -1;
  }
}

__device__ __forceinline__ bool before(float d1, int a1, float d2, int a2) { return d1 < d2 || (d1 == d2 && a1 < a2); }

template <bool kRmat>
__global__ __launch_bounds__(kThreads) void contact_kernel(const float* __restrict__ pcs, const float* __restrict__ valids,
                                                           const float* __restrict__ rot, const float* __restrict__ trans,
                                                           float thre_sq, int P, int N, int pairs,
                                                           float* __restrict__ contact, float* __restrict__ min_dist,
                                                           int* __restrict__ index) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  __shared__ float box[kWaves][12];
  __shared__ float red_d[kWaves];
  __shared__ int red_a[kWaves], red_c[kWaves];
  const long long b = blockIdx.x / pairs;
  int k = (int)(blockIdx.x - b * pairs);
  int i = 0;
  while (k >= P - i) {  // pair number -> (i, j = i + k), i <= j; at most P <= 64 steps, block-uniform
    k -= P - i;
    ++i;
  }
  const int j = i + k, t = threadIdx.x;
  const long long si = b * P + i, sj = b * P + j;
  const long long eij = si * P + j, eji = sj * P + i;
  if (i == j || valids[si] != 1.0f || valids[sj] != 1.0f) {  // nothing of a padded slot but its flag is read
    write_empty(eij, eji, true, contact, min_dist, index);
    return;
  }
  const int n3 = (3 * N + 3) & ~3;  // the second part starts 16-byte aligned
  float* __restrict__ ci = lds;
  float* __restrict__ cj = lds + n3;
  float bx[12];  // lo_i, hi_i, lo_j, hi_j
  stage_part<kRmat>(pcs, rot, trans, si, N, ci, bx + 0, bx + 3);
  stage_part<kRmat>(pcs, rot, trans, sj, N, cj, bx + 6, bx + 9);
  const bool flag_only = min_dist == nullptr && index == nullptr;
  if (flag_only) {
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
  if (flag_only) {
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
    if (mpa::dist_exact_f(g[0], g[1], g[2]) >= thre_sq) {  // block-uniform: every thread read the same LDS words
      write_empty(eij, eji, false, contact, min_dist, index);
      return;
    }
  }

  // ---- the walk: this thread's first minimum over its queries a = t, t + 256, ... of part i -------------------------------
  float my_d = __builtin_inff();
  int my_a = 0x7fffffff, my_c = 0;
  const float4* __restrict__ t4 = reinterpret_cast<const float4*>(cj);
  for (int base = 0; base < N; base += kQ * kThreads) {
    f32x2 X[kQ / 2], Y[kQ / 2], Z[kQ / 2], best[kQ / 2];
    int pos[kQ];
#pragma unroll
    for (int q = 0; q < kQ; ++q) {
      const int a = base + q * kThreads + t;
      const int aa = a < N ? a : 0;
      X[q >> 1][q & 1] = ci[3 * aa + 0];
      Y[q >> 1][q & 1] = ci[3 * aa + 1];
      Z[q >> 1][q & 1] = ci[3 * aa + 2];
      best[q >> 1][q & 1] = __builtin_inff();
      pos[q] = 0;
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
      const float sx = cj[3 * c + 0], sy = cj[3 * c + 1], sz = cj[3 * c + 2];
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
      const float d = best[q >> 1][q & 1];
      if (a < N && d < my_d) {  // strict: an earlier query of this thread keeps a tie
        const float x = X[q >> 1][q & 1], y = Y[q >> 1][q & 1], z = Z[q >> 1][q & 1];
        int cc = pos[q];
        const int end = cc + kChunk < N ? cc + kChunk : N;
        for (int e = cc; e < end; ++e) {  // the first target of the winning chunk that attains the minimum
          if (mpa::dist_exact_f(x - cj[3 * e + 0], y - cj[3 * e + 1], z - cj[3 * e + 2]) == d) {
            cc = e;
            break;
          }
        }
        my_d = d;
        my_a = a;
        my_c = cc;
      }
    }
  }
  if (my_a == 0x7fffffff && t < N) my_a = t;  // every distance of this thread overflowed to inf: its first query stands

  // ---- block reduction on (d, a), c carried along ------------------------------------------------------------------------------
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float od = __shfl_xor(my_d, off, 64);
    const int oa = __shfl_xor(my_a, off, 64), oc = __shfl_xor(my_c, off, 64);
    if (before(od, oa, my_d, my_a)) {
      my_d = od;
      my_a = oa;
      my_c = oc;
    }
  }
  if ((t & 63) == 0) {
    red_d[t >> 6] = my_d;
    red_a[t >> 6] = my_a;
    red_c[t >> 6] = my_c;
  }
  __syncthreads();
  if (t != 0) return;
#pragma unroll
  for (int w = 1; w < kWaves; ++w) {
    if (before(red_d[w], red_a[w], my_d, my_a)) {
      my_d = red_d[w];
      my_a = red_a[w];
      my_c = red_c[w];
    }
  }
  const bool touch = my_d < thre_sq;
  const float* __restrict__ pa = pcs + 3 * (si * N + my_a);  // canonical coordinates, copied as they are
  const float* __restrict__ pc = pcs + 3 * (sj * N + my_c);
  contact[4 * eij + 0] = touch ? 1.0f : 0.0f;
  contact[4 * eji + 0] = touch ? 1.0f : 0.0f;
#pragma unroll
  for (int e = 0; e < 3; ++e) {
    contact[4 * eij + 1 + e] = touch ? pa[e] : 0.0f;
    contact[4 * eji + 1 + e] = touch ? pc[e] : 0.0f;
  }
  if (min_dist != nullptr) min_dist[eij] = min_dist[eji] = my_d;
  if (index != nullptr) {
    index[eij] = my_a;
    index[eji] = my_c;
  }
}

template <bool kRmat>
int contact_table(const float* part_pcs, const float* valids, const float* rot, const float* trans, float thre_sq,
                   int64_t B, int64_t P, int64_t N, float* contact, float* min_dist, int32_t* index, void* stream,
                   const char* what) {
  MPA_REQUIRE(B >= 0, "%s: negative batch size", what);
  MPA_REQUIRE(P >= 1 && P <= kMaxParts, "%s: need 1 <= P <= %d part slots (P=%lld)", what, kMaxParts, (long long)P);
  MPA_REQUIRE(N >= 1 && N <= kMaxPoints, "%s: need 1 <= N <= %d points per part (N=%lld)", what, kMaxPoints, (long long)N);
  MPA_REQUIRE(B < (1LL << 31) && 4 * B * P * P < (1LL << 31), "%s: need 4 * B * P * P < 2^31", what);
  if (B == 0) return MPA_OK;
  MPA_REQUIRE(part_pcs && valids && rot && trans && contact, "%s: null pointer", what);
  const int64_t pairs = P * (P + 1) / 2;
  const size_t lds = 2 * sizeof(float) * (size_t)((3 * N + 3) & ~3LL);
  hipLaunchKernelGGL(contact_kernel<kRmat>, dim3((unsigned)(B * pairs)), dim3(kThreads), lds, mpa::as_stream(stream), part_pcs,
                     valids, rot, trans, thre_sq, (int)P, (int)N, (int)pairs, contact, min_dist, index);
  return mpa::check_launch(what);
}

}  // namespace

extern "C" int mpa_contact_points(const float* part_pcs, const float* valids, const float* quat, const float* trans,
                                  float thre_sq, int64_t B, int64_t P, int64_t N, float* contact_points,
                                  float* min_dist, int32_t* index, void* stream) {
  return contact_table<false>(part_pcs, valids, quat, trans, thre_sq, B, P, N, contact_points, min_dist, index, stream,
                               "contact_points");
}

extern "C" int mpa_contact_points_rmat(const float* part_pcs, const float* valids, const float* rmat, const float* trans,
                                       float thre_sq, int64_t B, int64_t P, int64_t N, float* contact_points,
                                       float* min_dist, int32_t* index, void* stream) {
  return contact_table<true>(part_pcs, valids, rmat, trans, thre_sq, B, P, N, contact_points, min_dist, index, stream,
                              "contact_points_rmat");
}
