// PointNet part encoder — forward and backward (training-mode BatchNorm) for gfx950.
//
// Replaces the torch module of the reference (multi_part_assembly/models/modules/encoder/pointnet.py:6-41):
// 5 x [1x1 Conv1d (no bias) -> BatchNorm1d -> ReLU (none after the last)] 3-64-64-64-128-F, max over the
// N points of each part; and the compaction around it (models/pn_transformer/network.py:59-68): the
// kernels take ALL B*P part slots plus the validity mask and simply skip padded parts, so launch
// shapes are static and no device->host sync is needed.
//
// Design:
//   * fp32 tensors (parity bar 1e-4).  The 1x1 convolutions conv2..conv5 are GEMMs over [points x channels] and run
//     on the bf16 matrix cores, fp32-grade: both operands split into three bf16 terms, six products of order <= 2
//     (csrc/dg_gemm_split.h has the error analysis).  Forward: pn_fwd_ws.h; backward: pn_bwd_q.h.  Both are
//     wave-specialised persistent kernels (stager, matrix-product and store / epilogue waves, one barrier per unit).
//   * activations are point-major  [row = part*N + point][channel].
//   * BatchNorm+ReLU of layer l-1 is applied on the fly wherever layer l needs its input (forward GEMM,
//     weight-gradient GEMM): only the pre-BatchNorm outputs Y_l are ever stored; the
//     per-channel sums BatchNorm needs fall out of the accumulator layout (a lane holds 16 rows of
//     one output channel) and are reduced in a fixed order: deterministic, no atomics.
//   * backward: BatchNorm backward is the per-channel affine map dY = alpha*dZ + gamma'*Y + beta'
//     (coefficients from two column sums); with Y = A W^T both gradients are written without Y (the Q form,
//     pn_bwd_q.h), and the per-block partial tables are summed by a second deterministic stage.  The 3-channel
//     first layer uses scalar-operand VALU panels (weights through the scalar cache), K = 3 being far too thin
//     for a matrix core.
#include <type_traits>

#include "common.h"
#include "coop_reduce.h"

namespace {

constexpr int kT = 256;      // threads per block (4 waves)
using mpa::CoopWs;
using mpa::coop_colsum;
using mpa::kEB;
using mpa::kSlices;

typedef float f32x16 __attribute__((ext_vector_type(16)));

// MFMA 32x32 accumulator layout: lane l holds column (l & 31) and, in register r, row acc_row(r, l >> 5).
__device__ __forceinline__ int acc_row(int reg, int half) { return (reg & 3) + 8 * (reg >> 2) + 4 * half; }

// Per-layer BatchNorm parameters, struct-of-arrays [4][C]: scale, shift, mean, invstd
//   z = y * scale + shift  ==  gamma * (y - mean) * invstd + beta
// Backward coefficients [3][C]: alpha, gammap, betap  with  dY = alpha*dZ + gammap*Y + betap.

// ---- small kernels ---------------------------------------------------------------------------------------
// number of valid points (BatchNorm's sample count), the compact list of valid parts (vlist[0] = how many, part
// ids from vlist[4] on, ascending) that the persistent backward kernels walk, and the reset of the tickets.
// one block of 1024 threads.
__global__ __launch_bounds__(1024) void pn_count_kernel(const float* __restrict__ valids, int M, int N,
                                                        float* __restrict__ count, unsigned* __restrict__ ticket,
                                                        int* __restrict__ vlist, const float* __restrict__ w1 = nullptr,
                                                        float* __restrict__ wt1 = nullptr) {
  __shared__ int wcnt[16];
  if (threadIdx.x < 4) ticket[threadIdx.x] = 0u;  // the cooperative reductions' counters (reset after every use)
  // (the first layer's 64 x 3 weights transposed for the kernels that recompute that layer: rode in its own launch before)
  if (w1 != nullptr && threadIdx.x < 192) wt1[(threadIdx.x % 3) * 64 + threadIdx.x / 3] = w1[threadIdx.x];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  int base = 0;
  for (int m0 = 0; m0 < M; m0 += 1024) {
    const int m = m0 + threadIdx.x;
    const bool ok = m < M && valids[m] != 0.0f;
    const unsigned long long b = __ballot(ok);
    if (lane == 0) wcnt[wave] = __popcll(b);
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const int c = wcnt[k];
      before += k < wave ? c : 0;
      total += c;
    }
    if (ok) vlist[4 + base + before + __popcll(b & ((1ull << lane) - 1ull))] = m;
    base += total;
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    count[0] = (float)base * (float)N;
    vlist[0] = base;
  }
}

// the (sum0, sum1) partial tables written by the forward / input-gradient kernels; rows of padded parts hold
// garbage and are skipped (valids == nullptr: one row per persistent block, all of them meaningful)
__device__ __forceinline__ bool reduce_partials(const float* __restrict__ partial,
                                                const float* __restrict__ valids, int M, int splits, int C,
                                                int c, const CoopWs ws, double& s0, double& s1) {
  return coop_colsum(M * splits, C, c, ws,
                     [&](int e, bool& ok, double& x, double& y) {
                       const float2 v = *reinterpret_cast<const float2*>(partial + ((long long)e * C + c) * 2);
                       ok = valids == nullptr || valids[e / splits] != 0.0f;
                       x = (double)v.x;
                       y = (double)v.y;
                     },
                     s0, s1);
}

// BatchNorm statistics -> scale/shift (+ running statistics).  grid = (C/64, ceil(M*splits/kEB)), block 1024.
__global__ __launch_bounds__(64 * kSlices) void pn_bn_finalize_kernel(
    const float* __restrict__ partial, const float* __restrict__ valids, int M, int splits, int C,
    const float* __restrict__ count, const float* __restrict__ gamma, const float* __restrict__ beta,
    float* __restrict__ running_mean, float* __restrict__ running_var, float momentum, float eps,
    float* __restrict__ bn, const CoopWs cw) {
  const int c = blockIdx.x * 64 + (threadIdx.x & 63);
  double s, ss;
  if (!reduce_partials(partial, valids, M, splits, C, c, cw, s, ss)) return;
  if (threadIdx.x >= 64) return;
  const double n = (double)count[0];
  if (n == 0.0) {  // no valid part in the whole call (the reference's BatchNorm would refuse an empty batch): a neutral
    bn[c] = 0.0f;  // map, running statistics untouched — every output row is a padded part's zero row anyway, and the
    bn[C + c] = beta[c];  // backward pass then produces zero gradients instead of 0 / 0
    bn[2 * C + c] = 0.0f;
    bn[3 * C + c] = 0.0f;
    return;
  }
  const double mean = s / n;
  double var = ss / n - mean * mean;  // biased: what BatchNorm normalises with
  if (var < 0.0) var = 0.0;
  const float invstd = (float)(1.0 / __builtin_sqrt(var + (double)eps));
  const float scale = gamma[c] * invstd;
  bn[c] = scale;
  bn[C + c] = beta[c] - (float)mean * scale;
  bn[2 * C + c] = (float)mean;
  bn[3 * C + c] = invstd;
  if (running_mean != nullptr) {  // running_var tracks the unbiased estimate
    const double unbiased = n > 1.0 ? var * n / (n - 1.0) : var;
    running_mean[c] = (1.0f - momentum) * running_mean[c] + momentum * (float)mean;
    running_var[c] = (1.0f - momentum) * running_var[c] + momentum * (float)unbiased;
  }
}

// eval mode: scale/shift from the running statistics
__global__ void pn_bn_from_running_kernel(int C, const float* __restrict__ gamma,
                                          const float* __restrict__ beta,
                                          const float* __restrict__ running_mean,
                                          const float* __restrict__ running_var, float eps,
                                          float* __restrict__ bn) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  if (c >= C) return;
  const float invstd = 1.0f / __builtin_sqrtf(running_var[c] + eps);
  const float scale = gamma[c] * invstd;
  bn[c] = scale;
  bn[C + c] = beta[c] - running_mean[c] * scale;
  bn[2 * C + c] = running_mean[c];
  bn[3 * C + c] = invstd;
}

__device__ __forceinline__ void write_coef(float* __restrict__ coef, int C, int c, float gamma,
                                           const float* __restrict__ bn, double s1, double s2, double n) {
  const float mean = bn[2 * C + c], invstd = bn[3 * C + c];
  const float alpha = gamma * invstd;
  if (n == 0.0) {  // no valid part: nothing to differentiate
    coef[c] = coef[C + c] = coef[2 * C + c] = 0.0f;
    return;
  }
  const float gammap = (float)(-(double)alpha * s2 / n * (double)invstd);
  coef[c] = alpha;
  coef[C + c] = gammap;
  coef[2 * C + c] = (float)(-(double)alpha * s1 / n - (double)gammap * (double)mean);
}

// coefficients of layer l from the (s1, s2) partials written by the input-gradient kernel of layer l+1
__global__ __launch_bounds__(64 * kSlices) void pn_bwd_coef_kernel(
    const float* __restrict__ partial, const float* __restrict__ valids, int M, int splits, int C,
    const float* __restrict__ count, const float* __restrict__ gamma, const float* __restrict__ bn,
    float* __restrict__ coef, float* __restrict__ dgamma, float* __restrict__ dbeta, const CoopWs cw) {
  const int c = blockIdx.x * 64 + (threadIdx.x & 63);
  double s1, s2;
  if (!reduce_partials(partial, valids, M, splits, C, c, cw, s1, s2)) return;
  if (threadIdx.x >= 64) return;
  write_coef(coef, C, c, gamma[c], bn, s1, s2, (double)count[0]);
  dgamma[c] = (float)s2;
  dbeta[c] = (float)s1;
}

// layer-5 coefficients: dZ5 is sparse, grad_feat[m,c] sits at row argmax[m,c] whose pre-BatchNorm value the
// forward saved in ybest[m,c].  grid = (F/64, ceil(M/kEB)), block 1024.
__global__ __launch_bounds__(64 * kSlices) void pn_bwd_top_kernel(
    const float* __restrict__ gfeat, const int* __restrict__ argmax, const float* __restrict__ ybest,
    const float* __restrict__ valids, int M, int F, const float* __restrict__ count,
    const float* __restrict__ gamma, const float* __restrict__ bn, float* __restrict__ coef,
    float* __restrict__ dgamma, float* __restrict__ dbeta, const CoopWs cw) {
  const int c = blockIdx.x * 64 + (threadIdx.x & 63);
  const float mean = bn[2 * F + c], invstd = bn[3 * F + c];
  double s1, s2;
  const bool last = coop_colsum(M, F, c, cw,
                                [&](int m, bool& ok, double& x, double& y) {
                                  const long long o = (long long)m * F + c;
                                  const float g = gfeat[o];
                                  ok = valids[m] != 0.0f && argmax[o] >= 0;  // all-NaN column: no gradient
                                  x = (double)g;
                                  y = (double)g * (double)((ybest[o] - mean) * invstd);
                                },
                                s1, s2);
  if (!last || threadIdx.x >= 64) return;
  write_coef(coef, F, c, gamma[c], bn, s1, s2, (double)count[0]);
  dgamma[c] = (float)s2;
  dbeta[c] = (float)s1;
}

// ---- top-2 extrema records (last layer) --------------------------------------------------------------------------
// The last layer has no ReLU and feeds a max over the points, so its output tensor is never stored: BatchNorm being
// a per-channel monotone map, max_n z[n] is the image of max_n y[n] (scale > 0) or min_n y[n] (scale < 0).  The
// sign of scale = gamma * invstd is gamma's, known before the statistics are: the forward GEMM keeps, per (part,
// channel), the two largest sign(gamma) * y with their point indices (order: value descending, index ascending;
// gamma == 0 maps every point to `shift` and is handled in the finalize kernel).  Two, because z = fma(y, scale, shift) can round two distinct y to
// the SAME z, and the reference's arg-max then is the lower index of the two — decided once scale/shift are known.
struct Top2 {
  float v1, v2;
  int n1, n2;
};
constexpr int kNoIdx = 0x7fffffff;

__device__ __forceinline__ Top2 top2_empty() { return Top2{-__builtin_inff(), -__builtin_inff(), kNoIdx, kNoIdx}; }
__device__ __forceinline__ bool top2_before(float y, int n, float y2, int n2) {
  return y > y2 || (y == y2 && n < n2);
}
// n is larger than every index pushed before
__device__ __forceinline__ void top2_push(Top2& t, float y, int n) {
  // selects, not branches: this runs once per accumulator element in the forward GEMM's epilogue
  const bool g1 = y > t.v1, g2 = y > t.v2;
  t.v2 = g1 ? t.v1 : (g2 ? y : t.v2);
  t.n2 = g1 ? t.n1 : (g2 ? n : t.n2);
  t.v1 = g1 ? y : t.v1;
  t.n1 = g1 ? n : t.n1;
}
__device__ __forceinline__ Top2 top2_merge(const Top2 a, const Top2 b) {
  Top2 r;
  if (top2_before(b.v1, b.n1, a.v1, a.n1)) {
    r.v1 = b.v1;
    r.n1 = b.n1;
    const bool s = top2_before(a.v1, a.n1, b.v2, b.n2);
    r.v2 = s ? a.v1 : b.v2;
    r.n2 = s ? a.n1 : b.n2;
  } else {
    r.v1 = a.v1;
    r.n1 = a.n1;
    const bool s = top2_before(a.v2, a.n2, b.v1, b.n1);
    r.v2 = s ? a.v2 : b.v1;
    r.n2 = s ? a.n2 : b.n1;
  }
  return r;
}
__device__ __forceinline__ Top2 top2_shfl_xor(const Top2 t, int mask) {
  return Top2{__shfl_xor(t.v1, mask, 64), __shfl_xor(t.v2, mask, 64), __shfl_xor(t.n1, mask, 64),
              __shfl_xor(t.n2, mask, 64)};
}

// BatchNorm of the last layer + max over the points of each part from the per-block top-2 records.
// topv/topn [M*splits][F][2] = the two largest s*y (s = the sign of the channel's gamma) and their indices.
// One thread per (m, c).
__global__ void pn_top_finalize_kernel(const float* __restrict__ topv, const int* __restrict__ topn,
                                       const float* __restrict__ bn, const float* __restrict__ valids,
                                       const float* __restrict__ y4, const float* __restrict__ bn4,
                                       const float* __restrict__ w5, int M, int N, int F, int C4, int splits,
                                       float* __restrict__ feat, int* __restrict__ argmax,
                                       float* __restrict__ ybest) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)M * F) return;
  const int m = (int)(i / F), c = (int)(i % F);
  if (valids[m] == 0.0f) {
    feat[i] = 0.0f;  // padded slots hold zeros (network.py:66)
    argmax[i] = -1;
    ybest[i] = 0.0f;
    return;
  }
  Top2 t = top2_empty();
  for (int sp = 0; sp < splits; ++sp) {
    const long long o = (((long long)m * splits + sp) * F + c) * 2;
    const float2 v = *reinterpret_cast<const float2*>(topv + o);
    const int2 n = *reinterpret_cast<const int2*>(topn + o);
    t = top2_merge(t, Top2{v.x, v.y, n.x, n.y});
  }
  const float scale = bn[c], shift = bn[F + c];
  float z, y;
  int arg;
  if (scale != 0.0f) {  // scale = gamma * invstd has gamma's sign: the records hold the extrema of sign(gamma) * y
    const float sg = scale > 0.0f ? 1.0f : -1.0f;
    const float y1 = sg * t.v1, y2 = sg * t.v2;
    const float z1 = __builtin_fmaf(y1, scale, shift), z2 = __builtin_fmaf(y2, scale, shift);
    const bool second = t.n2 != kNoIdx && z2 == z1 && t.n2 < t.n1;
    arg = t.n1 == kNoIdx ? -1 : (second ? t.n2 : t.n1);  // no candidate: an all-NaN column
    y = second ? y2 : y1;
    z = z1;
  } else {  // gamma == 0: every point maps to `shift`, the arg-max is the first point; its y is recomputed
    arg = 0;
    z = shift;
    const float* row = y4 + (long long)m * N * C4;
    y = 0.0f;
    for (int k = 0; k < C4; ++k)
      y = __builtin_fmaf(__builtin_fmaxf(__builtin_fmaf(row[k], bn4[k], bn4[C4 + k]), 0.0f), w5[(long long)c * C4 + k], y);
  }
  feat[i] = z;
  argmax[i] = arg;
  ybest[i] = y;
}

// Per part: the sparse operand of the last layer's input gradient, dA4 += S W5, as finished rows.  The arg-max entries
// (row, channel, alpha * grad) are sorted by (row, channel) in LDS; every DISTINCT arg-max row gets its sum
//     rsum[m][j][:] = sum over the row's entries, in channel order, of  val * W5[channel][:]
// (from 0.0f, one __builtin_fmaf per entry and column: the order and the instruction are part of the result), and every
// 32-row tile t a record rtile[m][t] = {j of its first distinct row, bit r set: row 32 t + r has a sum}.  Rows are numbered in
// ascending order, so row 32 t + r of a tile is  j = rtile.x + popcount(rtile.y & ((1 << r) - 1)).
// Blocks [0, C4 + 1) compute Q and c0 (pn_top_q below), blocks [C4 + 1, C4 + 1 + M) one part each: two independent, latency-bound
// jobs that both wait for the coefficients of the last BatchNorm — side by side instead of one after the other (Q's chain of
// F dependent FMAs is the longer one: its blocks go first).  block = 1024 threads: the first F sort (one counting scan of
// single-word keys; leaders of the rows and their numbers from ballots), then sixteen lanes per row, two float4 columns each.
__device__ __forceinline__ void pn_top_q_row(const float* __restrict__ w5, const float* __restrict__ coef, int F, int C4,
                                             float* __restrict__ q, int k);
constexpr int kTopRowsThreads = 1024;
__host__ __device__ constexpr int pn_top_csr_lds_words(int F, int T) { return 4 * F + 12 + 2 * (T + 1); }
__global__ __launch_bounds__(kTopRowsThreads) void pn_top_csr_kernel(
    const int* __restrict__ argmax, const float* __restrict__ gfeat, const float* __restrict__ coef,
    const float* __restrict__ valids, int N, int F, int2* __restrict__ rtile, float* __restrict__ rsum, int M,
    const float* __restrict__ w5, float* __restrict__ q) {
  constexpr int C4 = 128, QC = C4 / 4, LPR = 16;  // lanes per row
  constexpr int kNone = 0x7fffffff;
  // [F] keys (row << 8 | channel) | [F] keys, sorted | [F] values, sorted | [F + 1] row starts | [3] D, pad | [4] leaders of a
  // wave | [4] entries of a wave | [T + 1] first row of a tile | [T + 1] row mask of a tile
  extern __shared__ __attribute__((aligned(16))) int sm[];
  if ((int)blockIdx.x <= C4) {
    pn_top_q_row(w5, coef, F, C4, q, (int)blockIdx.x);
    return;
  }
  const int m = (int)blockIdx.x - (C4 + 1), c = threadIdx.x, T = (N + 31) / 32;
  if (valids[m] == 0.0f) return;
  int* keys = sm;
  int* skey = sm + F;
  float* sval = reinterpret_cast<float*>(sm + 2 * F);
  int* rs = sm + 3 * F;
  int* wlead = sm + 4 * F + 4;
  int* wcnt = wlead + 4;
  int* toff = wcnt + 4;
  int* tmask = toff + T + 1;
  int key = kNone;
  if (c < F) {
    const int arg = argmax[(long long)m * F + c];
    key = arg >= 0 ? (arg << 8 | c) : kNone;  // (F <= 256, rows < 32768)
    keys[c] = key;
    skey[c] = kNone;
  }
  for (int t = c; t < 2 * (T + 1); t += kTopRowsThreads) toff[t] = 0;
  __syncthreads();
  if (c < F && key != kNone) {
    const int4* keys4 = reinterpret_cast<const int4*>(keys);  // (four words a read, several reads in flight)
    int pos = 0;
#pragma unroll 4
    for (int k4 = 0; k4 < F / 4; ++k4) {
      const int4 v = keys4[k4];
      pos += (v.x < key ? 1 : 0) + (v.y < key ? 1 : 0) + (v.z < key ? 1 : 0) + (v.w < key ? 1 : 0);
    }
    skey[pos] = key;
    sval[pos] = coef[c] * gfeat[(long long)m * F + c];  // alpha_c * grad_feat[m, c]
  }
  __syncthreads();
  // thread p takes the entry at sorted position p: the first entry of a row (its lowest channel) is the row's leader
  int row = -1;
  bool leader = false;
  unsigned long long lb = 0;
  if (c < F) {
    const int k = skey[c];
    const int prev = c > 0 ? skey[c - 1] >> 8 : -1;
    row = k >> 8;
    leader = k != kNone && row != prev;
    lb = __ballot(leader);
    const unsigned long long vb = __ballot(k != kNone);
    if ((c & 63) == 0) {
      wlead[c >> 6] = __builtin_popcountll(lb);
      wcnt[c >> 6] = __builtin_popcountll(vb);
    }
  }
  __syncthreads();
  if (c < F) {
    int j = __builtin_popcountll(lb & ((1ull << (c & 63)) - 1ull)), D = 0, E = 0;
    for (int w = 0; w < F / 64; ++w) {
      j += w < (c >> 6) ? wlead[w] : 0;
      D += wlead[w];
      E += wcnt[w];
    }
    if (leader) {
      rs[j] = c;
      const int prev = c > 0 ? skey[c - 1] >> 8 : -1;
      if ((prev >> 5) != (row >> 5)) toff[row >> 5] = j;
      atomicOr(&tmask[row >> 5], (int)(1u << (row & 31)));
    }
    if (c == 0) {
      rs[D] = E;
      rs[F + 1] = D;
    }
  }
  __syncthreads();
  for (int t = c; t <= T; t += kTopRowsThreads) rtile[(long long)m * (T + 1) + t] = make_int2(toff[t], tmask[t]);
  const int D = rs[F + 1], cq = c & (LPR - 1);
  const float4* w4 = reinterpret_cast<const float4*>(w5);
  for (int j = c / LPR; j < D; j += kTopRowsThreads / LPR) {
    const int pb = rs[j], pe = rs[j + 1];
    float4 a0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), a1 = a0;
    for (int p = pb; p < pe; p += 4) {  // up to four entries' weight rows in flight, then their FMAs in entry order
      float4 u0[4], u1[4];
      float v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (p + u < pe) {
          const int ch = skey[p + u] & 255;
          v[u] = sval[p + u];
          u0[u] = w4[(long long)ch * QC + cq];
          u1[u] = w4[(long long)ch * QC + cq + LPR];
        }
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (p + u < pe) {
          a0.x = __builtin_fmaf(v[u], u0[u].x, a0.x);
          a0.y = __builtin_fmaf(v[u], u0[u].y, a0.y);
          a0.z = __builtin_fmaf(v[u], u0[u].z, a0.z);
          a0.w = __builtin_fmaf(v[u], u0[u].w, a0.w);
          a1.x = __builtin_fmaf(v[u], u1[u].x, a1.x);
          a1.y = __builtin_fmaf(v[u], u1[u].y, a1.y);
          a1.z = __builtin_fmaf(v[u], u1[u].z, a1.z);
          a1.w = __builtin_fmaf(v[u], u1[u].w, a1.w);
        }
    }
    float4* o = reinterpret_cast<float4*>(rsum) + ((long long)m * F + j) * QC + cq;
    o[0] = a0;
    o[LPR] = a1;
  }
}

// Q[k][d] = sum_c gammap_c W5[c][k] W5[c][d]  (dA4 = A4 Q + c0 + sparse),  c0[d] = sum_c betap_c W5[c][d].
// grid = C4 + 1 (row k; the extra block writes c0), block = C4 threads (d).
__device__ __forceinline__ void pn_top_q_row(const float* __restrict__ w5, const float* __restrict__ coef, int F, int C4,
                                             float* __restrict__ q, int k) {
  for (int d = threadIdx.x; d < C4; d += blockDim.x) {
    float acc = 0.0f;
    if (k < C4) {
#pragma unroll 8
      for (int c = 0; c < F; ++c)
        acc = __builtin_fmaf(coef[F + c] * w5[(long long)c * C4 + k], w5[(long long)c * C4 + d], acc);
    } else {
#pragma unroll 8
      for (int c = 0; c < F; ++c) acc = __builtin_fmaf(coef[2 * F + c], w5[(long long)c * C4 + d], acc);
    }
    q[(long long)k * C4 + d] = acc;
  }
}

// Weight gradient of the last layer:
//   dW5[c][ci] = alpha_c sum_m g[m,c] A4[m, argmax[m,c], ci]  +  gammap_c (W5 G)[c][ci]  +  betap_c a4sum[ci]
// with G = A4^T A4 and a4sum the column sums of A4 over all valid points (gram[C4][C4] followed by a4sum[C4]).
// grid = F (channel c), block 1024 = C4(=128) columns x 8 part-slices.
__global__ __launch_bounds__(1024) void pn_top_wgrad_kernel(
    const float* __restrict__ gfeat, const int* __restrict__ argmax, const float* __restrict__ valids,
    const float* __restrict__ y4, const float* __restrict__ bn4, const float* __restrict__ w5,
    const float* __restrict__ coef, const float* __restrict__ gram, int M, int N, int F,
    float* __restrict__ dw5) {
  constexpr int C4 = 128, S = 8, U = 80, CH = S * U;  // parts per chunk: the shipped M = 640 is one
  __shared__ float sm[2][S][C4];
  __shared__ int arg_s[CH];    // arg-max row of part m (of this output channel), -1: no contribution
  __shared__ float g_s[CH];
  const int c = blockIdx.x, ci = threadIdx.x & (C4 - 1), slice = threadIdx.x >> 7;
  const float sc = bn4[ci], sh = bn4[C4 + ci];
  // the dense term W5 G of this output channel: every slice takes 16 of the 128 k (requested now, used at the end — on
  // slice 0 alone it was a chain of 128 dependent FMAs behind four batches of loads at the end of a latency-bound kernel)
  float wk[C4 / S], gk[C4 / S];
#pragma unroll
  for (int k = 0; k < C4 / S; ++k) {
    wk[k] = w5[(long long)c * C4 + slice * (C4 / S) + k];
    gk[k] = gram[(slice * (C4 / S) + k) * C4 + ci];
  }
  float acc = 0.0f;
  for (int m0 = 0; m0 < M; m0 += CH) {
    // level 1, once per part instead of once per (part, input channel): arg-max row and gradient of the chunk's parts
    if ((int)threadIdx.x < CH) {
      const int m = m0 + (int)threadIdx.x, mm = m < M ? m : M - 1;
      const int arg = argmax[(long long)mm * F + c];
      arg_s[threadIdx.x] = (m < M && valids[mm] != 0.0f && arg >= 0) ? arg : -1;
      g_s[threadIdx.x] = gfeat[(long long)mm * F + c];
    }
    __syncthreads();
    // level 2: the rows themselves, UB of a thread's requests in flight together (all 80 would need 160 address registers)
    constexpr int UB = 40;
#pragma unroll 1
    for (int u0 = 0; u0 < U; u0 += UB) {
      float yv[UB];
#pragma unroll
      for (int u = 0; u < UB; ++u) {
        const int i = slice + (u0 + u) * S, arg = arg_s[i], mm = m0 + i < M ? m0 + i : M - 1;
        yv[u] = y4[((long long)mm * N + (arg >= 0 ? arg : 0)) * C4 + ci];
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int u = 0; u < UB; ++u) {
        const int i = slice + (u0 + u) * S;
        if (arg_s[i] >= 0) acc = __builtin_fmaf(g_s[i], __builtin_fmaxf(__builtin_fmaf(yv[u], sc, sh), 0.0f), acc);
      }
    }
    __syncthreads();
  }
  float wg = 0.0f;
#pragma unroll
  for (int k = 0; k < C4 / S; ++k) wg = __builtin_fmaf(wk[k], gk[k], wg);
  sm[0][slice][ci] = acc;
  sm[1][slice][ci] = wg;
  __syncthreads();
  if (slice != 0) return;
  float sparse = 0.0f;
  wg = 0.0f;
#pragma unroll
  for (int k = 0; k < S; ++k) {
    sparse += sm[0][k][ci];
    wg += sm[1][k][ci];
  }
  dw5[(long long)c * C4 + ci] = coef[c] * sparse + coef[F + c] * wg + coef[2 * F + c] * gram[C4 * C4 + ci];
}

// ---- first layer (3 -> 64): scalar-operand VALU panel ------------------------------------------------------
// lane = point; the 3x64 transposed weights are wave-uniform (scalar cache).  grid = (ceil(N/256), M).
// partial [M*tiles][64][2].
// STORE = false (the shipped path): only the BatchNorm sums leave the kernel.  Y1 — 256 bytes per point, 3 FMAs per
// value from a 12-byte point — is never written: the kernels that consume it (layer 2's forward pn_fwd_ws_kernel, and
// pn_bwd_q_kernel, layer 2's backward, which also yields layer 1's weight gradient) recompute their tile from the points
// with first_layer_y below, the SAME operation sequence, so every consumer sees the bits the statistics were taken
// from.  Saves one write and a read per consumer of the [rows x 64] tensor per step (94 MB each at 366 valid parts).
__device__ __forceinline__ float first_layer_y(float a0, float a1, float a2, float w0, float w1, float w2) {
  float v = a0 * w0;
  v = __builtin_fmaf(a1, w1, v);
  return __builtin_fmaf(a2, w2, v);
}

template <bool STORE>
__global__ __launch_bounds__(kT) void pn_fwd_first_kernel(const float* __restrict__ pts,
                                                          const float* __restrict__ wt,
                                                          const float* __restrict__ valids, int N,
                                                          float* __restrict__ y_out,
                                                          float* __restrict__ partial) {
  __shared__ float tile[kT / 64][64][65];
  __shared__ float red[kT / 64][64][2];
  const int m = blockIdx.y;
  if (valids[m] == 0.0f) return;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int n0 = blockIdx.x * kT + wave * 64, n = n0 + lane;
  const long long row = (long long)m * N + (n < N ? n : N - 1);
  const int rows_here = N - n0 < 64 ? (N - n0 < 0 ? 0 : N - n0) : 64;
  const float a0 = pts[row * 3 + 0], a1 = pts[row * 3 + 1], a2 = pts[row * 3 + 2];
#pragma unroll
  for (int c = 0; c < 64; ++c) tile[wave][lane][c] = first_layer_y(a0, a1, a2, wt[c], wt[64 + c], wt[128 + c]);
  __builtin_amdgcn_wave_barrier();
  float s = 0.0f, ss = 0.0f;
  float* dst = y_out + ((long long)m * N + n0) * 64 + lane;
  for (int i = 0; i < rows_here; ++i) {
    const float v = tile[wave][i][lane];
    if constexpr (STORE) dst[(long long)i * 64] = v;
    s += v;
    ss = __builtin_fmaf(v, v, ss);
  }
  red[wave][lane][0] = s;
  red[wave][lane][1] = ss;
  __syncthreads();
  if (threadIdx.x < 64) {
    float t0 = 0.0f, t1 = 0.0f;
#pragma unroll
    for (int w = 0; w < kT / 64; ++w) {
      t0 += red[w][threadIdx.x][0];
      t1 += red[w][threadIdx.x][1];
    }
    const long long blk = (long long)m * gridDim.x + blockIdx.x;
    partial[(blk * 64 + threadIdx.x) * 2 + 0] = t0;
    partial[(blk * 64 + threadIdx.x) * 2 + 1] = t1;
  }
}

// bf16 vectors of the split-bf16 kernels (pn_bwd_q.h, pn_fwd_ws.h)
typedef __bf16 pn_bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 pn_bf16x4 __attribute__((ext_vector_type(4)));

// dW[i] = sum over the blocks' partial dW (valids == nullptr) or over valid parts of dwpart[m][i].
// block 1024 = 64 elements x 16 slices.
__global__ __launch_bounds__(64 * kSlices) void pn_wgrad_reduce_kernel(const float* __restrict__ dwpart,
                                                                      const float* __restrict__ valids,
                                                                      int M, int elems,
                                                                      float* __restrict__ dw) {
  __shared__ float sm[kSlices][64];
  const int el = threadIdx.x & 63, slice = threadIdx.x >> 6, i = blockIdx.x * 64 + el;
  float s = 0.0f;
  if (i < elems) {
    constexpr int U = 8;  // independent loads in flight; padded parts' rows hold garbage and are skipped
    for (int m0 = slice; m0 < M; m0 += kSlices * U) {
      float v[U], ok[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int m = m0 + u * kSlices, mm = m < M ? m : M - 1;
        v[u] = dwpart[(long long)mm * elems + i];
        ok[u] = m < M ? (valids != nullptr ? valids[mm] : 1.0f) : 0.0f;
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (ok[u] != 0.0f) s += v[u];
    }
  }
  sm[slice][el] = s;
  __syncthreads();
  if (slice == 0 && i < elems) {
    float t = 0.0f;
#pragma unroll
    for (int k = 0; k < kSlices; ++k) t += sm[k][el];
    dw[i] = t;
  }
}

// The same reduction for up to four weight gradients in ONE launch (the layers' partial tables wait in their own regions of
// dwpart until the end of the backward pass): blocks [first[k], first[k + 1]) serve problem k.  Same summation order.
struct WgradReduceGroup {
  const float* part[4];
  float* dw[4];
  int rows[4], elems[4], first[5];
};
__global__ __launch_bounds__(64 * kSlices) void pn_wgrad_reduce_group_kernel(const WgradReduceGroup g) {
  __shared__ float sm[kSlices][64];
  int k = 0;
#pragma unroll
  for (int q = 1; q < 4; ++q) k += (int)blockIdx.x >= g.first[q] ? 1 : 0;
  const float* __restrict__ dwpart = g.part[k];
  const int M = g.rows[k], elems = g.elems[k];
  const int el = threadIdx.x & 63, slice = threadIdx.x >> 6, i = ((int)blockIdx.x - g.first[k]) * 64 + el;
  float s = 0.0f;
  if (i < elems) {
    constexpr int U = 8;
    for (int m0 = slice; m0 < M; m0 += kSlices * U) {
      float v[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int m = m0 + u * kSlices, mm = m < M ? m : M - 1;
        v[u] = dwpart[(long long)mm * elems + i];
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (m0 + u * kSlices < M) s += v[u];
    }
  }
  sm[slice][el] = s;
  __syncthreads();
  if (slice == 0 && i < elems) {
    float t = 0.0f;
#pragma unroll
    for (int q = 0; q < kSlices; ++q) t += sm[q][el];
    g.dw[k][i] = t;
  }
}

#include "pn_bwd_q.h"
#include "pn_fwd_ws.h"
#ifndef MPA_PN_FWD4_BLOCKS
#define MPA_PN_FWD4_BLOCKS 512
#endif
// Rows the workspace reserves for per-block tables: two blocks per CU (256 CUs).  pn_fwd_ws_kernel's conv4 launch leaves
// MPA_PN_FWD4_BLOCKS rows of `partial`; the other persistent kernels run one block per CU and leave 256 rows of `partial`
// and, in `dwpart`, 256 rows of their layer's partial table.
constexpr int kWsBlocks = 512;
static_assert(MPA_PN_FWD4_BLOCKS <= kWsBlocks, "every block of conv4's forward pass leaves one row of `partial`");

// ---- host side ------------------------------------------------------------------------------------------------
struct Dims {
  int64_t M, N, F, rows;
  int tiles1;      // 256-row tiles of the first-layer kernel
  int splits_top;  // row splits of the last layer's forward GEMM (MFMA-bound: shorter blocks even out the tail)
  int C[6];        // channel widths: C[0] = 3 ... C[5] = F
};

Dims make_dims(int64_t M, int64_t N, int64_t F) {
  Dims d;
  d.M = M;
  d.N = N;
  d.F = F;
  d.rows = M * N;
  d.tiles1 = (int)((N + kT - 1) / kT);
  const int T = (int)((N + 31) / 32);
  d.splits_top = T >= 32 ? 8 : (T >= 16 ? 2 : 1);
  d.C[0] = 3;
  d.C[1] = 64;
  d.C[2] = 64;
  d.C[3] = 64;
  d.C[4] = 128;
  d.C[5] = (int)F;
  return d;
}

struct PnWs {
  float* Y[6];    // pre-BN outputs Y[1..4] (the last layer's output is never stored)
  float* dZ[6];   // backward: dZ[1..4]
  float* Wt1;     // transposed first-layer weights [3][64]
  float* bn[6];   // [4][C] scale, shift, mean, invstd
  float* coef[6]; // [3][C] alpha, gammap, betap
  float* partial; // per-block column sums
  float* dwpart;  // per-block partial tables: the last layer's Gram matrix + column sums, then those of layers 4..2
  float* count;
  CoopWs coop;    // fp64 group sums + tickets of the cooperative reductions
  float* topv;    // [M*splits][F][2] top-2 records of the last layer (values)
  float* ybest;   // [M][F] pre-BatchNorm value at the arg-max
  float* q;       // [129][128] Q then c0
  float* gram;    // [129][128] Gram matrix then column sums of A4
  float* ql[5];   // Q form of conv2..conv4: [CIN + 1][CIN] Q then c0 of layer l
  float* red[5];  // ... and the layer's reduced tables [T | G | asum | (S, P^T P, psum)]
  float* rsum;    // [M][F][128] S W5 of part m's distinct arg-max row j (at most F of them), see pn_top_csr_kernel
  int64_t total;
};

struct PnIws {
  int* argmax;  // [M][F]
  int* topn;    // [M*splits][F][2]
  int* vlist;   // [4 + M] number of valid parts, then (from [4]) their ids
  int2* rtile;  // [M][T+1] {first distinct arg-max row, mask of the rows that have one} of part m's 32-row tile t
  int64_t total;
};

PnWs carve(float* base, const Dims& d) {
  PnWs w;
  mpa::Arena a(base);  // every field 16-byte aligned for float4 accesses
  w.Y[1] = nullptr;  // never stored: recomputed from the points by its consumers (pn_fwd_first_kernel)
  for (int l = 2; l <= 4; ++l) w.Y[l] = a.take<float>(d.rows * d.C[l], 16);
  w.Y[5] = nullptr;
  w.dZ[1] = nullptr;  // never leaves the conv2 kernel (pn_bwd_q.h)
  for (int l = 2; l <= 4; ++l) w.dZ[l] = a.take<float>(d.rows * d.C[l], 16);
  w.Wt1 = a.take<float>(192, 16);
  for (int l = 1; l <= 5; ++l) w.bn[l] = a.take<float>(4LL * d.C[l], 16);
  for (int l = 1; l <= 5; ++l) w.coef[l] = a.take<float>(4LL * d.C[l], 16);
  const int64_t maxc = d.F > 128 ? d.F : 128;
  // rows of `partial`: one per (part, row split) or per (part, tile) of the row-split kernels, one per block of the
  // persistent ones
  int64_t blocks = d.M * (d.tiles1 > d.splits_top ? d.tiles1 : d.splits_top);
  if (blocks < kWsBlocks) blocks = kWsBlocks;
  w.partial = a.take<float>(blocks * maxc * 2, 16);
  // the Gram partials of the last layer (reduced at once), then — in the same storage — the partial tables of layers 4..2,
  // which wait for ONE grouped reduction at the end of the backward pass
  {
    const int64_t gram = (int64_t)kWsBlocks * (128 * 128 + 128);
    const int64_t wait =
        (int64_t)kWsBlocks * (pn_bwd_q_elems(128, 64, false) + pn_bwd_q_elems(64, 64, false) + pn_bwd_q_elems(64, 64, true));
    w.dwpart = a.take<float>(gram > wait ? gram : wait, 16);
  }
  for (int l = 2; l <= 4; ++l) {
    w.ql[l] = a.take<float>((int64_t)(d.C[l - 1] + 1) * d.C[l - 1], 16);
    w.red[l] = a.take<float>(pn_bwd_q_elems(d.C[l], d.C[l - 1], l == 2), 16);
  }
  w.count = a.take<float>(4, 16);
  w.coop.ticket = a.take<unsigned>(4, 16);
  w.coop.stage = a.take<double>(2 * maxc * ((blocks + kEB - 1) / kEB), 16);
  w.topv = a.take<float>(d.M * d.splits_top * d.F * 2, 16);
  w.ybest = a.take<float>(d.M * d.F, 16);
  w.q = a.take<float>(129 * 128, 16);
  w.gram = a.take<float>(129 * 128, 16);
  w.rsum = a.take<float>(d.M * d.F * 128, 16);
  w.total = a.elems<float>();
  return w;
}

PnIws carve_int(int32_t* base, const Dims& d) {
  PnIws w;
  mpa::Arena a(base);
  w.argmax = a.take<int32_t>(d.M * d.F, 16);
  w.topn = a.take<int32_t>(d.M * d.splits_top * d.F * 2, 16);
  w.vlist = a.take<int32_t>(d.M + 4, 16);
  w.rtile = a.take<int2>(d.M * ((d.N + 31) / 32 + 1), 16);
  w.total = a.elems<int32_t>();
  return w;
}

int check_dims(int64_t M, int64_t N, int64_t F, const char* who) {
  MPA_REQUIRE(M >= 0 && N >= 1 && F >= 64, "%s: bad sizes", who);
  MPA_REQUIRE(F == 64 || F == 128 || F == 256, "%s: feat_dim must be 64, 128 or 256", who);
  MPA_REQUIRE(M <= 32767 && N <= 32768, "%s: at most 32767 parts of at most 32768 points", who);
  return MPA_OK;
}

}  // namespace

extern "C" int mpa_pointnet_workspace(int64_t M, int64_t N, int64_t F, int64_t* float_elems,
                                      int64_t* int_elems) {
  if (int st = check_dims(M, N, F, "pointnet_workspace")) return st;
  MPA_REQUIRE(float_elems && int_elems, "pointnet_workspace: null pointer");
  const Dims d = make_dims(M, N, F);
  *float_elems = carve(nullptr, d).total;
  *int_elems = carve_int(nullptr, d).total;
  return MPA_OK;
}

extern "C" int mpa_pointnet_forward(const float* points, const float* valids, const float* const* conv_w,
                                    const float* const* bn_w, const float* const* bn_b,
                                    float* const* running_mean, float* const* running_var, int training,
                                    float momentum, float eps, int64_t M, int64_t N, int64_t F,
                                    float* float_ws, int32_t* int_ws, float* feat, void* stream) {
  if (int st = check_dims(M, N, F, "pointnet_forward")) return st;
  if (M == 0) return MPA_OK;
  MPA_REQUIRE(points && valids && conv_w && bn_w && bn_b && running_mean && running_var && float_ws &&
                  int_ws && feat, "pointnet_forward: null pointer");
  hipStream_t s = mpa::as_stream(stream);
  const Dims d = make_dims(M, N, F);
  const PnWs w = carve(float_ws, d);
  const PnIws iw = carve_int(int_ws, d);
  hipLaunchKernelGGL(pn_count_kernel, dim3(1), dim3(1024), 0, s, valids, (int)M, (int)N, w.count, w.coop.ticket,
                     iw.vlist, conv_w[0], w.Wt1);
  for (int l = 1; l <= 5; ++l) {
    int splits = 1;
    int prow_m = (int)M;              // rows of `partial`: (part, split) pairs with the validity mask, or persistent blocks
    const float* prow_valid = valids;
    if (l >= 2 && l <= 4) {
      prow_m = 256;
      prow_valid = nullptr;
      if (l == 2)  // (64-row units, one 12-wave block per CU; 32-row units in two 10-wave blocks per CU measured 48 vs 38 us)
        hipLaunchKernelGGL((pn_fwd_ws_kernel<64, 64, 64, true>), dim3(256), dim3(768), 0, s, points, w.bn[1], conv_w[1], iw.vlist,
                           (int)N, w.Y[2], w.partial, (const float*)w.Wt1);
      else if (l == 3)
        hipLaunchKernelGGL((pn_fwd_ws_kernel<64, 64, 64, false>), dim3(256), dim3(768), 0, s, w.Y[2], w.bn[2], conv_w[2],
                           iw.vlist, (int)N, w.Y[3], w.partial, (const float*)nullptr);
      else {  // (58 KB of LDS and 76 registers: two blocks per CU)
        prow_m = MPA_PN_FWD4_BLOCKS;
        hipLaunchKernelGGL((pn_fwd_ws_kernel<64, 128, 32, false, 2>), dim3(MPA_PN_FWD4_BLOCKS), dim3(768), 0, s, w.Y[3], w.bn[3],
                           conv_w[3], iw.vlist, (int)N, w.Y[4], w.partial, (const float*)nullptr);
      }
    } else if (l == 1) {
      splits = d.tiles1;
      hipLaunchKernelGGL(pn_fwd_first_kernel<false>, dim3((unsigned)d.tiles1, (unsigned)M), dim3(kT), 0, s, points,
                         w.Wt1, valids, (int)N, (float*)nullptr, w.partial);
    } else {
      splits = d.splits_top;
#define MPA_FWD_TOP_WS(NWV)                                                                                               \
  hipLaunchKernelGGL((pn_fwd_ws_top_kernel<128, NWV>), dim3(256), dim3(64 * (4 + NWV)), 0, s, w.Y[4], w.bn[4], conv_w[4],  \
                     d.C[5], iw.vlist, (int)N, splits, w.partial, w.topv, iw.topn, bn_w[4])
      if (F == 256) MPA_FWD_TOP_WS(8);
      else if (F == 128) MPA_FWD_TOP_WS(4);
      else MPA_FWD_TOP_WS(2);
#undef MPA_FWD_TOP_WS
    }
    const dim3 cg((unsigned)(d.C[l] / 64));
    if (training)
      hipLaunchKernelGGL(pn_bn_finalize_kernel, dim3(cg.x, (unsigned)(((long long)prow_m * splits + kEB - 1) / kEB)),
                         dim3(64 * kSlices), 0, s, w.partial, prow_valid, prow_m, splits, d.C[l], w.count, bn_w[l - 1],
                         bn_b[l - 1], running_mean[l - 1], running_var[l - 1], momentum, eps, w.bn[l], w.coop);
    else
      hipLaunchKernelGGL(pn_bn_from_running_kernel, cg, dim3(64), 0, s, d.C[l], bn_w[l - 1], bn_b[l - 1],
                         running_mean[l - 1], running_var[l - 1], eps, w.bn[l]);
  }
  hipLaunchKernelGGL(pn_top_finalize_kernel, dim3((unsigned)((M * F + 255) / 256)), dim3(256), 0, s, w.topv, iw.topn,
                     w.bn[5], valids, w.Y[4], w.bn[4], conv_w[4], (int)M, (int)N, (int)F, d.C[4], d.splits_top, feat,
                     iw.argmax, w.ybest);
  return mpa::check_launch("pointnet_forward");
}

extern "C" int mpa_pointnet_backward(const float* grad_feat, const float* points, const float* valids,
                                     const float* const* conv_w, const float* const* bn_w, int64_t M,
                                     int64_t N, int64_t F, float* float_ws, const int32_t* int_ws,
                                     float* const* grad_conv_w, float* const* grad_bn_w,
                                     float* const* grad_bn_b, void* stream) {
  if (int st = check_dims(M, N, F, "pointnet_backward")) return st;
  if (M == 0) return MPA_OK;
  MPA_REQUIRE(grad_feat && points && valids && conv_w && bn_w && float_ws && int_ws && grad_conv_w &&
                  grad_bn_w && grad_bn_b, "pointnet_backward: null pointer");
  hipStream_t s = mpa::as_stream(stream);
  const Dims d = make_dims(M, N, F);
  const PnWs w = carve(float_ws, d);
  const PnIws iw = carve_int(const_cast<int32_t*>(int_ws), d);
  const int C4 = d.C[4];
  // ---- last layer: its output was never stored (see the Top2 notes); dY5 = alpha*dZ5 + gammap*Y5 + betap with
  //      dZ5 sparse and Y5 = A4 W5^T gives  dA4 = A4 Q + c0 + S W5  and  dW5 = S^T A4 + gammap (W5 G) + betap a4sum
  hipLaunchKernelGGL(pn_bwd_top_kernel, dim3((unsigned)(F / 64), (unsigned)((M + kEB - 1) / kEB)), dim3(64 * kSlices),
                     0, s, grad_feat, iw.argmax, w.ybest, valids, (int)M, (int)F, w.count, bn_w[4], w.bn[5],
                     w.coef[5], grad_bn_w[4], grad_bn_b[4], w.coop);
  hipLaunchKernelGGL(pn_top_csr_kernel, dim3((unsigned)(M + C4 + 1)), dim3(kTopRowsThreads),
                     sizeof(int) * pn_top_csr_lds_words((int)F, (int)((N + 31) / 32)), s, iw.argmax, grad_feat, w.coef[5], valids, (int)N,
                     (int)F, iw.rtile, w.rsum, (int)M, conv_w[4], w.q);
  hipLaunchKernelGGL((pn_bwd_top_q_kernel<128, 4, 4, 4>), dim3(256), dim3(768), 0, s, w.Y[4], w.bn[4], w.q, iw.vlist, (int)N,
                     w.dZ[4], w.partial, w.dwpart, iw.rtile, w.rsum, (int)F);
  hipLaunchKernelGGL(pn_bwd_coef_kernel, dim3((unsigned)(C4 / 64), (unsigned)((256 + kEB - 1) / kEB)), dim3(64 * kSlices), 0, s,
                     w.partial, (const float*)nullptr, 256, 1, C4, w.count, bn_w[3], w.bn[4], w.coef[4], grad_bn_w[3],
                     grad_bn_b[3], w.coop);
  hipLaunchKernelGGL(pn_wgrad_reduce_kernel, dim3((unsigned)((C4 * C4 + C4 + 63) / 64)), dim3(64 * kSlices), 0, s, w.dwpart,
                     (const float*)nullptr, 256, C4 * C4 + C4, w.gram);
  hipLaunchKernelGGL(pn_top_wgrad_kernel, dim3((unsigned)F), dim3(1024), 0, s, grad_feat, iw.argmax, valids, w.Y[4],
                     w.bn[4], conv_w[4], w.coef[5], w.gram, (int)M, (int)N, (int)F, grad_conv_w[4]);
  // ---- layers 4..2 in Q form (pn_bwd_q.h): Q / c0 of the layer, then input gradient + weight-gradient tables in one pass,
  //      then the next layer's BatchNorm-backward coefficients; the weight gradients themselves at the very end
  WgradReduceGroup rg{};
  PnFinish fin{};
  long long part_off = 0;
  for (int l = 4, i = 0; l >= 2; --l, ++i) {
    const int cout = d.C[l], cin = d.C[l - 1], elems = pn_bwd_q_elems(cout, cin, l == 2);
    hipLaunchKernelGGL(pn_bwd_q_prep_kernel, dim3((unsigned)(cin + 1)), dim3((unsigned)cin), 0, s, conv_w[l - 1], w.coef[l],
                       cout, cin, w.ql[l]);
    float* const dwl = w.dwpart + part_off;
#define MPA_QK(KK, RBB, NSS, NDD, NWW, FI, YP)                                                                        \
  hipLaunchKernelGGL((pn_bwd_q_kernel<KK, 64, RBB, NSS, NDD, NWW, FI, (KK == 128 ? 2 : 1)>), dim3(nb),                  \
                     dim3(64 * (NSS + NDD + NWW)), 0,                                                                   \
                     s, w.dZ[l], YP, w.bn[l - 1], conv_w[l - 1], w.coef[l], w.ql[l], iw.vlist, (int)N, w.dZ[l - 1],    \
                     w.partial, dwl, (const float*)w.Wt1)
    const int nb = 256;
    if (l == 2) MPA_QK(64, 64, 4, 4, 4, true, points);                // Yprev = conv1's output: recomputed from the points
    else if (cout == 64) MPA_QK(64, 64, 4, 4, 4, false, w.Y[l - 1]);  // 64 -> 64: 64-row units, four input-gradient tiles
    else MPA_QK(128, 32, 4, 4, 4, false, w.Y[l - 1]);                 // 64 -> 128: 32-row units, k-split input-gradient pairs
#undef MPA_QK
    hipLaunchKernelGGL(pn_bwd_coef_kernel, dim3((unsigned)(cin / 64), (unsigned)((nb + kEB - 1) / kEB)),
                       dim3(64 * kSlices), 0, s, w.partial, (const float*)nullptr, nb, 1, cin, w.count, bn_w[l - 2],
                       w.bn[l - 1], w.coef[l - 1], grad_bn_w[l - 2], grad_bn_b[l - 2], w.coop);
    rg.part[i] = dwl;
    rg.dw[i] = w.red[l];
    rg.rows[i] = nb;
    rg.elems[i] = elems;
    fin.red[i] = w.red[l];
    fin.w[i] = conv_w[l - 1];
    fin.coef[i] = w.coef[l];
    fin.dw[i] = grad_conv_w[l - 1];
    fin.K[i] = cout;
    fin.CIN[i] = cin;
    part_off += (long long)nb * elems;
  }
  rg.first[0] = 0;
  fin.first[0] = 0;
  for (int k = 0; k < 4; ++k) rg.first[k + 1] = rg.first[k] + (k < 3 ? (rg.elems[k] + 63) / 64 : 0);
  for (int k = 0; k < 3; ++k) fin.first[k + 1] = fin.first[k] + (fin.K[k] * fin.CIN[k] + 255) / 256;
  fin.w1 = conv_w[0];
  fin.coef1 = w.coef[1];
  fin.dw1 = grad_conv_w[0];
  fin.first_layer = 2;  // conv2's table carries S = dZ1^T P, P^T P and psum
  hipLaunchKernelGGL(pn_wgrad_reduce_group_kernel, dim3((unsigned)rg.first[4]), dim3(64 * kSlices), 0, s, rg);
  hipLaunchKernelGGL(pn_bwd_finish_kernel, dim3((unsigned)(fin.first[3] + 1)), dim3(256), 0, s, fin);
  return mpa::check_launch("pointnet_backward");
}
