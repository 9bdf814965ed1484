// Pieces shared by the matrix-core GEMMs over the point rows of the DGCNN encoder and the MLP layers (gfx950): the
// 32 x 32 accumulator layout, the grid rounding of the row tiles, and the fixed-order second stage of the weight
// gradients.  The GEMM kernels themselves are the fp32-grade split-bf16 kernels of dg_gemm_split.h.
//
// The reference's EdgeConv stages are 1x1 Conv2d over [n, 2C, N, k] edge tensors and a 1x1 Conv1d over the 512-wide
// concatenation (multi_part_assembly/models/modules/encoder/dgcnn.py:57-71,76-100); here they are plain GEMMs over
// R = (valid parts) x N point rows (csrc/dgcnn_enc.hip explains the algebra).
#pragma once

#include <hip/hip_runtime.h>

namespace dg {

typedef float f32x16 __attribute__((ext_vector_type(16)));

// MFMA 32x32 accumulator layout: lane l holds column (l & 31) and, in register r, row acc_row(r, l >> 5).
__device__ __forceinline__ int acc_row(int reg, int half) { return (reg & 3) + 8 * (reg >> 2) + 4 * half; }

constexpr int kKC = 32;  // K chunk
#define DG_GEMM_GRID_X(rows) ((unsigned)((((rows) + 127) / 128 + 7) / 8 * 8))  // row tiles, rounded up to the XCD count

// second stage of the weight gradient: out[e] = sum_chunk part[chunk][e], in a FIXED order (deterministic): a block of
// 256 threads owns EPB consecutive elements; 256 / EPB slices of the chunk range are summed side by side (eight
// independent partial sums each, so the loads pipeline) and combined in slice order.
template <int EPB>
__device__ __forceinline__ void tn_reduce_block(const float* __restrict__ part, int chunks, long long elems,
                                                float* __restrict__ out, int block) {
  constexpr int SL = 256 / EPB;
  __shared__ float red[SL][EPB];
  const int el = threadIdx.x % EPB, sl = threadIdx.x / EPB;
  const long long e = (long long)block * EPB + el;
  const int per = (chunks + SL - 1) / SL;
  const int c0 = sl * per, c1 = c0 + per < chunks ? c0 + per : chunks;
  float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (e < elems) {
    const float* p = part + e;
    int c = c0;
    for (; c + 8 <= c1; c += 8) {
#pragma unroll
      for (int u = 0; u < 8; ++u) a[u] += p[(long long)(c + u) * elems];
    }
    for (; c < c1; ++c) a[0] += p[(long long)c * elems];
  }
  red[sl][el] = ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
  __syncthreads();
  if (sl == 0 && e < elems) {
    float t = red[0][el];
#pragma unroll
    for (int q = 1; q < SL; ++q) t += red[q][el];
    out[e] = t;
  }
}
template <int EPB>
static __global__ __launch_bounds__(256) void gemm_tn_reduce_kernel(const float* __restrict__ part, int chunks,
                                                                    long long elems, float* __restrict__ out) {
  tn_reduce_block<EPB>(part, chunks, elems, out, (int)blockIdx.x);
}
// two tables in one launch: blocks [0, blocks_a) reduce table a, the others table b (an MLP layer's weight gradient and
// the per-tile column sums of its bias gradient)
static __global__ __launch_bounds__(256) void gemm_tn_reduce2_kernel(const float* __restrict__ pa, int chunks_a,
                                                                     long long elems_a, float* __restrict__ out_a,
                                                                     int blocks_a, const float* __restrict__ pb,
                                                                     int chunks_b, long long elems_b,
                                                                     float* __restrict__ out_b) {
  if ((int)blockIdx.x < blocks_a) tn_reduce_block<32>(pa, chunks_a, elems_a, out_a, (int)blockIdx.x);
  else tn_reduce_block<32>(pb, chunks_b, elems_b, out_b, (int)blockIdx.x - blocks_a);
}

// few elements and many chunks (the 128 x 4 first-layer gradient: thousands of row tiles) -> more slices per element
static inline void launch_tn_reduce(const float* part, int chunks, long long elems, float* out, hipStream_t s) {
  if (elems <= 4096)
    hipLaunchKernelGGL(gemm_tn_reduce_kernel<8>, dim3((unsigned)((elems + 7) / 8)), dim3(256), 0, s, part, chunks, elems, out);
  else
    hipLaunchKernelGGL(gemm_tn_reduce_kernel<32>, dim3((unsigned)((elems + 31) / 32)), dim3(256), 0, s, part, chunks, elems,
                       out);
}

}  // namespace dg
