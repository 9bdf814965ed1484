// The per-part transform of GeometryPartDataset.__getitem__ (multi_part_assembly/datasets/geometry_data.py:74-107,
// 133-146) as block-level device code: centroid = mean of the part's N float64 points, points -= centroid, points =
// (rot @ points^T)^T, points = points[order], float32 cast; part_trans = centroid.  One 256-thread block per part slot,
// float64, thread-strided partial sums folded by a fixed-order tree, no FMA (every file is built with
// -ffp-contract=off).  Two kernels run it: part_batch_transform_kernel (csrc/batch.hip) on a cloud in global memory,
// mesh_sample_kernel (csrc/mesh_sample.hip) on the cloud it has just sampled into LDS — the same operations in the same
// order, so the two produce the same bits from the same points.
#pragma once

namespace mpa {

constexpr int kPartThreads = 256;

// Padded slot: zeros (geometry_data.py:102-107).
__device__ __forceinline__ void part_zero_fill(int N, float* __restrict__ out, float* __restrict__ trans) {
  const int t = threadIdx.x;
  for (int i = t; i < 3 * N; i += kPartThreads) out[i] = 0.0f;
  if (t < 3) trans[t] = 0.0f;
}

// src [N,3] float64 (global memory or LDS, complete and visible to the whole block), rot [9] row-major, ord [N] point
// order (kPerm) -> out [N,3], trans [3].  Every thread of the block calls it.
template <bool kPerm>
__device__ __forceinline__ void part_transform_block(const double* __restrict__ src, const double* __restrict__ rot,
                                                     const int* __restrict__ ord, int N,
                                                     float* __restrict__ out, float* __restrict__ trans) {
  __shared__ double red[kPartThreads][3];
  __shared__ double cen[3];
  const int t = threadIdx.x;
  double sx = 0.0, sy = 0.0, sz = 0.0;
  for (int i = t; i < N; i += kPartThreads) {
    sx += src[3 * i + 0];
    sy += src[3 * i + 1];
    sz += src[3 * i + 2];
  }
  red[t][0] = sx;
  red[t][1] = sy;
  red[t][2] = sz;
  __syncthreads();
  for (int half = kPartThreads / 2; half >= 1; half >>= 1) {  // fixed-order tree
    if (t < half) {
      red[t][0] += red[t + half][0];
      red[t][1] += red[t + half][1];
      red[t][2] += red[t + half][2];
    }
    __syncthreads();
  }
  if (t < 3) {
    const double c = red[0][t] / (double)N;
    cen[t] = c;
    trans[t] = (float)c;
  }
  __syncthreads();
  const double cx = cen[0], cy = cen[1], cz = cen[2];
  double r[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) r[k] = rot[k];
  for (int i = t; i < N; i += kPartThreads) {
    const int s = kPerm ? ord[i] : i;
    const double px = src[3 * s + 0] - cx, py = src[3 * s + 1] - cy, pz = src[3 * s + 2] - cz;
    out[3 * i + 0] = (float)((r[0] * px + r[1] * py) + r[2] * pz);
    out[3 * i + 1] = (float)((r[3] * px + r[4] * py) + r[5] * pz);
    out[3 * i + 2] = (float)((r[6] * px + r[7] * py) + r[8] * pz);
  }
}

}  // namespace mpa
