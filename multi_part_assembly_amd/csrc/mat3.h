// Rotation-matrix helpers shared by the rmat kernels (rmat.hip, match.hip, assembly_loss.hip, transformer.hip).
//
// A rotation is 9 floats, row-major.  Applying it follows the reference's `(r @ v[..., None])` (utils/transforms.py:
// 155-172): out_i = (r_i0 x + r_i1 y) + r_i2 z, left to right, no FMA (the library is built with -ffp-contract=off) — the
// order the reference's CPU matmul of a 3x3 by a 3-vector produces.
#pragma once

#include <hip/hip_runtime.h>

namespace mpa {

struct Mat3 {
  float r[9];
};

__device__ __forceinline__ Mat3 load_mat3(const float* __restrict__ p) {
  Mat3 m;
#pragma unroll
  for (int k = 0; k < 9; ++k) m.r[k] = p[k];
  return m;
}

__device__ __forceinline__ void mat3_rotate(const Mat3& m, float px, float py, float pz, float& ox, float& oy,
                                            float& oz) {
  ox = (m.r[0] * px + m.r[1] * py) + m.r[2] * pz;
  oy = (m.r[3] * px + m.r[4] * py) + m.r[5] * pz;
  oz = (m.r[6] * px + m.r[7] * py) + m.r[8] * pz;
}

// F.normalize(v, p=2, eps=1e-12): v / max(|v|, eps)
__device__ __forceinline__ float normalize3(const float* v, float* out) {
  const float n = __builtin_sqrtf((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
  const float d = __builtin_fmaxf(n, 1e-12f);
#pragma unroll
  for (int k = 0; k < 3; ++k) out[k] = v[k] / d;
  return n;
}

// normalize_rot6d (reference regressor.py:6-27) and the first two rows of rotation_6d_to_matrix (pytorch3d):
//   b1 = normalize(a1), b2 = normalize(a2 - (b1 . a2) b1).  Returns |a1| and |a2 - (b1.a2) b1| in n[0], n[1].
__device__ __forceinline__ void gram_schmidt6(const float* a, float* b, float* n) {
  n[0] = normalize3(a, b);
  const float d = (b[0] * a[3] + b[1] * a[4]) + b[2] * a[5];
  const float c[3] = {a[3] - d * b[0], a[4] - d * b[1], a[5] - d * b[2]};
  n[1] = normalize3(c, b + 3);
}

// Backward of gram_schmidt6 (recomputed from the input a): g [6] = d/d(b1, b2) -> ga [6].
//   normalize: b = c / n  ->  dc = (gb - b (b . gb)) / n   (gb / eps where n <= eps)
//   c = a2 - d b1, d = b1 . a2  ->  da2 = dc + gd b1,  db1 += gd a2 - d dc,  gd = -(dc . b1)
__device__ __forceinline__ void gram_schmidt6_backward(const float* a, const float* g, float* ga) {
  float b[6], n[2];
  gram_schmidt6(a, b, n);
  const float d = (b[0] * a[3] + b[1] * a[4]) + b[2] * a[5];
  const float* b1 = b;
  const float* b2 = b + 3;
  float dc[3];
  {
    const float s = (b2[0] * g[3] + b2[1] * g[4]) + b2[2] * g[5];
    const bool big = n[1] > 1e-12f;
    const float inv = 1.0f / __builtin_fmaxf(n[1], 1e-12f);
#pragma unroll
    for (int k = 0; k < 3; ++k) dc[k] = big ? (g[3 + k] - b2[k] * s) * inv : g[3 + k] * inv;
  }
  const float gd = -((dc[0] * b1[0] + dc[1] * b1[1]) + dc[2] * b1[2]);
  float gb1[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    ga[3 + k] = dc[k] + gd * b1[k];
    gb1[k] = g[k] + gd * a[3 + k] - d * dc[k];
  }
  const float s = (b1[0] * gb1[0] + b1[1] * gb1[1]) + b1[2] * gb1[2];
  const bool big = n[0] > 1e-12f;
  const float inv = 1.0f / __builtin_fmaxf(n[0], 1e-12f);
#pragma unroll
  for (int k = 0; k < 3; ++k) ga[k] = big ? (gb1[k] - b1[k] * s) * inv : gb1[k] * inv;
}

}  // namespace mpa
