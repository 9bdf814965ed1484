// Rotation matrices (rot_type='rmat'): conversions and the rigid pose application, forward and backward.
//
// Reference: multi_part_assembly/utils/rotation.py:134-167 (Rotation3D builds [...,3,3] matrices from the 6D form with
// pytorch3d's rotation_6d_to_matrix), utils/transforms.py:126-244 (rmat_rot / rmat_transform) and base_model.py:128-132
// (the ground-truth quaternions converted with quaternion_to_matrix every step).  One thread per row or point, the
// rotation of a part in registers; arithmetic in the order of the reference's definitions (mat3.h).
#include "common.h"
#include "mat3.h"

namespace {

constexpr int kThreads = 256;

// pytorch3d quaternion_to_matrix: two_s = 2 / |q|^2, rows of the standard formula, (r, i, j, k) = (w, x, y, z)
__global__ __launch_bounds__(kThreads) void quat_to_rmat_kernel(const float* __restrict__ q, long long count,
                                                                float* __restrict__ out) {
  const long long m = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (m >= count) return;
  const float r = q[4 * m], i = q[4 * m + 1], j = q[4 * m + 2], k = q[4 * m + 3];
  const float two_s = 2.0f / (((r * r + i * i) + j * j) + k * k);
  float* o = out + 9 * m;
  o[0] = 1.0f - two_s * (j * j + k * k);
  o[1] = two_s * (i * j - k * r);
  o[2] = two_s * (i * k + j * r);
  o[3] = two_s * (i * j + k * r);
  o[4] = 1.0f - two_s * (i * i + k * k);
  o[5] = two_s * (j * k - i * r);
  o[6] = two_s * (i * k - j * r);
  o[7] = two_s * (j * k + i * r);
  o[8] = 1.0f - two_s * (i * i + j * j);
}

// rotation_6d_to_matrix: rows b1, b2 (Gram-Schmidt, mat3.h) and b3 = b1 x b2 (torch.cross)
__global__ __launch_bounds__(kThreads) void rot6d_to_rmat_kernel(const float* __restrict__ d6, long long count,
                                                                 float* __restrict__ out) {
  const long long m = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (m >= count) return;
  float a[6], b[6], n[2];
#pragma unroll
  for (int k = 0; k < 6; ++k) a[k] = d6[6 * m + k];
  mpa::gram_schmidt6(a, b, n);
  float* o = out + 9 * m;
#pragma unroll
  for (int k = 0; k < 6; ++k) o[k] = b[k];
  o[6] = b[1] * b[5] - b[2] * b[4];
  o[7] = b[2] * b[3] - b[0] * b[5];
  o[8] = b[0] * b[4] - b[1] * b[3];
}

// backward: g = d/d(b1, b2, b3) -> d/d(b1, b2) through b3 = b1 x b2 (db1 += b2 x g3, db2 += g3 x b1), then Gram-Schmidt
__global__ __launch_bounds__(kThreads) void rot6d_to_rmat_bwd_kernel(const float* __restrict__ d6,
                                                                     const float* __restrict__ grad, long long count,
                                                                     float* __restrict__ gd6) {
  const long long m = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (m >= count) return;
  float a[6], b[6], n[2], g[6], ga[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) a[k] = d6[6 * m + k];
  mpa::gram_schmidt6(a, b, n);
  const float* G = grad + 9 * m;
  const float g3[3] = {G[6], G[7], G[8]};
  g[0] = G[0] + (b[4] * g3[2] - b[5] * g3[1]);
  g[1] = G[1] + (b[5] * g3[0] - b[3] * g3[2]);
  g[2] = G[2] + (b[3] * g3[1] - b[4] * g3[0]);
  g[3] = G[3] + (g3[1] * b[2] - g3[2] * b[1]);
  g[4] = G[4] + (g3[2] * b[0] - g3[0] * b[2]);
  g[5] = G[5] + (g3[0] * b[1] - g3[1] * b[0]);
  mpa::gram_schmidt6_backward(a, g, ga);
#pragma unroll
  for (int k = 0; k < 6; ++k) gd6[6 * m + k] = ga[k];
}

// grid = (ceil(N / kThreads), M); one part per blockIdx.y so R / t / mask are wave-uniform
__global__ __launch_bounds__(kThreads) void rmat_apply_kernel(const float* __restrict__ pc, const float* __restrict__ rmat,
                                                              const float* __restrict__ trans,
                                                              const float* __restrict__ mask, float fill, int n_points,
                                                              float* __restrict__ out) {
  const int m = blockIdx.y;
  const int n = blockIdx.x * kThreads + threadIdx.x;
  if (n >= n_points) return;
  const mpa::Mat3 R = mpa::load_mat3(rmat + 9LL * m);
  const long long o = 3 * ((long long)m * n_points + n);
  float px, py, pz;
  if (mask != nullptr && mask[m] == 0.0f) {
    px = py = pz = fill;  // masked_fill(valid == 0, fill) before the transform (loss.py:173-175)
  } else {
    px = pc[o + 0];
    py = pc[o + 1];
    pz = pc[o + 2];
  }
  float ox, oy, oz;
  mpa::mat3_rotate(R, px, py, pz, ox, oy, oz);
  if (trans != nullptr) {
    ox = ox + trans[3 * m + 0];
    oy = oy + trans[3 * m + 1];
    oz = oz + trans[3 * m + 2];
  }
  out[o + 0] = ox;
  out[o + 1] = oy;
  out[o + 2] = oz;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// Backward of out = R p + t:  dR_ij = sum_n g_i p_j,  dt = sum_n g,  dp = R^T g (zero where masked).
// One block per part; fixed-shape tree reduction (deterministic).
__global__ __launch_bounds__(kThreads) void rmat_grad_kernel(const float* __restrict__ gout, const float* __restrict__ pc,
                                                             const float* __restrict__ rmat, const float* __restrict__ mask,
                                                             float fill, int n_points, float* __restrict__ grmat,
                                                             float* __restrict__ gtrans, float* __restrict__ gpc) {
  const int m = blockIdx.x;
  const mpa::Mat3 R = mpa::load_mat3(rmat + 9LL * m);
  const bool masked = mask != nullptr && mask[m] == 0.0f;
  float acc[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};  // dR (row-major), dt
  for (int n = threadIdx.x; n < n_points; n += kThreads) {
    const long long o = 3 * ((long long)m * n_points + n);
    const float g[3] = {gout[o + 0], gout[o + 1], gout[o + 2]};
    float p[3];
    if (masked) {
      p[0] = p[1] = p[2] = fill;
    } else {
      p[0] = pc[o + 0];
      p[1] = pc[o + 1];
      p[2] = pc[o + 2];
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
      for (int j = 0; j < 3; ++j) acc[3 * i + j] += g[i] * p[j];
      acc[9 + i] += g[i];
    }
    if (gpc != nullptr) {
      float r[3] = {0.0f, 0.0f, 0.0f};
      if (!masked) {
#pragma unroll
        for (int j = 0; j < 3; ++j) r[j] = (R.r[j] * g[0] + R.r[3 + j] * g[1]) + R.r[6 + j] * g[2];
      }
      gpc[o + 0] = r[0];
      gpc[o + 1] = r[1];
      gpc[o + 2] = r[2];
    }
  }
  __shared__ float red[kThreads / 64][12];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < 12; ++k) {
    const float s = wave_sum(acc[k]);
    if (lane == 0) red[wave][k] = s;
  }
  __syncthreads();
  if (threadIdx.x < 12) {
    float s = 0.0f;
#pragma unroll
    for (int v = 0; v < kThreads / 64; ++v) s += red[v][threadIdx.x];
    if (threadIdx.x < 9) grmat[9LL * m + threadIdx.x] = s;
    else if (gtrans != nullptr) gtrans[3LL * m + (threadIdx.x - 9)] = s;
  }
}

unsigned blocks_for(int64_t count) { return (unsigned)((count + kThreads - 1) / kThreads); }

}  // namespace

extern "C" int mpa_quat_to_rmat(const float* quat, int64_t count, float* rmat, void* stream) {
  MPA_REQUIRE(count >= 0 && count < (1LL << 40), "quat_to_rmat: bad size");
  if (count == 0) return MPA_OK;
  MPA_REQUIRE(quat && rmat, "quat_to_rmat: null pointer");
  hipLaunchKernelGGL(quat_to_rmat_kernel, dim3(blocks_for(count)), dim3(kThreads), 0, mpa::as_stream(stream), quat,
                     (long long)count, rmat);
  return mpa::check_launch("quat_to_rmat");
}

extern "C" int mpa_rot6d_to_rmat_forward(const float* rot6d, int64_t count, float* rmat, void* stream) {
  MPA_REQUIRE(count >= 0 && count < (1LL << 40), "rot6d_to_rmat_forward: bad size");
  if (count == 0) return MPA_OK;
  MPA_REQUIRE(rot6d && rmat, "rot6d_to_rmat_forward: null pointer");
  hipLaunchKernelGGL(rot6d_to_rmat_kernel, dim3(blocks_for(count)), dim3(kThreads), 0, mpa::as_stream(stream), rot6d,
                     (long long)count, rmat);
  return mpa::check_launch("rot6d_to_rmat_forward");
}

extern "C" int mpa_rot6d_to_rmat_backward(const float* rot6d, const float* grad_rmat, int64_t count, float* grad_rot6d,
                                          void* stream) {
  MPA_REQUIRE(count >= 0 && count < (1LL << 40), "rot6d_to_rmat_backward: bad size");
  if (count == 0) return MPA_OK;
  MPA_REQUIRE(rot6d && grad_rmat && grad_rot6d, "rot6d_to_rmat_backward: null pointer");
  hipLaunchKernelGGL(rot6d_to_rmat_bwd_kernel, dim3(blocks_for(count)), dim3(kThreads), 0, mpa::as_stream(stream), rot6d,
                     grad_rmat, (long long)count, grad_rot6d);
  return mpa::check_launch("rot6d_to_rmat_backward");
}

extern "C" int mpa_pose_apply_rmat_forward(const float* pc, const float* rmat, const float* trans, const float* mask,
                                           float fill, int64_t num_parts, int64_t num_points, float* out, void* stream) {
  MPA_REQUIRE(num_parts >= 0 && num_points >= 0, "pose_apply_rmat_forward: negative size");
  if (num_parts == 0 || num_points == 0) return MPA_OK;
  MPA_REQUIRE(pc && rmat && out, "pose_apply_rmat_forward: null pointer");
  MPA_REQUIRE(num_parts <= 65535 && num_points < (1LL << 31), "pose_apply_rmat_forward: size too large");
  dim3 grid(blocks_for(num_points), (unsigned)num_parts, 1);
  hipLaunchKernelGGL(rmat_apply_kernel, grid, dim3(kThreads), 0, mpa::as_stream(stream), pc, rmat, trans, mask, fill,
                     (int)num_points, out);
  return mpa::check_launch("pose_apply_rmat_forward");
}

extern "C" int mpa_pose_apply_rmat_backward(const float* grad_out, const float* pc, const float* rmat, const float* mask,
                                            float fill, int64_t num_parts, int64_t num_points, float* grad_rmat,
                                            float* grad_trans, float* grad_pc, void* stream) {
  MPA_REQUIRE(num_parts >= 0 && num_points >= 0, "pose_apply_rmat_backward: negative size");
  if (num_parts == 0) return MPA_OK;
  MPA_REQUIRE(grad_out && pc && rmat && grad_rmat, "pose_apply_rmat_backward: null pointer");
  MPA_REQUIRE(num_parts < (1LL << 31) && num_points < (1LL << 31), "pose_apply_rmat_backward: size too large");
  hipLaunchKernelGGL(rmat_grad_kernel, dim3((unsigned)num_parts), dim3(kThreads), 0, mpa::as_stream(stream), grad_out,
                     pc, rmat, mask, fill, (int)num_points, grad_rmat, grad_trans, grad_pc);
  return mpa::check_launch("pose_apply_rmat_backward");
}
