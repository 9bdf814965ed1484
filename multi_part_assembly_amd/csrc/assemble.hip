// Assembled shapes for export: coloured posed part clouds of a whole batch, and posed part meshes.
//
// Replaces the tail of BaseModel.sample_assembly (multi_part_assembly/models/modules/base_model.py:440-458: per sample
// and per shape a boolean-mask gather, a `.cpu()` and a host loop over the parts for the colours, utils/utils.py:49-64)
// and the mesh half of scripts/vis.py:75-96 (per part two 4x4 `apply_transform` calls on the host).
//
// Clouds: launch 1 turns `valids` into the row offsets of the shapes; launch 2 reads every point of a valid part once,
// poses it S + 1 times (S predictions, then the ground truth) with the device functions behind mpa_pose_apply[_rmat]_forward
// (quat.h / mat3.h: same operations in the same order, no FMA) and writes the 24-byte rows (x, y, z, r, g, b).  The
// rows of a block are one contiguous byte range of the slab, so they are staged in LDS and leave as flat 16-byte stores.
// Meshes: one thread per triangle of a selected part, float64 arithmetic on the store's (origin, e1, e2) rows.
#include "common.h"
#include "mat3.h"
#include "quat.h"

namespace {

constexpr int kThreads = 256;

// Copies `count` floats from LDS to `dst` (4-byte aligned) with the whole block: scalar stores up to the first 16-byte
// boundary of `dst`, one 16-byte store per lane behind it, scalar stores for the last < 4 floats.
__device__ __forceinline__ void store_staged(const float* lds, int count, float* __restrict__ dst) {
  const int t = threadIdx.x;
  int head = (int)((0u - (unsigned)(reinterpret_cast<uintptr_t>(dst) >> 2)) & 3u);
  if (head > count) head = count;
  const int vec = (count - head) >> 2;
  for (int i = t; i < vec; i += kThreads) {
    const float* s = lds + head + 4 * i;
    *reinterpret_cast<float4*>(dst + head + 4 * i) = make_float4(s[0], s[1], s[2], s[3]);
  }
  const int done = head + 4 * vec;
  if (t < head) dst[t] = lds[t];
  if (t >= mpa::kWave && t - mpa::kWave < count - done) dst[done + t - mpa::kWave] = lds[done + t - mpa::kWave];
}

// ---- clouds -------------------------------------------------------------------------------------------------------------
// One block: offsets[b] = N * (number of valid parts of the shapes before b), offsets[B] the rows in use.  Shapes are
// taken 256 at a time, an inclusive Hillis-Steele scan in LDS per chunk, the running total carried in `base`.
__global__ __launch_bounds__(kThreads) void cloud_offsets_kernel(const float* __restrict__ valids, int B, int P,
                                                                 long long N, int64_t* __restrict__ offsets) {
  __shared__ int scan[kThreads];
  const int t = threadIdx.x;
  long long base = 0;
  if (t == 0) offsets[0] = 0;
  for (int b0 = 0; b0 < B; b0 += kThreads) {
    const int b = b0 + t;
    int cnt = 0;
    if (b < B)
      for (int p = 0; p < P; ++p) cnt += valids[(long long)b * P + p] == 1.0f ? 1 : 0;
    scan[t] = cnt;
    __syncthreads();
    for (int off = 1; off < kThreads; off <<= 1) {
      const int add = t >= off ? scan[t - off] : 0;
      __syncthreads();
      scan[t] += add;
      __syncthreads();
    }
    if (b < B) offsets[b + 1] = (base + scan[t]) * N;
    base += scan[kThreads - 1];
    __syncthreads();
  }
}

template <bool kRmat>
struct Pose;
template <>
struct Pose<false> {
  mpa::Quat q;
  float t[3];
  __device__ __forceinline__ void load(const float* __restrict__ rot, const float* __restrict__ trans, long long m) {
    q = mpa::Quat{rot[4 * m + 0], rot[4 * m + 1], rot[4 * m + 2], rot[4 * m + 3]};
    t[0] = trans[3 * m + 0], t[1] = trans[3 * m + 1], t[2] = trans[3 * m + 2];
  }
  __device__ __forceinline__ void apply(float px, float py, float pz, float* o) const {
    float x, y, z;
    mpa::quat_rotate(q, px, py, pz, x, y, z);
    o[0] = x + t[0], o[1] = y + t[1], o[2] = z + t[2];
  }
};
template <>
struct Pose<true> {
  mpa::Mat3 r;
  float t[3];
  __device__ __forceinline__ void load(const float* __restrict__ rot, const float* __restrict__ trans, long long m) {
    r = mpa::load_mat3(rot + 9 * m);
    t[0] = trans[3 * m + 0], t[1] = trans[3 * m + 1], t[2] = trans[3 * m + 2];
  }
  __device__ __forceinline__ void apply(float px, float py, float pz, float* o) const {
    float x, y, z;
    mpa::mat3_rotate(r, px, py, pz, x, y, z);
    o[0] = x + t[0], o[1] = y + t[1], o[2] = z + t[2];
  }
};

// grid = (B * P part slots, ceil(N / 256)); a block owns up to 256 consecutive points of one part, one per thread.  A
// padded slot returns before it has read a point or a pose.  The staging buffer is doubled: slab s + 1 is posed into
// one half while the stores of slab s still read the other, one barrier per slab.
template <bool kRmat>
__global__ __launch_bounds__(kThreads) void assemble_clouds_kernel(
    const float* __restrict__ part_pcs, const float* __restrict__ valids, const float* __restrict__ rot,
    const float* __restrict__ trans, const float* __restrict__ gt_rot, const float* __restrict__ gt_trans,
    const float* __restrict__ colors, int S, int P, int N, long long slots, const int64_t* __restrict__ offsets,
    float* __restrict__ clouds) {
  __shared__ __align__(16) float stage[2][kThreads * 6];
  const long long m = blockIdx.x;
  if (valids[m] != 1.0f) return;
  const int b = (int)(m / P), p = (int)(m - (long long)b * P), t = threadIdx.x;
  int rank = 0;  // of this part among the valid parts of its shape: its colour, and its place in the segment
  for (int k = 0; k < p; ++k) rank += valids[(long long)b * P + k] == 1.0f ? 1 : 0;
  const int n0 = blockIdx.y * kThreads;
  const int rows = min(kThreads, N - n0);
  const long long row0 = offsets[b] + (long long)rank * N + n0;  // < offsets[b + 1] <= slots * N
  const float cr = colors[3 * rank + 0], cg = colors[3 * rank + 1], cb = colors[3 * rank + 2];
  float px = 0.0f, py = 0.0f, pz = 0.0f;
  if (t < rows) {
    const float* src = part_pcs + 3 * (m * N + n0 + t);
    px = src[0], py = src[1], pz = src[2];
  }
  const long long cap = slots * N;  // rows of one slab
  for (int s = 0; s <= S; ++s) {
    Pose<kRmat> pose;
    if (s < S) pose.load(rot, trans, (long long)s * slots + m);
    else pose.load(gt_rot, gt_trans, m);
    float* buf = stage[s & 1];
    if (t < rows) {
      float* o = buf + 6 * t;
      pose.apply(px, py, pz, o);
      o[3] = cr, o[4] = cg, o[5] = cb;
    }
    __syncthreads();
    store_staged(buf, 6 * rows, clouds + 6 * ((long long)s * cap + row0));
  }
}

// ---- meshes -------------------------------------------------------------------------------------------------------------
// grid = (M slots, ceil(max faces of a slot / 256)), one thread per triangle.  float64 throughout on the float32 poses
// widened, every operation rounded once (-ffp-contract=off), one rounding to float32 at the store.
__global__ __launch_bounds__(kThreads) void mesh_pose_kernel(
    const double* __restrict__ tri, const int64_t* __restrict__ part_face_off, int64_t parts_total,
    const int64_t* __restrict__ slot_part, const int64_t* __restrict__ out_face_off, int64_t faces_out,
    const float* __restrict__ gt_rmat, const float* __restrict__ gt_trans, const float* __restrict__ pred_rmat,
    const float* __restrict__ pred_trans, float* __restrict__ orig, float* __restrict__ input, float* __restrict__ pred) {
  const int m = blockIdx.x;
  const int64_t part = slot_part[m];
  if (part < 0 || part >= parts_total) return;
  const int64_t f0 = part_face_off[part], o0 = out_face_off[m];
  int64_t F = part_face_off[part + 1] - f0;
  if (o0 < 0) return;
  if (F > out_face_off[m + 1] - o0) F = out_face_off[m + 1] - o0;  // never past the slot's own rows,
  if (F > faces_out - o0) F = faces_out - o0;                      // nor past the outputs
  const int64_t f = (int64_t)blockIdx.y * kThreads + threadIdx.x;
  if (f >= F) return;
  double Rg[9], Tg[3], Rp[9], Tp[3];
#pragma unroll
  for (int k = 0; k < 9; ++k) Rg[k] = (double)gt_rmat[9 * m + k], Rp[k] = (double)pred_rmat[9 * m + k];
#pragma unroll
  for (int k = 0; k < 3; ++k) Tg[k] = (double)gt_trans[3 * m + k], Tp[k] = (double)pred_trans[3 * m + k];
  const double* r = tri + 9 * (f0 + f);
  const long long o = 9 * (o0 + f);
#pragma unroll
  for (int v = 0; v < 3; ++v) {
    double x[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) x[k] = v == 0 ? r[k] : r[k] + r[3 * v + k];  // origin, origin + e1, origin + e2
    const double d[3] = {x[0] - Tg[0], x[1] - Tg[1], x[2] - Tg[2]};
    double y[3];  // R_gt^T (x - T_gt)
#pragma unroll
    for (int k = 0; k < 3; ++k) y[k] = (Rg[k] * d[0] + Rg[3 + k] * d[1]) + Rg[6 + k] * d[2];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      orig[o + 3 * v + k] = (float)x[k];
      input[o + 3 * v + k] = (float)y[k];
      pred[o + 3 * v + k] = (float)(((Rp[3 * k] * y[0] + Rp[3 * k + 1] * y[1]) + Rp[3 * k + 2] * y[2]) + Tp[k]);
    }
  }
}

template <bool kRmat>
int assemble_clouds(const float* part_pcs, const float* valids, const float* rot, const float* trans, const float* gt_rot,
                    const float* gt_trans, const float* colors, int64_t S, int64_t B, int64_t P, int64_t N, int64_t C,
                    int64_t* offsets, float* clouds, void* stream, const char* what) {
  MPA_REQUIRE(S >= 0 && B >= 0 && P >= 0 && N >= 0 && C >= 0, "%s: negative size", what);
  MPA_REQUIRE(C >= P, "%s: %lld colours for %lld part slots (a part is coloured by its rank, which can reach P - 1)", what,
              (long long)C, (long long)P);
  if (B == 0) return MPA_OK;
  MPA_REQUIRE(B * P < (1LL << 31) && S < (1LL << 31) && N <= 65535LL * kThreads, "%s: size too large", what);
  MPA_REQUIRE(valids && offsets, "%s: null pointer", what);
  const bool empty = P == 0 || N == 0;
  MPA_REQUIRE(empty || (part_pcs && gt_rot && gt_trans && colors && clouds && (S == 0 || (rot && trans))),
              "%s: null pointer", what);
  hipLaunchKernelGGL(cloud_offsets_kernel, dim3(1), dim3(kThreads), 0, mpa::as_stream(stream), valids, (int)B, (int)P,
                     (long long)N, offsets);
  if (!empty) {
    dim3 grid((unsigned)(B * P), (unsigned)((N + kThreads - 1) / kThreads), 1);
    hipLaunchKernelGGL(assemble_clouds_kernel<kRmat>, grid, dim3(kThreads), 0, mpa::as_stream(stream), part_pcs, valids,
                       rot, trans, gt_rot, gt_trans, colors, (int)S, (int)P, (int)N, (long long)(B * P), offsets, clouds);
  }
  return mpa::check_launch(what);
}

}  // namespace

extern "C" int mpa_assemble_clouds(const float* part_pcs, const float* valids, const float* quat, const float* trans,
                                   const float* gt_quat, const float* gt_trans, const float* colors, int64_t S, int64_t B,
                                   int64_t P, int64_t N, int64_t C, int64_t* offsets, float* clouds, void* stream) {
  return assemble_clouds<false>(part_pcs, valids, quat, trans, gt_quat, gt_trans, colors, S, B, P, N, C, offsets, clouds,
                                stream, "assemble_clouds");
}

extern "C" int mpa_assemble_clouds_rmat(const float* part_pcs, const float* valids, const float* rmat, const float* trans,
                                        const float* gt_rmat, const float* gt_trans, const float* colors, int64_t S,
                                        int64_t B, int64_t P, int64_t N, int64_t C, int64_t* offsets, float* clouds,
                                        void* stream) {
  return assemble_clouds<true>(part_pcs, valids, rmat, trans, gt_rmat, gt_trans, colors, S, B, P, N, C, offsets, clouds,
                               stream, "assemble_clouds_rmat");
}

extern "C" int mpa_mesh_pose_parts(const double* tri, const int64_t* part_face_off, int64_t parts_total,
                                   const int64_t* slot_part, const int64_t* out_face_off, int64_t M, int64_t faces_out,
                                   int64_t max_faces, const float* gt_rmat, const float* gt_trans, const float* pred_rmat,
                                   const float* pred_trans, float* orig, float* input, float* pred, void* stream) {
  MPA_REQUIRE(M >= 0 && parts_total >= 0 && faces_out >= 0 && max_faces >= 0, "mesh_pose_parts: negative size");
  if (M == 0 || faces_out == 0 || max_faces == 0) return MPA_OK;
  MPA_REQUIRE(M < (1LL << 31) && max_faces <= 65535LL * kThreads, "mesh_pose_parts: size too large");
  MPA_REQUIRE(tri && part_face_off && slot_part && out_face_off && gt_rmat && gt_trans && pred_rmat && pred_trans &&
                  orig && input && pred,
              "mesh_pose_parts: null pointer");
  dim3 grid((unsigned)M, (unsigned)((max_faces + kThreads - 1) / kThreads), 1);
  hipLaunchKernelGGL(mesh_pose_kernel, grid, dim3(kThreads), 0, mpa::as_stream(stream), tri, part_face_off, parts_total,
                     slot_part, out_face_off, faces_out, gt_rmat, gt_trans, pred_rmat, pred_trans, orig, input, pred);
  return mpa::check_launch("mesh_pose_parts");
}
