// Geometry batches sampled from device-resident meshes: `GeometryPartDataset._get_pcs` + `__getitem__`
// (multi_part_assembly/datasets/geometry_data.py:74-146) for a whole batch in one launch.
//
// One block per part slot.  Phase 1 draws N surface samples of the slot's part — datasets.sample_surface restated op by
// op: pick = u0 * cum[last]; face = first index with cum[face] >= pick (numpy's searchsorted, a binary search over the
// part's segment of cum_area); (a, b) = (u1, u2), reflected to (|a - 1|, |b - 1|) where a + b > 1; p = (e1 * a + e2 * b) +
// origin, every operation rounded once (this file is built with -ffp-contract=off) — into LDS, 24 B per point: the raw
// float64 cloud never goes through HBM unless the caller asks for it (raw_out).  Phase 2 is part_transform.h on that
// LDS cloud: the very code csrc/batch.hip runs on a cloud in global memory.
//
// Replay mode: the three uniforms per point, the rotation and the point order come from the host.  Device-random mode:
// Philox4x32-10, stateless — key = seed, counter = (i, purpose, stream_lo, stream_hi); see include/mpa_hip.h.
// Cost per point: ~log2(faces) dependent 8-B reads of cum_area (L2), one 72-B triangle row, 12 B written.
#include <math.h>

#include "common.h"
#include "part_transform.h"
#include "philox.h"

namespace {

constexpr int kThreads = mpa::kPartThreads;
constexpr int64_t kMaxPoints = 2048;  // 48 KiB of LDS for the cloud; loss.part_order has the same limit

using mpa::U4;
using mpa::philox4x32_10;  // philox.h

// numpy's random_sample construction: 53 bits from two words, the first one the high part; exact in float64.
__device__ __forceinline__ double uniform53(uint32_t hi, uint32_t lo) {
  return ((double)(hi >> 5) * 67108864.0 + (double)(lo >> 6)) * (1.0 / 9007199254740992.0);
}

// The slot's rotation in device-random mode, by one thread: unit quaternion (w, x, y, z) of the rotation applied to the
// points -> rot [9] row-major (LDS) and quat [4] = its inverse, scalar first, as `_rotate_pc` returns it.
__device__ __forceinline__ void draw_rotation(uint32_t k0, uint32_t k1, uint32_t s0, uint32_t s1, double rot_range,
                                              double* rot, float* quat) {
  const U4 c2 = philox4x32_10(U4{0u, 2u, s0, s1}, k0, k1), c3 = philox4x32_10(U4{0u, 3u, s0, s1}, k0, k1);
  const double r0 = uniform53(c2.x, c2.y), r1 = uniform53(c2.z, c2.w), r2 = uniform53(c3.x, c3.y);
  double w, x, y, z;
  if (rot_range > 0.0) {  // R.from_euler('xyz', (u - 0.5) * 2 * rot_range, degrees=True): extrinsic, q = qz * qy * qx
    double sa, ca, sb, cb, sc, cc;  // half angles, in units of pi: degrees / 360
    sincospi((r0 - 0.5) * 2.0 * rot_range / 360.0, &sa, &ca);
    sincospi((r1 - 0.5) * 2.0 * rot_range / 360.0, &sb, &cb);
    sincospi((r2 - 0.5) * 2.0 * rot_range / 360.0, &sc, &cc);
    w = cc * cb * ca + sc * sb * sa;
    x = cc * cb * sa - sc * sb * ca;
    y = cc * sb * ca + sc * cb * sa;
    z = sc * cb * ca - cc * sb * sa;
  } else {  // Shoemake, "Uniform random rotations" (Graphics Gems III): uniform on the unit quaternions
    double s1v, c1v, s2v, c2v;
    sincospi(2.0 * r1, &s1v, &c1v);
    sincospi(2.0 * r2, &s2v, &c2v);
    const double a = sqrt(1.0 - r0), b = sqrt(r0);
    x = a * s1v;
    y = a * c1v;
    z = b * s2v;
    w = b * c2v;
  }
  rot[0] = 1.0 - 2.0 * (y * y + z * z);
  rot[1] = 2.0 * (x * y - z * w);
  rot[2] = 2.0 * (x * z + y * w);
  rot[3] = 2.0 * (x * y + z * w);
  rot[4] = 1.0 - 2.0 * (x * x + z * z);
  rot[5] = 2.0 * (y * z - x * w);
  rot[6] = 2.0 * (x * z - y * w);
  rot[7] = 2.0 * (y * z + x * w);
  rot[8] = 1.0 - 2.0 * (x * x + y * y);
  quat[0] = (float)w;
  quat[1] = (float)-x;
  quat[2] = (float)-y;
  quat[3] = (float)-z;
}

// grid = M part slots, block 256, dynamic LDS = 24 N bytes.  kReplay: uniforms / rot / perm from the host; otherwise
// Philox draws keyed by (seed, stream_id[m]).
template <bool kReplay>
__global__ __launch_bounds__(kThreads) void mesh_sample_kernel(
    const double* __restrict__ tri, const double* __restrict__ cum_area, const int64_t* __restrict__ part_face_off,
    int64_t parts_total, const int64_t* __restrict__ slot_part, int N, const double* __restrict__ uniforms,
    const double* __restrict__ rot, const int* __restrict__ perm, uint64_t seed, const int64_t* __restrict__ stream_id,
    double rot_range, float* __restrict__ part_pcs, float* __restrict__ part_trans, float* __restrict__ part_quat,
    double* __restrict__ raw_out) {
  extern __shared__ __align__(16) double pts[];  // [N][3]
  __shared__ double rot_lds[9];
  const int m = blockIdx.x, t = threadIdx.x;
  float* out = part_pcs + 3LL * m * N;
  double* raw = raw_out ? raw_out + 3LL * m * N : nullptr;
  const int64_t part = slot_part[m];
  int64_t f0 = 0, F = 0;
  if (part >= 0 && part < parts_total) {
    f0 = part_face_off[part];
    F = part_face_off[part + 1] - f0;
  }
  if (F <= 0) {  // padded slot (or a part id outside the store: never read past the tables)
    mpa::part_zero_fill(N, out, part_trans + 3 * m);
    if (part_quat && t < 4) part_quat[4 * m + t] = 0.0f;
    if (raw)
      for (int i = t; i < 3 * N; i += kThreads) raw[i] = 0.0;
    return;
  }
  const double* cum = cum_area + f0;
  const double* tr = tri + 9 * f0;
  const double total = cum[F - 1];
  uint32_t k0 = 0, k1 = 0, s0 = 0, s1 = 0;
  if (!kReplay) {
    const uint64_t s = (uint64_t)stream_id[m];
    k0 = (uint32_t)seed;
    k1 = (uint32_t)(seed >> 32);
    s0 = (uint32_t)s;
    s1 = (uint32_t)(s >> 32);
    if (t == 0) draw_rotation(k0, k1, s0, s1, rot_range, rot_lds, part_quat + 4 * m);
  }
  for (int i = t; i < N; i += kThreads) {
    double u0, a, b;
    if (kReplay) {
      const double* u = uniforms + 3 * ((long long)m * N + i);
      u0 = u[0];
      a = u[1];
      b = u[2];
    } else {
      const U4 c0 = philox4x32_10(U4{(uint32_t)i, 0u, s0, s1}, k0, k1);
      const U4 c1 = philox4x32_10(U4{(uint32_t)i, 1u, s0, s1}, k0, k1);
      u0 = uniform53(c0.x, c0.y);
      a = uniform53(c0.z, c0.w);
      b = uniform53(c1.x, c1.y);
    }
    const double pick = u0 * total;
    int64_t lo = 0, hi = F;  // first index with cum[index] >= pick
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (cum[mid] < pick) lo = mid + 1;
      else hi = mid;
    }
    if (lo > F - 1) lo = F - 1;  // cannot happen for u0 < 1; keeps a bad replay uniform inside the table
    if (a + b > 1.0) {
      a = fabs(a - 1.0);
      b = fabs(b - 1.0);
    }
    const double* f = tr + 9 * lo;
    const double px = (f[3] * a + f[6] * b) + f[0];
    const double py = (f[4] * a + f[7] * b) + f[1];
    const double pz = (f[5] * a + f[8] * b) + f[2];
    pts[3 * i + 0] = px;
    pts[3 * i + 1] = py;
    pts[3 * i + 2] = pz;
    if (raw) {
      raw[3 * i + 0] = px;
      raw[3 * i + 1] = py;
      raw[3 * i + 2] = pz;
    }
  }
  __syncthreads();
  if (kReplay)
    mpa::part_transform_block<true>(pts, rot + 9LL * m, perm + (long long)m * N, N, out, part_trans + 3 * m);
  else
    mpa::part_transform_block<false>(pts, rot_lds, nullptr, N, out, part_trans + 3 * m);
}

// The [B, P] slot table of a batch whose shape indices live in device memory: one thread per slot.  A shape index outside
// [0, S) (status 1) or a part count outside [min_part, max_part] (status 2) marks every slot of that shape padded; for a
// bad index nothing of shape_part_off is read.
__global__ __launch_bounds__(kThreads) void mesh_slot_table_kernel(
    const int64_t* __restrict__ shape_part_off, int64_t S, const int64_t* __restrict__ shape_index, int64_t M, int P,
    int min_part, int max_part, uint64_t stream_base, int64_t* __restrict__ slot_part, int64_t* __restrict__ stream_id,
    float* __restrict__ valids, float* __restrict__ part_ids, int32_t* __restrict__ status) {
  const int64_t m = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (m >= M) return;
  const int64_t b = m / P;
  const int j = (int)(m % P);
  const int64_t s = shape_index[b];
  int64_t start = 0, count = 0;
  int bad = 0;
  if (s < 0 || s >= S) {
    bad = 1;
  } else {
    start = shape_part_off[s];
    count = shape_part_off[s + 1] - start;
    if (count < min_part || count > max_part) {
      bad = 2;
      count = 0;
    }
  }
  if (bad && j == 0) *status = bad;
  const bool live = j < count;
  slot_part[m] = live ? start + j : -1;
  stream_id[m] = (int64_t)(stream_base + (uint64_t)m);
  valids[m] = live ? 1.0f : 0.0f;
  part_ids[m] = live ? (float)j : 0.0f;
}

}  // namespace

extern "C" int mpa_mesh_slot_table(const int64_t* shape_part_off, int64_t S, const int64_t* shape_index, int64_t B,
                                   int64_t P, int64_t min_part, int64_t max_part, uint64_t stream_base,
                                   int64_t* slot_part, int64_t* stream_id, float* valids, float* part_ids,
                                   int32_t* status, void* stream) {
  MPA_REQUIRE(B >= 0 && S >= 0 && B <= (1LL << 24), "mesh_slot_table: negative or oversized B / S (B <= 2^24)");
  MPA_REQUIRE(P >= 1 && P <= 4096, "mesh_slot_table: P=%lld outside [1, 4096]", (long long)P);
  MPA_REQUIRE(min_part >= 0 && min_part <= max_part && max_part <= P,
              "mesh_slot_table: part limits [%lld, %lld] do not fit the %lld slots of a shape", (long long)min_part,
              (long long)max_part, (long long)P);
  if (B == 0) return MPA_OK;
  MPA_REQUIRE(shape_part_off && shape_index && slot_part && stream_id && valids && part_ids && status,
              "mesh_slot_table: null pointer");
  const int64_t M = B * P;
  hipLaunchKernelGGL(mesh_slot_table_kernel, dim3((unsigned)((M + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                     mpa::as_stream(stream), shape_part_off, S, shape_index, M, (int)P, (int)min_part, (int)max_part,
                     stream_base, slot_part, stream_id, valids, part_ids, status);
  return mpa::check_launch("mesh_slot_table");
}

extern "C" int mpa_mesh_sample_batch(const double* tri, const double* cum_area, const int64_t* part_face_off,
                                     int64_t parts_total, const int64_t* slot_part, int64_t M, int64_t N,
                                     const double* uniforms, const double* rot, const int32_t* perm, uint64_t seed,
                                     const int64_t* stream_id, double rot_range, float* part_pcs, float* part_trans,
                                     float* part_quat, double* raw_out, void* stream) {
  MPA_REQUIRE(M >= 0 && M <= (1LL << 30) && parts_total >= 0, "mesh_sample_batch: negative or oversized M / parts_total");
  MPA_REQUIRE(N >= 1 && N <= kMaxPoints, "mesh_sample_batch: N=%lld outside [1, %lld] (the sampled cloud lives in LDS)",
              (long long)N, (long long)kMaxPoints);
  if (M == 0) return MPA_OK;
  MPA_REQUIRE(tri && cum_area && part_face_off && slot_part && part_pcs && part_trans,
              "mesh_sample_batch: null pointer");
  const size_t lds = (size_t)N * 3 * sizeof(double);
  if (uniforms) {
    MPA_REQUIRE(rot && perm, "mesh_sample_batch: null pointer (replay mode needs uniforms, rot and perm)");
    hipLaunchKernelGGL(mesh_sample_kernel<true>, dim3((unsigned)M), dim3(kThreads), lds, mpa::as_stream(stream), tri,
                       cum_area, part_face_off, parts_total, slot_part, (int)N, uniforms, rot, perm, seed, stream_id,
                       rot_range, part_pcs, part_trans, part_quat, raw_out);
  } else {
    MPA_REQUIRE(!rot && !perm, "mesh_sample_batch: rot / perm without uniforms (replay mode needs all three)");
    MPA_REQUIRE(stream_id && part_quat, "mesh_sample_batch: null pointer (device-random mode needs stream_id and part_quat)");
    hipLaunchKernelGGL(mesh_sample_kernel<false>, dim3((unsigned)M), dim3(kThreads), lds, mpa::as_stream(stream), tri,
                       cum_area, part_face_off, parts_total, slot_part, (int)N, uniforms, rot, perm, seed, stream_id,
                       rot_range, part_pcs, part_trans, part_quat, raw_out);
  }
  return mpa::check_launch("mesh_sample_batch");
}
