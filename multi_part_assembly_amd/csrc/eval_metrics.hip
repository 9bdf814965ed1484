// Evaluation metrics of one batch in two launches (+ one for the connectivity accuracy) — replaces the composition of
// library operators behind `BaseModel._calc_metrics` (reference: multi_part_assembly/utils/eval_utils.py:12-199,
// models/modules/base_model.py:316-339): two posed [B,P,N,3] clouds, the Chamfer operator, means and comparisons for
// `calc_part_acc`; three `trans_metrics` and three `rot_metrics` calls, each of the latter converting both rotations to
// Euler angles again; `_valid_mean` behind each — on the order of a hundred launches of a few microseconds.
//
//   slot_metrics_kernel   one 256-thread block per part slot (b, p).  The part's N points are read once, posed by the
//                         predicted and by the ground-truth pose with the inline functions of quat.h / mat3.h (the
//                         arithmetic of pose.hip / rmat.hip, so the coordinates are those of `pose_apply`), and both
//                         posed clouds stay in LDS (24 N bytes: 24 KB at N = 1000).  Every thread then holds up to four
//                         queries at a time and walks the other cloud through wave-uniform (broadcast) LDS reads with
//                         the distance form of chamfer_core.h, d = (dx*dx + dy*dy) + dz*dz, every operation rounded:
//                         the minima are the distances of mpa_chamfer_forward, bit for bit (only the minimum VALUE is
//                         needed, so no index is tracked).  The per-part Chamfer value is
//                             sum_i dist1[i] / N + sum_j dist2[j] / N
//                         with a fixed summation shape: <= 8 terms per thread in index order, the DPP wave sum of
//                         common.h, the four wave sums in wave order.  At most 8 + 6 + 3 additions lie on any path, one
//                         division and one more addition: <= 20 fp32 roundings of positive terms, a relative error of
//                         at most 20 * 2^-24 = 1.2e-6 against the exact mean of the same distances.
//                         Thread 0 computes the slot's translation and Euler-angle errors in float64 from the float32
//                         inputs (the 'zyx' formula of eval_utils.quat_to_euler_zyx_deg, degrees, min(d, 360 - d);
//                         rotation matrices first go through pytorch3d's matrix_to_quaternion, as Rotation3D.to_quat
//                         does) and stores them.  A slot with valids == 0 touches none of its points or poses and
//                         stores zeros.
//   batch_metrics_kernel  one thread per (metric, b): the reference's `_valid_mean` — sum_p value * valids / sum_p valids —
//                         over p in index order, accumulated in float64 and rounded once; part_acc is the integer count of
//                         correct valid parts over the integer count of valid parts (valid: valids == 1).
//   connectivity_kernel   ONE block: every (b, i, j) with contact_points[b,i,j,0] == 1 poses the 8 sign-flipped copies of
//                         its two contact points and takes the minimum of the 64 squared distances; hits and contacts are
//                         integer counters in LDS, the quotient is tiled to [B] (0 / 0 = NaN, as the composition gives).
//
// No atomics on floats, no memset / memcpy nodes, fixed reduction order: two runs give the same bits.
#include "chamfer_core.h"
#include "common.h"
#include "mat3.h"
#include "quat.h"

namespace {

using mpa::f32x2;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / mpa::kWave;
constexpr int kQ = 4;          // queries per thread and sweep of the other cloud
constexpr int kMaxPoints = 2048;  // both posed clouds in LDS: 24 * 2048 = 48 KB
constexpr int kSlotRows = 7;   // part_acc flag, trans mse / rmse / mae, rot mse / rmse / mae

// This thread's sum of min_j d(query_i, target_j) over its queries i = t, t + 256, ... (index order).
__device__ __forceinline__ float nn_sum(const float* __restrict__ qs, const float* __restrict__ ts, int N) {
  const int t = threadIdx.x;
  float total = 0.0f;
  for (int base = 0; base < N; base += kQ * kThreads) {
    f32x2 X[kQ / 2], Y[kQ / 2], Z[kQ / 2], best[kQ / 2];
    bool live[kQ];
#pragma unroll
    for (int q = 0; q < kQ; ++q) {
      const int i = base + q * kThreads + t;
      live[q] = i < N;
      const int ii = live[q] ? i : 0;
      X[q >> 1][q & 1] = qs[3 * ii + 0];
      Y[q >> 1][q & 1] = qs[3 * ii + 1];
      Z[q >> 1][q & 1] = qs[3 * ii + 2];
      best[q >> 1][q & 1] = 1e32f;  // chamfer_kernel.cu:60
    }
    const float4* __restrict__ t4 = reinterpret_cast<const float4*>(ts);
    int j = 0;
    for (; j + 4 <= N; j += 4) {  // 4 targets = 12 floats = 3 broadcast ds_read_b128
      const float4 a = t4[3 * (j >> 2) + 0], b = t4[3 * (j >> 2) + 1], c = t4[3 * (j >> 2) + 2];
      const float tx[4] = {a.x, a.w, b.z, c.y}, ty[4] = {a.y, b.x, b.w, c.z}, tz[4] = {a.z, b.y, c.x, c.w};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
#pragma unroll
        for (int h = 0; h < kQ / 2; ++h) {
          const f32x2 d = mpa::dist_exact_v(X[h] - tx[k], Y[h] - ty[k], Z[h] - tz[k]);
          best[h][0] = d[0] < best[h][0] ? d[0] : best[h][0];
          best[h][1] = d[1] < best[h][1] ? d[1] : best[h][1];
        }
      }
    }
    for (; j < N; ++j) {
      const float sx = ts[3 * j + 0], sy = ts[3 * j + 1], sz = ts[3 * j + 2];
#pragma unroll
      for (int h = 0; h < kQ / 2; ++h) {
        const f32x2 d = mpa::dist_exact_v(X[h] - sx, Y[h] - sy, Z[h] - sz);
        best[h][0] = d[0] < best[h][0] ? d[0] : best[h][0];
        best[h][1] = d[1] < best[h][1] ? d[1] : best[h][1];
      }
    }
#pragma unroll
    for (int q = 0; q < kQ; ++q)
      if (live[q]) total += best[q >> 1][q & 1];
  }
  return total;
}

// Block sum in a fixed order: DPP wave sums, then the waves in order.  `red` holds kWaves floats.
__device__ __forceinline__ float block_sum(float v, float* red) {
  const float w = mpa::wave_sum_dpp(v);
  __syncthreads();  // (red may still be read from the previous sum)
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = w;
  __syncthreads();
  float s = red[0];
#pragma unroll
  for (int k = 1; k < kWaves; ++k) s += red[k];
  return s;
}

// pytorch3d's matrix_to_quaternion (real part first, made non-negative) followed by Rotation3D's constructor rule
// (norm <= 0.5 -> identity), in float64.
__device__ void matrix_to_quat(const float* __restrict__ m, double* q) {
  const double m00 = m[0], m01 = m[1], m02 = m[2], m10 = m[3], m11 = m[4], m12 = m[5], m20 = m[6], m21 = m[7], m22 = m[8];
  const double s[4] = {1.0 + m00 + m11 + m22, 1.0 + m00 - m11 - m22, 1.0 - m00 + m11 - m22, 1.0 - m00 - m11 + m22};
  double qa[4];
  int best = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    qa[k] = s[k] > 0.0 ? sqrt(s[k]) : 0.0;
    if (qa[k] > qa[best]) best = k;  // first maximum, as argmax
  }
  const double c0[4] = {qa[0] * qa[0], m21 - m12, m02 - m20, m10 - m01};
  const double c1[4] = {m21 - m12, qa[1] * qa[1], m10 + m01, m02 + m20};
  const double c2[4] = {m02 - m20, m10 + m01, qa[2] * qa[2], m12 + m21};
  const double c3[4] = {m10 - m01, m20 + m02, m21 + m12, qa[3] * qa[3]};
  const double den = 2.0 * fmax(qa[best], 0.1);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double c = best == 0 ? c0[k] : best == 1 ? c1[k] : best == 2 ? c2[k] : c3[k];
    q[k] = c / den;
  }
  if (q[0] < 0.0) {
#pragma unroll
    for (int k = 0; k < 4; ++k) q[k] = -q[k];
  }
  if (!(sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]) > 0.5)) {
    q[0] = 1.0;
    q[1] = q[2] = q[3] = 0.0;
  }
}

// eval_utils.quat_to_euler_zyx_deg: (w, x, y, z) as given (nothing is normalised) -> degrees.
__device__ void quat_to_euler_deg(const double* q, double* e) {
  const double w = q[0], x = q[1], y = q[2], z = q[3];
  const double kPi = 3.14159265358979323846;
  e[0] = atan2(2.0 * (w * x + y * z), 1.0 - 2.0 * (x * x + y * y)) * 180.0 / kPi;
  e[1] = asin(fmin(fmax(2.0 * (w * y - x * z), -1.0), 1.0)) * 180.0 / kPi;
  e[2] = atan2(2.0 * (w * z + x * y), 1.0 - 2.0 * (y * y + z * z)) * 180.0 / kPi;
}

// mse / rmse / mae of three error components -> out[0..2]
__device__ void three_means(const double* d, double* out) {
  const double mse = (d[0] * d[0] + d[1] * d[1] + d[2] * d[2]) / 3.0;
  out[0] = mse;
  out[1] = sqrt(mse);
  out[2] = (fabs(d[0]) + fabs(d[1]) + fabs(d[2])) / 3.0;
}

template <bool kRmat>
__global__ __launch_bounds__(kThreads) void slot_metrics_kernel(
    const float* __restrict__ pcs, const float* __restrict__ trans_pred, const float* __restrict__ trans_gt,
    const float* __restrict__ rot_pred, const float* __restrict__ rot_gt, const float* __restrict__ valids, int N,
    long long slots, double* __restrict__ slot_out, float* __restrict__ per_part) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  __shared__ float red[kWaves];
  const long long m = blockIdx.x;
  const int t = threadIdx.x;
  if (valids[m] == 0.0f) {  // padded slot: its points and poses are never read
    if (t < kSlotRows) slot_out[t * slots + m] = 0.0;
    if (t == 0 && per_part != nullptr) per_part[m] = 0.0f;
    return;
  }
  const int n3 = (3 * N + 3) & ~3;  // second cloud starts 16-byte aligned
  float* __restrict__ cp = lds;
  float* __restrict__ cg = lds + n3;
  constexpr int kRot = kRmat ? 9 : 4;
  const float* rp = rot_pred + kRot * m;
  const float* rg = rot_gt + kRot * m;
  const float tp[3] = {trans_pred[3 * m + 0], trans_pred[3 * m + 1], trans_pred[3 * m + 2]};
  const float tg[3] = {trans_gt[3 * m + 0], trans_gt[3 * m + 1], trans_gt[3 * m + 2]};
  {
    const float* __restrict__ src = pcs + 3 * m * N;
    mpa::Mat3 mp, mg;
    mpa::Quat qp{1.0f, 0.0f, 0.0f, 0.0f}, qg{1.0f, 0.0f, 0.0f, 0.0f};
    if constexpr (kRmat) {
      mp = mpa::load_mat3(rp);
      mg = mpa::load_mat3(rg);
    } else {
      qp = mpa::Quat{rp[0], rp[1], rp[2], rp[3]};
      qg = mpa::Quat{rg[0], rg[1], rg[2], rg[3]};
    }
    for (int i = t; i < N; i += kThreads) {
      const float px = src[3 * i + 0], py = src[3 * i + 1], pz = src[3 * i + 2];
      float ax, ay, az, bx, by, bz;
      if constexpr (kRmat) {
        mpa::mat3_rotate(mp, px, py, pz, ax, ay, az);
        mpa::mat3_rotate(mg, px, py, pz, bx, by, bz);
      } else {
        mpa::quat_rotate(qp, px, py, pz, ax, ay, az);
        mpa::quat_rotate(qg, px, py, pz, bx, by, bz);
      }
      cp[3 * i + 0] = ax + tp[0];
      cp[3 * i + 1] = ay + tp[1];
      cp[3 * i + 2] = az + tp[2];
      cg[3 * i + 0] = bx + tg[0];
      cg[3 * i + 1] = by + tg[1];
      cg[3 * i + 2] = bz + tg[2];
    }
  }
  __syncthreads();
  const float s1 = block_sum(nn_sum(cp, cg, N), red);  // dist1: predicted cloud queries the ground-truth cloud
  const float s2 = block_sum(nn_sum(cg, cp, N), red);
  if (t != 0) return;
  const float cd = s1 / (float)N + s2 / (float)N;
  if (per_part != nullptr) per_part[m] = cd;
  double row[kSlotRows];
  row[0] = cd < 0.01f ? 1.0 : 0.0;
  const double dt[3] = {(double)tp[0] - (double)tg[0], (double)tp[1] - (double)tg[1], (double)tp[2] - (double)tg[2]};
  three_means(dt, row + 1);
  double qa[4], qb[4], ea[3], eb[3], de[3];
  if constexpr (kRmat) {
    matrix_to_quat(rp, qa);
    matrix_to_quat(rg, qb);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      qa[k] = rp[k];
      qb[k] = rg[k];
    }
  }
  quat_to_euler_deg(qa, ea);
  quat_to_euler_deg(qb, eb);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double d = fabs(ea[k] - eb[k]);
    de[k] = fmin(d, 360.0 - d);
  }
  three_means(de, row + 4);
#pragma unroll
  for (int k = 0; k < kSlotRows; ++k) slot_out[k * slots + m] = row[k];
}

__global__ __launch_bounds__(kThreads) void batch_metrics_kernel(const double* __restrict__ slot, const float* __restrict__ valids,
                                                                 int B, int P, float* __restrict__ out) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= kSlotRows * B) return;
  const int k = i / B, b = i % B;
  const double* __restrict__ row = slot + ((long long)k * B + b) * P;
  const float* __restrict__ v = valids + (long long)b * P;
  if (k == 0) {
    int ok = 0, n = 0;
    for (int p = 0; p < P; ++p) {
      const bool valid = v[p] == 1.0f;
      n += valid;
      ok += valid && row[p] != 0.0;
    }
    out[i] = (float)ok / (float)n;
    return;
  }
  double s = 0.0, vs = 0.0;
  for (int p = 0; p < P; ++p) {
    s += row[p] * (double)v[p];
    vs += (double)v[p];
  }
  out[i] = (float)(s / vs);
}

__device__ __forceinline__ void pose_point(const float* __restrict__ rot, const float* __restrict__ tr, bool rmat, float px,
                                           float py, float pz, float* o) {
  float x, y, z;
  if (rmat) {
    mpa::mat3_rotate(mpa::load_mat3(rot), px, py, pz, x, y, z);
  } else {
    mpa::quat_rotate(mpa::Quat{rot[0], rot[1], rot[2], rot[3]}, px, py, pz, x, y, z);
  }
  o[0] = x + tr[0];
  o[1] = y + tr[1];
  o[2] = z + tr[2];
}

constexpr int kConnThreads = 1024;

__global__ __launch_bounds__(kConnThreads) void connectivity_kernel(const float* __restrict__ contact, const float* __restrict__ trans,
                                                                    const float* __restrict__ rot, int rmat, int B, int P,
                                                                    float* __restrict__ out) {
  __shared__ int counts[2];  // contacts, hits
  if (threadIdx.x < 2) counts[threadIdx.x] = 0;
  __syncthreads();
  const int rs = rmat ? 9 : 4;
  const long long total = (long long)B * P * P;
  int contacts = 0, hits = 0;
  for (long long e = threadIdx.x; e < total; e += kConnThreads) {
    if (contact[4 * e] != 1.0f) continue;
    const int j = (int)(e % P), i = (int)((e / P) % P);
    const long long b = e / ((long long)P * P);
    const long long pi = b * P + i, pj = b * P + j;
    const float* c1 = contact + 4 * e + 1;
    const float* c2 = contact + 4 * ((b * P + j) * P + i) + 1;
    float a[8][3];
#pragma unroll
    for (int s = 0; s < 8; ++s)
      pose_point(rot + rs * pi, trans + 3 * pi, rmat != 0, (s & 4) ? -c1[0] : c1[0], (s & 2) ? -c1[1] : c1[1],
                 (s & 1) ? -c1[2] : c1[2], a[s]);
    float best = __builtin_inff();
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      float q[3];
      pose_point(rot + rs * pj, trans + 3 * pj, rmat != 0, (s & 4) ? -c2[0] : c2[0], (s & 2) ? -c2[1] : c2[1],
                 (s & 1) ? -c2[2] : c2[2], q);
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        const float d = mpa::dist_exact_f(a[r][0] - q[0], a[r][1] - q[1], a[r][2] - q[2]);
        best = d < best ? d : best;
      }
    }
    contacts += 1;
    hits += best < 0.01f;
  }
  if (contacts != 0) {  // integer counters: the order of the additions does not matter
    atomicAdd(&counts[0], contacts);
    atomicAdd(&counts[1], hits);
  }
  __syncthreads();
  const float acc = (float)counts[1] / (float)counts[0];
  for (int b = threadIdx.x; b < B; b += kConnThreads) out[b] = acc;
}

// the metrics' workspace: the per-slot rows [kSlotRows][B * P] of doubles
double* metrics_carve(mpa::Arena& a, int64_t B, int64_t P) { return a.take<double>(kSlotRows * B * P, 8); }

template <bool kRmat>
int assembly_metrics(const float* part_pcs, const float* trans_pred, const float* trans_gt, const float* rot_pred,
                     const float* rot_gt, const float* valids, int64_t B, int64_t P, int64_t N, void* workspace, float* out,
                     float* per_part, void* stream) {
  MPA_REQUIRE(B >= 0 && P >= 0 && N >= 0, "assembly_metrics: negative size");
  if (B == 0) return MPA_OK;
  MPA_REQUIRE(P >= 1 && N >= 1 && N <= kMaxPoints, "assembly_metrics: need P >= 1 and 1 <= N <= %d points per part (N=%lld)",
              kMaxPoints, (long long)N);
  MPA_REQUIRE(B * P < (1LL << 31) / kSlotRows, "assembly_metrics: too many part slots");
  MPA_REQUIRE(part_pcs && trans_pred && trans_gt && rot_pred && rot_gt && valids && workspace && out,
              "assembly_metrics: null pointer");
  MPA_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "assembly_metrics: workspace must be 8-byte aligned");
  mpa::Arena arena(workspace);
  double* slot = metrics_carve(arena, B, P);
  const size_t lds = 2 * sizeof(float) * (size_t)((3 * N + 3) & ~3LL);
  hipLaunchKernelGGL(slot_metrics_kernel<kRmat>, dim3((unsigned)(B * P)), dim3(kThreads), lds, mpa::as_stream(stream), part_pcs,
                     trans_pred, trans_gt, rot_pred, rot_gt, valids, (int)N, (long long)(B * P), slot, per_part);
  int st = mpa::check_launch("assembly_metrics (slots)");
  if (st != MPA_OK) return st;
  hipLaunchKernelGGL(batch_metrics_kernel, dim3((unsigned)((kSlotRows * B + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                     mpa::as_stream(stream), slot, valids, (int)B, (int)P, out);
  return mpa::check_launch("assembly_metrics (batch)");
}

}  // namespace

extern "C" int mpa_assembly_metrics_workspace(int64_t B, int64_t P, int64_t* bytes) {
  MPA_REQUIRE(bytes != nullptr, "assembly_metrics_workspace: null pointer");
  MPA_REQUIRE(B >= 0 && P >= 0 && B * P < (1LL << 31) / kSlotRows, "assembly_metrics_workspace: bad size");
  mpa::Arena a(nullptr);
  metrics_carve(a, B, P);
  *bytes = a.bytes();
  return MPA_OK;
}

extern "C" int mpa_assembly_metrics(const float* part_pcs, const float* trans_pred, const float* trans_gt,
                                    const float* quat_pred, const float* quat_gt, const float* valids, int64_t B, int64_t P,
                                    int64_t N, void* workspace, float* out, float* per_part, void* stream) {
  return assembly_metrics<false>(part_pcs, trans_pred, trans_gt, quat_pred, quat_gt, valids, B, P, N, workspace, out, per_part,
                                 stream);
}

extern "C" int mpa_assembly_metrics_rmat(const float* part_pcs, const float* trans_pred, const float* trans_gt,
                                         const float* rmat_pred, const float* rmat_gt, const float* valids, int64_t B,
                                         int64_t P, int64_t N, void* workspace, float* out, float* per_part, void* stream) {
  return assembly_metrics<true>(part_pcs, trans_pred, trans_gt, rmat_pred, rmat_gt, valids, B, P, N, workspace, out, per_part,
                                stream);
}

extern "C" int mpa_connectivity_acc(const float* contact_points, const float* trans, const float* rot, int is_rmat, int64_t B,
                                    int64_t P, float* out, void* stream) {
  MPA_REQUIRE(B >= 0 && P >= 0, "connectivity_acc: negative size");
  if (B == 0) return MPA_OK;
  MPA_REQUIRE(P >= 1 && B * P * P < (1LL << 31), "connectivity_acc: need P >= 1 and B * P * P < 2^31");
  MPA_REQUIRE(contact_points && trans && rot && out, "connectivity_acc: null pointer");
  hipLaunchKernelGGL(connectivity_kernel, dim3(1), dim3(kConnThreads), 0, mpa::as_stream(stream), contact_points, trans, rot,
                     is_rmat, (int)B, (int)P, out);
  return mpa::check_launch("connectivity_acc");
}
