// PartNet batches gathered from a device-resident store: `PartNetPartDataset.__getitem__` + the default collate
// (multi_part_assembly/datasets/partnet_data.py:127-243) for a whole batch in one launch.  include/mpa_hip.h has the
// contract; datasets.PartNetStore packs the arrays and validates them, so the kernel trusts the STORE (offsets, part
// counts) and checks what reaches it from device memory at call time: the shape indices and a replayed part order.
//
// Grid = B * (P + 1) blocks of 256 threads.  Every block first resolves its sample in wave 0: the shape's part range, and
// the part order — identity, the caller's row, or a Fisher-Yates shuffle whose permutation lives one entry per lane and is
// swapped with lane reads (no LDS, no dependent memory access: <= 63 steps of a handful of VALU instructions).  Block
// (b, j), j < P, then moves slot j: the 12 N bytes of the cloud with 16-byte accesses when N % 4 == 0 (and the pointers
// allow it), with dword accesses otherwise, plus the pose and the symmetry row; a padded slot is written as zeros.  Block
// (b, P) derives the sample's labels from the <= 64 ordered ids in wave 0 (lane reads again: no atomics, fixed order) and
// writes every label output and the contact block.  Every byte of every requested output is written on every call.
#include "common.h"
#include "philox.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxParts = 64;                // one lane per part
constexpr uint32_t kPurpose = 0x706E0000u;   // counter word 1 = kPurpose | block: the mesh sampler's is < 4, the match
                                             // sampler's 0x6D61xxxx

struct GatherArgs {
  const float* pcs;
  const float* poses;
  const float* sym;
  const int32_t* geo_ids;
  const int32_t* sem_ids;
  const int64_t* shape_part_off;
  const int64_t* shape_ids;
  const float* contacts;
  const int64_t* contact_off;
  int64_t S;
  const int64_t* shape_index;
  int P, N, C;
  const int32_t* perm;
  int random_order;
  uint32_t k0, k1;
  uint64_t counter;
  const uint64_t* counter_dev;
  float* part_pcs;
  float* part_trans;
  float* part_quat;
  float* part_valids;
  float* part_ids;
  float* instance_label;
  float* match_ids;
  float* part_label;
  float* contact_points;
  float* sym_out;
  float* valid_matrix;
  int64_t* shape_id;
  int32_t* order_out;
  int32_t* status;
};

__device__ __forceinline__ int lane_read(int v, int lane) { return __builtin_amdgcn_readlane(v, lane); }

template <bool kVec4>
__global__ __launch_bounds__(kThreads) void partnet_gather_kernel(const GatherArgs a) {
  __shared__ int s_order[kMaxParts];   // stored part of slot j (j < p)
  __shared__ int s_rank[kMaxParts];    // equal ids before slot j
  __shared__ int s_match[kMaxParts];   // match id of slot j
  __shared__ int s_geo[kMaxParts];
  __shared__ int s_sem[kMaxParts];
  __shared__ int s_p;
  __shared__ long long s_start, s_shape;
  const int t = threadIdx.x, P = a.P, N = a.N, C = a.C;
  const int b = blockIdx.x / (P + 1), slot = blockIdx.x % (P + 1);
  const bool label_block = slot == P;

  if (t < mpa::kWave) {  // wave 0: the sample's part range and part order
    const long long s = a.shape_index[b];
    long long start = 0;
    int p = 0;
    int bad = 0;
    if (s < 0 || s >= a.S) {
      bad = 1;  // a checked input: nothing of the store is read for it
    } else {
      start = a.shape_part_off[s];
      const long long cnt = a.shape_part_off[s + 1] - start;
      p = cnt < 0 ? 0 : (cnt > P ? P : (int)cnt);  // (the store's limits make this the identity)
    }
    int order = t;
    if (a.perm != nullptr) {  // replay: the row must permute 0..p-1, or the sample is refused like a bad index
      const int o = t < p ? a.perm[(long long)b * P + t] : t;
      const bool in_range = o >= 0 && o < p;
      int dup = 0;
      for (int i = 0; i < p; ++i) dup |= (i < t && lane_read(o, i) == o) ? 1 : 0;
      if (__any((t < p && (!in_range || dup)) ? 1 : 0)) {
        bad = 2;
        p = 0;
      }
      order = o;
    } else if (a.random_order && p > 1) {
      const uint64_t c = a.counter_dev != nullptr ? *a.counter_dev : a.counter;
      const mpa::U4 r = mpa::philox4x32_10(
          mpa::U4{(uint32_t)b, kPurpose | (uint32_t)(t >> 2), (uint32_t)c, (uint32_t)(c >> 32)}, a.k0, a.k1);
      const int q = t & 3;
      const uint32_t w = q == 0 ? r.x : q == 1 ? r.y : q == 2 ? r.z : r.w;  // lane k holds w_k
      for (int k = 0; k + 1 < p; ++k) {
        const uint32_t wk = (uint32_t)lane_read((int)w, k);
        const int j = k + (int)__umulhi(wk, (uint32_t)(p - k));  // k <= j < p, wave-uniform
        const int vk = lane_read(order, k), vj = lane_read(order, j);
        order = t == k ? vj : (t == j ? vk : order);
      }
    }
    if (bad && t == 0 && label_block) *a.status = bad;
    if (t == 0) {
      s_p = p;
      s_start = start;
      s_shape = bad ? -1 : s;
    }
    const bool live = t < p;
    s_order[t] = live ? order : -1;
    if (label_block) {
      const int g = live && a.geo_ids != nullptr ? a.geo_ids[start + order] : 0;
      int rank = 0, count = 0;
      for (int i = 0; i < p; ++i) {
        const int same = lane_read(g, i) == g ? 1 : 0;
        count += same;
        rank += (i < t) ? same : 0;
      }
      // a group: an id >= 1 held by two parts or more; its number is 1 + the groups with a smaller id
      const int leads = (live && g >= 1 && count >= 2 && rank == 0) ? 1 : 0;
      int label = 1;
      for (int i = 0; i < p; ++i) label += (lane_read(leads, i) && lane_read(g, i) < g) ? 1 : 0;
      s_geo[t] = g;
      s_rank[t] = live ? rank : -1;
      s_match[t] = (live && g >= 1 && count >= 2) ? label : 0;
      s_sem[t] = live && a.sem_ids != nullptr && C > 0 ? a.sem_ids[start + order] : 0;
    }
  }
  __syncthreads();
  const int p = s_p;
  const long long start = s_start;

  if (!label_block) {  // ---- slot (b, slot): cloud, pose, symmetry ----
    const long long m = (long long)b * P + slot;
    const bool live = slot < p;
    const long long part = live ? start + s_order[slot] : 0;
    if (a.part_pcs != nullptr) {
      float* dst = a.part_pcs + 3LL * m * N;
      const float* src = a.pcs + 3LL * part * N;
      if (kVec4) {
        float4* d4 = reinterpret_cast<float4*>(dst);
        const float4* s4 = reinterpret_cast<const float4*>(src);
        const int n4 = 3 * N / 4;
        if (live)
          for (int i = t; i < n4; i += kThreads) d4[i] = s4[i];
        else
          for (int i = t; i < n4; i += kThreads) d4[i] = float4{0.f, 0.f, 0.f, 0.f};
      } else {
        const int n1 = 3 * N;
        if (live)
          for (int i = t; i < n1; i += kThreads) dst[i] = src[i];
        else
          for (int i = t; i < n1; i += kThreads) dst[i] = 0.f;
      }
    }
    if (t < 7) {
      const float v = live && a.poses != nullptr ? a.poses[7 * part + t] : 0.f;
      if (t < 3) {
        if (a.part_trans != nullptr) a.part_trans[3 * m + t] = v;
      } else if (a.part_quat != nullptr) {
        a.part_quat[4 * m + (t - 3)] = v;
      }
    } else if (t >= 8 && t < 11 && a.sym_out != nullptr) {
      a.sym_out[3 * m + (t - 8)] = live ? a.sym[3 * part + (t - 8)] : 0.f;
    }
    return;
  }

  // ---- block (b, P): the labels of sample b ----
  const long long row = (long long)b * P;
  if (t < P) {
    const bool live = t < p;
    if (a.part_valids != nullptr) a.part_valids[row + t] = live ? 1.f : 0.f;
    if (a.part_ids != nullptr) a.part_ids[row + t] = live ? (float)s_geo[t] : 0.f;
    if (a.match_ids != nullptr) a.match_ids[row + t] = (float)s_match[t];
    if (a.order_out != nullptr) a.order_out[row + t] = s_order[t];
  }
  if (t == 0 && a.shape_id != nullptr) a.shape_id[b] = s_shape >= 0 ? a.shape_ids[s_shape] : -1;
  const int PP = P * P;
  if (a.instance_label != nullptr || a.valid_matrix != nullptr) {
    for (int e = t; e < PP; e += kThreads) {
      const int i = e / P, j = e % P;
      if (a.instance_label != nullptr) a.instance_label[row * P + e] = s_rank[i] == j ? 1.f : 0.f;  // rank -1: padded
      if (a.valid_matrix != nullptr) a.valid_matrix[row * P + e] = (i < p && j < p) ? 1.f : 0.f;
    }
  }
  if (a.part_label != nullptr && C > 0) {
    const int PC = P * C;
    for (int e = t; e < PC; e += kThreads) {
      const int i = e / C, c = e % C;
      a.part_label[row * C + e] = (i < p && s_sem[i] - 1 == c) ? 1.f : 0.f;
    }
  }
  if (a.contact_points != nullptr) {  // the stored p x p x 4 block in STORED part order, zero-padded to P x P x 4
    const float* src = s_shape >= 0 ? a.contacts + 4 * a.contact_off[s_shape] : nullptr;
    float* dst = a.contact_points + row * P * 4;
    for (int e = t; e < 4 * PP; e += kThreads) {
      const int i = e / (4 * P), j = (e / 4) % P, c = e & 3;
      dst[e] = (i < p && j < p) ? src[4 * (i * p + j) + c] : 0.f;
    }
  }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace

extern "C" int mpa_partnet_gather_batch(
    const float* pcs, const float* poses, const float* sym, const int32_t* geo_ids, const int32_t* sem_ids,
    const int64_t* shape_part_off, const int64_t* shape_ids, const float* contacts, const int64_t* contact_off, int64_t S,
    const int64_t* shape_index, int64_t B, int64_t P, int64_t N, int64_t C, const int32_t* perm, int32_t random_order,
    uint64_t seed, uint64_t counter, const uint64_t* counter_dev, float* part_pcs, float* part_trans, float* part_quat,
    float* part_valids, float* part_ids, float* instance_label, float* match_ids, float* part_label,
    float* contact_points, float* sym_out, float* valid_matrix, int64_t* shape_id, int32_t* order_out, int32_t* status,
    void* stream) {
  MPA_REQUIRE(P >= 1 && P <= kMaxParts, "partnet_gather_batch: P=%lld outside [1, %d] (one lane per part)", (long long)P,
              kMaxParts);
  MPA_REQUIRE(B >= 0 && S >= 0 && C >= 0 && N >= 0, "partnet_gather_batch: negative size (B=%lld S=%lld N=%lld C=%lld)",
              (long long)B, (long long)S, (long long)N, (long long)C);
  MPA_REQUIRE(B <= (1LL << 24) && N <= (1LL << 28) && C <= (1LL << 20),
              "partnet_gather_batch: oversized B / N / C (B <= 2^24, N <= 2^28, C <= 2^20)");
  MPA_REQUIRE(!(perm != nullptr && random_order), "partnet_gather_batch: a replayed part order (perm) and the "
              "device-random order exclude each other");
  MPA_REQUIRE(!(contact_points != nullptr && (contacts == nullptr || contact_off == nullptr)),
              "partnet_gather_batch: contact_points requested from a store without contacts");
  if (B == 0) return MPA_OK;
  MPA_REQUIRE(shape_part_off && shape_index && status,
              "partnet_gather_batch: null pointer (shape_part_off, shape_index and status are always needed)");
  MPA_REQUIRE(!(part_pcs != nullptr && pcs == nullptr) && !((part_trans != nullptr || part_quat != nullptr) && poses == nullptr)
              && !(sym_out != nullptr && sym == nullptr)
              && !((part_ids != nullptr || instance_label != nullptr || match_ids != nullptr) && geo_ids == nullptr)
              && !(part_label != nullptr && C > 0 && sem_ids == nullptr) && !(shape_id != nullptr && shape_ids == nullptr),
              "partnet_gather_batch: null pointer (a requested output needs the store array it is read from)");
  GatherArgs a;
  a.pcs = pcs, a.poses = poses, a.sym = sym, a.geo_ids = geo_ids, a.sem_ids = sem_ids;
  a.shape_part_off = shape_part_off, a.shape_ids = shape_ids, a.contacts = contacts, a.contact_off = contact_off;
  a.S = S, a.shape_index = shape_index, a.P = (int)P, a.N = (int)N, a.C = (int)C;
  a.perm = perm, a.random_order = random_order ? 1 : 0;
  a.k0 = (uint32_t)seed, a.k1 = (uint32_t)(seed >> 32), a.counter = counter, a.counter_dev = counter_dev;
  a.part_pcs = part_pcs, a.part_trans = part_trans, a.part_quat = part_quat, a.part_valids = part_valids;
  a.part_ids = part_ids, a.instance_label = instance_label, a.match_ids = match_ids, a.part_label = part_label;
  a.contact_points = contact_points, a.sym_out = sym_out, a.valid_matrix = valid_matrix, a.shape_id = shape_id;
  a.order_out = order_out, a.status = status;
  const dim3 grid((unsigned)(B * (P + 1)));
  if (N % 4 == 0 && aligned16(pcs) && aligned16(part_pcs))
    hipLaunchKernelGGL(partnet_gather_kernel<true>, grid, dim3(kThreads), 0, mpa::as_stream(stream), a);
  else
    hipLaunchKernelGGL(partnet_gather_kernel<false>, grid, dim3(kThreads), 0, mpa::as_stream(stream), a);
  return mpa::check_launch("partnet_gather_batch");
}
