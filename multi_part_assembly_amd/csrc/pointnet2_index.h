// The per-cloud inverted index behind the PointNet++ backward sums (csrc/pointnet2_ops.hip: grouping; csrc/pointnet2_interp.hip:
// three-point interpolation): for every source point the ascending list of the flat positions that name it.  One kernel, one
// carve; both files include this header and get their own copy (internal linkage).
#pragma once
#include "common.h"

namespace {

constexpr int kGrpThreads = 256;

int round64(int64_t v) { return (int)((v + 63) / 64 * 64); }

struct GroupWorkspace {
  int *start, *cursor, *list;
};
GroupWorkspace carve_group(mpa::Arena& a, int64_t M, int64_t N, int64_t SK) {
  GroupWorkspace w;
  w.start = a.take<int>(M * round64(N + 1), 256);
  w.cursor = a.take<int>(M * round64(N + 1), 256);
  w.list = a.take<int>(M * round64(SK), 256);
  return w;
}

// The inverted index of one cloud, by one block: start [N + 1] (exclusive prefix sums of the counts), list [SK] (for every
// point k the positions p with idx[p] == k at list[start[k] .. start[k + 1]), ascending).  `cursor` [N] is scratch.  The
// per-cloud strides are multiples of 64 words and the base is 256-byte aligned: no two blocks share a cache line.
__global__ __launch_bounds__(kGrpThreads) void group_index_kernel(const int32_t* __restrict__ idx, int N, int SK, int Ns,
                                                                 int SKs, int* start, int* cursor, int* list) {
  __shared__ int part[kGrpThreads];
  __shared__ int tile[kGrpThreads];
  const int t = threadIdx.x;
  idx += (int64_t)blockIdx.x * SK;
  start += (int64_t)blockIdx.x * Ns;
  cursor += (int64_t)blockIdx.x * Ns;
  list += (int64_t)blockIdx.x * SKs;
  for (int k = t; k < N; k += kGrpThreads) cursor[k] = 0;
  __syncthreads();
  for (int p = t; p < SK; p += kGrpThreads) {
    const int i = idx[p];
    if ((unsigned)i < (unsigned)N) atomicAdd(&cursor[i], 1);
  }
  __syncthreads();
  const int per = (N + kGrpThreads - 1) / kGrpThreads;
  const int k0 = t * per < N ? t * per : N, k1 = k0 + per < N ? k0 + per : N;
  int sum = 0;
  for (int k = k0; k < k1; ++k) sum += __hip_atomic_load(&cursor[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  part[t] = sum;
  __syncthreads();
  if (t == 0) {
    int run = 0;
    for (int u = 0; u < kGrpThreads; ++u) {
      const int v = part[u];
      part[u] = run;
      run += v;
    }
    start[N] = run;
  }
  __syncthreads();
  int run = part[t];
  for (int k = k0; k < k1; ++k) {
    const int c = __hip_atomic_load(&cursor[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    start[k] = run;
    cursor[k] = run;
    run += c;
  }
  __syncthreads();
  // stable placement, 256 positions at a time: a position's rank among the equal keys before it in the tile, on top of
  // the key's cursor; the last of a key in the tile moves the cursor on
  for (int base = 0; base < SK; base += kGrpThreads) {
    const int p = base + t;
    int key = p < SK ? idx[p] : -1;
    if ((unsigned)key >= (unsigned)N) key = -1;
    tile[t] = key;
    __syncthreads();
    int rank = 0;
    bool last = true;
    if (key >= 0) {
      for (int u = 0; u < kGrpThreads; ++u) {
        const bool same = tile[u] == key;
        rank += (same && u < t) ? 1 : 0;
        last = last && !(same && u > t);
      }
      list[cursor[key] + rank] = p;
    }
    __syncthreads();  // every cursor of this tile has been read
    if (key >= 0 && last) cursor[key] += rank + 1;
    __syncthreads();
  }
}

}  // namespace
