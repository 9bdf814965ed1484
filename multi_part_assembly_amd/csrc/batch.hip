// Batch producer, device side: the per-part transform of GeometryPartDataset.__getitem__
// (multi_part_assembly/datasets/geometry_data.py:74-107,133-146) for a whole batch in one launch.
//
// Per valid part the reference does, in float64 on a CPU worker: centroid = mean of the sampled points, points -=
// centroid, points = (rot_mat @ points^T)^T, points = points[order] (a random permutation), then pads to
// [max_num_part, N, 3] and casts to float32; part_trans = centroid.  Here one block per part slot does the same
// in float64 — fixed-order sums, no FMA (this file is built with -ffp-contract=off) — from the raw sampled
// points, the rotation matrices and the permutations the host drew (same RNG calls as the reference, see
// datasets.py), and writes the float32 batch tensors directly; padded slots are written as zeros.
// HBM-bound: 24 B read + 4 B index + 12 B written per point.
#include "common.h"
#include "part_transform.h"

namespace {

// grid = M part slots, block mpa::kPartThreads.
__global__ __launch_bounds__(mpa::kPartThreads) void part_batch_transform_kernel(
    const double* __restrict__ raw, const double* __restrict__ rot, const int* __restrict__ perm,
    const float* __restrict__ valids, int N, float* __restrict__ part_pcs, float* __restrict__ part_trans) {
  const int m = blockIdx.x;
  float* out = part_pcs + 3LL * m * N;
  if (valids[m] == 0.0f) {
    mpa::part_zero_fill(N, out, part_trans + 3 * m);
    return;
  }
  mpa::part_transform_block<true>(raw + 3LL * m * N, rot + 9LL * m, perm + (long long)m * N, N, out,
                                  part_trans + 3 * m);
}

}  // namespace

extern "C" int mpa_part_batch_transform(const double* raw, const double* rot, const int32_t* perm,
                                        const float* valids, int64_t M, int64_t N, float* part_pcs,
                                        float* part_trans, void* stream) {
  MPA_REQUIRE(M >= 0 && N >= 1 && N <= (1LL << 24), "part_batch_transform: bad sizes");
  if (M == 0) return MPA_OK;
  MPA_REQUIRE(raw && rot && perm && valids && part_pcs && part_trans, "part_batch_transform: null pointer");
  hipLaunchKernelGGL(part_batch_transform_kernel, dim3((unsigned)M), dim3(mpa::kPartThreads), 0, mpa::as_stream(stream), raw,
                     rot, perm, valids, (int)N, part_pcs, part_trans);
  return mpa::check_launch("part_batch_transform");
}
