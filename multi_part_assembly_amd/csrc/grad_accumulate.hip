// Gradient accumulation: one optimiser step over several micro-batches (Lightning's accumulate_grad_batches).
//
// Every gradient of the model lives in one flat fp32 buffer (optim.FlatBuffers), and under the GradSink the HIP backward
// kernels OVERWRITE their slices of it, so a second backward without zero_grad leaves a mixture of last and summed
// gradients.  The sum of a window of micro-batches is therefore kept in a second flat buffer, the accumulator, by ONE
// streaming launch behind every micro-batch's backward:
//   mode 0 FIRST  acc  <- grad          (8 B per parameter; the accumulator's old content is never read)
//   mode 1 ADD    acc  <- acc + grad    (12 B)
//   mode 2 LAST   grad <- acc + grad    (12 B; the sum lands in the flat GRADIENT, where the all-reduce, the guard, the
//                                        clipping, the Adam kernels, the commit and the average already look)
// A window of k >= 2 micro-batches is FIRST, ADD x (k - 2), LAST, so the flat gradient ends as ((g0 + g1) + g2) + ...;
// a window of one issues no launch.  The mode travels by value or in one device word (read by every lane: uniform), so
// a captured launch follows the word the host wrote in front of the replay; a word outside 0..2 writes nothing.  Every
// addition is one rounded fp32 operation; denormals are kept.  Restated in numpy by multi_part_assembly_amd/accum_ref.py.
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kAccBlocks = 2048;  // (mpa_adam_step_dev's and mpa_ema_update's grid: 8 blocks per CU)

__device__ __forceinline__ float4 add4(float4 a, float4 g) {
  a.x = __fadd_rn(a.x, g.x);
  a.y = __fadd_rn(a.y, g.y);
  a.z = __fadd_rn(a.z, g.z);
  a.w = __fadd_rn(a.w, g.w);
  return a;
}

// The mode word is a plain load of the same word in every lane (as ema_update_kernel reads the guard verdict), the branch
// on it uniform across the grid and outside the loops.  Grid-stride, a float4 per lane; i < n4 bounds every access.
__global__ __launch_bounds__(kThreads) void grad_accumulate_kernel(float4* __restrict__ grad, float4* __restrict__ acc,
                                                                   long long n4, int mode, const int* __restrict__ mode_dev) {
  if (mode_dev != nullptr) mode = mode_dev[0];
  const long long stride = (long long)gridDim.x * kThreads;
  const long long first = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (mode == 0) {
    for (long long i = first; i < n4; i += stride) acc[i] = grad[i];
  } else if (mode == 1) {
    for (long long i = first; i < n4; i += stride) acc[i] = add4(acc[i], grad[i]);
  } else if (mode == 2) {
    for (long long i = first; i < n4; i += stride) grad[i] = add4(acc[i], grad[i]);
  }
}

bool disjoint(const void* p, const void* q, int64_t bytes) {
  const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
  return a + (uintptr_t)bytes <= b || b + (uintptr_t)bytes <= a;
}

}  // namespace

extern "C" int mpa_grad_accumulate(float* grad, float* acc, int64_t numel, int mode, const int32_t* mode_dev,
                                   void* stream) {
  MPA_REQUIRE(numel >= 0 && numel % 4 == 0, "grad_accumulate: numel must be a non-negative multiple of 4");
  MPA_REQUIRE((uintptr_t)mode_dev % 4 == 0, "grad_accumulate: misaligned mode word");
  MPA_REQUIRE(mode_dev != nullptr || (mode >= 0 && mode <= 2),
              "grad_accumulate: mode must be 0 (first), 1 (add) or 2 (last), got %d", mode);
  if (numel > 0) {
    MPA_REQUIRE(grad && acc, "grad_accumulate: null pointer");
    MPA_REQUIRE(((uintptr_t)grad | (uintptr_t)acc) % 16 == 0, "grad_accumulate: buffers must be 16-byte aligned");
    MPA_REQUIRE(disjoint(grad, acc, numel * 4), "grad_accumulate: the gradient and the accumulator overlap");
  }
  if (numel == 0) return MPA_OK;  // nothing to add
  long long blocks = (numel / 4 + kThreads - 1) / kThreads;
  if (blocks > kAccBlocks) blocks = kAccBlocks;
  hipLaunchKernelGGL(grad_accumulate_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, mpa::as_stream(stream),
                     reinterpret_cast<float4*>(grad), reinterpret_cast<float4*>(acc), (long long)(numel / 4), mode,
                     (const int*)mode_dev);
  return mpa::check_launch("grad_accumulate");
}
