// Exponential moving average (EMA) of the model's weights, kept on the device beside the live ones.
//
// The reference trains through Lightning and keeps one copy of the weights; an averaged copy is what timm's ModelEmaV2
// and torch.optim.swa_utils.AveragedModel add: e <- e + (1 - d) (p - e) after every optimiser step.  Parameters live in
// one flat fp32 buffer here (optim.FlatBuffers) and every module buffer in one byte slab (optim.BufferSlab), so the
// average of a whole model is ONE streaming launch behind the Adam update (mpa_ema_update: 8 B read + 4 B written per
// parameter) and putting it in front of the model is ONE bitwise exchange (mpa_ema_swap): parameters and buffers stay
// views of the same memory, so kernels, the gradient sink and captured graphs see the averaged values with no re-homing.
//
// The coefficient is computed on the device from the optimiser's applied-step count (hyper[4], read behind this step's
// advance), and the launch returns before its first store behind a non-zero guard verdict: the average of a skipped step
// keeps its bits, and a captured launch stays valid across replays.  Every operation is one rounded fp32 operation
//   a = (float)t;  q = (1 + a) / (10 + a);  d = warmup ? fminf(decay, q) : decay;  c = 1 - d
//   e = e + c * (p - e)
// restated in numpy by multi_part_assembly_amd/ema_ref.py.
#include <math.h>

#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kEmaBlocks = 2048;  // (mpa_adam_step_dev's grid: 8 blocks per CU)
constexpr int kSegmentWords = 3;  // {byte offset, byte size, kind} as int64

__device__ __forceinline__ float ema_coefficient(const float* __restrict__ hyper, float decay, int warmup) {
  const float a = (float)__float_as_int(hyper[4]);
  const float q = __fdiv_rn(__fadd_rn(1.0f, a), __fadd_rn(10.0f, a));
  const float d = warmup ? fminf(decay, q) : decay;
  return __fsub_rn(1.0f, d);
}

__device__ __forceinline__ float ema_one(float p, float e, float c) {
  return __fadd_rn(e, __fmul_rn(c, __fsub_rn(p, e)));
}

__device__ __forceinline__ unsigned ema_word(unsigned p, unsigned e, float c) {
  return __float_as_uint(ema_one(__uint_as_float(p), __uint_as_float(e), c));
}

// The verdict and the step count are plain loads of the same words in every lane (uniform across the grid, as in
// adam_guarded_kernel); the coefficient is loop-invariant, so a wave computes it once.  Flat range: grid-stride, a float4
// per lane.  Slab: block b walks segments b, b + gridDim.x, ... (the grid has a block per segment unless there are more
// than kEmaBlocks), 16 bytes per lane; the slot's bytes behind `size` (BufferSlab's zero padding) are copied like kind 0.
__global__ __launch_bounds__(kThreads) void ema_update_kernel(const float4* __restrict__ param, float4* __restrict__ ema,
                                                              long long n4, const uint4* __restrict__ live,
                                                              uint4* __restrict__ ema_state,
                                                              const long long* __restrict__ segments, int num_segments,
                                                              const float* __restrict__ hyper, float decay, int warmup,
                                                              const int* __restrict__ guard) {
  if (guard != nullptr && guard[0] != 0) return;
  const float c = ema_coefficient(hyper, decay, warmup);
  const long long stride = (long long)gridDim.x * kThreads;
  for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n4; i += stride) {
    const float4 p = param[i];
    float4 e = ema[i];
    e.x = ema_one(p.x, e.x, c);
    e.y = ema_one(p.y, e.y, c);
    e.z = ema_one(p.z, e.z, c);
    e.w = ema_one(p.w, e.w, c);
    ema[i] = e;
  }
  for (int s = blockIdx.x; s < num_segments; s += gridDim.x) {
    const long long first = segments[kSegmentWords * s] / 16, size = segments[kSegmentWords * s + 1];
    const bool averaged = segments[kSegmentWords * s + 2] == 1;
    const long long units = (size + 15) / 16, words = size / 4;
    for (long long u = threadIdx.x; u < units; u += kThreads) {
      uint4 l = live[first + u];
      if (averaged) {
        const uint4 e = ema_state[first + u];
        const long long w = 4 * u;
        if (w + 0 < words) l.x = ema_word(l.x, e.x, c);
        if (w + 1 < words) l.y = ema_word(l.y, e.y, c);
        if (w + 2 < words) l.z = ema_word(l.z, e.z, c);
        if (w + 3 < words) l.w = ema_word(l.w, e.w, c);
      }
      ema_state[first + u] = l;
    }
  }
}

// bitwise exchange of two pairs of ranges in 16-byte units: one grid-stride walk over the units of both pairs
__global__ __launch_bounds__(kThreads) void ema_swap_kernel(uint4* __restrict__ a, uint4* __restrict__ b, long long units_ab,
                                                            uint4* __restrict__ c, uint4* __restrict__ d,
                                                            long long units_cd) {
  const long long stride = (long long)gridDim.x * kThreads;
  for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < units_ab + units_cd; i += stride) {
    uint4* __restrict__ x = i < units_ab ? a + i : c + (i - units_ab);
    uint4* __restrict__ y = i < units_ab ? b + i : d + (i - units_ab);
    const uint4 vx = *x, vy = *y;
    *x = vy;
    *y = vx;
  }
}

bool disjoint(const void* p, int64_t p_bytes, const void* q, int64_t q_bytes) {
  const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
  return a + (uintptr_t)p_bytes <= b || b + (uintptr_t)q_bytes <= a;
}
bool disjoint(const void* p, const void* q, int64_t bytes) { return disjoint(p, bytes, q, bytes); }

}  // namespace

extern "C" int mpa_ema_update(const float* param, float* ema, int64_t numel, const void* live, void* ema_state,
                              int64_t state_bytes, const int64_t* segments_host, const int64_t* segments,
                              int64_t num_segments, const float* hyper, float decay, int warmup, const int32_t* guard,
                              void* stream) {
  MPA_REQUIRE(numel >= 0 && numel % 4 == 0, "ema_update: numel must be a non-negative multiple of 4");
  MPA_REQUIRE(state_bytes >= 0 && state_bytes % 16 == 0, "ema_update: state_bytes must be a non-negative multiple of 16");
  MPA_REQUIRE(decay >= 0.0f && decay < 1.0f, "ema_update: decay must lie in [0, 1)");  // (false for a NaN)
  MPA_REQUIRE(num_segments >= 0 && num_segments < ((int64_t)1 << 31), "ema_update: bad segment count");
  MPA_REQUIRE(hyper != nullptr, "ema_update: null pointer (the optimiser's device words)");
  MPA_REQUIRE(((uintptr_t)hyper | (uintptr_t)guard) % 4 == 0, "ema_update: misaligned word");
  if (numel > 0) {
    MPA_REQUIRE(param && ema, "ema_update: null pointer");
    MPA_REQUIRE(((uintptr_t)param | (uintptr_t)ema) % 16 == 0, "ema_update: buffers must be 16-byte aligned");
    MPA_REQUIRE(disjoint(param, ema, numel * 4), "ema_update: the parameters and their average overlap");
  }
  if (state_bytes > 0) {
    MPA_REQUIRE(live && ema_state, "ema_update: null pointer");
    MPA_REQUIRE(((uintptr_t)live | (uintptr_t)ema_state) % 16 == 0, "ema_update: buffers must be 16-byte aligned");
    MPA_REQUIRE(disjoint(live, ema_state, state_bytes), "ema_update: the slab and its average overlap");
  }
  if (num_segments > 0) {
    MPA_REQUIRE(segments_host && segments, "ema_update: null pointer (the segment table and its device copy)");
    MPA_REQUIRE(((uintptr_t)segments_host | (uintptr_t)segments) % 8 == 0, "ema_update: misaligned segment table");
  }
  int64_t end = 0, slot_bytes = 0;  // slots ascend and do not overlap: no byte of the average is written twice
  for (int64_t s = 0; s < num_segments; ++s) {
    const int64_t off = segments_host[kSegmentWords * s], size = segments_host[kSegmentWords * s + 1];
    const int64_t kind = segments_host[kSegmentWords * s + 2];
    MPA_REQUIRE(off >= 0 && off % 16 == 0, "ema_update: segment %lld does not start on a 16-byte boundary (offset %lld)",
                (long long)s, (long long)off);
    MPA_REQUIRE(size >= 0 && size <= state_bytes && off <= state_bytes - (size + 15) / 16 * 16,
                "ema_update: segment %lld (offset %lld, %lld bytes) leaves the slab of %lld bytes", (long long)s,
                (long long)off, (long long)size, (long long)state_bytes);
    MPA_REQUIRE(off >= end, "ema_update: segment %lld overlaps the one before it", (long long)s);
    MPA_REQUIRE(kind == 0 || (kind == 1 && size % 4 == 0), "ema_update: segment %lld: kind must be 0 (copied) or 1 "
                "(float32, a multiple of 4 bytes)", (long long)s);
    end = off + (size + 15) / 16 * 16;
    slot_bytes += end - off;
  }
  if (numel == 0 && slot_bytes == 0) return MPA_OK;  // nothing to average
  long long blocks = (numel / 4 + kThreads - 1) / kThreads;
  if (blocks < num_segments) blocks = num_segments;
  if (blocks < 1) blocks = 1;
  if (blocks > kEmaBlocks) blocks = kEmaBlocks;
  hipLaunchKernelGGL(ema_update_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, mpa::as_stream(stream),
                     reinterpret_cast<const float4*>(param), reinterpret_cast<float4*>(ema), (long long)(numel / 4),
                     static_cast<const uint4*>(live), static_cast<uint4*>(ema_state),
                     reinterpret_cast<const long long*>(segments), (int)num_segments, hyper, decay, warmup,
                     (const int*)guard);
  return mpa::check_launch("ema_update");
}

extern "C" int mpa_ema_swap(void* param, void* ema, int64_t param_bytes, void* live, void* ema_state, int64_t state_bytes,
                            void* stream) {
  MPA_REQUIRE(param_bytes >= 0 && param_bytes % 16 == 0 && state_bytes >= 0 && state_bytes % 16 == 0,
              "ema_swap: sizes must be non-negative multiples of 16");
  if (param_bytes > 0) {
    MPA_REQUIRE(param && ema, "ema_swap: null pointer");
    MPA_REQUIRE(((uintptr_t)param | (uintptr_t)ema) % 16 == 0, "ema_swap: buffers must be 16-byte aligned");
    MPA_REQUIRE(disjoint(param, ema, param_bytes), "ema_swap: the two parameter ranges overlap");
  }
  if (state_bytes > 0) {
    MPA_REQUIRE(live && ema_state, "ema_swap: null pointer");
    MPA_REQUIRE(((uintptr_t)live | (uintptr_t)ema_state) % 16 == 0, "ema_swap: buffers must be 16-byte aligned");
    MPA_REQUIRE(disjoint(live, ema_state, state_bytes), "ema_swap: the two slab ranges overlap");
  }
  if (param_bytes > 0 && state_bytes > 0) {  // a unit exchanged twice in one launch would race
    MPA_REQUIRE(disjoint(param, param_bytes, live, state_bytes) && disjoint(param, param_bytes, ema_state, state_bytes) &&
                    disjoint(ema, param_bytes, live, state_bytes) && disjoint(ema, param_bytes, ema_state, state_bytes),
                "ema_swap: the parameter pair and the slab pair overlap");
  }
  const long long units = (param_bytes + state_bytes) / 16;
  if (units == 0) return MPA_OK;
  long long blocks = (units + kThreads - 1) / kThreads;
  if (blocks > kEmaBlocks) blocks = kEmaBlocks;
  hipLaunchKernelGGL(ema_swap_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, mpa::as_stream(stream),
                     static_cast<uint4*>(param), static_cast<uint4*>(ema), (long long)(param_bytes / 16),
                     static_cast<uint4*>(live), static_cast<uint4*>(ema_state), (long long)(state_bytes / 16));
  return mpa::check_launch("ema_swap");
}
