// Device-side draws of the B-LSTM seq2seq module (cfg.model.lstm_draws = "device").
//
// The reference draws, on the host and in every forward, the decoder's noise (`np.random.normal`, then a copy from
// pageable memory), the teacher-forcing coin (`random.random() < ratio`) and, in training mode, the LockedDropout mask of
// the decoder's inputs (multi_part_assembly/models/b_lstm/seq2seq.py:165-220,226-241).  Here one launch writes all three
// from Philox4x32-10 blocks (the layout is fixed in include/mpa_hip.h; multi_part_assembly_amd/seq2seq_draw_ref.py
// restates it in numpy): nothing crosses the bus, and the step counter can come from a device word, so that a captured
// step draws afresh on every replay.  One thread per Philox block: block 0 is the coin, the next 4 B blocks are the
// B x 16 normals (Box-Muller, two pairs per block), the rest are the T x B x 128 mask elements, four per block.
#include <math.h>

#include "common.h"
#include "philox.h"

namespace {

constexpr int kNoise = 16;                  // noise channels of the decoder's initial state
constexpr int kDC = 128;                    // decoder input width: the mask's channels (csrc/seq2seq.hip)
constexpr uint32_t kTag = 0x73320000u;      // counter word 1 = kTag | kind: no other user of the generator produces it
constexpr int kThreads = 256;

__device__ __forceinline__ float unit24(uint32_t w) { return (float)(w >> 8) * 5.9604644775390625e-08f; }  // [0, 1)

// two normals from two words: u1 in (0, 1) exactly, never 0; the accurate logf / sincosf
__device__ __forceinline__ void box_muller(uint32_t wa, uint32_t wb, float* out) {
  const float u1 = ((float)(wa >> 9) + 0.5f) * 1.1920928955078125e-07f;
  const float u2 = unit24(wb);
  const float r = sqrtf(-2.0f * logf(u1));
  float s, c;
  sincosf(6.283185307179586f * u2, &s, &c);
  out[0] = r * c;
  out[1] = r * s;
}

__global__ __launch_bounds__(kThreads) void seq2seq_draw_kernel(long long noise_blocks, long long mask_blocks, float p,
                                                                float keep, float ratio, uint32_t k0, uint32_t k1,
                                                                uint64_t counter,
                                                                const uint64_t* __restrict__ counter_dev, uint64_t salt,
                                                                float* __restrict__ noise, int* __restrict__ teacher,
                                                                float* __restrict__ mask) {
  const long long g = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (g >= 1 + noise_blocks + mask_blocks) return;
  const uint64_t c = (counter_dev != nullptr ? *counter_dev : counter) + salt;
  const uint32_t c2 = (uint32_t)c, c3 = (uint32_t)(c >> 32);
  if (g == 0) {
    const mpa::U4 r = mpa::philox4x32_10(mpa::U4{0u, kTag | 0u, c2, c3}, k0, k1);
    teacher[0] = unit24(r.x) < ratio ? 1 : 0;
  } else if (g <= noise_blocks) {
    const long long i = g - 1;
    const mpa::U4 r = mpa::philox4x32_10(mpa::U4{(uint32_t)i, kTag | 1u, c2, c3}, k0, k1);
    float* out = noise + 4 * i;
    box_muller(r.x, r.y, out);
    box_muller(r.z, r.w, out + 2);
  } else {
    const long long i = g - 1 - noise_blocks;
    const mpa::U4 r = mpa::philox4x32_10(mpa::U4{(uint32_t)i, kTag | 2u, c2, c3}, k0, k1);
    float* out = mask + 4 * i;
    out[0] = unit24(r.x) >= p ? keep : 0.0f;
    out[1] = unit24(r.y) >= p ? keep : 0.0f;
    out[2] = unit24(r.z) >= p ? keep : 0.0f;
    out[3] = unit24(r.w) >= p ? keep : 0.0f;
  }
}

}  // namespace

extern "C" int mpa_seq2seq_draw(int64_t B, int64_t T, float p, float ratio, uint64_t seed, uint64_t counter,
                                const uint64_t* counter_dev, uint64_t salt, float* noise, int32_t* teacher, float* mask,
                                void* stream) {
  MPA_REQUIRE(B >= 1 && B <= 64, "seq2seq_draw: B=%lld outside [1, 64]", (long long)B);
  MPA_REQUIRE(T >= 1 && T <= 4096, "seq2seq_draw: T=%lld outside [1, 4096]", (long long)T);
  MPA_REQUIRE(p >= 0.0f && p < 1.0f, "seq2seq_draw: p=%g outside [0, 1)", (double)p);
  MPA_REQUIRE(noise != nullptr && teacher != nullptr, "seq2seq_draw: null pointer");
  const long long noise_blocks = B * kNoise / 4, mask_blocks = mask == nullptr ? 0 : T * B * kDC / 4;
  const long long threads = 1 + noise_blocks + mask_blocks;  // <= 1 + 256 + 2^23
  const float keep = 1.0f / (1.0f - p);                       // rounded once, on the host: the mask's only nonzero value
  hipLaunchKernelGGL(seq2seq_draw_kernel, dim3((unsigned)((threads + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                     mpa::as_stream(stream), noise_blocks, mask_blocks, p, keep, ratio, (uint32_t)seed,
                     (uint32_t)(seed >> 32), counter, counter_dev, salt, noise, (int*)teacher, mask);
  return mpa::check_launch("seq2seq_draw");
}
