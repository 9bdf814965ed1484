// The inter-block exchange of the recurrent kernels (gru.hip: the (bi)directional GRU of RGL-NET and of the B-LSTM
// encoder; seq2seq.hip: the B-LSTM decoder): tagged 8-byte words instead of a grid barrier, the poll budget, the status
// word a launch raises when its blocks are not co-resident, and the co-residency check itself.
#pragma once

#include <stdlib.h>

#include "common.h"

namespace {

// Exchange between the blocks of a direction, once per step, WITHOUT a grid barrier: every value travels as one
// naturally aligned 8-byte {value, tag} word written by a single device-scope store (tag = the step's number), and a
// consumer polls the word itself until the tag is the one it waits for — data and "ready" arrive in the same store, so
// no fence, no counter and no arrival skew sit between a producer and its consumers (a counter barrier with its release /
// acquire fences measured ~7 us per step, most of a step's time).  The exchange buffers are zeroed before the launch
// (tags start at 1); two buffers by step parity suffice: a block can only be one step ahead of the slowest reader of
// its previous values.  All blocks of the grid must be co-resident (checked by gru_resident).
typedef unsigned long long tagged_t;
constexpr int kPollBudget = 1 << 22;
__device__ __forceinline__ void tagged_store(tagged_t* p, float v, unsigned tag) {
  __hip_atomic_store(p, ((tagged_t)tag << 32) | (tagged_t)__float_as_uint(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ tagged_t tagged_peek(const tagged_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// the value of *p once it carries `tag` (first poll result given).  A producer that never shows up (a grid that is not
// co-resident after all — e.g. another stream's kernels hold the CUs the missing blocks need) exhausts the wait's poll
// budget after a few seconds.  Then the launch gives up CLEANLY: the waiting thread raises the launch's status word (device
// memory of the caller), every other wait of every block sees it within 1024 polls and stops too, the kernel runs to its
// end on whatever values it has, and the host side turns the status word into an error (gru.py) — no trap (which
// takes the process's HIP context with it), no hang.  Without a status word (NULL) the kernel traps as before.
struct Poll {
  int budget, limit;
  int* status;
  bool dead;
};
__device__ __forceinline__ float tagged_wait(const tagged_t* p, tagged_t first, unsigned tag, Poll& pl) {
  tagged_t v = first;
  while ((unsigned)(v >> 32) != tag && !pl.dead) {
    --pl.budget;
    if (pl.budget < 0 || ((pl.budget & 1023) == 0 && pl.status != nullptr &&
                          __hip_atomic_load(pl.status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0)) {
      if (pl.status == nullptr) __builtin_trap();
      __hip_atomic_store(pl.status, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      pl.dead = true;
      break;
    }
    __builtin_amdgcn_s_sleep(2);
    v = tagged_peek(p);
  }
  pl.budget = pl.limit;  // the budget bounds ONE wait (a few seconds), not the launch's total polling
  return __uint_as_float((unsigned)v);
}
// PF words p[q * stride] (q < n valid): wait for the first one alone (ONE polled word per thread while the producers
// are still busy: the pollers' traffic delays the very stores they wait for — re-loading whole batches until every tag
// had arrived was 4x slower), then load the others together, and wait singly for a straggler.
template <int PF>
__device__ __forceinline__ void tagged_wait_all(const tagged_t* p, long long stride, int n, unsigned tag, Poll& budget,
                                                float (&out)[PF]) {
  out[0] = tagged_wait(p, tagged_peek(p), tag, budget);
  tagged_t v[PF];
#pragma unroll
  for (int q = 1; q < PF; ++q) v[q] = tagged_peek(p + (q < n ? q : 0) * stride);
#pragma unroll
  for (int q = 1; q < PF; ++q) out[q] = q < n ? tagged_wait(p + q * stride, v[q], tag, budget) : 0.0f;
}

// Every block polls for the words the other blocks of its direction publish in the same step: all blocks of a launch must be
// RESIDENT at once (a block that was never dispatched — e.g. on a partitioned device with fewer CUs, or with an LDS
// footprint that leaves one block per CU — would stall the others until their poll budget runs out).  Checked against the
// occupancy the runtime reports.
template <typename Kern>
int gru_resident(Kern kern, size_t smem, int blocks, const char* who, int threads = 256) {
  if (smem > 64 * 1024 &&
      hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem) !=
          hipSuccess)
    return mpa::fail(MPA_EINVAL, "%s: cannot reserve %zu bytes of LDS", who, smem);
  int dev = 0, cus = 0, per_cu = 0;
  if (hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
      hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void*>(kern), threads, smem) != hipSuccess)
    return mpa::fail(MPA_EINVAL, "%s: cannot query the device's occupancy", who);
  if ((long long)per_cu * cus < blocks)
    return mpa::fail(MPA_EINVAL, "%s: the per-step exchange needs all %d blocks resident, this device holds %d x %d", who, blocks,
                     per_cu, cus);
  return MPA_OK;
}
// polls one wait may spend (~1 us each) before the launch gives up; MPA_GRU_POLL_BUDGET overrides (tests shorten it)
int poll_limit() {
  if (const char* e = getenv("MPA_GRU_POLL_BUDGET")) {
    const long v = strtol(e, nullptr, 10);
    if (v >= 1024 && v <= (1L << 30)) return (int)v;
  }
  return kPollBudget;
}

}  // namespace
