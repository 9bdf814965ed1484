// Fused Adam / AdamW step over ONE flat fp32 parameter buffer.
//
// The reference optimises with torch.optim.Adam(lr=1e-3, weight_decay=0) — AdamW with parameter
// groups when weight_decay > 0 (multi_part_assembly/models/modules/base_model.py:389-406) — which
// PyTorch runs as several elementwise passes per tensor.  All parameters, gradients and both
// moments of the model live in four flat buffers here (multi_part_assembly_amd/optim.py), so one
// step is ONE streaming kernel: 16 B read + 12 B written per element, float4-vectorised.
// `grad_scale` folds the 1/world_size of the data-parallel gradient mean into the same pass.
// mpa_adam_step_dev is the graph-capturable twin: learning rate, grad_scale, the STEP COUNTER and the bias
// corrections live in an 8-float DEVICE buffer; a one-thread kernel in front of the update advances the counter and
// recomputes the corrections, so a captured launch stays valid across replays and the host never has to upload
// per-step scalars (a re-used pinned staging buffer would be overwritten by a host that runs steps ahead of the GPU).
// `decay_mask` (nullable): 1/0 per element — the reference exempts biases and normalisation weights from weight
// decay (utils/utils.py:90-125 filter_wd_parameters).  mpa_grad_clip_coef: global-norm gradient clipping
// (Lightning's gradient_clip_val, scripts/train.py:90) as a coefficient folded into the same update.
// mpa_step_guard + mpa_adam_step_guarded (opt-in): the guarded step.  One pass over the gradient — the clipping's two-stage
// double sum, which is finite exactly when every element is, plus the smallest index of a non-finite element — and a
// one-wave kernel whose lane 0 writes the coefficient, the verdict (non-finite gradient / raised launch status word) and the
// eight guard words, and advances the step count ONLY for verdict 0; the update then returns before its first store
// behind a non-zero verdict.  A bad step so leaves parameters, moments, step count and bias corrections bit-unchanged
// without the host looking (the reference: Lightning's GradScaler in its --fp16 runs).  mpa_guard_mark turns a raised
// status word into a NaN in grad[0] in front of a data-parallel all-reduce: every rank then reaches the same verdict.
// The unguarded entry points share their device functions with the guarded ones and keep their results bit for bit.
//
// Update rule = torch.optim.Adam's (single-tensor path), term by term:
//   g  = grad*grad_scale (+ wd*p for Adam's L2 form);   p *= 1 - lr*wd  for AdamW's decoupled form
//   m  = m + (g - m)*(1-beta1);   v = v*beta2 + g*g*(1-beta2)
//   p -= (lr/bc1) * m / (sqrt(v)/sqrt(bc2) + eps)
#include "common.h"

namespace {

constexpr int kThreads = 256;

struct AdamArgs {
  float lr, beta1, beta2, eps, weight_decay, bc1, bc2_sqrt, grad_scale;
  int decoupled;
};

__device__ __forceinline__ void adam_one(float& p, float g, float& m, float& v, const AdamArgs a, float wd) {
  g = g * a.grad_scale;
  if (wd != 0.0f) {
    if (a.decoupled) p = p * (1.0f - a.lr * wd);
    else g = g + wd * p;
  }
  m = m + (g - m) * (1.0f - a.beta1);
  v = v * a.beta2 + (g * g) * (1.0f - a.beta2);
  const float denom = __builtin_sqrtf(v) / a.bc2_sqrt + a.eps;
  p = p - (a.lr / a.bc1) * (m / denom);
}

// the update of one launch; shared by adam_kernel and its guarded twin (identical arithmetic on identical operands)
__device__ __forceinline__ void adam_update(float* __restrict__ param, const float* __restrict__ grad,
                                            float* __restrict__ exp_avg, float* __restrict__ exp_avg_sq,
                                            long long n, AdamArgs a, const float* __restrict__ dev_hyper,
                                            const float* __restrict__ decay_mask) {
  if (dev_hyper != nullptr) {  // {lr, bc1, bc2_sqrt, grad_scale, step bits, clip coefficient}
    a.lr = dev_hyper[0];
    a.bc1 = dev_hyper[1];
    a.bc2_sqrt = dev_hyper[2];
    a.grad_scale = dev_hyper[3] * dev_hyper[5];
  }
  const bool masked = decay_mask != nullptr && a.weight_decay != 0.0f;
  const long long n4 = n / 4;
  const long long stride = (long long)gridDim.x * kThreads;
  for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n4; i += stride) {
    float4 p = reinterpret_cast<float4*>(param)[i];
    const float4 g = reinterpret_cast<const float4*>(grad)[i];
    float4 m = reinterpret_cast<float4*>(exp_avg)[i];
    float4 v = reinterpret_cast<float4*>(exp_avg_sq)[i];
    float4 w = make_float4(a.weight_decay, a.weight_decay, a.weight_decay, a.weight_decay);
    if (masked) {
      const float4 k = reinterpret_cast<const float4*>(decay_mask)[i];
      w = make_float4(w.x * k.x, w.y * k.y, w.z * k.z, w.w * k.w);
    }
    adam_one(p.x, g.x, m.x, v.x, a, w.x);
    adam_one(p.y, g.y, m.y, v.y, a, w.y);
    adam_one(p.z, g.z, m.z, v.z, a, w.z);
    adam_one(p.w, g.w, m.w, v.w, a, w.w);
    reinterpret_cast<float4*>(param)[i] = p;
    reinterpret_cast<float4*>(exp_avg)[i] = m;
    reinterpret_cast<float4*>(exp_avg_sq)[i] = v;
  }
  // tail (< 4 elements)
  const long long t = n4 * 4 + (long long)blockIdx.x * kThreads + threadIdx.x;
  if (t < n) adam_one(param[t], grad[t], exp_avg[t], exp_avg_sq[t], a, masked ? a.weight_decay * decay_mask[t] : a.weight_decay);
}

__global__ __launch_bounds__(kThreads) void adam_kernel(float* __restrict__ param,
                                                        const float* __restrict__ grad,
                                                        float* __restrict__ exp_avg,
                                                        float* __restrict__ exp_avg_sq,
                                                        long long n, AdamArgs a,
                                                        const float* __restrict__ dev_hyper,
                                                        const float* __restrict__ decay_mask) {
  adam_update(param, grad, exp_avg, exp_avg_sq, n, a, dev_hyper, decay_mask);
}

// guarded twin: the verdict of mpa_step_guard is one plain load of the same word in every lane (uniform across the
// grid), and a step that was refused returns before its first store
__global__ __launch_bounds__(kThreads) void adam_guarded_kernel(float* __restrict__ param,
                                                                const float* __restrict__ grad,
                                                                float* __restrict__ exp_avg,
                                                                float* __restrict__ exp_avg_sq,
                                                                long long n, AdamArgs a,
                                                                const float* __restrict__ dev_hyper,
                                                                const float* __restrict__ decay_mask,
                                                                const int* __restrict__ guard) {
  if (guard[0] != 0) return;
  adam_update(param, grad, exp_avg, exp_avg_sq, n, a, dev_hyper, decay_mask);
}

// hyper[4] holds the step count (int32 bits): advance it and recompute the bias corrections, in double like the host
__device__ __forceinline__ void adam_advance(float* __restrict__ hyper, float beta1, float beta2) {
  const int step = __float_as_int(hyper[4]) + 1;
  hyper[4] = __int_as_float(step);
  hyper[1] = (float)(1.0 - pow((double)beta1, (double)step));
  hyper[2] = (float)sqrt(1.0 - pow((double)beta2, (double)step));
}

__global__ void adam_advance_kernel(float* __restrict__ hyper, float beta1, float beta2) {
  adam_advance(hyper, beta1, beta2);
}

// sum of squares of the gradient: per-block partials in double, then ONE block adds them in a fixed order
// kFind (mpa_step_guard's pass): besides the sum, the smallest flat index of a NaN / +-inf element per block (kNoBad
// if none).  A float4 whose sum of squares is finite holds finite elements only (the largest float squared is 1.2e77),
// so the per-element look happens only behind a non-finite term; the sums are the same operations in the same order.
constexpr int kNormBlocks = 512;
constexpr int kNoBad = 0x7fffffff;
__device__ __forceinline__ bool finite_f64(double x) {
  return ((unsigned long long)__double_as_longlong(x) & 0x7ff0000000000000ull) != 0x7ff0000000000000ull;
}
__device__ __forceinline__ bool finite_f32(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }

template <bool kFind>
__device__ __forceinline__ void grad_sqnorm(const float* __restrict__ grad, long long n, double* __restrict__ partial,
                                            int* __restrict__ first_bad) {
  __shared__ double red[kThreads];
  __shared__ int bad_red[kFind ? kThreads : 1];
  double acc = 0.0;
  int bad = kNoBad;
  const long long n4 = n / 4, stride = (long long)gridDim.x * kThreads;
  for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n4; i += stride) {
    const float4 g = reinterpret_cast<const float4*>(grad)[i];
    const double q = (double)g.x * g.x + (double)g.y * g.y + (double)g.z * g.z + (double)g.w * g.w;
    acc += q;
    if (kFind && !finite_f64(q) && bad == kNoBad)  // (i grows: the first hit of this thread is its smallest)
      bad = (int)(4 * i) + (!finite_f32(g.x) ? 0 : !finite_f32(g.y) ? 1 : !finite_f32(g.z) ? 2 : 3);
  }
  const long long t = n4 * 4 + (long long)blockIdx.x * kThreads + threadIdx.x;
  if (t < n) {
    acc += (double)grad[t] * grad[t];
    if (kFind && !finite_f32(grad[t]) && (int)t < bad) bad = (int)t;
  }
  red[threadIdx.x] = acc;
  if (kFind) bad_red[threadIdx.x] = bad;
  __syncthreads();
  for (int o = kThreads / 2; o > 0; o >>= 1) {
    if (threadIdx.x < o) {
      red[threadIdx.x] += red[threadIdx.x + o];
      if (kFind) bad_red[threadIdx.x] = min(bad_red[threadIdx.x], bad_red[threadIdx.x + o]);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    partial[blockIdx.x] = red[0];
    if (kFind) first_bad[blockIdx.x] = bad_red[0];
  }
}

__global__ __launch_bounds__(kThreads) void grad_sqnorm_kernel(const float* __restrict__ grad, long long n,
                                                               double* __restrict__ partial) {
  grad_sqnorm<false>(grad, n, partial, nullptr);
}

__global__ __launch_bounds__(kThreads) void grad_sqnorm_find_kernel(const float* __restrict__ grad, long long n,
                                                                    double* __restrict__ partial,
                                                                    int* __restrict__ first_bad) {
  grad_sqnorm<true>(grad, n, partial, first_bad);
}

// the clipping of both step forms: from the gradient's sum of squares, the norm of the (already scaled) mean gradient and
// the quotient that is the coefficient where it lies below 1 (torch.nn.utils.clip_grad_norm_), all in double
__device__ __forceinline__ void clip_coef(double s, const float* __restrict__ scale_dev, float scale, float max_norm,
                                          double& c, double& norm) {
  const double k = scale_dev != nullptr ? (double)scale_dev[0] : (double)scale;
  norm = __builtin_sqrt(s) * k;
  c = (double)max_norm / (norm + 1e-6);
}

__global__ void grad_clip_coef_kernel(const double* __restrict__ partial, int blocks, float max_norm,
                                      const float* __restrict__ scale_dev, float scale, float* __restrict__ coef) {
  double s = 0.0;
  for (int b = 0; b < blocks; ++b) s += partial[b];
  double c, norm;
  clip_coef(s, scale_dev, scale, max_norm, c, norm);
  coef[0] = c < 1.0 ? (float)c : 1.0f;
  coef[1] = (float)norm;
}

// mpa_step_guard's second launch (one wave, lane 0 decides): the coefficient exactly as grad_clip_coef_kernel computes it
// (clip_coef), the verdict, the eight guard words, and — for an accepted step only — adam_advance
constexpr int kVerdictLanes = 64;
__global__ __launch_bounds__(kVerdictLanes) void step_guard_verdict_kernel(const double* __restrict__ partial, const int* __restrict__ first_bad,
                                          int blocks, float max_norm, const float* __restrict__ scale_dev, float scale,
                                          const int* __restrict__ launch_status, float* __restrict__ hyper,
                                          int* __restrict__ guard, float beta1, float beta2) {
  // one wave: the lanes fetch the partials side by side (one round trip instead of a chain of them), lane 0 adds them in
  // grad_clip_coef_kernel's order b = 0, 1, ... and does everything else alone
  __shared__ double sums[kNormBlocks];
  __shared__ int bads[kVerdictLanes];
  int mine = kNoBad;
  for (int b = threadIdx.x; b < blocks; b += kVerdictLanes) {
    sums[b] = partial[b];
    mine = min(mine, first_bad[b]);
  }
  bads[threadIdx.x] = mine;
  __syncthreads();
  if (threadIdx.x != 0) return;
  double s = 0.0;
  for (int b = 0; b < blocks; ++b) s += sums[b];
  int bad = kNoBad;
  for (int l = 0; l < kVerdictLanes; ++l) bad = min(bad, bads[l]);
  const bool nonfinite = !finite_f64(s);
  const int verdict = (nonfinite ? 1 : 0) | (launch_status != nullptr && launch_status[0] != 0 ? 2 : 0);
  if (nonfinite) {
    hyper[5] = 1.0f;
    hyper[6] = __uint_as_float(0x7f800000u);  // "not finite", whichever of NaN / inf the sum came out as
  } else {
    double c, norm;
    clip_coef(s, scale_dev, scale, max_norm, c, norm);
    hyper[5] = max_norm > 0.0f && c < 1.0 ? (float)c : 1.0f;
    hyper[6] = (float)norm;
  }
  guard[0] = verdict;
  if (verdict == 0) {
    guard[1] += 1;
    guard[3] = 0;
    adam_advance(hyper, beta1, beta2);
  } else {
    guard[2] += 1;
    guard[3] += 1;
    guard[4] = nonfinite ? bad : -1;
    guard[5] = guard[1] + guard[2];
  }
  guard[6] |= verdict;
  guard[7] = 0;
}

__global__ void guard_mark_kernel(const int* __restrict__ launch_status, float* __restrict__ grad) {
  if (launch_status[0] != 0) grad[0] = __uint_as_float(0x7fc00000u);  // quiet NaN
}

// mpa_guard_commit: the verdict is one plain load of the same word in every lane (uniform across the grid, as in
// adam_guarded_kernel) and picks the DIRECTION of a bitwise copy in 16-byte units: applied step, shadow <- live; skipped
// step, live <- shadow.  uint4, not float4: the bytes are counters and flags as well as statistics.
constexpr int kCommitBlocks = 512;
__global__ __launch_bounds__(kThreads) void guard_commit_kernel(const int* __restrict__ guard, uint4* live, uint4* shadow,
                                                                long long units) {
  const bool skipped = guard[0] != 0;
  const uint4* __restrict__ src = skipped ? shadow : live;
  uint4* __restrict__ dst = skipped ? live : shadow;
  const long long stride = (long long)gridDim.x * kThreads;
  for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < units; i += stride) dst[i] = src[i];
}

// host side of the three update entry points: the arguments that travel by value (lr, grad_scale and both bias corrections
// are zero here: mpa_adam_step fills them in, the other two read them from `hyper` on the device) and the grid
AdamArgs adam_args(float beta1, float beta2, float eps, float weight_decay, int decoupled) {
  AdamArgs a;
  a.lr = a.bc1 = a.bc2_sqrt = a.grad_scale = 0.0f;
  a.beta1 = beta1;
  a.beta2 = beta2;
  a.eps = eps;
  a.weight_decay = weight_decay;
  a.decoupled = decoupled;
  return a;
}

dim3 adam_grid(int64_t numel) {
  long long blocks = (numel / 4 + kThreads - 1) / kThreads;
  if (blocks < 1) blocks = 1;
  if (blocks > 2048) blocks = 2048;
  return dim3((unsigned)blocks);
}

}  // namespace

extern "C" int mpa_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                             int64_t numel, float lr, float beta1, float beta2, float eps,
                             float weight_decay, int decoupled_weight_decay, int64_t step,
                             float grad_scale, const float* decay_mask, void* stream) {
  MPA_REQUIRE(numel >= 0 && step >= 1, "adam_step: bad numel/step");
  if (numel == 0) return MPA_OK;
  MPA_REQUIRE(param && grad && exp_avg && exp_avg_sq, "adam_step: null pointer");
  MPA_REQUIRE(((uintptr_t)param | (uintptr_t)grad | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) % 16 == 0,
              "adam_step: buffers must be 16-byte aligned");
  AdamArgs a = adam_args(beta1, beta2, eps, weight_decay, decoupled_weight_decay);
  a.lr = lr;
  a.grad_scale = grad_scale;
  // bias corrections in double, as torch computes them on the host
  a.bc1 = (float)(1.0 - __builtin_pow((double)beta1, (double)step));
  a.bc2_sqrt = (float)__builtin_sqrt(1.0 - __builtin_pow((double)beta2, (double)step));
  hipLaunchKernelGGL(adam_kernel, adam_grid(numel), dim3(kThreads), 0, mpa::as_stream(stream),
                     param, grad, exp_avg, exp_avg_sq, (long long)numel, a, (const float*)nullptr, decay_mask);
  return mpa::check_launch("adam_step");
}

extern "C" int mpa_adam_step_dev(float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                                 int64_t numel, float* hyper, float beta1, float beta2, float eps,
                                 float weight_decay, int decoupled_weight_decay, const float* decay_mask,
                                 void* stream) {
  MPA_REQUIRE(numel >= 0, "adam_step_dev: bad numel");
  if (numel == 0) return MPA_OK;
  MPA_REQUIRE(param && grad && exp_avg && exp_avg_sq && hyper, "adam_step_dev: null pointer");
  MPA_REQUIRE(((uintptr_t)param | (uintptr_t)grad | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) % 16 == 0,
              "adam_step_dev: buffers must be 16-byte aligned");
  hipLaunchKernelGGL(adam_advance_kernel, dim3(1), dim3(1), 0, mpa::as_stream(stream), hyper, beta1, beta2);
  hipLaunchKernelGGL(adam_kernel, adam_grid(numel), dim3(kThreads), 0, mpa::as_stream(stream),
                     param, grad, exp_avg, exp_avg_sq, (long long)numel,
                     adam_args(beta1, beta2, eps, weight_decay, decoupled_weight_decay), (const float*)hyper, decay_mask);
  return mpa::check_launch("adam_step_dev");
}

extern "C" int mpa_grad_clip_workspace(int64_t* bytes) {
  MPA_REQUIRE(bytes != nullptr, "grad_clip_workspace: null pointer");
  *bytes = (int64_t)kNormBlocks * 8;
  return MPA_OK;
}

extern "C" int mpa_grad_clip_coef(const float* grad, int64_t numel, float max_norm, const float* grad_scale_dev,
                                  float grad_scale, void* ws, float* coef, void* stream) {
  MPA_REQUIRE(numel >= 0 && max_norm > 0.0f, "grad_clip_coef: bad numel / max_norm");
  MPA_REQUIRE(grad && ws && coef, "grad_clip_coef: null pointer");
  MPA_REQUIRE((uintptr_t)grad % 16 == 0 && (uintptr_t)ws % 8 == 0, "grad_clip_coef: misaligned buffer");
  hipStream_t s = mpa::as_stream(stream);
  double* partial = static_cast<double*>(ws);
  hipLaunchKernelGGL(grad_sqnorm_kernel, dim3(kNormBlocks), dim3(kThreads), 0, s, grad, (long long)numel, partial);
  hipLaunchKernelGGL(grad_clip_coef_kernel, dim3(1), dim3(1), 0, s, (const double*)partial, kNormBlocks, max_norm,
                     grad_scale_dev, grad_scale, coef);
  return mpa::check_launch("grad_clip_coef");
}

// ---- guarded step -----------------------------------------------------------------------------------------------------
// workspace: kNormBlocks double partial sums, then kNormBlocks int32 first-bad indices
extern "C" int mpa_step_guard_workspace(int64_t* bytes) {
  MPA_REQUIRE(bytes != nullptr, "step_guard_workspace: null pointer");
  *bytes = (int64_t)kNormBlocks * 8 + (int64_t)kNormBlocks * 4;
  return MPA_OK;
}

extern "C" int mpa_step_guard(const float* grad, int64_t numel, float max_norm, const float* grad_scale_dev,
                              float grad_scale, const int32_t* launch_status, void* ws, float* hyper, int32_t* guard,
                              float beta1, float beta2, void* stream) {
  MPA_REQUIRE(numel >= 0 && numel < ((int64_t)1 << 31), "step_guard: numel must lie in [0, 2^31) (the first-bad index is one int32 word)");
  MPA_REQUIRE((grad || numel == 0) && ws && hyper && guard, "step_guard: null pointer");
  MPA_REQUIRE((uintptr_t)grad % 16 == 0 && (uintptr_t)ws % 8 == 0, "step_guard: misaligned buffer");
  MPA_REQUIRE(((uintptr_t)hyper | (uintptr_t)guard | (uintptr_t)grad_scale_dev | (uintptr_t)launch_status) % 4 == 0,
              "step_guard: misaligned word");
  hipStream_t s = mpa::as_stream(stream);
  double* partial = static_cast<double*>(ws);
  int* first_bad = reinterpret_cast<int*>(partial + kNormBlocks);
  hipLaunchKernelGGL(grad_sqnorm_find_kernel, dim3(kNormBlocks), dim3(kThreads), 0, s, grad, (long long)numel, partial,
                     first_bad);
  hipLaunchKernelGGL(step_guard_verdict_kernel, dim3(1), dim3(kVerdictLanes), 0, s, (const double*)partial, (const int*)first_bad,
                     kNormBlocks, max_norm, grad_scale_dev, grad_scale, (const int*)launch_status, hyper, (int*)guard,
                     beta1, beta2);
  return mpa::check_launch("step_guard");
}

extern "C" int mpa_adam_step_guarded(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t numel,
                                     const float* hyper, float beta1, float beta2, float eps, float weight_decay,
                                     int decoupled_weight_decay, const float* decay_mask, const int32_t* guard,
                                     void* stream) {
  MPA_REQUIRE(numel >= 0, "adam_step_guarded: bad numel");
  if (numel == 0) return MPA_OK;
  MPA_REQUIRE(param && grad && exp_avg && exp_avg_sq && hyper && guard, "adam_step_guarded: null pointer");
  MPA_REQUIRE(((uintptr_t)param | (uintptr_t)grad | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) % 16 == 0,
              "adam_step_guarded: buffers must be 16-byte aligned");
  MPA_REQUIRE(((uintptr_t)hyper | (uintptr_t)guard) % 4 == 0, "adam_step_guarded: misaligned word");
  hipLaunchKernelGGL(adam_guarded_kernel, adam_grid(numel), dim3(kThreads), 0, mpa::as_stream(stream),
                     param, grad, exp_avg, exp_avg_sq, (long long)numel,
                     adam_args(beta1, beta2, eps, weight_decay, decoupled_weight_decay), hyper, decay_mask, (const int*)guard);
  return mpa::check_launch("adam_step_guarded");
}

extern "C" int mpa_guard_mark(const int32_t* launch_status, float* grad, int64_t numel, void* stream) {
  MPA_REQUIRE(numel >= 1, "guard_mark: numel must be at least 1 (the mark is element 0)");
  MPA_REQUIRE(launch_status && grad, "guard_mark: null pointer");
  MPA_REQUIRE(((uintptr_t)launch_status | (uintptr_t)grad) % 4 == 0, "guard_mark: misaligned word");
  hipLaunchKernelGGL(guard_mark_kernel, dim3(1), dim3(1), 0, mpa::as_stream(stream), (const int*)launch_status, grad);
  return mpa::check_launch("guard_mark");
}

extern "C" int mpa_guard_commit(const int32_t* guard, void* live, void* shadow, int64_t bytes, void* stream) {
  MPA_REQUIRE(guard != nullptr, "guard_commit: null pointer (the guard words)");
  MPA_REQUIRE((uintptr_t)guard % 4 == 0, "guard_commit: misaligned word");
  MPA_REQUIRE(bytes >= 0 && bytes % 16 == 0, "guard_commit: bytes must be a non-negative multiple of 16");
  if (bytes == 0) return MPA_OK;
  MPA_REQUIRE(live && shadow, "guard_commit: null pointer");
  MPA_REQUIRE(((uintptr_t)live | (uintptr_t)shadow) % 16 == 0, "guard_commit: buffers must be 16-byte aligned");
  const uintptr_t a = (uintptr_t)live, b = (uintptr_t)shadow;
  MPA_REQUIRE(a + (uintptr_t)bytes <= b || b + (uintptr_t)bytes <= a, "guard_commit: the two ranges overlap");
  const long long units = bytes / 16;
  long long blocks = (units + kThreads - 1) / kThreads;
  if (blocks > kCommitBlocks) blocks = kCommitBlocks;
  hipLaunchKernelGGL(guard_commit_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, mpa::as_stream(stream),
                     (const int*)guard, static_cast<uint4*>(live), static_cast<uint4*>(shadow), units);
  return mpa::check_launch("guard_commit");
}
