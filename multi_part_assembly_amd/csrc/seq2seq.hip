// The decoder of the B-LSTM baseline's seq2seq module — all P steps of the live layer of
//   DecoderRNN(nn.GRU(128, 528, 2 layers))     multi_part_assembly/models/b_lstm/seq2seq.py:67-137,165-191
// and its output head  y = W2 (W1 h + b1) + b2  (linear1; its LeakyReLU(True) has slope 1.0: the identity) in ONE launch
// per pass, instead of the library's per-step GRU call, two Linear layers and a dropout for every part.  Layer 1 of the
// decoder feeds only itself and never reaches the loss: it is not computed.
//
// Forward, per step t (the GRU cell is torch.nn.GRU's, gate order r|z|n, as in gru.hip):
//   input projection gi_t: teacher forcing -> read from `gi` (one GEMM outside over the detached, masked targets);
//                          free running   -> W_ih (mask_t * y_{t-1}) + b_ih formed here (x_0 = 0: gi_0 = b_ih)
//   h_t = GRU(gi_t, h_{t-1});  z1_t = W1 h_t + b1;  y_t = W2 z1_t + b2
// Grid: kDU = 3 hidden units per block, 176 blocks (the LDS holds a block's 9 rows of W_hh, its 2 rows of W1 and the
// whole previous hidden state: (9 + 2 + B) x 528 floats = 158 KB at B = 64).  Three exchanges per step through tagged
// words (gru_xchg.h, no grid barrier): every block publishes its slice of h_t and gathers all of it; blocks 0..127 own
// two units of z1 each and publish them; the same blocks own one column of y each, sum it from the z1 words (four fixed
// partial sums per sample, added in a fixed order) and publish it for the next step's free-running input.  The y a
// block publishes is the y it writes out: the value fed back and the value returned are the same.
//
// Backward: the head's gradient dL/dh_t of every step is known up front (batched GEMMs outside: y is fed back DETACHED,
// so no gradient flows along the feedback); this file runs BPTT over the 528-wide recurrence like gru.hip's backward —
// each block keeps its 9 x 528 slice of dW_hh in registers, hands the partial dL/dh_{t-1} of its rows to the others as
// tagged words and sums them in block order (no float atomics: bit-reproducible) — and also returns dL/dh_0, the
// gradient into the encoder's final states.  All blocks must be co-resident (176 <= CUs, one block per CU by LDS).
#include "common.h"
#include "gru_xchg.h"

namespace {

constexpr int kDH = 528;             // decoder hidden size: 2 x lstm_hidden_size (256) + 16 noise channels
constexpr int kDC = 128;             // decoder input / output width (pc_feat_dim)
constexpr int kDZ = 256;             // linear1's hidden width
constexpr int kDU = 3;               // hidden units per block
constexpr int kDBlocks = kDH / kDU;  // 176
constexpr int kDZU = 2;              // z1 units per head block
constexpr int kDHead = kDZ / kDZU;   // 128 head blocks: block j owns z1 units 2j, 2j + 1 and y column j
constexpr int kDT = 256;             // threads per block
constexpr int kDMaxB = 64;
static_assert(kDH % kDU == 0 && kDHead == kDC && kDHead <= kDBlocks && kDMaxB * kDU <= kDT && 4 * kDMaxB <= kDT, "layout");

__device__ __forceinline__ float sigmoidf_dec(float x) { return 1.0f / (1.0f + expf(-x)); }

size_t dec_fwd_smem(int B) { return sizeof(float) * (size_t)(3 * kDU + kDZU + B) * kDH; }
size_t dec_bwd_smem(int B) { return sizeof(float) * (size_t)(3 * kDU * kDH + B * kDH + B * 3 * kDU + B * kDU); }

// gi [T][B][3H] (teacher forcing) or null (free running; mask [T][B][C] or null = no dropout), h0 [B][H],
// teacher: null, or a device word an earlier launch of the stream wrote that picks the mode instead (0 = free running,
// gi then given but unread): every block reads it once, in front of the step loop, so all of them agree,
// wih [3H][C], bih [3H], whh [3H][H], bhh [3H], w1 [Z][H], b1 [Z], w2 [C][Z], b2 [C]
// -> hs [T][B][H], saved [T][B][4][H] (r, z, n, W_hn h + b_hn), z1 [T][B][Z], y [T][B][C].
// xh [2][B][H], xz [2][B][Z], xy [2][B][C]: tagged words by step parity, zeroed before the launch; tag = step + 1.
__global__ __launch_bounds__(kDT) void dec_fwd_kernel(const float* __restrict__ gi, const float* __restrict__ mask,
                                                      const float* __restrict__ h0, const float* __restrict__ wih,
                                                      const float* __restrict__ bih, const float* __restrict__ whh,
                                                      const float* __restrict__ bhh, const float* __restrict__ w1,
                                                      const float* __restrict__ b1, const float* __restrict__ w2,
                                                      const float* __restrict__ b2, int B, int T, float* __restrict__ hs,
                                                      float* __restrict__ saved, float* __restrict__ z1,
                                                      float* __restrict__ y, tagged_t* __restrict__ xh,
                                                      tagged_t* __restrict__ xz, tagged_t* __restrict__ xy,
                                                      int* __restrict__ status, int poll_limit,
                                                      const int* __restrict__ teacher) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int H = kDH, C = kDC, Z = kDZ;
  float* W = smem;                     // [3 * kDU][H]: rows r(u0..), z(..), n(..)
  float* W1s = W + 3 * kDU * H;        // [kDZU][H]: the head block's rows of W1
  float* hp = W1s + kDZU * H;          // [B][H]: h_{t-1} during the GRU phase, h_t after the gather
  __shared__ float red[kDT];
  const int blk = blockIdx.x, u0 = blk * kDU;
  const bool head = blk < kDHead, free_run = teacher != nullptr ? *teacher == 0 : gi == nullptr;
  for (int e = threadIdx.x; e < 3 * kDU * H; e += kDT) {
    const int row = e / H, k = e % H, gate = row / kDU, u = row % kDU;
    W[e] = whh[(long long)(gate * H + u0 + u) * H + k];
  }
  if (head)
    for (int e = threadIdx.x; e < kDZU * H; e += kDT) W1s[e] = w1[(long long)(kDZU * blk) * H + e];
  for (int e = threadIdx.x; e < B * H; e += kDT) hp[e] = h0[e];
  Poll budget{poll_limit, poll_limit, status, false};
  __syncthreads();
  for (int t = 0; t < T; ++t) {
    // ---- GRU phase: thread (sample b, own unit u)
    if (threadIdx.x < B * kDU) {
      const int b = threadIdx.x / kDU, u = threadIdx.x % kDU, c = u0 + u;
      float gr, gz, gn;
      if (!free_run) {
        const float* g = gi + ((long long)t * B + b) * 3 * H + c;
        gr = g[0], gz = g[H], gn = g[2 * H];
      } else {
        gr = bih[c], gz = bih[H + c], gn = bih[2 * H + c];
        if (t > 0) {  // x_t = mask_t * y_{t-1}: the y words the head blocks published in step t - 1
          const tagged_t* yr = xy + (long long)((t - 1) & 1) * B * C + (long long)b * C;
          const float* mk = mask == nullptr ? nullptr : mask + ((long long)t * B + b) * C;
          const float *wr = wih + (long long)c * C, *wz = wih + (long long)(H + c) * C, *wn = wih + (long long)(2 * H + c) * C;
          float ar = 0.0f, az = 0.0f, an = 0.0f;
          constexpr int PF = 32;
          for (int k0 = 0; k0 < C; k0 += PF) {
            float yv[PF];
            tagged_wait_all<PF>(yr + k0, 1, PF, (unsigned)t, budget, yv);
#pragma unroll
            for (int q = 0; q < PF; ++q) {
              const int k = k0 + q;
              const float x = mk == nullptr ? yv[q] : mk[k] * yv[q];
              ar = __builtin_fmaf(wr[k], x, ar);
              az = __builtin_fmaf(wz[k], x, az);
              an = __builtin_fmaf(wn[k], x, an);
            }
          }
          gr += ar, gz += az, gn += an;
        }
      }
      const float* hb = hp + b * H;
      const float *wr = W + (0 * kDU + u) * H, *wz = W + (1 * kDU + u) * H, *wn = W + (2 * kDU + u) * H;
      float ar = 0.0f, az = 0.0f, an = 0.0f;
#pragma unroll 4
      for (int k = 0; k < H; k += 4) {
        const float4 h4 = *reinterpret_cast<const float4*>(hb + k);
        const float4 r4 = *reinterpret_cast<const float4*>(wr + k);
        const float4 z4 = *reinterpret_cast<const float4*>(wz + k);
        const float4 n4 = *reinterpret_cast<const float4*>(wn + k);
        ar = __builtin_fmaf(h4.x, r4.x, ar);
        az = __builtin_fmaf(h4.x, z4.x, az);
        an = __builtin_fmaf(h4.x, n4.x, an);
        ar = __builtin_fmaf(h4.y, r4.y, ar);
        az = __builtin_fmaf(h4.y, z4.y, az);
        an = __builtin_fmaf(h4.y, n4.y, an);
        ar = __builtin_fmaf(h4.z, r4.z, ar);
        az = __builtin_fmaf(h4.z, z4.z, az);
        an = __builtin_fmaf(h4.z, n4.z, an);
        ar = __builtin_fmaf(h4.w, r4.w, ar);
        az = __builtin_fmaf(h4.w, z4.w, az);
        an = __builtin_fmaf(h4.w, n4.w, an);
      }
      const float r = sigmoidf_dec(gr + ar + bhh[c]);
      const float z = sigmoidf_dec(gz + az + bhh[H + c]);
      const float hn = an + bhh[2 * H + c];
      const float n = tanhf(gn + r * hn);
      const float hnew = (1.0f - z) * n + z * hb[c];
      hs[((long long)t * B + b) * H + c] = hnew;
      tagged_store(xh + (long long)(t & 1) * B * H + b * H + c, hnew, (unsigned)(t + 1));
      float* sv = saved + ((long long)t * B + b) * 4 * H;
      sv[c] = r;
      sv[H + c] = z;
      sv[2 * H + c] = n;
      sv[3 * H + c] = hn;
    }
    __syncthreads();  // every thread is done with h_{t-1}
    // ---- gather h_t (all units) into hp
    {
      const tagged_t* xr = xh + (long long)(t & 1) * B * H;
      constexpr int PF = 32;
      for (int e0 = threadIdx.x; e0 < B * H; e0 += PF * kDT) {
        float hv[PF];
        const int n = (B * H - e0 + kDT - 1) / kDT;
        tagged_wait_all<PF>(xr + e0, kDT, n < PF ? n : PF, (unsigned)(t + 1), budget, hv);
#pragma unroll
        for (int q = 0; q < PF; ++q) {
          const int e = e0 + q * kDT;
          if (e < B * H) hp[e] = hv[q];
        }
      }
    }
    __syncthreads();
    if (head) {
      // ---- z1 phase: thread (sample b, own z1 unit v)
      if (threadIdx.x < B * kDZU) {
        const int b = threadIdx.x / kDZU, v = threadIdx.x % kDZU, j = kDZU * blk + v;
        const float* hb = hp + b * H;
        const float* wv = W1s + v * H;
        float a = 0.0f;
#pragma unroll 4
        for (int k = 0; k < H; k += 4) {
          const float4 h4 = *reinterpret_cast<const float4*>(hb + k);
          const float4 w4 = *reinterpret_cast<const float4*>(wv + k);
          a = __builtin_fmaf(h4.x, w4.x, a);
          a = __builtin_fmaf(h4.y, w4.y, a);
          a = __builtin_fmaf(h4.z, w4.z, a);
          a = __builtin_fmaf(h4.w, w4.w, a);
        }
        a += b1[j];
        z1[((long long)t * B + b) * Z + j] = a;
        tagged_store(xz + (long long)(t & 1) * B * Z + b * Z + j, a, (unsigned)(t + 1));
      }
      // ---- y phase: column j = blk; thread (sample b, quarter g of the 256 z1 units)
      const int j = blk;
      float part = 0.0f;
      if (threadIdx.x < 4 * B) {
        const int b = threadIdx.x >> 2, g = threadIdx.x & 3;
        const tagged_t* zr = xz + (long long)(t & 1) * B * Z + (long long)b * Z + g * (Z / 4);
        const float* wj = w2 + (long long)j * Z + g * (Z / 4);
        constexpr int PF = 32;
        for (int k0 = 0; k0 < Z / 4; k0 += PF) {
          float zv[PF];
          tagged_wait_all<PF>(zr + k0, 1, PF, (unsigned)(t + 1), budget, zv);
#pragma unroll
          for (int q = 0; q < PF; ++q) part = __builtin_fmaf(wj[k0 + q], zv[q], part);
        }
      }
      red[threadIdx.x] = part;
      __syncthreads();
      if (threadIdx.x < B) {
        const int b = threadIdx.x;
        const float v = ((red[4 * b] + red[4 * b + 1]) + (red[4 * b + 2] + red[4 * b + 3])) + b2[j];
        y[((long long)t * B + b) * C + j] = v;
        if (free_run) tagged_store(xy + (long long)(t & 1) * B * C + b * C + j, v, (unsigned)(t + 1));
      }
      __syncthreads();  // red is rewritten by the next step
    }
  }
}

// backward through time.  dh [T][B][H] (the head's gradient w.r.t. h_t), hs / saved from the forward
// -> dgi [T][B][3H] (w.r.t. the gates' pre-activations incl. b_ih), dwhh [3H][H], dbhh [3H], dh0 [B][H].
// part [2][nblk][B][H]: per-step partial dL/dh_{t-1} of every block's rows (tag T - t).
__global__ __launch_bounds__(kDT) void dec_bwd_kernel(const float* __restrict__ dh_in, const float* __restrict__ h0,
                                                      const float* __restrict__ whh, const float* __restrict__ hs,
                                                      const float* __restrict__ saved, int B, int T,
                                                      float* __restrict__ dgi, float* __restrict__ dwhh,
                                                      float* __restrict__ dbhh, float* __restrict__ dh0,
                                                      tagged_t* __restrict__ part, int* __restrict__ status,
                                                      int poll_limit) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int H = kDH, R = 3 * kDU;
  constexpr int CPT = (H + kDT - 1) / kDT;  // columns per thread: k = threadIdx.x + kDT * c (< H)
  float* W = smem;                          // [R][H]
  float* hp = W + R * H;                    // [B][H] h_{t-1}
  float* dg = hp + B * H;                   // [B][R] gate gradients of the own rows (r, z, n-hidden)
  float* dhc = dg + B * R;                  // [B][kDU] carried dL/dh of the own units
  const int blk = blockIdx.x, nblk = gridDim.x, u0 = blk * kDU;
  for (int e = threadIdx.x; e < R * H; e += kDT) {
    const int row = e / H, k = e % H, gate = row / kDU, u = row % kDU;
    W[e] = whh[(long long)(gate * H + u0 + u) * H + k];
  }
  for (int e = threadIdx.x; e < B * kDU; e += kDT) dhc[e] = 0.0f;
  Poll budget{poll_limit, poll_limit, status, false};
  float dw[R][CPT], wreg[R][CPT];
  __syncthreads();
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int c = 0; c < CPT; ++c) {
      const int k = threadIdx.x + kDT * c;
      dw[r][c] = 0.0f;
      wreg[r][c] = k < H ? W[r * H + k] : 0.0f;
    }
  float db_acc = 0.0f;  // threads 0 .. R - 1: bias gradient of row threadIdx.x
  for (int t = T - 1; t >= 0; --t) {
    for (int e = threadIdx.x; e < B * (H / 4); e += kDT) {
      const int b = e / (H / 4), k = 4 * (e % (H / 4));
      const float* src = t == 0 ? h0 + (long long)b * H + k : hs + ((long long)(t - 1) * B + b) * H + k;
      *reinterpret_cast<float4*>(&hp[b * H + k]) = *reinterpret_cast<const float4*>(src);
    }
    __syncthreads();
    if (threadIdx.x < B * kDU) {
      const int e = threadIdx.x, b = e / kDU, u = e % kDU, c = u0 + u;
      float dh = dh_in[((long long)t * B + b) * H + c] + dhc[e];
      if (t < T - 1) {  // + what the other rows sent back through W_hh in step t + 1, in block order
        const tagged_t* pp = part + (long long)((t + 1) & 1) * nblk * B * H + (long long)b * H + c;
        constexpr int PF = 32;
        for (int k0 = 0; k0 < nblk; k0 += PF) {
          float pv[PF];
          const int n = nblk - k0 < PF ? nblk - k0 : PF;
          tagged_wait_all<PF>(pp + (long long)k0 * B * H, (long long)B * H, n, (unsigned)(T - (t + 1)), budget, pv);
#pragma unroll
          for (int q = 0; q < PF; ++q)
            if (q < n) dh += pv[q];
        }
      }
      const float* sv = saved + ((long long)t * B + b) * 4 * H;
      const float r = sv[c], z = sv[H + c], n = sv[2 * H + c], hn = sv[3 * H + c];
      const float hprev = hp[b * H + c];
      const float dn = dh * (1.0f - z), dz = dh * (hprev - n);
      const float dn_pre = dn * (1.0f - n * n);
      const float dr_pre = dn_pre * hn * r * (1.0f - r);
      const float dz_pre = dz * z * (1.0f - z);
      dhc[e] = dh * z;  // the direct path to h_{t-1}
      float* go = dgi + ((long long)t * B + b) * 3 * H;
      go[c] = dr_pre;
      go[H + c] = dz_pre;
      go[2 * H + c] = dn_pre;
      dg[b * R + u] = dr_pre;
      dg[b * R + kDU + u] = dz_pre;
      dg[b * R + 2 * kDU + u] = dn_pre * r;  // gradient w.r.t. (W_hn h + b_hn)
    }
    __syncthreads();
    // dW_hh[row][k] += sum_b dg[b][row] h_{t-1}[b][k];  db_hh[row] += sum_b dg[b][row]
    for (int b = 0; b < B; ++b) {
      float hk[CPT];
#pragma unroll
      for (int c = 0; c < CPT; ++c) {
        const int k = threadIdx.x + kDT * c;
        hk[c] = k < H ? hp[b * H + k] : 0.0f;
      }
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const float gv = dg[b * R + r];
#pragma unroll
        for (int c = 0; c < CPT; ++c) dw[r][c] = __builtin_fmaf(gv, hk[c], dw[r][c]);
      }
    }
    if (threadIdx.x < R) {
      float a = db_acc;
      for (int b = 0; b < B; ++b) a += dg[b * R + threadIdx.x];
      db_acc = a;
    }
    // partial dL/dh_{t-1}[b][k] = sum over the own rows of dg[b][row] W[row][k]
    tagged_t* po = part + (long long)(t & 1) * nblk * B * H + (long long)blk * B * H;
    const unsigned otag = (unsigned)(T - t);
    for (int b = 0; b < B; ++b) {
      float a[CPT];
#pragma unroll
      for (int c = 0; c < CPT; ++c) a[c] = 0.0f;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const float gv = dg[b * R + r];
#pragma unroll
        for (int c = 0; c < CPT; ++c) a[c] = __builtin_fmaf(gv, wreg[r][c], a[c]);
      }
#pragma unroll
      for (int c = 0; c < CPT; ++c) {
        const int k = threadIdx.x + kDT * c;
        if (k < H) tagged_store(po + (long long)b * H + k, a[c], otag);
      }
    }
    __syncthreads();  // hp, dg and dhc are rewritten by the next step
  }
  // dL/dh_0 of the own units: the direct path plus every block's partial of step 0, in block order
  if (threadIdx.x < B * kDU) {
    const int e = threadIdx.x, b = e / kDU, c = u0 + e % kDU;
    float dh = dhc[e];
    const tagged_t* pp = part + (long long)b * H + c;  // parity of step 0
    constexpr int PF = 32;
    for (int k0 = 0; k0 < nblk; k0 += PF) {
      float pv[PF];
      const int n = nblk - k0 < PF ? nblk - k0 : PF;
      tagged_wait_all<PF>(pp + (long long)k0 * B * H, (long long)B * H, n, (unsigned)T, budget, pv);
#pragma unroll
      for (int q = 0; q < PF; ++q)
        if (q < n) dh += pv[q];
    }
    dh0[(long long)b * H + c] = dh;
  }
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int gate = r / kDU, u = r % kDU;
#pragma unroll
    for (int c = 0; c < CPT; ++c) {
      const int k = threadIdx.x + kDT * c;
      if (k < H) dwhh[(long long)(gate * H + u0 + u) * H + k] = dw[r][c];
    }
  }
  if (threadIdx.x < R) {
    const int gate = threadIdx.x / kDU, u = threadIdx.x % kDU;
    dbhh[gate * H + u0 + u] = db_acc;
  }
}

int dec_check(int64_t B, int64_t T, const char* who) {
  MPA_REQUIRE(B >= 1 && B <= kDMaxB && T >= 1 && T <= 4096, "%s: 1 <= batch <= %d, 1 <= steps <= 4096", who, kDMaxB);
  return MPA_OK;
}

// saved gates | 8-byte tagged exchange words: forward [2][B][H + Z + C], backward [2][nblk][B][H] | padding
struct DecWs { float* saved; tagged_t* xch; int64_t total; };
DecWs dec_carve(float* ws, int64_t B, int64_t T) {
  mpa::Arena a(ws);
  const int64_t fwd = 2 * B * (kDH + kDZ + kDC), bwd = 2LL * kDBlocks * B * kDH;
  float* saved = a.take<float>(T * B * 4 * kDH, 4);
  tagged_t* xch = a.take<tagged_t>(fwd > bwd ? fwd : bwd, 4);  // (8-byte aligned when the workspace is: the launchers check)
  a.take<float>(64, 4);
  return {saved, xch, a.elems<float>()};
}

}  // namespace

extern "C" int mpa_seq2seq_decoder_resident(int64_t B, int* ok) {
  MPA_REQUIRE(ok != nullptr, "seq2seq_decoder_resident: null pointer");
  *ok = 0;
  if (B < 1 || B > kDMaxB) return MPA_OK;
  int st = gru_resident(dec_fwd_kernel, dec_fwd_smem((int)B), kDBlocks, "seq2seq_decoder", kDT);
  if (st == MPA_OK) st = gru_resident(dec_bwd_kernel, dec_bwd_smem((int)B), kDBlocks, "seq2seq_decoder", kDT);
  *ok = st == MPA_OK;
  return MPA_OK;
}

extern "C" int mpa_seq2seq_decoder_workspace(int64_t B, int64_t T, int64_t* float_elems) {
  if (int st = dec_check(B, T, "seq2seq_decoder_workspace")) return st;
  MPA_REQUIRE(float_elems != nullptr, "seq2seq_decoder_workspace: null pointer");
  *float_elems = dec_carve(nullptr, B, T).total;
  return MPA_OK;
}

namespace {

int dec_forward(const char* who, const float* gi, const float* mask, const int32_t* teacher, const float* h0,
                const float* wih, const float* bih, const float* whh, const float* bhh, const float* w1, const float* b1,
                const float* w2, const float* b2, int64_t B, int64_t T, float* ws, float* hs, float* z1, float* y,
                int32_t* status, void* stream) {
  if (int st = dec_check(B, T, who)) return st;
  MPA_REQUIRE(h0 && wih && bih && whh && bhh && w1 && b1 && w2 && b2 && ws && hs && z1 && y, "%s: null pointer", who);
  hipStream_t s = mpa::as_stream(stream);
  const auto [saved, xh, total] = dec_carve(ws, B, T);
  MPA_REQUIRE((uintptr_t)xh % 8 == 0, "%s: workspace must be 8-byte aligned", who);
  tagged_t* xz = xh + 2 * B * kDH;
  tagged_t* xy = xz + 2 * B * kDZ;
  const size_t smem = dec_fwd_smem((int)B);
  MPA_REQUIRE(smem <= 160 * 1024, "%s: the batch does not fit the 160 KB of LDS", who);
  mpa::zero_words_async(xh, 2 * 2 * B * (kDH + kDZ + kDC), s);  // load-bearing: tags run 1..T in every launch
  static size_t checked = 0;  // LDS request + co-residency of the whole grid, once per footprint
  if (smem != checked) {
    if (int st = gru_resident(dec_fwd_kernel, smem, kDBlocks, who, kDT)) return st;
    checked = smem;
  }
  hipLaunchKernelGGL(dec_fwd_kernel, dim3(kDBlocks), dim3(kDT), smem, s, gi, mask, h0, wih, bih, whh, bhh, w1, b1, w2, b2,
                     (int)B, (int)T, hs, saved, z1, y, xh, xz, xy, (int*)status, poll_limit(), (const int*)teacher);
  return mpa::check_launch(who);
}

}  // namespace

extern "C" int mpa_seq2seq_decoder_forward(const float* gi, const float* mask, const float* h0, const float* wih,
                                           const float* bih, const float* whh, const float* bhh, const float* w1,
                                           const float* b1, const float* w2, const float* b2, int64_t B, int64_t T,
                                           float* ws, float* hs, float* z1, float* y, int32_t* status, void* stream) {
  return dec_forward("seq2seq_decoder_forward", gi, mask, nullptr, h0, wih, bih, whh, bhh, w1, b1, w2, b2, B, T, ws, hs,
                     z1, y, status, stream);
}

extern "C" int mpa_seq2seq_decoder_forward_sel(const float* gi, const float* mask, const int32_t* teacher,
                                               const float* h0, const float* wih, const float* bih, const float* whh,
                                               const float* bhh, const float* w1, const float* b1, const float* w2,
                                               const float* b2, int64_t B, int64_t T, float* ws, float* hs, float* z1,
                                               float* y, int32_t* status, void* stream) {
  MPA_REQUIRE(gi != nullptr && teacher != nullptr, "seq2seq_decoder_forward_sel: null pointer (gi and teacher are both "
              "given: the mode is read on the device)");
  return dec_forward("seq2seq_decoder_forward_sel", gi, mask, teacher, h0, wih, bih, whh, bhh, w1, b1, w2, b2, B, T, ws,
                     hs, z1, y, status, stream);
}

extern "C" int mpa_seq2seq_decoder_backward(const float* dh, const float* h0, const float* whh, const float* hs,
                                            int64_t B, int64_t T, float* ws, float* dgi, float* dwhh, float* dbhh,
                                            float* dh0, int32_t* status, void* stream) {
  if (int st = dec_check(B, T, "seq2seq_decoder_backward")) return st;
  MPA_REQUIRE(dh && h0 && whh && hs && ws && dgi && dwhh && dbhh && dh0, "seq2seq_decoder_backward: null pointer");
  hipStream_t s = mpa::as_stream(stream);
  const auto [saved, part, total] = dec_carve(ws, B, T);
  MPA_REQUIRE((uintptr_t)part % 8 == 0, "seq2seq_decoder_backward: workspace must be 8-byte aligned");
  const size_t smem = dec_bwd_smem((int)B);
  MPA_REQUIRE(smem <= 160 * 1024, "seq2seq_decoder_backward: the batch does not fit the 160 KB of LDS");
  mpa::zero_words_async(part, 2 * 2LL * kDBlocks * B * kDH, s);  // load-bearing, see the forward
  static size_t checked = 0;
  if (smem != checked) {
    if (int st = gru_resident(dec_bwd_kernel, smem, kDBlocks, "seq2seq_decoder_backward", kDT)) return st;
    checked = smem;
  }
  hipLaunchKernelGGL(dec_bwd_kernel, dim3(kDBlocks), dim3(kDT), smem, s, dh, h0, whh, hs, saved, (int)B, (int)T, dgi,
                     dwhh, dbhh, dh0, part, (int*)status, poll_limit());
  return mpa::check_launch("seq2seq_decoder_backward");
}
