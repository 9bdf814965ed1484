// PointNet++ set-abstraction level for evaluation, in one kernel: gather -> three (GEMM, per-channel scale / shift, ReLU)
// -> max over the samples of every centre, without the [M, C, S, K] tensors of the library chain ever existing.
// include/mpa_hip.h has the definition; multi_part_assembly_amd/pointnet2_ref.py (`sa_mlp_max`) restates it in numpy.
//
//   pack     one launch per layer: W [Cout, Cin] fp32 -> the three bf16 planes of dg_gemm_split.h (h + m + l == W exactly),
//            Cin zero-padded to the k-chunk of 32, laid out as the LDS panels are ([chunk][channel][h(32) | m(32) | l(32)]):
//            a wave's weight fragments of one chunk are 6 KiB of contiguous memory.  scale / shift behind the planes.
//   forward  a block of four waves owns a tile of ROWS rows of the virtual input (whole centres, K rows each; a centre with
//            K > ROWS is walked in tiles under a running maximum).  Products are the six-term split-bf16 form on
//            v_mfma_f32_32x32x16_bf16 (GS_MMA6).  Every wave owns 32 channels of a 128-channel column chunk and ALL rows of
//            the tile, so a weight fragment has exactly one reader: it goes from global memory (L2-resident, shared by
//            every block) straight to registers, and the k loops over resident activations have no barrier.
//              layer 1  the input is streamed: a 32-column chunk of [xyz - centre ; features] is gathered, split and staged
//                       in one LDS panel per k step; the output panel A1 (all C1 channels, split) stays in LDS.
//              layer 2  computed in column chunks of 128 channels out of A1; each chunk is split into the panel P2 and fed
//              layer 3  at once, as four k-chunks, into the accumulators of ALL C3 channels — the 512-wide layer of the
//                       last level never exists as a panel.  Layer 3's output is reduced from the accumulators.
//            Layers 1 and 2 run TRANSPOSED (weights as the MFMA's first operand): a lane then holds one row and four
//            consecutive channels per register quad, which is what one 8-byte panel store per plane wants.  Layer 3 runs
//            the other way round: a lane holds one channel and 16 rows, so the max over rows is in-lane; segments (centres)
//            end with one LDS integer max (the values are >= 0 after the ReLU, so their bit patterns order as integers
//            and 0 is the identity).  Rows that pad a tile carry segment -1 and take no part.
//            ROWS = 64 while A1 has at most four chunk panels (C1 <= 128), else 32: A1 + P2 + the maxima stay under 160 KiB.
#include "common.h"
#include "dg_gemm_split.h"

namespace {

using dg::f32x16;
using dg::Frag3;
using dg::kGsRow;

constexpr int kSaThreads = 256;
constexpr int kSaWaves = kSaThreads / mpa::kWave;
constexpr int kSaChunk = 32;          // k-chunk: the padding unit of Cin, one LDS panel
constexpr int kSaCols = 32 * kSaWaves;  // channels per column chunk (32 per wave)
constexpr int kSaMaxSeg = 8;          // centres per tile at most (rows of the maxima table)
constexpr int kSaMaxC = 512;
constexpr int kSaPlaneRow = 3 * kSaChunk * 2;  // bytes of one (chunk, channel) entry of a packed layer: 192
constexpr int64_t kSaInt31 = 1LL << 31;

__host__ __device__ inline int64_t sa_padded(int64_t cin) { return (cin + kSaChunk - 1) / kSaChunk * kSaChunk; }
inline int64_t sa_plane_bytes(int64_t cout, int64_t cin) { return sa_padded(cin) / kSaChunk * cout * kSaPlaneRow; }

// ---- pack ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sa_pack_kernel(const float* __restrict__ W, const float* __restrict__ gamma,
                                                      const float* __restrict__ beta, const float* __restrict__ mean,
                                                      const float* __restrict__ var, float eps, int Cout, int Cin, int Cinp,
                                                      unsigned char* __restrict__ packed) {
  const int e = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (e >= Cout * Cinp) return;
  const int n = e / Cinp, k = e % Cinp;
  const float x = k < Cin ? W[(int64_t)n * Cin + k] : 0.f;
  const __bf16 h = (__bf16)x;
  const float r = x - (float)h;
  const __bf16 m = (__bf16)r;
  const __bf16 l = (__bf16)(r - (float)m);
  __bf16* row = reinterpret_cast<__bf16*>(packed + ((int64_t)(k / kSaChunk) * Cout + n) * kSaPlaneRow);
  row[k % kSaChunk] = h;
  row[kSaChunk + k % kSaChunk] = m;
  row[2 * kSaChunk + k % kSaChunk] = l;
  if (e < Cout) {
    float* ss = reinterpret_cast<float*>(packed + (int64_t)(Cinp / kSaChunk) * Cout * kSaPlaneRow);
    const float sc = gamma[e] / sqrtf(var[e] + eps);
    ss[e] = sc;
    ss[Cout + e] = beta[e] - mean[e] * sc;
  }
}

// ---- forward -------------------------------------------------------------------------------------------------------------
struct SaLayer {
  const unsigned char* planes;  // [Cinp / 32][Cout][192]
  const float* scale;           // [Cout]
  const float* shift;           // [Cout]
};

// weight fragment of channel n, k-chunk c, k-step s (lane half hh): the layout of gs_frag, from global memory
__device__ __forceinline__ Frag3 sa_wfrag(const unsigned char* __restrict__ planes, int Cout, int n, int c, int s, int hh) {
  const unsigned char* p = planes + ((int64_t)c * Cout + n) * kSaPlaneRow + 32 * s + 16 * hh;
  Frag3 f;
  f.h = *reinterpret_cast<const dg::gs_bf16x8*>(p);
  f.m = *reinterpret_cast<const dg::gs_bf16x8*>(p + 64);
  f.l = *reinterpret_cast<const dg::gs_bf16x8*>(p + 128);
  return f;
}

// Epilogue of a transposed accumulator (lane = row `row` of the tile, register quad g = channels nb + 8 g + 4 hh ..+3):
// relu(scale * acc + shift), split, into chunk panel `panel`.
__device__ __forceinline__ void sa_store_act(unsigned char* panel, int row, int hh, const f32x16& acc,
                                             const float* __restrict__ scale, const float* __restrict__ shift, int nb) {
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const float4 sc = *reinterpret_cast<const float4*>(scale + nb + 8 * g + 4 * hh);
    const float4 sh = *reinterpret_cast<const float4*>(shift + nb + 8 * g + 4 * hh);
    float4 v;
    v.x = __builtin_fmaxf(sc.x * acc[4 * g + 0] + sh.x, 0.f);
    v.y = __builtin_fmaxf(sc.y * acc[4 * g + 1] + sh.y, 0.f);
    v.z = __builtin_fmaxf(sc.z * acc[4 * g + 2] + sh.z, 0.f);
    v.w = __builtin_fmaxf(sc.w * acc[4 * g + 3] + sh.w, 0.f);
    dg::gs_stash(panel, row, 2 * g + hh, v);
  }
}

// ROWS: tile height (32 | 64).  NT3: column chunks of layer 3, ceil(C3 / 128).
// Dynamic LDS: A1 [C1 / 32] panels | P2 [min(C2, 128) / 32] panels (panel 0 doubles as layer 1's staging panel) |
// maxima [kSaMaxSeg][C3] int | row table (source point, centre, segment) [ROWS].
template <int ROWS, int NT3>
__global__ __launch_bounds__(kSaThreads) void sa_mlp_max_kernel(const float* __restrict__ xyz,
                                                                const float* __restrict__ new_xyz,
                                                                const float* __restrict__ feat,
                                                                const int32_t* __restrict__ idx, int N, int S, int K, int C,
                                                                int64_t MS, int cpt, SaLayer L1, SaLayer L2, SaLayer L3,
                                                                int C1, int C2, int C3, float* __restrict__ out) {
  constexpr int RT = ROWS / 32;             // 32-row accumulator tiles
  constexpr int PANEL = ROWS * kGsRow;      // bytes of one chunk panel
  constexpr int TPR = kSaThreads / ROWS;    // staging threads per row
  constexpr int NQ = kSaChunk / 4 / TPR;    // float4 per staging thread and chunk
  extern __shared__ __attribute__((aligned(16))) unsigned char sa_lds[];
  const int p2_panels = (C2 < kSaCols ? C2 : kSaCols) / kSaChunk;
  unsigned char* A1 = sa_lds;
  unsigned char* P2 = A1 + (C1 / kSaChunk) * PANEL;
  int* red = reinterpret_cast<int*>(P2 + p2_panels * PANEL);
  int* s_src = red + kSaMaxSeg * C3;
  int* s_seg = s_src + ROWS;
  float* s_ctr = reinterpret_cast<float*>(s_seg + ROWS);  // [ROWS][3]

  const int t = threadIdx.x, wave = t >> 6, lane = t & 63, j = lane & 31, hh = lane >> 5;
  const int Cinp = (int)sa_padded(3 + C), in_chunks = Cinp / kSaChunk;
  const bool walk = K > ROWS;  // one centre per block, K walked in tiles
  const int64_t c_base = (int64_t)blockIdx.x * cpt;
  const int ktiles = walk ? (K + ROWS - 1) / ROWS : 1;

  for (int e = t; e < kSaMaxSeg * C3; e += kSaThreads) red[e] = 0;

  for (int kt = 0; kt < ktiles; ++kt) {
    // ---- the tile's rows: source point (m N + index, -1: reads as zero), centre, segment (-1: a padding row) ----
    __syncthreads();  // the previous tile's readers of the row table and the panels are done; `red` is cleared
    if (t < ROWS) {
      const int seg = walk ? 0 : t / K;
      const int l = walk ? kt * ROWS + t : t % K;
      const int64_t ci = c_base + seg;
      const bool valid = (walk ? l < K : seg < cpt) && ci < MS;
      int src = -1;
      float cx = 0.f, cy = 0.f, cz = 0.f;
      if (valid) {
        const int64_t m = ci / S;
        const int i = idx != nullptr ? idx[ci * K + l] : l;
        if ((unsigned)i < (unsigned)N) src = (int)(m * N + i);  // an index outside [0, N) is never dereferenced
        if (new_xyz != nullptr) {
          cx = new_xyz[ci * 3 + 0];
          cy = new_xyz[ci * 3 + 1];
          cz = new_xyz[ci * 3 + 2];
        }
      }
      s_src[t] = src;
      s_seg[t] = valid ? seg : -1;
      s_ctr[3 * t + 0] = cx;
      s_ctr[3 * t + 1] = cy;
      s_ctr[3 * t + 2] = cz;
    }
    __syncthreads();

    // ---- layer 1: the gathered input, streamed by k-chunk through the staging panel, into A1 ----
    {
      const int srow = t / TPR, scol = (t % TPR) * (4 * NQ);
      const int src = s_src[srow];
      const bool live = s_seg[srow] >= 0;
      const float cx = s_ctr[3 * srow + 0], cy = s_ctr[3 * srow + 1], cz = s_ctr[3 * srow + 2];
      const float* prow = xyz + (int64_t)(src < 0 ? 0 : src) * 3;
      const float* frow = feat + (int64_t)(src < 0 ? 0 : src) * C;
      for (int cc = 0; cc * kSaCols < C1; ++cc) {
        const int nb = cc * kSaCols + 32 * wave;
        const bool active = nb < C1;
        f32x16 acc[RT];
#pragma unroll
        for (int a = 0; a < RT; ++a) acc[a] = f32x16{0};
        for (int c = 0; c < in_chunks; ++c) {
          if (c > 0 || cc > 0) __syncthreads();  // the staging panel's readers are done
#pragma unroll
          for (int q = 0; q < NQ; ++q) {
            float v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
              const int vc = c * kSaChunk + scol + 4 * q + u;  // column of the virtual input
              float x = 0.f;
              if (live) {
                if (vc < 3) x = (src >= 0 ? prow[vc] : 0.f) - (vc == 0 ? cx : vc == 1 ? cy : cz);
                else if (vc - 3 < C && src >= 0) x = frow[vc - 3];
              }
              v[u] = x;
            }
            dg::gs_stash(P2, srow, scol / 4 + q, make_float4(v[0], v[1], v[2], v[3]));
          }
          __syncthreads();
          if (active) {
#pragma unroll
            for (int s = 0; s < 2; ++s) {
              const Frag3 wf = sa_wfrag(L1.planes, C1, nb + j, c, s, hh);
#pragma unroll
              for (int a = 0; a < RT; ++a) {
                const Frag3 af = dg::gs_frag(P2, 32 * a + j, s, hh);
                GS_MMA6(acc[a], wf, af)
              }
            }
          }
        }
        if (active) {
#pragma unroll
          for (int a = 0; a < RT; ++a) sa_store_act(A1 + (nb / kSaChunk) * PANEL, 32 * a + j, hh, acc[a], L1.scale, L1.shift, nb);
        }
      }
    }
    __syncthreads();  // A1 is complete; the staging panel is free

    // ---- layer 2 in column chunks, each fed at once into layer 3 ----
    f32x16 acc3[NT3][RT];
#pragma unroll
    for (int i = 0; i < NT3; ++i)
#pragma unroll
      for (int a = 0; a < RT; ++a) acc3[i][a] = f32x16{0};
    const int k1_chunks = C1 / kSaChunk;
    for (int cc = 0; cc * kSaCols < C2; ++cc) {
      const int nb = cc * kSaCols + 32 * wave;
      if (nb < C2) {
        f32x16 acc[RT];
#pragma unroll
        for (int a = 0; a < RT; ++a) acc[a] = f32x16{0};
        for (int c = 0; c < k1_chunks; ++c) {
#pragma unroll
          for (int s = 0; s < 2; ++s) {
            const Frag3 wf = sa_wfrag(L2.planes, C2, nb + j, c, s, hh);
#pragma unroll
            for (int a = 0; a < RT; ++a) {
              const Frag3 af = dg::gs_frag(A1 + c * PANEL, 32 * a + j, s, hh);
              GS_MMA6(acc[a], wf, af)
            }
          }
        }
#pragma unroll
        for (int a = 0; a < RT; ++a) sa_store_act(P2 + wave * PANEL, 32 * a + j, hh, acc[a], L2.scale, L2.shift, nb);
      }
      __syncthreads();  // the chunk of layer 2 is in P2
      const int left = (C2 - cc * kSaCols) / kSaChunk, nk = left < kSaWaves ? left : kSaWaves;
#pragma unroll
      for (int i = 0; i < NT3; ++i) {
        const int n3 = i * kSaCols + 32 * wave;
        if (n3 < C3) {
          for (int kc = 0; kc < nk; ++kc) {
#pragma unroll
            for (int s = 0; s < 2; ++s) {
              const Frag3 wf = sa_wfrag(L3.planes, C3, n3 + j, cc * kSaWaves + kc, s, hh);
#pragma unroll
              for (int a = 0; a < RT; ++a) {
                const Frag3 af = dg::gs_frag(P2 + kc * PANEL, 32 * a + j, s, hh);
                GS_MMA6(acc3[i][a], af, wf)
              }
            }
          }
        }
      }
      __syncthreads();  // P2 may be rewritten
    }

    // ---- layer 3's epilogue: lane = channel, registers = rows in ascending order; one LDS max per segment end ----
#pragma unroll
    for (int i = 0; i < NT3; ++i) {
      const int ch = i * kSaCols + 32 * wave + j;
      if (ch < C3) {
        const float sc = L3.scale[ch], sh = L3.shift[ch];
        int cur = -1;
        float mx = 0.f;
#pragma unroll
        for (int a = 0; a < RT; ++a)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int sg = s_seg[32 * a + dg::acc_row(r, hh)];
            if (sg != cur) {
              if (cur >= 0) atomicMax(&red[cur * C3 + ch], __float_as_int(mx));
              cur = sg;
              mx = 0.f;
            }
            if (sg >= 0) mx = __builtin_fmaxf(mx, sc * acc3[i][a][r] + sh);
          }
        if (cur >= 0) atomicMax(&red[cur * C3 + ch], __float_as_int(mx));
      }
    }
  }
  __syncthreads();
  for (int e = t; e < cpt * C3; e += kSaThreads) {
    const int64_t ci = c_base + e / C3;
    if (ci < MS) out[ci * C3 + e % C3] = __int_as_float(red[e]);
  }
}

struct SaShape {
  int rows, nt3, cpt;
  int64_t blocks;
  size_t lds;
};

SaShape sa_shape(int64_t MS, int64_t K, int64_t C1, int64_t C2, int64_t C3) {
  SaShape p;
  p.rows = C1 <= 128 ? 64 : 32;
  p.nt3 = (int)((C3 + kSaCols - 1) / kSaCols);
  if (K > p.rows) p.cpt = 1;
  else p.cpt = (int)(p.rows / K < kSaMaxSeg ? p.rows / K : kSaMaxSeg);
  p.blocks = (MS + p.cpt - 1) / p.cpt;
  const int64_t panel = (int64_t)p.rows * kGsRow;
  p.lds = (size_t)((C1 / kSaChunk + (C2 < kSaCols ? C2 : kSaCols) / kSaChunk) * panel + kSaMaxSeg * C3 * 4 + p.rows * 20);
  return p;
}

template <int ROWS, int NT3>
int sa_launch(const SaShape& p, hipStream_t s, const float* xyz, const float* new_xyz, const float* feat, const int32_t* idx,
              int N, int S, int K, int C, int64_t MS, SaLayer L1, SaLayer L2, SaLayer L3, int C1, int C2, int C3, float* out) {
  auto kern = sa_mlp_max_kernel<ROWS, NT3>;
  static bool reserved = false;  // the opt-in to more than 64 KB of dynamic LDS is per kernel, once (not inside a capture)
  if (p.lds > 64 * 1024 && !reserved) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) !=
        hipSuccess)
      return mpa::fail(MPA_EINVAL, "sa_mlp_max_forward: cannot reserve %zu bytes of LDS", p.lds);
    reserved = true;
  }
  hipLaunchKernelGGL(kern, dim3((unsigned)p.blocks), dim3(kSaThreads), p.lds, s, xyz, new_xyz, feat, idx, N, S, K, C, MS, p.cpt,
                     L1, L2, L3, C1, C2, C3, out);
  return mpa::check_launch("sa_mlp_max_forward");
}

bool sa_width_ok(int64_t c) { return c >= 32 && c <= kSaMaxC && c % 32 == 0; }

SaLayer sa_layer(const void* packed, int64_t cout, int64_t cin) {
  SaLayer l;
  l.planes = static_cast<const unsigned char*>(packed);
  l.scale = reinterpret_cast<const float*>(l.planes + sa_plane_bytes(cout, cin));
  l.shift = l.scale + cout;
  return l;
}

}  // namespace

extern "C" int mpa_sa_mlp_packed_bytes(int64_t Cout, int64_t Cin, int64_t* bytes) {
  MPA_REQUIRE(bytes != nullptr, "sa_mlp_packed_bytes: null pointer");
  MPA_REQUIRE(Cout >= 0 && Cin >= 0, "sa_mlp_packed_bytes: negative size (Cout=%lld, Cin=%lld)", (long long)Cout,
              (long long)Cin);
  MPA_REQUIRE(Cout * sa_padded(Cin) < kSaInt31, "sa_mlp_packed_bytes: Cout Cin = %lld must stay below 2^31",
              (long long)(Cout * Cin));
  *bytes = sa_plane_bytes(Cout, Cin) + 2 * Cout * (int64_t)sizeof(float);
  return MPA_OK;
}

extern "C" int mpa_sa_mlp_pack(const float* W, const float* gamma, const float* beta, const float* running_mean,
                               const float* running_var, float eps, int64_t Cout, int64_t Cin, void* packed, void* stream) {
  MPA_REQUIRE(Cout >= 0 && Cin >= 0, "sa_mlp_pack: negative size (Cout=%lld, Cin=%lld)", (long long)Cout, (long long)Cin);
  if (Cout == 0) return MPA_OK;
  MPA_REQUIRE(sa_width_ok(Cout), "sa_mlp_pack: Cout=%lld must be a multiple of 32 in [32, %d]", (long long)Cout, kSaMaxC);
  MPA_REQUIRE(Cin >= 1 && Cin <= kSaMaxC + 3, "sa_mlp_pack: Cin=%lld must lie in [1, %d]", (long long)Cin, kSaMaxC + 3);
  MPA_REQUIRE(W != nullptr && gamma != nullptr && beta != nullptr && running_mean != nullptr && running_var != nullptr &&
                  packed != nullptr,
              "sa_mlp_pack: null pointer");
  MPA_REQUIRE((reinterpret_cast<uintptr_t>(packed) & 15u) == 0, "sa_mlp_pack: the packed buffer must be 16-byte aligned");
  const int Cinp = (int)sa_padded(Cin);
  const unsigned blocks = (unsigned)((Cout * Cinp + 255) / 256);
  hipLaunchKernelGGL(sa_pack_kernel, dim3(blocks), dim3(256), 0, mpa::as_stream(stream), W, gamma, beta, running_mean,
                     running_var, eps, (int)Cout, (int)Cin, Cinp, static_cast<unsigned char*>(packed));
  return mpa::check_launch("sa_mlp_pack");
}

extern "C" int mpa_sa_mlp_max_forward(const float* xyz, const float* new_xyz, const float* features, const int32_t* idx,
                                      int64_t M, int64_t N, int64_t S, int64_t K, int64_t C, const void* layer1,
                                      const void* layer2, const void* layer3, int64_t C1, int64_t C2, int64_t C3, float* out,
                                      void* stream) {
  MPA_REQUIRE(M >= 0 && N >= 0 && S >= 0 && K >= 0 && C >= 0 && C1 >= 0 && C2 >= 0 && C3 >= 0,
              "sa_mlp_max_forward: negative size (M=%lld, N=%lld, S=%lld, K=%lld, C=%lld, C1=%lld, C2=%lld, C3=%lld)",
              (long long)M, (long long)N, (long long)S, (long long)K, (long long)C, (long long)C1, (long long)C2,
              (long long)C3);
  if (M == 0 || S == 0 || C3 == 0) return MPA_OK;
  MPA_REQUIRE(sa_width_ok(C1), "sa_mlp_max_forward: C1=%lld must be a multiple of 32 in [32, %d]", (long long)C1, kSaMaxC);
  MPA_REQUIRE(sa_width_ok(C2), "sa_mlp_max_forward: C2=%lld must be a multiple of 32 in [32, %d]", (long long)C2, kSaMaxC);
  MPA_REQUIRE(sa_width_ok(C3), "sa_mlp_max_forward: C3=%lld must be a multiple of 32 in [32, %d]", (long long)C3, kSaMaxC);
  MPA_REQUIRE(C <= kSaMaxC, "sa_mlp_max_forward: C=%lld must lie in [0, %d]", (long long)C, kSaMaxC);
  MPA_REQUIRE(K >= 1, "sa_mlp_max_forward: K=%lld must be at least 1", (long long)K);
  MPA_REQUIRE(N >= 1, "sa_mlp_max_forward: N=%lld must be at least 1", (long long)N);
  MPA_REQUIRE((new_xyz == nullptr) == (idx == nullptr),
              "sa_mlp_max_forward: new_xyz and idx are given together, or both NULL (one group of every point)");
  const bool all = idx == nullptr;
  MPA_REQUIRE(!all || (S == 1 && K == N), "sa_mlp_max_forward: one group of every point needs S=1 and K=N (S=%lld, K=%lld, N=%lld)",
              (long long)S, (long long)K, (long long)N);
  MPA_REQUIRE(3 * M * N < kSaInt31 && 3 * M * S < kSaInt31 && M * N * (C > 0 ? C : 1) < kSaInt31 && M * S * K < kSaInt31 &&
                  M * S * C3 < kSaInt31,
              "sa_mlp_max_forward: 3 M N = %lld, M N C = %lld, M S K = %lld and M S C3 = %lld must stay below 2^31",
              (long long)(3 * M * N), (long long)(M * N * C), (long long)(M * S * K), (long long)(M * S * C3));
  MPA_REQUIRE(xyz != nullptr && out != nullptr && layer1 != nullptr && layer2 != nullptr && layer3 != nullptr &&
                  (features != nullptr) == (C > 0),
              "sa_mlp_max_forward: null pointer (features are NULL exactly when C=0)");
  MPA_REQUIRE(((reinterpret_cast<uintptr_t>(layer1) | reinterpret_cast<uintptr_t>(layer2) | reinterpret_cast<uintptr_t>(layer3)) &
               15u) == 0,
              "sa_mlp_max_forward: the packed layers must be 16-byte aligned");
  const SaShape p = sa_shape(M * S, K, C1, C2, C3);
  MPA_REQUIRE(p.lds <= 160 * 1024, "sa_mlp_max_forward: %zu bytes of LDS", p.lds);
  const SaLayer L1 = sa_layer(layer1, C1, 3 + C), L2 = sa_layer(layer2, C2, C1), L3 = sa_layer(layer3, C3, C2);
  hipStream_t s = mpa::as_stream(stream);
#define SA_GO(ROWS, NT3)                                                                                                     \
  return sa_launch<ROWS, NT3>(p, s, xyz, new_xyz, features, idx, (int)N, (int)S, (int)K, (int)C, M * S, L1, L2, L3, (int)C1, \
                              (int)C2, (int)C3, out)
  if (p.rows == 64) {
    switch (p.nt3) {
      case 1: SA_GO(64, 1);
      case 2: SA_GO(64, 2);
      case 3: SA_GO(64, 3);
      default: SA_GO(64, 4);
    }
  }
  switch (p.nt3) {
    case 1: SA_GO(32, 1);
    case 2: SA_GO(32, 2);
    case 3: SA_GO(32, 3);
    default: SA_GO(32, 4);
  }
#undef SA_GO
}
