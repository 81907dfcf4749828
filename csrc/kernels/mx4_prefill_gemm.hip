// MXFP4 weight-only prefill GEMM (M > 64): one launch per projection where the skinny kernel
// (mx4_gemm.hip, M <= 64) needs one launch -- and one pass over the weights -- per 64 rows.
//
//   out[m, n] = epilogue( rstd[m] * sum_k X[m, k] * (e2m1(code[n, k]) * 2^(e8m0[n, k / 32] - 127)) )
//
// It reads the Mx4Weight planes of mx4_gemm.hip unchanged (layout in that file's header):
// codes u32 [G][P][64][4], scales u32 [G][P][16], G = N / 16 column groups, P = K / 128
// super-steps of four 32-wide k-steps.
//
// Work split.  One workgroup of 8 waves per BM x BN tile over the whole K (no split-K, no
// atomics: bit-identical from run to run), BM in {64, 128, 256}, BN in {64, 128}.  The waves
// form 4 rows x 2 columns: wave (wr, wc) owns the MTW = BM / 64 m-tiles (16 rows each)
// wr * MTW .. and the NW = BN / 32 weight streams (16-column groups) wc * NW ..  BN counts
// WEIGHT columns: SwiGLU pairs a gate group with the up group up_off further on, so a tile
// stores BN / 2 output columns there and BN elsewhere.
//
// Weights never touch LDS.  The storage order is the B-fragment order of
// v_mfma_f32_16x16x32_bf16: per super-step a wave loads one 16-byte word per lane and stream
// (plus the scale word), widens it in registers (widen_fp4, exact) and feeds the MFMA.  One
// widened fragment serves the wave's MTW m-tiles, so the conversion cost per MFMA falls with
// BM.  The codes of super-step p + 1 are loaded before the MFMAs of p (plain loads: the other
// row tiles of the grid read the same words out of L2).
//
// Activations go through LDS, double-buffered by super-step: As[2][BM][128 + 8] bf16.
//   stage: thread t loads 16-byte chunk (t & 15) of rows (t >> 4) + 32 i, i < BM / 32, of
//          super-step p + 1 into registers before the MFMAs of p and writes them to the
//          other buffer after them; one barrier per super-step (buffer b is written in step
//          p and was last read in step p - 1, a barrier earlier).  Rows >= M read row M - 1
//          and are never stored.
//   bank conflicts: a row is 256 B of data + 16 B of padding = 68 dwords.  The A-fragment
//          ds_read_b128 of lane (r = l & 15, q = l >> 4) at k-step h starts at dword
//          68 r + 16 h + 4 q: the 16 lanes of one q (one quarter-wave pass) start at banks
//          4 r + const (mod 64) and cover the 64 banks exactly once.  The staging
//          ds_write_b128 of 16 consecutive lanes covers one row's 64 consecutive dwords.
//   The LDS-DMA helpers (lds_pipe.h) are not used: a DMA lands a wave's 64 x 16 B
//   contiguously, which rules out the padded rows (it would need the XOR swizzle of
//   prefill_gemm.h on the global side and that file's counted waits); register staging keeps
//   every wait the compiler's own.  Not measured against a DMA variant.
//
// NORM: in-loop sums of squares over the A fragments the wave reads anyway (sumsq8); the two
// column waves of a row compute the same sums, nothing crosses waves.
// EPI_QKV_ROPE: the rows' slots and positions are fetched before the k loop, the (cos, sin)
// pairs per column group right after it.
//
// Registers reached per instantiation (kernel-resource-usage remarks of the build): the table
// at pf_tile_ok.  Zero scratch (_build.NO_SCRATCH).
#include "gemm_epilogue.h"
#include "mx4_common.h"

namespace {

constexpr int PF_THREADS = 512;
constexpr int PF_WC = 2;         // wave columns (x 4 wave rows)
constexpr int PF_LDA = 128 + 8;  // bf16 per LDS row

// The tile ladder.  LDS = 2 * BM * 272 B: 34, 68, 136 KiB of 160.  VGPRs reached (no AGPRs,
// no scratch; 256 available at 8 waves per workgroup), NORM on:
//   BM x BN      store / resid / silu / f32    qkv_rope
//    64 x  64     76                             90
//    64 x 128    106                            120
//   128 x  64    118                            142
//   128 x 128    158                            182
//   256 x  64    192                            192 (the rows' slots and positions are
//   256 x 128    248                            248  fetched after the k loop here)
// Without NORM 8 .. 48 fewer.
constexpr bool pf_tile_ok(int bm, int bn) {
  return (bm == 64 || bm == 128 || bm == 256) && (bn == 64 || bn == 128);
}

template <int BM, int BN, int EPI, bool NORM>
__global__ __launch_bounds__(PF_THREADS) void mx4_prefill_kernel(
    const u32x4* __restrict__ codes, const unsigned* __restrict__ scales,
    const bf16* __restrict__ X, int ldx, int M, int K, int gout, int up_off, int tiles_m,
    void* __restrict__ out, int ldo, float eps, EpiArgs ea) {
  constexpr int NB = (EPI == EPI_SILU) ? 2 : 1;
  constexpr int MTW = BM / 64;  // m-tiles per wave
  constexpr int NW = BN / 32;   // weight streams per wave
  constexpr int NGO = NW / NB;  // output column groups per wave
  constexpr int LPT = BM / 32;  // 16-byte staging chunks per thread and super-step
  __shared__ __attribute__((aligned(16))) bf16 As[2][BM * PF_LDA];

  const int P = K >> 7;
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);  // wave-uniform
  const int wr = w >> 1, wc = w & 1;
  const int r = lane & 15, q = lane >> 4;
  const int tm = blockIdx.x % tiles_m, tn = blockIdx.x / tiles_m;  // row tiles of one column
  const int m0 = tm * BM;                                           // tile run back to back
  const int go0 = (tn * PF_WC + wc) * NGO;  // the wave's first output group

  // weight streams: b = c * NB + h (h = 1: the up half).  A group past the last one (N not a
  // multiple of the tile) streams group 0 and is never stored.
  const u32x4* cb[NW];
  const unsigned* sb[NW];
#pragma unroll
  for (int c = 0; c < NGO; ++c)
#pragma unroll
    for (int h = 0; h < NB; ++h) {
      const int go = go0 + c;
      const size_t g = (size_t)((go < gout ? go : 0) + h * up_off);
      cb[c * NB + h] = codes + g * P * 64 + lane;
      sb[c * NB + h] = scales + g * P * 16 + r;
    }

  // staging: chunk (tid & 15) of rows (tid >> 4) + 32 i
  const bf16* xs[LPT];
  int sd[LPT];
#pragma unroll
  for (int i = 0; i < LPT; ++i) {
    const int row = (tid >> 4) + 32 * i;
    const int m = m0 + row < M ? m0 + row : M - 1;
    xs[i] = X + (size_t)m * ldx + 8 * (tid & 15);
    sd[i] = row * PF_LDA + 8 * (tid & 15);
  }

  // EPI_QKV_ROPE: the rows' KV slots and positions, fetched before the k loop (after it at
  // four m-tiles per wave, where 32 more live registers would spill)
  constexpr bool kEarly = MTW < 4;
  int rslot[MTW][4], rpos[MTW][4];
  auto load_rows = [&]() {
    if constexpr (EPI == EPI_QKV_ROPE) {
#pragma unroll
      for (int mt = 0; mt < MTW; ++mt)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int m = m0 + (wr * MTW + mt) * 16 + q * 4 + j;
          rslot[mt][j] = m < M ? ea.slots[m] : -1;
          rpos[mt][j] = m < M ? ea.pos[m] : 0;
        }
    }
  };
  if constexpr (kEarly) load_rows();

  f32x4 acc[NW][MTW];
  float ss[MTW];
#pragma unroll
  for (int b = 0; b < NW; ++b)
#pragma unroll
    for (int mt = 0; mt < MTW; ++mt) acc[b][mt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int mt = 0; mt < MTW; ++mt) ss[mt] = 0.f;

  u32x4 cw[NW], cwn[NW];
  unsigned sw[NW], swn[NW];
  bf16x8 st[LPT];
#pragma unroll
  for (int b = 0; b < NW; ++b) {
    cw[b] = cb[b][0];
    sw[b] = sb[b][0];
  }
#pragma unroll
  for (int i = 0; i < LPT; ++i) st[i] = *reinterpret_cast<const bf16x8*>(xs[i]);
#pragma unroll
  for (int i = 0; i < LPT; ++i) *reinterpret_cast<bf16x8*>(&As[0][sd[i]]) = st[i];
  __syncthreads();

  const int arow = (wr * MTW * 16 + r) * PF_LDA + 8 * q;  // the lane's A fragment, m-tile 0
  for (int p = 0; p < P; ++p) {
    const bool more = p + 1 < P;
    if (more) {
#pragma unroll
      for (int i = 0; i < LPT; ++i)
        st[i] = *reinterpret_cast<const bf16x8*>(xs[i] + (size_t)(p + 1) * 128);
#pragma unroll
      for (int b = 0; b < NW; ++b) {
        cwn[b] = cb[b][(size_t)(p + 1) * 64];
        swn[b] = sb[b][(size_t)(p + 1) * 16];
      }
    }
    const bf16* ab = &As[p & 1][arow];
#pragma unroll
    for (int h = 0; h < 4; ++h) {
      bf16x8 a[MTW], bw[NW];
#pragma unroll
      for (int mt = 0; mt < MTW; ++mt)
        a[mt] = *reinterpret_cast<const bf16x8*>(ab + mt * 16 * PF_LDA + h * 32);
#pragma unroll
      for (int b = 0; b < NW; ++b) bw[b] = widen_fp4(cw[b][h], sw[b], h);
#pragma unroll
      for (int mt = 0; mt < MTW; ++mt) {
#pragma unroll
        for (int b = 0; b < NW; ++b)
          acc[b][mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[mt], bw[b], acc[b][mt], 0, 0, 0);
        if constexpr (NORM) ss[mt] = sumsq8(a[mt], ss[mt]);
      }
    }
    if (more) {
#pragma unroll
      for (int i = 0; i < LPT; ++i) *reinterpret_cast<bf16x8*>(&As[(p + 1) & 1][sd[i]]) = st[i];
#pragma unroll
      for (int b = 0; b < NW; ++b) {
        cw[b] = cwn[b];
        sw[b] = swn[b];
      }
    }
    __syncthreads();
  }

  if constexpr (!kEarly) load_rows();

  // ---- epilogue: accumulator element j of a lane is row q * 4 + j, column r of its tile;
  // the row's sum of squares sits in the lanes with (l & 15) == row after the fold over q
  float rstd[MTW][4];
#pragma unroll
  for (int mt = 0; mt < MTW; ++mt) {
    if constexpr (NORM) {
      ss[mt] += __shfl_xor(ss[mt], 16, 64);
      ss[mt] += __shfl_xor(ss[mt], 32, 64);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      rstd[mt][j] = 1.f;
      if constexpr (NORM) rstd[mt][j] = rsqrtf(__shfl(ss[mt], q * 4 + j, 64) / (float)K + eps);
    }
  }
#pragma unroll
  for (int c = 0; c < NGO; ++c) {
    const int g = go0 + c;
    const bool gok = g < gout;
    float2 csv[MTW][4];
    if constexpr (EPI == EPI_QKV_ROPE) {
      const int kk = g & 7;
      const int dd = ((r < 8) ? 8 * kk + r : 64 + 8 * kk + (r - 8)) & 63;
#pragma unroll
      for (int mt = 0; mt < MTW; ++mt)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int m = m0 + (wr * MTW + mt) * 16 + q * 4 + j;
          csv[mt][j] = float2{1.f, 0.f};
          if (gok && m < M) csv[mt][j] = ea.cs[(size_t)rpos[mt][j] * 64 + dd];
        }
    }
#pragma unroll
    for (int mt = 0; mt < MTW; ++mt)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int m = m0 + (wr * MTW + mt) * 16 + q * 4 + j;
        const float s = rstd[mt][j];
        if constexpr (EPI == EPI_QKV_ROPE) {
          epi_store<EPI>(m, gok && m < M, g, r, acc[c][mt][j] * s, 0.f, out, ldo, ea, csv[mt][j],
                         rslot[mt][j]);
        } else {
          epi_store<EPI>(m, gok && m < M, g, r, acc[c * NB][mt][j] * s,
                         acc[c * NB + NB - 1][mt][j] * s, out, ldo, ea);
        }
      }
  }
}

// ------------------------------------------------------------------ launch ladder
struct PfPlan {
  int bm, bn, gout, up_off, tiles_m, tiles_n;
};

struct PfCall {
  const void *codes, *scales, *X;
  int ldx, M, K;
  void* out;
  int ldo;
  float eps;
  const EpiArgs* ea;
  hipStream_t st;
};

// Shape checks and the tile (code = BM / 64 | BN / 64 << 4; 0 = the default of this shape).
// False = not served.
bool pf_plan(int M, int K, int N, int epi, int norm, int code, PfPlan* pl) {
  if (M <= 64 || K <= 0 || (K % 128) != 0 || N <= 0 || (N % 16) != 0) return false;
  if (!(epi == EPI_STORE || epi == EPI_RESID || epi == EPI_SILU || epi == EPI_F32 ||
        epi == EPI_QKV_ROPE))
    return false;
  if (epi == EPI_QKV_ROPE && !norm) return false;
  const int nb = epi == EPI_SILU ? 2 : 1;
  if (N % (16 * nb)) return false;
  pl->gout = N / (16 * nb);
  pl->up_off = nb == 2 ? pl->gout : 0;
  if (code) {
    if (code < 0 || (code >> 8)) return false;
    pl->bm = (code & 0xf) * 64, pl->bn = (code >> 4) * 64;
    if (!pf_tile_ok(pl->bm, pl->bn)) return false;
  } else {
    // default tile by (rows, weight columns), from profiles/mx4_prefill_gemm.jsonl (8B and
    // 70B projections, 96..1024 rows; the fastest tile or within 10 % of it at every record):
    //   gate_up widths (N >= 16384): 256x128 where its grid still covers the chip, 128x64 at
    //     <= 128 rows and at 257..384 (a second, 128-row-full row of 256-row tiles idles);
    //   N >= 8192: 64x64 up to 256 rows, then 128x64;  narrower: 64x64 up to 512 rows, then
    //     128x64 -- the small tiles win until their grid is several rounds deep
    if (N >= 16384) {
      const bool small = M <= 128 || (M > 256 && M <= 384);
      pl->bm = small ? 128 : 256, pl->bn = small ? 64 : 128;
    } else {
      pl->bm = M <= (N >= 8192 ? 256 : 512) ? 64 : 128, pl->bn = 64;
    }
  }
  pl->tiles_m = (M + pl->bm - 1) / pl->bm;
  const int gt = PF_WC * (pl->bn / 32 / nb);  // output groups per tile
  pl->tiles_n = (pl->gout + gt - 1) / gt;
  return true;
}

template <int BM, int BN, int EPI, bool NORM>
int pf_launch(const PfPlan& pl, const PfCall& c) {
  hipLaunchKernelGGL((mx4_prefill_kernel<BM, BN, EPI, NORM>), dim3(pl.tiles_m * pl.tiles_n),
                     dim3(PF_THREADS), 0, c.st, (const u32x4*)c.codes, (const unsigned*)c.scales,
                     (const bf16*)c.X, c.ldx, c.M, c.K, pl.gout, pl.up_off, pl.tiles_m, c.out, c.ldo,
                     c.eps, *c.ea);
  return (int)hipGetLastError();
}

template <int EPI, bool NORM>
int pf_launch_t(const PfPlan& pl, const PfCall& c) {
  switch (pl.bm + pl.bn / 64) {
    case 64 + 1: return pf_launch<64, 64, EPI, NORM>(pl, c);
    case 64 + 2: return pf_launch<64, 128, EPI, NORM>(pl, c);
    case 128 + 1: return pf_launch<128, 64, EPI, NORM>(pl, c);
    case 128 + 2: return pf_launch<128, 128, EPI, NORM>(pl, c);
    case 256 + 1: return pf_launch<256, 64, EPI, NORM>(pl, c);
    case 256 + 2: return pf_launch<256, 128, EPI, NORM>(pl, c);
  }
  return (int)hipErrorInvalidValue;
}

template <int EPI>
int pf_launch_n(int norm, const PfPlan& pl, const PfCall& c) {
  if constexpr (EPI == EPI_QKV_ROPE) {
    return pf_launch_t<EPI, true>(pl, c);
  } else {
    return norm ? pf_launch_t<EPI, true>(pl, c) : pf_launch_t<EPI, false>(pl, c);
  }
}

int pf_dispatch(const void* codes, const void* scales, const void* X, int ldx, int M, int K, int N,
                int epi, int norm, void* out, int ldo, float eps, int code, const EpiArgs& ea,
                hipStream_t st) {
  PfPlan pl;
  if (!codes || !scales || !X || !pf_plan(M, K, N, epi, norm, code, &pl)) return (int)hipErrorInvalidValue;
  // 16-byte row chunks
  if (ldx < K || (ldx % 8) != 0 || ((uintptr_t)X & 15) != 0) return (int)hipErrorInvalidValue;
  const PfCall c = {codes, scales, X, ldx, M, K, out, ldo, eps, &ea, st};
  switch (epi) {
    case EPI_STORE: return pf_launch_n<EPI_STORE>(norm, pl, c);
    case EPI_RESID: return pf_launch_n<EPI_RESID>(norm, pl, c);
    case EPI_SILU: return pf_launch_n<EPI_SILU>(norm, pl, c);
    case EPI_F32: return pf_launch_n<EPI_F32>(norm, pl, c);
    case EPI_QKV_ROPE: return pf_launch_n<EPI_QKV_ROPE>(norm, pl, c);
  }
  return (int)hipErrorInvalidValue;
}

}  // namespace

// 1 if p2p_mx4_prefill_gemm / p2p_mx4_prefill_gemm_qkv_rope serve this shape with this tile
// code (0 = default)
P2P_API int p2p_mx4_prefill_ok(int M, int K, int N, int epi, int norm, int code) {
  PfPlan pl;
  return pf_plan(M, K, N, epi, norm, code, &pl) ? 1 : 0;
}

// As p2p_mx4_gemm for M > 64 rows in one launch.  code: BM / 64 | BN / 64 << 4, 0 = default.
// hipErrorInvalidValue for anything not served; nothing is launched then.
P2P_API int p2p_mx4_prefill_gemm(const void* codes, const void* scales, const void* X, int ldx,
                                 int M, int K, int N, int epi, int norm, void* out, int ldo,
                                 float eps, int code, hipStream_t stream) {
  if (epi == EPI_QKV_ROPE || !out) return (int)hipErrorInvalidValue;
  EpiArgs ea = {};
  return pf_dispatch(codes, scales, X, ldx, M, K, N, epi, norm, out, ldo, eps, code, ea, stream);
}

// Fused qkv projection (rows in ops.gemm.rope_row_perm order) + RoPE + KV-cache write.
P2P_API int p2p_mx4_prefill_gemm_qkv_rope(const void* codes, const void* scales, const void* X,
                                          int ldx, int M, int K, int Hq, int Hkv, const int* pos,
                                          const int* slots, const void* cos_sin, void* q_out,
                                          int ldq, void* k_cache, void* v_cache, float eps,
                                          int code, hipStream_t stream) {
  if (Hq <= 0 || Hkv <= 0 || !pos || !slots || !cos_sin || !q_out || !k_cache || !v_cache)
    return (int)hipErrorInvalidValue;
  EpiArgs ea = {};
  ea.pos = pos;
  ea.slots = slots;
  ea.cs = (const float2*)cos_sin;
  ea.q_out = (bf16*)q_out;
  ea.ldq = ldq;
  ea.kc = (bf16*)k_cache;
  ea.vc = (bf16*)v_cache;
  ea.Hq = Hq;
  ea.Hkv = Hkv;
  const int N = (Hq + 2 * Hkv) * HD;
  return pf_dispatch(codes, scales, X, ldx, M, K, N, EPI_QKV_ROPE, 1, nullptr, 0, eps, code, ea,
                     stream);
}
