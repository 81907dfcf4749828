// MXFP4 weight-only grouped (per-expert) prefill GEMM: the tile of mx4_prefill_gemm.hip applied
// to an expert's gathered rows, for the launches above 64 rows where the window kernel
// (mx4_moe_gemm.hip) streams a block's weights once per 64-row window and every A fragment
// once per column-group block.  The contract is p2p_mx4_grouped_gemm's:
//
//   for every local expert e, i < min(cnt[e], max_rows), slot = rows[e * rows_stride + i]:
//     out[slot] = epi( rstd(X[slot / x_div]) * X[slot / x_div] @ W_e^T )
//   EPI_SILU  (norm = 1): silu(gate) * up, gate / up = column groups g and g + N / 32
//   EPI_STORE (norm = 0): times row_w[slot] when row_w != null
//
// on the same stacked Mx4Weight planes: codes u32 [E][G][P][64][4], scales u32 [E][G][P][16],
// G = N / 16, P = K / 128 (layout in mx4_gemm.hip).
//
// Work split.  One workgroup of 8 waves per BM x BN tile over the whole K (no split-K, no
// atomics: bit-identical from run to run), BM in {64, 128, 256} list entries of one expert, BN
// in {64, 128} weight columns.  The host knows max_rows only (no sync, the launch can be
// captured), so every expert gets ceil(max_rows / BM) row tiles; a block reads cnt[e] (one
// scalar load) and with n = min(cnt[e], max_rows) - BM * tile <= 0 returns before any barrier
// and any weight load.
//
// Grid: one dimension, row tiles x experts x column tiles, walked through xcd_remap
// (common.h): logical id i = row tile + tiles_m * (expert + E * column tile).  The row tiles
// of one (expert, column tile) are consecutive on ONE XCD, so their repeats of the weight
// words hit that XCD's L2, and every XCD gets a contiguous range of column tiles of all
// experts.  On a plain (row tiles x column tiles, experts) grid the hardware deals the row
// tiles of one unit round-robin over the 8 XCDs and each reads the weights into its own L2:
// measured with 64-row tiles, the remap is 2.0x faster at 512 tokens x top-2 over 8 experts
// and 2.8x at 1024.  Not explained by either grid: tiles that leave 2 or 4 row tiles per
// expert with only the first filled (128-row tiles at 192 and 256 tokens, 64-row tiles at
// 256) ran 2.3x .. 3x slower than the same tile one token count lower; the default tile
// (gp_plan) steers clear of them.
//
// The waves form 4 rows x 2 columns.  Wave (wr, wc) owns the NW = BN / 32 weight streams
// wc * NW .. (SwiGLU: gate / up pairs) and the MTW = BM / 64 m-tiles wr, wr + 4, wr + 8, ..
// of 16 list entries each -- interleaved, not consecutive as in the dense kernel: a tile
// filled to n entries has ceil(n / 16) live m-tiles, and interleaving spreads them over the
// four wave rows (256 tokens x top-2 over 8 experts: 64 entries per expert on average, one
// m-tile per wave row whatever BM).  live = the wave's m-tiles below ceil(n / 16) is
// wave-uniform and selects one of MTW + 1 copies of the k loop, compiled for exactly that many
// m-tiles: a tile wholly past n costs no A load, no MFMA and no epilogue work, a wave with no
// live tile loads no weights, and every wave still stages its share of A and meets every
// barrier.
//
// Weights never touch LDS: per super-step one 16-byte code word per lane and stream plus the
// scale word, loaded one super-step ahead and widened once (widen_fp4) for all of the wave's
// m-tiles.  Column groups past N / 16 (ragged N) stream group 0 and are never stored.
//
// Activations go through LDS, double-buffered by super-step, in the dense kernel's padded,
// conflict-free rows (As[2][BM][128 + 8] bf16, the argument is in mx4_prefill_gemm.hip).  The
// rows are gathered: before the k loop threads 0 .. BM - 1 stage the tile's list into LDS --
// slot, X row (slot / x_div: the one division per entry) and row weight; entries past n take
// the tile's first entry (an MFMA output row depends on its own A row only) and are never
// stored.  A staging thread keeps the 32-bit X rows of its BM / 32 chunks in registers (half
// of the dense kernel's 64-bit pointers; the 256-row tiles re-read them from LDS every
// super-step instead: with eight more live registers 256 x 128 SwiGLU spilled 68 B) and skips
// the 16-row groups past n; the epilogue takes slot and row weight from the LDS list, so it
// waits for no dependent global load.
//
// NORM (w13): sums of squares over the A fragments the wave reads anyway; nothing crosses waves.
//
// Registers reached per instantiation: the table at gp_tile_ok.  Zero scratch
// (_build.NO_SCRATCH).
#include <type_traits>

#include "gemm_epilogue.h"
#include "mx4_common.h"

namespace {

constexpr int GP_THREADS = 512;
constexpr int GP_WC = 2;         // wave columns (x 4 wave rows)
constexpr int GP_LDA = 128 + 8;  // bf16 per LDS row

// The tile ladder.  LDS = 2 * BM * 272 B + the list (BM * 8 B, 12 B with row weights): 34.5,
// 69, 138 KiB (34.75, 69.5, 139) of 160.  VGPRs reached (no AGPRs, no scratch; 256 available
// at 8 waves per workgroup):
//   BM x BN      silu (norm)   store
//    64 x  64      82            73
//    64 x 128     112          104
//   128 x  64     139          117
//   128 x 128     190          164
//   256 x  64     185          137
//   256 x 128     243          195
constexpr bool gp_tile_ok(int bm, int bn) {
  return (bm == 64 || bm == 128 || bm == 256) && (bn == 64 || bn == 128);
}

struct GpLists {
  const int* cnt;      // [E] rows routed to each local expert
  const int* rows;     // [E][rows_stride] their slots
  const float* row_w;  // [slots] or null
  int rows_stride, x_div, max_rows;
  long long stride_codes, stride_scales;  // per expert, in u32x4 / u32
};

template <int L>
using gp_tiles_c = std::integral_constant<int, L>;

template <int BM, int BN, int EPI>
__global__ __launch_bounds__(GP_THREADS) void mx4_moe_prefill_kernel(
    const u32x4* __restrict__ codes, const unsigned* __restrict__ scales,
    const bf16* __restrict__ X, int ldx, int K, int gout, int up_off, int tiles_m, int n_experts,
    bf16* __restrict__ out, int ldo, float eps, GpLists ml) {
  constexpr bool NORM = EPI == EPI_SILU;
  constexpr int NB = NORM ? 2 : 1;
  constexpr int MTW = BM / 64;  // m-tiles per wave
  constexpr int NW = BN / 32;   // weight streams per wave
  constexpr int NGO = NW / NB;  // output column groups per wave
  constexpr int LPT = BM / 32;  // 16-byte staging chunks per thread and super-step
  const int bid = xcd_remap(blockIdx.x, gridDim.x);
  const int tm = bid % tiles_m, unit = bid / tiles_m;
  const int e = unit % n_experts, tn = unit / n_experts;
  const int n = min(ml.cnt[e], ml.max_rows) - BM * tm;  // list entries of this tile
  if (n <= 0) return;                                   // whole block: before any barrier

  __shared__ __attribute__((aligned(16))) bf16 As[2][BM * GP_LDA];
  __shared__ int l_slot[BM], l_xrow[BM];
  __shared__ float l_w[EPI == EPI_STORE ? BM : 1];

  const int P = K >> 7;
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);  // wave-uniform
  const int wr = w >> 1, wc = w & 1;
  const int r = lane & 15, q = lane >> 4;
  const int nt = min(BM / 16, (n + 15) >> 4);  // live m-tiles of the block
  const int live = (nt - wr + 3) >> 2;         // of this wave: tiles wr + 4 mt < nt
  const int go0 = (tn * GP_WC + wc) * NGO;     // the wave's first output group

  // ---- the tile's list: slot, X row and row weight of entry i (entries past n: the first)
  if (tid < BM) {
    const int* rl = ml.rows + (size_t)e * ml.rows_stride + (size_t)BM * tm;
    const int s = rl[tid < n ? tid : 0];
    l_slot[tid] = s;
    l_xrow[tid] = (int)((unsigned)s / (unsigned)ml.x_div);
    if constexpr (EPI == EPI_STORE) l_w[tid] = ml.row_w ? ml.row_w[s] : 1.f;
  }
  __syncthreads();

  // staging: chunk (tid & 15) of entries (tid >> 4) + 32 i; a wave's four entries lie in one
  // 16-entry group, so "below nt * 16" is wave-uniform
  const int srow = tid >> 4, scol = 8 * (tid & 15);
  const int nrows = nt * 16;
  constexpr bool kKeep = LPT < 8;  // 256-row tiles re-read the X row from LDS per super-step
  int xrow[kKeep ? LPT : 1];
  if constexpr (kKeep) {
#pragma unroll
    for (int i = 0; i < LPT; ++i) xrow[i] = srow + 32 * i < nrows ? l_xrow[srow + 32 * i] : 0;
  }

  f32x4 acc[NW][MTW];
  float ss[MTW];
#pragma unroll
  for (int b = 0; b < NW; ++b)
#pragma unroll
    for (int mt = 0; mt < MTW; ++mt) acc[b][mt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int mt = 0; mt < MTW; ++mt) ss[mt] = 0.f;

  // ---- the k loop, compiled for L live m-tiles of this wave
  auto run = [&](auto tiles) {
    constexpr int L = decltype(tiles)::value;
    constexpr int LW = L > 0 ? NW : 0;  // a wave with no live tile streams no weights
    // weight streams: b = c * NB + h (h = 1: the up half); wave-uniform bases
    const u32x4* cb[NW];
    const unsigned* sb[NW];
#pragma unroll
    for (int c = 0; c < NGO; ++c)
#pragma unroll
      for (int h = 0; h < NB; ++h) {
        const int go = go0 + c;
        const size_t g = (size_t)((go < gout ? go : 0) + h * up_off);
        cb[c * NB + h] = codes + (size_t)e * ml.stride_codes + g * P * 64;
        sb[c * NB + h] = scales + (size_t)e * ml.stride_scales + g * P * 16;
      }
    u32x4 cw[NW], cwn[NW];
    unsigned sw[NW], swn[NW];
    bf16x8 st[LPT];
    auto stage_load = [&](int p) {
#pragma unroll
      for (int i = 0; i < LPT; ++i)
        if (srow + 32 * i < nrows) {
          const int xr = kKeep ? xrow[kKeep ? i : 0] : l_xrow[srow + 32 * i];
          st[i] = *reinterpret_cast<const bf16x8*>(X + (size_t)xr * ldx + (size_t)p * 128 + scol);
        }
    };
    auto stage_store = [&](int p) {
#pragma unroll
      for (int i = 0; i < LPT; ++i)
        if (srow + 32 * i < nrows)
          *reinterpret_cast<bf16x8*>(&As[p & 1][(srow + 32 * i) * GP_LDA + scol]) = st[i];
    };
#pragma unroll
    for (int b = 0; b < LW; ++b) {
      cw[b] = cb[b][lane];
      sw[b] = sb[b][r];
    }
    stage_load(0);
    stage_store(0);
    __syncthreads();

    const int arow = (wr * 16 + r) * GP_LDA + 8 * q;  // the lane's A fragment, m-tile 0
    for (int p = 0; p < P; ++p) {
      const bool more = p + 1 < P;
      if (more) {
        stage_load(p + 1);
#pragma unroll
        for (int b = 0; b < LW; ++b) {
          cwn[b] = cb[b][(size_t)(p + 1) * 64 + lane];
          swn[b] = sb[b][(size_t)(p + 1) * 16 + r];
        }
      }
      if constexpr (L > 0) {
        const bf16* ab = &As[p & 1][arow];
#pragma unroll
        for (int h = 0; h < 4; ++h) {
          bf16x8 a[L], bw[NW];
#pragma unroll
          for (int mt = 0; mt < L; ++mt)
            a[mt] = *reinterpret_cast<const bf16x8*>(ab + mt * 64 * GP_LDA + h * 32);
#pragma unroll
          for (int b = 0; b < NW; ++b) bw[b] = widen_fp4(cw[b][h], sw[b], h);
#pragma unroll
          for (int mt = 0; mt < L; ++mt) {
#pragma unroll
            for (int b = 0; b < NW; ++b)
              acc[b][mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[mt], bw[b], acc[b][mt], 0, 0, 0);
            if constexpr (NORM) ss[mt] = sumsq8(a[mt], ss[mt]);
          }
        }
      }
      if (more) {
        stage_store(p + 1);
#pragma unroll
        for (int b = 0; b < LW; ++b) {
          cw[b] = cwn[b];
          sw[b] = swn[b];
        }
      }
      __syncthreads();
    }
  };
  if constexpr (MTW == 1) {
    if (live <= 0) run(gp_tiles_c<0>{});
    else run(gp_tiles_c<1>{});
  } else if constexpr (MTW == 2) {
    if (live <= 0) run(gp_tiles_c<0>{});
    else if (live == 1) run(gp_tiles_c<1>{});
    else run(gp_tiles_c<2>{});
  } else {
    switch (live) {
      case 1: run(gp_tiles_c<1>{}); break;
      case 2: run(gp_tiles_c<2>{}); break;
      case 3: run(gp_tiles_c<3>{}); break;
      case 4: run(gp_tiles_c<4>{}); break;
      default: run(gp_tiles_c<0>{}); break;
    }
  }

  // ---- epilogue: accumulator element j of a lane is entry q * 4 + j, column r of its tile;
  // the entry's sum of squares sits in the lanes with (l & 15) == entry after the fold over q
#pragma unroll
  for (int mt = 0; mt < MTW; ++mt)
    if (mt < live) {
      if constexpr (NORM) {
        ss[mt] += __shfl_xor(ss[mt], 16, 64);
        ss[mt] += __shfl_xor(ss[mt], 32, 64);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int i = (mt * 4 + wr) * 16 + q * 4 + j;  // list entry
        float s = 1.f;
        if constexpr (NORM) s = rsqrtf(__shfl(ss[mt], q * 4 + j, 64) / (float)K + eps);
        if constexpr (EPI == EPI_STORE) s = l_w[i];
        if (i < n) {
          bf16* o = out + (size_t)l_slot[i] * ldo + r;
#pragma unroll
          for (int c = 0; c < NGO; ++c) {
            const int g = go0 + c;
            if (g < gout) {
              if constexpr (EPI == EPI_SILU)
                o[g * 16] = f2bf(silu(acc[c * 2][mt][j] * s) * (acc[c * 2 + 1][mt][j] * s));
              else
                o[g * 16] = f2bf(acc[c][mt][j] * s);
            }
          }
        }
      }
    }
}

// ------------------------------------------------------------------ launch ladder
struct GpPlan {
  int bm, bn, gout, up_off, tiles_m, tiles_n;
};

struct GpCall {
  const void *codes, *scales, *X;
  int ldx, K, n_experts;
  void* out;
  int ldo;
  float eps;
  GpLists ml;
  hipStream_t st;
};

// Shape checks and the tile (code = BM / 64 | BN / 64 << 4; 0 = the default of this shape).
// False = not served.
bool gp_plan(int max_rows, int K, int N, int epi, int norm, int code, GpPlan* pl) {
  if (max_rows <= 64 || K <= 0 || (K % 128) != 0 || N <= 0 || (N % 16) != 0) return false;
  // the two epilogues of the MoE layer, each with its own norm setting
  if (!((epi == EPI_SILU && norm) || (epi == EPI_STORE && !norm))) return false;
  const int nb = epi == EPI_SILU ? 2 : 1;
  if (N % (16 * nb)) return false;
  pl->gout = N / (16 * nb);
  pl->up_off = nb == 2 ? pl->gout : 0;
  if (code) {
    if (code < 0 || (code >> 8)) return false;
    pl->bm = (code & 0xf) * 64, pl->bn = (code >> 4) * 64;
    if (!gp_tile_ok(pl->bm, pl->bn)) return false;
  } else {
    // default tile by (max_rows = tokens, weight columns), from
    // profiles/mx4_moe_prefill_gemm.jsonl (bench/mx4_moe_prefill_bench.py: Mixtral-8x7B w13 and
    // w2, 96 .. 1024 tokens x top-2 over 8 experts, so about max_rows / 4 entries per expert;
    // the fastest tile or within 10 % of it at every record).  The kernel is latency-bound at
    // these fills (one m-tile per wave), so the small tile, two workgroups per CU, wins nearly
    // everywhere; 193 .. 256 tokens are the exception: there four 64-row tiles per expert of
    // which the first is full and the second holds a few entries ran 1.7x slower than one
    // 256-row tile.
    //   w13 widths (N >= 16384): 64x128, 256x128 at 193 .. 256
    //   narrower (w2): 128x64 up to 128 rows, 64x64 up to 192, 256x128 up to 256, then 64x128
    if (max_rows > 192 && max_rows <= 256) pl->bm = 256, pl->bn = 128;
    else if (N >= 16384 || max_rows > 256) pl->bm = 64, pl->bn = 128;
    else if (max_rows <= 128) pl->bm = 128, pl->bn = 64;
    else pl->bm = 64, pl->bn = 64;
  }
  pl->tiles_m = (max_rows + pl->bm - 1) / pl->bm;
  const int gt = GP_WC * (pl->bn / 32 / nb);  // output groups per tile
  pl->tiles_n = (pl->gout + gt - 1) / gt;
  return true;
}

template <int BM, int BN, int EPI>
int gp_launch(const GpPlan& pl, const GpCall& c) {
  hipLaunchKernelGGL((mx4_moe_prefill_kernel<BM, BN, EPI>),
                     dim3(pl.tiles_m * pl.tiles_n * c.n_experts), dim3(GP_THREADS), 0, c.st,
                     (const u32x4*)c.codes, (const unsigned*)c.scales, (const bf16*)c.X, c.ldx, c.K,
                     pl.gout, pl.up_off, pl.tiles_m, c.n_experts, (bf16*)c.out, c.ldo, c.eps, c.ml);
  return (int)hipGetLastError();
}

template <int EPI>
int gp_launch_t(const GpPlan& pl, const GpCall& c) {
  switch (pl.bm + pl.bn / 64) {
    case 64 + 1: return gp_launch<64, 64, EPI>(pl, c);
    case 64 + 2: return gp_launch<64, 128, EPI>(pl, c);
    case 128 + 1: return gp_launch<128, 64, EPI>(pl, c);
    case 128 + 2: return gp_launch<128, 128, EPI>(pl, c);
    case 256 + 1: return gp_launch<256, 64, EPI>(pl, c);
    case 256 + 2: return gp_launch<256, 128, EPI>(pl, c);
  }
  return (int)hipErrorInvalidValue;
}

}  // namespace

// 1 if p2p_mx4_grouped_prefill_gemm serves this shape with this tile code (0 = default)
P2P_API int p2p_mx4_grouped_prefill_ok(int max_rows, int K, int N, int epi, int norm, int code) {
  GpPlan pl;
  return gp_plan(max_rows, K, N, epi, norm, code, &pl) ? 1 : 0;
}

// As p2p_mx4_grouped_gemm (mx4_moe_gemm.hip) for max_rows > 64, one workgroup per BM x BN tile
// of an expert's list.  code: BM / 64 | BN / 64 << 4, 0 = default.  hipErrorInvalidValue for
// anything not served; nothing is launched then.
P2P_API int p2p_mx4_grouped_prefill_gemm(const void* codes, const void* scales,
                                         long long expert_stride_codes,
                                         long long expert_stride_scales, int n_experts,
                                         const int* cnt, const int* rows, int rows_stride,
                                         int x_div, const float* row_w, const void* X, int ldx,
                                         int max_rows, int K, int N, int epi, int norm, void* out,
                                         int ldo, float eps, int code, hipStream_t stream) {
  GpPlan pl;
  if (!codes || !scales || !cnt || !rows || !X || !out) return (int)hipErrorInvalidValue;
  if (n_experts <= 0 || n_experts > 65535 || rows_stride < max_rows || x_div < 0)
    return (int)hipErrorInvalidValue;
  if (expert_stride_codes < 0 || expert_stride_codes % 16 || expert_stride_scales < 0 ||
      expert_stride_scales % 4)
    return (int)hipErrorInvalidValue;
  if (!gp_plan(max_rows, K, N, epi, norm, code, &pl)) return (int)hipErrorInvalidValue;
  if ((long long)pl.tiles_m * pl.tiles_n * n_experts > 0x7fffffffLL) return (int)hipErrorInvalidValue;
  // 16-byte row chunks
  if (ldx < K || (ldx % 8) != 0 || ((uintptr_t)X & 15) != 0) return (int)hipErrorInvalidValue;
  const GpCall c = {codes, scales, X, ldx, K, n_experts, out, ldo, eps,
                    {cnt, rows, epi == EPI_STORE ? row_w : nullptr, rows_stride,
                     x_div > 0 ? x_div : 1, max_rows, expert_stride_codes / 16,
                     expert_stride_scales / 4},
                    stream};
  return epi == EPI_SILU ? gp_launch_t<EPI_SILU>(pl, c) : gp_launch_t<EPI_STORE>(pl, c);
}
