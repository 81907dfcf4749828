// MXFP4 weight-only grouped (per-expert) GEMM for the MoE expert FFNs: the grouped
// counterpart of mx4_gemm.hip, with the contract of p2p_grouped_gemm (skinny_gemm.hip).
//
//   for every local expert e, i < min(cnt[e], max_rows), slot = rows[e * rows_stride + i]:
//     out[slot] = epi( rstd(X[slot / x_div]) * X[slot / x_div] @ W_e^T )
//   EPI_SILU  (norm = 1): silu(gate) * up, gate / up = column groups g and g + N / 32
//   EPI_STORE (norm = 0): times row_w[slot] when row_w != null
//
// Weights: the two Mx4Weight planes of mx4_gemm.hip with a leading expert dimension,
// codes u32 [E][G][P][64][4] and scales u32 [E][G][P][16] (G = N / 16, P = K / 128), widened
// by widen_fp4: the MFMA multiplies exactly Mx4Weight.dequantize_f32().
//
// Work split.  Grid = (64-row windows, column-group blocks, experts), the window fastest.
// A block first reads cnt[e] (one scalar load): with n = min(cnt[e], max_rows) - 64 * window
// <= 0 it returns before it touches a weight, so at batch 1 six of Mixtral's eight experts
// cost a scalar load per block.  Otherwise the block is the dense kernel's: K split over its
// waves by super-step range, weights + scales loaded in batches of U super-steps, the
// activation fragments in a 4-k-step ring refilled one super-step ahead, every A fragment
// shared by NG column groups (x2 for SwiGLU), the partial sums reduced through an LDS slab
// by wave 0, which runs the epilogue.  No atomics: a launch is bit-identical from run to run,
// needs no host knowledge of cnt and can be captured into a graph.
//
// More than 64 rows per expert.  Window z serves list entries [64 z, 64 z + 64) and streams
// the block's weights again.  The windows of one (expert, column block) have consecutive
// block ids, so they are dispatched back to back and the repeats can hit L2; for that the
// codes are loaded non-temporally only by single-window launches.
//
// Live m-tiles.  The host knows max_rows only and picks MT (1, 2 or 4 16-row tiles); the
// block knows n.  live = min(MT, ceil(n / 16)) is wave-uniform and selects one of MT copies
// of the stream loop, compiled for exactly that many tiles: a tile wholly past n costs no A
// load, no MFMA, no slab traffic and no branch inside the loop (32 decode rows x top-2 over
// 8 experts: 8 rows per expert on average under max_rows = 32).
//
// Gather / scatter.  Lane l owns list entry 16 mt + (l & 15) of each tile: its slot, its A
// row pointer (X + (slot / x_div) * ldx) and row_w[slot] are loaded once before the stream
// (entries past n read the window's first entry: an MFMA output row depends on its own A row
// only, and those rows are never stored).  The epilogue's rows 16 mt + 4 (l >> 4) + j take
// slot and weight from the owning lane by a shuffle, so it waits for no dependent load.
//
// Registers reached per instantiation (kernel-resource-usage remarks): the table at
// mx4_moe_fits.  The unit is built with zero scratch (_build.NO_SCRATCH).
#include <type_traits>

#include "gemm_epilogue.h"
#include "mx4_common.h"  // u32x4, widen_fp4

namespace {

// The launch ladder: which (MT, WAVES, U, NG) exist (nb = 2 for SwiGLU).  The dense kernel's
// estimate plus 3 registers per m-tile (slot, row weight, one more address): accumulators
// 4 NW MT + A ring 16 MT + weights 5 U NW + gather 3 MT + ~48; 8 waves get 128, fewer 200.
//
// Reached (VGPRs + AGPRs; EPI_STORE, 4 waves; 8 waves: MT 1 U 4 NG 1 = 62, MT 2 U 4 NG 1 = 90;
// the largest of the unit is EPI_SILU MT 4 U 4 NG 1 at 4 waves, 190 + 36):
//            U1 NG1   U4 NG1   U4 NG2   U4 NG4   U8 NG1   U8 NG2
//   MT = 1   38 + 4   58 + 4   96 + 8   164 + 16 98 + 4   176 + 8
//   MT = 2   62 + 8   82 + 8   118 + 16 186 + 32 122 + 8  198 + 16
//   MT = 4   104 + 16 120 + 16 158 + 32 refused  160 + 16 refused
constexpr bool mx4_moe_fits(int mt, int nb, int waves, int u, int ng) {
  const int nw = ng * nb;
  if (!(mt == 1 || mt == 2 || mt == 4) || !(waves == 1 || waves == 2 || waves == 4 || waves == 8))
    return false;
  if (!((u == 1 && ng == 1) || (u == 4 && (ng == 1 || ng == 2 || ng == 4)) ||
        (u == 8 && (ng == 1 || ng == 2))))
    return false;
  if (nw * mt > 16) return false;                // 64 accumulator VGPRs at most
  if ((waves - 1) * nw * mt > 56) return false;  // split-K slab, KiB
  return 4 * nw * mt + 19 * mt + 5 * u * nw + 48 <= (waves == 8 ? 128 : 200);
}

struct MoeLists {
  const int* cnt;    // [E] rows routed to each local expert
  const int* rows;   // [E][rows_stride] their slots
  const float* row_w;  // [slots] or null
  int rows_stride, x_div, max_rows;
  long long stride_codes, stride_scales;  // per expert, in u32x4 / u32
};

template <int L>
using tiles_c = std::integral_constant<int, L>;

template <int MT, int WAVES, int EPI, int U, int NG>
__global__ __launch_bounds__(WAVES * 64) void mx4_moe_gemm_kernel(
    const u32x4* __restrict__ codes, const unsigned* __restrict__ scales,
    const bf16* __restrict__ X, int ldx, int K, int up_group_offset, bf16* __restrict__ out,
    int ldo, float eps, MoeLists ml) {
  constexpr bool NORM = EPI == EPI_SILU;
  constexpr int NB = NORM ? 2 : 1;
  constexpr int NW = NG * NB;  // weight streams per wave
  const int e = blockIdx.z;
  const int c_all = min(ml.cnt[e], ml.max_rows);
  const int n = c_all - 64 * (int)blockIdx.x;  // list entries of this window
  if (n <= 0) return;                          // whole block: before any barrier
  const int live = min(MT, (n + 15) >> 4);     // block-uniform

  const int P = K >> 7;  // super-steps of 4 k-steps
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // wave-uniform
  const int g0 = blockIdx.y * NG;
  const int p0 = (P * w) / WAVES;
  const int p1 = (P * (w + 1)) / WAVES;
  const int r = lane & 15, q = lane >> 4;
  const bool nt = gridDim.x == 1;  // one window: every weight byte is read once

  const u32x4* cb[NW];  // wave-uniform stream bases
  const unsigned* sb[NW];
#pragma unroll
  for (int c = 0; c < NG; ++c)
#pragma unroll
    for (int h = 0; h < NB; ++h) {
      const size_t g = (size_t)(g0 + c + h * up_group_offset);
      cb[c * NB + h] = codes + (size_t)e * ml.stride_codes + g * P * 64;
      sb[c * NB + h] = scales + (size_t)e * ml.stride_scales + g * P * 16;
    }

  // ---- gather: the lane's list entry of every m-tile (slot, A row, row weight)
  const int* rl = ml.rows + (size_t)e * ml.rows_stride + 64 * blockIdx.x;
  int aslot[MT];
  float aw[MT];
  const bf16* xp[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const int i = mt * 16 + r;
    const int s = rl[i < n ? i : 0];
    aslot[mt] = s;
    aw[mt] = 1.f;
    if constexpr (EPI == EPI_STORE)
      if (ml.row_w) aw[mt] = ml.row_w[s];
    xp[mt] = X + (size_t)((unsigned)s / (unsigned)ml.x_div) * ldx + 8 * q;
  }

  f32x4 acc[NW][MT];
  float ss[MT];
#pragma unroll
  for (int b = 0; b < NW; ++b)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[b][mt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) ss[mt] = 0.f;

  // ---- the stream over this wave's super-steps, compiled for L live m-tiles
  auto stream = [&](auto tiles) {
    constexpr int L = decltype(tiles)::value;
    u32x4 cw[U][NW];
    unsigned sw[U][NW];
    bf16x8 a[4][L];  // ring: slot h = k-step 4p + h of the super-step being consumed
    auto load_a = [&](int p, int h) {
#pragma unroll
      for (int mt = 0; mt < L; ++mt)
        a[h][mt] = *reinterpret_cast<const bf16x8*>(xp[mt] + (size_t)(4 * p + h) * 32);
    };
#pragma unroll
    for (int h = 0; h < 4; ++h) load_a(p0, h);
    for (int pb = p0; pb < p1; pb += U) {
      // one batch: the code + scale loads of up to U super-steps, issued together
      if (nt) {
#pragma unroll
        for (int u = 0; u < U; ++u)
          if (pb + u < p1) {
#pragma unroll
            for (int b = 0; b < NW; ++b) {
              cw[u][b] = __builtin_nontemporal_load(cb[b] + (size_t)(pb + u) * 64 + lane);
              sw[u][b] = sb[b][(size_t)(pb + u) * 16 + r];
            }
          }
      } else {
#pragma unroll
        for (int u = 0; u < U; ++u)
          if (pb + u < p1) {
#pragma unroll
            for (int b = 0; b < NW; ++b) {
              cw[u][b] = cb[b][(size_t)(pb + u) * 64 + lane];
              sw[u][b] = sb[b][(size_t)(pb + u) * 16 + r];
            }
          }
      }
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (pb + u < p1) {
          const int p = pb + u;
#pragma unroll
          for (int h = 0; h < 4; ++h) {
            bf16x8 bw[NW];
#pragma unroll
            for (int b = 0; b < NW; ++b) bw[b] = widen_fp4(cw[u][b][h], sw[u][b], h);
#pragma unroll
            for (int mt = 0; mt < L; ++mt) {
#pragma unroll
              for (int b = 0; b < NW; ++b)
                acc[b][mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[h][mt], bw[b], acc[b][mt], 0, 0, 0);
              if constexpr (NORM) ss[mt] = sumsq8(a[h][mt], ss[mt]);
            }
            if (p + 1 < p1) load_a(p + 1, h);  // the slot's fragment one super-step ahead
          }
        }
    }
  };
  if (p0 < p1) {
    if constexpr (MT == 1) {
      stream(tiles_c<1>{});
    } else if constexpr (MT == 2) {
      if (live == 1) stream(tiles_c<1>{});
      else stream(tiles_c<2>{});
    } else {
      switch (live) {
        case 1: stream(tiles_c<1>{}); break;
        case 2: stream(tiles_c<2>{}); break;
        case 3: stream(tiles_c<3>{}); break;
        default: stream(tiles_c<4>{}); break;
      }
    }
  }

  // ---- split-K reduction across the block's waves (live tiles only) ----
  if constexpr (NORM) {
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      ss[mt] += __shfl_xor(ss[mt], 16, 64);
      ss[mt] += __shfl_xor(ss[mt], 32, 64);
    }
  }
  float rstd[MT][4];
  if constexpr (WAVES > 1) {
    __shared__ float red[WAVES - 1][NW * MT * 4][64];
    __shared__ float red_ss[WAVES][MT][16];
    if (w > 0) {
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
        if (mt < live) {
#pragma unroll
          for (int b = 0; b < NW; ++b)
#pragma unroll
            for (int j = 0; j < 4; ++j) red[w - 1][(b * MT + mt) * 4 + j][lane] = acc[b][mt][j];
        }
    }
    if constexpr (NORM) {
      if (q == 0) {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) red_ss[w][mt][r] = ss[mt];
      }
    }
    __syncthreads();
    if (w != 0) return;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
      if (mt < live) {
#pragma unroll
        for (int ww = 0; ww < WAVES - 1; ++ww)
#pragma unroll
          for (int b = 0; b < NW; ++b)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[b][mt][j] += red[ww][(b * MT + mt) * 4 + j][lane];
      }
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        rstd[mt][j] = 1.f;
        if constexpr (NORM) {
          float t = 0.f;
#pragma unroll
          for (int ww = 0; ww < WAVES; ++ww) t += red_ss[ww][mt][q * 4 + j];
          rstd[mt][j] = rsqrtf(t / (float)K + eps);
        }
      }
  } else {
    // single wave: rstd of row m lives in lane (m & 15) of the same m-tile
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        rstd[mt][j] = 1.f;
        if constexpr (NORM) {
          const float t = __shfl(ss[mt], q * 4 + j, 64);
          rstd[mt][j] = rsqrtf(t / (float)K + eps);
        }
      }
  }

  // ---- epilogue (wave 0): scatter to the slots' rows ----
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
    if (mt < live) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int m = mt * 16 + q * 4 + j;
        const int slot = __shfl(aslot[mt], q * 4 + j, 64);  // all 64 lanes
        const float s = rstd[mt][j] * __shfl(aw[mt], q * 4 + j, 64);
        if (m < n) {
          bf16* o = out + (size_t)slot * ldo + r;
#pragma unroll
          for (int c = 0; c < NG; ++c) {
            if constexpr (EPI == EPI_SILU)
              o[(g0 + c) * 16] = f2bf(silu(acc[c * 2][mt][j] * s) * (acc[c * 2 + 1][mt][j] * s));
            else
              o[(g0 + c) * 16] = f2bf(acc[c][mt][j] * s);
          }
        }
      }
    }
}

// ------------------------------------------------------------------ launch ladder
struct MoeCall {
  const void *codes, *scales, *X;
  int ldx, K, groups, up_off, windows, n_experts;
  void* out;
  int ldo;
  float eps;
  MoeLists ml;
  hipStream_t st;
};

template <int MT, int WAVES, int EPI, int U, int NG>
int moe_launch(const MoeCall& c) {
  if constexpr (!mx4_moe_fits(MT, EPI == EPI_SILU ? 2 : 1, WAVES, U, NG)) {
    return (int)hipErrorInvalidValue;
  } else {
    hipLaunchKernelGGL((mx4_moe_gemm_kernel<MT, WAVES, EPI, U, NG>),
                       dim3(c.windows, c.groups / NG, c.n_experts), dim3(WAVES * 64), 0, c.st,
                       (const u32x4*)c.codes, (const unsigned*)c.scales, (const bf16*)c.X, c.ldx,
                       c.K, c.up_off, (bf16*)c.out, c.ldo, c.eps, c.ml);
    return (int)hipGetLastError();
  }
}

template <int MT, int WAVES, int EPI>
int moe_launch_ung(int u, int ng, const MoeCall& c) {
  switch (u << 4 | ng) {
    case 1 << 4 | 1: return moe_launch<MT, WAVES, EPI, 1, 1>(c);
    case 4 << 4 | 1: return moe_launch<MT, WAVES, EPI, 4, 1>(c);
    case 4 << 4 | 2: return moe_launch<MT, WAVES, EPI, 4, 2>(c);
    case 4 << 4 | 4: return moe_launch<MT, WAVES, EPI, 4, 4>(c);
    case 8 << 4 | 1: return moe_launch<MT, WAVES, EPI, 8, 1>(c);
    case 8 << 4 | 2: return moe_launch<MT, WAVES, EPI, 8, 2>(c);
  }
  return (int)hipErrorInvalidValue;
}

template <int MT, int EPI>
int moe_launch_w(int waves, int u, int ng, const MoeCall& c) {
  switch (waves) {
    case 1: return moe_launch_ung<MT, 1, EPI>(u, ng, c);
    case 2: return moe_launch_ung<MT, 2, EPI>(u, ng, c);
    case 4: return moe_launch_ung<MT, 4, EPI>(u, ng, c);
    case 8: return moe_launch_ung<MT, 8, EPI>(u, ng, c);
  }
  return (int)hipErrorInvalidValue;
}

template <int EPI>
int moe_launch_m(int mt, int waves, int u, int ng, const MoeCall& c) {
  switch (mt) {
    case 1: return moe_launch_w<1, EPI>(waves, u, ng, c);
    case 2: return moe_launch_w<2, EPI>(waves, u, ng, c);
    case 4: return moe_launch_w<4, EPI>(waves, u, ng, c);
  }
  return (int)hipErrorInvalidValue;
}

struct MoePlan {
  int mt, groups, up_off, waves, u, ng, windows;
};

// Shape checks and the launch code (waves | U << 8 | NG << 16; 0 = the default plan).
// False = not served.
bool mx4_moe_plan(int max_rows, int K, int N, int epi, int norm, int code, MoePlan* pl) {
  if (max_rows <= 0 || K <= 0 || (K % 128) != 0 || N <= 0 || (N % 16) != 0) return false;
  // the two epilogues of the MoE layer, each with its own norm setting
  if (!((epi == EPI_SILU && norm) || (epi == EPI_STORE && !norm))) return false;
  if (code < 0 || (code >> 24)) return false;
  pl->mt = max_rows <= 16 ? 1 : (max_rows <= 32 ? 2 : 4);
  pl->windows = (max_rows + 63) / 64;
  pl->groups = N / 16;
  pl->up_off = 0;
  const int nb = epi == EPI_SILU ? 2 : 1;
  if (nb == 2) {
    if (N % 32) return false;
    pl->groups = N / 32;
    pl->up_off = pl->groups;
  }
  if (pl->groups > 65535) return false;  // grid.y
  if (code) {
    pl->waves = code & 0xff, pl->u = (code >> 8) & 0xff, pl->ng = (code >> 16) & 0xff;
    return mx4_moe_fits(pl->mt, nb, pl->waves, pl->u, pl->ng) && pl->groups % pl->ng == 0;
  }
  // default, from profiles/mx4_moe_gemm.jsonl (bench/mx4_moe_bench.py, Mixtral-8x7B w13 and
  // w2, 1 .. 1024 tokens x top-2 over 8 experts): 4-deep batches; 4 waves where that leaves
  // each two super-steps (8 waves were never best above one token: the grid is already
  // experts x groups blocks); one m-tile: two weight streams per wave (NG = 1 for SwiGLU,
  // 2 else; best or within 5 % but for w2 at one token, 20.4 us against 16.6 us of U = 8
  // over 8 waves, which is 24 % behind at 8 tokens); more m-tiles: as many column groups as
  // the ladder fits (best or within 0.5 % at every pattern of 32 tokens and more)
  const int P = K / 128;
  for (int ng = 4; ng >= 1; ng >>= 1)
    for (int waves = 4; waves >= 1; waves >>= 1) {
      if (pl->groups % ng || (waves > 1 && P / waves < 2)) continue;
      if (pl->mt == 1 && ng * nb > 2) continue;
      if (!mx4_moe_fits(pl->mt, nb, waves, 4, ng)) continue;
      pl->waves = waves, pl->u = 4, pl->ng = ng;
      return true;
    }
  return false;
}

}  // namespace

// 1 if p2p_mx4_grouped_gemm serves this shape with this launch code
P2P_API int p2p_mx4_grouped_ok(int max_rows, int K, int N, int epi, int norm, int code) {
  MoePlan pl;
  return mx4_moe_plan(max_rows, K, N, epi, norm, code, &pl) ? 1 : 0;
}

// Grouped (MoE) MXFP4 projection over the local experts, as p2p_grouped_gemm: expert e
// multiplies rows slot = rows[e * rows_stride + i] (i < min(cnt[e], max_rows)) of X (row
// slot / x_div) with its weights and writes output row slot.  codes / scales: the planes of a
// stacked ops.gemm.Mx4Weight, expert e at byte offset e * expert_stride_codes /
// e * expert_stride_scales.  epi: 0 store (norm 0; scaled by row_w[slot] if row_w) | 2
// silu(gate) * up (norm 1).  code: waves | U << 8 | NG << 16, 0 = default.
// hipErrorInvalidValue for anything else; nothing is launched then.
P2P_API int p2p_mx4_grouped_gemm(const void* codes, const void* scales,
                                 long long expert_stride_codes, long long expert_stride_scales,
                                 int n_experts, const int* cnt, const int* rows, int rows_stride,
                                 int x_div, const float* row_w, const void* X, int ldx,
                                 int max_rows, int K, int N, int epi, int norm, void* out, int ldo,
                                 float eps, int code, hipStream_t stream) {
  MoePlan pl;
  if (!codes || !scales || !cnt || !rows || !X || !out) return (int)hipErrorInvalidValue;
  if (n_experts <= 0 || n_experts > 65535 || rows_stride < max_rows || x_div < 0)
    return (int)hipErrorInvalidValue;
  if (expert_stride_codes < 0 || expert_stride_codes % 16 || expert_stride_scales < 0 ||
      expert_stride_scales % 4)
    return (int)hipErrorInvalidValue;
  if (!mx4_moe_plan(max_rows, K, N, epi, norm, code, &pl)) return (int)hipErrorInvalidValue;
  MoeCall c = {codes, scales, X, ldx, K, pl.groups, pl.up_off, pl.windows, n_experts, out, ldo, eps,
               {cnt, rows, epi == EPI_STORE ? row_w : nullptr, rows_stride, x_div > 0 ? x_div : 1,
                max_rows, expert_stride_codes / 16, expert_stride_scales / 4},
               stream};
  return epi == EPI_SILU ? moe_launch_m<EPI_SILU>(pl.mt, pl.waves, pl.u, pl.ng, c)
                         : moe_launch_m<EPI_STORE>(pl.mt, pl.waves, pl.u, pl.ng, c);
}
