// FP8 weight-only prefill GEMM (M > 64): one launch per projection where the skinny kernel's
// F8 path (skinny_gemm_impl.h, M <= 64) needs one launch -- and one pass over the weights --
// per 64 rows.
//
//   out[m, n] = epilogue( rstd[m] * wscale[n] * sum_k X[m, k] * e4m3(code[n, k]) )
//
// It reads the Fp8Weight planes unchanged (ops.gemm.Fp8Weight, pair_f8): codes u32x4
// [G][K / 64][64], G = N / 16 column groups in the B-fragment order of
// v_mfma_f32_16x16x32_bf16 with k-steps interleaved in pairs (a lane's 16-byte word of pair
// pp holds its 8 codes of k-step 2 pp, then of k-step 2 pp + 1), and scales fp32 [N].
//
// Work split.  One workgroup of 8 waves per BM x BN tile over the whole K (no split-K, no
// atomics, no cross-workgroup waits: bit-identical from run to run), BM in {64, 128, 256},
// BN in {64, 128}.  BN counts WEIGHT columns: SwiGLU pairs a gate group with the up group
// up_off further on, so a tile stores BN / 2 output columns there and BN elsewhere.  Row
// tiles of one column tile run back to back on blockIdx.x, so concurrent workgroups share
// weight words in L2.
//
// Wave grid: 2 rows x 4 columns (the MXFP4 kernel runs 4 x 2).  Wave (wr, wc) owns the
// MTW = BM / 32 m-tiles wr * MTW .. and the NW = BN / 64 weight streams wc * NW ..  Chosen
// from this arithmetic, per 128-wide K stage; the 4 x 2 grid was not built and the two
// are not measured against each other:
//   registers  an FP8 stream holds two 16-byte words per lane and stage where MXFP4 holds
//              one, double-buffered: 16 VGPRs per stream.  At 256 x 128 the 4 x 2 grid has
//              four streams per wave = 64 VGPRs where the MXFP4 kernel, at 248 of 256 there,
//              has 40: it cannot fit.  2 x 4 has two streams = 32; the accumulators (64) and
//              the staging registers (32) are the same in both grids.
//   weights    every wave row re-reads the tile's BN x 128 bytes out of L1 / L2: 2 reads
//              instead of 4, at twice MXFP4's bytes per MFMA.
//   converts   one widened fragment (four v_cvt_scalef32_pk_bf16_fp8) serves the wave's MTW
//              m-tiles: 4 / MTW converts per MFMA, 2 .. 0.5 instead of 4 .. 1.
//   LDS reads  the price: an A fragment is read by 4 waves instead of 2, one 1 KiB
//              ds_read_b128 per NW MFMAs and wave; and with NORM the sums of squares run on
//              4 waves instead of 2 (four v_dot2 per fragment).
// SwiGLU at BN = 64 is the exception: a wave needs the gate and the up stream of its group,
// so those instantiations run 4 x 2 (MTW = BM / 64, NW = 2; 32 VGPRs of weights).
//
// Weights never touch LDS.  Per stage a wave loads two 16-byte words per lane and stream
// (two pairs = four k-steps), widens each half in registers (widen_fp8, exact: e4m3 is a
// subset of bf16) and feeds the MFMA; no in-loop scales.  The codes of stage p + 1 are loaded
// before the MFMAs of p (plain loads: the other row tiles read the same words out of L2).
//
// Activations go through LDS, double-buffered by stage: As[2][BM][128 + 8] bf16, 2 x BM x
// 272 B = 34, 68, 136 KiB of 160.  Thread t loads 16-byte chunk (t & 15) of rows (t >> 4) +
// 32 i, i < BM / 32, of stage p + 1 into registers before the MFMAs of p and writes them to
// the other buffer after them; one barrier per stage.  Rows >= M read row M - 1 and are
// never stored.  Rows are padded to 68 dwords, so the A-fragment ds_read_b128 and the
// staging ds_write_b128 are conflict-free (derivation in mx4_prefill_gemm.hip; the lane
// pattern is the same here).  A fragments are read in groups of up to four m-tiles, the next
// group while this one multiplies, with a scheduling fence per group.
//
// Epilogue: wscale[16 g + r] on the fp32 accumulators first, then rstd, then residual /
// SwiGLU / fp32 store / RoPE + KV write (gemm_epilogue.h), m-tile by m-tile.  NORM: in-loop
// sums of squares over the A fragments the wave reads anyway (sumsq8); nothing crosses waves.
// EPI_QKV_ROPE: the rows' slots and positions are fetched before the k loop up to four
// m-tiles per wave, per m-tile in the epilogue at eight (64 live registers otherwise).
//
// Plain C++ and builtins only.  Zero scratch (_build.NO_SCRATCH); VGPRs reached per
// instantiation: the table at pf_tile_ok.
#include "gemm_epilogue.h"

namespace {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

constexpr int PF_THREADS = 512;
constexpr int PF_LDA = 128 + 8;  // bf16 per LDS row

// The tile ladder.  VGPRs reached (kernel-resource-usage remarks of the build; no scratch,
// 256 available at 8 waves per workgroup), NORM on:
//   BM x BN      store / resid / f32    silu    qkv_rope
//    64 x  64     65                     80      90
//    64 x 128     95                     95     120
//   128 x  64    103                    107     152
//   128 x 128    141                    141     190
//   256 x  64    147                    165     147 (the rows' slots and positions are
//   256 x 128    201                    201     201  fetched per m-tile in the epilogue here)
// Without NORM 2 .. 19 fewer.
constexpr bool pf_tile_ok(int bm, int bn) {
  return (bm == 64 || bm == 128 || bm == 256) && (bn == 64 || bn == 128);
}

// wave columns: 4, but 2 where SwiGLU needs two streams per wave in a 64-column tile
constexpr int pf_wc(int bn, int nb) { return (nb == 2 && bn == 64) ? 2 : 4; }

// 8 e4m3 codes (half h of a pair word) -> 8 bf16: four v_cvt_scalef32_pk_bf16_fp8 (as widen
// in skinny_gemm_impl.h)
__device__ __forceinline__ bf16x8 widen_fp8(const u32x4& p, int h) {
  const unsigned lo = h ? p.z : p.x, hi = h ? p.w : p.y;
  const bf16x2 a = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(lo, 1.0f, false);
  const bf16x2 b = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(lo, 1.0f, true);
  const bf16x2 c = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(hi, 1.0f, false);
  const bf16x2 d = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(hi, 1.0f, true);
  bf16x8 r;
  r[0] = a.x; r[1] = a.y; r[2] = b.x; r[3] = b.y;
  r[4] = c.x; r[5] = c.y; r[6] = d.x; r[7] = d.y;
  return r;
}

template <int BM, int BN, int EPI, bool NORM>
__global__ __launch_bounds__(PF_THREADS) void fp8_prefill_kernel(
    const u32x4* __restrict__ codes, const bf16* __restrict__ X, int ldx, int M, int K, int gout,
    int up_off, int tiles_m, void* __restrict__ out, int ldo, float eps, EpiArgs ea) {
  constexpr int NB = (EPI == EPI_SILU) ? 2 : 1;
  constexpr int WC = pf_wc(BN, NB);      // wave columns
  constexpr int WR = 8 / WC;             // wave rows
  constexpr int MTW = BM / (16 * WR);    // m-tiles per wave
  constexpr int NW = BN / (16 * WC);     // weight streams per wave
  constexpr int NGO = NW / NB;           // output column groups per wave
  constexpr int AG = MTW < 4 ? MTW : 4;  // m-tiles per A-fragment group
  constexpr int NGR = MTW / AG;          // groups per k-step
  constexpr int LPT = BM / 32;           // 16-byte staging chunks per thread and stage
  __shared__ __attribute__((aligned(16))) bf16 As[2][BM * PF_LDA];

  const int P = K >> 7;  // stages; a group holds 2 P pair words per lane
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);  // wave-uniform
  const int wr = w / WC, wc = w % WC;
  const int r = lane & 15, q = lane >> 4;
  const int tm = blockIdx.x % tiles_m, tn = blockIdx.x / tiles_m;  // row tiles of one column
  const int m0 = tm * BM;                                           // tile run back to back
  const int go0 = (tn * WC + wc) * NGO;  // the wave's first output group

  // weight streams: b = c * NB + h (h = 1: the up half).  A group past the last one (N not a
  // multiple of the tile) streams group 0 and is never stored.
  const u32x4* cb[NW];
  int gs[NW];
#pragma unroll
  for (int c = 0; c < NGO; ++c)
#pragma unroll
    for (int h = 0; h < NB; ++h) {
      const int go = go0 + c;
      gs[c * NB + h] = (go < gout ? go : 0) + h * up_off;
      cb[c * NB + h] = codes + (size_t)gs[c * NB + h] * P * 128 + lane;
    }

  // staging: chunk (tid & 15) of rows (tid >> 4) + 32 i
  const bf16* xs[LPT];
#pragma unroll
  for (int i = 0; i < LPT; ++i) {
    const int row = (tid >> 4) + 32 * i;
    const int m = m0 + row < M ? m0 + row : M - 1;
    xs[i] = X + (size_t)m * ldx + 8 * (tid & 15);
  }
  const int sd0 = (tid >> 4) * PF_LDA + 8 * (tid & 15);  // + 32 i rows

  // EPI_QKV_ROPE: the rows' KV slots and positions
  constexpr bool kEarly = MTW <= 4;
  constexpr int NE = (EPI == EPI_QKV_ROPE && kEarly) ? MTW : 1;
  int rslot[NE][4], rpos[NE][4];
  auto load_rows = [&](int mt, int* slot, int* pos) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int m = m0 + (wr * MTW + mt) * 16 + q * 4 + j;
      slot[j] = m < M ? ea.slots[m] : -1;
      pos[j] = m < M ? ea.pos[m] : 0;
    }
  };
  if constexpr (EPI == EPI_QKV_ROPE && kEarly) {
#pragma unroll
    for (int mt = 0; mt < MTW; ++mt) load_rows(mt, rslot[mt], rpos[mt]);
  }

  f32x4 acc[NW][MTW];
  float ss[MTW];
#pragma unroll
  for (int b = 0; b < NW; ++b)
#pragma unroll
    for (int mt = 0; mt < MTW; ++mt) acc[b][mt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int mt = 0; mt < MTW; ++mt) ss[mt] = 0.f;

  u32x4 cw[NW][2], cwn[NW][2];
  bf16x8 st[LPT];
#pragma unroll
  for (int b = 0; b < NW; ++b) {
    cw[b][0] = cb[b][0];
    cw[b][1] = cb[b][64];
  }
#pragma unroll
  for (int i = 0; i < LPT; ++i) st[i] = *reinterpret_cast<const bf16x8*>(xs[i]);
#pragma unroll
  for (int i = 0; i < LPT; ++i)
    *reinterpret_cast<bf16x8*>(&As[0][sd0 + 32 * i * PF_LDA]) = st[i];
  __syncthreads();

  const int arow = (wr * MTW * 16 + r) * PF_LDA + 8 * q;  // the lane's A fragment, m-tile 0
  for (int p = 0; p < P; ++p) {
    // the next stage's activations and codes, in flight during this stage's MFMAs.  The last
    // stage reloads itself (and stores into the idle buffer) rather than branch: one basic
    // block per stage keeps the sums of squares next to their MFMAs -- behind a branch the
    // compiler sinks them below it and every A fragment of the stage stays live until then
    const size_t pn = p + 1 < P ? p + 1 : p;
#pragma unroll
    for (int i = 0; i < LPT; ++i) st[i] = *reinterpret_cast<const bf16x8*>(xs[i] + pn * 128);
#pragma unroll
    for (int b = 0; b < NW; ++b) {
      cwn[b][0] = cb[b][pn * 128];
      cwn[b][1] = cb[b][pn * 128 + 64];
    }
    const bf16* ab = &As[p & 1][arow];
    // A fragments in groups of AG m-tiles, the next group read while this one multiplies
    // (a scheduling fence per group: left alone the compiler hoists a stage's 4 MTW
    // ds_read_b128 to its top, 128 VGPRs at eight m-tiles)
    bf16x8 a[2][AG], bw[NW];
    auto read_a = [&](int s, bf16x8* dst) {
#pragma unroll
      for (int i = 0; i < AG; ++i)
        dst[i] = *reinterpret_cast<const bf16x8*>(ab + ((s % NGR) * AG + i) * 16 * PF_LDA +
                                                  (s / NGR) * 32);
    };
    read_a(0, a[0]);
#pragma unroll
    for (int s = 0; s < 4 * NGR; ++s) {
      const int h = s / NGR;
      if (s + 1 < 4 * NGR) read_a(s + 1, a[(s + 1) & 1]);
      if (s % NGR == 0) {
#pragma unroll
        for (int b = 0; b < NW; ++b) bw[b] = widen_fp8(cw[b][h >> 1], h & 1);
      }
#pragma unroll
      for (int i = 0; i < AG; ++i) {
        const int mt = (s % NGR) * AG + i;
#pragma unroll
        for (int b = 0; b < NW; ++b)
          acc[b][mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[s & 1][i], bw[b], acc[b][mt], 0, 0, 0);
        if constexpr (NORM) ss[mt] = sumsq8(a[s & 1][i], ss[mt]);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int i = 0; i < LPT; ++i)
      *reinterpret_cast<bf16x8*>(&As[(p + 1) & 1][sd0 + 32 * i * PF_LDA]) = st[i];
#pragma unroll
    for (int b = 0; b < NW; ++b) {
      cw[b][0] = cwn[b][0];
      cw[b][1] = cwn[b][1];
    }
    __syncthreads();
  }

  // ---- epilogue: accumulator element j of a lane is row q * 4 + j, column r of its tile;
  // the row's sum of squares sits in the lanes with (l & 15) == row after the fold over q
  float ws[NW];  // per-output-channel weight scales of the wave's streams
#pragma unroll
  for (int b = 0; b < NW; ++b) ws[b] = ea.wscale[(size_t)gs[b] * 16 + r];
#pragma unroll
  for (int mt = 0; mt < MTW; ++mt) {
    float rstd[4];
    if constexpr (NORM) {
      ss[mt] += __shfl_xor(ss[mt], 16, 64);
      ss[mt] += __shfl_xor(ss[mt], 32, 64);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      rstd[j] = 1.f;
      if constexpr (NORM) rstd[j] = rsqrtf(__shfl(ss[mt], q * 4 + j, 64) / (float)K + eps);
    }
    int slot[4] = {-1, -1, -1, -1}, pos[4] = {0, 0, 0, 0};
    if constexpr (EPI == EPI_QKV_ROPE) {
      if constexpr (kEarly) {
#pragma unroll
        for (int j = 0; j < 4; ++j) slot[j] = rslot[mt][j], pos[j] = rpos[mt][j];
      } else {
        load_rows(mt, slot, pos);
      }
    }
#pragma unroll
    for (int c = 0; c < NGO; ++c) {
      const int g = go0 + c;
      const bool gok = g < gout;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int m = m0 + (wr * MTW + mt) * 16 + q * 4 + j;
        const float v = acc[c * NB][mt][j] * ws[c * NB] * rstd[j];
        if constexpr (EPI == EPI_QKV_ROPE) {
          const int kk = g & 7;
          const int dd = ((r < 8) ? 8 * kk + r : 64 + 8 * kk + (r - 8)) & 63;
          float2 cs = float2{1.f, 0.f};
          if (gok && m < M) cs = ea.cs[(size_t)pos[j] * 64 + dd];
          epi_store<EPI>(m, gok && m < M, g, r, v, 0.f, out, ldo, ea, cs, slot[j]);
        } else {
          const float u = acc[c * NB + NB - 1][mt][j] * ws[c * NB + NB - 1] * rstd[j];
          epi_store<EPI>(m, gok && m < M, g, r, v, u, out, ldo, ea);
        }
      }
    }
  }
}

// ------------------------------------------------------------------ launch ladder
struct PfPlan {
  int bm, bn, gout, up_off, tiles_m, tiles_n;
};

struct PfCall {
  const void *codes, *X;
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
    // default tile by (rows, weight columns, norm), from profiles/fp8_prefill_gemm.jsonl (8B
    // and 70B projections, 96..1024 rows; the fastest tile or within 10 % of it at every
    // record but 70B down at 192 rows, 11.5 %):
    //   gate_up widths (N >= 16384): 128x128, but 64x128 at 129..192 rows (half of a second
    //     128-row tile would idle);
    //   narrower: 64x64 up to 128 rows (512 at N <= 4096: the small tile wins until its grid
    //     is several rounds deep), 64x128 up to 512, then 128x128 -- with NORM 64x128 (the qkv
    //     records; supposed, not measured: a taller wave's sums of squares cost more than
    //     the converts it saves)
    if (N >= 16384) {
      pl->bm = (M > 128 && M <= 192) ? 64 : 128, pl->bn = 128;
    } else if (M <= (N <= 4096 ? 512 : 128)) {
      pl->bm = 64, pl->bn = 64;
    } else {
      pl->bm = (M <= 512 || norm) ? 64 : 128, pl->bn = 128;
    }
  }
  pl->tiles_m = (M + pl->bm - 1) / pl->bm;
  const int gt = pl->bn / (16 * nb);  // output groups per tile
  pl->tiles_n = (pl->gout + gt - 1) / gt;
  return true;
}

template <int BM, int BN, int EPI, bool NORM>
int pf_launch(const PfPlan& pl, const PfCall& c) {
  hipLaunchKernelGGL((fp8_prefill_kernel<BM, BN, EPI, NORM>), dim3(pl.tiles_m * pl.tiles_n),
                     dim3(PF_THREADS), 0, c.st, (const u32x4*)c.codes, (const bf16*)c.X, c.ldx, c.M,
                     c.K, pl.gout, pl.up_off, pl.tiles_m, c.out, c.ldo, c.eps, *c.ea);
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

int pf_dispatch(const void* codes, const void* X, int ldx, int M, int K, int N, int epi, int norm,
                void* out, int ldo, float eps, int code, const EpiArgs& ea, hipStream_t st) {
  PfPlan pl;
  if (!codes || !ea.wscale || !X || !pf_plan(M, K, N, epi, norm, code, &pl))
    return (int)hipErrorInvalidValue;
  // 16-byte row chunks
  if (ldx < K || (ldx % 8) != 0 || ((uintptr_t)X & 15) != 0) return (int)hipErrorInvalidValue;
  const PfCall c = {codes, X, ldx, M, K, out, ldo, eps, &ea, st};
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

// 1 if p2p_fp8_prefill_gemm / p2p_fp8_prefill_gemm_qkv_rope serve this shape with this tile
// code (0 = default)
P2P_API int p2p_fp8_prefill_ok(int M, int K, int N, int epi, int norm, int code) {
  PfPlan pl;
  return pf_plan(M, K, N, epi, norm, code, &pl) ? 1 : 0;
}

// As p2p_skinny_gemm with FP8 weights for M > 64 rows in one launch.  code: BM / 64 |
// BN / 64 << 4, 0 = default.  hipErrorInvalidValue for anything not served; nothing is
// launched then.
P2P_API int p2p_fp8_prefill_gemm(const void* codes, const void* wscale, const void* X, int ldx,
                                 int M, int K, int N, int epi, int norm, void* out, int ldo,
                                 float eps, int code, hipStream_t stream) {
  if (epi == EPI_QKV_ROPE || !out) return (int)hipErrorInvalidValue;
  EpiArgs ea = {};
  ea.wscale = (const float*)wscale;
  return pf_dispatch(codes, X, ldx, M, K, N, epi, norm, out, ldo, eps, code, ea, stream);
}

// Fused qkv projection (rows in ops.gemm.rope_row_perm order) + RoPE + KV-cache write.
P2P_API int p2p_fp8_prefill_gemm_qkv_rope(const void* codes, const void* wscale, const void* X,
                                          int ldx, int M, int K, int Hq, int Hkv, const int* pos,
                                          const int* slots, const void* cos_sin, void* q_out,
                                          int ldq, void* k_cache, void* v_cache, float eps,
                                          int code, hipStream_t stream) {
  if (Hq <= 0 || Hkv <= 0 || !pos || !slots || !cos_sin || !q_out || !k_cache || !v_cache)
    return (int)hipErrorInvalidValue;
  EpiArgs ea = {};
  ea.wscale = (const float*)wscale;
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
  return pf_dispatch(codes, X, ldx, M, K, N, EPI_QKV_ROPE, 1, nullptr, 0, eps, code, ea, stream);
}
