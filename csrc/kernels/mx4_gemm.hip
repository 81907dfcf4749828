// MXFP4 weight-only skinny GEMM (M <= 64) for the decode / short-prefill projections.
//
//   out[m, n] = epilogue( rstd[m] * sum_k X[m, k] * (e2m1(code[n, k]) * 2^(e8m0[n, k / 32] - 127)) )
//
// OCP MX v1.0: one e8m0 scale per 32 elements along K.  A k-step of v_mfma_f32_16x16x32_bf16
// is 32 wide too, so a lane's 8 codes of one k-step share one scale, and gfx950's
// v_cvt_scalef32_pk_bf16_fp4 (two e2m1 codes -> two bf16, times a float scale) applies it
// while widening.  e2m1 times a power of two is exact in bf16: the MFMA multiplies exactly
// the values Mx4Weight.dequantize_f32() returns, in bf16 x bf16 -> fp32 like the bf16
// kernel, and nothing of the scale is left for the epilogue.
//
// Layout (ops.gemm.quantize_mxfp4; G = N / 16 column groups, P = K / 128 super-steps):
//   codes  u32 [G][P][64 lanes][4]: word h of lane l at super-step p holds the 8 codes the
//          bf16 layout gives that lane at k-step 4p + h,
//              W[16 g + (l & 15)][32 (4p + h) + 8 (l >> 4) + j],  j = nibble index (low first),
//          so one 16-byte load per lane (1 KiB per wave instruction) feeds four MFMAs.
//   scales u32 [G][P][16]: word r holds the four scale bytes of column 16 g + r for k-steps
//          4p .. 4p + 3 (byte h = k-step 4p + h); the four lanes sharing r read the same
//          word.  64 B per 1 KiB of codes: 4.25 bits per weight.
//
// Pipeline.  Vector-memory loads retire in issue order, so an activation load that is
// consumed soon after it is issued also waits for every weight load issued before it: a
// rolling weight prefetch can never be deeper than the activations' lead.  Hence
//   * weights + scales are loaded in batches of U super-steps (5 VGPRs per super-step and
//     weight stream; one wait per batch with U * NW KiB in flight per wave, where the bf16
//     kernel holds 20 VGPRs per KiB);
//   * the activation fragments run through a 4-k-step ring (16 * MT VGPRs) that is refilled
//     one super-step ahead and keeps rolling across batches (L2 hits);
//   * every A fragment is shared by NG column groups (x2 for SwiGLU's gate / up pair): the
//     weight fragment is the cheap operand here, NG = 4 brings the A : W traffic ratio back
//     to the bf16 kernel's.
// K is split over the block's waves by super-step ranges (a wave with an empty range still
// reaches the barrier) and reduced through an LDS slab by wave 0, which runs the epilogue
// (gemm_epilogue.h).  The ladder (mx4_fits) refuses what would not fit the 56 KiB slab or
// the register file; the unit is built with zero scratch (_build.NO_SCRATCH).
//
// Registers reached per instantiation (kernel-resource-usage remarks): the table at mx4_fits.
#include "gemm_epilogue.h"
#include "mx4_common.h"  // u32x4, widen_fp4

namespace {

// The launch ladder: which (MT, WAVES, U, NG) exist (nb = 2 for SwiGLU).  Estimated registers
// = accumulators 4 NW MT + A ring 16 MT + weights 5 U NW + ~48 of addresses and epilogue
// operands; 8 waves get 128 (so MT = 4 never runs 8 waves), fewer waves 200.
//
// Reached (VGPRs + AGPRs, the accumulators live in AGPRs below 8 waves; EPI_STORE, 4 waves;
// 8 waves: MT 1 U 4 NG 1 = 54, MT 2 U 8 NG 1 = 96):
//            U1 NG1   U4 NG1   U4 NG2   U4 NG4   U8 NG1   U8 NG2
//   MT = 1   36 + 4   50 + 4   82 + 8   138 + 16 70 + 4   124 + 8
//   MT = 2   54 + 12  76 + 8   92 + 24  140 + 40 96 + 8   132 + 24
//   MT = 4   96 + 26  120 + 16 134 + 40 refused  140 + 16 refused
constexpr bool mx4_fits(int mt, int nb, int waves, int u, int ng) {
  const int nw = ng * nb;
  if (!(mt == 1 || mt == 2 || mt == 4) || !(waves == 1 || waves == 2 || waves == 4 || waves == 8))
    return false;
  // (U, NG) pairs: the unpipelined baseline, 4-deep at every NG, 8-deep up to two groups
  if (!((u == 1 && ng == 1) || (u == 4 && (ng == 1 || ng == 2 || ng == 4)) ||
        (u == 8 && (ng == 1 || ng == 2))))
    return false;
  if (nw * mt > 16) return false;                // 64 accumulator VGPRs at most
  if ((waves - 1) * nw * mt > 56) return false;  // split-K slab, KiB
  return 4 * nw * mt + 16 * mt + 5 * u * nw + 48 <= (waves == 8 ? 128 : 200);
}

template <int MT, int WAVES, int EPI, bool NORM, int U, int NG>
__global__ __launch_bounds__(WAVES * 64) void mx4_gemm_kernel(
    const u32x4* __restrict__ codes, const unsigned* __restrict__ scales,
    const bf16* __restrict__ X, int ldx, int M, int K, int up_group_offset,
    void* __restrict__ out, int ldo, float eps, EpiArgs ea) {
  constexpr int NB = (EPI == EPI_SILU) ? 2 : 1;
  constexpr int NW = NG * NB;  // weight streams per wave
  const int P = K >> 7;        // super-steps of 4 k-steps
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // wave-uniform
  const int g0 = blockIdx.x * NG;
  const int p0 = (P * w) / WAVES;
  const int p1 = (P * (w + 1)) / WAVES;
  const int r = lane & 15, q = lane >> 4;

  const u32x4* cb[NW];    // wave-uniform stream bases
  const unsigned* sb[NW];
#pragma unroll
  for (int c = 0; c < NG; ++c)
#pragma unroll
    for (int h = 0; h < NB; ++h) {
      const size_t g = (size_t)(g0 + c + h * up_group_offset);
      cb[c * NB + h] = codes + g * P * 64;
      sb[c * NB + h] = scales + g * P * 16;
    }

  // rows >= M read row 0: an MFMA output row depends on its own A row only, and rows >= M
  // are never stored
  const bf16* xp[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const int row = mt * 16 + r;
    xp[mt] = X + (size_t)(row < M ? row : 0) * ldx + 8 * q;
  }

  // ---- epilogue operands, fetched before the stream by the finishing wave (0): the rows'
  // KV slots and positions always; the (cos, sin) pairs and the residual at MT = 1 (else
  // they are fetched as one batch right after the main loop and land during the reduction)
  constexpr bool kEarly = MT == 1;
  int rslot[MT][4], rpos[MT][4];
  float resv[NG][MT][4];
  float2 csv[NG][MT][4];
  if constexpr (EPI == EPI_QKV_ROPE) {
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int m = mt * 16 + q * 4 + j;
        const bool ok = m < M && w == 0;
        rslot[mt][j] = ok ? ea.slots[m] : -1;
        rpos[mt][j] = ok ? ea.pos[m] : 0;
      }
  }
  auto load_epi_operands = [&]() {
#pragma unroll
    for (int c = 0; c < NG; ++c)
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int m = mt * 16 + q * 4 + j;
          const bool ok = w == 0 && m < M;
          resv[c][mt][j] = 0.f;
          csv[c][mt][j] = float2{1.f, 0.f};
          if constexpr (EPI == EPI_RESID)
            if (ok) resv[c][mt][j] = (float)reinterpret_cast<const bf16*>(out)[(size_t)m * ldo + (g0 + c) * 16 + r];
          if constexpr (EPI == EPI_QKV_ROPE) {
            const int kk = (g0 + c) & 7;
            const int dd = ((r < 8) ? 8 * kk + r : 64 + 8 * kk + (r - 8)) & 63;
            if (ok) csv[c][mt][j] = ea.cs[(size_t)rpos[mt][j] * 64 + dd];
          }
        }
  };
  if constexpr (kEarly) load_epi_operands();

  f32x4 acc[NW][MT];
  float ss[MT];
#pragma unroll
  for (int b = 0; b < NW; ++b)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[b][mt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) ss[mt] = 0.f;

  if (p0 < p1) {
    u32x4 cw[U][NW];
    unsigned sw[U][NW];
    bf16x8 a[4][MT];  // ring: slot h = k-step 4p + h of the super-step being consumed
    auto load_a = [&](int p, int h) {
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
        a[h][mt] = *reinterpret_cast<const bf16x8*>(xp[mt] + (size_t)(4 * p + h) * 32);
    };
#pragma unroll
    for (int h = 0; h < 4; ++h) load_a(p0, h);
    for (int pb = p0; pb < p1; pb += U) {
      // one batch: the code + scale loads of up to U super-steps, issued together
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (pb + u < p1) {
#pragma unroll
          for (int b = 0; b < NW; ++b) {
            cw[u][b] = __builtin_nontemporal_load(cb[b] + (size_t)(pb + u) * 64 + lane);
            sw[u][b] = sb[b][(size_t)(pb + u) * 16 + r];
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
            for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
              for (int b = 0; b < NW; ++b)
                acc[b][mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[h][mt], bw[b], acc[b][mt], 0, 0, 0);
              if constexpr (NORM) ss[mt] = sumsq8(a[h][mt], ss[mt]);
            }
            if (p + 1 < p1) load_a(p + 1, h);  // the slot's fragment one super-step ahead
          }
        }
    }
  }

  if constexpr (!kEarly) load_epi_operands();

  // ---- split-K reduction across the block's waves ----
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
      for (int b = 0; b < NW; ++b)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
          for (int j = 0; j < 4; ++j) red[w - 1][(b * MT + mt) * 4 + j][lane] = acc[b][mt][j];
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
    for (int ww = 0; ww < WAVES - 1; ++ww)
#pragma unroll
      for (int b = 0; b < NW; ++b)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[b][mt][j] += red[ww][(b * MT + mt) * 4 + j][lane];
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

  // ---- epilogue (wave 0) ----
#pragma unroll
  for (int c = 0; c < NG; ++c) {
    const int g = g0 + c;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int m = mt * 16 + q * 4 + j;
        const float s = rstd[mt][j];
        if constexpr (EPI == EPI_QKV_ROPE) {
          epi_store<EPI>(m, m < M, g, r, acc[c][mt][j] * s, 0.f, out, ldo, ea, csv[c][mt][j],
                         rslot[mt][j]);
        } else if constexpr (EPI == EPI_RESID) {
          if (m < M)
            reinterpret_cast<bf16*>(out)[(size_t)m * ldo + g * 16 + r] =
                f2bf(resv[c][mt][j] + acc[c][mt][j] * s);
        } else {
          epi_store<EPI>(m, m < M, g, r, acc[c * NB][mt][j] * s, acc[c * NB + NB - 1][mt][j] * s,
                         out, ldo, ea);
        }
      }
  }
}

// ------------------------------------------------------------------ launch ladder
struct Mx4Call {
  const void *codes, *scales, *X;
  int ldx, M, K, groups, up_off;
  void* out;
  int ldo;
  float eps;
  const EpiArgs* ea;
  hipStream_t st;
};

template <int MT, int WAVES, int EPI, bool NORM, int U, int NG>
int mx4_launch(const Mx4Call& c) {
  if constexpr (!mx4_fits(MT, EPI == EPI_SILU ? 2 : 1, WAVES, U, NG)) {
    return (int)hipErrorInvalidValue;
  } else {
    hipLaunchKernelGGL((mx4_gemm_kernel<MT, WAVES, EPI, NORM, U, NG>), dim3(c.groups / NG),
                       dim3(WAVES * 64), 0, c.st, (const u32x4*)c.codes, (const unsigned*)c.scales,
                       (const bf16*)c.X, c.ldx, c.M, c.K, c.up_off, c.out, c.ldo, c.eps, *c.ea);
    return (int)hipGetLastError();
  }
}

template <int MT, int WAVES, int EPI, bool NORM, int U>
int mx4_launch_g(int ng, const Mx4Call& c) {
  switch (ng) {
    case 1: return mx4_launch<MT, WAVES, EPI, NORM, U, 1>(c);
    case 2: return mx4_launch<MT, WAVES, EPI, NORM, U, 2>(c);
    case 4: return mx4_launch<MT, WAVES, EPI, NORM, U, 4>(c);
  }
  return (int)hipErrorInvalidValue;
}

template <int MT, int WAVES, int EPI, bool NORM>
int mx4_launch_u(int u, int ng, const Mx4Call& c) {
  switch (u) {
    case 1: return mx4_launch_g<MT, WAVES, EPI, NORM, 1>(ng, c);
    case 4: return mx4_launch_g<MT, WAVES, EPI, NORM, 4>(ng, c);
    case 8: return mx4_launch_g<MT, WAVES, EPI, NORM, 8>(ng, c);
  }
  return (int)hipErrorInvalidValue;
}

template <int MT, int EPI, bool NORM>
int mx4_launch_w(int waves, int u, int ng, const Mx4Call& c) {
  switch (waves) {
    case 1: return mx4_launch_u<MT, 1, EPI, NORM>(u, ng, c);
    case 2: return mx4_launch_u<MT, 2, EPI, NORM>(u, ng, c);
    case 4: return mx4_launch_u<MT, 4, EPI, NORM>(u, ng, c);
    case 8: return mx4_launch_u<MT, 8, EPI, NORM>(u, ng, c);
  }
  return (int)hipErrorInvalidValue;
}

template <int EPI, bool NORM>
int mx4_launch_m(int mt, int waves, int u, int ng, const Mx4Call& c) {
  switch (mt) {
    case 1: return mx4_launch_w<1, EPI, NORM>(waves, u, ng, c);
    case 2: return mx4_launch_w<2, EPI, NORM>(waves, u, ng, c);
    case 4: return mx4_launch_w<4, EPI, NORM>(waves, u, ng, c);
  }
  return (int)hipErrorInvalidValue;
}

template <int EPI>
int mx4_launch_n(int norm, int mt, int waves, int u, int ng, const Mx4Call& c) {
  if constexpr (EPI == EPI_QKV_ROPE) {
    return norm ? mx4_launch_m<EPI, true>(mt, waves, u, ng, c) : (int)hipErrorInvalidValue;
  } else {
    return norm ? mx4_launch_m<EPI, true>(mt, waves, u, ng, c)
                : mx4_launch_m<EPI, false>(mt, waves, u, ng, c);
  }
}

struct Mx4Plan {
  int mt, groups, up_off, waves, u, ng;
};

// Shape checks and the launch code (waves | U << 8 | NG << 16; 0 = the default of this
// (MT, epilogue)).  False = not served.
bool mx4_plan(int M, int K, int N, int epi, int norm, int code, Mx4Plan* pl) {
  if (M <= 0 || M > 64 || K <= 0 || (K % 128) != 0 || N <= 0 || (N % 16) != 0) return false;
  if (!(epi == EPI_STORE || epi == EPI_RESID || epi == EPI_SILU || epi == EPI_F32 ||
        epi == EPI_QKV_ROPE))
    return false;
  if (epi == EPI_QKV_ROPE && !norm) return false;
  if (code < 0 || (code >> 24)) return false;
  pl->mt = M <= 16 ? 1 : (M <= 32 ? 2 : 4);
  pl->groups = N / 16;
  pl->up_off = 0;
  const int nb = epi == EPI_SILU ? 2 : 1;
  if (nb == 2) {
    if (N % 32) return false;
    pl->groups = N / 32;
    pl->up_off = pl->groups;
  }
  if (code) {
    pl->waves = code & 0xff, pl->u = (code >> 8) & 0xff, pl->ng = (code >> 16) & 0xff;
    return mx4_fits(pl->mt, nb, pl->waves, pl->u, pl->ng) && pl->groups % pl->ng == 0;
  }
  // default: 4-deep batches, as many column groups per wave as fit and divide the groups,
  // as many waves as leave each at least two super-steps
  const int P = K / 128;
  for (int ng = 4; ng >= 1; ng >>= 1)
    for (int waves = 8; waves >= 1; waves >>= 1) {
      if (pl->groups % ng || (waves > 1 && P / waves < 2)) continue;
      // one m-tile: two groups per wave (twice the bytes in flight) where that still leaves a
      // block per CU, i.e. from 512 groups (measured best or tied there at M = 1 and 8, and
      // 15-25 % slower at the 256-group projections; profiles/mx4_gemm.jsonl); never four
      if (pl->mt == 1 && (ng > 2 || (ng == 2 && pl->groups < 512))) continue;
      if (!mx4_fits(pl->mt, nb, waves, 4, ng)) continue;
      pl->waves = waves, pl->u = 4, pl->ng = ng;
      return true;
    }
  return false;
}

int mx4_dispatch(const void* codes, const void* scales, const void* X, int ldx, int M, int K, int N,
                 int epi, int norm, void* out, int ldo, float eps, int code, const EpiArgs& ea,
                 hipStream_t st) {
  Mx4Plan pl;
  if (!codes || !scales || !X || !mx4_plan(M, K, N, epi, norm, code, &pl)) return (int)hipErrorInvalidValue;
  const Mx4Call c = {codes, scales, X, ldx, M, K, pl.groups, pl.up_off, out, ldo, eps, &ea, st};
  switch (epi) {
    case EPI_STORE: return mx4_launch_n<EPI_STORE>(norm, pl.mt, pl.waves, pl.u, pl.ng, c);
    case EPI_RESID: return mx4_launch_n<EPI_RESID>(norm, pl.mt, pl.waves, pl.u, pl.ng, c);
    case EPI_SILU: return mx4_launch_n<EPI_SILU>(norm, pl.mt, pl.waves, pl.u, pl.ng, c);
    case EPI_F32: return mx4_launch_n<EPI_F32>(norm, pl.mt, pl.waves, pl.u, pl.ng, c);
    case EPI_QKV_ROPE: return mx4_launch_n<EPI_QKV_ROPE>(norm, pl.mt, pl.waves, pl.u, pl.ng, c);
  }
  return (int)hipErrorInvalidValue;
}

}  // namespace

// 1 if p2p_mx4_gemm / p2p_mx4_gemm_qkv_rope serve this shape with this launch code
P2P_API int p2p_mx4_gemm_ok(int M, int K, int N, int epi, int norm, int code) {
  Mx4Plan pl;
  return mx4_plan(M, K, N, epi, norm, code, &pl) ? 1 : 0;
}

// codes / scales: the two planes of an ops.gemm.Mx4Weight (layout in the header).  epi as in
// p2p_skinny_gemm (0 store, 1 residual add in place, 2 silu(gate) * up, 3 fp32 store).
// code: waves | U << 8 | NG << 16, 0 = default.  hipErrorInvalidValue for anything the
// ladder does not serve; nothing is launched then.
P2P_API int p2p_mx4_gemm(const void* codes, const void* scales, const void* X, int ldx, int M, int K,
                         int N, int epi, int norm, void* out, int ldo, float eps, int code,
                         hipStream_t stream) {
  if (epi == EPI_QKV_ROPE || !out) return (int)hipErrorInvalidValue;
  EpiArgs ea = {};
  return mx4_dispatch(codes, scales, X, ldx, M, K, N, epi, norm, out, ldo, eps, code, ea, stream);
}

// Fused qkv projection (rows in ops.gemm.rope_row_perm order) + RoPE + KV-cache write.
P2P_API int p2p_mx4_gemm_qkv_rope(const void* codes, const void* scales, const void* X, int ldx,
                                  int M, int K, int Hq, int Hkv, const int* pos, const int* slots,
                                  const void* cos_sin, void* q_out, int ldq, void* k_cache,
                                  void* v_cache, float eps, int code, hipStream_t stream) {
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
  return mx4_dispatch(codes, scales, X, ldx, M, K, N, EPI_QKV_ROPE, 1, nullptr, 0, eps, code, ea,
                      stream);
}
