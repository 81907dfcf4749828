// Causal prefill attention on MFMA over the FP8 KV cache: flash_prefill.hip v2 reading the
// e4m3 pages of kv_fp8_write.hip.
//
// Cache format, per layer, for K and for V:
//     codes  [num_pages][n_kv_heads][PAGE=64][D=128] OCP e4m3 (one page of one head: 8 KiB)
//     scales [num_pages][n_kv_heads][PAGE=64]        fp32, one per (token, kv head) row
//
// Contract and geometry are v2's (flash_prefill.hip): a workgroup = one kv head x 256/G
// consecutive tokens of one query tile, 8 waves x 32 query rows, one 64-key page per step,
// v_mfma_f32_32x32x16_bf16 for both products, the S^T accumulator registers are the P^T
// operand (K rows staged through kperm), heaviest tiles first through xcd_remap, deferred
// rescale of O and l.
//
// Numerics are kv_fp8_attention.hip's, so a sequence prefilled here and decoded there sees
// the same math up to bf16 rounding.  The codes widen exactly to bf16
// (v_cvt_scalef32_pk_bf16_fp8 with scale 1) and no scale multiplies a code:
//     S^T[key][row]  = codes_k[key] . q[row]                   MFMA, fp32
//     s              = S^T * (s_k[key] * scale * log2 e)       one multiplier per S^T register
//     p              = exp2(s - m[row]),  l[row] += p          the plain p
//     P^T operand    = bf16(p * s_v[key])                      V scale folded into p
//     O^T[d][row]   += codes_v[key][d] . P^T                   MFMA, fp32
// S^T rows are keys, so both multipliers of register rr are entries of the page's two
// 64-float scale rows in LDS (eight consecutive keys per lane = two 16-byte reads each).
// A null page (zero codes, zero scales) scores 0 and adds 0: no special case.
//
// Data path -- choice (a), widen once at staging.  Per 64-key page:
//   global   512 threads x (16 B of K codes + 16 B of V codes), threads 0..127 one scale:
//            16.5 KiB per page against v2's 32 KiB, two register sets of 9 VGPRs against
//            v2's 2 x 16, issued two pages ahead as in v2
//   stash    a thread widens its 16 + 16 codes: 16 packed converts, then v2's LDS images --
//            K [key][d] bf16 (two b128 stores), V^T [d][key] bf16 (16 b16 stores; a wave
//            holds the 64 keys of one 16-dim block, each store covers 128 contiguous bytes)
//   per wave 32 MFMAs (32 issue cycles each: 1024) next to about 300 VALU ops: v2's 230
//            (32 max, 32 exp, 32 fma, 32 add, 32 bf16 converts, the mask on diagonal pages)
//            + 16 converts at staging + 32 + 32 scale multiplies and 16 b128 scale reads
// Choice (b), codes in LDS widened per fragment, would put the whole page's conversion on
// every wave: 64 packed converts per operand and page = +128 VALU ops per wave (+40 %), and
// for V a byte transpose on top, to halve LDS bytes that are not the bound here -- the
// softmax VALU work already runs level with the MFMAs (32 x v_exp_f32 at quarter rate alone
// are 512 cycles).  So the LDS images, the fragment reads and both MFMA loops are v2's.
//
// Resources (-Rpass-analysis=kernel-resource-usage, gfx950):
//     G   LDS bytes/block   VGPRs   waves/SIMD   scratch
//     1   72704             205     2            0
//     2   72704             207     2            0
//     4   72704             207     2            0
//     8   72704             207     2            0
// (71680 B of page images as v2 + 2 stages x 2 x 64 fp32 scales; v2 itself: 212 / 214 VGPRs.
// A 512-thread block is 2 waves per SIMD, so one block per CU holds up to 256 VGPRs.)
//
// Measured on MI355X (bench/kv_fp8_flash_bench.py, profiles/kv_fp8_flash.jsonl: cold pages,
// kernels alternated, pass-to-pass spread <= 0.6 %).  Against the per-row kernel on the same
// rows: 0.83x its time at 128 rows of 8B heads (16 workgroups), 0.36-0.56x at 32 workgroups,
// 0.03x from 2K rows.  Against the bf16 flash prefill it is SLOWER: 1.13-1.25x its time from
// 1K rows at both head shapes (8K rows, 8B heads: 632 us = 870 TFLOP/s against 548 us =
// 1004 TFLOP/s), so the halved bytes buy nothing here.  The bf16 kernel reads twice the bytes
// and is faster, so neither is bound by bytes at these shapes; what this kernel adds is the
// VALU work counted above (scale multiplies, scale reads, staging converts: about +30 % per
// page next to the same 32 MFMAs), and the softmax VALU work already ran level with the
// MFMAs.  That is the reading of the counts; no counter run has confirmed it.  It is faster
// (0.76x) only where the bf16 route falls to its 16-token kernel (512 rows at position
// 31744, 8B heads).
#include "flash_tile.h"

namespace {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

constexpr int SC_ELEMS = 2 * PAGE;  // fp32 scales of a stage: K (pre-multiplied), then V

// 16 e4m3 codes -> 16 bf16, exact
__device__ __forceinline__ void widen16(const u32x4& c, bf16x8& lo, bf16x8& hi) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const bf16x2 a = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(c[i], 1.0f, false);
    const bf16x2 b = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(c[i], 1.0f, true);
    bf16x8& d = i < 2 ? lo : hi;
    const int o = 4 * (i & 1);
    d[o] = a[0];
    d[o + 1] = a[1];
    d[o + 2] = b[0];
    d[o + 3] = b[1];
  }
}

template <int G>
__global__ __launch_bounds__(512) void flash_prefill_fp8_kernel(
    const bf16* __restrict__ q, int ldq, const unsigned char* __restrict__ kc,
    const unsigned char* __restrict__ vc, const float* __restrict__ ksc,
    const float* __restrict__ vsc, const int* __restrict__ bt, int bt_stride,
    const Tile* __restrict__ tiles, int n_tiles, int Hkv, float scale_log2,
    bf16* __restrict__ out, int ldo) {
  constexpr int WPH = 8 / G;  // waves per q head
  __shared__ __attribute__((aligned(16))) bf16 lds[2 * (KS_ELEMS + VS_ELEMS)];
  __shared__ __attribute__((aligned(16))) float sls[2 * SC_ELEMS];

  // heads outermost, heaviest (latest) tiles first; one head's tiles share an XCD's L2
  const int nb = n_tiles * Hkv;
  const int b = xcd_remap(blockIdx.x, nb);
  const int kvh = b / n_tiles, ti = n_tiles - 1 - b % n_tiles;
  const Tile T = tiles[ti];
  if (T.n <= 0) return;  // padding tile of a graph-captured prefill (fixed grid)
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  const int r32 = lane & 31, hh = lane >> 5;
  const int h = kvh * G + w / WPH;
  const int t = (w % WPH) * 32 + r32;      // token of this lane's query row
  const int tok = t < T.n ? t : T.n - 1;
  const int my_pos = T.pos0 + tok;
  const int row = T.row0 + tok;

  // Q^T B fragments: k-step s covers d = 16s .. 16s+15, lane half hh holds 8hh .. 8hh+7
  bf16x8 qf[8];
  {
    const bf16* qp = q + (size_t)row * ldq + h * HD + 8 * hh;
#pragma unroll
    for (int s = 0; s < 8; ++s) qf[s] = *reinterpret_cast<const bf16x8*>(qp + 16 * s);
  }
  f32x16_t o[4];
#pragma unroll
  for (int db = 0; db < 4; ++db)
#pragma unroll
    for (int i = 0; i < 16; ++i) o[db][i] = 0.f;
  float m = -INFINITY, l = 0.f;  // m: running max of the scaled scores, log2 units

  const int last = T.pos0 + T.n - 1;
  const int n_kt = last / PAGE + 1;
  const int* btr = bt + (size_t)T.seq * bt_stride;
  const int krow = kperm(r32);

  // A page travels global -> registers -> (widen) -> LDS; two register sets, so its loads
  // are issued two tiles before it is staged (as v2).
  // K: thread c holds key (c >> 3), dims 16 (c & 7)..+15 (row-major image).
  // V: thread c holds key (c & 63), dims 16 (c >> 6)..+15 -- a wave holds the 64 keys of
  // ONE 16-dim column block, so each transposed b16 store writes 128 contiguous bytes.
  // Scales: thread c < 64 the K scale of key c, 64 <= c < 128 the V scale of key c - 64.
  u32x4 kA, vA, kB, vB;
  float sA = 0.f, sB = 0.f;
  auto fetch = [&](int kt, u32x4& kr, u32x4& vr, float& sr) {
    const size_t prow = ((size_t)btr[kt] * Hkv + kvh) * PAGE;  // first (token, head) row
    kr = *reinterpret_cast<const u32x4*>(kc + prow * HD + 16 * tid);
    vr = *reinterpret_cast<const u32x4*>(vc + (prow + (tid & 63)) * HD + 16 * (tid >> 6));
    if (tid < 2 * PAGE) sr = (tid < PAGE ? ksc : vsc)[prow + (tid & 63)];
  };
  auto stash = [&](int st, const u32x4& kr, const u32x4& vr, float sr) {
    bf16* Ks = lds + st * (KS_ELEMS + VS_ELEMS);
    bf16* Vt = Ks + KS_ELEMS;
    bf16x8 lo, hi;
    widen16(kr, lo, hi);
    bf16* kd = &Ks[(tid >> 3) * KLD2 + (tid & 7) * 16];
    *reinterpret_cast<bf16x8*>(kd) = lo;
    *reinterpret_cast<bf16x8*>(kd + 8) = hi;
    widen16(vr, lo, hi);
    bf16* vd = &Vt[(tid >> 6) * 16 * VLD2 + (tid & 63)];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      vd[j * VLD2] = lo[j];
      vd[(8 + j) * VLD2] = hi[j];
    }
    if (tid < 2 * PAGE) sls[st * SC_ELEMS + tid] = tid < PAGE ? sr * scale_log2 : sr;
  };
  auto tile = [&](int kt, int st) {
    const bf16* Ks = lds + st * (KS_ELEMS + VS_ELEMS);
    const bf16* Vt = Ks + KS_ELEMS;
    // this lane's keys of register rr: 32 kh + 16 (rr >> 3) + 8 hh + (rr & 7)
    const float* ksl = sls + st * SC_ELEMS + 8 * hh;
    const float* vsl = ksl + PAGE;

    // ---- S^T = K . Q^T, two 32-key halves ----
    f32x16_t sc[2];
#pragma unroll
    for (int kh = 0; kh < 2; ++kh) {
#pragma unroll
      for (int i = 0; i < 16; ++i) sc[kh][i] = 0.f;
      const bf16* kp = Ks + (32 * kh + krow) * KLD2 + 8 * hh;
#pragma unroll
      for (int s = 0; s < 8; ++s)
        sc[kh] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
            *reinterpret_cast<const bf16x8*>(kp + 16 * s), qf[s], sc[kh], 0, 0, 0);
    }
    // ---- the K scales: scores in log2 units ----
#pragma unroll
    for (int kh = 0; kh < 2; ++kh)
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        const f32x4 s4 =
            *reinterpret_cast<const f32x4*>(ksl + 32 * kh + 16 * (g4 >> 1) + 4 * (g4 & 1));
#pragma unroll
        for (int j = 0; j < 4; ++j) sc[kh][4 * g4 + j] *= s4[j];
      }
    // ---- online softmax for this lane's query row, deferred rescale as v2: O and l are
    // rescaled only when some row's max grew by more than RESCALE_THR, so the unrescaled p
    // stay <= 2^RESCALE_THR ----
    constexpr float RESCALE_THR = 8.f;
    const int k0 = kt * PAGE;
    // some key of the tile may be in the future (workgroup-uniform branch: diagonal pages)
    if (__builtin_amdgcn_readfirstlane(k0 + PAGE - 1 > T.pos0)) {
#pragma unroll
      for (int kh = 0; kh < 2; ++kh)
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) {
          const int key = k0 + 32 * kh + 16 * (rr >> 3) + 8 * hh + (rr & 7);
          if (key > my_pos) sc[kh][rr] = -INFINITY;
        }
    }
    float mx = -INFINITY;
#pragma unroll
    for (int kh = 0; kh < 2; ++kh)
#pragma unroll
      for (int rr = 0; rr < 16; ++rr) mx = fmaxf(mx, sc[kh][rr]);
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    if (__any(mx - m > RESCALE_THR)) {
      const float mn = fmaxf(m, mx);
      const float alpha = exp2f(m - mn);
      m = mn;
      l *= alpha;
#pragma unroll
      for (int db = 0; db < 4; ++db) o[db] *= alpha;
    }
    float ps = 0.f;
    bf16x8 pf[2][2];
#pragma unroll
    for (int kh = 0; kh < 2; ++kh)
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        const f32x4 s4 =
            *reinterpret_cast<const f32x4*>(vsl + 32 * kh + 16 * (g4 >> 1) + 4 * (g4 & 1));
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          // raw v_exp_f32 (arguments <= RESCALE_THR; underflow to 0 is what we want)
          const float p = __builtin_amdgcn_exp2f(sc[kh][4 * g4 + j] - m);
          ps += p;
          pf[kh][g4 >> 1][4 * (g4 & 1) + j] = f2bf(p * s4[j]);
        }
      }
    l += ps;
    // ---- O^T += V^T . P^T ----
#pragma unroll
    for (int db = 0; db < 4; ++db) {
      const bf16* vp = Vt + (32 * db + r32) * VLD2 + 8 * hh;
#pragma unroll
      for (int kh = 0; kh < 2; ++kh)
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2)
          o[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
              *reinterpret_cast<const bf16x8*>(vp + 32 * kh + 16 * s2), pf[kh][s2], o[db], 0, 0, 0);
    }
  };

  fetch(0, kA, vA, sA);
  if (n_kt > 1) fetch(1, kB, vB, sB);
  for (int kt = 0; kt < n_kt; kt += 2) {
    stash(0, kA, vA, sA);
    __syncthreads();  // stage 0 complete; every wave is past tile kt-1 (WAR on stage 1)
    if (kt + 2 < n_kt) fetch(kt + 2, kA, vA, sA);
    tile(kt, 0);
    if (kt + 1 >= n_kt) break;
    stash(1, kB, vB, sB);
    __syncthreads();
    if (kt + 3 < n_kt) fetch(kt + 3, kB, vB, sB);
    tile(kt + 1, 1);
  }

  l += __shfl_xor(l, 32, 64);
  if (t < T.n) {
    const float inv = 1.f / l;
    bf16* op = out + (size_t)row * ldo + h * HD + 4 * hh;
#pragma unroll
    for (int db = 0; db < 4; ++db)
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {  // regs 4g4..4g4+3 = d 32db + 8g4 + 4hh + 0..3
        bf16x4 v;
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = f2bf(o[db][4 * g4 + j] * inv);
        *reinterpret_cast<bf16x4*>(op + 32 * db + 8 * g4) = v;
      }
  }
}

template <int G>
int launch_fp8(const bf16* q, int ldq, const unsigned char* kc, const unsigned char* vc,
               const float* ksc, const float* vsc, const int* bt, int bt_stride,
               const Tile* tiles, int n_tiles, int Hkv, float scale, bf16* out, int ldo,
               hipStream_t st) {
  const float sl2 = scale * 1.4426950408889634f;
  hipLaunchKernelGGL(flash_prefill_fp8_kernel<G>, dim3(n_tiles * Hkv), dim3(512), 0, st, q, ldq,
                     kc, vc, ksc, vsc, bt, bt_stride, tiles, n_tiles, Hkv, sl2, out, ldo);
  P2P_CHECK_LAUNCH();
}

}  // namespace

// As p2p_flash_prefill2 (tiles of at most 256 / (Hq/Hkv) tokens whose K/V, positions
// 0 .. pos0+n-1, are already in the cache; whole 64-key pages of the block table), with the
// code pages and their scale planes in place of the bf16 pages.  Returns 1 for a shape the
// kernel does not take (head_dim != 128, rows not 16-byte aligned), 2 for a group size
// outside {1, 2, 4, 8}.
P2P_API int p2p_flash_prefill_fp8(const void* q, int ldq, const void* k_codes,
                                  const void* v_codes, const float* k_scale,
                                  const float* v_scale, const int* bt, int bt_stride,
                                  const int* tiles, int n_tiles, int n_heads, int n_kv,
                                  int head_dim, float scale, void* out, int ldo, void* stream) {
  if (head_dim != HD || n_kv <= 0 || n_heads % n_kv || (ldq & 7) || (ldo & 3)) return 1;
  if (n_tiles <= 0) return 0;
#define P2P_FLASH_FP8(G_)                                                                     \
  case G_:                                                                                    \
    return launch_fp8<G_>((const bf16*)q, ldq, (const unsigned char*)k_codes,                 \
                          (const unsigned char*)v_codes, k_scale, v_scale, bt, bt_stride,     \
                          (const Tile*)tiles, n_tiles, n_kv, scale, (bf16*)out, ldo,          \
                          (hipStream_t)stream)
  switch (n_heads / n_kv) {
    P2P_FLASH_FP8(1);
    P2P_FLASH_FP8(2);
    P2P_FLASH_FP8(4);
    P2P_FLASH_FP8(8);
  }
#undef P2P_FLASH_FP8
  return 2;
}
