// Paged attention over the FP8 KV cache (decode rows and per-token causal prompt rows).
//
// Cache format (kv_fp8_write.hip, engine/kv_cache.py): per layer, for K and for V,
//     codes  [num_pages][n_kv_heads][PAGE=64][D=128] OCP e4m3 (one page of one head: 8 KiB)
//     scales [num_pages][n_kv_heads][PAGE=64]        fp32, one per (token, kv head) row
// and dequant = float(code) * scale.  The scales never touch the inner products:
//     score[key] = (q . codes_k[key]) * s_k[key] * scale      (once per key, after the dot)
//     out        = sum_key (p[key] * s_v[key]) * codes_v[key]  (once per key, on p)
//
// Contract as paged_attention.hip: grid (chunk, kv head, row), a chunk = 256 keys, all
// G = Hq / Hkv query heads of a kv head scored against the same bytes; one chunk writes the
// bf16 output, more leave fp32 (m, l, o) partials for attn_combine_kernel (attn_combine.h).
// A launch with enough rows to fill the GPU on its own (prompt chunks, large batches) runs
// grid (1, kv head, row) instead: a block walks the chunks its row has (LOOP below).
//
// Load plan (a key is 128 B of codes, half the bf16 kernel's bytes): block = 16 waves x 16
// keys; lane = (key t = lane >> 2, quarter = lane & 3) holds 32 dims = 32 B of its key: two
// 16-byte loads for K, two for V, plus the key's K and V scale (the four quarter lanes read
// the same word: one scale load per key and wave).  Every global load of the wave is issued
// before any math and before the context length is looked at; keys past the context read
// the null page through the zero tail of the block table.
//
// QK: the codes widen in registers to packed bf16 (v_cvt_scalef32_pk_bf16_fp8, two values
// per instruction, exact) and feed v_dot2_f32_bf16 against q in LDS, as in the bf16
// kernel; s_k * scale multiplies the sum after the quarter-lane reduction.
//
// P.V: V goes to LDS STILL AS CODES (row stride 144 B), not widened.  Why: the wave's 16 V
// rows are 2.25 KiB instead of 4.25 KiB, every lane writes two 16-byte words instead of
// four, and the P.V loop reads one dword = 4 dims per key and lane and widens it with two
// v_cvt_pk_f32_fp8 right into the fp32 FMAs -- widening before LDS would cost the same
// conversions plus twice the LDS traffic.  With 4 dims per lane, 32 lanes cover a row, so
// the wave's halves take the even and the odd keys (8 keys deep instead of 16) and meet by
// one xor-32 shuffle per accumulator.  p * s_v is stored per key as [key][head], so a lane
// reads its key's G probabilities as 16-byte words.
//
// Resources (-Rpass-analysis=kernel-resource-usage, gfx950, zero scratch; the bf16 kernel of
// paged_attention.hip in brackets):
//     G   LDS bytes/block   VGPRs       waves/SIMD   blocks/CU
//     1   38272  (71040)     48  (52)   8            2
//     2   39680  (72448)     56  (59)   8            2
//     4   42496  (75264)     64  (61)   8            2   (held at 64 by amdgpu_waves_per_eu)
//     8   76800  (80896)    128 (102)   4            1   (the fp32 merge region, 64 KiB, sets
//                                                         the LDS; the accumulators the VGPRs)
// A 16-wave block takes 4 of a SIMD's 8 wave slots, so two blocks per CU is the ceiling
// whatever the LDS: the smaller V region does not add residency here, it halves the LDS
// bytes written and read per key.
//
// Measured on MI355X (bench/kv_fp8_attn_bench.py, profiles/kv_fp8_attn.jsonl, cold pages):
// 0.76-0.87x the bf16 kernel's time at G = 4 and 0.90-0.94x at G = 8 over 256 .. 32K keys,
// never slower, and not the 0.5x the halved bytes allow: at 8 rows x 32K keys it moves
// 3.4 TB/s of codes where the bf16 kernel moves 5.1 TB/s.  With the same lanes and half the
// bytes per lane the CU has half the bytes in flight (2 blocks x 1024 lanes x 64 B), so the
// long contexts are bound by the block-table -> K/V latency chain, not by HBM.  Two keys
// per lane (512 keys per block) would restore the bytes in flight; not done here.
#include "attn_combine.h"  // PAGE, HD, CHUNK and the split-context combine kernel

namespace {

constexpr int WAVES = 16;
constexpr int KPW = CHUNK / WAVES;  // keys per wave = 16
constexpr int VSB = HD + 16;        // V code row stride in LDS (bytes)
constexpr int LOOP_MIN_BLOCKS = 256;  // (row, kv head) pairs from which a block walks its row

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

// LOOP = false: block (c, h, r) takes chunk c (split mode).  LOOP = true: block (0, h, r)
// walks the chunks of its row's own context and carries (m, l, o) in registers -- thread
// i < G * 128 owns output i -- so it writes the bf16 output itself: no partials, no combine,
// and no blocks for chunks a row does not have.
// (With the loop-carried state it does not fit the 64 VGPRs of two blocks per CU without
// spills, so it is built for 128: 64 / 70 / 88 / 98 VGPRs at G = 1 / 2 / 4 / 8, zero scratch,
// one block per CU from G = 2.)
template <int G, bool LOOP>
__global__ __launch_bounds__(WAVES * 64)
__attribute__((amdgpu_waves_per_eu(G <= 4 && !LOOP ? 8 : 4)))
void paged_attn_fp8_kernel(
    const bf16* __restrict__ q, int ldq, const unsigned char* __restrict__ kc,
    const unsigned char* __restrict__ vc, const float* __restrict__ ksc,
    const float* __restrict__ vsc, const int* __restrict__ bt, int bt_stride,
    const int* __restrict__ row_bt, const int* __restrict__ ctx_lens, int Hkv, float scale,
    int n_chunks, bf16* __restrict__ out, int ldo, float* __restrict__ part_o,
    float* __restrict__ part_ml) {
  static_assert(G * HD <= WAVES * 64, "one merged output per thread");
  const int h = blockIdx.y, r = blockIdx.z;
  const int ctx = ctx_lens[r];
  const int rb = row_bt ? row_bt[r] : r;  // null: row r uses block-table row r (decode)
  const int Hq = Hkv * G;
  float run_m = -INFINITY, run_num = 0.f, run_den = 0.f;  // LOOP: carried over the chunks
  int tid_v = threadIdx.x;

  __shared__ bf16x2 qs[G][HD / 2];
  // V codes (P.V) and the wave partials of O (merge) share one region, as in the bf16 kernel
  constexpr int kVsBytes = WAVES * KPW * VSB;
  constexpr int kSoBytes = WAVES * G * HD * 4;
  __shared__ __attribute__((aligned(16))) char vs_so[kVsBytes > kSoBytes ? kVsBytes : kSoBytes];
  auto& vs = *reinterpret_cast<unsigned char(*)[WAVES][KPW][VSB]>(vs_so);
  auto& so = *reinterpret_cast<float(*)[WAVES][G][HD]>(vs_so);
  __shared__ __attribute__((aligned(16))) float ps[WAVES][KPW][G];  // p * s_v
  __shared__ float sm[WAVES][G], sl[WAVES][G];

  const int c0 = LOOP ? 0 : blockIdx.x;
  // LOOP: the chunks this row has (bounded by max_ctx, as the split grid is)
  const int c1 = LOOP ? min((ctx + CHUNK - 1) / CHUNK, n_chunks) : c0 + 1;
#pragma nounroll
  for (int c = c0; c < c1; ++c) {
  // LOOP: the thread index is made opaque per chunk, so the per-lane addresses derived from
  // it are recomputed (a few VALU ops) instead of held in registers across the chunks
  if (LOOP) asm volatile("" : "+v"(tid_v));
  const int tid = tid_v, lane = tid & 63, w = tid >> 6;
  const int t = lane >> 2, quarter = lane & 3;
  const int og = tid / HD, od = tid % HD;  // the merged output this thread owns (tid < G * HD)
  const int key0 = c * CHUNK + w * KPW;  // first key of this wave

  // 1) all global loads first: 32 codes (2 x 16 B) of K and of V row `t`, and its scales
  u32x4 kr[2], vr[2];
  float sk, sv;
  {
    const int key = key0 + t;
    const int pcol = min(key / PAGE, bt_stride - 1);
    const int page = bt[(size_t)rb * bt_stride + pcol];
    const size_t row = ((size_t)page * Hkv + h) * PAGE + (key % PAGE);
    const u32x4* kp = reinterpret_cast<const u32x4*>(kc + row * HD + quarter * 32);
    const u32x4* vp = reinterpret_cast<const u32x4*>(vc + row * HD + quarter * 32);
    kr[0] = kp[0];
    kr[1] = kp[1];
    vr[0] = vp[0];
    vr[1] = vp[1];
    sk = ksc[row];
    sv = vsc[row];
  }
  if (!LOOP || c == 0) {
    const bf16x2* qrow = reinterpret_cast<const bf16x2*>(q + (size_t)r * ldq + (size_t)h * G * HD);
    for (int i = tid; i < G * HD / 2; i += WAVES * 64) qs[i / (HD / 2)][i % (HD / 2)] = qrow[i];
  }
  if (!LOOP && c * CHUNK >= ctx) return;  // block-uniform: the whole chunk is past the context
  const int n_valid = min(max(ctx - key0, 0), KPW);
  const bool mine = t < n_valid;
  // q is staged; LOOP: and every thread is done reading the last chunk's merge region,
  // which the V rows below overwrite
  __syncthreads();

  const int half = lane >> 5, col = lane & 31;  // P.V: keys of parity `half`, dims 4 col..
  float o[G][4];
  float mg[G], lg[G];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    o[g][0] = o[g][1] = o[g][2] = o[g][3] = 0.f;
    mg[g] = -INFINITY;
    lg[g] = 0.f;
  }
  if (n_valid > 0) {
    // 2) scores
    float s[G];
#pragma unroll
    for (int g = 0; g < G; ++g) s[g] = 0.f;
    if (mine) {
#pragma unroll
      for (int i = 0; i < 2; ++i) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const unsigned cw = kr[i][j];  // dims 32 quarter + 16 i + 4 j .. + 3
          const bf16x2 k01 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(cw, 1.0f, false);
          const bf16x2 k23 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(cw, 1.0f, true);
          const int d2 = quarter * 16 + i * 8 + j * 2;
#pragma unroll
          for (int g = 0; g < G; ++g) {
            s[g] = __builtin_amdgcn_fdot2_f32_bf16(qs[g][d2], k01, s[g], false);
            s[g] = __builtin_amdgcn_fdot2_f32_bf16(qs[g][d2 + 1], k23, s[g], false);
          }
        }
      }
      u32x4* vrow = reinterpret_cast<u32x4*>(&vs[w][t][quarter * 32]);
      vrow[0] = vr[0];
      vrow[1] = vr[1];
    }
    const float kscale = sk * scale;
#pragma unroll
    for (int g = 0; g < G; ++g) {
      s[g] += __shfl_xor(s[g], 1, 64);
      s[g] += __shfl_xor(s[g], 2, 64);
      const float sc = mine ? s[g] * kscale : -INFINITY;
      float m = sc;
#pragma unroll
      for (int o2 = 4; o2 < 64; o2 <<= 1) m = fmaxf(m, __shfl_xor(m, o2, 64));
      const float p = mine ? __expf(sc - m) : 0.f;
      float l = p;
#pragma unroll
      for (int o2 = 4; o2 < 64; o2 <<= 1) l += __shfl_xor(l, o2, 64);
      mg[g] = m;
      lg[g] = l;  // the xor-4..32 sum runs over one lane per key (same quarter)
      if ((g & 3) == quarter) ps[w][t][g] = mine ? p * sv : 0.f;
    }
    // 3) P.V over the wave's keys (same-wave LDS ops stay in order)
    __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0)
    __builtin_amdgcn_wave_barrier();
#pragma unroll 4
    for (int k = half; k < n_valid; k += 2) {
      const unsigned cw = *reinterpret_cast<const unsigned*>(&vs[w][k][4 * col]);
      const f32x2 v01 = __builtin_amdgcn_cvt_pk_f32_fp8(cw, false);
      const f32x2 v23 = __builtin_amdgcn_cvt_pk_f32_fp8(cw, true);
#pragma unroll
      for (int g = 0; g < G; ++g) {
        const float p = ps[w][k][g];
        o[g][0] = fmaf(p, v01[0], o[g][0]);
        o[g][1] = fmaf(p, v01[1], o[g][1]);
        o[g][2] = fmaf(p, v23[0], o[g][2]);
        o[g][3] = fmaf(p, v23[1], o[g][3]);
      }
    }
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
      for (int j = 0; j < 4; ++j) o[g][j] += __shfl_xor(o[g][j], 32, 64);
  }
  __syncthreads();  // every wave's P.V has read its V rows: the region becomes `so`
#pragma unroll
  for (int g = 0; g < G; ++g) {
    if (half == 0)
      *reinterpret_cast<f32x4*>(&so[w][g][4 * col]) = f32x4{o[g][0], o[g][1], o[g][2], o[g][3]};
    if (lane == 0) {
      sm[w][g] = mg[g];
      sl[w][g] = lg[g];
    }
  }
  __syncthreads();
  float M = -INFINITY, num = 0.f, den = 0.f;  // the chunk's (m, o, l) of output (og, od)
  if (tid < G * HD) {
#pragma unroll
    for (int ww = 0; ww < WAVES; ++ww) M = fmaxf(M, sm[ww][og]);
    if (M != -INFINITY) {
#pragma unroll
      for (int ww = 0; ww < WAVES; ++ww) {
        const float e = __expf(sm[ww][og] - M);
        num = fmaf(e, so[ww][og][od], num);
        den = fmaf(e, sl[ww][og], den);
      }
    }
  }
  const size_t oidx = (size_t)r * ldo + (size_t)(h * G + og) * HD + od;
  if (!LOOP) {
    if (tid < G * HD) {
      if (n_chunks == 1) {
        out[oidx] = f2bf(num / den);
      } else {
        const size_t pidx = ((size_t)r * Hq + h * G + og) * n_chunks + c;
        part_o[pidx * HD + od] = num;
        if (od == 0) {
          part_ml[pidx * 2] = M;
          part_ml[pidx * 2 + 1] = den;
        }
      }
    }
  } else {
    // fold the chunk into the running (m, l, o); every chunk here has a valid key, so M is
    // finite and the first fold multiplies the empty state by exp(-inf) = 0
    const float m_new = fmaxf(run_m, M);
    const float ea = __expf(run_m - m_new), eb = __expf(M - m_new);
    run_num = run_num * ea + num * eb;
    run_den = run_den * ea + den * eb;
    run_m = m_new;
  }
  }
  if (LOOP && c1 > 0 && tid_v < G * HD)
    out[(size_t)r * ldo + (size_t)h * G * HD + tid_v] = f2bf(run_num / run_den);
}

template <int G>
int launch_attn_fp8(const void* q, int ldq, const void* kc, const void* vc, const float* ksc,
                    const float* vsc, const int* bt, int bt_stride, const int* row_bt,
                    const int* ctx, int R, int Hkv, float scale, int n_chunks, void* out, int ldo,
                    float* part_o, float* part_ml, hipStream_t st) {
  // From LOOP_MIN_BLOCKS (row, kv head) pairs the rows alone fill the GPU (one block per CU):
  // each block walks its own row's chunks.  That is a prompt chunk (one row per token, the
  // context bound a graph's bucket, far above most rows' contexts) or a large decode batch;
  // below it the chunks of a long context are what spreads the work, so they get a block each.
  if (n_chunks > 1 && (long)R * Hkv >= LOOP_MIN_BLOCKS) {
    hipLaunchKernelGGL((paged_attn_fp8_kernel<G, true>), dim3(1, Hkv, R), dim3(WAVES * 64), 0, st,
                       (const bf16*)q, ldq, (const unsigned char*)kc, (const unsigned char*)vc,
                       ksc, vsc, bt, bt_stride, row_bt, ctx, Hkv, scale, n_chunks, (bf16*)out,
                       ldo, part_o, part_ml);
    return (int)hipGetLastError();
  }
  hipLaunchKernelGGL((paged_attn_fp8_kernel<G, false>), dim3(n_chunks, Hkv, R), dim3(WAVES * 64),
                     0, st, (const bf16*)q, ldq, (const unsigned char*)kc,
                     (const unsigned char*)vc, ksc, vsc, bt, bt_stride, row_bt, ctx, Hkv, scale,
                     n_chunks, (bf16*)out, ldo, part_o, part_ml);
  int e = (int)hipGetLastError();
  if (e || n_chunks == 1) return e;
  hipLaunchKernelGGL(attn_combine_kernel, dim3(R, Hkv * G), dim3(HD * CG), 0, st, part_o, part_ml,
                     ctx, Hkv * G, n_chunks, (bf16*)out, ldo);
  return (int)hipGetLastError();
}

}  // namespace

// Arguments as p2p_paged_attention, with the code pages and their scale planes in place of
// the bf16 pages.  part_o / part_ml: workspace of R*Hq*n_chunks*(128 | 2) floats, unused
// when max_ctx <= 256.
P2P_API int p2p_paged_attention_fp8(const void* q, int ldq, const void* k_codes,
                                    const void* v_codes, const float* k_scale,
                                    const float* v_scale, const int* block_tables, int bt_stride,
                                    const int* row_bt, const int* ctx_lens, int R, int Hq, int Hkv,
                                    int head_dim, float scale, int max_ctx, void* out, int ldo,
                                    float* part_o, float* part_ml, hipStream_t stream) {
  if (head_dim != HD || Hkv <= 0 || Hq % Hkv != 0 || R <= 0 || bt_stride <= 0 || (ldq & 1))
    return (int)hipErrorInvalidValue;
  const int n_chunks = (max_ctx + CHUNK - 1) / CHUNK;
  if (n_chunks < 1 || n_chunks > MAX_CHUNKS) return (int)hipErrorInvalidValue;
  if (n_chunks > 1 && (!part_o || !part_ml)) return (int)hipErrorInvalidValue;
#define P2P_FP8_ATTN(G_)                                                                        \
  case G_:                                                                                      \
    return launch_attn_fp8<G_>(q, ldq, k_codes, v_codes, k_scale, v_scale, block_tables,        \
                               bt_stride, row_bt, ctx_lens, R, Hkv, scale, n_chunks, out, ldo,  \
                               part_o, part_ml, stream)
  switch (Hq / Hkv) {
    P2P_FP8_ATTN(1);
    P2P_FP8_ATTN(2);
    P2P_FP8_ATTN(4);
    P2P_FP8_ATTN(8);
  }
#undef P2P_FP8_ATTN
  return (int)hipErrorInvalidValue;
}
