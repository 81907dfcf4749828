// RoPE + quantising KV write for the FP8 KV cache (engine/kv_cache.py, kv_dtype "fp8").
//
// Cache format, per layer, for K and for V:
//     codes  [num_pages][n_kv_heads][PAGE=64][D=128] OCP e4m3 (one page of one head: 8 KiB)
//     scales [num_pages][n_kv_heads][PAGE=64]        fp32, one per (token, kv head) row
// For a row x (K after RoPE, V as projected): s = amax(|x|) / 448 (s = 1 for a zero row),
// code = e4m3_rne(x / s), so amax maps to 448 and nothing clips.
//
// Input: the [T, (Hq + 2 Hkv) * 128] bf16 output of the qkv projection in
// ops.gemm.rope_row_perm column order: inside a head, 16-column group k holds dims
// 8k..8k+7 then 64+8k..64+8k+7, so the rotate-half partner of a column sits 8 columns on.
//
// Work split: one wave per (token, head), four heads per workgroup.  Lane l loads the
// column pair (2l, 2l+1) = dims (d0, d0+1) with d0 = 64 * hi + 8 * (l >> 3) + 2 * (l & 3),
// hi = bit 2 of l; its partner pair is in lane l ^ 4 (one xor-shuffle per value).  The
// rotation runs with separate roundings (no FMA contraction), the same arithmetic as the
// PyTorch reference, so both sides of a CPU/GPU comparison quantise the same fp32 values.
// K/V heads: amax by the wave reduction of common.h, each lane packs its two codes with
// v_cvt_pk_fp8_f32, and the natural dim order is restored in registers: 16-bit slot
// n = 32 * hi + 4 * (l >> 3) + (l & 3) of the row belongs to lane l, so lane j < 32 fetches
// slots 2j and 2j+1 (two adjacent lanes) and the wave stores the row once, as 32 dwords =
// one full 128-byte row per store instruction; lane 0 stores the scale.  Nothing in the
// cache is read.  q heads take the same route with bf16 pairs (64 dwords = the 256-byte
// q row in natural order, what the attention kernels read).
#include "common.h"

namespace {

constexpr int PAGE = 64;
constexpr int HD = 128;
constexpr float E4M3_MAX = 448.f;

// lane that holds 16-bit (codes) or 32-bit (q) slot n of the natural-order row
__device__ __forceinline__ int slot_lane(int n) {
  return (((n >> 2) & 7) << 3) | (((n >> 5) & 1) << 2) | (n & 3);
}

// rotate_half with the reference's roundings: two products, one add
__device__ __forceinline__ float rot(float mine, float other, float2 c, bool hi) {
#pragma clang fp contract(off)
  const float a = mine * c.x, b = other * c.y;
  return hi ? a + b : a - b;
}

__global__ __launch_bounds__(256) void rope_cache_fp8_kernel(
    const bf16* __restrict__ qkv, int ldqkv, const int* __restrict__ pos,
    const int* __restrict__ slots, const float2* __restrict__ cs, int Hq, int Hkv,
    bf16* __restrict__ q_out, int ldq, unsigned char* __restrict__ kc,
    unsigned char* __restrict__ vc, float* __restrict__ ksc, float* __restrict__ vsc) {
  const int t = blockIdx.y;
  const int hh = blockIdx.x * 4 + (threadIdx.x >> 6);  // wave-uniform
  const int l = threadIdx.x & 63;
  if (hh >= Hq + 2 * Hkv) return;
  const int slot = slots[t];
  if (hh >= Hq && slot < 0) return;  // padding rows write only q
  const bool hi = (l >> 2) & 1;
  const bf16x2 x = *reinterpret_cast<const bf16x2*>(qkv + (size_t)t * ldqkv + (size_t)hh * HD + 2 * l);
  float y0 = (float)x[0], y1 = (float)x[1];
  if (hh < Hq + Hkv) {
    const float2* c = cs + (size_t)pos[t] * 64 + 8 * (l >> 3) + 2 * (l & 3);
    const float2 c0 = c[0], c1 = c[1];
    const float o0 = __shfl_xor(y0, 4, 64), o1 = __shfl_xor(y1, 4, 64);
    y0 = rot(y0, o0, c0, hi);
    y1 = rot(y1, o1, c1, hi);
  }
  if (hh < Hq) {
    union { bf16x2 b; unsigned u; } pk;
    pk.b = bf16x2{f2bf(y0), f2bf(y1)};
    const unsigned v = __shfl(pk.u, slot_lane(l), 64);
    reinterpret_cast<unsigned*>(q_out + (size_t)t * ldq + (size_t)hh * HD)[l] = v;
    return;
  }
  const bool is_k = hh < Hq + Hkv;
  const int h = hh - Hq - (is_k ? 0 : Hkv);
  const float amax = wave_max(fmaxf(fabsf(y0), fabsf(y1)));
  float s = amax / E4M3_MAX;
  if (!(s > 0.f)) s = 1.f;
  const float a0 = fminf(fmaxf(y0 / s, -E4M3_MAX), E4M3_MAX);
  const float a1 = fminf(fmaxf(y1 / s, -E4M3_MAX), E4M3_MAX);
  const unsigned pk = (unsigned)__builtin_amdgcn_cvt_pk_fp8_f32(a0, a1, 0, false);  // bytes 0, 1
  const int src = slot_lane(2 * (l & 31));
  const unsigned lo = __shfl(pk, src, 64) & 0xffffu;
  const unsigned up = __shfl(pk, src + 1, 64) << 16;
  const size_t row = ((size_t)(slot / PAGE) * Hkv + h) * PAGE + (slot % PAGE);
  if (l < 32) reinterpret_cast<unsigned*>((is_k ? kc : vc) + row * HD)[l] = lo | up;
  if (l == 0) (is_k ? ksc : vsc)[row] = s;
}

}  // namespace

// qkv: rope_row_perm column order (see the header); q_out [T, Hq * 128] natural order.
// slots[t] = page * 64 + offset, < 0: the row writes no K/V.
P2P_API int p2p_rope_cache_fp8(const void* qkv, int ldqkv, const int* pos, const int* slots,
                               const void* cos_sin, int T, int Hq, int Hkv, int head_dim,
                               void* q_out, int ldq, void* k_codes, void* v_codes, float* k_scale,
                               float* v_scale, hipStream_t st) {
  if (head_dim != HD || T <= 0 || Hq <= 0 || Hkv <= 0 || (ldqkv & 1) || (ldq & 1))
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(rope_cache_fp8_kernel, dim3((Hq + 2 * Hkv + 3) / 4, T), dim3(256), 0, st,
                     (const bf16*)qkv, ldqkv, pos, slots, (const float2*)cos_sin, Hq, Hkv,
                     (bf16*)q_out, ldq, (unsigned char*)k_codes, (unsigned char*)v_codes, k_scale,
                     v_scale);
  return (int)hipGetLastError();
}
