// Split-context combine shared by the paged attention kernels (paged_attention.hip on
// bf16 pages, kv_fp8_attention.hip on e4m3 pages): both leave fp32 (m, l, o) partials per
// 256-key chunk in the same workspace format.
#pragma once
#include "common.h"

namespace {

constexpr int PAGE = 64;
constexpr int HD = 128;
constexpr int CHUNK = 4 * PAGE;

// Split-K combine: one block per (row, q head).  The chunk statistics go to LDS first
// (one load per chunk, all in flight together), then CG groups of HD threads each sum
// the partial outputs of every CG-th chunk with 8 loads in flight per thread, and the
// groups meet in LDS.  (A serial per-dimension loop over the chunks leaves one load
// in flight per thread: ~85 us per layer at a 32K context.)
constexpr int CG = 8;                  // chunk groups per block
constexpr int MAX_CHUNKS = 131072 / CHUNK;  // 128K-token contexts
__global__ __launch_bounds__(HD * CG) void attn_combine_kernel(const float* __restrict__ part_o,
                                                               const float* __restrict__ part_ml,
                                                               const int* __restrict__ ctx_lens,
                                                               int Hq, int n_chunks,
                                                               bf16* __restrict__ out, int ldo) {
  __shared__ float s_e[MAX_CHUNKS];  // exp(m_c - M)
  __shared__ float s_l[MAX_CHUNKS];
  __shared__ float s_red[CG][HD];
  __shared__ float s_wmax[HD * CG / 64];
  const int r = blockIdx.x, hq = blockIdx.y, tid = threadIdx.x;
  const int d = tid % HD, grp = tid / HD;
  const int nc = min(min((ctx_lens[r] + CHUNK - 1) / CHUNK, n_chunks), MAX_CHUNKS);
  const size_t base = ((size_t)r * Hq + hq) * n_chunks;
  float mloc = -INFINITY;
  for (int c = tid; c < nc; c += HD * CG) {
    const float m = part_ml[(base + c) * 2];
    s_e[c] = m;
    s_l[c] = part_ml[(base + c) * 2 + 1];
    mloc = fmaxf(mloc, m);
  }
  mloc = wave_max(mloc);
  if ((tid & 63) == 0) s_wmax[tid >> 6] = mloc;
  __syncthreads();
  float M = -INFINITY;
#pragma unroll
  for (int i = 0; i < HD * CG / 64; ++i) M = fmaxf(M, s_wmax[i]);
  __syncthreads();
  for (int c = tid; c < nc; c += HD * CG) s_e[c] = s_e[c] == -INFINITY ? 0.f : __expf(s_e[c] - M);
  __syncthreads();
  float num = 0.f;
  const float* po = part_o + base * HD + d;
  int c = grp;
  for (; c + 7 * CG < nc; c += 8 * CG) {
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = po[(size_t)(c + u * CG) * HD];
#pragma unroll
    for (int u = 0; u < 8; ++u) num = fmaf(s_e[c + u * CG], v[u], num);
  }
  for (; c < nc; c += CG) num = fmaf(s_e[c], po[(size_t)c * HD], num);
  s_red[grp][d] = num;
  __syncthreads();
  if (grp == 0) {
    float tot = 0.f, den = 0.f;
#pragma unroll
    for (int g = 0; g < CG; ++g) tot += s_red[g][d];
    for (int i = 0; i < nc; ++i) den = fmaf(s_e[i], s_l[i], den);
    out[(size_t)r * ldo + (size_t)hq * HD + d] = f2bf(den > 0.f ? tot / den : 0.f);
  }
}

}  // namespace
