// What the 256-row MFMA flash prefill kernels share (flash_prefill.hip v2 over bf16 pages,
// kv_fp8_flash_prefill.hip over e4m3 pages): the query-tile record, the LDS images of one
// 64-key page and the S^T row permutation.  See the v2 comment in flash_prefill.hip.
#pragma once
#include "common.h"

namespace {

constexpr int PAGE = 64, HD = 128;

struct Tile {
  int row0, n, seq, pos0;
};

constexpr int KLD2 = HD + 8;  // K image row stride (bf16)
constexpr int VLD2 = 64 + 8;  // V^T image row stride (bf16)
constexpr int KS_ELEMS = 64 * KLD2, VS_ELEMS = HD * VLD2;

typedef float f32x16_t __attribute__((ext_vector_type(16)));

__device__ __forceinline__ int kperm(int rho) {  // S^T row rho -> key within the 32-key half
  const int s = rho >> 4, r = rho & 15;
  return 16 * s + 8 * ((r >> 2) & 1) + 4 * (r >> 3) + (r & 3);
}

}  // namespace
