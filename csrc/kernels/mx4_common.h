// Shared by the MXFP4 GEMMs (mx4_gemm.hip, mx4_prefill_gemm.hip): the in-register widening
// of one lane's codes of one k-step.
#pragma once
#include "common.h"

namespace {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// 8 e2m1 codes (one k-step of a lane) * 2^(e - 127) -> 8 bf16: four v_cvt_scalef32_pk_bf16_fp4
__device__ __forceinline__ bf16x8 widen_fp4(unsigned wd, unsigned sw, int h) {
  const float sf = __uint_as_float(((sw >> (8 * h)) & 0xffu) << 23);
  const bf16x2 a = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(wd, sf, 0);
  const bf16x2 b = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(wd, sf, 1);
  const bf16x2 c = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(wd, sf, 2);
  const bf16x2 d = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(wd, sf, 3);
  bf16x8 r;
  r[0] = a.x; r[1] = a.y; r[2] = b.x; r[3] = b.y;
  r[4] = c.x; r[5] = c.y; r[6] = d.x; r[7] = d.y;
  return r;
}

}  // namespace
