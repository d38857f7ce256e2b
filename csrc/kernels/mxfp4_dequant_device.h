// e2m1 codes times a power-of-two block scale -> bf16 in registers, shared by linear_mxfp4.hip (skinny M) and
// linear_mxfp4_gemm.hip (M > 64). v_cvt_scalef32_pk_bf16_fp4 converts the two codes of one byte of a dword (low
// nibble into the low half) and multiplies by an fp32 scale; a code has 2 significant bits, so the result is exact.
#pragma once

#include "common.h"

namespace cs {

typedef __bf16 mxfp4_bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned mxfp4_u32x4 __attribute__((ext_vector_type(4)));

// the eight e2m1 codes of one dword times `scale` -> eight bf16 values in k (nibble) order
__device__ __forceinline__ mxfp4_bf16x8 dequant8(unsigned d, float scale) {
  mxfp4_u32x4 r;
  r[0] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, scale, 0));
  r[1] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, scale, 1));
  r[2] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, scale, 2));
  r[3] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, scale, 3));
  return __builtin_bit_cast(mxfp4_bf16x8, r);
}

}  // namespace cs
