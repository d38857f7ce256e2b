// e4m3fn codes -> bf16 in registers, shared by linear_fp8.hip (skinny M) and linear_fp8_gemm.hip (M > 64).
// v_cvt_pk_f32_fp8 gives two exact fp32 values per call; their upper halves are the bf16 values (an e4m3 value has
// 4 significant bits: truncation is exact, subnormals and +-0 included), packed two per register by one v_perm_b32.
#pragma once

#include "common.h"

namespace cs {

typedef __bf16 fp8_bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned fp8_u32x4 __attribute__((ext_vector_type(4)));

// eight e4m3fn codes (two registers) -> eight bf16 values in k order
__device__ __forceinline__ fp8_bf16x8 dequant8(unsigned lo, unsigned hi) {
  fp8_u32x4 r;
  const unsigned w[2] = {lo, hi};
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const auto a = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[i], false);  // bytes 0, 1
    const auto b = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[i], true);   // bytes 2, 3
    // the upper halves of two fp32 values, the first in the low half
    r[2 * i] = __builtin_amdgcn_perm(__float_as_uint(a[1]), __float_as_uint(a[0]), 0x07060302u);
    r[2 * i + 1] = __builtin_amdgcn_perm(__float_as_uint(b[1]), __float_as_uint(b[0]), 0x07060302u);
  }
  return __builtin_bit_cast(fp8_bf16x8, r);
}

}  // namespace cs
