// The row arithmetic of the FP8 KV-cache format, shared by kv_append_fp8.hip and kv_append_paged.hip (the format
// itself is stated at the top of kv_append_fp8.hip).
#pragma once

#include <math.h>

#include "common.h"

// A bf16 row of D = 8 * LPK elements lies in LPK adjacent lanes, eight elements (w) per lane; all lanes of the row
// must be active. -> this lane's eight e4m3fn codes; e: the exponent of the row's scale 2^e, the same in all its
// lanes. amax over the row's lanes by xor shuffles (no LDS), four v_cvt_pk_fp8_f32 per lane.
template <int LPK>
__device__ __forceinline__ uint2 kv_quantize_row(const uint4& w, int& e) {
  float f[8];
  f[0] = __uint_as_float(w.x << 16); f[1] = __uint_as_float(w.x & 0xffff0000u);
  f[2] = __uint_as_float(w.y << 16); f[3] = __uint_as_float(w.y & 0xffff0000u);
  f[4] = __uint_as_float(w.z << 16); f[5] = __uint_as_float(w.z & 0xffff0000u);
  f[6] = __uint_as_float(w.w << 16); f[7] = __uint_as_float(w.w & 0xffff0000u);
  float amax = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) amax = fmaxf(amax, fabsf(f[j]));
#pragma unroll
  for (int off = 1; off < LPK; off <<= 1) amax = fmaxf(amax, __shfl_xor(amax, off, 64));

  e = 0;
  if (amax > 0.f) {
    const unsigned bits = __float_as_uint(amax);
    e = (int)((bits >> 23) & 0xffu) - 126 - ((bits & 0x7fffffu) <= 0x600000u ? 9 : 8);
    e = e < -126 ? -126 : e;  // e <= 121 (Inf): both exponent fields below stay in [1, 254]
  }
  const float inv = __uint_as_float((unsigned)(127 - e) << 23);
#pragma unroll
  for (int j = 0; j < 8; ++j) f[j] = fminf(fmaxf(f[j] * inv, -448.f), 448.f);
  uint2 c;
  c.x = (unsigned)__builtin_amdgcn_cvt_pk_fp8_f32(f[0], f[1], 0, false);
  c.x = (unsigned)__builtin_amdgcn_cvt_pk_fp8_f32(f[2], f[3], (int)c.x, true);
  c.y = (unsigned)__builtin_amdgcn_cvt_pk_fp8_f32(f[4], f[5], 0, false);
  c.y = (unsigned)__builtin_amdgcn_cvt_pk_fp8_f32(f[6], f[7], (int)c.y, true);
  return c;
}

// the fp32 scale 2^e of a row (e in [-126, 121])
__device__ __forceinline__ float kv_scale_of(int e) { return __uint_as_float((unsigned)(127 + e) << 23); }
