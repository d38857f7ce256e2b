// Quantising append to an FP8 KV cache for gfx950: k and v rows in bf16 -> OCP e4m3fn codes plus one fp32
// power-of-two scale per (token, kv head), both tensors in one launch.
//
// k / v: bf16 [B, S, Hkv, D] contiguous; kc / vc: e4m3fn [B, Smax, Hkv, D] (row stride Hkv * D bytes, batch
// stride an argument); ks / vs: fp32 [B, Smax, Hkv] (row stride Hkv, batch stride an argument); pos: int32 [B]
// on the device or null. Token (b, s) goes to position (pos ? pos[b] : 0) + s, clamped into [0, Smax - 1] here,
// so no value of pos can move a store out of the cache. Where the clamp folds several tokens of a sequence
// onto one position the last of them is stored and the others are dropped (a token is dropped when its
// successor lands on its own position): which one wins is not left to the order the hardware runs the rows in.
//
// The format of a row x[0 .. D): amax = max |x|; s = 2^e with e the smallest integer with amax * 2^-e <= 448
// (so a non-zero row has amax / s in (224, 448]), read off the fp32 bits of amax = m * 2^x, m in [0.5, 1):
// e = x - 9 if m <= 0.875 (448 = 0.875 * 2^9), else x - 8; e is kept >= -126 so that s and 1 / s are normal
// fp32 numbers; amax == 0 gives s = 1. The code of x[i] is x[i] * 2^-e (exact in fp32) rounded to e4m3fn,
// nearest-even, by v_cvt_pk_fp8_f32 after a clamp to +-448 that a finite row never needs. A non-finite row
// gets unspecified codes in its own place.
//
// kv_append_fp8_kernel<D>: a row lies in D / 8 adjacent lanes, one 16-byte load per lane; amax over the row's
// lanes by xor shuffles (no LDS); four v_cvt_pk_fp8_f32 and one 8-byte store per lane; lane 0 of the row
// stores the scale. 256 / (D / 8) rows per workgroup, the k rows first, then the v rows. Plain vector stores.
#include <math.h>

#include "common.h"
#include "launchers.h"

namespace {

template <int D>
__global__ __launch_bounds__(256) void kv_append_fp8_kernel(const __bf16* __restrict__ k, const __bf16* __restrict__ v,
                                                            const int* __restrict__ pos, unsigned char* __restrict__ kc,
                                                            unsigned char* __restrict__ vc, float* __restrict__ ks,
                                                            float* __restrict__ vs, int S, int Smax, int Hkv,
                                                            size_t batch_stride, size_t scale_batch_stride,
                                                            long long rows) {
  constexpr int LPK = D / 8;  // lanes per row
  const long long r2 = (long long)blockIdx.x * (256 / LPK) + threadIdx.x / LPK;  // the same in all lanes of a row
  if (r2 >= 2 * rows) return;
  const bool is_v = r2 >= rows;
  const long long r = is_v ? r2 - rows : r2;  // (b, s, h)
  const int d0 = (threadIdx.x % LPK) * 8;
  const int h = (int)(r % Hkv);
  const long long t = r / Hkv;
  const int s = (int)(t % S);
  const long long b = t / S;

  const long long p = (long long)(pos != nullptr ? pos[b] : 0) + s;
  const long long last = Smax - 1;
  const long long pc = p < 0 ? 0 : (p > last ? last : p);
  if (s + 1 < S && (p + 1 < 0 ? 0 : (p + 1 > last ? last : p + 1)) == pc) return;  // the successor lands here too

  const uint4 w = *reinterpret_cast<const uint4*>((is_v ? v : k) + r * D + d0);
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

  int e = 0;
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

  // b < B, pc < Smax, h < Hkv: inside the cache and the scales
  const size_t slot = (size_t)pc * Hkv + h;
  *reinterpret_cast<uint2*>((is_v ? vc : kc) + (size_t)b * batch_stride + slot * D + d0) = c;
  if (d0 == 0) (is_v ? vs : ks)[(size_t)b * scale_batch_stride + slot] = __uint_as_float((unsigned)(127 + e) << 23);
}

template <int D>
hipError_t launch_append(const void* k, const void* v, const int* pos, void* kc, void* vc, float* ks, float* vs, int S,
                         int Smax, int Hkv, size_t batch_stride, size_t scale_batch_stride, long long rows,
                         hipStream_t st) {
  constexpr int RPB = 256 / (D / 8);
  const long long blocks = (2 * rows + RPB - 1) / RPB;
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(kv_append_fp8_kernel<D>, dim3((unsigned)blocks), dim3(256), 0, st, (const __bf16*)k,
                     (const __bf16*)v, pos, (unsigned char*)kc, (unsigned char*)vc, ks, vs, S, Smax, Hkv, batch_stride,
                     scale_batch_stride, rows);
  return hipGetLastError();
}

bool aligned(const void* p, uintptr_t n) { return p != nullptr && reinterpret_cast<uintptr_t>(p) % n == 0; }

}  // namespace

hipError_t cs_kv_append_fp8(const void* k, const void* v, const int* pos, void* kc, void* vc, float* ks, float* vs,
                            int B, int S, int Smax, int Hkv, int D, size_t batch_stride, size_t scale_batch_stride,
                            hipStream_t stream) {
  if (B < 0 || S < 0 || Smax < 1 || Hkv < 1 || (D != 64 && D != 128)) return hipErrorInvalidValue;
  if (B == 0 || S == 0) return hipSuccess;
  if (batch_stride % 8 != 0 || batch_stride < (size_t)Smax * Hkv * D) return hipErrorInvalidValue;
  if (scale_batch_stride < (size_t)Smax * Hkv) return hipErrorInvalidValue;
  if (!aligned(k, 16) || !aligned(v, 16) || !aligned(kc, 8) || !aligned(vc, 8) || !aligned(ks, 4) || !aligned(vs, 4))
    return hipErrorInvalidValue;
  if (pos != nullptr && !aligned(pos, 4)) return hipErrorInvalidValue;
  const long long rows = (long long)B * S * Hkv;
  if (rows > (1LL << 40)) return hipErrorInvalidValue;
  if (D == 128)
    return launch_append<128>(k, v, pos, kc, vc, ks, vs, S, Smax, Hkv, batch_stride, scale_batch_stride, rows, stream);
  return launch_append<64>(k, v, pos, kc, vc, ks, vs, S, Smax, Hkv, batch_stride, scale_batch_stride, rows, stream);
}
