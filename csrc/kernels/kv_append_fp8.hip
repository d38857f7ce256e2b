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
// The row arithmetic (amax, exponent, codes) is kv_quantize_row in kv_quant_device.h, shared with kv_append_paged.hip.
#include <math.h>

#include "common.h"
#include "kv_quant_device.h"
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
  int e;
  const uint2 c = kv_quantize_row<LPK>(w, e);  // kv_quant_device.h

  // b < B, pc < Smax, h < Hkv: inside the cache and the scales
  const size_t slot = (size_t)pc * Hkv + h;
  *reinterpret_cast<uint2*>((is_v ? vc : kc) + (size_t)b * batch_stride + slot * D + d0) = c;
  if (d0 == 0) (is_v ? vs : ks)[(size_t)b * scale_batch_stride + slot] = kv_scale_of(e);
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
