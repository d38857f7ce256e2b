// Append to a paged KV cache for gfx950: k and v rows in bf16 -> the page pools of one layer, through the block
// table, both tensors in one launch. bf16 pools take the rows as they are; FP8 pools take OCP e4m3fn codes plus
// one fp32 power-of-two scale per (token, kv head), the format and the arithmetic of kv_append_fp8.hip
// (kv_quant_device.h).
//
// k / v: bf16 [B, S, Hkv, D] contiguous; kp / vp: pools [P, page, Hkv, D] (row stride Hkv * D elements, page
// stride an argument, a multiple of 8); ks / vs: fp32 [P, page, Hkv] (row stride Hkv, page stride an argument),
// FP8 only; table: int32 [B, C] (column stride 1, row stride an argument); pos, counts: int32 [B] on the device
// or null. Token (b, s) goes to logical position p = (pos ? pos[b] : 0) + s, which is row p % page of page
// table[b, p / page]. It is stored only if s < (counts ? counts[b] : S), 0 <= p < C * page and the table entry
// lies in [0, P); otherwise it is dropped. Nothing is clamped: in a pool shared by all sequences a folded write
// would land in somebody's live data. So no value of pos, counts or the table moves a store outside the pools
// and the scales, and distinct tokens of a sequence never share a destination. Two table rows that name one
// page are the caller's error (the page then holds one of the writers' rows, in bounds).
//
// kv_append_paged_kernel<D, Fp8>: a row lies in D / 8 adjacent lanes, one 16-byte load per lane; the predicate
// is evaluated per row (the same in all its lanes). bf16: one 16-byte store per lane. FP8: kv_quantize_row, one
// 8-byte store per lane, lane 0 of the row stores the scale. 256 / (D / 8) rows per workgroup, the k rows first,
// then the v rows. Plain vector stores.
#include "common.h"
#include "kv_quant_device.h"
#include "launchers.h"

namespace {

struct PagedPools {
  void *k, *v;
  float *ks, *vs;  // Fp8 only
  size_t page_stride, scale_page_stride;
  const int* table;
  size_t table_stride;
  int C, pages, page;
};

template <int D, bool Fp8>
__global__ __launch_bounds__(256) void kv_append_paged_kernel(const __bf16* __restrict__ k, const __bf16* __restrict__ v,
                                                              const int* __restrict__ pos,
                                                              const int* __restrict__ counts, const PagedPools pool,
                                                              int S, int Hkv, long long rows) {
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

  // the store predicate, per row; every return below takes all lanes of the row
  if (counts != nullptr && s >= counts[b]) return;
  const long long p = (long long)(pos != nullptr ? pos[b] : 0) + s;
  if (p < 0 || p >= (long long)pool.C * pool.page) return;
  const int col = (int)p / pool.page, prow = (int)p - col * pool.page;  // p < C * page <= INT_MAX
  const int entry = pool.table[(size_t)b * pool.table_stride + col];  // col < C: inside the table
  if (entry < 0 || entry >= pool.pages) return;

  // entry < P, prow < page, h < Hkv: inside the pools and the scales
  const size_t slot = (size_t)prow * Hkv + h;
  const uint4 w = *reinterpret_cast<const uint4*>((is_v ? v : k) + r * D + d0);
  if constexpr (Fp8) {
    int e;
    const uint2 c = kv_quantize_row<LPK>(w, e);
    unsigned char* dst = static_cast<unsigned char*>(is_v ? pool.v : pool.k);
    *reinterpret_cast<uint2*>(dst + (size_t)entry * pool.page_stride + slot * D + d0) = c;
    if (d0 == 0) (is_v ? pool.vs : pool.ks)[(size_t)entry * pool.scale_page_stride + slot] = kv_scale_of(e);
  } else {
    __bf16* dst = static_cast<__bf16*>(is_v ? pool.v : pool.k);
    *reinterpret_cast<uint4*>(dst + (size_t)entry * pool.page_stride + slot * D + d0) = w;
  }
}

template <int D, bool Fp8>
hipError_t launch_append(const void* k, const void* v, const int* pos, const int* counts, const PagedPools& pool, int S,
                         int Hkv, long long rows, hipStream_t st) {
  constexpr int RPB = 256 / (D / 8);
  const long long blocks = (2 * rows + RPB - 1) / RPB;
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL((kv_append_paged_kernel<D, Fp8>), dim3((unsigned)blocks), dim3(256), 0, st, (const __bf16*)k,
                     (const __bf16*)v, pos, counts, pool, S, Hkv, rows);
  return hipGetLastError();
}

bool aligned(const void* p, uintptr_t n) { return p != nullptr && reinterpret_cast<uintptr_t>(p) % n == 0; }

}  // namespace

hipError_t cs_kv_append_paged(const void* k, const void* v, const int* pos, const int* counts, const int* table,
                              void* kp, void* vp, float* ks, float* vs, int B, int S, int C, int Hkv, int D, int pages,
                              int page, size_t page_stride, size_t scale_page_stride, size_t table_stride,
                              hipStream_t stream) {
  const bool fp8 = ks != nullptr || vs != nullptr;
  const int tile = cs_attn_decode_key_tile();
  if (B < 0 || S < 0 || C < 1 || Hkv < 1 || pages < 1 || (D != 64 && D != 128)) return hipErrorInvalidValue;
  if (page < tile || page % tile != 0 || (long long)C * page > 0x7fffffffLL) return hipErrorInvalidValue;
  if (B == 0 || S == 0) return hipSuccess;
  if (page_stride % 8 != 0 || page_stride < (size_t)page * Hkv * D || table_stride < (size_t)C)
    return hipErrorInvalidValue;
  const uintptr_t pool_align = fp8 ? 8 : 16;
  if (!aligned(k, 16) || !aligned(v, 16) || !aligned(kp, pool_align) || !aligned(vp, pool_align) || !aligned(table, 4))
    return hipErrorInvalidValue;
  if (fp8 && (!aligned(ks, 4) || !aligned(vs, 4) || scale_page_stride < (size_t)page * Hkv))
    return hipErrorInvalidValue;
  if ((pos != nullptr && !aligned(pos, 4)) || (counts != nullptr && !aligned(counts, 4))) return hipErrorInvalidValue;
  const long long rows = (long long)B * S * Hkv;
  if (rows > (1LL << 40)) return hipErrorInvalidValue;
  const PagedPools pool{kp, vp, ks, vs, page_stride, scale_page_stride, table, table_stride, C, pages, page};
  if (D == 128)
    return fp8 ? launch_append<128, true>(k, v, pos, counts, pool, S, Hkv, rows, stream)
               : launch_append<128, false>(k, v, pos, counts, pool, S, Hkv, rows, stream);
  return fp8 ? launch_append<64, true>(k, v, pos, counts, pool, S, Hkv, rows, stream)
             : launch_append<64, false>(k, v, pos, counts, pool, S, Hkv, rows, stream);
}
