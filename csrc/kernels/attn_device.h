// The device helpers of the flash-attention kernels, shared by attention.hip (forward and backward) and
// attn_extend.hip (the forward against a filled KV cache): the swizzled [rows][D] LDS image, the MFMA operand
// fragments read from it, the accumulator-as-operand conversion and the LDS-DMA tile copy. attention.hip's header
// comment describes how they fit together.
#pragma once

#include <math.h>

#include "common.h"

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef short i16x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// [rows][D] bf16 image, 16-byte chunks XOR-swizzled per row
template <int D>
struct Img {
  static constexpr int NCH = D / 8;
  static constexpr int ROW = 2 * D;  // bytes
  __device__ static int off(int r, int ch) {
    const int sw = (((r & 3) << 2) | ((r >> 2) & 3)) & (NCH - 1);
    return ROW * r + 16 * (ch ^ sw);
  }
};

__device__ __forceinline__ f32x16 mfma(bf16x8 a, bf16x8 b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}

__device__ __forceinline__ f32x16 zero16() {
  f32x16 z;
#pragma unroll
  for (int e = 0; e < 16; ++e) z[e] = 0.f;
  return z;
}

// row-read operand fragment: image row `row`, k = d = 16 kk + 8h + j (natural order)
template <int D>
__device__ __forceinline__ bf16x8 row_frag(const char* img, int row, int kk, int h) {
  return *reinterpret_cast<const bf16x8*>(img + Img<D>::off(row, 2 * kk + h));
}

// transposed-read operand fragment for "A . X" with X an accumulator tile: lane (r, h) gets
// column d = dbase + r of image rows k0 + 16s.. in the accumulator's k order
// (j -> row k0 + 8(j>>2) + 4h + (j&3)); k0 already includes 16s
template <int D>
__device__ __forceinline__ bf16x8 tr_frag(const char* img, int k0, int dbase, int lane) {
  const int g = lane >> 4, i = lane & 15, q = i >> 2, p = i & 3;
  const int row = k0 + 4 * (g >> 1) + q;
  const int ch = ((dbase + 16 * (g & 1)) >> 3) + (p >> 1);
  const char* a0 = img + Img<D>::off(row, ch) + 8 * (p & 1);
  const char* a1 = img + Img<D>::off(row + 8, ch) + 8 * (p & 1);
  const i16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) i16x4*)(a0));
  const i16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) i16x4*)(a1));
  const bf16x4 blo = __builtin_bit_cast(bf16x4, lo), bhi = __builtin_bit_cast(bf16x4, hi);
  return __builtin_shufflevector(blo, bhi, 0, 1, 2, 3, 4, 5, 6, 7);
}

// registers 8s..8s+7 of an accumulator tile as a bf16 operand fragment
__device__ __forceinline__ bf16x8 acc_frag(const f32x16& x, int s) {
  bf16x8 f;
#pragma unroll
  for (int j = 0; j < 8; ++j) f[j] = (__bf16)x[8 * s + j];
  return f;
}

__device__ __forceinline__ bf16x8 gload8(const __bf16* p, bool ok) {
  if (ok) return *reinterpret_cast<const bf16x8*>(p);
  bf16x8 z;
#pragma unroll
  for (int j = 0; j < 8; ++j) z[j] = (__bf16)0.f;
  return z;
}

// accumulator row of register e for lane half h
__device__ __forceinline__ int acc_row(int e, int h) { return (e & 3) + 8 * (e >> 2) + 4 * h; }

// store an O^T-shaped accumulator set (rows = d, lane = one row of the output) as bf16
template <int D>
__device__ __forceinline__ void store_rowT(const f32x16 (&acc)[D / 32], float mul, __bf16* dst, int h) {
#pragma unroll
  for (int dt = 0; dt < D / 32; ++dt)
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) {
      bf16x4 v;
#pragma unroll
      for (int x = 0; x < 4; ++x) v[x] = (__bf16)(acc[dt][4 * g4 + x] * mul);
      *reinterpret_cast<bf16x4*>(dst + 32 * dt + 8 * g4 + 4 * h) = v;
    }
}

constexpr int kBM = 128;  // queries per workgroup (fwd, dq) / keys per workgroup (dkdv)
constexpr int kBN = 64;   // keys per K/V tile (fwd, dq) / queries per Q/dO tile (dkdv)

// LDS-DMA copy (buffer_load ... lds) of a 64-row [rows][D] global tile into an LDS image, no
// registers: each wave-instruction writes 64 16-byte pieces = 1 KiB of the image contiguously,
// so the swizzle is applied on the SOURCE side (image piece (row, pc) <- global chunk
// pc ^ swz(row)); rows >= nrows get an out-of-range offset and land as zeros.
constexpr int kOOB = 0x7ffffff0;

template <int D>
struct Dma {
  static constexpr int NCH = D / 8, PER_WAVE = kBN * NCH / (4 * 64);  // instructions per wave
  __amdgpu_buffer_rsrc_t rs;
  size_t stride;  // bytes between rows
  int nrows;
  __device__ Dma(const __bf16* base, size_t stride_elems, int nrows_) : stride(stride_elems * 2), nrows(nrows_) {
    const int64_t bytes = nrows_ > 0 ? (int64_t)(nrows_ - 1) * (int64_t)stride + 2 * D : 0;
    rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<__bf16*>(base), (short)0, (int)bytes, 0x00020000);
  }
  __device__ __forceinline__ void issue(char* img, int row0) const {
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
#pragma unroll
    for (int i = 0; i < PER_WAVE; ++i) {
      const int slot = (wv * PER_WAVE + i) * 64 + lane, row = slot / NCH, pc = slot % NCH;
      const int sw = (((row & 3) << 2) | ((row >> 2) & 3)) & (NCH - 1);
      const int grow = row0 + row;
      const int off = grow < nrows ? (int)((size_t)grow * stride) + 16 * (pc ^ sw) : kOOB;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void*)(img + (wv * PER_WAVE + i) * 1024),
                                               16, off, 0, 0, 0);
    }
  }
};

// every wave's LDS-DMA has landed and every wave is past its reads of the other buffer
__device__ __forceinline__ void dma_barrier() {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
}

__device__ __forceinline__ int clampi(int x, int lo, int hi) { return min(max(x, lo), hi); }

}  // namespace
