// Decoder-LM elementwise hot ops for gfx950 (the BASELINE "Llama-3 8B bf16 pure DP"
// extension config): RMSNorm forward/backward, SwiGLU forward/backward, rotary
// position embedding forward/backward. fp32 or bf16 storage, fp32 math.
//
// RMSNorm: one 256-thread workgroup per row (D up to 16K), row sum of squares by
// wave shuffles + LDS, vectorised 8-byte (bf16 x4) / 16-byte (fp32 x4) accesses.
// The weight gradient is reduced deterministically: every workgroup writes one
// fp32 partial row per ROWS_PER_BLOCK rows, a second kernel sums the partials.
#include <hip/hip_bf16.h>

#include <initializer_list>

#include "common.h"
#include "launchers.h"

namespace {

__device__ __forceinline__ float ld(const float* p, size_t i) { return p[i]; }
__device__ __forceinline__ float ld(const __hip_bfloat16* p, size_t i) { return __bfloat162float(p[i]); }
__device__ __forceinline__ void st(float* p, size_t i, float v) { p[i] = v; }
__device__ __forceinline__ void st(__hip_bfloat16* p, size_t i, float v) { p[i] = __float2bfloat16(v); }

constexpr int kRowsPerBlock = 8;

// ---- the RMSNorm row arithmetic, one definition for the plain kernels and for the ones that fuse the
// residual add (add_rmsnorm_*): the same expressions over the same values give the same bits
__device__ __forceinline__ float rms_rstd(float ss, int D, float eps) { return rsqrtf(ss / (float)D + eps); }
__device__ __forceinline__ float rms_scale(float x, float r, float w) { return x * r * w; }
__device__ __forceinline__ float rms_dot(float w, float g, float x) { return w * g * x; }
// c = r^3 dot / D;  dx_j = r*w_j*g_j - c x_j;  dw partial_j += g_j x_j r
__device__ __forceinline__ float rms_c(float r, float dot, int D) { return r * r * r * dot / (float)D; }
__device__ __forceinline__ float rms_dx(float r, float c, float w, float g, float x) { return r * w * g - c * x; }
__device__ __forceinline__ float rms_dw(float g, float x, float r) { return g * x * r; }

template <typename T, typename W>
__global__ __launch_bounds__(256) void rmsnorm_fwd_kernel(const T* __restrict__ x, const W* __restrict__ w,
                                                          T* __restrict__ y, float* __restrict__ rstd, int rows,
                                                          int D, float eps) {
  __shared__ float red[16];
  const int row = blockIdx.x;
  if (row >= rows) return;
  const T* xr = x + (size_t)row * D;
  float ss = 0.f;
  for (int i = threadIdx.x; i < D; i += blockDim.x) {
    const float v = ld(xr, i);
    ss += v * v;
  }
  ss = cs::block_sum(ss, red);
  const float r = rms_rstd(ss, D, eps);
  if (threadIdx.x == 0) rstd[row] = r;
  T* yr = y + (size_t)row * D;
  for (int i = threadIdx.x; i < D; i += blockDim.x) st(yr, i, rms_scale(ld(xr, i), r, ld(w, i)));
}

// dx_j = r*w_j*g_j - (r^3/D) x_j sum_i(w_i g_i x_i);  dw partial_j = sum_rows g_j x_j r
template <typename T, typename W>
__global__ __launch_bounds__(256) void rmsnorm_bwd_kernel(const T* __restrict__ x, const W* __restrict__ w,
                                                          const float* __restrict__ rstd, const T* __restrict__ g,
                                                          T* __restrict__ dx, float* __restrict__ dw_part, int rows,
                                                          int D) {
  __shared__ float red[16];
  const int r0 = blockIdx.x * kRowsPerBlock;
  float* part = dw_part + (size_t)blockIdx.x * D;
  for (int i = threadIdx.x; i < D; i += blockDim.x) part[i] = 0.f;
  for (int rr = 0; rr < kRowsPerBlock; ++rr) {
    const int row = r0 + rr;
    if (row >= rows) break;
    const T* xr = x + (size_t)row * D;
    const T* gr = g + (size_t)row * D;
    const float r = rstd[row];
    float dot = 0.f;
    for (int i = threadIdx.x; i < D; i += blockDim.x) dot += rms_dot(ld(w, i), ld(gr, i), ld(xr, i));
    dot = cs::block_sum(dot, red);
    const float c = rms_c(r, dot, D);
    T* dxr = dx + (size_t)row * D;
    for (int i = threadIdx.x; i < D; i += blockDim.x) {
      const float xv = ld(xr, i), gv = ld(gr, i);
      st(dxr, i, rms_dx(r, c, ld(w, i), gv, xv));
      part[i] += rms_dw(gv, xv, r);  // same thread owns column i for every row: no race
    }
  }
}

// ---- 4-wide path (D % 4 == 0, D <= 4 * 256 * kMaxQ): 16/8-byte accesses, the row held in
// registers between the reduction and the scaling pass, the weight-gradient partial of a block
// kept in registers across its rows (one store per block instead of a read-modify-write per row)
constexpr int kMaxQ = 8, kRows4 = 16;

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ float4 ld4(const __hip_bfloat16* p) {
  const uint2 r = *reinterpret_cast<const uint2*>(p);
  return make_float4(__uint_as_float(r.x << 16), __uint_as_float(r.x & 0xffff0000u), __uint_as_float(r.y << 16),
                     __uint_as_float(r.y & 0xffff0000u));
}
__device__ __forceinline__ void st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }
__device__ __forceinline__ void st4(__hip_bfloat16* p, float4 v) {
  __hip_bfloat16 e[4] = {__float2bfloat16(v.x), __float2bfloat16(v.y), __float2bfloat16(v.z), __float2bfloat16(v.w)};
  *reinterpret_cast<uint2*>(p) = *reinterpret_cast<const uint2*>(e);
}

__device__ __forceinline__ float rms_ss4(float4 v) { return v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w; }
__device__ __forceinline__ float4 rms_scale4(float4 v, float r, float4 w) {
  return make_float4(v.x * r * w.x, v.y * r * w.y, v.z * r * w.z, v.w * r * w.w);
}
__device__ __forceinline__ float rms_dot4(float4 w, float4 g, float4 x) {
  return w.x * g.x * x.x + w.y * g.y * x.y + w.z * g.z * x.z + w.w * g.w * x.w;
}
__device__ __forceinline__ float4 rms_dx4(float r, float c, float4 w, float4 g, float4 x) {
  return make_float4(r * w.x * g.x - c * x.x, r * w.y * g.y - c * x.y, r * w.z * g.z - c * x.z,
                     r * w.w * g.w - c * x.w);
}
__device__ __forceinline__ void rms_dw4(float4& acc, float4 g, float4 x, float r) {
  acc.x += g.x * x.x * r;
  acc.y += g.y * x.y * r;
  acc.z += g.z * x.z * r;
  acc.w += g.w * x.w * r;
}

template <typename T, typename W, typename O>
__global__ __launch_bounds__(256) void rmsnorm_fwd4_kernel(const T* __restrict__ x, const W* __restrict__ w,
                                                           O* __restrict__ y, float* __restrict__ rstd, int rows,
                                                           int D, float eps) {
  __shared__ float red[16];
  const int row = blockIdx.x, DQ = D >> 2;
  const T* xr = x + (size_t)row * D;
  float4 v[kMaxQ];
  float ss = 0.f;
#pragma unroll
  for (int k = 0; k < kMaxQ; ++k) {
    const int q = threadIdx.x + k * 256;
    if (q < DQ) {
      v[k] = ld4(xr + 4 * q);
      ss += rms_ss4(v[k]);
    }
  }
  ss = cs::block_sum(ss, red);
  const float r = rms_rstd(ss, D, eps);
  if (threadIdx.x == 0) rstd[row] = r;
  O* yr = y + (size_t)row * D;
#pragma unroll
  for (int k = 0; k < kMaxQ; ++k) {
    const int q = threadIdx.x + k * 256;
    if (q < DQ) {
      st4(yr + 4 * q, rms_scale4(v[k], r, ld4(w + 4 * q)));
    }
  }
}

// kRows4 rows per block; dw_part[block][D] = sum over the block's rows of g*x*r
template <typename T, typename W, typename G>
__global__ __launch_bounds__(256) void rmsnorm_bwd4_kernel(const T* __restrict__ x, const W* __restrict__ w,
                                                           const float* __restrict__ rstd, const G* __restrict__ g,
                                                           T* __restrict__ dx, float* __restrict__ dw_part, int rows,
                                                           int D) {
  __shared__ float red[16];
  const int DQ = D >> 2;
  float4 wv[kMaxQ], acc[kMaxQ];
#pragma unroll
  for (int k = 0; k < kMaxQ; ++k) {
    const int q = threadIdx.x + k * 256;
    wv[k] = q < DQ ? ld4(w + 4 * q) : make_float4(0.f, 0.f, 0.f, 0.f);
    acc[k] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  const int r0 = blockIdx.x * kRows4;
  for (int rr = 0; rr < kRows4; ++rr) {
    const int row = r0 + rr;
    if (row >= rows) break;  // uniform across the block
    const T* xr = x + (size_t)row * D;
    const G* gr = g + (size_t)row * D;
    float4 xv[kMaxQ], gv[kMaxQ];
    float dot = 0.f;
#pragma unroll
    for (int k = 0; k < kMaxQ; ++k) {
      const int q = threadIdx.x + k * 256;
      if (q < DQ) {
        xv[k] = ld4(xr + 4 * q);
        gv[k] = ld4(gr + 4 * q);
        dot += rms_dot4(wv[k], gv[k], xv[k]);
      }
    }
    dot = cs::block_sum(dot, red);
    const float r = rstd[row];
    const float c = rms_c(r, dot, D);
    T* dxr = dx + (size_t)row * D;
#pragma unroll
    for (int k = 0; k < kMaxQ; ++k) {
      const int q = threadIdx.x + k * 256;
      if (q < DQ) {
        st4(dxr + 4 * q, rms_dx4(r, c, wv[k], gv[k], xv[k]));
        rms_dw4(acc[k], gv[k], xv[k], r);
      }
    }
  }
  float* part = dw_part + (size_t)blockIdx.x * D;
#pragma unroll
  for (int k = 0; k < kMaxQ; ++k) {
    const int q = threadIdx.x + k * 256;
    if (q < DQ) st4(part + 4 * q, acc[k]);
  }
}

// dw[4q..4q+3] = sum_p part[p][4q..]: 16 column quads x 16 partial lanes per block, lanes
// combined through LDS in lane order (deterministic)
template <typename W>
__global__ __launch_bounds__(256) void colsum4_kernel(const float* __restrict__ part, int P, int D,
                                                      W* __restrict__ dw) {
  __shared__ float4 sh[16][16];
  const int cq = threadIdx.x & 15, pl = threadIdx.x >> 4, q = blockIdx.x * 16 + cq;
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  if (4 * q < D) {
#pragma unroll 8
    for (int p = pl; p < P; p += 16) {
      const float4 v = ld4(part + (size_t)p * D + 4 * q);
      s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
  }
  sh[pl][cq] = s;
  __syncthreads();
  if (pl != 0 || 4 * q >= D) return;
  float4 t = sh[0][cq];
  for (int l = 1; l < 16; ++l) {
    t.x += sh[l][cq].x; t.y += sh[l][cq].y; t.z += sh[l][cq].z; t.w += sh[l][cq].w;
  }
  st4(dw + 4 * q, t);
}

template <typename W>
__global__ __launch_bounds__(256) void colsum_kernel(const float* __restrict__ part, int P, int D,
                                                     W* __restrict__ dw) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= D) return;
  float s = 0.f;
  for (int p = 0; p < P; ++p) s += part[(size_t)p * D + i];
  st(dw, i, s);
}

// ---- residual add fused into the norm that follows it: h = x + delta, y = rms_norm(h, w).
// The sum is one fp32 add rounded once to h's dtype, and the statistics and y are those of h as
// stored, so the pair is rms_norm_fwd(x + delta) bit for bit and the backward, which re-reads the
// stored h, differentiates the function that ran.
__device__ __forceinline__ float as_stored(const float*, float v) { return v; }
__device__ __forceinline__ float as_stored(const __hip_bfloat16*, float v) {
  return __bfloat162float(__float2bfloat16(v));
}
template <typename T>
__device__ __forceinline__ float4 as_stored4(const T* p, float4 v) {
  return make_float4(as_stored(p, v.x), as_stored(p, v.y), as_stored(p, v.z), as_stored(p, v.w));
}
// an add that stays an add (__fadd_rn, and operands that are never products: a loaded value and a
// finished result), so that the sum has the bits of the two-kernel composition
__device__ __forceinline__ float4 add4_rn(float4 a, float4 b) {
  return make_float4(__fadd_rn(a.x, b.x), __fadd_rn(a.y, b.y), __fadd_rn(a.z, b.z), __fadd_rn(a.w, b.w));
}

// scalar path: x, delta, h, y of one dtype
template <typename T, typename W>
__global__ __launch_bounds__(256) void add_rmsnorm_fwd_kernel(const T* __restrict__ x, const T* __restrict__ delta,
                                                              const W* __restrict__ w, T* __restrict__ h,
                                                              T* __restrict__ y, float* __restrict__ rstd, int rows,
                                                              int D, float eps) {
  __shared__ float red[16];
  const int row = blockIdx.x;
  if (row >= rows) return;
  const T* xr = x + (size_t)row * D;
  const T* dr = delta + (size_t)row * D;
  T* hr = h + (size_t)row * D;
  float ss = 0.f;
  for (int i = threadIdx.x; i < D; i += blockDim.x) {
    const float v = as_stored(hr, __fadd_rn(ld(xr, i), ld(dr, i)));
    st(hr, i, v);
    ss += v * v;
  }
  ss = cs::block_sum(ss, red);
  const float r = rms_rstd(ss, D, eps);
  if (threadIdx.x == 0) rstd[row] = r;
  T* yr = y + (size_t)row * D;
  // every thread re-reads the elements of h that it wrote itself
  for (int i = threadIdx.x; i < D; i += blockDim.x) st(yr, i, rms_scale(ld(hr, i), r, ld(w, i)));
}

// scalar path: g, gh, dx in h's dtype; gh == nullptr: no gradient reaches h but the norm's;
// dx == nullptr: only the weight gradient is wanted
template <typename T, typename W>
__global__ __launch_bounds__(256) void add_rmsnorm_bwd_kernel(const T* __restrict__ h, const W* __restrict__ w,
                                                              const float* __restrict__ rstd, const T* __restrict__ g,
                                                              const T* __restrict__ gh, T* __restrict__ dx,
                                                              float* __restrict__ dw_part, int rows, int D) {
  __shared__ float red[16];
  const int r0 = blockIdx.x * kRowsPerBlock;
  float* part = dw_part + (size_t)blockIdx.x * D;
  for (int i = threadIdx.x; i < D; i += blockDim.x) part[i] = 0.f;
  for (int rr = 0; rr < kRowsPerBlock; ++rr) {
    const int row = r0 + rr;
    if (row >= rows) break;
    const T* xr = h + (size_t)row * D;
    const T* gr = g + (size_t)row * D;
    const float r = rstd[row];
    float dot = 0.f;
    for (int i = threadIdx.x; i < D; i += blockDim.x) dot += rms_dot(ld(w, i), ld(gr, i), ld(xr, i));
    dot = cs::block_sum(dot, red);
    const float c = rms_c(r, dot, D);
    for (int i = threadIdx.x; i < D; i += blockDim.x) {
      const float xv = ld(xr, i), gv = ld(gr, i);
      float d = rms_dx(r, c, ld(w, i), gv, xv);
      if (gh) d = __fadd_rn(ld(gh, (size_t)row * D + i), d);
      if (dx) st(dx, (size_t)row * D + i, d);
      part[i] += rms_dw(gv, xv, r);  // same thread owns column i for every row: no race
    }
  }
}

// 4-wide: x (and h) of dtype T, delta of dtype Dl, y of dtype O
template <typename T, typename Dl, typename W, typename O>
__global__ __launch_bounds__(256) void add_rmsnorm_fwd4_kernel(const T* __restrict__ x, const Dl* __restrict__ delta,
                                                               const W* __restrict__ w, T* __restrict__ h,
                                                               O* __restrict__ y, float* __restrict__ rstd, int rows,
                                                               int D, float eps) {
  __shared__ float red[16];
  const int row = blockIdx.x, DQ = D >> 2;
  const T* xr = x + (size_t)row * D;
  const Dl* dr = delta + (size_t)row * D;
  T* hr = h + (size_t)row * D;
  float4 v[kMaxQ];
  float ss = 0.f;
#pragma unroll
  for (int k = 0; k < kMaxQ; ++k) {
    const int q = threadIdx.x + k * 256;
    if (q < DQ) {
      v[k] = as_stored4(hr, add4_rn(ld4(xr + 4 * q), ld4(dr + 4 * q)));
      st4(hr + 4 * q, v[k]);
      ss += rms_ss4(v[k]);
    }
  }
  ss = cs::block_sum(ss, red);
  const float r = rms_rstd(ss, D, eps);
  if (threadIdx.x == 0) rstd[row] = r;
  O* yr = y + (size_t)row * D;
#pragma unroll
  for (int k = 0; k < kMaxQ; ++k) {
    const int q = threadIdx.x + k * 256;
    if (q < DQ) st4(yr + 4 * q, rms_scale4(v[k], r, ld4(w + 4 * q)));
  }
}

// 4-wide: kRows4 rows per block and the dw partials exactly as rmsnorm_bwd4_kernel; d = gh + dx of the
// norm, stored in h's dtype (dx) and / or in delta's (dd) where those are wanted
template <typename T, typename W, typename G, typename Dd>
__global__ __launch_bounds__(256) void add_rmsnorm_bwd4_kernel(const T* __restrict__ h, const W* __restrict__ w,
                                                               const float* __restrict__ rstd, const G* __restrict__ g,
                                                               const T* __restrict__ gh, T* __restrict__ dx,
                                                               Dd* __restrict__ dd, float* __restrict__ dw_part,
                                                               int rows, int D) {
  __shared__ float red[16];
  const int DQ = D >> 2;
  float4 wv[kMaxQ], acc[kMaxQ];
#pragma unroll
  for (int k = 0; k < kMaxQ; ++k) {
    const int q = threadIdx.x + k * 256;
    wv[k] = q < DQ ? ld4(w + 4 * q) : make_float4(0.f, 0.f, 0.f, 0.f);
    acc[k] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  const int r0 = blockIdx.x * kRows4;
  for (int rr = 0; rr < kRows4; ++rr) {
    const int row = r0 + rr;
    if (row >= rows) break;  // uniform across the block
    const T* xr = h + (size_t)row * D;
    const G* gr = g + (size_t)row * D;
    const size_t ro = (size_t)row * D;
    float4 xv[kMaxQ], gv[kMaxQ], hv[kMaxQ];
    float dot = 0.f;
#pragma unroll
    for (int k = 0; k < kMaxQ; ++k) {
      const int q = threadIdx.x + k * 256;
      if (q < DQ) {
        xv[k] = ld4(xr + 4 * q);
        gv[k] = ld4(gr + 4 * q);
        if (gh) hv[k] = ld4(gh + ro + 4 * q);  // in flight across the reduction, not issued behind it
        dot += rms_dot4(wv[k], gv[k], xv[k]);
      }
    }
    dot = cs::block_sum(dot, red);
    const float r = rstd[row];
    const float c = rms_c(r, dot, D);
#pragma unroll
    for (int k = 0; k < kMaxQ; ++k) {
      const int q = threadIdx.x + k * 256;
      if (q < DQ) {
        float4 d = rms_dx4(r, c, wv[k], gv[k], xv[k]);
        if (gh) d = add4_rn(hv[k], d);
        if (dx) st4(dx + ro + 4 * q, d);
        if (dd) st4(dd + ro + 4 * q, d);
        rms_dw4(acc[k], gv[k], xv[k], r);
      }
    }
  }
  float* part = dw_part + (size_t)blockIdx.x * D;
#pragma unroll
  for (int k = 0; k < kMaxQ; ++k) {
    const int q = threadIdx.x + k * 256;
    if (q < DQ) st4(part + 4 * q, acc[k]);
  }
}

__device__ __forceinline__ float sigmoidf(float a) { return 1.f / (1.f + __expf(-a)); }

template <typename T>
__global__ __launch_bounds__(256) void swiglu_fwd_kernel(const T* __restrict__ a, const T* __restrict__ b,
                                                         T* __restrict__ out, size_t n) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const float av = ld(a, i);
    st(out, i, av * sigmoidf(av) * ld(b, i));
  }
}

// One definition for the scalar and the 4-wide backward, with the one fusable multiply-add written as
// an fma: left to -ffp-contract the compiler fused it in the 4-wide kernels and in the scalar loop's
// steady state but not in its peeled first trip, so the same element could differ by an ulp between
// the two kernels (and with its position in the grid).
__device__ __forceinline__ void swiglu_grad1(float a, float b, float g, float& da, float& db) {
  const float s = sigmoidf(a);
  da = g * b * s * fmaf(a, 1.f - s, 1.f);
  db = g * a * s;
}

template <typename T>
__global__ __launch_bounds__(256) void swiglu_bwd_kernel(const T* __restrict__ a, const T* __restrict__ b,
                                                         const T* __restrict__ g, T* __restrict__ da,
                                                         T* __restrict__ db, size_t n) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    float x, y;
    swiglu_grad1(ld(a, i), ld(b, i), ld(g, i), x, y);
    st(da, i, x);
    st(db, i, y);
  }
}

// 4-wide SwiGLU (8-byte bf16 / 16-byte fp32 accesses; n % 4 == 0, 16-byte aligned operands):
// the [tokens, 14336] gate/up pair of the Llama-3-8B MLP is a pure bandwidth pass
template <typename T>
__global__ __launch_bounds__(256) void swiglu_fwd4_kernel(const T* __restrict__ a, const T* __restrict__ b,
                                                          T* __restrict__ out, size_t n4) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
    const float4 av = ld4(a + 4 * i), bv = ld4(b + 4 * i);
    st4(out + 4 * i, make_float4(av.x * sigmoidf(av.x) * bv.x, av.y * sigmoidf(av.y) * bv.y,
                                 av.z * sigmoidf(av.z) * bv.z, av.w * sigmoidf(av.w) * bv.w));
  }
}

template <typename T>
__global__ __launch_bounds__(256) void swiglu_bwd4_kernel(const T* __restrict__ a, const T* __restrict__ b,
                                                          const T* __restrict__ g, T* __restrict__ da,
                                                          T* __restrict__ db, size_t n4) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
    const float4 av = ld4(a + 4 * i), bv = ld4(b + 4 * i), gv = ld4(g + 4 * i);
    float4 x, y;
    swiglu_grad1(av.x, bv.x, gv.x, x.x, y.x);
    swiglu_grad1(av.y, bv.y, gv.y, x.y, y.y);
    swiglu_grad1(av.z, bv.z, gv.z, x.z, y.z);
    swiglu_grad1(av.w, bv.w, gv.w, x.w, y.w);
    st4(da + 4 * i, x);
    st4(db + 4 * i, y);
  }
}

bool aligned16(std::initializer_list<const void*> ps) {
  for (const void* p : ps)
    if (reinterpret_cast<uintptr_t>(p) % 16 != 0) return false;
  return true;
}

// x: [B, S, H, hd] contiguous, pairs (2j, 2j+1) rotated by angle (pos, j); sign = +1 fwd, -1 bwd
template <typename T>
__global__ __launch_bounds__(256) void rope_kernel(const T* __restrict__ x, const float* __restrict__ cosv,
                                                   const float* __restrict__ sinv, T* __restrict__ out, int S, int H,
                                                   int hd, size_t npairs, float sign) {
  const int half = hd >> 1;
  for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < npairs; p += (size_t)gridDim.x * blockDim.x) {
    const int j = (int)(p % half);
    const size_t rowi = p / half;  // (b, s, h)
    const int s = (int)((rowi / H) % S);
    const float c = cosv[(size_t)s * half + j], sn = sign * sinv[(size_t)s * half + j];
    const float x0 = ld(x, 2 * p), x1 = ld(x, 2 * p + 1);
    st(out, 2 * p, x0 * c - x1 * sn);
    st(out, 2 * p + 1, x0 * sn + x1 * c);
  }
}

int grid_for(size_t n) {
  size_t b = (n + 255) / 256;
  return (int)(b > 16384 ? 16384 : (b == 0 ? 1 : b));
}

// ---- QK-norm: RMSNorm over the head dimension of q [B, S, Hq, HD] and k [B, S, Hkv, HD] (one fp32 gain
// [HD] per projection) followed by the rotation of rope_kernel, rounded once. One launch walks the
// nq = B*S*Hq head-rows of q and then the nk = B*S*Hkv of k as one row range [0, nq + nk).
// A head-row lives in HD / 4 adjacent lanes of one wave (half a wave for HD = 128, a quarter for
// HD = 64), 4 elements = 2 rotation pairs per lane: 8-byte (bf16) / 16-byte (fp32) accesses, the row
// sums by __shfl_xor inside those lanes, the rotation inside a lane. A block holds kQKThreads / (HD / 4)
// rows at a time and walks the range with the grid's stride; the grid is capped at kQKMaxBlocks.
// The shuffles run in uniform control flow: rows past the end load zeros and store nothing.
constexpr int kQKThreads = 256, kQKMaxBlocks = 2048;

template <int HD>
struct QKRow {
  static constexpr int kLanes = HD / 4, kRows = kQKThreads / kLanes;
  bool live, isq;
  size_t off;   // element offset of this lane's 4 elements inside its own projection
  size_t trig;  // offset of this lane's 2 (cos, sin) entries
  __device__ __forceinline__ QKRow(int64_t row, int lane, int nq, int nk, int S, int Hq, int Hkv) {
    live = row < (int64_t)nq + nk;
    isq = row < nq;
    const int lr = live ? (int)(isq ? row : row - nq) : 0;
    const int s = (lr / (isq ? Hq : Hkv)) % S;  // the projection's own head count
    off = (size_t)lr * HD + 4 * lane;
    trig = (size_t)s * (HD / 2) + 2 * lane;
  }
};

template <int LANES>
__device__ __forceinline__ float qk_row_sum(float v) {
#pragma unroll
  for (int o = LANES / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

template <typename T, int HD>
__global__ __launch_bounds__(kQKThreads) void qk_norm_rope_fwd_kernel(
    const T* __restrict__ q, const T* __restrict__ k, const float* __restrict__ wq, const float* __restrict__ wk,
    const float* __restrict__ cosv, const float* __restrict__ sinv, T* __restrict__ yq, T* __restrict__ yk, int nq,
    int nk, int S, int Hq, int Hkv, float eps) {
  using R = QKRow<HD>;
  const int lane = threadIdx.x % R::kLanes, slot = threadIdx.x / R::kLanes;
  const float4 wqv = ld4(wq + 4 * lane), wkv = ld4(wk + 4 * lane);
  const int64_t total = (int64_t)nq + nk;
  for (int64_t base = (int64_t)blockIdx.x * R::kRows; base < total; base += (int64_t)gridDim.x * R::kRows) {
    const R row(base + slot, lane, nq, nk, S, Hq, Hkv);
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (row.live) v = ld4((row.isq ? q : k) + row.off);
    const float r = rms_rstd(qk_row_sum<R::kLanes>(rms_ss4(v)), HD, eps);
    if (row.live) {
      const float2 c = *reinterpret_cast<const float2*>(cosv + row.trig);
      const float2 sn = *reinterpret_cast<const float2*>(sinv + row.trig);
      const float4 n = rms_scale4(v, r, row.isq ? wqv : wkv);
      st4((row.isq ? yq : yk) + row.off, make_float4(n.x * c.x - n.y * sn.x, n.x * sn.x + n.y * c.x,
                                                     n.z * c.y - n.w * sn.y, n.z * sn.y + n.w * c.y));
    }
  }
}

// gn = R^T g (the rotation with -sin), xh = x r, c = mean(w gn xh), dx = r (w gn - xh c), and the row's
// weight-gradient term t = gn xh; r is recomputed from x. A thread adds the t of its rows, in row
// order, into one q and one k accumulator for its 4 columns; the block's row slots are then added in
// slot order through LDS and the block stores one partial row [q sums | k sums] of 2 * HD floats
// (zeros where it had no row of that kind). colsum4_kernel over the partials gives [dwq | dwk]: no
// atomics, the same bits every run.
template <typename T, int HD>
__global__ __launch_bounds__(kQKThreads) void qk_norm_rope_bwd_kernel(
    const T* __restrict__ q, const T* __restrict__ k, const float* __restrict__ wq, const float* __restrict__ wk,
    const float* __restrict__ cosv, const float* __restrict__ sinv, const T* __restrict__ gq,
    const T* __restrict__ gk, T* __restrict__ dq, T* __restrict__ dk, float* __restrict__ part, int nq, int nk, int S,
    int Hq, int Hkv, float eps) {
  using R = QKRow<HD>;
  __shared__ float4 sh[2][R::kRows][R::kLanes];
  const int lane = threadIdx.x % R::kLanes, slot = threadIdx.x / R::kLanes;
  const float4 wqv = ld4(wq + 4 * lane), wkv = ld4(wk + 4 * lane);
  float4 aq = make_float4(0.f, 0.f, 0.f, 0.f), ak = aq;
  const int64_t total = (int64_t)nq + nk;
  for (int64_t base = (int64_t)blockIdx.x * R::kRows; base < total; base += (int64_t)gridDim.x * R::kRows) {
    const R row(base + slot, lane, nq, nk, S, Hq, Hkv);
    float4 x = make_float4(0.f, 0.f, 0.f, 0.f), gn = x;
    const float4 w = row.isq ? wqv : wkv;
    if (row.live) {
      x = ld4((row.isq ? q : k) + row.off);
      const float4 g = ld4((row.isq ? gq : gk) + row.off);
      const float2 c = *reinterpret_cast<const float2*>(cosv + row.trig);
      const float2 sn = *reinterpret_cast<const float2*>(sinv + row.trig);
      gn = make_float4(g.x * c.x + g.y * sn.x, g.y * c.x - g.x * sn.x, g.z * c.y + g.w * sn.y,
                       g.w * c.y - g.z * sn.y);
    }
    const float ss = qk_row_sum<R::kLanes>(rms_ss4(x));
    const float dot = qk_row_sum<R::kLanes>(rms_dot4(w, gn, x));
    if (row.live) {
      const float r = rms_rstd(ss, HD, eps);
      const float4 xh = make_float4(x.x * r, x.y * r, x.z * r, x.w * r);
      const float c = r * dot / (float)HD;  // mean(w gn xh)
      st4((row.isq ? dq : dk) + row.off,
          make_float4(r * (w.x * gn.x - xh.x * c), r * (w.y * gn.y - xh.y * c), r * (w.z * gn.z - xh.z * c),
                      r * (w.w * gn.w - xh.w * c)));
      const float4 t = make_float4(gn.x * xh.x, gn.y * xh.y, gn.z * xh.z, gn.w * xh.w);
      if (row.isq) {  // a row adds to its own projection's sums only
        aq.x += t.x; aq.y += t.y; aq.z += t.z; aq.w += t.w;
      } else {
        ak.x += t.x; ak.y += t.y; ak.z += t.z; ak.w += t.w;
      }
    }
  }
  sh[0][slot][lane] = aq;
  sh[1][slot][lane] = ak;
  __syncthreads();
  if (threadIdx.x >= 2 * R::kLanes) return;
  // threads [0, kLanes): the q columns, [kLanes, 2 kLanes): the k columns; slots in order
  const int which = threadIdx.x / R::kLanes;
  float4 t = sh[which][0][lane];
  for (int l = 1; l < R::kRows; ++l) {
    const float4 u = sh[which][l][lane];
    t.x += u.x; t.y += u.y; t.z += u.z; t.w += u.w;
  }
  st4(part + (size_t)blockIdx.x * (2 * HD) + which * HD + 4 * lane, t);
}

// ---- softmax cross-entropy over bf16 / fp32 logits [R, V] (V % 8 == 0), mean over rows:
// forward = one read of the logits (online max / sum-exp per row: 8-element vectors, wave
// shuffles, then the 4 waves in order) -> per-row loss and log-sum-exp; backward = one more read
// and one write: dlogits = (softmax - onehot) * g / R, with the upstream scalar g read on device.
// Replaces the fp32 upcast + log_softmax + nll (and their backward) of nn.CrossEntropyLoss.
__device__ __forceinline__ void ms_combine(float& m, float& s, float m2, float s2) {
  if (m2 == -INFINITY) return;
  if (m == -INFINITY) {
    m = m2;
    s = s2;
    return;
  }
  if (m2 > m) {
    s = s * __expf(m - m2) + s2;
    m = m2;
  } else {
    s += s2 * __expf(m2 - m);
  }
}

template <typename T>
__device__ __forceinline__ void ld8(const T* p, float (&v)[8]) {
  const float4 a = ld4(p), b = ld4(p + 4);
  v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}

// log-sum-exp of one row of V logits by the block's 256 threads: valid in thread 0 only
template <typename T>
__device__ __forceinline__ float xent_row_lse(const T* __restrict__ x, int V, float* sm, float* ss) {
  float m = -INFINITY, s = 0.f;
  for (int i = threadIdx.x * 8; i < V; i += 256 * 8) {
    float v[8];
    ld8(x + i, v);
    float vm = v[0];
#pragma unroll
    for (int j = 1; j < 8; ++j) vm = fmaxf(vm, v[j]);
    float vs = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) vs += __expf(v[j] - vm);
    ms_combine(m, s, vm, vs);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float m2 = __shfl_xor(m, off, 64), s2 = __shfl_xor(s, off, 64);
    ms_combine(m, s, m2, s2);
  }
  if ((threadIdx.x & 63) == 0) {
    sm[threadIdx.x >> 6] = m;
    ss[threadIdx.x >> 6] = s;
  }
  __syncthreads();
  if (threadIdx.x != 0) return 0.f;
  m = sm[0];
  s = ss[0];
  for (int w = 1; w < 4; ++w) ms_combine(m, s, sm[w], ss[w]);
  return m + __logf(s);
}

template <typename T>
__global__ __launch_bounds__(256) void xent_fwd_kernel(const T* __restrict__ logits, const int64_t* __restrict__ tgt,
                                                       float* __restrict__ loss, float* __restrict__ lse, int V) {
  __shared__ float sm[4], ss[4];
  const int row = blockIdx.x;
  const T* x = logits + (size_t)row * V;
  const float l = xent_row_lse(x, V, sm, ss);
  if (threadIdx.x != 0) return;
  lse[row] = l;
  const int64_t t = tgt[row];
  loss[row] = (t >= 0 && t < V) ? l - ld(x, (size_t)t) : NAN;  // an out-of-range target poisons the loss
}

template <typename T>
__global__ __launch_bounds__(256) void xent_bwd_kernel(const T* __restrict__ logits, const int64_t* __restrict__ tgt,
                                                       const float* __restrict__ lse, const float* __restrict__ g,
                                                       float inv_n, T* __restrict__ dlogits, int V) {
  const int row = blockIdx.x;
  const T* x = logits + (size_t)row * V;
  T* d = dlogits + (size_t)row * V;
  const float l = lse[row], scale = g[0] * inv_n;
  const int64_t t = tgt[row];
  for (int i = threadIdx.x * 8; i < V; i += 256 * 8) {
    float v[8];
    ld8(x + i, v);
    float4 a, b;
    float o[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = (__expf(v[j] - l) - (i + j == t ? 1.f : 0.f)) * scale;
    a = make_float4(o[0], o[1], o[2], o[3]);
    b = make_float4(o[4], o[5], o[6], o[7]);
    st4(d + i, a);
    st4(d + i + 4, b);
  }
}

// ---- the same with an ignore index and a z-loss (z * lse^2 per row), mean over the rows whose
// target is not the ignore index. A row with the ignore index costs the forward nothing (the block
// leaves before it loads a logit; loss = lse = 0) and the backward one write of zeros. Any other
// target outside [0, V) poisons the loss as above. stats (double[4], written by xent_reduce_kernel):
// {sum of the row losses, n_valid, inv = (float)(1.0 / max(n_valid, 1)), mean = (float)(sum * inv)}
template <typename T>
__global__ __launch_bounds__(256) void xent_fwd_masked_kernel(const T* __restrict__ logits,
                                                              const int64_t* __restrict__ tgt,
                                                              float* __restrict__ loss, float* __restrict__ lse,
                                                              int V, int64_t ignore, float z) {
  __shared__ float sm[4], ss[4];
  const int row = blockIdx.x;
  const int64_t t = tgt[row];
  if (t == ignore) {  // uniform across the block: safe ahead of the barrier in xent_row_lse
    if (threadIdx.x == 0) {
      loss[row] = 0.f;
      lse[row] = 0.f;
    }
    return;
  }
  const T* x = logits + (size_t)row * V;
  const float l = xent_row_lse(x, V, sm, ss);
  if (threadIdx.x != 0) return;
  lse[row] = l;
  if (t < 0 || t >= V) {
    loss[row] = NAN;
    return;
  }
  const float nll = l - ld(x, (size_t)t);
  loss[row] = z != 0.f ? nll + z * l * l : nll;  // z == 0: the bits of xent_fwd_kernel, also for an infinite lse
}

// one block of 1024 threads: thread i sums rows i, i + 1024, ... in ascending order in double, then a
// fixed tree over the threads; no atomics, the same bits every run. Eight rows per trip with the
// loads issued together at clamped (in-bounds) indices: the kernel is a chain of memory latencies,
// not of bandwidth. Rows with an out-of-range target count as valid (their NaN poisons the sum anyway).
constexpr int kRedThreads = 1024, kRedBatch = 8;

__global__ __launch_bounds__(kRedThreads) void xent_reduce_kernel(const float* __restrict__ loss,
                                                                  const int64_t* __restrict__ tgt, int R,
                                                                  int64_t ignore, double* __restrict__ stats) {
#pragma clang fp contract(off)
  __shared__ double rs[kRedThreads];
  __shared__ int rn[kRedThreads];
  double acc = 0.0;
  int n = 0;
  for (int64_t base = threadIdx.x; base < R; base += kRedThreads * kRedBatch) {
    float v[kRedBatch];
    int64_t t[kRedBatch];
#pragma unroll
    for (int k = 0; k < kRedBatch; ++k) {
      const int64_t i = base + (int64_t)k * kRedThreads, j = i < R ? i : R - 1;
      v[k] = loss[j];
      t[k] = i < R ? tgt[j] : ignore;
    }
#pragma unroll
    for (int k = 0; k < kRedBatch; ++k) {
      if (t[k] != ignore) {
        acc += (double)v[k];
        ++n;
      }
    }
  }
  rs[threadIdx.x] = acc;
  rn[threadIdx.x] = n;
  __syncthreads();
#pragma unroll
  for (int s = kRedThreads / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      rs[threadIdx.x] += rs[threadIdx.x + s];
      rn[threadIdx.x] += rn[threadIdx.x + s];
    }
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  const int nv = rn[0];
  const float inv = (float)(1.0 / (double)(nv > 1 ? nv : 1));  // a double division rounded once, as Python's 1.0 / R
  stats[0] = rs[0];
  stats[1] = (double)nv;
  stats[2] = (double)inv;
  stats[3] = (double)(float)(rs[0] * (double)inv);  // no valid row: 0 * 1 = 0, not 0 / 0
}

// ZL = false: the arithmetic of xent_bwd_kernel with inv_n = stats[2] (no multiply by 1)
template <typename T, bool ZL>
__global__ __launch_bounds__(256) void xent_bwd_masked_kernel(const T* __restrict__ logits,
                                                              const int64_t* __restrict__ tgt,
                                                              const float* __restrict__ lse,
                                                              const float* __restrict__ g,
                                                              const double* __restrict__ stats,
                                                              T* __restrict__ dlogits, int V, int64_t ignore,
                                                              float z) {
  const int row = blockIdx.x;
  T* d = dlogits + (size_t)row * V;
  const int64_t t = tgt[row];
  if (t == ignore) {  // dlogits is uninitialised memory: the row is written, its logits are not read
    // 16 bytes per lane whatever T: a write-only block gets nothing else to hide half-filled stores behind
    uint4* dz = reinterpret_cast<uint4*>(d);
    const int nvec = V / (16 / (int)sizeof(T));  // V % 8 == 0 and a 16-byte aligned base: whole vectors
    for (int i = threadIdx.x; i < nvec; i += 256) dz[i] = make_uint4(0u, 0u, 0u, 0u);
    return;
  }
  const T* x = logits + (size_t)row * V;
  const float l = lse[row], scale = g[0] * (float)stats[2];
  const float c = 1.f + 2.f * z * l;  // d(lse + z lse^2) / d lse
  for (int i = threadIdx.x * 8; i < V; i += 256 * 8) {
    float v[8];
    ld8(x + i, v);
    float4 a, b;
    float o[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float p = __expf(v[j] - l);
      if (ZL) p *= c;
      o[j] = (p - (i + j == t ? 1.f : 0.f)) * scale;
    }
    a = make_float4(o[0], o[1], o[2], o[3]);
    b = make_float4(o[4], o[5], o[6], o[7]);
    st4(d + i, a);
    st4(d + i + 4, b);
  }
}

// ---- the chunked LM head (ops/lm.py linear_cross_entropy): forward and backward of one chunk of
// rows in one launch, in place. The chunk's logits [rows, V] become their own gradient
// (softmax * c - onehot) * stats[2], the bits xent_bwd_masked_kernel writes for g = 1; loss / lse are
// the full-length [R] arrays and the chunk's rows are row0 .. row0 + rows - 1 of them (and of tgt),
// written with the arithmetic of xent_fwd_masked_kernel. stats[2] = 1 / max(n_valid, 1) over all R
// rows is there before the first chunk (xent_count_kernel).
// In place: a thread overwrites in pass 2 exactly the 8-vectors it read in pass 1 (the same i), and
// x[t] is taken from the registers of the thread whose vector holds column t before that vector is
// stored; that thread writes the loss. A target outside [0, V) has no such thread: thread 0 writes NaN.
template <typename T, bool ZL>
__global__ __launch_bounds__(256) void xent_fused_kernel(T* logits, const int64_t* __restrict__ tgt,
                                                         float* __restrict__ loss, float* __restrict__ lse,
                                                         const double* __restrict__ stats, int V, int row0,
                                                         int64_t ignore, float z) {
  __shared__ float sm[4], ss[4];
  __shared__ float sl;
  const size_t row = (size_t)row0 + blockIdx.x;
  T* x = logits + (size_t)blockIdx.x * V;
  const int64_t t = tgt[row];
  if (t == ignore) {  // uniform across the block; the row is written, its logits are not read
    uint4* dz = reinterpret_cast<uint4*>(x);
    const int nvec = V / (16 / (int)sizeof(T));
    for (int i = threadIdx.x; i < nvec; i += 256) dz[i] = make_uint4(0u, 0u, 0u, 0u);
    if (threadIdx.x == 0) {
      loss[row] = 0.f;
      lse[row] = 0.f;
    }
    return;
  }
  const float l0 = xent_row_lse(x, V, sm, ss);
  if (threadIdx.x == 0) sl = l0;
  __syncthreads();
  const float l = sl, scale = (float)stats[2];
  const float c = 1.f + 2.f * z * l;  // d(lse + z lse^2) / d lse
  float xt = 0.f;
  bool own = false;
  for (int i = threadIdx.x * 8; i < V; i += 256 * 8) {
    float v[8];
    ld8(x + i, v);
    float4 a, b;
    float o[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const bool hit = i + j == t;
      if (hit) {
        xt = v[j];
        own = true;
      }
      float p = __expf(v[j] - l);
      if (ZL) p *= c;
      o[j] = (p - (hit ? 1.f : 0.f)) * scale;
    }
    a = make_float4(o[0], o[1], o[2], o[3]);
    b = make_float4(o[4], o[5], o[6], o[7]);
    st4(x + i, a);
    st4(x + i + 4, b);
  }
  if (threadIdx.x == 0) lse[row] = l;
  if (own) {
    const float nll = l - xt;
    loss[row] = z != 0.f ? nll + z * l * l : nll;
  } else if (threadIdx.x == 0 && (t < 0 || t >= V)) {
    loss[row] = NAN;
  }
}

// n_valid and its reciprocal over all R targets, ahead of the first chunk: the thread-to-row layout,
// the fixed tree and the rounding of xent_reduce_kernel, so stats[1] and stats[2] are the bits it
// writes after the last chunk. stats[0] and stats[3] (the sum and the mean, not known yet) are set to 0.
__global__ __launch_bounds__(kRedThreads) void xent_count_kernel(const int64_t* __restrict__ tgt, int R,
                                                                 int64_t ignore, double* __restrict__ stats) {
  __shared__ int rn[kRedThreads];
  int n = 0;
  for (int64_t base = threadIdx.x; base < R; base += kRedThreads * kRedBatch) {
    int64_t t[kRedBatch];
#pragma unroll
    for (int k = 0; k < kRedBatch; ++k) {
      const int64_t i = base + (int64_t)k * kRedThreads;
      t[k] = i < R ? tgt[i] : ignore;
    }
#pragma unroll
    for (int k = 0; k < kRedBatch; ++k) n += t[k] != ignore ? 1 : 0;
  }
  rn[threadIdx.x] = n;
  __syncthreads();
#pragma unroll
  for (int s = kRedThreads / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) rn[threadIdx.x] += rn[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  const int nv = rn[0];
  const float inv = (float)(1.0 / (double)(nv > 1 ? nv : 1));
  stats[0] = 0.0;
  stats[1] = (double)nv;
  stats[2] = (double)inv;
  stats[3] = 0.0;
}

bool use4(int D) { return D % 4 == 0 && D / 4 <= 256 * kMaxQ; }

}  // namespace

bool cs_rmsnorm_vec4(int D) { return use4(D); }

int cs_rmsnorm_bwd_partials(int rows, int D) {
  return use4(D) ? (rows + kRows4 - 1) / kRows4 : (rows + kRowsPerBlock - 1) / kRowsPerBlock;
}

#define CS_DT_DISPATCH(dt, ...)                                         \
  do {                                                                  \
    if ((dt) == CS_F32) {                                               \
      using T = float;                                                  \
      __VA_ARGS__;                                                      \
    } else if ((dt) == CS_BF16) {                                       \
      using T = __hip_bfloat16;                                         \
      __VA_ARGS__;                                                      \
    } else {                                                            \
      return hipErrorInvalidValue;                                      \
    }                                                                   \
  } while (0)

#define CS_DT_DISPATCH2(dt, U, ...)                                    \
  do {                                                                  \
    if ((dt) == CS_F32) {                                               \
      using U = float;                                                  \
      __VA_ARGS__;                                                      \
    } else if ((dt) == CS_BF16) {                                       \
      using U = __hip_bfloat16;                                         \
      __VA_ARGS__;                                                      \
    } else {                                                            \
      return hipErrorInvalidValue;                                      \
    }                                                                   \
  } while (0)

hipError_t cs_rmsnorm_fwd(int dt, int wdt, int odt, const void* x, const void* w, void* y, float* rstd, int rows,
                          int D, float eps, hipStream_t s) {
  if (rows <= 0) return hipSuccess;
  if (use4(D)) {
    CS_DT_DISPATCH2(dt, T, CS_DT_DISPATCH2(wdt, Wt, CS_DT_DISPATCH2(odt, O,
        hipLaunchKernelGGL((rmsnorm_fwd4_kernel<T, Wt, O>), dim3(rows), dim3(256), 0, s, (const T*)x, (const Wt*)w,
                           (O*)y, rstd, rows, D, eps))));
    return hipGetLastError();
  }
  if (odt != dt) return hipErrorInvalidValue;  // the scalar path writes the input's dtype
  if (wdt == CS_F32) {
    CS_DT_DISPATCH(dt, hipLaunchKernelGGL((rmsnorm_fwd_kernel<T, float>), dim3(rows), dim3(256), 0, s,
                                          (const T*)x, (const float*)w, (T*)y, rstd, rows, D, eps));
  } else {
    CS_DT_DISPATCH(dt, hipLaunchKernelGGL((rmsnorm_fwd_kernel<T, __hip_bfloat16>), dim3(rows), dim3(256), 0, s,
                                          (const T*)x, (const __hip_bfloat16*)w, (T*)y, rstd, rows, D, eps));
  }
  return hipGetLastError();
}

hipError_t cs_rmsnorm_bwd(int dt, int wdt, int gdt, const void* x, const void* w, const float* rstd, const void* g,
                          void* dx, void* dw, float* part, int rows, int D, hipStream_t s) {
  if (rows <= 0) return hipSuccess;
  const int P = cs_rmsnorm_bwd_partials(rows, D);
  if (use4(D)) {
    CS_DT_DISPATCH2(dt, T, CS_DT_DISPATCH2(wdt, Wt, CS_DT_DISPATCH2(gdt, G,
        hipLaunchKernelGGL((rmsnorm_bwd4_kernel<T, Wt, G>), dim3(P), dim3(256), 0, s, (const T*)x, (const Wt*)w,
                           rstd, (const G*)g, (T*)dx, part, rows, D))));
    CS_DT_DISPATCH2(wdt, Wt, hipLaunchKernelGGL((colsum4_kernel<Wt>), dim3((D / 4 + 15) / 16), dim3(256), 0, s,
                                                part, P, D, (Wt*)dw));
    return hipGetLastError();
  }
  if (gdt != dt) return hipErrorInvalidValue;  // the scalar path reads the gradient in the input's dtype
  if (wdt == CS_F32) {
    CS_DT_DISPATCH(dt, hipLaunchKernelGGL((rmsnorm_bwd_kernel<T, float>), dim3(P), dim3(256), 0, s, (const T*)x,
                                          (const float*)w, rstd, (const T*)g, (T*)dx, part, rows, D));
    hipLaunchKernelGGL((colsum_kernel<float>), dim3((D + 255) / 256), dim3(256), 0, s, part, P, D, (float*)dw);
  } else {
    CS_DT_DISPATCH(dt, hipLaunchKernelGGL((rmsnorm_bwd_kernel<T, __hip_bfloat16>), dim3(P), dim3(256), 0, s,
                                          (const T*)x, (const __hip_bfloat16*)w, rstd, (const T*)g, (T*)dx, part,
                                          rows, D));
    hipLaunchKernelGGL((colsum_kernel<__hip_bfloat16>), dim3((D + 255) / 256), dim3(256), 0, s, part, P, D,
                       (__hip_bfloat16*)dw);
  }
  return hipGetLastError();
}

hipError_t cs_add_rmsnorm_fwd(int dt, int ddt, int wdt, int odt, const void* x, const void* delta, const void* w,
                              void* h, void* y, float* rstd, int rows, int D, float eps, hipStream_t s) {
  if (rows <= 0) return hipSuccess;
  if (D <= 0) return hipErrorInvalidValue;
  if (use4(D)) {
    CS_DT_DISPATCH2(dt, T, CS_DT_DISPATCH2(ddt, Dl, CS_DT_DISPATCH2(wdt, Wt, CS_DT_DISPATCH2(odt, O,
        hipLaunchKernelGGL((add_rmsnorm_fwd4_kernel<T, Dl, Wt, O>), dim3(rows), dim3(256), 0, s, (const T*)x,
                           (const Dl*)delta, (const Wt*)w, (T*)h, (O*)y, rstd, rows, D, eps)))));
    return hipGetLastError();
  }
  if (odt != dt || ddt != dt) return hipErrorInvalidValue;  // the scalar path: one dtype for x, delta, h, y
  CS_DT_DISPATCH2(dt, T, CS_DT_DISPATCH2(wdt, Wt,
      hipLaunchKernelGGL((add_rmsnorm_fwd_kernel<T, Wt>), dim3(rows), dim3(256), 0, s, (const T*)x, (const T*)delta,
                         (const Wt*)w, (T*)h, (T*)y, rstd, rows, D, eps)));
  return hipGetLastError();
}

hipError_t cs_add_rmsnorm_bwd(int dt, int wdt, int gdt, int ddt, const void* h, const void* w, const float* rstd,
                              const void* g, const void* gh, void* dx, void* ddelta, void* dw, float* part, int rows,
                              int D, hipStream_t s) {
  if (rows <= 0) return hipSuccess;
  if (D <= 0) return hipErrorInvalidValue;
  const int P = cs_rmsnorm_bwd_partials(rows, D);
  if (use4(D)) {
    CS_DT_DISPATCH2(dt, T, CS_DT_DISPATCH2(wdt, Wt, CS_DT_DISPATCH2(gdt, G, CS_DT_DISPATCH2(ddt, Dd,
        hipLaunchKernelGGL((add_rmsnorm_bwd4_kernel<T, Wt, G, Dd>), dim3(P), dim3(256), 0, s, (const T*)h,
                           (const Wt*)w, rstd, (const G*)g, (const T*)gh, (T*)dx, (Dd*)ddelta, part, rows, D)))));
    CS_DT_DISPATCH2(wdt, Wt, hipLaunchKernelGGL((colsum4_kernel<Wt>), dim3((D / 4 + 15) / 16), dim3(256), 0, s,
                                                part, P, D, (Wt*)dw));
    return hipGetLastError();
  }
  // the scalar path reads the gradients and writes dx in h's dtype: a second copy has nothing to add
  if (gdt != dt || ddelta != nullptr) return hipErrorInvalidValue;
  CS_DT_DISPATCH2(dt, T, CS_DT_DISPATCH2(wdt, Wt,
      hipLaunchKernelGGL((add_rmsnorm_bwd_kernel<T, Wt>), dim3(P), dim3(256), 0, s, (const T*)h, (const Wt*)w, rstd,
                         (const T*)g, (const T*)gh, (T*)dx, part, rows, D)));
  CS_DT_DISPATCH2(wdt, Wt, hipLaunchKernelGGL((colsum_kernel<Wt>), dim3((D + 255) / 256), dim3(256), 0, s, part, P,
                                              D, (Wt*)dw));
  return hipGetLastError();
}

hipError_t cs_xent_fwd(int dt, const void* logits, const int64_t* tgt, float* loss, float* lse, int R, int V,
                       hipStream_t s) {
  if (R <= 0) return hipSuccess;
  if (V % 8 != 0) return hipErrorInvalidValue;
  CS_DT_DISPATCH(dt, hipLaunchKernelGGL((xent_fwd_kernel<T>), dim3(R), dim3(256), 0, s, (const T*)logits, tgt, loss,
                                        lse, V));
  return hipGetLastError();
}

hipError_t cs_xent_bwd(int dt, const void* logits, const int64_t* tgt, const float* lse, const float* g, float inv_n,
                       void* dlogits, int R, int V, hipStream_t s) {
  if (R <= 0) return hipSuccess;
  if (V % 8 != 0) return hipErrorInvalidValue;
  CS_DT_DISPATCH(dt, hipLaunchKernelGGL((xent_bwd_kernel<T>), dim3(R), dim3(256), 0, s, (const T*)logits, tgt, lse, g,
                                        inv_n, (T*)dlogits, V));
  return hipGetLastError();
}

hipError_t cs_xent_fwd_masked(int dt, const void* logits, const int64_t* tgt, float* loss, float* lse, double* stats,
                              int R, int V, int64_t ignore, float z, hipStream_t s) {
  if (R < 0 || V <= 0 || V % 8 != 0 || !(z >= 0.f) || stats == nullptr) return hipErrorInvalidValue;
  if (R > 0)
    CS_DT_DISPATCH(dt, hipLaunchKernelGGL((xent_fwd_masked_kernel<T>), dim3(R), dim3(256), 0, s, (const T*)logits, tgt,
                                          loss, lse, V, ignore, z));
  hipLaunchKernelGGL(xent_reduce_kernel, dim3(1), dim3(kRedThreads), 0, s, loss, tgt, R, ignore, stats);
  return hipGetLastError();
}

hipError_t cs_xent_bwd_masked(int dt, const void* logits, const int64_t* tgt, const float* lse, const float* g,
                              const double* stats, void* dlogits, int R, int V, int64_t ignore, float z,
                              hipStream_t s) {
  if (R <= 0) return hipSuccess;
  if (V % 8 != 0 || !(z >= 0.f) || stats == nullptr) return hipErrorInvalidValue;
  if (z != 0.f) {
    CS_DT_DISPATCH(dt, hipLaunchKernelGGL((xent_bwd_masked_kernel<T, true>), dim3(R), dim3(256), 0, s,
                                          (const T*)logits, tgt, lse, g, stats, (T*)dlogits, V, ignore, z));
  } else {
    CS_DT_DISPATCH(dt, hipLaunchKernelGGL((xent_bwd_masked_kernel<T, false>), dim3(R), dim3(256), 0, s,
                                          (const T*)logits, tgt, lse, g, stats, (T*)dlogits, V, ignore, z));
  }
  return hipGetLastError();
}

hipError_t cs_xent_count(const int64_t* tgt, int R, int64_t ignore, double* stats, hipStream_t s) {
  if (R < 0 || stats == nullptr) return hipErrorInvalidValue;
  hipLaunchKernelGGL(xent_count_kernel, dim3(1), dim3(kRedThreads), 0, s, tgt, R, ignore, stats);
  return hipGetLastError();
}

hipError_t cs_xent_reduce(const float* loss, const int64_t* tgt, int R, int64_t ignore, double* stats,
                          hipStream_t s) {
  if (R < 0 || stats == nullptr) return hipErrorInvalidValue;
  hipLaunchKernelGGL(xent_reduce_kernel, dim3(1), dim3(kRedThreads), 0, s, loss, tgt, R, ignore, stats);
  return hipGetLastError();
}

hipError_t cs_xent_fused(int dt, void* logits, const int64_t* tgt, float* loss, float* lse, const double* stats,
                         int rows, int V, int R, int row0, int64_t ignore, float z, hipStream_t s) {
  if (rows < 0 || row0 < 0 || (int64_t)row0 + rows > R || V <= 0 || V % 8 != 0 || !(z >= 0.f) || stats == nullptr)
    return hipErrorInvalidValue;
  if (rows == 0) return hipSuccess;
  if (z != 0.f) {
    CS_DT_DISPATCH(dt, hipLaunchKernelGGL((xent_fused_kernel<T, true>), dim3(rows), dim3(256), 0, s, (T*)logits, tgt,
                                          loss, lse, stats, V, row0, ignore, z));
  } else {
    CS_DT_DISPATCH(dt, hipLaunchKernelGGL((xent_fused_kernel<T, false>), dim3(rows), dim3(256), 0, s, (T*)logits, tgt,
                                          loss, lse, stats, V, row0, ignore, z));
  }
  return hipGetLastError();
}

hipError_t cs_swiglu_fwd(int dt, const void* a, const void* b, void* out, size_t n, hipStream_t s) {
  if (n % 4 == 0 && aligned16({a, b, out})) {
    CS_DT_DISPATCH(dt, hipLaunchKernelGGL((swiglu_fwd4_kernel<T>), dim3(grid_for(n / 4)), dim3(256), 0, s,
                                          (const T*)a, (const T*)b, (T*)out, n / 4));
    return hipGetLastError();
  }
  CS_DT_DISPATCH(dt, hipLaunchKernelGGL((swiglu_fwd_kernel<T>), dim3(grid_for(n)), dim3(256), 0, s, (const T*)a,
                                        (const T*)b, (T*)out, n));
  return hipGetLastError();
}

hipError_t cs_swiglu_bwd(int dt, const void* a, const void* b, const void* g, void* da, void* db, size_t n,
                         hipStream_t s) {
  if (n % 4 == 0 && aligned16({a, b, g, da, db})) {
    CS_DT_DISPATCH(dt, hipLaunchKernelGGL((swiglu_bwd4_kernel<T>), dim3(grid_for(n / 4)), dim3(256), 0, s,
                                          (const T*)a, (const T*)b, (const T*)g, (T*)da, (T*)db, n / 4));
    return hipGetLastError();
  }
  CS_DT_DISPATCH(dt, hipLaunchKernelGGL((swiglu_bwd_kernel<T>), dim3(grid_for(n)), dim3(256), 0, s, (const T*)a,
                                        (const T*)b, (const T*)g, (T*)da, (T*)db, n));
  return hipGetLastError();
}

hipError_t cs_rope(int dt, const void* x, const float* cosv, const float* sinv, void* out, int B, int S, int H, int hd,
                   int inverse, hipStream_t s) {
  if (hd & 1) return hipErrorInvalidValue;
  const size_t npairs = (size_t)B * S * H * (hd / 2);
  if (npairs == 0) return hipSuccess;
  CS_DT_DISPATCH(dt, hipLaunchKernelGGL((rope_kernel<T>), dim3(grid_for(npairs)), dim3(256), 0, s, (const T*)x, cosv,
                                        sinv, (T*)out, S, H, hd, npairs, inverse ? -1.f : 1.f));
  return hipGetLastError();
}

int cs_qk_norm_rope_rows_per_block(int hd) { return hd == 64 || hd == 128 ? kQKThreads / (hd / 4) : 0; }

int cs_qk_norm_rope_max_blocks() { return kQKMaxBlocks; }

int cs_qk_norm_rope_partials(int64_t rows, int hd) {
  const int rpb = cs_qk_norm_rope_rows_per_block(hd);
  if (rpb == 0 || rows <= 0) return 0;
  const int64_t b = (rows + rpb - 1) / rpb;
  return (int)(b > kQKMaxBlocks ? kQKMaxBlocks : b);
}

namespace {

// the host-side range checks of both launchers; rows = B * S * (Hq + Hkv) must fit an int
bool qk_args_ok(int dt, int B, int S, int Hq, int Hkv, int hd) {
  if (dt != CS_F32 && dt != CS_BF16) return false;
  if (hd != 64 && hd != 128) return false;
  if (B <= 0 || S <= 0 || Hq <= 0 || Hkv <= 0) return false;
  return (int64_t)B * S * ((int64_t)Hq + Hkv) <= 0x7fffffff;
}

bool qk_ptrs_ok(std::initializer_list<const void*> ps) {
  for (const void* p : ps)
    if (p == nullptr) return false;
  return aligned16(ps);
}

}  // namespace

#define CS_QK_DISPATCH(dt, hd, ...)                                     \
  CS_DT_DISPATCH(dt, if ((hd) == 64) {                                  \
    constexpr int HD = 64;                                              \
    __VA_ARGS__;                                                        \
  } else {                                                              \
    constexpr int HD = 128;                                             \
    __VA_ARGS__;                                                        \
  })

hipError_t cs_qk_norm_rope_fwd(int dt, const void* q, const void* k, const float* wq, const float* wk,
                               const float* cosv, const float* sinv, void* yq, void* yk, int B, int S, int Hq, int Hkv,
                               int hd, float eps, hipStream_t s) {
  if (B == 0 || S == 0) return hipSuccess;
  if (!qk_args_ok(dt, B, S, Hq, Hkv, hd) || !qk_ptrs_ok({q, k, wq, wk, cosv, sinv, yq, yk}))
    return hipErrorInvalidValue;
  const int nq = B * S * Hq, nk = B * S * Hkv;
  const int grid = cs_qk_norm_rope_partials((int64_t)nq + nk, hd);
  CS_QK_DISPATCH(dt, hd, hipLaunchKernelGGL((qk_norm_rope_fwd_kernel<T, HD>), dim3(grid), dim3(kQKThreads), 0, s,
                                            (const T*)q, (const T*)k, wq, wk, cosv, sinv, (T*)yq, (T*)yk, nq, nk, S,
                                            Hq, Hkv, eps));
  return hipGetLastError();
}

hipError_t cs_qk_norm_rope_bwd(int dt, const void* q, const void* k, const float* wq, const float* wk,
                               const float* cosv, const float* sinv, const void* gq, const void* gk, void* dq,
                               void* dk, float* dw, float* part, int B, int S, int Hq, int Hkv, int hd, float eps,
                               hipStream_t s) {
  if (B == 0 || S == 0) return hipSuccess;
  if (!qk_args_ok(dt, B, S, Hq, Hkv, hd) || !qk_ptrs_ok({q, k, wq, wk, cosv, sinv, gq, gk, dq, dk, dw, part}))
    return hipErrorInvalidValue;
  const int nq = B * S * Hq, nk = B * S * Hkv;
  const int P = cs_qk_norm_rope_partials((int64_t)nq + nk, hd);
  CS_QK_DISPATCH(dt, hd, hipLaunchKernelGGL((qk_norm_rope_bwd_kernel<T, HD>), dim3(P), dim3(kQKThreads), 0, s,
                                            (const T*)q, (const T*)k, wq, wk, cosv, sinv, (const T*)gq, (const T*)gk,
                                            (T*)dq, (T*)dk, part, nq, nk, S, Hq, Hkv, eps));
  hipLaunchKernelGGL((colsum4_kernel<float>), dim3((2 * hd / 4 + 15) / 16), dim3(256), 0, s, part, P, 2 * hd, dw);
  return hipGetLastError();
}
