// Fused AdamW with global-norm gradient clipping: one norm launch over every parameter of the
// model and one update launch per parameter group (reference rule: torch.optim.AdamW, decoupled
// weight decay; clip coefficient: torch.nn.utils.clip_grad_norm_).
//
//   g' = g * grad_scale * coef                    coef = min(1, max_norm / (norm + 1e-6)), or 1
//   p  = p * (1 - lr*wd)
//   m  = m + (1-b1) * (g' - m)
//   v  = b2*v + (1-b2) * g'*g'
//   p  = p - (lr/bc1) * m / (sqrt(v)/sqrt(bc2) + eps)
//
// Both kernels walk the CsAdamEntry table in 4096-element chunks (chunk starts as a prefix array,
// a chunk's tensor by binary search: sgd_multi_kernel's scheme), up to 2048 blocks of 256 threads,
// block b taking chunks b, b + grid, ... The pass is memory traffic only (16 B read + 12 B written
// per element, + 2 B for a bf16 shadow, + 4 B read by the norm pass): float4 accesses where the
// entry's pointers allow them, a scalar loop otherwise, and sgd.hip's plain loop shape (its header:
// more loads in flight bought nothing for this kind of pass).
//
// The norm is deterministic: no atomics; a block sums its chunks in a fixed order and a fixed LDS
// tree, in double, into partials[b]; every block of the update re-reduces the 2048 partials in one
// fixed order (16 KB from L2). Nothing is read back to the host.
#include "common.h"
#include "launchers.h"

namespace {

struct AdamArgs {
  float decay, b1, b2, omb1, omb2, eps, step_size, bc2_sqrt, scale, max_norm;
};

// Every rounding is spelled out (explicit fma, contraction off), as in sgd_device.h: the vector and
// the scalar loop, and any launch shape, give the same bits for the same inputs.
__device__ __forceinline__ void adam1(float& p, float g, float& m, float& v, const AdamArgs& a, float coef) {
#pragma clang fp contract(off)
  g = g * a.scale;
  g = g * coef;
  p = p * a.decay;                                   // param.mul_(1 - lr*wd)
  m = __builtin_fmaf(a.omb1, g - m, m);              // exp_avg.lerp_(grad, 1 - beta1)
  v = __builtin_fmaf(a.omb2, g * g, v * a.b2);       // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
  const float denom = sqrtf(v) / a.bc2_sqrt + a.eps;
  p = __builtin_fmaf(-a.step_size, m / denom, p);    // param.addcdiv_(exp_avg, denom, value=-step_size)
}

// round-to-nearest-even bf16 of x (NaN kept quiet): the sgd_multi_kernel shadow column's code
__device__ __forceinline__ uint16_t bf16_rne(float x) {
  const uint32_t u = __float_as_uint(x);
  return (x != x) ? (uint16_t)((u >> 16) | 0x40u) : (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

__device__ __forceinline__ int tensor_of_chunk(const int64_t* __restrict__ chunk_start, int ntens, int c) {
  int lo = 0, hi = ntens - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (chunk_start[mid] <= c) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// sum over the block in a fixed tree; the result is valid in thread 0 (and in every thread after
// the closing barrier through red[0])
__device__ __forceinline__ double block_sum(double x, double* red) {
  red[threadIdx.x] = x;
  __syncthreads();
#pragma unroll
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}

__global__ __launch_bounds__(256) void cs_grad_sumsq_kernel(const CsAdamEntry* __restrict__ tab, int ntens,
                                                            const int64_t* __restrict__ chunk_start, int nchunks,
                                                            float scale, double* __restrict__ partials) {
#pragma clang fp contract(off)
  __shared__ double red[256];
  double acc = 0.0;
  for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const int t = tensor_of_chunk(chunk_start, ntens, c);
    const CsAdamEntry e = tab[t];
    const int64_t base = (int64_t)(c - chunk_start[t]) * 4096;
    if (base < 0 || base >= e.n) continue;  // a chunk outside this run of the table: nothing to do
    const int64_t end = base + 4096 < e.n ? base + 4096 : e.n;
    int64_t tail = base;
    if (e.flags & CS_ADAM_VEC_G) {
      const int64_t n4 = (end - base) >> 2;
      const float4* g4 = reinterpret_cast<const float4*>(e.g + base);
      for (int64_t i = threadIdx.x; i < n4; i += 256) {
        const float4 gv = g4[i];
        const double x = (double)(gv.x * scale), y = (double)(gv.y * scale), z = (double)(gv.z * scale),
                     w = (double)(gv.w * scale);
        acc += x * x;
        acc += y * y;
        acc += z * z;
        acc += w * w;
      }
      tail = base + (n4 << 2);
    }
    for (int64_t i = tail + threadIdx.x; i < end; i += 256) {
      const double x = (double)(e.g[i] * scale);
      acc += x * x;
    }
  }
  const double s = block_sum(acc, red);
  if (threadIdx.x == 0) partials[blockIdx.x] = s;
  // the slots past the grid: zero, so the consumer always sums CS_ADAM_PARTIALS values
  if (blockIdx.x == 0)
    for (int i = gridDim.x + threadIdx.x; i < CS_ADAM_PARTIALS; i += 256) partials[i] = 0.0;
}

__global__ __launch_bounds__(256) void cs_adamw_multi_kernel(const CsAdamEntry* __restrict__ tab, int ntens,
                                                             const int64_t* __restrict__ chunk_start, int first_chunk,
                                                             int nchunks, AdamArgs a,
                                                             const double* __restrict__ partials,
                                                             float* __restrict__ norm_out) {
  float coef = 1.f;
  if (partials != nullptr) {
#pragma clang fp contract(off)
    __shared__ double red[256];
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < CS_ADAM_PARTIALS / 256; ++k) acc += partials[k * 256 + threadIdx.x];
    const float norm = (float)sqrt(block_sum(acc, red));
    // torch's clip_grad_norm_: clamp(max_norm / (norm + 1e-6), max=1.0); a NaN norm stays NaN
    const float c = a.max_norm / (norm + 1e-6f);
    coef = c > 1.f ? 1.f : c;
    if (blockIdx.x == 0 && threadIdx.x == 0) *norm_out = norm;
  }
  for (int cc = blockIdx.x; cc < nchunks; cc += gridDim.x) {
    const int c = first_chunk + cc;
    const int t = tensor_of_chunk(chunk_start, ntens, c);
    const CsAdamEntry e = tab[t];
    const int64_t base = (int64_t)(c - chunk_start[t]) * 4096;
    if (base < 0 || base >= e.n) continue;  // a chunk outside this run of the table: nothing to do
    const int64_t end = base + 4096 < e.n ? base + 4096 : e.n;
    int64_t tail = base;
    if (e.flags & CS_ADAM_VEC) {
      const int64_t n4 = (end - base) >> 2;
      float4* p4 = reinterpret_cast<float4*>(e.p + base);
      const float4* g4 = reinterpret_cast<const float4*>(e.g + base);
      float4* m4 = reinterpret_cast<float4*>(e.m + base);
      float4* v4 = reinterpret_cast<float4*>(e.v + base);
      uint2* s4 = e.shadow != nullptr ? reinterpret_cast<uint2*>(e.shadow + base) : nullptr;
      for (int64_t i = threadIdx.x; i < n4; i += 256) {
        float4 pv = p4[i], mv = m4[i], vv = v4[i];
        const float4 gv = g4[i];
        adam1(pv.x, gv.x, mv.x, vv.x, a, coef);
        adam1(pv.y, gv.y, mv.y, vv.y, a, coef);
        adam1(pv.z, gv.z, mv.z, vv.z, a, coef);
        adam1(pv.w, gv.w, mv.w, vv.w, a, coef);
        p4[i] = pv;
        m4[i] = mv;
        v4[i] = vv;
        if (s4 != nullptr)
          s4[i] = make_uint2((uint32_t)bf16_rne(pv.x) | ((uint32_t)bf16_rne(pv.y) << 16),
                             (uint32_t)bf16_rne(pv.z) | ((uint32_t)bf16_rne(pv.w) << 16));
      }
      tail = base + (n4 << 2);
    }
    for (int64_t i = tail + threadIdx.x; i < end; i += 256) {
      float pv = e.p[i], mv = e.m[i], vv = e.v[i];
      adam1(pv, e.g[i], mv, vv, a, coef);
      e.p[i] = pv;
      e.m[i] = mv;
      e.v[i] = vv;
      if (e.shadow != nullptr) e.shadow[i] = bf16_rne(pv);
    }
  }
}

}  // namespace

hipError_t cs_grad_sumsq(const CsAdamEntry* tab_dev, int ntens, const int64_t* chunk_start_dev, int nchunks,
                         float grad_scale, double* partials, hipStream_t stream) {
  if (ntens <= 0 || nchunks <= 0) return hipErrorInvalidValue;
  const int blocks = nchunks < CS_ADAM_PARTIALS ? nchunks : CS_ADAM_PARTIALS;
  hipLaunchKernelGGL(cs_grad_sumsq_kernel, dim3(blocks), dim3(256), 0, stream, tab_dev, ntens, chunk_start_dev,
                     nchunks, grad_scale, partials);
  return hipGetLastError();
}

hipError_t cs_adamw_multi(const CsAdamEntry* tab_dev, int ntens, const int64_t* chunk_start_dev, int first_chunk,
                          int nchunks, double lr, double beta1, double beta2, double eps, double wd, double bc1,
                          double bc2, float grad_scale, float max_norm, const double* partials, float* norm_out,
                          hipStream_t stream) {
  if (ntens <= 0 || nchunks <= 0) return hipSuccess;
  if (partials != nullptr && norm_out == nullptr) return hipErrorInvalidValue;
  // the scalars torch forms in Python doubles and rounds once to float: 1 - lr*wd, 1 - beta, lr/bc1, sqrt(bc2)
  AdamArgs a{(float)(1.0 - lr * wd), (float)beta1, (float)beta2, (float)(1.0 - beta1), (float)(1.0 - beta2),
             (float)eps,             (float)(lr / bc1), (float)sqrt(bc2), grad_scale, max_norm};
  const int blocks = nchunks < 2048 ? nchunks : 2048;
  hipLaunchKernelGGL(cs_adamw_multi_kernel, dim3(blocks), dim3(256), 0, stream, tab_dev, ntens, chunk_start_dev,
                     first_chunk, nchunks, a, partials, norm_out);
  return hipGetLastError();
}
