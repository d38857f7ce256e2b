// Fused token sampler for gfx950: temperature, top-k, min-p, top-p and the inverse-CDF draw of one token per row
// of logits [B, V] (fp32, bf16 or fp16, unit inner stride) in one launch, one workgroup of 1024 threads per row.
// The contract is docs/sampling.md; in short, with s_i = float(z_i) / T in fp32 and smax their maximum:
//   top-k  keeps s_i >= the k-th largest value (ties kept), exact on the fp32 values;
//   min-p  keeps exp(s_i - smax) >= min_p;
//   top-p  keeps s_i >= t*, the largest kept value whose upper set holds top_p of the kept mass (ties kept);
//   draw   the smallest kept i whose running mass in vocabulary order reaches u * W_kept.
//
// Nothing is sorted and no floating-point value is ever added atomically. s maps to a 32-bit key that orders
// like the floats; a weight w = exp(s - smax) in (0, 1] becomes the integer max(1, trunc(w * 2^shift)), shift =
// min(44, 62 - bits(V)), so the mass of a whole row fits 63 bits, and every sum (LDS histogram atomics, register
// partials, block scans) is an integer sum: the same bits in whatever order the adds arrive. One radix descent
// (12 + 10 + 10 key bits, histograms of 64-bit integers in LDS, a block suffix scan that finds the bin where the
// running total from the top reaches the target) serves top-k, with 1 per element and target k, and top-p, with
// the mass per kept element and target ceil(top_p * W). The row does not fit LDS (128256 fp32 = 513 KB) and is
// re-read on each pass, from L2 after the first: 1 pass for the maximum, 3 per active descent, 1 for the kept
// count and mass, 1 (ending at the token) for the draw. Loads are 16-byte vectors from the first 16-byte boundary
// of the row; the at most 7 elements before it and after the last whole vector are scalar loads.
//
// T == 0: the lowest index of the maximum, kept = 1. A row with a NaN, without a finite s, or with s = +inf gets
// the lowest index of its maximum over the non-NaN values as well (NaN counts as -inf): always inside [0, V).
// Per-row settings are clamped on the device: T to >= 0 (NaN: 0), k to >= 1, top_p and min_p to [0, 1].
#include <climits>

#include "common.h"
#include "launchers.h"

namespace {

typedef unsigned long long u64;
constexpr int NT = 1024, NW = NT / 64;
constexpr int BINS1 = 4096, BINS2 = 1024;  // key bits 31..20, then 19..10, then 9..0

struct SampleArgs {
  const void* logits;
  long long row_stride;  // elements
  const float* u;
  const float *temp, *topp, *minp;  // [B] or null: the scalar below
  const int* topk;
  float temp_s, topp_s, minp_s;
  int topk_s;  // 0: no top-k
  unsigned char* finished;  // [B] or null
  long long eos;
  long long* tokens;
  int* kept;
  int V, shift;
};

template <int DT> struct Row;
template <> struct Row<CS_F32> {
  using E = float;
  static constexpr int VEC = 4;
  static __device__ __forceinline__ float f(E e) { return e; }
  static __device__ __forceinline__ float at(const unsigned (&w)[4], int i) { return __uint_as_float(w[i]); }
};
template <> struct Row<CS_BF16> {
  using E = unsigned short;
  static constexpr int VEC = 8;
  static __device__ __forceinline__ float f(E e) { return __uint_as_float((unsigned)e << 16); }
  static __device__ __forceinline__ float at(const unsigned (&w)[4], int i) {
    return __uint_as_float((i & 1) ? (w[i >> 1] & 0xffff0000u) : (w[i >> 1] << 16));
  }
};
template <> struct Row<CS_F16> {
  using E = unsigned short;
  static constexpr int VEC = 8;
  static __device__ __forceinline__ float f(E e) { return (float)__builtin_bit_cast(_Float16, e); }
  static __device__ __forceinline__ float at(const unsigned (&w)[4], int i) {
    return f((E)((i & 1) ? (w[i >> 1] >> 16) : (w[i >> 1] & 0xffffu)));
  }
};

// where a row's 16-byte vectors start and how many there are: indices [0, head) and [head + nvec * VEC, V) are
// scalar, vector j holds indices head + j * VEC ...
struct Span {
  int head, nvec;
};

// f(index, logit) for every element of the row, each exactly once; a thread's indices ascend
template <int DT, class F>
__device__ __forceinline__ void for_each(const typename Row<DT>::E* row, int V, Span sp, F&& f) {
  using R = Row<DT>;
  const int tid = threadIdx.x;
  if (tid < sp.head) f(tid, R::f(row[tid]));
  const uint4* vp = reinterpret_cast<const uint4*>(row + sp.head);
  for (int j = tid; j < sp.nvec; j += NT) {
    const uint4 q = vp[j];
    const unsigned w[4] = {q.x, q.y, q.z, q.w};
    const int base = sp.head + j * R::VEC;
#pragma unroll
    for (int i = 0; i < R::VEC; ++i) f(base + i, R::at(w, i));
  }
  const int t0 = sp.head + sp.nvec * R::VEC;
  if (t0 + tid < V) f(t0 + tid, R::f(row[t0 + tid]));
}

// s as every pass sees it: a NaN counts as -inf, -0 as +0 (one key per value)
__device__ __forceinline__ float clean(float s) { return s != s ? -INFINITY : s + 0.0f; }

// order-preserving map of a non-NaN float to 32 bits
__device__ __forceinline__ unsigned key_of(float s) {
  const unsigned b = __float_as_uint(s);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__device__ __forceinline__ u64 wave_sum_u64(u64 v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// sum over the block, in every thread; red: NW values
__device__ __forceinline__ u64 block_sum_u64(u64 v, u64* red) {
  v = wave_sum_u64(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  u64 r = 0;
#pragma unroll
  for (int w = 0; w < NW; ++w) r += red[w];
  __syncthreads();
  return r;
}

__device__ __forceinline__ int block_max_int(int v, int* red) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = max(v, __shfl_xor(v, off, 64));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  int r = red[0];
#pragma unroll
  for (int w = 1; w < NW; ++w) r = max(r, red[w]);
  __syncthreads();
  return r;
}

// exclusive prefix of v over the block in thread order, and the block's total; red: NW values
__device__ __forceinline__ u64 block_scan_u64(u64 v, u64* red, u64& total) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  u64 inc = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const u64 o = __shfl_up(inc, off, 64);
    if (lane >= off) inc += o;
  }
  if (lane == 63) red[wid] = inc;
  __syncthreads();
  u64 base = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < NW; ++w) {
    const u64 r = red[w];
    if (w < wid) base += r;
    tot += r;
  }
  __syncthreads();
  total = tot;
  return base + inc - v;
}

struct Lds {
  u64 hist[BINS1];
  u64 red[NW];
  u64 res[2];
  float redv[NW];
  int redi[NW];
  int redn[NW];
  int tok;
};

// The bin, counted from the top, at which the running total of hist[nbins] reaches target (>= 1), and the total
// of the bins above it. A target beyond the sum of all bins gives bin 0. PER = nbins / NT bins per thread.
template <int PER>
__device__ __forceinline__ void find_bin(Lds& L, u64 target, int& bin, u64& above) {
  constexpr int nbins = PER * NT;
  const int tid = threadIdx.x;
  u64 v[PER], loc = 0;
#pragma unroll
  for (int e = 0; e < PER; ++e) {
    v[e] = L.hist[nbins - 1 - (tid * PER + e)];
    loc += v[e];
  }
  if (tid == 0) {
    L.res[0] = 0;
    L.res[1] = 0;
  }
  u64 total;
  u64 excl = block_scan_u64(loc, L.red, total);  // its first barrier orders the defaults before the hit
  if (excl < target && target <= excl + loc) {
#pragma unroll
    for (int e = 0; e < PER; ++e) {
      if (target <= excl + v[e]) {
        L.res[0] = (u64)(nbins - 1 - (tid * PER + e));
        L.res[1] = excl;
        break;
      }
      excl += v[e];
    }
  }
  __syncthreads();
  bin = (int)L.res[0];
  above = L.res[1];
  __syncthreads();
}

__device__ __forceinline__ u64 frac_target(double frac, u64 total) {
  const double t = ceil(frac * (double)total);
  u64 r = t >= 9.2e18 ? total : (u64)t;
  if (r > total) r = total;
  return r < 1 ? 1 : r;
}

// Radix descent. val(s, key): an element's non-negative integer weight, 0 for one that does not take part.
// Returns the largest key t among the takers for which the weight of {key >= t} reaches the target: `target`
// itself when frac < 0, otherwise ceil(frac * the takers' total weight), at least 1.
template <int DT, class Val>
__device__ __forceinline__ unsigned descend(Lds& L, const typename Row<DT>::E* row, int V, Span sp, float T, Val&& val,
                                            u64 target, double frac) {
  const int tid = threadIdx.x;
  for (int i = tid; i < BINS1; i += NT) L.hist[i] = 0;
  __syncthreads();
  for_each<DT>(row, V, sp, [&](int, float z) {
    const float s = clean(__fdiv_rn(z, T));
    const unsigned key = key_of(s);
    const u64 m = val(s, key);
    if (m) atomicAdd(&L.hist[key >> 20], m);
  });
  __syncthreads();
  if (frac >= 0.0) {
    u64 loc = 0;
    for (int i = tid; i < BINS1; i += NT) loc += L.hist[i];
    target = frac_target(frac, block_sum_u64(loc, L.red));
  }
  int bin;
  u64 above;
  find_bin<BINS1 / NT>(L, target, bin, above);
  target -= above;
  unsigned prefix = (unsigned)bin;  // key >> 20

  L.hist[tid] = 0;  // BINS2 == NT
  __syncthreads();
  for_each<DT>(row, V, sp, [&](int, float z) {
    const float s = clean(__fdiv_rn(z, T));
    const unsigned key = key_of(s);
    if ((key >> 20) == prefix) {
      const u64 m = val(s, key);
      if (m) atomicAdd(&L.hist[(key >> 10) & 1023u], m);
    }
  });
  __syncthreads();
  find_bin<1>(L, target, bin, above);
  target -= above;
  prefix = (prefix << 10) | (unsigned)bin;  // key >> 10

  L.hist[tid] = 0;
  __syncthreads();
  for_each<DT>(row, V, sp, [&](int, float z) {
    const float s = clean(__fdiv_rn(z, T));
    const unsigned key = key_of(s);
    if ((key >> 10) == prefix) {
      const u64 m = val(s, key);
      if (m) atomicAdd(&L.hist[key & 1023u], m);
    }
  });
  __syncthreads();
  find_bin<1>(L, target, bin, above);
  return (prefix << 10) | (unsigned)bin;
}

static_assert(BINS2 == NT, "the lower levels clear and scan one bin per thread");

template <int DT>
__global__ __launch_bounds__(NT) void sample_kernel(const SampleArgs a) {
  using R = Row<DT>;
  using E = typename R::E;
  constexpr int VEC = R::VEC;
  __shared__ Lds L;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int V = a.V;

  // every thread reads the flag before the first barrier; thread 0 alone writes it, after the last one
  if (a.finished != nullptr && a.finished[b] != 0) {
    if (tid == 0) {
      a.tokens[b] = a.eos;
      a.kept[b] = 0;
    }
    return;
  }
  auto finish = [&](int tok, int kept) {
    if (tid == 0) {
      tok = min(max(tok, 0), V - 1);
      a.tokens[b] = tok;
      a.kept[b] = kept;
      if (a.finished != nullptr && (long long)tok == a.eos) a.finished[b] = 1;
    }
  };

  const E* row = static_cast<const E*>(a.logits) + (size_t)b * a.row_stride;
  Span sp;
  {
    const unsigned mis = (unsigned)(reinterpret_cast<uintptr_t>(row) & 15u) / (unsigned)sizeof(E);
    sp.head = mis ? min(V, (int)(16u / sizeof(E) - mis)) : 0;
    sp.nvec = (V - sp.head) / VEC;
  }

  float T = a.temp != nullptr ? a.temp[b] : a.temp_s;
  T = fmaxf(T, 0.f);  // NaN -> 0
  const int k = a.topk != nullptr ? max(a.topk[b], 1) : a.topk_s;
  const float p = fminf(fmaxf(a.topp != nullptr ? a.topp[b] : a.topp_s, 0.f), 1.f);
  const float mp = fminf(fmaxf(a.minp != nullptr ? a.minp[b] : a.minp_s, 0.f), 1.f);
  const bool greedy = T == 0.f;

  // pass 1: the maximum of s (of z when greedy), its lowest index, whether a NaN was seen
  float bv = -INFINITY;
  int bi = INT_MAX, nan = 0;
  for_each<DT>(row, V, sp, [&](int i, float z) {
    nan |= (z != z);
    const float s = clean(greedy ? z : __fdiv_rn(z, T));
    if (s > bv || (s == bv && i < bi)) {
      bv = s;
      bi = i;
    }
  });
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float ov = __shfl_xor(bv, off, 64);
    const int oi = __shfl_xor(bi, off, 64);
    nan |= __shfl_xor(nan, off, 64);
    if (ov > bv || (ov == bv && oi < bi)) {
      bv = ov;
      bi = oi;
    }
  }
  if (lane == 0) {
    L.redv[wid] = bv;
    L.redi[wid] = bi;
    L.redn[wid] = nan;
  }
  __syncthreads();
  bv = L.redv[0];
  bi = L.redi[0];
  nan = L.redn[0];
#pragma unroll
  for (int w = 1; w < NW; ++w) {
    const float ov = L.redv[w];
    const int oi = L.redi[w];
    nan |= L.redn[w];
    if (ov > bv || (ov == bv && oi < bi)) {
      bv = ov;
      bi = oi;
    }
  }
  if (greedy || nan || !(bv > -INFINITY) || bv == INFINITY) {
    finish(bi, 1);
    return;
  }
  const float smax = bv;
  const float scale = __uint_as_float((unsigned)(127 + a.shift) << 23);

  // top-k: the key of the k-th largest value, counting every element of the row
  unsigned klo = 0;
  if (k < V)
    klo = descend<DT>(L, row, V, sp, T, [](float, unsigned) -> u64 { return 1; }, (u64)k, -1.0);

  // the integer mass of an element that passed top-k and min-p; 0 for one that did not
  auto mass = [&](float s, unsigned key) -> u64 {
    if (!(s > -INFINITY) || key < klo) return 0;
    const float w = expf(s - smax);
    if (w < mp) return 0;
    const u64 m = __float2ull_rz(w * scale);
    return m ? m : 1;
  };

  unsigned tkey = klo;
  if (p < 1.f) tkey = descend<DT>(L, row, V, sp, T, mass, 0, (double)p);

  // the kept set: its size, its mass, its highest index
  u64 wl = 0, cl = 0;
  int hl = -1;
  for_each<DT>(row, V, sp, [&](int i, float z) {
    const float s = clean(__fdiv_rn(z, T));
    const unsigned key = key_of(s);
    if (key >= tkey) {
      const u64 m = mass(s, key);
      if (m) {
        wl += m;
        cl += 1;
        hl = i;  // a thread's indices ascend
      }
    }
  });
  const u64 W = block_sum_u64(wl, L.red);
  const int kept = (int)block_sum_u64(cl, L.red);
  const int hi = block_max_int(hl, L.redi);
  if (kept == 0) {  // not reachable: the maximum passes every filter
    finish(bi, 1);
    return;
  }

  // the draw: tiles of NT threads in index order, each thread's elements adjacent
  const u64 target = frac_target((double)a.u[b], W);
  if (tid == 0) L.tok = -1;
  u64 carry = 0;
  // one tile: thread t holds n adjacent elements from index base with masses m[]; true once the token is known
  auto tile = [&](const u64 (&m)[VEC], int n, int base) -> bool {
    u64 loc = 0;
#pragma unroll
    for (int e = 0; e < VEC; ++e) loc += e < n ? m[e] : 0;
    u64 total;
    u64 excl = carry + block_scan_u64(loc, L.red, total);
    if (excl < target && target <= excl + loc) {
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        if (e < n) {
          if (target <= excl + m[e]) {
            L.tok = base + e;
            break;
          }
          excl += m[e];
        }
      }
    }
    carry += total;
    __syncthreads();
    return L.tok >= 0;
  };
  auto mass_at = [&](float z) -> u64 {
    const float s = clean(__fdiv_rn(z, T));
    const unsigned key = key_of(s);
    return key >= tkey ? mass(s, key) : 0;
  };
  bool done = false;
  if (sp.head > 0) {
    u64 m[VEC] = {};
    if (tid < sp.head) m[0] = mass_at(R::f(row[tid]));
    done = tile(m, tid < sp.head ? 1 : 0, tid);
  }
  const uint4* vp = reinterpret_cast<const uint4*>(row + sp.head);
  for (int j0 = 0; j0 < sp.nvec && !done; j0 += NT) {
    const int j = j0 + tid;
    u64 m[VEC] = {};
    if (j < sp.nvec) {
      const uint4 q = vp[j];
      const unsigned w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
      for (int e = 0; e < VEC; ++e) m[e] = mass_at(R::at(w, e));
    }
    done = tile(m, j < sp.nvec ? VEC : 0, sp.head + j * VEC);
  }
  const int t0 = sp.head + sp.nvec * VEC;
  if (!done && t0 < V) {
    u64 m[VEC] = {};
    if (t0 + tid < V) m[0] = mass_at(R::f(row[t0 + tid]));
    done = tile(m, t0 + tid < V ? 1 : 0, t0 + tid);
  }
  // target <= W and the sums are exact, so the token is always found; the highest kept index otherwise
  finish(done ? L.tok : hi, kept);
}

template <int DT>
hipError_t launch(const SampleArgs& a, int B, hipStream_t st) {
  hipLaunchKernelGGL((sample_kernel<DT>), dim3((unsigned)B), dim3(NT), 0, st, a);
  return hipGetLastError();
}

bool aligned(const void* p, uintptr_t n) { return reinterpret_cast<uintptr_t>(p) % n == 0; }

}  // namespace

hipError_t cs_sample_logits(int dt, const void* logits, int64_t row_stride, int B, int V, const float* u,
                            const float* temperature, float temperature_s, const int* top_k, int top_k_s,
                            const float* top_p, float top_p_s, const float* min_p, float min_p_s,
                            unsigned char* finished, int64_t eos_id, int64_t* tokens, int* kept, hipStream_t stream) {
  if (B < 0 || V < 1 || row_stride < V) return hipErrorInvalidValue;
  if (dt != CS_F32 && dt != CS_BF16 && dt != CS_F16) return hipErrorInvalidValue;
  if (B == 0) return hipSuccess;
  const uintptr_t esize = dt == CS_F32 ? 4 : 2;
  if (logits == nullptr || u == nullptr || tokens == nullptr || kept == nullptr) return hipErrorInvalidValue;
  if (!aligned(logits, esize) || !aligned(u, 4) || !aligned(tokens, 8) || !aligned(kept, 4) ||
      !aligned(temperature, 4) || !aligned(top_k, 4) || !aligned(top_p, 4) || !aligned(min_p, 4))
    return hipErrorInvalidValue;
  if (!(temperature_s >= 0.f) || top_k_s < 0 || !(top_p_s > 0.f && top_p_s <= 1.f) ||
      !(min_p_s >= 0.f && min_p_s <= 1.f))
    return hipErrorInvalidValue;
  int bits = 0;
  while ((1LL << bits) <= (long long)V) ++bits;  // V < 2^bits
  SampleArgs a;
  a.logits = logits;
  a.row_stride = row_stride;
  a.u = u;
  a.temp = temperature;
  a.topp = top_p;
  a.minp = min_p;
  a.topk = top_k;
  a.temp_s = temperature_s;
  a.topp_s = top_p_s;
  a.minp_s = min_p_s;
  a.topk_s = top_k_s == 0 ? INT_MAX : top_k_s;
  a.finished = finished;
  a.eos = eos_id;
  a.tokens = reinterpret_cast<long long*>(tokens);
  a.kept = kept;
  a.V = V;
  a.shift = 62 - bits < 44 ? 62 - bits : 44;
  if (dt == CS_F32) return launch<CS_F32>(a, B, stream);
  if (dt == CS_BF16) return launch<CS_BF16>(a, B, stream);
  return launch<CS_F16>(a, B, stream);
}
