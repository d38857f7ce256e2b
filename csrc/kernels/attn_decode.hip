// Decode attention for gfx950: one query row per head against a KV cache, split over the keys.
//
// q / o: bf16 [B, Hq, D]; kc / vc: bf16 caches [B, Smax, Hkv, D] (row stride Hkv * D, batch stride an
// argument, so cache[:, :n] of a longer cache is an operand); lens: int32 [B], sequence b sees keys
// 0 .. lens[b] - 1 (clamped into [0, Smax] here). D in {64, 128}, G = Hq / Hkv in {1, 2, 4, 8}.
//
// attn_decode_kernel<D, G, Cache>, grid (nsplit, Hkv, B), one 256-thread workgroup per (slice of the keys, kv
// head, sequence): it serves all G query heads of its kv head, so K and V are read from memory once per kv head.
// A key row (D elements) lies in D / 8 adjacent lanes, one load per lane straight into VGPRs (no LDS staging);
// a wave reads 64 / (D / 8) keys per load instruction and the workgroup a tile of kDecKT = 64 keys per trip.
// The G dot products of a key are fp32 FMAs on the VALU, summed over the key's lanes by DPP
// (quad_perm, row_half_mirror, row_mirror: no LDS traffic); the matrix cores are not used: with at most 8
// query rows an MFMA tile would be half padding, V would need a transpose through LDS for the second
// product, and the kernel is bound by the K/V read, not by arithmetic. Every lane group keeps its own online
// softmax state (m, l, acc) in base 2 (scores times c = log2(e) * scale) over the keys it has seen; the groups
// of a wave are merged by shuffles and the four waves through LDS, in a fixed order, at the end.
//
// A key at or past lens[b] is never loaded: its K and V registers are zero and its score is -inf, which
// neither moves the running max nor weighs anything, so stale cache rows (NaN, Inf) contribute exactly nothing.
//
// The slice of split s is a run of whole key tiles of the clamped length, divided as evenly as possible over
// nsplit; an empty slice writes m = -inf, l = 0 and a zero partial. With nsplit > 1 a slice writes the fp32
// partial o_part[b, hq, s, :] (unnormalised) and (m, l), and attn_decode_combine_kernel sums the slices of a
// row in split order and writes bf16 o. With nsplit == 1 the first kernel writes o itself. No float atomics,
// no arrival counters: the same bits every run.
//
// The cache format is the kernel's third template argument, and all that depends on it is in the two structs
// below: the width of a lane's load, the unpack, and whether and where scales are read.
//   Bf16Cache (cs_attn_decode): 16 bytes per lane, eight bf16 values.
//   Fp8Cache (cs_attn_decode_fp8): kc / vc hold OCP e4m3fn codes, one byte each, and ks / vs fp32 [B, Smax, Hkv]
//   one power-of-two scale per (token, kv head); kv_append_fp8.hip writes both. 8 bytes per lane, unpacked two
//   values at a time by v_cvt_pk_f32_fp8. The key's scale multiplies the finished score, (q . k8) * ks, and the
//   value's scale the weight, p * vs: G multiplies per key each, not D. A masked key loads neither codes nor
//   scales. With power-of-two scales this is the arithmetic of the bf16 instantiation on the dequantised cache.
//
// Where key n of sequence b lives is the other compile-time property of the cache argument (kPaged).
//   Contiguous (Bf16Cache, Fp8Cache): row n of cache[b].
//   Paged (PagedBf16Cache: cs_attn_decode_paged, PagedFp8Cache: cs_attn_decode_paged_fp8): kc / vc are pools
//   [P, page, Hkv, D] shared by all sequences (ks / vs [P, page, Hkv]), page a multiple of the key tile, and
//   table int32 [B, C] names the pages of a sequence: key n is row n % page of page table[b, n / page], and
//   Smax = C * page. A page is whole tiles, so a tile has one table entry: the workgroup reads it once per trip
//   (it depends on blockIdx and the trip count only: a scalar load), and an entry outside [0, P) masks the
//   tile's keys in the predicate that guards the loads, exactly like keys past the length: never loaded, score
//   -inf. Nothing else differs, so for equal nsplit and lens the paged kernels return the bits of the
//   contiguous ones on the gathered cache.
#include <math.h>

#include "common.h"
#include "launchers.h"

namespace {

constexpr int kDecKT = 64;     // keys per workgroup trip
constexpr int kDecWaves = 4;   // waves per workgroup
constexpr int kDecTarget = 768;  // workgroups aimed at: 3 per CU on 256 CUs
constexpr int kDecMinTiles = 2;  // key tiles per split the heuristic keeps
constexpr int kDecMaxSplits = 256;

template <int CTRL>
__device__ __forceinline__ float dpp_mov(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, false));
}

// the sum of v over the LPK (8 or 16) adjacent lanes of a key, left in every one of them
template <int LPK>
__device__ __forceinline__ float key_sum(float v) {
  v += dpp_mov<0xB1>(v);   // quad_perm [1, 0, 3, 2]
  v += dpp_mov<0x4E>(v);   // quad_perm [2, 3, 0, 1]
  v += dpp_mov<0x141>(v);  // row_half_mirror: the other quad of the 8
  if (LPK == 16) v += dpp_mov<0x140>(v);  // row_mirror: the other half of the 16
  return v;
}

__device__ __forceinline__ void unpack8(const uint4& w, float (&f)[8]) {
  f[0] = __uint_as_float(w.x << 16); f[1] = __uint_as_float(w.x & 0xffff0000u);
  f[2] = __uint_as_float(w.y << 16); f[3] = __uint_as_float(w.y & 0xffff0000u);
  f[4] = __uint_as_float(w.z << 16); f[5] = __uint_as_float(w.z & 0xffff0000u);
  f[6] = __uint_as_float(w.w << 16); f[7] = __uint_as_float(w.w & 0xffff0000u);
}

// The cache formats. Row: what a lane loads of a key row, its eight elements; k / v and batch_stride count
// elements; unpack: the eight values in fp32; kScaled: whether ks / vs [B, Smax, Hkv] hold a scale per row;
// kPaged: whether the rows are reached through a block table (PageMap below).
struct Bf16Cache {
  using Row = uint4;
  static constexpr bool kScaled = false;
  static constexpr bool kPaged = false;
  const __bf16 *k, *v;
  size_t batch_stride;
  static __device__ __forceinline__ void unpack(const Row& w, float (&f)[8]) { unpack8(w, f); }
};

struct Fp8Cache {
  using Row = uint2;
  static constexpr bool kScaled = true;
  static constexpr bool kPaged = false;
  const unsigned char *k, *v;
  size_t batch_stride;
  const float *ks, *vs;
  size_t scale_batch_stride;
  // eight e4m3fn codes, two per v_cvt_pk_f32_fp8
  static __device__ __forceinline__ void unpack(const Row& w, float (&f)[8]) {
    const auto a = __builtin_amdgcn_cvt_pk_f32_fp8((int)w.x, false), b = __builtin_amdgcn_cvt_pk_f32_fp8((int)w.x, true);
    const auto c = __builtin_amdgcn_cvt_pk_f32_fp8((int)w.y, false), d = __builtin_amdgcn_cvt_pk_f32_fp8((int)w.y, true);
    f[0] = a[0]; f[1] = a[1]; f[2] = b[0]; f[3] = b[1];
    f[4] = c[0]; f[5] = c[1]; f[6] = d[0]; f[7] = d[1];
  }
};

// The block table of a paged cache: table[b * row_stride + c] is the page of keys c * page .. (c + 1) * page - 1
// of sequence b, valid when it lies in [0, pages); tiles = page / kDecKT. In the paged formats batch_stride and
// scale_batch_stride are the strides of a page, and k / v / ks / vs the pools.
struct PageMap {
  const int* table;
  size_t row_stride;
  int pages, tiles;
};

struct PagedBf16Cache : Bf16Cache {
  static constexpr bool kPaged = true;
  PageMap map;
};

struct PagedFp8Cache : Fp8Cache {
  static constexpr bool kPaged = true;
  PageMap map;
};

// exp2(a - m) with m = -inf (nothing seen yet) read as 0: exp2(-inf - 0) = 0, never exp2(-inf + inf)
__device__ __forceinline__ float safe_max(float m) { return m == -INFINITY ? 0.f : m; }

template <int D, int G, typename Cache>
__global__ __launch_bounds__(256) void attn_decode_kernel(const __bf16* __restrict__ q, const Cache cache,
                                                          const int* __restrict__ lens, __bf16* __restrict__ o,
                                                          float* __restrict__ ws_o, float* __restrict__ ws_ml,
                                                          int Smax, int Hkv, float c) {
  using Row = typename Cache::Row;
  constexpr int LPK = D / 8;                       // lanes per key row
  constexpr int KPW = 64 / LPK;                    // keys per wave load
  constexpr int U = kDecKT / (kDecWaves * KPW);    // loads of K (and of V) per lane and trip
  static_assert(U * kDecWaves * KPW == kDecKT, "tile");
  __shared__ float sm_acc[kDecWaves][G][D];
  __shared__ float sm_ml[kDecWaves][G][2];

  const int split = blockIdx.x, nsplit = gridDim.x, hkv = blockIdx.y, b = blockIdx.z;
  const int Hq = Hkv * G;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane / LPK, d0 = (lane % LPK) * 8;

  int len = lens[b];
  len = len < 0 ? 0 : (len > Smax ? Smax : len);
  const int ntiles = (len + kDecKT - 1) / kDecKT;
  const int base = ntiles / nsplit, rem = ntiles % nsplit;
  const int t0 = split * base + (split < rem ? split : rem);
  const int t1 = t0 + base + (split < rem ? 1 : 0);

  float qf[G][8], m[G], l[G], acc[G][8];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    const uint4 w = *reinterpret_cast<const uint4*>(q + ((size_t)b * Hq + (size_t)hkv * G + g) * D + d0);
    unpack8(w, qf[g]);
    m[g] = -INFINITY;
    l[g] = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) { qf[g][j] *= c; acc[g][j] = 0.f; }
  }

  const size_t row = (size_t)Hkv * D;
  const size_t seq = Cache::kPaged ? 0 : b;  // a pool has no sequence axis: the page's offset is added per tile
  const size_t head = seq * cache.batch_stride + (size_t)hkv * D + d0;
  size_t shead = 0;
  if constexpr (Cache::kScaled) shead = seq * cache.scale_batch_stride + hkv;
  // kPaged: tile t is tile `pt` of table column `col`; both follow t without a division per trip
  int col = 0, pt = 0;
  if constexpr (Cache::kPaged) {
    col = t0 / cache.map.tiles;
    pt = t0 - col * cache.map.tiles;
  }
  for (int t = t0; t < t1; ++t) {
    Row kr[U], vr[U];
    float ksr[U], vsr[U];  // kScaled: the scales of the key's K and V rows, the same in all its lanes
    bool ok[U];
    // kPaged: the tile's page, one load for the workgroup. t < ntiles, so col < C: inside the table. An entry
    // outside [0, pages) masks the tile and is never turned into an address.
    bool page_ok = true;
    size_t phead = 0, pshead = 0;
    if constexpr (Cache::kPaged) {
      const int entry = cache.map.table[(size_t)b * cache.map.row_stride + col];
      page_ok = entry >= 0 && entry < cache.map.pages;
      if (page_ok) {
        phead = head + (size_t)entry * cache.batch_stride;
        if constexpr (Cache::kScaled) pshead = shead + (size_t)entry * cache.scale_batch_stride;
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int key = t * kDecKT + u * (kDecWaves * KPW) + wave * KPW + r;
      ok[u] = key < len;
      if constexpr (Cache::kPaged) ok[u] = ok[u] && page_ok;
      // Row(0u), not Row{}: value-initialisation makes the compiler schedule the bf16 instantiations differently,
      // measurably slower at B 64 (docs/decode_attention.md, "Shared template")
      kr[u] = Row(0u);
      vr[u] = Row(0u);
      ksr[u] = vsr[u] = 0.f;
      if (ok[u]) {  // key < len <= Smax: inside the caches and the scales; a masked key reads neither
        // kPaged: row pt * kDecKT + (key - t * kDecKT) < page of a page in [0, pages)
        const size_t prow = (size_t)(pt * kDecKT + u * (kDecWaves * KPW) + wave * KPW + r);
        const size_t off = Cache::kPaged ? phead + prow * row : head + (size_t)key * row;
        kr[u] = *reinterpret_cast<const Row*>(cache.k + off);
        vr[u] = *reinterpret_cast<const Row*>(cache.v + off);
        if constexpr (Cache::kScaled) {
          ksr[u] = cache.ks[Cache::kPaged ? pshead + prow * Hkv : shead + (size_t)key * Hkv];
          vsr[u] = cache.vs[Cache::kPaged ? pshead + prow * Hkv : shead + (size_t)key * Hkv];
        }
      }
    }
    if constexpr (Cache::kPaged) {
      if (++pt == cache.map.tiles) { pt = 0; ++col; }
    }
    float s[U][G];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      float kf[8];
      Cache::unpack(kr[u], kf);
#pragma unroll
      for (int g = 0; g < G; ++g) {
        float d = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) d = fmaf(qf[g][j], kf[j], d);
        d = key_sum<LPK>(d);
        if constexpr (Cache::kScaled) d *= ksr[u];  // the key's scale once per score
        s[u][g] = ok[u] ? d : -INFINITY;
      }
    }
#pragma unroll
    for (int g = 0; g < G; ++g) {
      float mx = m[g];
#pragma unroll
      for (int u = 0; u < U; ++u) mx = fmaxf(mx, s[u][g]);
      const float ms = safe_max(mx);
      const float alpha = __builtin_amdgcn_exp2f(m[g] - ms);
      float ps = 0.f;
#pragma unroll
      for (int u = 0; u < U; ++u) {
        s[u][g] = __builtin_amdgcn_exp2f(s[u][g] - ms);
        ps += s[u][g];
      }
      l[g] = l[g] * alpha + ps;
      m[g] = mx;
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[g][j] *= alpha;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      float vf[8];
      Cache::unpack(vr[u], vf);
#pragma unroll
      for (int g = 0; g < G; ++g) {
        float p = s[u][g];
        if constexpr (Cache::kScaled) p *= vsr[u];  // the value's scale once per weight
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[g][j] = fmaf(p, vf[j], acc[g][j]);
      }
    }
  }

  // the lane groups of a wave: a butterfly over the group index; group 0's result is the wave's
#pragma unroll
  for (int off = LPK; off < 64; off <<= 1) {
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const float m2 = __shfl_xor(m[g], off, 64), l2 = __shfl_xor(l[g], off, 64);
      const float mx = fmaxf(m[g], m2), ms = safe_max(mx);
      const float a1 = __builtin_amdgcn_exp2f(m[g] - ms), a2 = __builtin_amdgcn_exp2f(m2 - ms);
      l[g] = l[g] * a1 + l2 * a2;
      m[g] = mx;
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[g][j] = acc[g][j] * a1 + __shfl_xor(acc[g][j], off, 64) * a2;
    }
  }
  if (r == 0) {
#pragma unroll
    for (int g = 0; g < G; ++g) {
#pragma unroll
      for (int j = 0; j < 8; ++j) sm_acc[wave][g][d0 + j] = acc[g][j];
      if (d0 == 0) { sm_ml[wave][g][0] = m[g]; sm_ml[wave][g][1] = l[g]; }
    }
  }
  __syncthreads();
  // the four waves, in wave order
  for (int i = tid; i < G * D; i += 256) {
    const int g = i / D, d = i % D;
    float mx = -INFINITY;
#pragma unroll
    for (int w = 0; w < kDecWaves; ++w) mx = fmaxf(mx, sm_ml[w][g][0]);
    const float ms = safe_max(mx);
    float L = 0.f, O = 0.f;
#pragma unroll
    for (int w = 0; w < kDecWaves; ++w) {
      const float a = __builtin_amdgcn_exp2f(sm_ml[w][g][0] - ms);
      L += sm_ml[w][g][1] * a;
      O += sm_acc[w][g][d] * a;
    }
    const size_t hq = (size_t)b * Hq + (size_t)hkv * G + g;
    if (nsplit == 1) {
      o[hq * D + d] = (__bf16)(L > 0.f ? O / L : 0.f);
    } else {
      ws_o[(hq * nsplit + split) * D + d] = O;
      if (d == 0) {
        ws_ml[(hq * nsplit + split) * 2] = mx;
        ws_ml[(hq * nsplit + split) * 2 + 1] = L;
      }
    }
  }
}

// one block of D threads per (b, hq) row: the splits in split order
template <int D>
__global__ __launch_bounds__(D) void attn_decode_combine_kernel(const float* __restrict__ ws_o,
                                                                const float* __restrict__ ws_ml,
                                                                __bf16* __restrict__ o, int nsplit) {
  const size_t rowi = blockIdx.x;
  const int d = threadIdx.x;
  const float* ml = ws_ml + rowi * nsplit * 2;
  float mx = -INFINITY;
  for (int s = 0; s < nsplit; ++s) mx = fmaxf(mx, ml[2 * s]);
  const float ms = safe_max(mx);
  float L = 0.f, O = 0.f;
  for (int s = 0; s < nsplit; ++s) {
    const float a = __builtin_amdgcn_exp2f(ml[2 * s] - ms);
    L += ml[2 * s + 1] * a;
    O += ws_o[(rowi * nsplit + s) * D + d] * a;
  }
  o[rowi * D + d] = (__bf16)(L > 0.f ? O / L : 0.f);
}

template <int D, int G, typename Cache>
hipError_t launch_decode(const void* q, const Cache& cache, const int* lens, void* o, float* ws, int B, int Smax,
                         int Hkv, int nsplit, float scale, hipStream_t st) {
  const size_t rows = (size_t)B * Hkv * G;
  float* ws_o = ws;
  float* ws_ml = ws == nullptr ? nullptr : ws + rows * nsplit * D;
  const float c = scale * 1.4426950408889634f;
  hipLaunchKernelGGL((attn_decode_kernel<D, G, Cache>), dim3(nsplit, Hkv, B), dim3(256), 0, st, (const __bf16*)q, cache,
                     lens, (__bf16*)o, ws_o, ws_ml, Smax, Hkv, c);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || nsplit == 1) return e;
  hipLaunchKernelGGL(attn_decode_combine_kernel<D>, dim3((unsigned)rows), dim3(D), 0, st, ws_o, ws_ml, (__bf16*)o,
                     nsplit);
  return hipGetLastError();
}

template <int D, typename Cache>
hipError_t launch_decode_g(int G, const void* q, const Cache& cache, const int* lens, void* o, float* ws, int B,
                           int Smax, int Hkv, int nsplit, float scale, hipStream_t st) {
#define CS_DECODE_G(g) \
  case g: return launch_decode<D, g>(q, cache, lens, o, ws, B, Smax, Hkv, nsplit, scale, st)
  switch (G) {
    CS_DECODE_G(1);
    CS_DECODE_G(2);
    CS_DECODE_G(4);
    CS_DECODE_G(8);
  }
#undef CS_DECODE_G
  return hipErrorInvalidValue;
}

bool aligned16(const void* p) { return p != nullptr && reinterpret_cast<uintptr_t>(p) % 16 == 0; }

}  // namespace

int cs_attn_decode_key_tile() { return kDecKT; }

int cs_attn_decode_max_splits(int Smax) { return Smax < 1 ? 1 : (Smax + kDecKT - 1) / kDecKT; }

int cs_attn_decode_splits(int B, int Hkv, int Smax) {
  if (B < 1 || Hkv < 1 || Smax < 1) return 1;
  const int64_t groups = (int64_t)B * Hkv;
  int64_t n = (kDecTarget + groups - 1) / groups;
  const int64_t cap = cs_attn_decode_max_splits(Smax) / kDecMinTiles;
  if (n > cap) n = cap;
  if (n > kDecMaxSplits) n = kDecMaxSplits;
  return n < 1 ? 1 : (int)n;
}

size_t cs_attn_decode_ws_floats(int B, int Hq, int D, int nsplit) {
  return nsplit <= 1 ? 0 : (size_t)B * Hq * nsplit * ((size_t)D + 2);
}

namespace {

// whether the cache holds Smax rows per sequence (contiguous) or its pages hold `page` rows (paged)
template <typename Cache>
bool layout_ok(const Cache& cache, int Smax, int Hkv, int D) {
  if constexpr (Cache::kPaged) {
    const PageMap& m = cache.map;
    if (m.table == nullptr || reinterpret_cast<uintptr_t>(m.table) % 4 != 0 || m.pages < 1 || m.tiles < 1) return false;
    if (Smax % (m.tiles * kDecKT) != 0 || m.row_stride < (size_t)(Smax / (m.tiles * kDecKT))) return false;
    return cache.batch_stride % 8 == 0 && cache.batch_stride >= (size_t)m.tiles * kDecKT * Hkv * D;
  } else {
    return cache.batch_stride % 8 == 0 && cache.batch_stride >= (size_t)Smax * Hkv * D;
  }
}

template <typename Cache>
hipError_t decode_checked(const void* q, const Cache& cache, const int* lens, void* o, float* ws, int B, int Smax,
                          int Hq, int Hkv, int D, int nsplit, float scale, hipStream_t stream) {
  if (B == 0) return hipSuccess;
  if (B < 0 || B > 65535 || Hkv < 1 || Hkv > 65535 || Hq < 1 || Hq % Hkv != 0 || Smax < 1) return hipErrorInvalidValue;
  if (nsplit < 1 || nsplit > cs_attn_decode_max_splits(Smax)) return hipErrorInvalidValue;
  if (!layout_ok(cache, Smax, Hkv, D)) return hipErrorInvalidValue;
  if (!aligned16(q) || !aligned16(cache.k) || !aligned16(cache.v) || !aligned16(o) || lens == nullptr)
    return hipErrorInvalidValue;
  if (nsplit > 1 && !aligned16(ws)) return hipErrorInvalidValue;
  if ((size_t)B * Hq > 0x7fffffffu) return hipErrorInvalidValue;
  const int G = Hq / Hkv;
  if (D == 128) return launch_decode_g<128>(G, q, cache, lens, o, ws, B, Smax, Hkv, nsplit, scale, stream);
  if (D == 64) return launch_decode_g<64>(G, q, cache, lens, o, ws, B, Smax, Hkv, nsplit, scale, stream);
  return hipErrorInvalidValue;
}

}  // namespace

hipError_t cs_attn_decode(const void* q, const void* kc, const void* vc, const int* lens, void* o, float* ws, int B,
                          int Smax, int Hq, int Hkv, int D, size_t batch_stride, int nsplit, float scale,
                          hipStream_t stream) {
  const Bf16Cache cache{(const __bf16*)kc, (const __bf16*)vc, batch_stride};
  return decode_checked(q, cache, lens, o, ws, B, Smax, Hq, Hkv, D, nsplit, scale, stream);
}

hipError_t cs_attn_decode_fp8(const void* q, const void* kc, const void* vc, const float* ks, const float* vs,
                              const int* lens, void* o, float* ws, int B, int Smax, int Hq, int Hkv, int D,
                              size_t batch_stride, size_t scale_batch_stride, int nsplit, float scale,
                              hipStream_t stream) {
  if (B > 0 && (ks == nullptr || vs == nullptr || reinterpret_cast<uintptr_t>(ks) % 4 != 0 ||
                reinterpret_cast<uintptr_t>(vs) % 4 != 0 || Smax < 1 || Hkv < 1 ||
                scale_batch_stride < (size_t)Smax * Hkv))
    return hipErrorInvalidValue;
  const Fp8Cache cache{(const unsigned char*)kc, (const unsigned char*)vc, batch_stride, ks, vs, scale_batch_stride};
  return decode_checked(q, cache, lens, o, ws, B, Smax, Hq, Hkv, D, nsplit, scale, stream);
}

namespace {

// Smax = C * page of a paged cache, or 0 when page is no positive multiple of the key tile or Smax overflows
int paged_smax(int C, int page) {
  if (C < 1 || page < kDecKT || page % kDecKT != 0 || (int64_t)C * page > 0x7fffffff) return 0;
  return C * page;
}

}  // namespace

hipError_t cs_attn_decode_paged(const void* q, const void* kp, const void* vp, const int* table, const int* lens,
                                void* o, float* ws, int B, int C, int Hq, int Hkv, int D, int pages, int page,
                                size_t page_stride, size_t table_stride, int nsplit, float scale, hipStream_t stream) {
  const int Smax = paged_smax(C, page);
  if (B > 0 && Smax == 0) return hipErrorInvalidValue;
  PagedBf16Cache cache{{(const __bf16*)kp, (const __bf16*)vp, page_stride}, {table, table_stride, pages, page / kDecKT}};
  return decode_checked(q, cache, lens, o, ws, B, Smax, Hq, Hkv, D, nsplit, scale, stream);
}

hipError_t cs_attn_decode_paged_fp8(const void* q, const void* kp, const void* vp, const float* ks, const float* vs,
                                    const int* table, const int* lens, void* o, float* ws, int B, int C, int Hq,
                                    int Hkv, int D, int pages, int page, size_t page_stride, size_t scale_page_stride,
                                    size_t table_stride, int nsplit, float scale, hipStream_t stream) {
  const int Smax = paged_smax(C, page);
  if (B > 0 && (Smax == 0 || ks == nullptr || vs == nullptr || reinterpret_cast<uintptr_t>(ks) % 4 != 0 ||
                reinterpret_cast<uintptr_t>(vs) % 4 != 0 || Hkv < 1 || scale_page_stride < (size_t)page * Hkv))
    return hipErrorInvalidValue;
  PagedFp8Cache cache{{(const unsigned char*)kp, (const unsigned char*)vp, page_stride, ks, vs, scale_page_stride},
                      {table, table_stride, pages, page / kDecKT}};
  return decode_checked(q, cache, lens, o, ws, B, Smax, Hq, Hkv, D, nsplit, scale, stream);
}
