// Extend attention for gfx950: T new query tokens per sequence against a KV cache that already holds their keys
// and values behind whatever the sequence held before (append, then attend). The forward-only sibling of
// attn_fwd_kernel (attention.hip), from whose device helpers (attn_device.h) it is built: one workgroup = 4 waves =
// 128 queries of one (batch, query head), K/V tiles of 64 keys LDS-DMA-staged into the double-buffered swizzled
// image, scores transposed (S^T = K . Q^T) so that the accumulator feeds the second product, online softmax in
// base 2, bf16 P, f32 accumulation, bf16 out. No split over the keys, no atomics: the same bits every run.
//
// q / o: bf16 [B, T, Hq, D], right-padded. start[b] (clamped into [0, Smax]) is row b's length before these
// tokens, counts[b] (clamped into [0, min(T, Smax - start)]; absent = T) the number of real ones. Query
// i < counts[b] sits at position start[b] + i and sees keys 0 .. start[b] + i (the bottom-right aligned causal
// mask); rows i >= counts[b] of o are zeros. A workgroup's key loop ends at the tile of its last live query.
//
// Stale data contributes exactly nothing, V included (0 x NaN inside an MFMA is NaN, so masking the score is not
// enough): every key at or past n = start[b] + counts[b] lands in LDS as zeros, because the buffer resource the
// DMA reads through ends at row n - 1 and rows past it get an out-of-range offset.
//
// Contiguous cache: bf16 [B, Smax, Hkv, D] with a batch stride (cache[:, :n] is an operand).
// Paged cache: pools [P, page, Hkv, D] and table int32 [B, C], page a multiple of the key tile, so a tile has ONE
// table entry, read once per tile, uniform over the workgroup. Each tile gets a resource of its own over its
// page's live rows only (32-bit offsets stay inside one page; no resource spans the pool). An entry outside
// [0, P) masks the whole tile: nothing is staged, nothing is computed, the entry never becomes an address.
//
// Out of scope here: T = 1 and small T work but waste the 128-query tile (decode attention, attn_decode.hip, is
// the kernel for T = 1; packing the G query heads of a kv head into the tile and a split over the keys are not
// done), and FP8 caches (LDS-DMA cannot dequantise; ops/attention.py dequantises into a bf16 scratch).
#include <math.h>

#include "attn_device.h"
#include "common.h"
#include "launchers.h"

namespace {

struct ExtPaged {
  const int* table;     // [B, C], column stride 1
  size_t table_stride;  // entries between rows
  int pages;            // P
  int page;             // rows per page, a multiple of kBN
};

template <int D, bool PAGED>
__global__ __launch_bounds__(256, 2) void attn_extend_kernel(const __bf16* __restrict__ q, const __bf16* __restrict__ k,
                                                          const __bf16* __restrict__ v, __bf16* __restrict__ o,
                                                          const int* __restrict__ start, const int* __restrict__ counts,
                                                          int T, int Smax, int Hq, int Hkv, size_t outer_stride,
                                                          float c, ExtPaged pg) {
  constexpr int KK = D / 16, DT = D / 32, TILE = kBN * D * 2;  // bytes of one K or V image
  extern __shared__ __attribute__((aligned(16))) char smem[];  // [2 buffers][K image, V image]
  const int nqb = (T + kBM - 1) / kBM;
  const int qb = nqb - 1 - (int)blockIdx.x;  // the longest (latest) query blocks first
  const int hq = blockIdx.y, b = blockIdx.z, hk = hq / (Hq / Hkv);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
  const int q0 = qb * kBM, q0w = q0 + 32 * w, qi = q0w + r;
  const size_t qs = (size_t)Hq * D, ks = (size_t)Hkv * D;
  // block-uniform, clamped: nothing below depends on the contents of start / counts for its bounds
  const int st = clampi(start[b], 0, Smax);
  const int cnt = clampi(counts != nullptr ? counts[b] : T, 0, min(T, Smax - st));
  const int nvis = st + cnt;  // the row's length with the new tokens: keys at or past it are stale
  __bf16* orow = o + ((size_t)b * T + qi) * qs + (size_t)hq * D;

  f32x16 acc[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) acc[dt] = zero16();
  if (q0 >= cnt) {  // block-uniform: only padding here
    if (qi < T) store_rowT<D>(acc, 0.f, orow, h);
    return;
  }
  const bool live = qi < cnt;
  const int lim = live ? st + qi : -1;  // the last key this lane's query sees; a padded row sees none
  bf16x8 qf[KK];
#pragma unroll
  for (int kk = 0; kk < KK; ++kk) qf[kk] = gload8(q + ((size_t)b * T + qi) * qs + (size_t)hq * D + 16 * kk + 8 * h, live);
  float m = -INFINITY, l = 0.f;

  const int kend = st + min(q0 + kBM, cnt);  // one past the block's last live query's position; <= nvis <= Smax
  const int nkt = (kend + kBN - 1) / kBN;
  // the wave's last live query's position (wave-uniform); -1 when the wave holds padding only
  const int wlast = q0w < cnt ? st + min(q0w + 31, cnt - 1) : -1;
  const bool ragged = q0w + 31 >= cnt;  // the wave holds padded rows

  // the contiguous cache: one resource for the whole loop, ending at the row's last live key
  const size_t cbase = PAGED ? 0 : (size_t)b * outer_stride + (size_t)hk * D;
  const Dma<D> dkc(k + cbase, ks, PAGED ? 0 : nvis), dvc(v + cbase, ks, PAGED ? 0 : nvis);
  // Paged: the tiles are staged in order, so the (table column, first row inside its page) pair of the next tile
  // to stage runs along without a division, and that tile's table entry is loaded one tile ahead of its use (the
  // scalar load's latency falls on a tile's arithmetic, not on the DMA issue). kt * kBN < kend <= Smax = C * page,
  // so a column that is read lies in [0, C).
  int ncol = 0, nrow = 0, entry = -1;
  const int* trow = nullptr;
  if constexpr (PAGED) {
    trow = pg.table + (size_t)b * pg.table_stride;
    entry = trow[0];  // nkt >= 1
  }
  // stage key tile kt into buf; false (paged) when its table entry names no page: nothing is loaded then
  auto stage = [&](int kt, char* buf) -> bool {
    if constexpr (PAGED) {
      const int e = __builtin_amdgcn_readfirstlane(entry), col = ncol, row0 = nrow;
      nrow += kBN;
      if (nrow == pg.page) {
        nrow = 0;
        ++ncol;
      }
      if (kt + 1 < nkt) entry = trow[ncol];  // the next tile's, used at the next call
      if (e < 0 || e >= pg.pages) return false;
      const int rows = min(pg.page, nvis - col * pg.page);  // the page's live rows, >= 1
      const size_t base = (size_t)e * outer_stride + (size_t)hk * D;
      const Dma<D> dk(k + base, ks, rows), dv(v + base, ks, rows);
      dk.issue(buf, row0);
      dv.issue(buf + TILE, row0);
    } else {
      dkc.issue(buf, kt * kBN);
      dvc.issue(buf + TILE, kt * kBN);
    }
    return true;
  };

  bool have = stage(0, smem);
  dma_barrier();
  for (int kt = 0; kt < nkt; ++kt) {
    const int cur = kt & 1;
    bool have_next = false;
    if (kt + 1 < nkt) have_next = stage(kt + 1, smem + (cur ^ 1) * 2 * TILE);  // its readers passed the last barrier
    const char* Kl = smem + cur * 2 * TILE;
    const char* Vl = Kl + TILE;
    const int k0 = kt * kBN;
    // wave-uniform: the tile is there and some key of it is visible to this wave
    if (have && k0 <= wlast) {
      f32x16 s[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        s[t] = zero16();
#pragma unroll
        for (int kk = 0; kk < KK; ++kk) s[t] = mfma(row_frag<D>(Kl, 32 * t + r, kk, h), qf[kk], s[t]);
      }
      const bool edge = ragged || k0 + kBN - 1 > st + q0w;
      float mx = -INFINITY;
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          float x = s[t][e] * c;
          if (edge) {
            const int key = k0 + 32 * t + acc_row(e, h);
            if (key > lim) x = -INFINITY;
          }
          s[t][e] = x;
          mx = fmaxf(mx, x);
        }
      mx = fmaxf(mx, __shfl_xor(mx, 32));
      const float mn = fmaxf(m, mx);
      const float mu = mn == -INFINITY ? 0.f : mn;
      const float alpha = __builtin_amdgcn_exp2f(m - mu);
      float rs = 0.f;
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const float p = __builtin_amdgcn_exp2f(s[t][e] - mu);
          s[t][e] = p;
          rs += p;
        }
      rs += __shfl_xor(rs, 32);
      l = l * alpha + rs;
      m = mn;
#pragma unroll
      for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[dt][e] *= alpha;
      bf16x8 pf[2][2];
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int ss = 0; ss < 2; ++ss) pf[t][ss] = acc_frag(s[t], ss);
#pragma unroll
      for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int ss = 0; ss < 2; ++ss) acc[dt] = mfma(tr_frag<D>(Vl, 32 * t + 16 * ss, 32 * dt, lane), pf[t][ss], acc[dt]);
    }
    dma_barrier();
    have = have_next;
  }
  if (qi < T) store_rowT<D>(acc, l > 0.f ? 1.f / l : 0.f, orow, h);
}

template <int D, bool PAGED>
hipError_t launch_extend(const void* q, const void* k, const void* v, void* o, const int* start, const int* counts, int B,
                         int T, int Smax, int Hq, int Hkv, size_t outer_stride, float scale, const ExtPaged& pg,
                         hipStream_t st) {
  const dim3 grid((T + kBM - 1) / kBM, Hq, B);
  hipLaunchKernelGGL((attn_extend_kernel<D, PAGED>), grid, dim3(256), 2 * 2 * (size_t)kBN * D * 2, st, (const __bf16*)q,
                     (const __bf16*)k, (const __bf16*)v, (__bf16*)o, start, counts, T, Smax, Hq, Hkv, outer_stride,
                     scale * 1.4426950408889634f, pg);
  return hipGetLastError();
}

bool aligned(const void* p, uintptr_t a) { return p != nullptr && reinterpret_cast<uintptr_t>(p) % a == 0; }

// `rows` cache rows of Hkv * D elements (one sequence of a contiguous cache, one page of a pool) lie `outer_stride`
// elements apart; a resource over them, and the out-of-range offset kOOB beyond it, must fit 32-bit byte offsets
template <bool PAGED>
hipError_t extend_checked(const void* q, const void* k, const void* v, void* o, const int* start, const int* counts,
                          int B, int T, int Smax, int rows, int Hq, int Hkv, int D, size_t outer_stride, float scale,
                          const ExtPaged& pg, hipStream_t stream) {
  if (B == 0 || T == 0) return hipSuccess;
  if (B < 0 || B > 65535 || T < 0 || Hq < 1 || Hq > 65535 || Hkv < 1 || Hq % Hkv != 0 || Smax < 1 || rows < 1)
    return hipErrorInvalidValue;
  if (D != 64 && D != 128) return hipErrorInvalidValue;
  if (!aligned(q, 16) || !aligned(k, 16) || !aligned(v, 16) || !aligned(o, 16) || !aligned(start, 4))
    return hipErrorInvalidValue;
  if (counts != nullptr && !aligned(counts, 4)) return hipErrorInvalidValue;
  if (outer_stride % 8 != 0 || outer_stride < (size_t)rows * Hkv * D) return hipErrorInvalidValue;
  if ((int64_t)(rows - 1) * Hkv * D * 2 + 2 * D > (int64_t)kOOB) return hipErrorInvalidValue;
  if (PAGED) {
    if (!aligned(pg.table, 4) || pg.pages < 1 || pg.table_stride < (size_t)(Smax / pg.page)) return hipErrorInvalidValue;
  }
  if (D == 128)
    return launch_extend<128, PAGED>(q, k, v, o, start, counts, B, T, Smax, Hq, Hkv, outer_stride, scale, pg, stream);
  return launch_extend<64, PAGED>(q, k, v, o, start, counts, B, T, Smax, Hq, Hkv, outer_stride, scale, pg, stream);
}

}  // namespace

hipError_t cs_attn_extend(const void* q, const void* kc, const void* vc, const int* start, const int* counts, void* o,
                          int B, int T, int Smax, int Hq, int Hkv, int D, size_t batch_stride, float scale,
                          hipStream_t stream) {
  return extend_checked<false>(q, kc, vc, o, start, counts, B, T, Smax, Smax, Hq, Hkv, D, batch_stride, scale,
                               ExtPaged{nullptr, 0, 0, 0}, stream);
}

hipError_t cs_attn_extend_paged(const void* q, const void* kp, const void* vp, const int* table, const int* start,
                                const int* counts, void* o, int B, int T, int C, int Hq, int Hkv, int D, int pages,
                                int page, size_t page_stride, size_t table_stride, float scale, hipStream_t stream) {
  if (B == 0 || T == 0) return hipSuccess;
  if (C < 1 || page < kBN || page % kBN != 0 || (int64_t)C * page > 0x7fffffff) return hipErrorInvalidValue;
  return extend_checked<true>(q, kp, vp, o, start, counts, B, T, C * page, page, Hq, Hkv, D, page_stride, scale,
                              ExtPaged{table, table_stride, pages, page}, stream);
}
