// Causal grouped-query attention (flash style) for gfx950, bf16 in / bf16 out, f32 softmax and
// accumulation: the attention of the Llama-3 extension config (models/llama.py; BASELINE.json
// "Llama-3 8B bf16 pure data-parallel"), replacing scaled_dot_product_attention's forward and
// backward. Tensors in the model's natural [B, S, H, D] layout (no transposes); D = 64 or 128.
//
// All products are v_mfma_f32_32x32x16_bf16. The score tile is computed transposed,
// S^T = K . Q^T (keys on the accumulator rows, the query on the lane), so a query's scores sit
// in one lane pair (lane, lane ^ 32): row max / row sum are in-register plus one xor-32 shuffle.
// The accumulator then feeds the next product as its B operand with no lane movement
// (cdna_hip_programming.md §3 "An accumulator tile as the next MFMA's operand"): registers
// 8s..8s+7 of a 32x32 tile, converted to bf16, are k-step s, with k (= key) order
// 16s + 8(j>>2) + 4h + (j&3) for element j of lane half h — the A operand (V^T, K^T, dO^T, Q^T)
// is read with ds_read_b64_tr_b16 in exactly that k order from a row-major [rows][D] LDS image.
// LDS images put 16-byte chunk ch of row r at ch ^ swz(r) (guide T10 layout (b)), which serves
// both the ds_read_b128 row reads and the transposed reads.
//
// Forward: one workgroup = 4 waves = 128 queries of one (batch, head); K/V tiles of 64 keys,
// LDS-DMA-staged into a double-buffered LDS image (one barrier per tile); online softmax in
// base 2 (c = log2(e)/sqrt(D)); writes O and the row log-sum-exp L2 = m + log2(l) (base 2).
// Backward (deterministic, no float atomics):
//   attn_delta: delta = rowsum(dO * O) per (b, head, query);
//   attn_dq:    per 128-query block, like the forward: S^T, P^T, dP^T = V . dO^T,
//               dS^T = P^T (dP^T - delta), dQ^T += K^T dS^T;
//   attn_dkdv:  per 128-key block of one kv head, every query head of its group: S = Q K^T,
//               dP = dO V^T (key on the lane), dV^T += dO^T P, dK^T += Q^T dS; Q/dO tiles of 64
//               queries (+ their L2 and delta) double-buffered in LDS.
// Document mask for packed sequences (causal only): DOC variants of the forward, dQ, dK/dV and
// one-launch backward kernels, described before the forward kernel.
#include <math.h>

#include "attn_device.h"
#include "common.h"
#include "launchers.h"

namespace {

// Document mask (DOC; causal only; packed sequences): kstart[b, i] = first key query i may see,
// qend[b, j] = one past the last query that may see key j, both int32 [B, S] and non-decreasing
// along S; query i sees key j iff kstart[i] <= j <= i, i.e. j <= i < qend[j]. The values are
// clamped on load (kstart into [0, i], qend into [j + 1, S]) so that no contents can move a tile
// range outside [0, S) or leave a query without its own key. DOC = false compiles to the code
// without the mask: no extra register, no extra argument.
__device__ __forceinline__ const int* doc_ptr(const int* p) { return p; }

// Doc: empty (the plain kernel, whose signature it leaves as it was), or (const int* kstart)
template <int D, typename... Doc>
__global__ __launch_bounds__(256, 2) void attn_fwd_kernel(const __bf16* __restrict__ q, const __bf16* __restrict__ k,
                                                       const __bf16* __restrict__ v, __bf16* __restrict__ o,
                                                       float* __restrict__ lse, int S, int Hq, int Hkv, float c,
                                                       int causal, Doc... doc) {
  constexpr bool DOC = sizeof...(Doc) != 0;
  constexpr int KK = D / 16, DT = D / 32, TILE = kBN * D * 2;  // bytes of one K or V image
  extern __shared__ __attribute__((aligned(16))) char smem[];  // [2 buffers][K image, V image]
  const int nqb = (S + kBM - 1) / kBM;
  const int qb = nqb - 1 - (int)blockIdx.x;  // the longest (latest) query blocks first
  const int hq = blockIdx.y, b = blockIdx.z, hk = hq / (Hq / Hkv);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
  const int q0 = qb * kBM, q0w = q0 + 32 * w, qi = q0w + r;
  const size_t qs = (size_t)Hq * D, ks = (size_t)Hkv * D;
  const __bf16* Q = q + (size_t)b * S * qs + (size_t)hq * D;
  const __bf16* K = k + (size_t)b * S * ks + (size_t)hk * D;
  const __bf16* V = v + (size_t)b * S * ks + (size_t)hk * D;

  bf16x8 qf[KK];
#pragma unroll
  for (int kk = 0; kk < KK; ++kk) qf[kk] = gload8(Q + (size_t)qi * qs + 16 * kk + 8 * h, qi < S);
  f32x16 acc[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) acc[dt] = zero16();
  float m = -INFINITY, l = 0.f;

  const int kend = causal ? min(S, q0 + kBM) : S;
  const int nkt = (kend + kBN - 1) / kBN;
  // DOC: this lane's kstart; the wave's first / last query's (wave-uniform; the arrays are monotone,
  // so those are the wave's minimum / maximum); the block's first key tile (its first query's)
  int ksi = 0, ksw = 0, ksh = 0, kt0 = 0;
  if constexpr (DOC) {
    const int* KS = doc_ptr(doc...) + (size_t)b * S;
    const int qc = min(qi, S - 1);
    ksi = clampi(KS[qc], 0, qc);
    ksw = __builtin_amdgcn_readfirstlane(ksi);
    ksh = __builtin_amdgcn_readlane(ksi, 31);
    kt0 = clampi(KS[q0], 0, q0) / kBN;  // q0 < S; kt0 * kBN <= q0, so kt0 < nkt
  }
  const Dma<D> dk(K, ks, S), dv(V, ks, S);
  dk.issue(smem, kt0 * kBN);
  dv.issue(smem + TILE, kt0 * kBN);
  dma_barrier();
  for (int kt = kt0; kt < nkt; ++kt) {
    const int cur = DOC ? (kt - kt0) & 1 : kt & 1;  // buffer parity follows the loop's own count
    if (kt + 1 < nkt) {  // the other buffer: every wave finished reading it before the last barrier
      char* nx = smem + (cur ^ 1) * 2 * TILE;
      dk.issue(nx, (kt + 1) * kBN);
      dv.issue(nx + TILE, (kt + 1) * kBN);
    }
    const char* Kl = smem + cur * 2 * TILE;
    const char* Vl = Kl + TILE;
    const int k0 = kt * kBN;
    // wave-uniform: some key of the tile is visible to this wave (DOC: and not wholly before the
    // wave's first query's document)
    if ((!causal || k0 <= q0w + 31) && (!DOC || k0 + kBN > ksw)) {
      f32x16 s[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        s[t] = zero16();
#pragma unroll
        for (int kk = 0; kk < KK; ++kk) s[t] = mfma(row_frag<D>(Kl, 32 * t + r, kk, h), qf[kk], s[t]);
      }
      const bool edge = (causal && k0 + kBN - 1 > q0w) || k0 + kBN > S || (DOC && k0 < ksh);
      float mx = -INFINITY;
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          float x = s[t][e] * c;
          if (edge) {
            const int key = k0 + 32 * t + acc_row(e, h);
            if ((causal && key > qi) || key >= S || (DOC && key < ksi)) x = -INFINITY;
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
  }
  if (qi < S) {
    store_rowT<D>(acc, l > 0.f ? 1.f / l : 0.f, o + ((size_t)b * S + qi) * qs + (size_t)hq * D, h);
    if (h == 0) lse[((size_t)b * Hq + hq) * S + qi] = m + __log2f(l);
  }
}

// delta[b, h, q] = sum_d dO * O (f32), one 16-lane group per (b, q, h) row
template <int D>
__global__ __launch_bounds__(256) void attn_delta_kernel(const __bf16* __restrict__ o, const __bf16* __restrict__ dout,
                                                         float* __restrict__ delta, int B, int S, int H) {
  const int row = blockIdx.x * 16 + (threadIdx.x >> 4), l16 = threadIdx.x & 15;
  const int rows = B * S * H;
  float s = 0.f;
  if (row < rows) {
    const __bf16* op = o + (size_t)row * D;
    const __bf16* gp = dout + (size_t)row * D;
    for (int d = 8 * l16; d < D; d += 128) {
      const bf16x8 a = *reinterpret_cast<const bf16x8*>(op + d);
      const bf16x8 g = *reinterpret_cast<const bf16x8*>(gp + d);
#pragma unroll
      for (int j = 0; j < 8; ++j) s += (float)a[j] * (float)g[j];
    }
  }
#pragma unroll
  for (int x = 8; x >= 1; x >>= 1) s += __shfl_xor(s, x, 16);
  if (row < rows && l16 == 0) {
    const int hh = row % H, bq = row / H, qq = bq % S, bb = bq / S;
    delta[((size_t)bb * H + hh) * S + qq] = s;
  }
}

template <int D, bool DOC>
__device__ __forceinline__ void dq_body(const __bf16* __restrict__ q, const __bf16* __restrict__ k,
                                                      const __bf16* __restrict__ v, const __bf16* __restrict__ dout,
                                                      const float* __restrict__ lse, const float* __restrict__ delta,
                                                      __bf16* __restrict__ dq, int S, int Hq, int Hkv, float c,
                                                      float scale, int causal, int bx, int by, int bz,
                                                      const int* __restrict__ kstart) {
  constexpr int KK = D / 16, DT = D / 32, TILE = kBN * D * 2;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int nqb = (S + kBM - 1) / kBM;
  const int qb = nqb - 1 - bx;
  const int hq = by, b = bz, hk = hq / (Hq / Hkv);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
  const int q0 = qb * kBM, q0w = q0 + 32 * w, qi = q0w + r;
  const size_t qs = (size_t)Hq * D, ks = (size_t)Hkv * D;
  const size_t qrow = ((size_t)b * S + qi) * qs + (size_t)hq * D;
  const __bf16* K = k + (size_t)b * S * ks + (size_t)hk * D;
  const __bf16* V = v + (size_t)b * S * ks + (size_t)hk * D;
  bf16x8 qf[KK], gf[KK];
#pragma unroll
  for (int kk = 0; kk < KK; ++kk) {
    qf[kk] = gload8(q + qrow + 16 * kk + 8 * h, qi < S);
    gf[kk] = gload8(dout + qrow + 16 * kk + 8 * h, qi < S);
  }
  const size_t st = ((size_t)b * Hq + hq) * S + qi;
  const float L2 = qi < S ? lse[st] : 0.f, dl = qi < S ? delta[st] : 0.f;
  f32x16 acc[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) acc[dt] = zero16();

  const int kend = causal ? min(S, q0 + kBM) : S;
  const int nkt = (kend + kBN - 1) / kBN;
  int ksi = 0, ksw = 0, ksh = 0, kt0 = 0;  // DOC: as in the forward
  if constexpr (DOC) {
    const int* KS = kstart + (size_t)b * S;
    const int qc = min(qi, S - 1);
    ksi = clampi(KS[qc], 0, qc);
    ksw = __builtin_amdgcn_readfirstlane(ksi);
    ksh = __builtin_amdgcn_readlane(ksi, 31);
    kt0 = clampi(KS[q0], 0, q0) / kBN;
  }
  const Dma<D> dmk(K, ks, S), dmv(V, ks, S);
  dmk.issue(smem, kt0 * kBN);
  dmv.issue(smem + TILE, kt0 * kBN);
  dma_barrier();
  for (int kt = kt0; kt < nkt; ++kt) {
    const int cur = DOC ? (kt - kt0) & 1 : kt & 1;
    if (kt + 1 < nkt) {
      char* nx = smem + (cur ^ 1) * 2 * TILE;
      dmk.issue(nx, (kt + 1) * kBN);
      dmv.issue(nx + TILE, (kt + 1) * kBN);
    }
    const char* Kl = smem + cur * 2 * TILE;
    const char* Vl = Kl + TILE;
    const int k0 = kt * kBN;
    // one 32-key half of the tile at a time (no running max here: P = exp2(S c - L2) is final),
    // which keeps two score tiles live instead of four: two waves per SIMD fit
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      if (causal && k0 + 32 * t > q0w + 31) continue;  // wave-uniform: the half is above the diagonal
      if (DOC && k0 + 32 * t + 32 <= ksw) continue;     // ... or wholly before the wave's first document
      f32x16 s = zero16(), dp = zero16();
#pragma unroll
      for (int kk = 0; kk < KK; ++kk) {
        s = mfma(row_frag<D>(Kl, 32 * t + r, kk, h), qf[kk], s);
        dp = mfma(row_frag<D>(Vl, 32 * t + r, kk, h), gf[kk], dp);
      }
      const bool edge = (causal && k0 + 32 * t + 31 > q0w) || k0 + 32 * t + 32 > S || (DOC && k0 + 32 * t < ksh);
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        float p = __builtin_amdgcn_exp2f(s[e] * c - L2);
        if (edge) {
          const int key = k0 + 32 * t + acc_row(e, h);
          if ((causal && key > qi) || key >= S || (DOC && key < ksi)) p = 0.f;
        }
        s[e] = p * (dp[e] - dl);  // dS^T
      }
#pragma unroll
      for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int ss = 0; ss < 2; ++ss)
          acc[dt] = mfma(tr_frag<D>(Kl, 32 * t + 16 * ss, 32 * dt, lane), acc_frag(s, ss), acc[dt]);
    }
    dma_barrier();
  }
  if (qi < S) store_rowT<D>(acc, scale, dq + qrow, h);
}

template <int D>
__global__ __launch_bounds__(256, 2) void attn_dq_kernel(const __bf16* __restrict__ q, const __bf16* __restrict__ k,
                                                      const __bf16* __restrict__ v, const __bf16* __restrict__ dout,
                                                      const float* __restrict__ lse, const float* __restrict__ delta,
                                                      __bf16* __restrict__ dq, int S, int Hq, int Hkv, float c,
                                                      float scale, int causal) {
  dq_body<D, false>(q, k, v, dout, lse, delta, dq, S, Hq, Hkv, c, scale, causal, blockIdx.x, blockIdx.y, blockIdx.z,
                    nullptr);
}

template <int D>
__global__ __launch_bounds__(256, 2) void attn_dq_doc_kernel(const __bf16* __restrict__ q, const __bf16* __restrict__ k,
                                                          const __bf16* __restrict__ v, const __bf16* __restrict__ dout,
                                                          const float* __restrict__ lse, const float* __restrict__ delta,
                                                          __bf16* __restrict__ dq, int S, int Hq, int Hkv, float c,
                                                          float scale, const int* __restrict__ kstart) {
  dq_body<D, true>(q, k, v, dout, lse, delta, dq, S, Hq, Hkv, c, scale, 1, blockIdx.x, blockIdx.y, blockIdx.z, kstart);
}

template <int D, bool DOC>
__device__ __forceinline__ void dkdv_body(const __bf16* __restrict__ q, const __bf16* __restrict__ k,
                                                        const __bf16* __restrict__ v, const __bf16* __restrict__ dout,
                                                        const float* __restrict__ lse, const float* __restrict__ delta,
                                                        __bf16* __restrict__ dk, __bf16* __restrict__ dv, int S, int Hq,
                                                        int Hkv, float c, float scale, int causal, int bx, int by, int bz,
                                                        const int* __restrict__ qend) {
  constexpr int KK = D / 16, DT = D / 32, TILE = kBN * D * 2;
  // [2 buffers][Q image, dO image, L2[64], delta[64]]
  constexpr int BUF = 2 * TILE + 2 * kBN * 4;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int nkb = (S + kBM - 1) / kBM;
  const int kb = causal ? bx : nkb - 1 - bx;  // causal: early keys see the most queries
  const int hk = by, b = bz, grp = Hq / Hkv;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
  const int kw0 = kb * kBM + 32 * w, kj = kw0 + r;  // this lane's key (the accumulator column)
  const size_t qs = (size_t)Hq * D, ks = (size_t)Hkv * D;
  const size_t krow = ((size_t)b * S + kj) * ks + (size_t)hk * D;
  bf16x8 kf[KK], vf[KK];
#pragma unroll
  for (int kk = 0; kk < KK; ++kk) {
    kf[kk] = gload8(k + krow + 16 * kk + 8 * h, kj < S);
    vf[kk] = gload8(v + krow + 16 * kk + 8 * h, kj < S);
  }
  f32x16 adk[DT], adv[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) {
    adk[dt] = zero16();
    adv[dt] = zero16();
  }
  // query tiles of 64: from the block's first key (causal) to the end, for every head of the group
  const int qt0 = causal ? (kb * kBM) / kBN : 0;
  // DOC: this lane's qend; the wave's last key's (wave-uniform, the wave's maximum); the query range
  // ends with the document of the block's last key
  int qej = S, qew = S, qlim = S;
  if constexpr (DOC) {
    const int* QE = qend + (size_t)b * S;
    const int kc = min(kj, S - 1), kl = min(kb * kBM + kBM - 1, S - 1);
    qej = clampi(QE[kc], kc + 1, S);
    qew = __builtin_amdgcn_readlane(qej, 31);
    qlim = clampi(QE[kl], kl + 1, S);  // > kb * kBM: at least one query tile
  }
  const int nqt = (qlim + kBN - 1) / kBN - qt0;
  const int total = nqt * grp;
  // Q / dO tiles by LDS-DMA; L2 / delta (64 floats each) through registers
  auto store = [&](int it, int buf) {
    char* base = smem + buf * BUF;
    {
      const int hq = hk * grp + it / nqt, q0 = (qt0 + it % nqt) * kBN;
      const Dma<D> dq_(q + (size_t)b * S * qs + (size_t)hq * D, qs, S), dg(dout + (size_t)b * S * qs + (size_t)hq * D, qs, S);
      dq_.issue(base, q0);
      dg.issue(base + TILE, q0);
    }
    if (threadIdx.x < 2 * kBN) {  // L2 and delta of the tile's 64 queries
      const int hq = hk * grp + it / nqt, q0 = (qt0 + it % nqt) * kBN;
      const int qq = q0 + (threadIdx.x & (kBN - 1));
      const float* src = threadIdx.x < kBN ? lse : delta;
      reinterpret_cast<float*>(base + 2 * TILE)[threadIdx.x] =
          qq < S ? src[((size_t)b * Hq + hq) * S + qq] : 0.f;
    }
  };
  if (total > 0) store(0, 0);
  dma_barrier();
  for (int it = 0; it < total; ++it) {
    const int cur = it & 1;
    if (it + 1 < total) store(it + 1, cur ^ 1);  // the other buffer: its readers passed the last barrier
    const char* Ql = smem + cur * BUF;
    const char* Gl = Ql + TILE;
    const float* L2s = reinterpret_cast<const float*>(Ql + 2 * TILE);
    const float* Dls = L2s + kBN;
    const int q0 = (qt0 + it % nqt) * kBN;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int qu = q0 + 32 * u;  // this 32-query slice
      if (causal && qu + 31 < kw0) continue;  // wave-uniform: every query precedes this wave's keys
      if (qu >= S) continue;
      if (DOC && qu >= qew) continue;  // wave-uniform: every query is past this wave's last document
      f32x16 s = zero16(), dp = zero16();
#pragma unroll
      for (int kk = 0; kk < KK; ++kk) {
        s = mfma(row_frag<D>(Ql, 32 * u + r, kk, h), kf[kk], s);
        dp = mfma(row_frag<D>(Gl, 32 * u + r, kk, h), vf[kk], dp);
      }
      // rows = queries (registers), column = this lane's key
      f32x16 ds;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int qr = 32 * u + acc_row(e, h), qq = q0 + qr;
        float p = __builtin_amdgcn_exp2f(s[e] * c - L2s[qr]);
        if ((causal && kj > qq) || qq >= S || kj >= S || (DOC && qq >= qej)) p = 0.f;
        s[e] = p;
        ds[e] = p * (dp[e] - Dls[qr]);
      }
#pragma unroll
      for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int ss = 0; ss < 2; ++ss) {
          adv[dt] = mfma(tr_frag<D>(Gl, 32 * u + 16 * ss, 32 * dt, lane), acc_frag(s, ss), adv[dt]);
          adk[dt] = mfma(tr_frag<D>(Ql, 32 * u + 16 * ss, 32 * dt, lane), acc_frag(ds, ss), adk[dt]);
        }
    }
    dma_barrier();
  }
  if (kj < S) {
    store_rowT<D>(adk, scale, dk + krow, h);
    store_rowT<D>(adv, 1.f, dv + krow, h);
  }
}

template <int D>
__global__ __launch_bounds__(256) void attn_dkdv_kernel(const __bf16* __restrict__ q, const __bf16* __restrict__ k,
                                                        const __bf16* __restrict__ v, const __bf16* __restrict__ dout,
                                                        const float* __restrict__ lse, const float* __restrict__ delta,
                                                        __bf16* __restrict__ dk, __bf16* __restrict__ dv, int S, int Hq,
                                                        int Hkv, int B, float c, float scale, int causal) {
  // 1-D grid, key block slowest-varying: every head's heaviest (earliest, causal) key blocks dispatch
  // first. At one wave per SIMD (356 VGPR+AGPR) the 512 blocks of the Llama-3-8B shape run in two
  // rounds on 256 CUs; heaviest-first keeps the second round from starting with a 16x-longer block.
  const int L = (int)blockIdx.x;
  dkdv_body<D, false>(q, k, v, dout, lse, delta, dk, dv, S, Hq, Hkv, c, scale, causal, L / (Hkv * B), L % Hkv,
                      (L / Hkv) % B, nullptr);
}

template <int D>
__global__ __launch_bounds__(256) void attn_dkdv_doc_kernel(const __bf16* __restrict__ q, const __bf16* __restrict__ k,
                                                            const __bf16* __restrict__ v,
                                                            const __bf16* __restrict__ dout,
                                                            const float* __restrict__ lse,
                                                            const float* __restrict__ delta, __bf16* __restrict__ dk,
                                                            __bf16* __restrict__ dv, int S, int Hq, int Hkv, int B,
                                                            float c, float scale, const int* __restrict__ qend) {
  const int L = (int)blockIdx.x;  // the same order as attn_dkdv_kernel
  dkdv_body<D, true>(q, k, v, dout, lse, delta, dk, dv, S, Hq, Hkv, c, scale, 1, L / (Hkv * B), L % Hkv,
                     (L / Hkv) % B, qend);
}

// Causal backward in ONE launch: the dK/dV blocks first (key block ascending = most query tiles
// first), then the dQ blocks (latest query block first). A dK/dV block of an early key block
// walks up to 16x the query tiles of a late one, so run alone that kernel leaves most CUs idle
// in its tail; here the dQ blocks (independent: they write only dQ) fill those CUs as the short
// dK/dV blocks retire. Same bodies, same arithmetic, same results as the two launches.
template <int D>
__global__ __launch_bounds__(256) void attn_bwd_fused_kernel(const __bf16* __restrict__ q, const __bf16* __restrict__ k,
                                                             const __bf16* __restrict__ v,
                                                             const __bf16* __restrict__ dout,
                                                             const float* __restrict__ lse,
                                                             const float* __restrict__ delta, __bf16* __restrict__ dq,
                                                             __bf16* __restrict__ dk, __bf16* __restrict__ dv, int S,
                                                             int Hq, int Hkv, int B, float c, float scale, int causal) {
  const int nb = (S + kBM - 1) / kBM;
  const int n_kv = nb * Hkv * B;
  int L = (int)blockIdx.x;
  if (L < n_kv) {  // key block slowest-varying: all heads' heaviest key blocks dispatch first
    dkdv_body<D, false>(q, k, v, dout, lse, delta, dk, dv, S, Hq, Hkv, c, scale, causal, L / (Hkv * B), L % Hkv,
                        (L / Hkv) % B, nullptr);
  } else {
    L -= n_kv;
    dq_body<D, false>(q, k, v, dout, lse, delta, dq, S, Hq, Hkv, c, scale, causal, L / (Hq * B), L % Hq,
                      (L / Hq) % B, nullptr);
  }
}

// The document-masked backward in one launch: the same bodies in the same block order. With
// documents of uneven length "key block ascending" is no longer "heaviest first" (a key block's
// work ends with its document); the order is not re-balanced for that.
template <int D>
__global__ __launch_bounds__(256) void attn_bwd_fused_doc_kernel(
    const __bf16* __restrict__ q, const __bf16* __restrict__ k, const __bf16* __restrict__ v,
    const __bf16* __restrict__ dout, const float* __restrict__ lse, const float* __restrict__ delta,
    __bf16* __restrict__ dq, __bf16* __restrict__ dk, __bf16* __restrict__ dv, int S, int Hq, int Hkv, int B, float c,
    float scale, const int* __restrict__ kstart, const int* __restrict__ qend) {
  const int nb = (S + kBM - 1) / kBM;
  const int n_kv = nb * Hkv * B;
  int L = (int)blockIdx.x;
  if (L < n_kv) {
    dkdv_body<D, true>(q, k, v, dout, lse, delta, dk, dv, S, Hq, Hkv, c, scale, 1, L / (Hkv * B), L % Hkv,
                       (L / Hkv) % B, qend);
  } else {
    L -= n_kv;
    dq_body<D, true>(q, k, v, dout, lse, delta, dq, S, Hq, Hkv, c, scale, 1, L / (Hq * B), L % Hq, (L / Hq) % B,
                     kstart);
  }
}

// The causal backward runs as one launch (attn_bwd_fused_kernel) by default; CS_ATTN_BWD_FUSED=0 gives
// dQ then dK/dV (heaviest-first grid). Llama-3-8B step on MI355X: two launches in grid order 18.79k
// tokens/s (dK/dV 1156 us), heaviest-first 19.76k (dK/dV 645 us), one launch 20.12k.
bool attn_bwd_fused() {
  static const bool on = [] {
    const char* e = getenv("CS_ATTN_BWD_FUSED");
    return e == nullptr || atoi(e) != 0;
  }();
  return on;
}

template <int D>
size_t fwd_lds() { return 2 * 2 * (size_t)kBN * D * 2; }
template <int D>
size_t dkdv_lds() { return 2 * (2 * (size_t)kBN * D * 2 + 2 * kBN * 4); }

template <int D>
hipError_t launch_fwd(const void* q, const void* k, const void* v, void* o, float* lse, int B, int S, int Hq, int Hkv,
                      float scale, int causal, hipStream_t st) {
  const dim3 grid((S + kBM - 1) / kBM, Hq, B);
  hipLaunchKernelGGL(attn_fwd_kernel<D>, grid, dim3(256), fwd_lds<D>(), st, (const __bf16*)q, (const __bf16*)k,
                     (const __bf16*)v, (__bf16*)o, lse, S, Hq, Hkv, scale * 1.4426950408889634f, causal);
  return hipGetLastError();
}

template <int D>
hipError_t launch_fwd_doc(const void* q, const void* k, const void* v, void* o, float* lse, int B, int S, int Hq,
                          int Hkv, float scale, const int* kstart, hipStream_t st) {
  const dim3 grid((S + kBM - 1) / kBM, Hq, B);
  hipLaunchKernelGGL((attn_fwd_kernel<D, const int*>), grid, dim3(256), fwd_lds<D>(), st, (const __bf16*)q,
                     (const __bf16*)k, (const __bf16*)v, (__bf16*)o, lse, S, Hq, Hkv, scale * 1.4426950408889634f, 1,
                     kstart);
  return hipGetLastError();
}

template <int D>
hipError_t launch_bwd(const void* q, const void* k, const void* v, const void* o, const void* dout, const float* lse,
                      float* delta, void* dq, void* dk, void* dv, int B, int S, int Hq, int Hkv, float scale, int causal,
                      hipStream_t st) {
  const int rows = B * S * Hq;
  hipLaunchKernelGGL(attn_delta_kernel<D>, dim3((rows + 15) / 16), dim3(256), 0, st, (const __bf16*)o,
                     (const __bf16*)dout, delta, B, S, Hq);
  const float c = scale * 1.4426950408889634f;
  const int nb = (S + kBM - 1) / kBM;
  if (causal && attn_bwd_fused()) {
    const size_t lds = dkdv_lds<D>() > fwd_lds<D>() ? dkdv_lds<D>() : fwd_lds<D>();
    hipLaunchKernelGGL(attn_bwd_fused_kernel<D>, dim3(nb * (Hkv + Hq) * B), dim3(256), lds, st, (const __bf16*)q,
                       (const __bf16*)k, (const __bf16*)v, (const __bf16*)dout, lse, delta, (__bf16*)dq, (__bf16*)dk,
                       (__bf16*)dv, S, Hq, Hkv, B, c, scale, causal);
    return hipGetLastError();
  }
  hipLaunchKernelGGL(attn_dq_kernel<D>, dim3(nb, Hq, B), dim3(256), fwd_lds<D>(), st,
                     (const __bf16*)q, (const __bf16*)k, (const __bf16*)v, (const __bf16*)dout, lse, delta,
                     (__bf16*)dq, S, Hq, Hkv, c, scale, causal);
  hipLaunchKernelGGL(attn_dkdv_kernel<D>, dim3(nb * Hkv * B), dim3(256), dkdv_lds<D>(), st,
                     (const __bf16*)q, (const __bf16*)k, (const __bf16*)v, (const __bf16*)dout, lse, delta,
                     (__bf16*)dk, (__bf16*)dv, S, Hq, Hkv, B, c, scale, causal);
  return hipGetLastError();
}

template <int D>
hipError_t launch_bwd_doc(const void* q, const void* k, const void* v, const void* o, const void* dout,
                          const float* lse, float* delta, void* dq, void* dk, void* dv, int B, int S, int Hq, int Hkv,
                          float scale, const int* kstart, const int* qend, hipStream_t st) {
  const int rows = B * S * Hq;
  hipLaunchKernelGGL(attn_delta_kernel<D>, dim3((rows + 15) / 16), dim3(256), 0, st, (const __bf16*)o,
                     (const __bf16*)dout, delta, B, S, Hq);
  const float c = scale * 1.4426950408889634f;
  const int nb = (S + kBM - 1) / kBM;
  if (attn_bwd_fused()) {
    const size_t lds = dkdv_lds<D>() > fwd_lds<D>() ? dkdv_lds<D>() : fwd_lds<D>();
    hipLaunchKernelGGL(attn_bwd_fused_doc_kernel<D>, dim3(nb * (Hkv + Hq) * B), dim3(256), lds, st, (const __bf16*)q,
                       (const __bf16*)k, (const __bf16*)v, (const __bf16*)dout, lse, delta, (__bf16*)dq, (__bf16*)dk,
                       (__bf16*)dv, S, Hq, Hkv, B, c, scale, kstart, qend);
    return hipGetLastError();
  }
  hipLaunchKernelGGL(attn_dq_doc_kernel<D>, dim3(nb, Hq, B), dim3(256), fwd_lds<D>(), st, (const __bf16*)q,
                     (const __bf16*)k, (const __bf16*)v, (const __bf16*)dout, lse, delta, (__bf16*)dq, S, Hq, Hkv, c,
                     scale, kstart);
  hipLaunchKernelGGL(attn_dkdv_doc_kernel<D>, dim3(nb * Hkv * B), dim3(256), dkdv_lds<D>(), st, (const __bf16*)q,
                     (const __bf16*)k, (const __bf16*)v, (const __bf16*)dout, lse, delta, (__bf16*)dk, (__bf16*)dv, S,
                     Hq, Hkv, B, c, scale, qend);
  return hipGetLastError();
}

}  // namespace

hipError_t cs_attn_fwd(const void* q, const void* k, const void* v, void* o, float* lse, int B, int S, int Hq, int Hkv,
                       int D, float scale, int causal, hipStream_t stream) {
  if (B == 0 || S == 0) return hipSuccess;
  if (D == 128) return launch_fwd<128>(q, k, v, o, lse, B, S, Hq, Hkv, scale, causal, stream);
  if (D == 64) return launch_fwd<64>(q, k, v, o, lse, B, S, Hq, Hkv, scale, causal, stream);
  return hipErrorInvalidValue;
}

hipError_t cs_attn_bwd(const void* q, const void* k, const void* v, const void* o, const void* dout, const float* lse,
                       float* delta, void* dq, void* dk, void* dv, int B, int S, int Hq, int Hkv, int D, float scale,
                       int causal, hipStream_t stream) {
  if (B == 0 || S == 0) return hipSuccess;
  if (D == 128) return launch_bwd<128>(q, k, v, o, dout, lse, delta, dq, dk, dv, B, S, Hq, Hkv, scale, causal, stream);
  if (D == 64) return launch_bwd<64>(q, k, v, o, dout, lse, delta, dq, dk, dv, B, S, Hq, Hkv, scale, causal, stream);
  return hipErrorInvalidValue;
}

hipError_t cs_attn_fwd_doc(const void* q, const void* k, const void* v, void* o, float* lse, int B, int S, int Hq,
                           int Hkv, int D, float scale, const int* kstart, hipStream_t stream) {
  if (B == 0 || S == 0) return hipSuccess;
  if (kstart == nullptr) return hipErrorInvalidValue;
  if (D == 128) return launch_fwd_doc<128>(q, k, v, o, lse, B, S, Hq, Hkv, scale, kstart, stream);
  if (D == 64) return launch_fwd_doc<64>(q, k, v, o, lse, B, S, Hq, Hkv, scale, kstart, stream);
  return hipErrorInvalidValue;
}

hipError_t cs_attn_bwd_doc(const void* q, const void* k, const void* v, const void* o, const void* dout,
                           const float* lse, float* delta, void* dq, void* dk, void* dv, int B, int S, int Hq, int Hkv,
                           int D, float scale, const int* kstart, const int* qend, hipStream_t stream) {
  if (B == 0 || S == 0) return hipSuccess;
  if (kstart == nullptr || qend == nullptr) return hipErrorInvalidValue;
  if (D == 128)
    return launch_bwd_doc<128>(q, k, v, o, dout, lse, delta, dq, dk, dv, B, S, Hq, Hkv, scale, kstart, qend, stream);
  if (D == 64)
    return launch_bwd_doc<64>(q, k, v, o, dout, lse, delta, dq, dk, dv, B, S, Hq, Hkv, scale, kstart, qend, stream);
  return hipErrorInvalidValue;
}
