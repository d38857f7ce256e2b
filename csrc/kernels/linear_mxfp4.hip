// MXFP4 weight-only linear for decoding on gfx950 (W4A16, skinny M):
//   y[M, N] = x[M, K] . W^T,  W[c][k] = e2m1(codes[c][k]) * 2^(scales[c][k / 32] - 127)
// x bf16 (rows ldx elements apart, unit inner stride); codes uint8 [N, K / 2] (rows ldw bytes apart), two OCP
// e2m1 codes per byte, element 2 i in the low nibble and 2 i + 1 in the high one, values +-{0, .5, 1, 1.5, 2, 3, 4,
// 6}; scales uint8 [N, K / 32] (rows lds bytes apart), one e8m0 exponent per block of 32 consecutive k of a row;
// y bf16 [M, N] contiguous. 1 <= M <= 64, K % 128 == 0, N % 8 == 0. A code has 2 significant bits and a scale is a
// power of two, so every dequantised weight is exactly a bf16 number (the quantiser keeps the exponent in
// [-125, 125]: normal numbers only) and every product x * W is exact in fp32: the only roundings are the fp32
// sums and the final bf16 store. The block scale varies along K, so it is folded into the MFMA operand; nothing is
// scaled after the sum.
//
// The product is bound by the weight bytes (half of linear_fp8.hip's): each is read from HBM once per call, 16
// bytes per lane, straight into registers, dequantised there to bf16 and multiplied on v_mfma_f32_16x16x32_bf16.
//
// Lane maps (lane = 16 g + n, g = lane / 16 in 0..3, n = lane % 16), for the chunk at k0 = 128 * chunk:
//   weights  lane (n, g) loads the 16 bytes 64 chunk + 16 g .. + 15 of channel c0 + n (one uint4): the 32 codes
//            k0 + 32 g .. k0 + 32 g + 31, exactly one scale block. Dword s of it (8 codes) feeds MFMA K-step s:
//            in step s the lane's eight A-operand values are k = k0 + 32 g + 8 s + j, j = 0..7, nibble j of the
//            dword. (The MFMA calls them k' = 8 g + j and only sums over them, so any assignment of real k to
//            (g, s, j) is right as long as both operands use it.)
//   scale    lane (n, g) needs the one byte scales[c0 + n][4 chunk + g]: see "Scale path".
//   x        lane (n, g) holds row m = 16 mb + n of x for block mb: four uint4 loads of eight bf16,
//            k = k0 + 32 g + 8 s + j for s = 0..3: the same (g, s, j) -> k map.
//   product  acc = mfma(A = weights, B = x): register j of lane (n, g) is y[m = 16 mb + n][c0 + 4 g + j]: four
//            consecutive channels of one row, one 8-byte bf16 store (or one 16-byte fp32 store to the workspace).
//
// Dequantisation: v_cvt_scalef32_pk_bf16_fp4 converts the two codes of one byte of a dword (low nibble into the
// low half) and multiplies by an fp32 scale, here (byte << 23) reinterpreted: 2^(byte - 127). Four calls per
// K-step fragment, 16 per weight load.
//
// Scale path: a one-byte global load per lane, issued together with the lane's weight load. Its address depends
// on the chunk index only (not on the weight data), so both loads of a chunk, and those of the second chunk of a
// trip, are in flight before the first MFMA: it is not a dependent load in front of the chunk. The four lane
// groups of a channel read four neighbouring bytes and the 16 channels of a tile 16 rows, so a wave's request is
// 16 short segments; a row's scales for 4096 k are one 128-byte line that the row's later chunks hit in L1 / L2.
// Against the alternatives: a dword shared by the four lane groups is the same number of load instructions per
// lane plus a shift by 8 g, and staging a slab's scales in LDS costs a barrier per slab where a slab is often a
// single chunk per wave (K 4096 in 8 slabs).
//
// Work split (linear_fp8.hip's). A workgroup is 4 waves and owns kNT = 2 tiles of 16 output channels over a run
// of K. K is cut into chunks of 128; the chunks are divided, as evenly as possible, into `slabs` contiguous
// slabs, and the slabs into the gridDim.y workgroups of a channel-tile pair. Inside a slab, wave w takes chunks
// w, w + 4, ... and accumulates them in one MFMA chain, two chunks per trip of its loop; the four waves are then
// summed through LDS in wave order. With slabs == 1 that sum is stored as y. Otherwise it is the fp32 partial
// ws[slab][M][Ntot], and linear_mxfp4_combine_kernel sums the slabs of an element in slab order and stores. The
// slab count comes from the shapes and the CU count only and it alone fixes the summation tree; how many
// workgroups share the slabs (`wgs`, the caller's `splits`) moves work and changes no bit. No atomics, no arrival
// counters. Two tiles, not four: docs/linear_mxfp4.md, "Tile count".
//
// One kernel, three entries. linear_mxfp4_kernel<MB, Epi> reads a by-value table of 1 to 3 segments (weights that
// share x). kStore: blockIdx.x runs over the 32-channel tile pairs of all segments, a workgroup finds its segment
// from blockIdx.x alone and stores its own channels: the plain call is a group of one. kSwiglu: segment 0 is the
// gate and segment 1 the up weight, tile 0 is gate channels [c, c + 16) and tile 1 up channels [c, c + 16); both
// sums are rounded to bf16 and lm.hip's SwiGLU expression applied, in the epilogue or in the combine. Per output
// element the chunks, the MFMA chain, the wave order and the slab order are the same in every mode, so at equal
// `slabs` the grouped and the paired results have the bits of the composition of plain calls.
//
// Rows >= M and channels >= N are clamped onto the last row for the loads (in bounds, unconditional) and never
// stored: an MFMA output depends on one A row and one B column only.
#include "common.h"
#include "launchers.h"
#include "mxfp4_dequant_device.h"

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int kKC = 128;        // K per chunk: 16 bytes (32 codes, one scale block) in each of the four lane groups
constexpr int kWaves = 4;       // waves per workgroup, interleaved over the chunks of a slab
constexpr int kNT = 2;          // 16-channel tiles per workgroup
constexpr int kCT = 16 * kNT;   // channels per workgroup (kStore)
constexpr int kMaxM = 64;
constexpr int kMinChunks = 2;   // chunks per slab the heuristic keeps
constexpr int kMaxSlabs = 64;
constexpr int kMaxGroup = 3;    // weights of one grouped launch (q, k and v)
enum Epi { kStore = 0, kSwiglu = 1 };

// one weight of a launch
struct Segment {
  const unsigned char* codes;   // [N, K / 2], rows ldw bytes apart
  const unsigned char* scales;  // [N, K / 32], rows lds bytes apart
  __bf16* y;                    // [M, N] contiguous (kSwiglu: segment 0's is the output, segment 1's unused)
  size_t ldw, lds;
  int N, tile0, col0;           // first tile pair (kStore) and first workspace column of the segment
};
struct Group {
  Segment seg[kMaxGroup];
  int G, Ntot;  // Ntot: workspace columns, the summed N
};

using cs::dequant8;  // mxfp4_dequant_device.h

// the chunks [c0, c1) of part i when n chunks are divided as evenly as possible into parts
__device__ __forceinline__ void even_part(int n, int parts, int i, int& c0, int& c1) {
  const int base = n / parts, rem = n % parts;
  c0 = i * base + (i < rem ? i : rem);
  c1 = c0 + base + (i < rem ? 1 : 0);
}

// what a lane holds of one chunk: 32 codes and their scale byte for each of its kNT channels, 32 bf16 of each of
// its MB rows of x
template <int MB>
struct Chunk {
  uint4 wq[kNT], xq[MB][4];
  unsigned sc[kNT];
  __device__ __forceinline__ void load(const unsigned char* const (&wrow)[kNT], const unsigned char* const (&srow)[kNT],
                                       const __bf16* const (&xrow)[MB], size_t c) {
    // c < K / 128: code bytes 64 c + 16 g .. + 15 < K / 2, scale byte 4 c + g < K / 32, x 128 c + 32 g + 31 < K
#pragma unroll
    for (int nt = 0; nt < kNT; ++nt) {
      wq[nt] = *reinterpret_cast<const uint4*>(wrow[nt] + c * (kKC / 2));
      sc[nt] = srow[nt][c * (kKC / 32)];
    }
#pragma unroll
    for (int mb = 0; mb < MB; ++mb)
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) xq[mb][ks] = *reinterpret_cast<const uint4*>(xrow[mb] + c * kKC + 8 * ks);
  }
  __device__ __forceinline__ void mma(f32x4 (&acc)[MB][kNT]) const {
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      bf16x8 wf[kNT];
#pragma unroll
      for (int nt = 0; nt < kNT; ++nt) {
        const unsigned d = ks == 0 ? wq[nt].x : ks == 1 ? wq[nt].y : ks == 2 ? wq[nt].z : wq[nt].w;
        wf[nt] = dequant8(d, __uint_as_float(sc[nt] << 23));
      }
#pragma unroll
      for (int mb = 0; mb < MB; ++mb) {
        const bf16x8 xf = __builtin_bit_cast(bf16x8, xq[mb][ks]);
#pragma unroll
        for (int nt = 0; nt < kNT; ++nt)
          acc[mb][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[nt], xf, acc[mb][nt], 0, 0, 0);
      }
    }
  }
};

// the sum of the four waves' stages of one accumulator quad, in wave order
template <int MB>
__device__ __forceinline__ f32x4 wave_sum(const f32x4 (&sm)[kWaves][MB * kNT][64], int f, int l) {
  f32x4 v = sm[0][f][l];
#pragma unroll
  for (int w = 1; w < kWaves; ++w) v += sm[w][f][l];
  return v;
}

__device__ __forceinline__ bf16x4 to_bf16(f32x4 v) {
  return bf16x4{(__bf16)v[0], (__bf16)v[1], (__bf16)v[2], (__bf16)v[3]};
}

// four outputs from the fp32 sums of four gate and four up channels: both rounded to bf16 as the plain store
// rounds them, then swiglu_fwd_kernel's expression (lm.hip)
__device__ __forceinline__ bf16x4 swiglu4(f32x4 gv, f32x4 uv) {
  bf16x4 o;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float a = (float)(__bf16)gv[j], b = (float)(__bf16)uv[j];
    o[j] = (__bf16)(a * (1.f / (1.f + __expf(-a))) * b);
  }
  return o;
}

template <int MB, int E>
__global__ __launch_bounds__(64 * kWaves) void linear_mxfp4_kernel(const __bf16* __restrict__ x, const Group grp,
                                                                   float* __restrict__ ws, int M, int K, size_t ldx,
                                                                   int slabs) {
  __shared__ f32x4 sm[kWaves][MB * kNT][64];
  const int tid = threadIdx.x, lane = tid & 63, n = lane & 15, g = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // wave-uniform: the chunk loop is scalar control flow

  // kStore: the last segment that starts at or before this tile pair (an unused table entry is never looked at);
  // kSwiglu: segment 0, the gate, whose N and y are the launch's
  Segment sg = grp.seg[0];
  if (E == kStore) {
#pragma unroll
    for (int i = 1; i < kMaxGroup; ++i)
      if (i < grp.G && (int)blockIdx.x >= grp.seg[i].tile0) sg = grp.seg[i];
  }
  const int N = sg.N;
  const int ch0 = E == kStore ? ((int)blockIdx.x - sg.tile0) * kCT : (int)blockIdx.x * 16;

  const unsigned char* wrow[kNT];
  const unsigned char* srow[kNT];
  const __bf16* xrow[MB];
#pragma unroll
  for (int nt = 0; nt < kNT; ++nt) {
    const Segment& t = E == kStore ? sg : grp.seg[nt];
    const int ch = (E == kStore ? ch0 + 16 * nt : ch0) + n, chc = ch < N ? ch : N - 1;
    wrow[nt] = t.codes + (size_t)chc * t.ldw + 16 * g;
    srow[nt] = t.scales + (size_t)chc * t.lds + g;
  }
#pragma unroll
  for (int mb = 0; mb < MB; ++mb) {
    const int m = 16 * mb + n;
    xrow[mb] = x + (size_t)(m < M ? m : M - 1) * ldx + 32 * g;
  }

  int s0, s1;
  even_part(slabs, gridDim.y, blockIdx.y, s0, s1);
  for (int s = s0; s < s1; ++s) {
    int c0, c1;
    even_part(K / kKC, slabs, s, c0, c1);
    f32x4 acc[MB][kNT];
#pragma unroll
    for (int mb = 0; mb < MB; ++mb)
#pragma unroll
      for (int nt = 0; nt < kNT; ++nt) acc[mb][nt] = f32x4{0.f, 0.f, 0.f, 0.f};

    // two chunks per trip: the loads of both (weights, scale bytes, x) are issued before the first MFMA; a last
    // odd chunk is loaded twice (an L1 hit) and multiplied once
    for (int c = c0 + wave; c < c1; c += 2 * kWaves) {
      const bool two = c + kWaves < c1;
      Chunk<MB> a, b;
      a.load(wrow, srow, xrow, (size_t)c);
      b.load(wrow, srow, xrow, (size_t)(two ? c + kWaves : c));
      a.mma(acc);
      if (two) b.mma(acc);
    }

    if (s != s0) __syncthreads();  // the previous slab's sums have been read
#pragma unroll
    for (int mb = 0; mb < MB; ++mb)
#pragma unroll
      for (int nt = 0; nt < kNT; ++nt) sm[wave][mb * kNT + nt][lane] = acc[mb][nt];
    __syncthreads();

    if (E == kStore) {
      // the four waves in wave order; one thread per accumulator quad: four channels of one row
      for (int q = tid; q < MB * kNT * 64; q += 64 * kWaves) {
        const int f = q >> 6, l = q & 63;
        const int m = 16 * (f / kNT) + (l & 15), ch = ch0 + 16 * (f % kNT) + 4 * (l >> 4);
        if (m >= M || ch >= N) continue;  // N % 8 == 0 and ch % 4 == 0: ch < N means ch + 3 < N
        const f32x4 v = wave_sum<MB>(sm, f, l);
        if (slabs == 1)
          *reinterpret_cast<bf16x4*>(sg.y + (size_t)m * N + ch) = to_bf16(v);
        else
          *reinterpret_cast<f32x4*>(ws + ((size_t)s * M + m) * grp.Ntot + sg.col0 + ch) = v;
      }
    } else {
      // one thread per pair of quads: four gate channels of one row and the same four up channels
      for (int q = tid; q < MB * 64; q += 64 * kWaves) {
        const int mb = q >> 6, l = q & 63;
        const int m = 16 * mb + (l & 15), ch = ch0 + 4 * (l >> 4);
        if (m >= M || ch >= N) continue;
        const f32x4 gv = wave_sum<MB>(sm, mb * kNT, l), uv = wave_sum<MB>(sm, mb * kNT + 1, l);
        if (slabs == 1) {
          *reinterpret_cast<bf16x4*>(sg.y + (size_t)m * N + ch) = swiglu4(gv, uv);
        } else {
          float* row = ws + ((size_t)s * M + m) * grp.Ntot + ch;
          *reinterpret_cast<f32x4*>(row + grp.seg[0].col0) = gv;
          *reinterpret_cast<f32x4*>(row + grp.seg[1].col0) = uv;
        }
      }
    }
  }
}

// the slabs of ws[slab][M][Ntot] in slab order, then the store of the epilogue above. kStore: one thread per four
// columns of a row (col0_i % 8 == 0: a quad lies in one segment); kSwiglu: one thread per four channels
template <int E>
__global__ __launch_bounds__(256) void linear_mxfp4_combine_kernel(const float* __restrict__ ws, const Group grp, int M,
                                                                   int slabs) {
  const size_t cols = E == kStore ? (size_t)grp.Ntot : (size_t)grp.seg[0].N;
  const size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i >= (size_t)M * cols) return;
  const size_t m = i / cols, slab = (size_t)M * grp.Ntot;
  const int c = (int)(i % cols);
  const float* row = ws + m * grp.Ntot;
  if (E == kStore) {
    Segment sg = grp.seg[0];
#pragma unroll
    for (int j = 1; j < kMaxGroup; ++j)
      if (j < grp.G && c >= grp.seg[j].col0) sg = grp.seg[j];
    f32x4 v = *reinterpret_cast<const f32x4*>(row + c);
    for (int s = 1; s < slabs; ++s) v += *reinterpret_cast<const f32x4*>(row + s * slab + c);
    *reinterpret_cast<bf16x4*>(sg.y + m * sg.N + (c - sg.col0)) = to_bf16(v);
  } else {
    const float* gp = row + grp.seg[0].col0 + c;
    const float* up = row + grp.seg[1].col0 + c;
    f32x4 gv = *reinterpret_cast<const f32x4*>(gp), uv = *reinterpret_cast<const f32x4*>(up);
    for (int s = 1; s < slabs; ++s) {
      gv += *reinterpret_cast<const f32x4*>(gp + s * slab);
      uv += *reinterpret_cast<const f32x4*>(up + s * slab);
    }
    *reinterpret_cast<bf16x4*>(grp.seg[0].y + i) = swiglu4(gv, uv);
  }
}

template <int MB, int E>
hipError_t launch_main(const void* x, const Group& grp, float* ws, int M, int K, size_t ldx, int tiles, int slabs,
                       int wgs, hipStream_t st) {
  hipLaunchKernelGGL((linear_mxfp4_kernel<MB, E>), dim3((unsigned)tiles, (unsigned)wgs), dim3(64 * kWaves), 0, st,
                     (const __bf16*)x, grp, ws, M, K, ldx, slabs);
  return hipGetLastError();
}

// the main kernel on `tiles` workgroups per slab share and, when K is split, the combine over `quads` float4s
template <int E>
hipError_t launch(const void* x, const Group& grp, float* ws, int M, int K, size_t ldx, int tiles, size_t quads,
                  int slabs, int wgs, hipStream_t st) {
  hipError_t e = hipErrorInvalidValue;
  switch ((M + 15) / 16) {
    case 1: e = launch_main<1, E>(x, grp, ws, M, K, ldx, tiles, slabs, wgs, st); break;
    case 2: e = launch_main<2, E>(x, grp, ws, M, K, ldx, tiles, slabs, wgs, st); break;
    case 3: e = launch_main<3, E>(x, grp, ws, M, K, ldx, tiles, slabs, wgs, st); break;
    case 4: e = launch_main<4, E>(x, grp, ws, M, K, ldx, tiles, slabs, wgs, st); break;
  }
  if (e != hipSuccess || slabs == 1) return e;
  hipLaunchKernelGGL((linear_mxfp4_combine_kernel<E>), dim3((unsigned)((quads + 255) / 256)), dim3(256), 0, st, ws, grp,
                     M, slabs);
  return hipGetLastError();
}

bool aligned16(const void* p) { return p != nullptr && reinterpret_cast<uintptr_t>(p) % 16 == 0; }

// the CUs of the current device; 256 (an MI355X) where there is none to ask
int cu_count() {
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1) {
    (void)hipGetLastError();
    return 256;
  }
  return cus;
}

// the slab count for `tiles` workgroups per slab: from M, the tiles, K and the CU count only
int slabs_for_tiles(int M, int64_t tiles, int K) {
  if (M < 1 || tiles < 1 || K < kKC) return 1;
  // workgroups aimed at: 4 per CU while one block of x rows keeps a workgroup light, 2 per CU above (the fp32
  // partials cost M * N * 4 bytes per slab to write and to read back)
  const int64_t target = (int64_t)cu_count() * (M <= 16 ? 4 : 2);
  int64_t n = (target + tiles - 1) / tiles;
  const int cap = cs_linear_mxfp4_max_splits(K);
  if (n > cap) n = cap;
  return n < 1 ? 1 : (int)n;
}

// what every entry asks of x, K and the split
bool common_ok(const void* x, int M, int K, size_t ldx, const float* ws, int slabs, int wgs) {
  if (M < 1 || M > kMaxM || K < kKC || K % kKC != 0) return false;
  if (ldx < (size_t)K || ldx % 8 != 0 || !aligned16(x)) return false;
  if (slabs < 1 || slabs > cs_linear_mxfp4_max_splits(K) || wgs < 1 || wgs > slabs) return false;
  return slabs == 1 || aligned16(ws);
}

// one weight of N > 0 channels: the strides hold a row and keep the code rows 16-byte aligned
bool weight_ok(const void* codes, const void* scales, const void* y, int N, int K, size_t ldw, size_t lds) {
  if (N < 8 || N % 8 != 0 || ldw < (size_t)K / 2 || ldw % 16 != 0 || lds < (size_t)K / 32) return false;
  return aligned16(codes) && aligned16(scales) && aligned16(y);
}

}  // namespace

int cs_linear_mxfp4_max_m() { return kMaxM; }
int cs_linear_mxfp4_max_group() { return kMaxGroup; }

int cs_linear_mxfp4_max_splits(int K) {
  const int n = K / kKC / kMinChunks;
  return n < 1 ? 1 : (n > kMaxSlabs ? kMaxSlabs : n);
}

int cs_linear_mxfp4_splits(int M, int N, int K) { return slabs_for_tiles(M, ((int64_t)N + kCT - 1) / kCT, K); }

int cs_linear_mxfp4_grouped_splits(int M, const int* N, int G, int K) {
  int64_t tiles = 0;
  for (int i = 0; i < G; ++i) tiles += N[i] > 0 ? ((int64_t)N[i] + kCT - 1) / kCT : 0;
  return slabs_for_tiles(M, tiles, K);
}

int cs_swiglu_linear_mxfp4_splits(int M, int N, int K) { return slabs_for_tiles(M, ((int64_t)N + 15) / 16, K); }

size_t cs_linear_mxfp4_ws_floats(int M, int N, int slabs) { return slabs <= 1 ? 0 : (size_t)slabs * M * N; }
size_t cs_swiglu_linear_mxfp4_ws_floats(int M, int N, int slabs) { return cs_linear_mxfp4_ws_floats(M, N, slabs) * 2; }

hipError_t cs_linear_mxfp4_grouped(const void* x, const void* const* codes, const void* const* scales, void* const* y,
                                   const int* N, const size_t* ldw, const size_t* lds, int G, float* ws, int M, int K,
                                   size_t ldx, int slabs, int wgs, hipStream_t stream) {
  if (G < 1 || G > kMaxGroup || M < 0) return hipErrorInvalidValue;
  if (M == 0) return hipSuccess;
  if (!common_ok(x, M, K, ldx, ws, slabs, wgs)) return hipErrorInvalidValue;
  Group grp = {};
  int64_t tiles = 0, cols = 0;
  for (int i = 0; i < G; ++i) {
    if (!weight_ok(codes[i], scales[i], y[i], N[i], K, ldw[i], lds[i])) return hipErrorInvalidValue;
    grp.seg[i] = Segment{(const unsigned char*)codes[i], (const unsigned char*)scales[i], (__bf16*)y[i], ldw[i], lds[i],
                         N[i], (int)tiles, (int)cols};
    tiles += (N[i] + kCT - 1) / kCT;
    cols += N[i];
    if (cols > INT_MAX) return hipErrorInvalidValue;
  }
  grp.G = G;
  grp.Ntot = (int)cols;
  return launch<kStore>(x, grp, ws, M, K, ldx, (int)tiles, (size_t)M * cols / 4, slabs, wgs, stream);
}

hipError_t cs_linear_mxfp4(const void* x, const void* codes, const void* scales, void* y, float* ws, int M, int N, int K,
                           size_t ldx, size_t ldw, size_t lds, int slabs, int wgs, hipStream_t stream) {
  if (N == 0 && M >= 0) return hipSuccess;
  return cs_linear_mxfp4_grouped(x, &codes, &scales, &y, &N, &ldw, &lds, 1, ws, M, K, ldx, slabs, wgs, stream);
}

hipError_t cs_linear_mxfp4_combine(const float* ws, void* y, int M, int N, int slabs, hipStream_t stream) {
  if (M == 0 || N == 0) return hipSuccess;
  if (M < 0 || N < 0 || N % 8 != 0 || slabs < 1 || !aligned16(ws) || !aligned16(y)) return hipErrorInvalidValue;
  const size_t quads = (size_t)M * N / 4;
  if ((quads + 255) / 256 > 0x7fffffffu) return hipErrorInvalidValue;
  Group grp = {};
  grp.seg[0] = Segment{nullptr, nullptr, (__bf16*)y, 0, 0, N, 0, 0};  // a group of one: every column is its own
  grp.G = 1;
  grp.Ntot = N;
  hipLaunchKernelGGL((linear_mxfp4_combine_kernel<kStore>), dim3((unsigned)((quads + 255) / 256)), dim3(256), 0, stream,
                     ws, grp, M, slabs);
  return hipGetLastError();
}

hipError_t cs_swiglu_linear_mxfp4(const void* x, const void* gate, const void* gate_scales, const void* up,
                                  const void* up_scales, void* y, float* ws, int M, int N, int K, size_t ldx, size_t ldg,
                                  size_t ldgs, size_t ldu, size_t ldus, int slabs, int wgs, hipStream_t stream) {
  if (M < 0 || N < 0) return hipErrorInvalidValue;
  if (M == 0 || N == 0) return hipSuccess;
  if (!common_ok(x, M, K, ldx, ws, slabs, wgs) || N > INT_MAX / 2) return hipErrorInvalidValue;
  if (!weight_ok(gate, gate_scales, y, N, K, ldg, ldgs) || !weight_ok(up, up_scales, y, N, K, ldu, ldus))
    return hipErrorInvalidValue;
  Group grp = {};
  grp.seg[0] = Segment{(const unsigned char*)gate, (const unsigned char*)gate_scales, (__bf16*)y, ldg, ldgs, N, 0, 0};
  grp.seg[1] = Segment{(const unsigned char*)up, (const unsigned char*)up_scales, (__bf16*)y, ldu, ldus, N, 0, N};
  grp.G = 2;
  grp.Ntot = 2 * N;
  return launch<kSwiglu>(x, grp, ws, M, K, ldx, (N + 15) / 16, (size_t)M * N / 4, slabs, wgs, stream);
}
