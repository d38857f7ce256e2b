// FP8 weight-only linear for decoding on gfx950 (W8A16, skinny M):
//   y[M, N] = (x[M, K] . codes[N, K]^T) * scale[N]
// x bf16 (rows ldx elements apart, unit inner stride), codes OCP e4m3fn bytes (rows ldw bytes apart, K
// contiguous), scale fp32 [N], one power of two per output channel (the format of kv_quant_device.h applied to
// the rows of a weight), y bf16 [M, N] contiguous. 1 <= M <= 64, K % 64 == 0, N % 8 == 0. Every code is exactly a
// bf16 number and every product x * code is exact in fp32, so the only roundings are the fp32 sums and the
// final bf16 store.
//
// The product is bound by the weight bytes: each is read from HBM once per call, 16 bytes per lane, straight
// into registers (a weight byte is used by one wave only, so LDS would buy nothing), dequantised there to bf16
// and multiplied on v_mfma_f32_16x16x32_bf16.
//
// Work split. A workgroup is 4 waves and owns kNT = 2 tiles of 16 output channels (32 channels) over a run of
// K. K is cut into chunks of 64; the chunks are divided, as evenly as possible, into `slabs` contiguous slabs,
// and the slabs into the gridDim.y workgroups of a channel-tile pair. Inside a slab, wave w takes chunks
// w, w + 4, ... and accumulates them in one MFMA chain; the four waves are then summed through LDS in wave
// order. With slabs == 1 that sum is scaled and stored as y. Otherwise it is the fp32 partial ws[slab][M][N],
// and linear_fp8_combine_kernel sums the slabs of an element in slab order, scales once and stores bf16.
// The slab count comes from M, N, K and the CU count only (cs_linear_fp8_splits), and it alone fixes the
// summation tree: how many workgroups share the slabs (the `wgs` argument, the caller's `splits` override) moves
// work between workgroups and changes no bit. No atomics, no arrival counters.
//
// Lane maps (lane = 16 g + n, g = lane / 16 in 0..3, n = lane % 16), for the chunk at k0 = 64 * chunk:
//   weights  lane (n, g) loads the 16 bytes k0 + 16 g .. k0 + 16 g + 15 of channel c0 + n (one uint4). Bytes
//            0..7 of it feed MFMA K-step s = 0 and bytes 8..15 K-step s = 1: in step s the lane's eight A-operand
//            values are k = k0 + 16 g + 8 s + j, j = 0..7. (The MFMA itself calls them k' = 8 g + j; it only
//            sums over them, so any assignment of real k to (g, j, s) is right as long as both operands use it.)
//   x        lane (n, g) holds row m = 16 mb + n of x for block mb: two uint4 loads of eight bf16,
//            k = k0 + 16 g + 8 s + j for s = 0 and 1: the same (g, s, j) -> k map as the weights.
//   product  acc = mfma(A = weights, B = x): A's rows are channels, B's columns are x rows, so register j of
//            lane (n, g) is y[m = 16 mb + n][channel = c0 + 4 g + j]: four consecutive channels of one row,
//            one 8-byte bf16 store (or one 16-byte fp32 store to the workspace).
// M > 16 runs MB = ceil(M / 16) <= 4 blocks of x over the same dequantised weight registers: MB * kNT
// accumulators of 4 registers. Rows >= M and channels >= N are never stored.
//
// x is read from global memory, not staged in LDS: with K split across the waves of a workgroup no two of its
// waves read the same x bytes, so staging would add a write, a barrier and a read of the same data. x is at
// most 1.8 MB, lives in L2, and the workgroups of a slab that share a CU hit it in L1. The x fragment a wave
// loads is used for both of its channel tiles, which halves the x loads per weight byte. That is not enough at
// M >= 32: there the kernel's time grows with M and it falls behind the bf16 library GEMM on the large shapes
// (docs/linear_fp8.md, "Measurements"): 2 * MB x loads per 2 weight loads at 2 to 4 waves per SIMD.
//
// Dequantisation: v_cvt_pk_f32_fp8 gives two exact fp32 values per call; their upper halves are the bf16 values
// (an e4m3 value has 4 significant bits: truncation is exact, subnormals and +-0 included), packed two per
// register by one v_perm_b32. NaN codes (0x7f, 0xff) are not produced by the quantiser; they give NaN or Inf in
// the channel's outputs and touch no address.
#include "common.h"
#include "fp8_dequant_device.h"
#include "launchers.h"

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kKC = 64;         // K per chunk: 16 bytes of a channel in each of the four lane groups
constexpr int kWaves = 4;       // waves per workgroup, interleaved over the chunks of a slab
constexpr int kNT = 2;          // 16-channel tiles per workgroup
constexpr int kCT = 16 * kNT;   // channels per workgroup
constexpr int kMaxM = 64;
constexpr int kMinChunks = 2;   // chunks per slab the heuristic keeps
constexpr int kMaxSlabs = 64;
constexpr int kMaxGroup = 3;    // weights of one grouped launch (q, k and v)

using cs::dequant8;  // eight e4m3fn codes (two registers) -> eight bf16 values in k order (fp8_dequant_device.h)

// the chunks [c0, c1) of part i when n chunks are divided as evenly as possible into parts
__device__ __forceinline__ void even_part(int n, int parts, int i, int& c0, int& c1) {
  const int base = n / parts, rem = n % parts;
  c0 = i * base + (i < rem ? i : rem);
  c1 = c0 + base + (i < rem ? 1 : 0);
}

// what a lane holds of one chunk: 16 codes of each of its kNT channels, 16 bf16 of each of its MB rows of x
template <int MB>
struct Chunk {
  uint4 wq[kNT], xq[MB][2];
  __device__ __forceinline__ void load(const unsigned char* const (&wrow)[kNT], const __bf16* const (&xrow)[MB],
                                       size_t k0) {
#pragma unroll
    for (int nt = 0; nt < kNT; ++nt) wq[nt] = *reinterpret_cast<const uint4*>(wrow[nt] + k0);
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) {
      xq[mb][0] = *reinterpret_cast<const uint4*>(xrow[mb] + k0);      // K-step 0: k0 + 16 g + 0..7
      xq[mb][1] = *reinterpret_cast<const uint4*>(xrow[mb] + k0 + 8);  // K-step 1: k0 + 16 g + 8..15
    }
  }
  __device__ __forceinline__ void mma(f32x4 (&acc)[MB][kNT]) const {
    bf16x8 wf[kNT][2];
#pragma unroll
    for (int nt = 0; nt < kNT; ++nt) {
      wf[nt][0] = dequant8(wq[nt].x, wq[nt].y);  // K-step 0: bytes 0..7
      wf[nt][1] = dequant8(wq[nt].z, wq[nt].w);  // K-step 1: bytes 8..15
    }
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int mb = 0; mb < MB; ++mb) {
        const bf16x8 xf = __builtin_bit_cast(bf16x8, xq[mb][ks]);
#pragma unroll
        for (int nt = 0; nt < kNT; ++nt)
          acc[mb][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[nt][ks], xf, acc[mb][nt], 0, 0, 0);
      }
  }
};

// one slab of one wave: the chunks c0 + wave, c0 + wave + 4, ... of [c0, c1) in one MFMA chain per accumulator.
// The loop of linear_fp8_kernel, for the grouped and the paired kernel. linear_fp8_kernel keeps its own copy inline:
// called through this function its register allocation changes (60 VGPRs / 8 AGPRs instead of 62 / 12 at MB 1), and
// its measurements in docs/linear_fp8.md stand on the allocation it has.
template <int MB>
__device__ __forceinline__ void slab_mma(const unsigned char* const (&wrow)[kNT], const __bf16* const (&xrow)[MB],
                                         int c0, int c1, int wave, f32x4 (&acc)[MB][kNT]) {
#pragma unroll
  for (int mb = 0; mb < MB; ++mb)
#pragma unroll
    for (int nt = 0; nt < kNT; ++nt) acc[mb][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
  // two chunks per trip: the loads of both are issued before the first MFMA, so a wave keeps 2 * kNT weight
  // loads in flight; a last odd chunk is loaded twice (an L1 hit) and multiplied once
  for (int c = c0 + wave; c < c1; c += 2 * kWaves) {
    const bool two = c + kWaves < c1;
    Chunk<MB> a, b;
    a.load(wrow, xrow, (size_t)c * kKC);  // c < K / 64: bytes k0 + 16 g .. + 15 lie inside the row
    b.load(wrow, xrow, (size_t)(two ? c + kWaves : c) * kKC);
    a.mma(acc);
    if (two) b.mma(acc);
  }
}

// a wave's accumulators into its LDS stage, and the sum of the four stages of one quad in wave order
template <int MB>
__device__ __forceinline__ void stage(f32x4 (&sm)[kWaves][MB * kNT][64], int wave, int lane,
                                      const f32x4 (&acc)[MB][kNT]) {
#pragma unroll
  for (int mb = 0; mb < MB; ++mb)
#pragma unroll
    for (int nt = 0; nt < kNT; ++nt) sm[wave][mb * kNT + nt][lane] = acc[mb][nt];
}
template <int MB>
__device__ __forceinline__ f32x4 wave_sum(const f32x4 (&sm)[kWaves][MB * kNT][64], int f, int l) {
  f32x4 v = sm[0][f][l];
#pragma unroll
  for (int w = 1; w < kWaves; ++w) v += sm[w][f][l];
  return v;
}

template <int MB>
__global__ __launch_bounds__(64 * kWaves) void linear_fp8_kernel(const __bf16* __restrict__ x,
                                                                 const unsigned char* __restrict__ codes,
                                                                 const float* __restrict__ scale,
                                                                 __bf16* __restrict__ y, float* __restrict__ ws, int M,
                                                                 int N, int K, size_t ldx, size_t ldw, int slabs) {
  __shared__ f32x4 sm[kWaves][MB * kNT][64];
  const int tid = threadIdx.x, lane = tid & 63, n = lane & 15, g = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // wave-uniform: the chunk loop is scalar control flow
  const int ch0 = blockIdx.x * kCT;

  // the lane's rows: channel ch0 + 16 nt + n of the weights, row 16 mb + n of x. A row outside the operand is
  // clamped onto its last row: the loads stay in bounds and unconditional, and since an MFMA output depends on
  // one A row and one B column only, what such a lane loads reaches only outputs that are never stored
  const unsigned char* wrow[kNT];
  const __bf16* xrow[MB];
#pragma unroll
  for (int nt = 0; nt < kNT; ++nt) {
    const int ch = ch0 + 16 * nt + n;
    wrow[nt] = codes + (size_t)(ch < N ? ch : N - 1) * ldw + 16 * g;
  }
#pragma unroll
  for (int mb = 0; mb < MB; ++mb) {
    const int m = 16 * mb + n;
    xrow[mb] = x + (size_t)(m < M ? m : M - 1) * ldx + 16 * g;
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

    // two chunks per trip: the loads of both are issued before the first MFMA, so a wave keeps 2 * kNT weight
    // loads in flight; a last odd chunk is loaded twice (an L1 hit) and multiplied once
    for (int c = c0 + wave; c < c1; c += 2 * kWaves) {
      const bool two = c + kWaves < c1;
      Chunk<MB> a, b;
      a.load(wrow, xrow, (size_t)c * kKC);  // c < K / 64: bytes k0 + 16 g .. + 15 lie inside the row
      b.load(wrow, xrow, (size_t)(two ? c + kWaves : c) * kKC);
      a.mma(acc);
      if (two) b.mma(acc);
    }

    if (s != s0) __syncthreads();  // the previous slab's sums have been read
    stage<MB>(sm, wave, lane, acc);
    __syncthreads();
    // the four waves in wave order; one thread per accumulator quad: four channels of one row
    for (int q = tid; q < MB * kNT * 64; q += 64 * kWaves) {
      const int f = q >> 6, l = q & 63;
      f32x4 v = wave_sum<MB>(sm, f, l);
      const int m = 16 * (f / kNT) + (l & 15), ch = ch0 + 16 * (f % kNT) + 4 * (l >> 4);
      if (m >= M || ch >= N) continue;  // N % 8 == 0 and ch % 4 == 0: ch < N means ch + 3 < N
      if (slabs == 1) {
        v *= *reinterpret_cast<const f32x4*>(scale + ch);
        const bf16x4 o = {(__bf16)v[0], (__bf16)v[1], (__bf16)v[2], (__bf16)v[3]};
        *reinterpret_cast<bf16x4*>(y + (size_t)m * N + ch) = o;
      } else {
        *reinterpret_cast<f32x4*>(ws + ((size_t)s * M + m) * N + ch) = v;
      }
    }
  }
}

// y = (sum of the slabs in slab order) * scale; one thread per four channels of a row
__global__ __launch_bounds__(256) void linear_fp8_combine_kernel(const float* __restrict__ ws,
                                                                 const float* __restrict__ scale,
                                                                 __bf16* __restrict__ y, size_t MN, int N, int slabs) {
  const size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i >= MN) return;
  f32x4 v = *reinterpret_cast<const f32x4*>(ws + i);
  for (int s = 1; s < slabs; ++s) v += *reinterpret_cast<const f32x4*>(ws + (size_t)s * MN + i);
  v *= *reinterpret_cast<const f32x4*>(scale + i % (size_t)N);
  const bf16x4 o = {(__bf16)v[0], (__bf16)v[1], (__bf16)v[2], (__bf16)v[3]};
  *reinterpret_cast<bf16x4*>(y + i) = o;
}

// ---- grouped mode: up to kMaxGroup weights [N_i, K] that share x, one launch. Each weight stays its own tensor:
// the kernel gets a table of segments by value. blockIdx.x runs over the 32-channel tile pairs of all segments
// (segment i owns tiles [tile0_i, tile0_{i+1})), so a workgroup never straddles two segments, and it finds its
// segment from blockIdx.x alone: scalar compares and selects. From there on it is linear_fp8_kernel on that
// segment: the same lane maps, chunk loop and fixed-order sums, so for equal `slabs` the bits are linear_fp8's. The
// slab count is picked from the summed tiles, which is the point: the narrow segments (k and v: 32 tile pairs
// each) ride in a grid the wide one already fills. Workspace: ws[slab][M][Ntot], segment i at columns col0_i.
struct Segment {
  const unsigned char* codes;  // [N, K] e4m3fn, rows ldw bytes apart
  const float* scale;          // [N]
  __bf16* y;                   // [M, N] contiguous
  size_t ldw;
  int N, tile0, col0;
};
struct Group {
  Segment seg[kMaxGroup];
  int G, Ntot;
};

template <int MB>
__global__ __launch_bounds__(64 * kWaves) void linear_fp8_grouped_kernel(const __bf16* __restrict__ x, const Group grp,
                                                                         float* __restrict__ ws, int M, int K,
                                                                         size_t ldx, int slabs) {
  __shared__ f32x4 sm[kWaves][MB * kNT][64];
  const int tid = threadIdx.x, lane = tid & 63, n = lane & 15, g = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  // the last segment that starts at or before this tile pair; an unused table entry is never looked at
  Segment sg = grp.seg[0];
#pragma unroll
  for (int i = 1; i < kMaxGroup; ++i)
    if (i < grp.G && (int)blockIdx.x >= grp.seg[i].tile0) sg = grp.seg[i];
  const int N = sg.N, ch0 = ((int)blockIdx.x - sg.tile0) * kCT;

  // rows outside the segment or x are clamped onto its last row, as in linear_fp8_kernel: in bounds, never stored
  const unsigned char* wrow[kNT];
  const __bf16* xrow[MB];
#pragma unroll
  for (int nt = 0; nt < kNT; ++nt) {
    const int ch = ch0 + 16 * nt + n;
    wrow[nt] = sg.codes + (size_t)(ch < N ? ch : N - 1) * sg.ldw + 16 * g;
  }
#pragma unroll
  for (int mb = 0; mb < MB; ++mb) {
    const int m = 16 * mb + n;
    xrow[mb] = x + (size_t)(m < M ? m : M - 1) * ldx + 16 * g;
  }

  int s0, s1;
  even_part(slabs, gridDim.y, blockIdx.y, s0, s1);
  for (int s = s0; s < s1; ++s) {
    int c0, c1;
    even_part(K / kKC, slabs, s, c0, c1);
    f32x4 acc[MB][kNT];
    slab_mma<MB>(wrow, xrow, c0, c1, wave, acc);
    if (s != s0) __syncthreads();
    stage<MB>(sm, wave, lane, acc);
    __syncthreads();
    for (int q = tid; q < MB * kNT * 64; q += 64 * kWaves) {
      const int f = q >> 6, l = q & 63;
      f32x4 v = wave_sum<MB>(sm, f, l);
      const int m = 16 * (f / kNT) + (l & 15), ch = ch0 + 16 * (f % kNT) + 4 * (l >> 4);
      if (m >= M || ch >= N) continue;
      if (slabs == 1) {
        v *= *reinterpret_cast<const f32x4*>(sg.scale + ch);
        const bf16x4 o = {(__bf16)v[0], (__bf16)v[1], (__bf16)v[2], (__bf16)v[3]};
        *reinterpret_cast<bf16x4*>(sg.y + (size_t)m * N + ch) = o;
      } else {
        *reinterpret_cast<f32x4*>(ws + ((size_t)s * M + m) * grp.Ntot + sg.col0 + ch) = v;
      }
    }
  }
}

// the slabs of ws[slab][M][Ntot] in slab order, scaled, into the G outputs; one thread per four columns of a row
// (col0_i % 8 == 0: a quad lies in one segment)
__global__ __launch_bounds__(256) void linear_fp8_grouped_combine_kernel(const float* __restrict__ ws, const Group grp,
                                                                         int M, int slabs) {
  const size_t MN = (size_t)M * grp.Ntot, i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i >= MN) return;
  const int m = (int)(i / (size_t)grp.Ntot), c = (int)(i % (size_t)grp.Ntot);
  Segment sg = grp.seg[0];
#pragma unroll
  for (int j = 1; j < kMaxGroup; ++j)
    if (j < grp.G && c >= grp.seg[j].col0) sg = grp.seg[j];
  f32x4 v = *reinterpret_cast<const f32x4*>(ws + i);
  for (int s = 1; s < slabs; ++s) v += *reinterpret_cast<const f32x4*>(ws + (size_t)s * MN + i);
  v *= *reinterpret_cast<const f32x4*>(sg.scale + (c - sg.col0));
  const bf16x4 o = {(__bf16)v[0], (__bf16)v[1], (__bf16)v[2], (__bf16)v[3]};
  *reinterpret_cast<bf16x4*>(sg.y + (size_t)m * sg.N + (c - sg.col0)) = o;
}

// ---- paired SwiGLU mode: y[M, N] = swiglu(g, u), g = bf16((x . gate^T) * sg), u = bf16((x . up^T) * su), both
// weights [N, K]. The two tiles of a workgroup are not 32 neighbouring channels: tile 0 is gate channels
// [c, c + 16) and tile 1 is up channels [c, c + 16), so the x fragment a wave loads still serves two weight tiles,
// and after the wave-order sum the thread that holds a gate quad reads the matching up quad from the same LDS
// stage. The roundings of g and u to bf16 are deliberate: the result is, bit for bit,
// swiglu_fwd_kernel(linear_fp8(x, gate), linear_fp8(x, up)) at the same `slabs`, and neither intermediate reaches
// memory. Workspace (slabs > 1): ws[slab][M][2 N], gate at column ch and up at column N + ch.

// four outputs from the fp32 sums of four gate and four up channels: swiglu_fwd_kernel's expression (lm.hip)
__device__ __forceinline__ bf16x4 swiglu4(f32x4 gv, f32x4 uv, const float* __restrict__ sg,
                                          const float* __restrict__ su) {
  gv *= *reinterpret_cast<const f32x4*>(sg);
  uv *= *reinterpret_cast<const f32x4*>(su);
  bf16x4 o;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float a = (float)(__bf16)gv[j], b = (float)(__bf16)uv[j];
    o[j] = (__bf16)(a * (1.f / (1.f + __expf(-a))) * b);
  }
  return o;
}

template <int MB>
__global__ __launch_bounds__(64 * kWaves) void swiglu_linear_fp8_kernel(
    const __bf16* __restrict__ x, const unsigned char* __restrict__ gate, const float* __restrict__ sg,
    const unsigned char* __restrict__ up, const float* __restrict__ su, __bf16* __restrict__ y, float* __restrict__ ws,
    int M, int N, int K, size_t ldx, size_t ldg, size_t ldu, int slabs) {
  __shared__ f32x4 sm[kWaves][MB * kNT][64];
  const int tid = threadIdx.x, lane = tid & 63, n = lane & 15, g = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ch0 = blockIdx.x * 16;

  const int chn = ch0 + n < N ? ch0 + n : N - 1;  // clamped as in linear_fp8_kernel
  const unsigned char* const wrow[kNT] = {gate + (size_t)chn * ldg + 16 * g, up + (size_t)chn * ldu + 16 * g};
  const __bf16* xrow[MB];
#pragma unroll
  for (int mb = 0; mb < MB; ++mb) {
    const int m = 16 * mb + n;
    xrow[mb] = x + (size_t)(m < M ? m : M - 1) * ldx + 16 * g;
  }

  int s0, s1;
  even_part(slabs, gridDim.y, blockIdx.y, s0, s1);
  for (int s = s0; s < s1; ++s) {
    int c0, c1;
    even_part(K / kKC, slabs, s, c0, c1);
    f32x4 acc[MB][kNT];
    slab_mma<MB>(wrow, xrow, c0, c1, wave, acc);
    if (s != s0) __syncthreads();
    stage<MB>(sm, wave, lane, acc);
    __syncthreads();
    // one thread per pair of quads: four gate channels of one row and the same four up channels
    for (int q = tid; q < MB * 64; q += 64 * kWaves) {
      const int mb = q >> 6, l = q & 63;
      const int m = 16 * mb + (l & 15), ch = ch0 + 4 * (l >> 4);
      if (m >= M || ch >= N) continue;
      const f32x4 gv = wave_sum<MB>(sm, mb * kNT, l), uv = wave_sum<MB>(sm, mb * kNT + 1, l);
      if (slabs == 1) {
        *reinterpret_cast<bf16x4*>(y + (size_t)m * N + ch) = swiglu4(gv, uv, sg + ch, su + ch);
      } else {
        float* row = ws + ((size_t)s * M + m) * 2 * N + ch;
        *reinterpret_cast<f32x4*>(row) = gv;
        *reinterpret_cast<f32x4*>(row + N) = uv;
      }
    }
  }
}

// both halves of ws[slab][M][2 N] in slab order, then the epilogue above; one thread per four channels of a row
__global__ __launch_bounds__(256) void swiglu_linear_fp8_combine_kernel(const float* __restrict__ ws,
                                                                        const float* __restrict__ sg,
                                                                        const float* __restrict__ su,
                                                                        __bf16* __restrict__ y, int M, int N, int slabs) {
  const size_t MN = (size_t)M * N, i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i >= MN) return;
  const size_t m = i / (size_t)N, ch = i % (size_t)N;
  const float* row = ws + m * 2 * N + ch;
  f32x4 gv = *reinterpret_cast<const f32x4*>(row), uv = *reinterpret_cast<const f32x4*>(row + N);
  for (int s = 1; s < slabs; ++s) {
    gv += *reinterpret_cast<const f32x4*>(row + (size_t)s * 2 * MN);
    uv += *reinterpret_cast<const f32x4*>(row + (size_t)s * 2 * MN + N);
  }
  *reinterpret_cast<bf16x4*>(y + i) = swiglu4(gv, uv, sg + ch, su + ch);
}

template <int MB>
hipError_t launch_grouped(const void* x, const Group& grp, float* ws, int M, int K, size_t ldx, int tiles, int slabs,
                          int wgs, hipStream_t st) {
  hipLaunchKernelGGL(linear_fp8_grouped_kernel<MB>, dim3((unsigned)tiles, (unsigned)wgs), dim3(64 * kWaves), 0, st,
                     (const __bf16*)x, grp, ws, M, K, ldx, slabs);
  return hipGetLastError();
}

template <int MB>
hipError_t launch_swiglu(const void* x, const void* gate, const float* sg, const void* up, const float* su, void* y,
                         float* ws, int M, int N, int K, size_t ldx, size_t ldg, size_t ldu, int slabs, int wgs,
                         hipStream_t st) {
  hipLaunchKernelGGL(swiglu_linear_fp8_kernel<MB>, dim3((unsigned)((N + 15) / 16), (unsigned)wgs), dim3(64 * kWaves), 0,
                     st, (const __bf16*)x, (const unsigned char*)gate, sg, (const unsigned char*)up, su, (__bf16*)y, ws,
                     M, N, K, ldx, ldg, ldu, slabs);
  return hipGetLastError();
}

template <int MB>
hipError_t launch_linear(const void* x, const void* codes, const float* scale, void* y, float* ws, int M, int N, int K,
                         size_t ldx, size_t ldw, int slabs, int wgs, hipStream_t st) {
  hipLaunchKernelGGL(linear_fp8_kernel<MB>, dim3((unsigned)((N + kCT - 1) / kCT), (unsigned)wgs), dim3(64 * kWaves), 0,
                     st, (const __bf16*)x, (const unsigned char*)codes, scale, (__bf16*)y, ws, M, N, K, ldx, ldw, slabs);
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

}  // namespace

int cs_linear_fp8_max_m() { return kMaxM; }

int cs_linear_fp8_max_splits(int K) {
  const int n = K / kKC / kMinChunks;
  return n < 1 ? 1 : (n > kMaxSlabs ? kMaxSlabs : n);
}

// the slab count for `tiles` workgroups per slab: from M, the tiles, K and the CU count only
static int slabs_for_tiles(int M, int64_t tiles, int K) {
  if (M < 1 || tiles < 1 || K < kKC) return 1;
  // workgroups aimed at: 4 per CU while one block of x rows keeps a workgroup light, 2 per CU above (the fp32
  // partials cost M * N * 4 bytes per slab to write and to read back)
  const int64_t target = (int64_t)cu_count() * (M <= 16 ? 4 : 2);
  int64_t n = (target + tiles - 1) / tiles;
  const int cap = cs_linear_fp8_max_splits(K);
  if (n > cap) n = cap;
  return n < 1 ? 1 : (int)n;
}

int cs_linear_fp8_splits(int M, int N, int K) { return slabs_for_tiles(M, ((int64_t)N + kCT - 1) / kCT, K); }

int cs_linear_fp8_grouped_splits(int M, const int* N, int G, int K) {
  int64_t tiles = 0;
  for (int i = 0; i < G; ++i) tiles += N[i] > 0 ? ((int64_t)N[i] + kCT - 1) / kCT : 0;
  return slabs_for_tiles(M, tiles, K);
}

int cs_swiglu_linear_fp8_splits(int M, int N, int K) { return slabs_for_tiles(M, ((int64_t)N + 15) / 16, K); }

size_t cs_linear_fp8_ws_floats(int M, int N, int slabs) { return slabs <= 1 ? 0 : (size_t)slabs * M * N; }

hipError_t cs_linear_fp8(const void* x, const void* codes, const float* scale, void* y, float* ws, int M, int N, int K,
                         size_t ldx, size_t ldw, int slabs, int wgs, hipStream_t stream) {
  if (M == 0 || N == 0) return hipSuccess;
  if (M < 0 || M > kMaxM || N < 0 || N % 8 != 0 || K < kKC || K % kKC != 0) return hipErrorInvalidValue;
  if (ldx < (size_t)K || ldx % 8 != 0 || ldw < (size_t)K || ldw % 16 != 0) return hipErrorInvalidValue;
  if (!aligned16(x) || !aligned16(codes) || !aligned16(scale) || !aligned16(y)) return hipErrorInvalidValue;
  if (slabs < 1 || slabs > cs_linear_fp8_max_splits(K) || wgs < 1 || wgs > slabs) return hipErrorInvalidValue;
  if (slabs > 1 && !aligned16(ws)) return hipErrorInvalidValue;
  hipError_t e = hipErrorInvalidValue;
  switch ((M + 15) / 16) {
    case 1: e = launch_linear<1>(x, codes, scale, y, ws, M, N, K, ldx, ldw, slabs, wgs, stream); break;
    case 2: e = launch_linear<2>(x, codes, scale, y, ws, M, N, K, ldx, ldw, slabs, wgs, stream); break;
    case 3: e = launch_linear<3>(x, codes, scale, y, ws, M, N, K, ldx, ldw, slabs, wgs, stream); break;
    case 4: e = launch_linear<4>(x, codes, scale, y, ws, M, N, K, ldx, ldw, slabs, wgs, stream); break;
  }
  if (e != hipSuccess || slabs == 1) return e;
  const size_t MN = (size_t)M * N;
  hipLaunchKernelGGL(linear_fp8_combine_kernel, dim3((unsigned)((MN / 4 + 255) / 256)), dim3(256), 0, stream, ws, scale,
                     (__bf16*)y, MN, N, slabs);
  return hipGetLastError();
}

hipError_t cs_linear_fp8_combine(const float* ws, const float* scale, void* y, int M, int N, int slabs,
                                 hipStream_t stream) {
  if (M == 0 || N == 0) return hipSuccess;
  if (M < 0 || N < 0 || N % 8 != 0 || slabs < 1) return hipErrorInvalidValue;
  if (!aligned16(ws) || !aligned16(scale) || !aligned16(y)) return hipErrorInvalidValue;
  const size_t MN = (size_t)M * N, blocks = (MN / 4 + 255) / 256;
  if (blocks > 0x7fffffffu) return hipErrorInvalidValue;
  hipLaunchKernelGGL(linear_fp8_combine_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, ws, scale, (__bf16*)y, MN,
                     N, slabs);
  return hipGetLastError();
}

int cs_linear_fp8_max_group() { return kMaxGroup; }

hipError_t cs_linear_fp8_grouped(const void* x, const void* const* codes, const float* const* scale, void* const* y,
                                 const int* N, const size_t* ldw, int G, float* ws, int M, int K, size_t ldx, int slabs,
                                 int wgs, hipStream_t stream) {
  if (G < 1 || G > kMaxGroup || M < 0 || M > kMaxM || K < kKC || K % kKC != 0) return hipErrorInvalidValue;
  if (M == 0) return hipSuccess;
  if (ldx < (size_t)K || ldx % 8 != 0 || !aligned16(x)) return hipErrorInvalidValue;
  if (slabs < 1 || slabs > cs_linear_fp8_max_splits(K) || wgs < 1 || wgs > slabs) return hipErrorInvalidValue;
  if (slabs > 1 && !aligned16(ws)) return hipErrorInvalidValue;
  Group grp = {};
  int64_t tiles = 0, cols = 0;
  for (int i = 0; i < G; ++i) {
    if (N[i] < 8 || N[i] % 8 != 0 || ldw[i] < (size_t)K || ldw[i] % 16 != 0) return hipErrorInvalidValue;
    if (!aligned16(codes[i]) || !aligned16(scale[i]) || !aligned16(y[i])) return hipErrorInvalidValue;
    grp.seg[i] = Segment{(const unsigned char*)codes[i], scale[i], (__bf16*)y[i], ldw[i], N[i], (int)tiles, (int)cols};
    tiles += (N[i] + kCT - 1) / kCT;
    cols += N[i];
    if (cols > INT_MAX) return hipErrorInvalidValue;
  }
  grp.G = G;
  grp.Ntot = (int)cols;
  hipError_t e = hipErrorInvalidValue;
  switch ((M + 15) / 16) {
    case 1: e = launch_grouped<1>(x, grp, ws, M, K, ldx, (int)tiles, slabs, wgs, stream); break;
    case 2: e = launch_grouped<2>(x, grp, ws, M, K, ldx, (int)tiles, slabs, wgs, stream); break;
    case 3: e = launch_grouped<3>(x, grp, ws, M, K, ldx, (int)tiles, slabs, wgs, stream); break;
    case 4: e = launch_grouped<4>(x, grp, ws, M, K, ldx, (int)tiles, slabs, wgs, stream); break;
  }
  if (e != hipSuccess || slabs == 1) return e;
  const size_t MN = (size_t)M * grp.Ntot;
  hipLaunchKernelGGL(linear_fp8_grouped_combine_kernel, dim3((unsigned)((MN / 4 + 255) / 256)), dim3(256), 0, stream, ws,
                     grp, M, slabs);
  return hipGetLastError();
}

size_t cs_swiglu_linear_fp8_ws_floats(int M, int N, int slabs) { return slabs <= 1 ? 0 : (size_t)slabs * M * N * 2; }

hipError_t cs_swiglu_linear_fp8(const void* x, const void* gate, const float* gate_scale, const void* up,
                                const float* up_scale, void* y, float* ws, int M, int N, int K, size_t ldx, size_t ldg,
                                size_t ldu, int slabs, int wgs, hipStream_t stream) {
  if (M == 0 || N == 0) return hipSuccess;
  if (M < 0 || M > kMaxM || N < 0 || N % 8 != 0 || K < kKC || K % kKC != 0) return hipErrorInvalidValue;
  if (ldx < (size_t)K || ldx % 8 != 0 || ldg < (size_t)K || ldg % 16 != 0 || ldu < (size_t)K || ldu % 16 != 0)
    return hipErrorInvalidValue;
  if (!aligned16(x) || !aligned16(gate) || !aligned16(gate_scale) || !aligned16(up) || !aligned16(up_scale) ||
      !aligned16(y))
    return hipErrorInvalidValue;
  if (slabs < 1 || slabs > cs_linear_fp8_max_splits(K) || wgs < 1 || wgs > slabs) return hipErrorInvalidValue;
  if (slabs > 1 && !aligned16(ws)) return hipErrorInvalidValue;
  hipError_t e = hipErrorInvalidValue;
  switch ((M + 15) / 16) {
    case 1: e = launch_swiglu<1>(x, gate, gate_scale, up, up_scale, y, ws, M, N, K, ldx, ldg, ldu, slabs, wgs, stream); break;
    case 2: e = launch_swiglu<2>(x, gate, gate_scale, up, up_scale, y, ws, M, N, K, ldx, ldg, ldu, slabs, wgs, stream); break;
    case 3: e = launch_swiglu<3>(x, gate, gate_scale, up, up_scale, y, ws, M, N, K, ldx, ldg, ldu, slabs, wgs, stream); break;
    case 4: e = launch_swiglu<4>(x, gate, gate_scale, up, up_scale, y, ws, M, N, K, ldx, ldg, ldu, slabs, wgs, stream); break;
  }
  if (e != hipSuccess || slabs == 1) return e;
  const size_t MN = (size_t)M * N;
  hipLaunchKernelGGL(swiglu_linear_fp8_combine_kernel, dim3((unsigned)((MN / 4 + 255) / 256)), dim3(256), 0, stream, ws,
                     gate_scale, up_scale, (__bf16*)y, M, N, slabs);
  return hipGetLastError();
}
