// FP8 weight-only GEMM for prefill and batches over 64 rows on gfx950 (W8A16, M > 64):
//   y[M, N] = (x[M, K] . codes[N, K]^T) * scale[N]
// The operand formats are linear_fp8.hip's: x bf16 (rows ldx elements apart, unit inner stride), codes OCP e4m3fn
// bytes (rows ldw bytes apart, K contiguous), scale fp32 [N], one power of two per output channel, y bf16 [M, N]
// contiguous. M >= 1, K % 64 == 0, N % 8 == 0, 16-byte aligned rows and bases. linear_fp8 routes M > 64 here; the
// skinny kernel keeps M <= 64 (its bits are not these bits: it splits K over its waves).
//
// Numerical contract.
//  1. The only roundings are the fp32 sums and the final bf16 store: every code is exactly a bf16 number
//     (fp8_dequant_device.h), every product is exact in fp32 and the scale is a power of two.
//  2. For a fixed `slabs` the summation order of an output element depends on K and `slabs` alone: slab s sums the
//     K-tiles [c0_s, c1_s) of even_part(K / 64, slabs, s) in rising order in one MFMA chain, each K-tile as K-step
//     0 then K-step 1, and the slabs are added in slab order by linear_fp8_combine_kernel. Nothing in it depends on
//     M, on the row's place in its tile, on the other rows or on the tile, so a row has the same bits in a call of
//     65 rows and in one of 300, and from run to run. No atomics, no arrival counters.
//  3. NaN codes (0x7f, 0xff) are not produced by the quantiser; they give NaN or Inf in their channel's outputs and
//     touch no address.
//
// Work split. A workgroup of 4 waves owns 128 rows of x by 128 channels over the K-tiles (64 k each) of one slab;
// grid (ceil(M / 128) * ceil(N / 128), slabs), row tile fastest: the workgroups that run together share a weight
// panel, which is the operand that comes from HBM. The tile order is otherwise plain: no XCD remap has been
// measured to help here. The waves are 2 (rows) x 2 (channels); a wave owns 64 rows x 64 channels as 4 x 4 tiles of
// v_mfma_f32_16x16x32_bf16: 64 accumulator registers. As in linear_fp8.hip and gemm_bf16.hip the weights are the
// MFMA's A operand and x its B operand, so register j of lane (n, g) (lane = 16 g + n) of accumulator (rb, cb) is
//   y[m0 + 64 wr + 16 rb + n][n0 + 64 wc + 16 cb + 4 g + j]:
// four consecutive channels of one row, one 8-byte bf16 store (or one 16-byte fp32 store to the workspace).
//
// K order inside a K-tile at k0: in K-step s a lane's eight operand values are k = k0 + 16 g + 8 s + j, j = 0..7,
// for both operands. It is linear_fp8.hip's map, not the k0 + 32 s + 8 g + j of gemm_bf16.hip, and this departs
// from two 8-byte reads per channel tile: with it the sixteen codes a lane needs for both K-steps of a channel are
// one ds_read_b128 (bytes 0..7 feed step 0, bytes 8..15 step 1), which halves the LDS read instructions of the
// weight side. The MFMA only sums over its k', so any assignment of real k to (g, j, s) is right as long as both
// operands use it.
//
// Staging. Both operands reach LDS by LDS-DMA (buffer_load ... lds, 16 bytes per lane, 1 KiB lane-linear per wave
// instruction) through buffer descriptors based at the tile's first row and the slab's first k (64-bit bases, 32-bit
// offsets inside: see cs_linear_fp8_gemm in launchers.h for the bounds). The swizzles are applied to the per-lane
// SOURCE address. Rows >= M and channels >= N get an out-of-range offset and land as zeros; the descriptor ends on
// the last byte of the last valid row of the slab, so nothing outside the tensors is read and nothing is padded.
//   x image      bf16 [128 rows][64 k] = 16 KiB, 128-byte rows; the 16-byte chunk c (k = 8 c .. 8 c + 7) of row r is
//                at chunk slot c ^ ((r >> 1) & 7). A fragment read (ds_read_b128) takes chunk 2 g + s of rows
//                r0 + n: the 16 lanes of one g are 16 consecutive rows, whose addresses mod 256 are
//                128 (r & 1) + 16 (c ^ ((r >> 1) & 7)): 16 distinct 16-byte bank slots, all 64 banks once.
//   codes image  e4m3 [128 channels][64 bytes] = 8 KiB: the codes stay FP8 in LDS, which halves the weight side's
//                LDS footprint and traffic. Chunk g (bytes 16 g .. 16 g + 15) of channel row r is at slot
//                g ^ ((r >> 2) & 3). The 16 lanes of one g read 16 consecutive rows, whose addresses mod 256 are
//                64 (r & 3) + 16 (g ^ ((r >> 2) & 3)): for each r & 3 the four rows differ in (r >> 2) & 3, so again
//                16 distinct 16-byte bank slots. (Unswizzled, rows 64 bytes apart would put them on 4 slots.)
// Two buffers of both images, 48 KiB, so two workgroups fit a CU's 160 KiB. A K-tile is computed in two phases:
// phase 0 dequantises the wave's four channel fragments (both K-steps: 8 VALU operations per fragment, each used by
// all four row blocks) and multiplies row blocks 0 and 1, phase 1 multiplies row blocks 2 and 3 with the same
// weight registers. Staging pieces: P0 = the codes image and the x rows with (r >> 5) & 1 == 0 (what phase 0
// reads; 4 DMA instructions per wave), P1 = the x rows with (r >> 5) & 1 == 1 (2 instructions). Phase p of tile t
// waits (counted vmcnt) for piece p of tile t, passes a raw s_barrier, stages piece p of tile t + 1 into the other
// buffer and runs its 16 MFMAs: vmcnt(2) before phase 0 leaves P1(t) in flight, vmcnt(4) before phase 1 leaves
// P0(t + 1) in flight, and the queue is never drained inside the K loop.
//   WAR: piece p of the other buffer was last read in phase p of tile t - 1; every wave has passed two barriers
//   since, after consuming those reads.  RAW: a wave's own vmcnt retires its DMAs, the barrier after it orders
//   every other wave's.
//
// Split-K. ceil(M / 128) * ceil(N / 128) tiles can leave most CUs idle (M 128 x N 4096: 32 tiles on 256 CUs), so K
// is cut into `slabs` contiguous runs of K-tiles (cs_linear_fp8_gemm_splits: from M, N, K and the CU count only).
// With slabs > 1 a workgroup writes its fp32 partial to ws[slab][M][N] and linear_fp8_combine_kernel (linear_fp8.hip)
// sums the slabs in slab order, scales once and stores bf16. With slabs == 1 the epilogue scales in fp32 and stores.
//
// Built without the packed fp32 VALU instructions (_build.py, _NO_PK_FP32_FILES), as every new kernel is: the only
// candidates are the four multiplies by the scale per accumulator in the epilogue, and the resource report
// (profiles/linear_fp8_gemm_resources.txt) is the same with and without the flag.
#include <algorithm>

#include "common.h"
#include "fp8_dequant_device.h"
#include "launchers.h"

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int kTM = 128, kTN = 128;  // rows of x and channels per workgroup
constexpr int kBK = 64;              // k per K-tile
constexpr int kThreads = 256;
constexpr int kXImg = kTM * kBK * 2;  // bytes of the bf16 x image
constexpr int kWImg = kTN * kBK;      // bytes of the FP8 codes image
constexpr int kBuf = kXImg + kWImg;
constexpr int kOOB = 0x7ffffff0;  // past the end of every descriptor (the launcher bounds their sizes)
constexpr int kMinTiles = 4;      // K-tiles per slab the heuristic keeps
constexpr int kMaxGrid = 65535;   // slabs ride in gridDim.y
// the heuristic never asks for more fp32 partials than this: slabs * M * N * 4 bytes
constexpr int64_t kMaxWsBytes = (int64_t)256 << 20;

using cs::dequant8;

// the K-tiles [c0, c1) of part i when n are divided as evenly as possible into parts (linear_fp8.hip's rule)
__device__ __forceinline__ void even_part(int n, int parts, int i, int& c0, int& c1) {
  const int base = n / parts, rem = n % parts;
  c0 = i * base + (i < rem ? i : rem);
  c1 = c0 + base + (i < rem ? 1 : 0);
}

template <int N>
__device__ __forceinline__ void wait_vm() {
  if constexpr (N == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  else if constexpr (N == 2) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
  else if constexpr (N == 4) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
}

__device__ __forceinline__ void barrier() {
  __builtin_amdgcn_sched_barrier(0);
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_sched_barrier(0);
}

__device__ __forceinline__ void dma16(__amdgpu_buffer_rsrc_t rs, char* lds, int off) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void*)lds, 16, off, 0, 0, 0);
}

// What a wave stages of every K-tile. x half h = the tile rows r with (r >> 5) & 1 == h, 8 groups of 8 rows; wave w
// issues groups 2 w and 2 w + 1 of each half: lane l fills chunk slot l & 7 of row r0 + (l >> 3). The codes image
// is 8 groups of 16 rows; wave w issues groups 2 w and 2 w + 1: lane l fills slot l & 3 of row r0 + (l >> 2).
// Per-lane byte offsets at the slab's first K-tile are computed once (kOOB for rows past the operand).
struct Stager {
  __amdgpu_buffer_rsrc_t xrs, wrs;
  int xoff[2][2], woff[2];  // per lane
  int xlds[2][2], wlds[2];  // wave-uniform image offsets of the instruction's first row

  // xb / wb: element (first row of the tile, first k of the slab); rows / chans: valid ones from there; kbytes:
  // k of the slab. The descriptors end with the slab's last byte of the last valid row.
  __device__ Stager(const __bf16* xb, const unsigned char* wb, int64_t ldx, int64_t ldw, int rows, int chans,
                    int kslab, int wv, int lane) {
    xrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<__bf16*>(xb), (short)0,
                                            (int)((int64_t)(rows - 1) * ldx * 2 + (int64_t)kslab * 2), 0x00020000);
    wrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char*>(wb), (short)0,
                                            (int)((int64_t)(chans - 1) * ldw + kslab), 0x00020000);
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int pr0 = 8 * (2 * wv + i);  // first row of the group within the half
        const int r0 = (pr0 >> 5) * 64 + h * 32 + (pr0 & 31);
        const int r = r0 + (lane >> 3), c = (lane & 7) ^ ((r >> 1) & 7);
        xoff[h][i] = r < rows ? r * (int)(ldx * 2) + c * 16 : kOOB;
        xlds[h][i] = r0 * 128;
      }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int r0 = 16 * (2 * wv + i);
      const int r = r0 + (lane >> 2), c = (lane & 3) ^ ((r >> 2) & 3);
      woff[i] = r < chans ? r * (int)ldw + c * 16 : kOOB;
      wlds[i] = kXImg + r0 * 64;
    }
  }
  // piece 0 of local K-tile t into buf: the codes image and x half 0; piece 1: x half 1
  __device__ __forceinline__ void piece0(char* buf, int t) const {
#pragma unroll
    for (int i = 0; i < 2; ++i) dma16(wrs, buf + wlds[i], woff[i] == kOOB ? kOOB : woff[i] + t * kBK);
#pragma unroll
    for (int i = 0; i < 2; ++i) dma16(xrs, buf + xlds[0][i], xoff[0][i] == kOOB ? kOOB : xoff[0][i] + t * kBK * 2);
  }
  __device__ __forceinline__ void piece1(char* buf, int t) const {
#pragma unroll
    for (int i = 0; i < 2; ++i) dma16(xrs, buf + xlds[1][i], xoff[1][i] == kOOB ? kOOB : xoff[1][i] + t * kBK * 2);
  }
};

// Fragment reads are inline assembly: hipcc orders its own LDS reads after LDS-DMA by waiting vmcnt(0), which
// would drain the load queue in every K-tile. The phases order them by the counted waits and barriers above
// instead. A read's result is only valid after lds_wait, which takes every fragment as an in-out operand so that no
// use of one can be scheduled before the wait.
template <int OFF>
__device__ __forceinline__ u32x4 lds_read16(unsigned addr) {
  u32x4 v;
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF) : "memory");
  return v;
}
__device__ __forceinline__ void lds_wait(u32x4 (&a)[4]) {
  asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3])::"memory");
}
__device__ __forceinline__ void lds_wait(u32x4 (&a)[4], u32x4 (&b)[4]) {
  asm volatile("s_waitcnt lgkmcnt(0)"
               : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(b[0]), "+v"(b[1]), "+v"(b[2]), "+v"(b[3])::"memory");
}

// x fragments of row blocks RB0 and RB0 + 1 (16 rows = 2 KiB apart), both K-steps: xq[2 i + s]
template <int RB0>
__device__ __forceinline__ void read_x(u32x4 (&xq)[4], unsigned xrd0, unsigned xrd1) {
  xq[0] = lds_read16<RB0 * 2048>(xrd0);
  xq[1] = lds_read16<RB0 * 2048>(xrd1);
  xq[2] = lds_read16<(RB0 + 1) * 2048>(xrd0);
  xq[3] = lds_read16<(RB0 + 1) * 2048>(xrd1);
}

// the 16 MFMAs of one phase: row blocks RB0 and RB0 + 1 of the wave against its four dequantised channel fragments
template <int RB0>
__device__ __forceinline__ void mma_half(f32x4 (&acc)[4][4], const bf16x8 (&wf)[4][2], const u32x4 (&xq)[4]) {
  __builtin_amdgcn_s_setprio(1);
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int cb = 0; cb < 4; ++cb)
        acc[RB0 + i][cb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[cb][s], __builtin_bit_cast(bf16x8, xq[2 * i + s]),
                                                                   acc[RB0 + i][cb], 0, 0, 0);
  __builtin_amdgcn_s_setprio(0);
}

// one K-tile from the buffer at LDS address `cur`; STAGE: local K-tile tn is staged into `nxt` meanwhile.
// xrd0 / xrd1 / wrd: the lane's fragment offsets inside a buffer (see the kernel)
template <bool STAGE>
__device__ __forceinline__ void ktile(f32x4 (&acc)[4][4], unsigned cur, char* nxt, const Stager& st, int tn,
                                      unsigned xrd0, unsigned xrd1, unsigned wrd) {
  bf16x8 wf[4][2];
  u32x4 wq[4], xq[4];
  wait_vm<2>();  // piece 0 of this tile has landed; piece 1 may be in flight
  barrier();
  if constexpr (STAGE) st.piece0(nxt, tn);
  wq[0] = lds_read16<0>(cur + wrd);  // channel block cb is 16 channels = 1 KiB further
  wq[1] = lds_read16<1024>(cur + wrd);
  wq[2] = lds_read16<2048>(cur + wrd);
  wq[3] = lds_read16<3072>(cur + wrd);
  read_x<0>(xq, cur + xrd0, cur + xrd1);
  lds_wait(wq, xq);
#pragma unroll
  for (int cb = 0; cb < 4; ++cb) {
    wf[cb][0] = dequant8(wq[cb][0], wq[cb][1]);  // K-step 0: bytes 0..7,  k = k0 + 16 g + j
    wf[cb][1] = dequant8(wq[cb][2], wq[cb][3]);  // K-step 1: bytes 8..15, k = k0 + 16 g + 8 + j
  }
  mma_half<0>(acc, wf, xq);
  wait_vm<STAGE ? 4 : 0>();  // piece 1 of this tile has landed; piece 0 of the next may be in flight
  barrier();
  if constexpr (STAGE) st.piece1(nxt, tn);
  read_x<2>(xq, cur + xrd0, cur + xrd1);
  lds_wait(xq);
  mma_half<2>(acc, wf, xq);
}

__global__ __launch_bounds__(kThreads, 2) void linear_fp8_gemm_kernel(const __bf16* __restrict__ x,
                                                                    const unsigned char* __restrict__ codes,
                                                                    const float* __restrict__ scale,
                                                                    __bf16* __restrict__ y, float* __restrict__ ws,
                                                                    int M, int N, int K, int64_t ldx, int64_t ldw,
                                                                    int slabs) {
  __shared__ __attribute__((aligned(1024))) char smem[2 * kBuf];
  const int nM = (M + kTM - 1) / kTM;
  const int tm = blockIdx.x % nM, tn = blockIdx.x / nM, slab = blockIdx.y;
  const int m0 = tm * kTM, n0 = tn * kTN;
  const int rows = M - m0 < kTM ? M - m0 : kTM, chans = N - n0 < kTN ? N - n0 : kTN;
  int c0, c1;
  even_part(K / kBK, slabs, slab, c0, c1);  // slabs <= K / 64: never empty
  const int nk = c1 - c0;

  const int lane = threadIdx.x & 63, n = lane & 15, g = lane >> 4;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), wr = wv >> 1, wc = wv & 1;
  const Stager st(x + (int64_t)m0 * ldx + (int64_t)c0 * kBK, codes + (int64_t)n0 * ldw + (int64_t)c0 * kBK, ldx, ldw,
                  rows, chans, nk * kBK, wv, lane);

  // the lane's fragment addresses inside a buffer, for row block 0 / channel block 0 and K-step 0. Row
  // r = 64 wr + 16 rb + n has (r >> 1) & 7 == (n >> 1) & 7 and channel row r = 64 wc + 16 cb + n has
  // (r >> 2) & 3 == (n >> 2) & 3 for every block, so the blocks are constant strides apart; x chunk 2 g + s sits at
  // slot (2 g + s) ^ ((n >> 1) & 7)
  const unsigned xrd0 = (64 * wr + n) * 128 + (((2 * g) ^ ((n >> 1) & 7)) << 4);
  const unsigned xrd1 = (64 * wr + n) * 128 + (((2 * g + 1) ^ ((n >> 1) & 7)) << 4);
  const unsigned wrd = kXImg + (64 * wc + n) * 64 + ((g ^ ((n >> 2) & 3)) << 4);
  const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char*)smem;

  f32x4 acc[4][4];
#pragma unroll
  for (int rb = 0; rb < 4; ++rb)
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) acc[rb][cb] = f32x4{0.f, 0.f, 0.f, 0.f};

  st.piece0(smem, 0);
  st.piece1(smem, 0);
  int t = 0;
  for (; t + 1 < nk; ++t)
    ktile<true>(acc, lds0 + (t & 1) * kBuf, smem + ((t + 1) & 1) * kBuf, st, t + 1, xrd0, xrd1, wrd);
  ktile<false>(acc, lds0 + (t & 1) * kBuf, nullptr, st, 0, xrd0, xrd1, wrd);

  // epilogue: register j of acc[rb][cb] is y[m0 + 64 wr + 16 rb + n][n0 + 64 wc + 16 cb + 4 g + j].
  // N % 8 == 0 and ch % 4 == 0: ch < N means ch + 3 < N
#pragma unroll
  for (int cb = 0; cb < 4; ++cb) {
    const int ch = n0 + 64 * wc + 16 * cb + 4 * g;
    if (ch >= N) continue;
    f32x4 sc = {1.f, 1.f, 1.f, 1.f};
    if (slabs == 1) sc = *reinterpret_cast<const f32x4*>(scale + ch);
#pragma unroll
    for (int rb = 0; rb < 4; ++rb) {
      const int m = m0 + 64 * wr + 16 * rb + n;
      if (m >= M) continue;
      if (slabs == 1) {
        const f32x4 v = acc[rb][cb] * sc;
        const bf16x4 o = {(__bf16)v[0], (__bf16)v[1], (__bf16)v[2], (__bf16)v[3]};
        *reinterpret_cast<bf16x4*>(y + (size_t)m * N + ch) = o;
      } else {
        *reinterpret_cast<f32x4*>(ws + ((size_t)slab * M + m) * N + ch) = acc[rb][cb];
      }
    }
  }
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

int cs_linear_fp8_gemm_max_splits(int K) {
  const int n = K / kBK;
  return n < 1 ? 1 : (n > kMaxGrid ? kMaxGrid : n);
}

int64_t cs_linear_fp8_gemm_max_ldx() { return (kOOB - 1) / (2 * kTM); }
int64_t cs_linear_fp8_gemm_max_ldw() { return (kOOB - 1) / kTN; }

int cs_linear_fp8_gemm_splits(int M, int N, int K) {
  if (M < 1 || N < 1 || K < kBK) return 1;
  const int64_t tiles = (int64_t)((M + kTM - 1) / kTM) * ((N + kTN - 1) / kTN);
  const int cus = cu_count();
  if (tiles >= cus) return 1;  // every CU has a tile already
  // aimed at: two workgroups per CU (what fits one). Kept: kMinTiles K-tiles per slab, and partials that cost no
  // more than twice the weight bytes: a slab writes and the combine reads M * N * 4 bytes, the codes are N * K
  int64_t n = 2 * (int64_t)cus / tiles;
  n = std::min<int64_t>(n, K / kBK / kMinTiles);
  n = std::min<int64_t>(n, (int64_t)K / (4 * (int64_t)M));
  if (n < 2 || n * M * N * 4 > kMaxWsBytes) return 1;
  return (int)n;
}

hipError_t cs_linear_fp8_gemm(const void* x, const void* codes, const float* scale, void* y, float* ws, int M, int N,
                              int K, size_t ldx, size_t ldw, int slabs, hipStream_t stream) {
  if (M == 0 || N == 0) return hipSuccess;
  if (M < 0 || N < 0 || N % 8 != 0 || K < kBK || K % kBK != 0) return hipErrorInvalidValue;
  if (ldx < (size_t)K || ldx % 8 != 0 || ldw < (size_t)K || ldw % 16 != 0) return hipErrorInvalidValue;
  // 32-bit offsets inside a descriptor: a tile addresses 128 rows of its operand, so the last byte it can name is
  // below 128 * ldx * 2 (x) or 128 * ldw (codes), which must stay below kOOB
  if (ldx > (size_t)cs_linear_fp8_gemm_max_ldx() || ldw > (size_t)cs_linear_fp8_gemm_max_ldw()) return hipErrorInvalidValue;
  if (!aligned16(x) || !aligned16(codes) || !aligned16(scale) || !aligned16(y)) return hipErrorInvalidValue;
  if (slabs < 1 || slabs > cs_linear_fp8_gemm_max_splits(K)) return hipErrorInvalidValue;
  if (slabs > 1 && !aligned16(ws)) return hipErrorInvalidValue;
  const int64_t tiles = (int64_t)((M + kTM - 1) / kTM) * ((N + kTN - 1) / kTN);
  if (tiles > 0x7fffffff) return hipErrorInvalidValue;
  hipLaunchKernelGGL(linear_fp8_gemm_kernel, dim3((unsigned)tiles, (unsigned)slabs), dim3(kThreads), 0, stream,
                     (const __bf16*)x, (const unsigned char*)codes, scale, (__bf16*)y, ws, M, N, K, (int64_t)ldx,
                     (int64_t)ldw, slabs);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess || slabs == 1) return e;
  return cs_linear_fp8_combine(ws, scale, y, M, N, slabs, stream);
}
