// MXFP4 weight-only GEMM for prefill and batches over 64 rows on gfx950 (W4A16, M > 64):
//   y[M, N] = x[M, K] . W^T,  W[c][k] = e2m1(codes[c][k]) * 2^(scales[c][k / 32] - 127)
// The operand formats are linear_mxfp4.hip's: x bf16 (rows ldx elements apart, unit inner stride), codes uint8
// [N, K / 2] (rows ldw bytes apart, element 2 i in the low nibble of byte i), scales uint8 [N, K / 32] (rows lds bytes
// apart, one e8m0 exponent per 32 k), y bf16 [M, N] contiguous. M >= 1, K % 128 == 0, N % 8 == 0, 16-byte aligned
// rows and bases of x and codes, lds % 4 == 0 and a 4-byte aligned scale base. linear_mxfp4 routes M > 64 here; the
// skinny kernel keeps M <= 64 (its bits are not these bits: it splits K over its waves).
//
// Numerical contract.
//  1. The only roundings are the fp32 sums and the final bf16 store: a code has 2 significant bits and a block scale
//     is a power of two (the quantiser keeps its exponent in [-125, 125]), so every dequantised weight is exactly a
//     bf16 number (mxfp4_dequant_device.h) and every product is exact in fp32. The scale varies along K, so it is
//     folded into the MFMA operand and nothing is scaled after the sum.
//  2. For a fixed `slabs` the summation order of an output element depends on K and `slabs` alone: slab s sums the
//     128-k chunks [c0_s, c1_s) of even_part(K / 128, slabs, s) in rising order in one MFMA chain, each chunk as its
//     two K-tiles and each K-tile as K-step 0 then K-step 1, and the slabs are added in slab order by
//     linear_mxfp4_combine_kernel. Nothing in it depends on M, on the row's place in its tile, on the other rows or on
//     the tile, so a row has the same bits in a call of 65 rows and in one of 300, and from run to run. No atomics,
//     no arrival counters.
//  3. The bits differ from the skinny kernel's (other chains); M <= 64 stays there, so no earlier result changes.
//
// Work split. A workgroup of 4 waves owns 128 rows of x by 128 channels over the chunks of one slab; grid
// (ceil(M / 128) * ceil(N / 128), slabs), row tile fastest: the workgroups that run together share a weight panel.
// The waves are 2 (rows) x 2 (channels); a wave owns 64 rows x 64 channels as 4 x 4 tiles of
// v_mfma_f32_16x16x32_bf16: 64 accumulator registers. The weights are the MFMA's A operand and x its B operand, so
// register j of lane (n, g) (lane = 16 g + n) of accumulator (rb, cb) is
//   y[m0 + 64 wr + 16 rb + n][n0 + 64 wc + 16 cb + 4 g + j]:
// four consecutive channels of one row, one 8-byte bf16 store (or one 16-byte fp32 store to the workspace).
//
// K map. A K-tile is 64 k, a chunk two K-tiles. In K-step s of the K-tile at k0 a lane's eight operand values are
// k = k0 + 16 g + 8 s + j, j = 0..7, for both operands (linear_fp8_gemm.hip's map). On the weight side these are
// nibble j of dword s of the 8 bytes 8 g .. 8 g + 7 of the channel's 32 code bytes of the tile: one ds_read_b64 per
// channel block holds both K-steps. All sixteen codes lie in scale block k0 / 32 + (g >> 1), so a lane needs one
// scale per channel block and K-tile: byte 2 (t & 1) + (g >> 1) of the chunk's four, t the K-tile's index in the slab.
//
// Staging. Everything reaches LDS by LDS-DMA (buffer_load ... lds) through buffer descriptors based at the tile's
// first row and the slab's first k (64-bit bases, 32-bit offsets inside: see cs_linear_mxfp4_gemm in launchers.h).
// The swizzles are applied to the per-lane SOURCE address. Rows >= M and channels >= N get an out-of-range offset
// and land as zeros (zero codes are +0, a zero scale byte gives the scale +0); every descriptor ends on the last
// valid byte of the slab's last valid row, so nothing outside the tensors is read and nothing is padded.
//   x image      bf16 [128 rows][64 k] = 16 KiB, linear_fp8_gemm.hip's as it is: the 16-byte chunk c of row r is at
//                chunk slot c ^ ((r >> 1) & 7); a ds_read_b128 of the 16 lanes of one g takes 16 consecutive rows
//                at addresses mod 256 of 128 (r & 1) + 16 (c ^ ((r >> 1) & 7)): 16 distinct 16-byte bank slots.
//   codes image  e2m1 [128 channels][32 bytes] = 4 KiB, packed as in memory: a quarter of a bf16 image's footprint
//                and LDS traffic. Filled 16 bytes per lane: the half c (bytes 16 c .. 16 c + 15, k0 + 32 c .. + 31)
//                of channel row r is at slot c ^ ((r >> 3) & 1). A fragment read is a ds_read_b64, served in two
//                halves of 32 lanes: lanes (n, g) with one g >> 1, 16 consecutive rows r0 + n times the two 8-byte
//                halves g & 1 of source half c = g >> 1. Their addresses mod 256 are
//                  32 (r & 7) + 16 (c ^ ((r >> 3) & 1)) + 8 (g & 1):
//                8 x 2 x 2 = 32 distinct 8-byte slots, all 64 banks once. (Unswizzled, rows r and r + 8 share a
//                slot and half the banks idle: a 2-way conflict on every fragment read.)
//   scale image  e8m0 [128 channels][4 bytes] = 512 B per chunk: the four block scales of a channel for one chunk,
//                one 4-byte DMA per lane from waves 0 and 1 (64 channels each, 256 B lane-linear). A lane reads its
//                byte with ds_read_u8 (16 rows x 4 bytes = 64 consecutive bytes per read: no conflict, the four g
//                share two bytes by broadcast) and forms the fp32 scale as byte << 23. Chosen over per-lane dword
//                loads into registers: those join the vmcnt queue of all four waves in every chunk and cost four
//                VGPRs held a chunk ahead, where the image costs waves 0 and 1 one more DMA every other K-tile.
// Two buffers of the x and codes images (by K-tile parity) and two of the scale image (by chunk parity): 41 KiB, so
// three workgroups fit a CU's 160 KiB. A slab is whole chunks, so its K-tiles come in pairs and the K-tile's parity is
// a compile-time constant of the loop body.
//
// Phases and waits. A K-tile is computed in two phases: phase 0 dequantises the wave's four channel fragments (both
// K-steps: 8 v_cvt_scalef32_pk_bf16_fp4 per fragment, each fragment used by all four row blocks) and multiplies row
// blocks 0 and 1, phase 1 multiplies row blocks 2 and 3 with the same weight registers. Staging pieces: P0 = the
// codes image, the x rows with (r >> 5) & 1 == 0 and, for an even K-tile, the chunk's scale image (what phase 0
// reads; 3 DMA instructions per wave, 4 in waves 0 and 1 for an even tile), P1 = the x rows with (r >> 5) & 1 == 1
// (2 instructions). Phase p of tile t waits (counted vmcnt) for piece p of tile t, passes a raw s_barrier, stages
// piece p of tile t + 1 and runs its 16 MFMAs: vmcnt(2) before phase 0 leaves P1(t) in flight, vmcnt(3) before phase
// 1 (vmcnt(4) in waves 0 and 1 when t + 1 is even: a wave-uniform branch) leaves P0(t + 1) in flight, and the queue
// is never drained inside the K loop. No global load stands in front of a K-tile.
//   WAR, x and codes: piece p of the other buffer was last read in phase p of tile t - 1; every wave has passed two
//   barriers since, after consuming those reads.  WAR, scales: the image of chunk q (buffer q & 1) is staged in phase
//   0 of tile 2 q - 1, after that phase's barrier; the buffer was last read in phase 0 of tile 2 q - 3 (chunk q - 2),
//   four barriers earlier, and chunk q - 1, which tile 2 q - 1 is reading, is in the other buffer.
//   RAW: a wave's own vmcnt retires its DMAs (the scale DMA is issued before P1 of its tile, so vmcnt(2) covers it),
//   the barrier after it orders every other wave's. Tile 2 q + 1 reads the scale image again with nothing written
//   to it in between.
//
// Split-K. ceil(M / 128) * ceil(N / 128) tiles can leave most CUs idle, so K is cut into `slabs` contiguous runs of
// chunks (cs_linear_mxfp4_gemm_splits: from M, N, K and the CU count only). With slabs > 1 a workgroup writes its
// fp32 partial to ws[slab][M][N] and linear_mxfp4_combine_kernel (linear_mxfp4.hip) sums the slabs in slab order and
// stores bf16. With slabs == 1 the epilogue stores bf16.
//
// Built without the packed fp32 VALU instructions (_build.py, _NO_PK_FP32_FILES), as every new kernel is.
#include <algorithm>

#include "common.h"
#include "launchers.h"
#include "mxfp4_dequant_device.h"

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

constexpr int kTM = 128, kTN = 128;  // rows of x and channels per workgroup
constexpr int kBK = 64;              // k per K-tile
constexpr int kKC = 128;             // k per chunk: two K-tiles, four scale blocks
constexpr int kThreads = 256;
constexpr int kXImg = kTM * kBK * 2;  // bytes of the bf16 x image
constexpr int kWImg = kTN * kBK / 2;  // bytes of the packed codes image
constexpr int kBuf = kXImg + kWImg;
constexpr int kSImg = kTN * 4;        // bytes of the scale image of one chunk
constexpr int kSBase = 2 * kBuf;      // the two scale images follow the two buffers
constexpr int kOOB = 0x7ffffff0;  // past the end of every descriptor (the launcher bounds their sizes)
constexpr int kMinChunks = 2;     // chunks per slab the heuristic keeps
constexpr int kMaxGrid = 65535;   // slabs ride in gridDim.y
// the heuristic never asks for more fp32 partials than this: slabs * M * N * 4 bytes
constexpr int64_t kMaxWsBytes = (int64_t)256 << 20;

using cs::dequant8;

// the chunks [c0, c1) of part i when n are divided as evenly as possible into parts (linear_mxfp4.hip's rule)
__device__ __forceinline__ void even_part(int n, int parts, int i, int& c0, int& c1) {
  const int base = n / parts, rem = n % parts;
  c0 = i * base + (i < rem ? i : rem);
  c1 = c0 + base + (i < rem ? 1 : 0);
}

template <int N>
__device__ __forceinline__ void wait_vm() {
  if constexpr (N == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  else if constexpr (N == 2) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
  else if constexpr (N == 3) asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
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
__device__ __forceinline__ void dma4(__amdgpu_buffer_rsrc_t rs, char* lds, int off) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void*)lds, 4, off, 0, 0, 0);
}

// What a wave stages of every K-tile. x half h = the tile rows r with (r >> 5) & 1 == h, 8 groups of 8 rows; wave w
// issues groups 2 w and 2 w + 1 of each half: lane l fills chunk slot l & 7 of row r0 + (l >> 3). The codes image
// is 4 groups of 32 channel rows, one per wave: lane l fills slot l & 1 of row 32 w + (l >> 1). The scale image is 2
// groups of 64 channel rows, waves 0 and 1: lane l fills the four bytes of row 64 w + l.
// Per-lane byte offsets at the slab's first K-tile are computed once (kOOB for rows past the operand).
struct Stager {
  __amdgpu_buffer_rsrc_t xrs, wrs, srs;
  int xoff[2][2], woff, soff;  // per lane
  int xlds[2][2], wlds, slds;  // wave-uniform image offsets of the instruction's first row
  bool scales;                 // wave-uniform: this wave stages scales

  // xb / wb / sb: element (first row of the tile, first k of the slab); rows / chans: valid ones from there; kslab:
  // k of the slab. The descriptors end with the slab's last byte of the last valid row.
  __device__ Stager(const __bf16* xb, const unsigned char* wb, const unsigned char* sb, int64_t ldx, int64_t ldw,
                    int64_t lds, int rows, int chans, int kslab, int wv, int lane) {
    xrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<__bf16*>(xb), (short)0,
                                            (int)((int64_t)(rows - 1) * ldx * 2 + (int64_t)kslab * 2), 0x00020000);
    wrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char*>(wb), (short)0,
                                            (int)((int64_t)(chans - 1) * ldw + kslab / 2), 0x00020000);
    srs = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char*>(sb), (short)0,
                                            (int)((int64_t)(chans - 1) * lds + kslab / 32), 0x00020000);
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
    {
      const int r = 32 * wv + (lane >> 1), c = (lane & 1) ^ ((r >> 3) & 1);
      woff = r < chans ? r * (int)ldw + c * 16 : kOOB;
      wlds = kXImg + 32 * wv * 32;
    }
    scales = wv < 2;
    const int rs = 64 * (wv & 1) + lane;
    soff = rs < chans ? rs * (int)lds : kOOB;
    slds = kSBase + 64 * (wv & 1) * 4;
  }
  // piece 0 of local K-tile t into buf: the codes image, x half 0 and, for an even t, the scale image of chunk
  // t / 2 into its buffer (smem: the start of the workgroup's LDS); piece 1: x half 1
  template <bool EVEN>
  __device__ __forceinline__ void piece0(char* smem, char* buf, int t) const {
    dma16(wrs, buf + wlds, woff == kOOB ? kOOB : woff + t * (kBK / 2));
    if constexpr (EVEN) {
      if (scales) dma4(srs, smem + slds + ((t >> 1) & 1) * kSImg, soff == kOOB ? kOOB : soff + (t >> 1) * 4);
    }
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
template <int OFF>
__device__ __forceinline__ u32x2 lds_read8(unsigned addr) {
  u32x2 v;
  asm volatile("ds_read_b64 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF) : "memory");
  return v;
}
template <int OFF>
__device__ __forceinline__ unsigned lds_read1(unsigned addr) {
  unsigned v;
  asm volatile("ds_read_u8 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF) : "memory");
  return v;
}
__device__ __forceinline__ void lds_wait(u32x4 (&a)[4]) {
  asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3])::"memory");
}
__device__ __forceinline__ void lds_wait(u32x2 (&w)[4], unsigned (&s)[4], u32x4 (&a)[4]) {
  asm volatile("s_waitcnt lgkmcnt(0)"
               : "+v"(w[0]), "+v"(w[1]), "+v"(w[2]), "+v"(w[3]), "+v"(s[0]), "+v"(s[1]), "+v"(s[2]), "+v"(s[3]),
                 "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3])::"memory");
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

// Local K-tile t (ODD: its parity, which is its buffer's) of the slab; STAGE: K-tile t + 1 is staged into the
// other buffer meanwhile. lds0: the LDS address of smem; xrd0 / xrd1 / wrd / srd: the lane's fragment offsets inside
// a buffer and inside a scale image (see the kernel)
template <bool STAGE, bool ODD>
__device__ __forceinline__ void ktile(f32x4 (&acc)[4][4], unsigned lds0, char* smem, const Stager& st, int t,
                                      unsigned xrd0, unsigned xrd1, unsigned wrd, unsigned srd) {
  bf16x8 wf[4][2];
  u32x2 wq[4];
  unsigned sc[4];
  u32x4 xq[4];
  const unsigned cur = lds0 + (ODD ? kBuf : 0);
  char* nxt = smem + (ODD ? 0 : kBuf);
  // the lane's scale byte of this K-tile: blocks 2 (t & 1) + (g >> 1) of the chunk, in the chunk's buffer
  const unsigned sa = lds0 + kSBase + ((t >> 1) & 1) * kSImg + srd + (ODD ? 2 : 0);
  wait_vm<2>();  // piece 0 of this tile has landed; piece 1 may be in flight
  barrier();
  if constexpr (STAGE) st.template piece0<ODD>(smem, nxt, t + 1);  // t + 1 is even when t is odd
  wq[0] = lds_read8<0>(cur + wrd);  // channel block cb is 16 channels = 512 bytes of codes, 64 of scales further
  wq[1] = lds_read8<512>(cur + wrd);
  wq[2] = lds_read8<1024>(cur + wrd);
  wq[3] = lds_read8<1536>(cur + wrd);
  sc[0] = lds_read1<0>(sa);
  sc[1] = lds_read1<64>(sa);
  sc[2] = lds_read1<128>(sa);
  sc[3] = lds_read1<192>(sa);
  read_x<0>(xq, cur + xrd0, cur + xrd1);
  lds_wait(wq, sc, xq);
#pragma unroll
  for (int cb = 0; cb < 4; ++cb) {
    const float scale = __uint_as_float(sc[cb] << 23);  // 2^(byte - 127)
    wf[cb][0] = dequant8(wq[cb][0], scale);  // K-step 0: bytes 0..3, k = k0 + 16 g + j
    wf[cb][1] = dequant8(wq[cb][1], scale);  // K-step 1: bytes 4..7, k = k0 + 16 g + 8 + j
  }
  mma_half<0>(acc, wf, xq);
  // piece 1 of this tile has landed; piece 0 of the next may be in flight: 3 instructions, 4 where it holds scales
  if constexpr (!STAGE) wait_vm<0>();
  else if constexpr (!ODD) wait_vm<3>();
  else if (st.scales) wait_vm<4>();
  else wait_vm<3>();
  barrier();
  if constexpr (STAGE) st.piece1(nxt, t + 1);
  read_x<2>(xq, cur + xrd0, cur + xrd1);
  lds_wait(xq);
  mma_half<2>(acc, wf, xq);
}

__global__ __launch_bounds__(kThreads, 3) void linear_mxfp4_gemm_kernel(const __bf16* __restrict__ x,
                                                                      const unsigned char* __restrict__ codes,
                                                                      const unsigned char* __restrict__ scales,
                                                                      __bf16* __restrict__ y, float* __restrict__ ws,
                                                                      int M, int N, int K, int64_t ldx, int64_t ldw,
                                                                      int64_t lds, int slabs) {
  __shared__ __attribute__((aligned(1024))) char smem[2 * kBuf + 2 * kSImg];
  const int nM = (M + kTM - 1) / kTM;
  const int tm = blockIdx.x % nM, tn = blockIdx.x / nM, slab = blockIdx.y;
  const int m0 = tm * kTM, n0 = tn * kTN;
  const int rows = M - m0 < kTM ? M - m0 : kTM, chans = N - n0 < kTN ? N - n0 : kTN;
  int c0, c1;
  even_part(K / kKC, slabs, slab, c0, c1);  // slabs <= K / 128: never empty
  const int nk = 2 * (c1 - c0);             // K-tiles: an even number

  const int lane = threadIdx.x & 63, n = lane & 15, g = lane >> 4;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), wr = wv >> 1, wc = wv & 1;
  const Stager st(x + (int64_t)m0 * ldx + (int64_t)c0 * kKC, codes + (int64_t)n0 * ldw + (int64_t)c0 * (kKC / 2),
                  scales + (int64_t)n0 * lds + (int64_t)c0 * (kKC / 32), ldx, ldw, lds, rows, chans, (c1 - c0) * kKC,
                  wv, lane);

  // the lane's fragment addresses inside a buffer, for row block 0 / channel block 0 and K-step 0. Row
  // r = 64 wr + 16 rb + n has (r >> 1) & 7 == (n >> 1) & 7 and channel row r = 64 wc + 16 cb + n has
  // (r >> 3) & 1 == (n >> 3) & 1 for every block, so the blocks are constant strides apart; x chunk 2 g + s sits at
  // slot (2 g + s) ^ ((n >> 1) & 7), the code bytes 8 g .. 8 g + 7 in half (g >> 1) ^ ((n >> 3) & 1) at 8 (g & 1)
  const unsigned xrd0 = (64 * wr + n) * 128 + (((2 * g) ^ ((n >> 1) & 7)) << 4);
  const unsigned xrd1 = (64 * wr + n) * 128 + (((2 * g + 1) ^ ((n >> 1) & 7)) << 4);
  const unsigned wrd = kXImg + (64 * wc + n) * 32 + ((((g >> 1) ^ ((n >> 3) & 1))) << 4) + ((g & 1) << 3);
  const unsigned srd = (64 * wc + n) * 4 + (g >> 1);
  const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char*)smem;

  f32x4 acc[4][4];
#pragma unroll
  for (int rb = 0; rb < 4; ++rb)
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) acc[rb][cb] = f32x4{0.f, 0.f, 0.f, 0.f};

  st.piece0<true>(smem, smem, 0);
  st.piece1(smem, 0);
  int t = 0;
  for (; t + 2 < nk; t += 2) {
    ktile<true, false>(acc, lds0, smem, st, t, xrd0, xrd1, wrd, srd);
    ktile<true, true>(acc, lds0, smem, st, t + 1, xrd0, xrd1, wrd, srd);
  }
  ktile<true, false>(acc, lds0, smem, st, t, xrd0, xrd1, wrd, srd);
  ktile<false, true>(acc, lds0, smem, st, t + 1, xrd0, xrd1, wrd, srd);

  // epilogue: register j of acc[rb][cb] is y[m0 + 64 wr + 16 rb + n][n0 + 64 wc + 16 cb + 4 g + j].
  // N % 8 == 0 and ch % 4 == 0: ch < N means ch + 3 < N
#pragma unroll
  for (int cb = 0; cb < 4; ++cb) {
    const int ch = n0 + 64 * wc + 16 * cb + 4 * g;
    if (ch >= N) continue;
#pragma unroll
    for (int rb = 0; rb < 4; ++rb) {
      const int m = m0 + 64 * wr + 16 * rb + n;
      if (m >= M) continue;
      if (slabs == 1) {
        const f32x4 v = acc[rb][cb];
        const bf16x4 o = {(__bf16)v[0], (__bf16)v[1], (__bf16)v[2], (__bf16)v[3]};
        *reinterpret_cast<bf16x4*>(y + (size_t)m * N + ch) = o;
      } else {
        *reinterpret_cast<f32x4*>(ws + ((size_t)slab * M + m) * N + ch) = acc[rb][cb];
      }
    }
  }
}

bool aligned(const void* p, uintptr_t a) { return p != nullptr && reinterpret_cast<uintptr_t>(p) % a == 0; }

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

int cs_linear_mxfp4_gemm_max_splits(int K) {
  const int n = K / kKC;
  return n < 1 ? 1 : (n > kMaxGrid ? kMaxGrid : n);
}

int64_t cs_linear_mxfp4_gemm_max_ldx() { return (kOOB - 1) / (2 * kTM); }
int64_t cs_linear_mxfp4_gemm_max_ldw() { return (kOOB - 1) / kTN; }
int64_t cs_linear_mxfp4_gemm_max_lds() { return (kOOB - 1) / kTN; }

int cs_linear_mxfp4_gemm_splits(int M, int N, int K) {
  if (M < 1 || N < 1 || K < kKC) return 1;
  const int64_t tiles = (int64_t)((M + kTM - 1) / kTM) * ((N + kTN - 1) / kTN);
  const int cus = cu_count();
  if (tiles >= cus) return 1;  // every CU has a tile already
  // aimed at: two workgroups per CU. Kept: kMinChunks chunks per slab, and partials that cost no more than twice
  // the weight bytes: a slab writes and the combine reads M * N * 4 bytes, the codes are N * K / 2
  int64_t n = 2 * (int64_t)cus / tiles;
  n = std::min<int64_t>(n, K / kKC / kMinChunks);
  n = std::min<int64_t>(n, (int64_t)K / (8 * (int64_t)M));
  if (n < 2 || n * M * N * 4 > kMaxWsBytes) return 1;
  return (int)n;
}

hipError_t cs_linear_mxfp4_gemm(const void* x, const void* codes, const void* scales, void* y, float* ws, int M, int N,
                                int K, size_t ldx, size_t ldw, size_t lds, int slabs, hipStream_t stream) {
  if (M == 0 || N == 0) return hipSuccess;
  if (M < 0 || N < 0 || N % 8 != 0 || K < kKC || K % kKC != 0) return hipErrorInvalidValue;
  if (ldx < (size_t)K || ldx % 8 != 0 || ldw < (size_t)K / 2 || ldw % 16 != 0 || lds < (size_t)K / 32 || lds % 4 != 0)
    return hipErrorInvalidValue;
  // 32-bit offsets inside a descriptor: a tile addresses 128 rows of its operand, so the last byte it can name is
  // below 128 * ldx * 2 (x), 128 * ldw (codes) or 128 * lds (scales), which must stay below kOOB
  if (ldx > (size_t)cs_linear_mxfp4_gemm_max_ldx() || ldw > (size_t)cs_linear_mxfp4_gemm_max_ldw() ||
      lds > (size_t)cs_linear_mxfp4_gemm_max_lds())
    return hipErrorInvalidValue;
  if (!aligned(x, 16) || !aligned(codes, 16) || !aligned(scales, 4) || !aligned(y, 16)) return hipErrorInvalidValue;
  if (slabs < 1 || slabs > cs_linear_mxfp4_gemm_max_splits(K)) return hipErrorInvalidValue;
  if (slabs > 1 && !aligned(ws, 16)) return hipErrorInvalidValue;
  const int64_t tiles = (int64_t)((M + kTM - 1) / kTM) * ((N + kTN - 1) / kTN);
  if (tiles > 0x7fffffff) return hipErrorInvalidValue;
  hipLaunchKernelGGL(linear_mxfp4_gemm_kernel, dim3((unsigned)tiles, (unsigned)slabs), dim3(kThreads), 0, stream,
                     (const __bf16*)x, (const unsigned char*)codes, (const unsigned char*)scales, (__bf16*)y, ws, M, N, K,
                     (int64_t)ldx, (int64_t)ldw, (int64_t)lds, slabs);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess || slabs == 1) return e;
  return cs_linear_mxfp4_combine(ws, y, M, N, slabs, stream);
}
