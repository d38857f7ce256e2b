// Host-side launch API of the gfx950 kernels (raw pointers + stream; no torch headers,
// so every .hip compiles in seconds and the kernels are reusable from the C++ runtime).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

struct CsTensorEntry {
  float* p;
  float* g;
  float* m;
  int64_t n;
  uint16_t* shadow;  // optional bf16 copy of p, rewritten by the update (the bf16 GEMMs' operand)
};

// data pipeline
hipError_t cs_augment(const uint8_t* data, const int64_t* idx, const int32_t* params, float* out, int B, int nhwc,
                      int cstride, const float* mean, const float* std_, hipStream_t stream);
hipError_t cs_gather_labels(const int64_t* labels, const int64_t* idx, int64_t* out, int B, hipStream_t stream);
// engine batch: sample = perm[*cursor * stride + b] (or idx_in[b] when perm is null) -> NHWC x4 input, idx_out, labels
hipError_t cs_make_batch(const uint8_t* data, const int64_t* labels, const int64_t* perm, const int64_t* cursor,
                         int stride, const int64_t* idx_in, const int32_t* params, float* out, int64_t* idx_out,
                         int64_t* ylab, int B, const float* mean, const float* std_, hipStream_t stream);

// optimizer
// counter (optional): incremented once by the launch (the engine's device-side step cursor)
// The F3 conv math's weight bounds, produced by the SGD launch that writes the weights: up to
// CS_WB_MAX conv-weight intervals [lo, hi) (element offsets relative to the launch's range start),
// each with the CS_AMAX_SLOT bound the absolute maximum of its updated elements is folded into. Each
// element counts for the interval that holds it, so the bounds are exact per weight tensor whatever
// the SGD launch's range (a block, a bucket, the whole buffer). n == 0: none.
#define CS_WB_MAX 16
struct CsWeightBounds {
  int64_t lo[CS_WB_MAX], hi[CS_WB_MAX];
  float* amax[CS_WB_MAX];
  int n;
};
// the absolute maximum of x[0, n) folded (atomic max) into one CS_AMAX_SLOT bound
hipError_t cs_amax(const float* x, int64_t n, float* amax, hipStream_t stream);
// F3 weight bounds of the blocks in `mask`: cur = next, next = 0 (CS_AMAX_SLOT slots, block l at l)
hipError_t cs_amax_rotate(float* cur, float* next, unsigned mask, int L, hipStream_t stream);
hipError_t cs_sgd_flat(float* p, const float* g, float* m, int64_t n, float lr, float mom, float wd, float damp,
                       float scale, int first, hipStream_t stream, int64_t* counter = nullptr,
                       const CsWeightBounds* wb = nullptr);
// faithful sync modes on flat gradients (flat_ops.hip): dst = mean over `rows` rows of src [rows][n];
// g = g + t, then / div when div > 0
hipError_t cs_rows_mean(float* src, int rows, int64_t n, float* dst, int bcast, hipStream_t stream);
hipError_t cs_accumulate(float* g, const float* t, int64_t n, float div, hipStream_t stream);
// bf16 gradient transport: to_bf16 = 1: fp32 src -> bf16 dst (round to nearest even); 0: bf16 -> fp32
hipError_t cs_cast_grad(const void* src, void* dst, int64_t n, int to_bf16, hipStream_t stream);
hipError_t cs_sgd_multi(const CsTensorEntry* tab_dev, int ntens, const int64_t* chunk_start_dev, int nchunks,
                        float lr, float mom, float wd, float damp, float scale, int first, hipStream_t stream);

// AdamW with global-norm gradient clipping (adamw.hip): a table of its own, walked in the same
// 4096-element chunks as cs_sgd_multi (chunk starts as a prefix array over the whole table)
struct CsAdamEntry {
  float* p;
  float* g;
  float* m;  // exp_avg
  float* v;  // exp_avg_sq
  int64_t n;
  uint16_t* shadow;  // optional bf16 copy of p, rewritten by the update
  int64_t flags;     // CS_ADAM_VEC: every pointer allows 4-element vector access; CS_ADAM_VEC_G: g does
};
#define CS_ADAM_VEC 1
#define CS_ADAM_VEC_G 2
#define CS_ADAM_PARTIALS 2048
// partials[CS_ADAM_PARTIALS] (double): block b's sum of (g * grad_scale)^2 over chunks b, b + grid, ...
// of the whole table, the slots past the grid zeroed. No atomics: the same table gives the same bits.
hipError_t cs_grad_sumsq(const CsAdamEntry* tab_dev, int ntens, const int64_t* chunk_start_dev, int nchunks,
                         float grad_scale, double* partials, hipStream_t stream);
// The update of the tensors [0, ntens) of tab_dev (a contiguous run of the table: one parameter group),
// whose chunks are [first_chunk, first_chunk + nchunks) of the table's numbering. partials != nullptr:
// the gradient is clipped to max_norm by the global norm (torch's clip_grad_norm_ coefficient) and the
// norm is written to norm_out. bc1 = 1 - beta1^step and bc2 = 1 - beta2^step come from the host; the
// launcher folds 1 - lr*wd, lr/bc1 and sqrt(bc2) in double and rounds each to float once, as torch does.
hipError_t cs_adamw_multi(const CsAdamEntry* tab_dev, int ntens, const int64_t* chunk_start_dev, int first_chunk,
                          int nchunks, double lr, double beta1, double beta2, double eps, double wd, double bc1,
                          double bc2, float grad_scale, float max_norm, const double* partials, float* norm_out,
                          hipStream_t stream);

// classifier head
// bn (optional, part 0 / 1): the features are the last VGG block's BatchNorm + ReLU + 2x2 max-pool of
// its pre-BN output y [B][2][2][K] (scale / shift per channel), computed in the row pass (bn_apply's
// arithmetic and max order: the same bits) and written to feat for the column pass
// the classifier's per-column pass (dW, db, loss, correct count) as data (P = C*ceil(K/64)+1
// wave-sized pieces)
struct CsHeadCols {
  const float* feat;
  int B, K, C;
  const float* ws;
  float* dW;
  float* db;
  float* loss_out;
  int* correct_out;
  int P;
};
inline int cs_head_cols_pieces(int K, int C) { return C * ((K + 63) / 64) + 1; }
struct CsHeadBn {
  const float* y;
  const float* scale;
  const float* shift;
};
hipError_t cs_linear_xent(const float* feat, const float* W, const float* bias, const int64_t* labels, int B, int K,
                          int C, float gscale, float* loss_out, int* correct_out, float* logits_out, float* dW,
                          float* db, float* dfeat, int64_t* pred_out, float* ws, hipStream_t stream, int part = 0,
                          const CsHeadBn* bn = nullptr);
// part: 0 both launches; 1 the per-row pass (logits, prediction, dlogits -> ws, dfeat); 2 the
// per-column pass (dW, db, loss, correct count from ws and feat) — run after part 1 (ws)
inline int64_t cs_linear_xent_ws(int B, int C) { return (int64_t)B * (C + 2); }
hipError_t cs_softmax_xent(const float* logits, const int64_t* labels, int B, int C, float gscale, float* loss_out,
                           float* dlogits, int* correct_out, hipStream_t stream);

// ---------------------------------------------------------------- conv (implicit GEMM, fp32 MFMA)
enum { CS_CONV_FWD = 0, CS_CONV_DGRAD = 1, CS_CONV_WGRAD = 2 };
// operand absolute-maximum bounds (the F3 conv math's scales) are kept as CS_AMAX_SHARDS shards,
// each the atomic max of the producer workgroups with blockIdx % CS_AMAX_SHARDS == shard (one atomic
// per workgroup, shards CS_AMAX_STRIDE floats = one 128-byte line apart: no hot word or line), and
// the bound is the largest shard; a slot is CS_AMAX_SLOT floats
#define CS_AMAX_SHARDS 64
#define CS_AMAX_STRIDE 32
#define CS_AMAX_SLOT (CS_AMAX_SHARDS * CS_AMAX_STRIDE)

// One BN-backward partial-sum pass (bn.hip "reduce"): y, incoming gradient G, the forward's
// scale/shift/mean/invstd, partials out part [P][C][3]. P == 0: none.
struct CsBnRed {
  const float *y, *G, *scale, *shift, *mean, *invstd;
  float* part;
  int B, H, W, C, pool, P;
};

// An SGD update of one parameter range carried by extra blocks appended to a GEMM launch (after
// its tiles, like CsBnRed): P blocks (the launcher sizes it when n > 0); n == 0: none.
struct CsSgdTail {
  float* p;
  const float* g;
  float* m;
  int64_t n;
  float lr, mom, wd, damp;
  int first, P;
  CsWeightBounds wb;  // optional (wb.n == 0): the weights' bounds for the F3 conv math
};

// BatchNorm finalize by the last-arriving block of the launch that produces the statistics
// partials (bn_fin.h): FWD with CsConvArgs::stats (scale / shift / mean / invstd -> bnv [4][C],
// running stats, num_batches_tracked), BWD with CsConvArgs::ered (coef [C][3], dgamma, dbeta,
// dbias; ered.part is then [T][C][4]). cnt == null: off (the separate finalize launch runs).
struct CsBnFin {
  int* cnt;    // zeroed ticket counters, >= cs_bn_fin_ints(...) ints (left zeroed by the launch)
  float* grp;  // level-1 group partials, >= cs_bn_fin_grp_floats(...) floats
  int T, R, M;  // row tiles of the partials, rows per tile, rows (the last tile may be short)
  int count;    // BWD: elements per channel of the BN layer (full resolution) for the means
  const float *gamma, *beta, *invstd;  // invstd: BWD (the forward's)
  float *rmean, *rvar;                 // FWD running stats (may be null)
  int64_t* nbt;                        // FWD (may be null)
  float momentum, eps;
  float* bnv;                          // FWD out [4][C]
  float *coef, *dgamma, *dbeta, *dbias;  // BWD out (dgamma / dbeta / dbias may be null)
};
// tickets and group-partial floats a launch needs for T row tiles of C channels in column
// tiles of nc channels (64 or 128)
inline int cs_bn_fin_groups(int T, int nc) { return (T + 8 * (256 / nc) - 1) / (8 * (256 / nc)); }
inline int cs_bn_fin_ints(int T, int C, int nc) { return ((C + nc - 1) / nc) * (cs_bn_fin_groups(T, nc) + 1); }
inline int64_t cs_bn_fin_grp_floats(int T, int C, int nc) { return (int64_t)cs_bn_fin_groups(T, nc) * C * 4; }

struct CsConvArgs {
  const float* x;     // FWD / WGRAD: conv input, NHWC [B,H,W,Cin] (Cin = 4 for the padded conv0 input)
  const float* w;     // FWD / DGRAD: weights, OHWI [Cout][9][Cin]; conv0 (w_oihw=1): OIHW [Cout][3][9]
  const float* dz;    // DGRAD / WGRAD: gradient w.r.t. conv output, NHWC [B,H,W,Cout]
  const float* bias;  // FWD: [Cout] or null
  float* out;         // FWD: y [M][Cout]; DGRAD: dx [M][Cin]; WGRAD: dW (OHWI, or OIHW for conv0)
  float* ws;          // split-K slabs [splits][M][N] (required when splits > 1)
  float* stats;       // FWD: per-row-tile BN partials [tiles][Cout][2] = (mean, M2); may be null
  int B, H, W, Cin, Cout;
  int w_oihw;
  // DGRAD: the BN-backward partial sums of the block below (whose output gradient this GEMM
  // produces), taken from the finished output values where they are still in registers — the
  // GEMM epilogue, or the split-K combine — instead of a separate reduce pass over G and y.
  // Uses y, scale, shift, mean, invstd, pool and part ([row tiles][N][3], row tiles of BM rows,
  // or CS_SPLITK_STAT_ROWS behind the split-K combine: cs_conv_ered_rows); part == null: none
  CsBnRed ered;
  // an independent SGD update appended to the launch (the serial world-1 step: block l+1's
  // parameters, whose last reader has run, ride block l's weight-gradient GEMM)
  CsSgdTail sgd;
  // CS_STAGE_F3: device pointers to CS_AMAX_SLOT bounds (largest shard) of |A| / |B| (the
  // GEMM's A operand: FWD x, DGRAD / WGRAD dz; B: FWD / DGRAD w, WGRAD x); each sets its operand's
  // power-of-two scale
  const float* amax_a;
  const float* amax_b;
  // FWD (with stats) / DGRAD (with ered): the BN finalize by the launch's last-arriving block
  // (or the split-K combine's); fin.cnt == null: off
  CsBnFin fin;
  // filled by the launcher:
  int lgH, lgW, lgCin, lgCout, M, N, K, ksteps_per_split, total_ksteps;
};

void cs_conv_fill_dims(CsConvArgs* a, int mode);

// VGG block 0 (3 -> 64 channels, 32 x 32, input padded to 4 channels NHWC, OIHW weights) as direct
// f32 kernels (conv0.hip). fwd: y [pix][64] (+bias) and, when stats != null, the BatchNorm tile
// statistics [pix / cs_conv0_tile_rows()][64][2] = (mean, M2); wgrad: dW (OIHW [64][27]) through
// `part` scratch of cs_conv0_wgrad_part_floats() floats (fixed-order sum: deterministic)
// the training batch itself (augment.hip make_batch's job) as conv0's input source: sample index
// (device cursor into the permutation, or idx_in), label gather, RandomCrop(32, 4) + HFlip +
// Normalize of the uint8 images straight into the conv's LDS halo; the block-0 input x_out
// (for the weight gradient) is written as make_batch writes it
struct CsBatchSrc {
  const uint8_t* data;
  const int64_t* labels;
  const int64_t* perm;
  const int64_t* cursor;
  int stride;
  const int64_t* idx_in;
  const int32_t* params;
  float* x_out;
  int64_t* idx_out;
  int64_t* ylab;
  float m[3], inv[3];
};
int cs_conv0_tile_rows();
size_t cs_conv0_wgrad_part_floats(int B, int H, int W);
// zero_bounds (optional): zero_slots F3 operand bounds (CS_AMAX_SLOT apart) this launch resets;
// rot_cur / rot_next / rot_mask (optional): the weight-bound rotation of cs_amax_rotate, folded in
hipError_t cs_conv0_fwd(const float* x, const float* w, const float* bias, float* y, float* stats, int B, int H,
                        int W, int Cout, hipStream_t stream, const CsBatchSrc* batch = nullptr,
                        float* zero_bounds = nullptr, int zero_slots = 0, float* rot_cur = nullptr,
                        float* rot_next = nullptr, unsigned rot_mask = 0);
// sgd (optional): block 0's parameter range, whose SGD step then rides the fixed-order sum (dW at
// w_rel within the range; the range's other gradients must be final; counter: the batch cursor)
hipError_t cs_conv0_wgrad(const float* x, const float* dz, float* part, float* dw, int B, int H, int W, int Cout,
                          hipStream_t stream, const CsSgdTail* sgd = nullptr, int w_rel = 0,
                          int64_t* counter = nullptr);
// the same weight gradient with block 0's BN (+ReLU, 2x2 max-pool) backward apply folded in: dZ is
// computed in LDS from y (pre-BN conv output), G (gradient of the pooled output), the forward's
// scale/shift/mean/invstd and the backward finalize's coef [C][3] (cs_bn_bwd_finalize) — the
// same bits as cs_bn_bwd_tail's dZ, never written to memory
hipError_t cs_conv0_wgrad_bn(const float* x, const float* y, const float* G, const float* scale, const float* shift,
                             const float* mean, const float* invstd, const float* coef, float* part, float* dw, int B,
                             int H, int W, int Cout, hipStream_t stream, const CsSgdTail* sgd = nullptr,
                             int w_rel = 0, int64_t* counter = nullptr);
// bm, bn in {64, 128}; bk in {16, 32}; splits >= 1 (split-K over blockIdx.z + deterministic reduce).
// FWD stats tiles have `bm` rows when splits == 1 and CS_SPLITK_STAT_ROWS rows otherwise.
#define CS_SPLITK_STAT_ROWS 16
// stage: CS_STAGE_REGS (global -> registers -> ds_write, padded LDS) or CS_STAGE_LDS_DMA(_DEEP)
// (buffer_load ... lds into a 3- (5-) deep ring of swizzled images; bk = 32, not conv0's fwd;
// the deep ring only where 5 images fit the 160 KiB LDS)
// CS_STAGE_KG2 / KG4: register staging with 2 / 4 K-groups of 4 waves per block (bk >= 32 / 64)
// | CS_STAGE_X6: the same staging with fp32-accurate split-bf16 math (3 bf16 pieces per
// operand, 6 v_mfma_f32_32x32x16_bf16 per 32x32x16 product; conv_gemm.hip "X6")
// | CS_STAGE_X6S: X6 math with the split done once at the LDS store into bf16 planes (register
// staging / K-groups only; bk 64 only with 64x64 tiles)
// | CS_STAGE_BF16: operands rounded to bf16 at the LDS store, one bf16 MFMA, f32 accumulate
// (reduced precision: only for the engine's opt-in bf16 mode, never picked by the f32 autotune)
// | CS_STAGE_F3: fp32-class split into two fp16 planes of the power-of-two-scaled operand (scales
// from CsConvArgs::amax_a / amax_b, required), 3 v_mfma_f32_32x32x16_f16 per product (conv_gemm.hip "F3")
enum { CS_STAGE_REGS = 0, CS_STAGE_LDS_DMA = 1, CS_STAGE_LDS_DMA_DEEP = 2, CS_STAGE_KG2 = 3, CS_STAGE_KG4 = 4,
       CS_STAGE_X6 = 8, CS_STAGE_X6S = 16, CS_STAGE_BF16 = 32, CS_STAGE_F3 = 64 };
// whether a (stage, tile, bk) combination has a kernel
bool cs_conv_stage_ok(int stage, int bm, int bn, int bk, bool conv0_fwd);
hipError_t cs_conv_gemm(CsConvArgs a, int mode, int bm, int bn, int bk, int splits, hipStream_t stream,
                        int stage = CS_STAGE_REGS);
// deterministic split-K combine of `splits` fp32 slabs in a.ws (dims filled): sum in split order
// (+bias and BN tile statistics of CS_SPLITK_STAT_ROWS rows for FWD; conv0's OIHW scatter for WGRAD)
hipError_t cs_conv_splitk_reduce(const CsConvArgs& a, int mode, int splits, hipStream_t stream);
// the split count cs_conv_gemm actually launches (K-steps re-balanced over splits)
int cs_conv_effective_splits(int K, int bk, int splits);
// FWD statistics tile height for a launch (bm, or CS_SPLITK_STAT_ROWS behind the reduce kernel)
int cs_conv_stat_rows(int K, int bm, int bk, int splits);
// rows per BN-backward partial of a DGRAD launch carrying `ered` (bm, or CS_SPLITK_STAT_ROWS
// when split-K: the combine launch computes them)
int cs_conv_ered_rows(int K, int bm, int bk, int splits);

// ---------------------------------------------------------------- BatchNorm + ReLU (+ 2x2 max-pool), NHWC
hipError_t cs_bn_finalize(const float* part, int T, int R, int M, int C, const float* gamma, const float* beta,
                          float* running_mean, float* running_var, int64_t* nbt, float momentum, float eps,
                          float* scale, float* shift, float* save_mean, float* save_invstd, hipStream_t stream);
hipError_t cs_bn_eval_coeffs(const float* gamma, const float* beta, const float* rm, const float* rv, int C, float eps,
                             float* scale, float* shift, hipStream_t stream);
// amax (optional): a CS_AMAX_SLOT bound the output's absolute maximum is atomically folded into
// (the F3 conv math's operand bound); the same for dz in the BN-backward launchers below
hipError_t cs_bn_apply(const float* y, const float* scale, const float* shift, float* out, int B, int H, int W, int C,
                       int pool, hipStream_t stream, float* amax = nullptr);
int cs_bn_bwd_blocks(int B, int H, int W, int C, int pool);
// part: [cs_bn_bwd_blocks][C][3] scratch; coef: [C][3] scratch; dgamma/dbeta/dbias may be null.
// LDS bytes the BN-backward reduce body needs (C channels)
inline size_t cs_bn_red_lds(int C) { return (size_t)(256 / (C / 4)) * C * 3 * sizeof(float); }
// finalize + apply of the BN backward when the reduce already ran (part from P blocks, e.g.
// appended to the weight-gradient GEMM launch of the block above, or P row tiles of the data-
// gradient GEMM that produced G: CsConvArgs::ered); signal: optional stream-link counter the
// finalize launch bumps when it starts
hipError_t cs_bn_bwd_tail(const float* y, const float* G, int B, int H, int W, int C, int pool, const float* scale,
                          const float* shift, const float* mean, const float* invstd, const float* gamma,
                          const float* part, int P, float* coef, float* dgamma, float* dbeta, float* dbias, float* dz,
                          hipStream_t stream, unsigned long long* signal = nullptr, float* amax = nullptr);
// the finalize half of cs_bn_bwd_tail alone (coef, dgamma / dbeta / dbias), for a consumer that
// applies the backward itself (cs_conv0_wgrad_bn)
hipError_t cs_bn_bwd_finalize(const float* part, int P, int C, int M, const float* gamma, const float* invstd,
                              float* coef, float* dgamma, float* dbeta, float* dbias, hipStream_t stream,
                              unsigned long long* signal = nullptr);
hipError_t cs_bn_bwd(const float* y, const float* G, int B, int H, int W, int C, int pool, const float* scale,
                     const float* shift, const float* mean, const float* invstd, const float* gamma, float* part,
                     float* coef, float* dgamma, float* dbeta, float* dbias, float* dz, hipStream_t stream,
                     float* amax = nullptr);

// single-launch BN for small layers (one block per 16 channels owns all their rows):
// forward = finalize (tile partials -> bnv [4][C] = scale, shift, mean, invstd + running stats)
// + normalize/ReLU(/pool); backward = reduce + finalize + apply (coef [C][3] scratch)
hipError_t cs_bn_fused_fwd(const float* part, int T, int R, int M, int C, const float* gamma, const float* beta,
                           float* running_mean, float* running_var, int64_t* nbt, float momentum, float eps,
                           float* bnv, const float* y, float* out, int B, int H, int W, int pool, hipStream_t stream);
hipError_t cs_bn_fused_bwd(const float* y, const float* G, int B, int H, int W, int C, int pool, const float* bnv,
                           const float* gamma, float* coef, float* dgamma, float* dbeta, float* dbias, float* dz,
                           hipStream_t stream, unsigned long long* signal = nullptr, float* amax = nullptr);
// finalize + apply of the BN backward in ONE launch when the reduce already ran (the data-gradient
// epilogue's P row-tile partials [P][C][3], CsConvArgs::ered): grid (C/16, row chunks), every block
// finalizes its 16 channels from the P partials (the same fixed-order sum in every block), block row
// 0 publishes coef / dgamma / dbeta / dbias, each block applies dZ to its chunk of rows — the
// backward twin of cs_bn_fused_fwd (one launch boundary fewer than cs_bn_bwd_tail)
hipError_t cs_bn_bwd_tail_fused(const float* y, const float* G, int B, int H, int W, int C, int pool, const float* bnv,
                                const float* gamma, const float* part, int P, float* coef, float* dgamma, float* dbeta,
                                float* dbias, float* dz, hipStream_t stream, unsigned long long* signal = nullptr);
// the BN backward's apply pass alone (dZ from G, y and the finalized coef [C][3]): the finalize
// ran as the last-arriver tail of the data-gradient launch that produced G (CsConvArgs::fin)
hipError_t cs_bn_bwd_apply(const float* y, const float* G, int B, int H, int W, int C, int pool, const float* scale,
                           const float* shift, const float* mean, const float* invstd, const float* coef, float* dz,
                           hipStream_t stream, unsigned long long* signal = nullptr);

// ---------------------------------------------------------------- ordering-probe communicator (comm_probe.hip)
enum { CS_SCRAMBLE_F32 = 0, CS_SCRAMBLE_I64 = 1, CS_SCRAMBLE_I32 = 2 };
// a bounded (<= 0.1 s) busy wait of `us` microseconds on `stream`
// ctas > 0: that many busy 256-thread workgroups (an RCCL collective's CTA footprint) instead
// of one sleeping wave; sink: 256 floats never written in practice
hipError_t cs_comm_spin(double us, hipStream_t stream, int ctas = 0, float* sink = nullptr);
// exact invertible scramble: floats x2 (inverse x0.5), integers +1 (inverse -1)
hipError_t cs_comm_scramble(void* buf, int64_t n, int kind, int inverse, hipStream_t stream);

// ---------------------------------------------------------------- stream links (stream_link.hip)
// signal: count += 1 on `stream`; wait: *expect += delta, then poll until count >= *expect.
// The wait ends early only when the host sets *abort (host-mapped; *err = 2) or after timeout_s
// (*err = 1; the engine sets it to the communicator timeout, so the step watchdog fires
// first). count / expect: device memory, zeroed; err / abort: host-mapped.
hipError_t cs_link_signal(unsigned long long* count, hipStream_t stream);
hipError_t cs_link_wait(const unsigned long long* count, unsigned long long* expect, int* err, const int* abort,
                        double timeout_s, hipStream_t stream, unsigned long long delta = 1);

// Diagnostic shader-clock sampler (clock_probe.hip; scripts/ramp_clock.py): out holds
// max_samples + 1 pairs (s_memrealtime, s_memtime), 0-terminated when stopped early; stop and
// slots: device memory, zeroed. Not used by the engine.
hipError_t cs_clock_sampler(unsigned long long* out, int max_samples, int* stop, hipStream_t stream);
hipError_t cs_clock_stamp(unsigned long long* slots, int i, hipStream_t stream);
hipError_t cs_clock_stop(int* stop, hipStream_t stream);

// ---------------------------------------------------------------- decoder-LM elementwise ops (lm.hip)
enum { CS_F32 = 0, CS_BF16 = 1, CS_F16 = 2 };  // CS_F16: the sampler's logits only
int cs_rmsnorm_bwd_partials(int rows, int D);
// whether RMSNorm of width D runs the 4-wide kernels (D % 4 == 0 and D <= 8192): their 16-byte (fp32) /
// 8-byte (bf16) accesses need x, w, y, g, dx and dw 16-byte aligned, and only they mix dtypes
bool cs_rmsnorm_vec4(int D);
// y has dtype odt (e.g. bf16 out of an fp32 residual stream under autocast; odt != dt needs cs_rmsnorm_vec4(D))
hipError_t cs_rmsnorm_fwd(int dt, int wdt, int odt, const void* x, const void* w, void* y, float* rstd, int rows,
                          int D, float eps, hipStream_t s);
// part: [cs_rmsnorm_bwd_partials(rows, D)][D] fp32 scratch; dw has the weight's dtype, g dtype gdt, dx x's
hipError_t cs_rmsnorm_bwd(int dt, int wdt, int gdt, const void* x, const void* w, const float* rstd, const void* g,
                          void* dx, void* dw, float* part, int rows, int D, hipStream_t s);
// residual add fused into the norm: h = x + delta (x's dtype dt, rounded once), y = rms_norm(h, w) of dtype
// odt, rstd of h as stored. delta has dtype ddt; ddt != dt and odt != dt need cs_rmsnorm_vec4(D)
hipError_t cs_add_rmsnorm_fwd(int dt, int ddt, int wdt, int odt, const void* x, const void* delta, const void* w,
                              void* h, void* y, float* rstd, int rows, int D, float eps, hipStream_t s);
// d = gh + (the norm's dx of g), stored to dx in h's dtype dt and / or to ddelta in dtype ddt; gh (dtype dt),
// dx and ddelta may each be null (gh: no gradient reaches h itself; dx, ddelta: not wanted). dw and part as
// cs_rmsnorm_bwd. ddelta and gdt != dt need cs_rmsnorm_vec4(D)
hipError_t cs_add_rmsnorm_bwd(int dt, int wdt, int gdt, int ddt, const void* h, const void* w, const float* rstd,
                              const void* g, const void* gh, void* dx, void* ddelta, void* dw, float* part, int rows,
                              int D, hipStream_t s);
// softmax cross-entropy, logits [R, V] fp32/bf16 with V % 8 == 0, targets in [0, V): per-row loss and
// log-sum-exp; backward dlogits = (softmax - onehot) * g[0] * inv_n in the logits' dtype
hipError_t cs_xent_fwd(int dt, const void* logits, const int64_t* tgt, float* loss, float* lse, int R, int V,
                       hipStream_t s);
hipError_t cs_xent_bwd(int dt, const void* logits, const int64_t* tgt, const float* lse, const float* g, float inv_n,
                       void* dlogits, int R, int V, hipStream_t s);
// the same with an ignore index and a z-loss: rows whose target == ignore are skipped (loss = lse = 0, a
// zero dlogits row, their logits never read), every other row's loss is (lse - x_t) + z * lse^2, and the
// mean runs over the non-ignored rows. The forward also writes stats (4 doubles, on the device, in a
// fixed order): {sum of the row losses, n_valid, inv = (float)(1.0 / max(n_valid, 1)), mean = sum * inv};
// the backward reads inv from there: dlogits = (softmax * (1 + 2 z lse) - onehot) * g[0] * inv.
hipError_t cs_xent_fwd_masked(int dt, const void* logits, const int64_t* tgt, float* loss, float* lse, double* stats,
                              int R, int V, int64_t ignore, float z, hipStream_t s);
hipError_t cs_xent_bwd_masked(int dt, const void* logits, const int64_t* tgt, const float* lse, const float* g,
                              const double* stats, void* dlogits, int R, int V, int64_t ignore, float z,
                              hipStream_t s);
// the chunked LM head: cs_xent_count writes stats[1] = n_valid and stats[2] = (float)(1.0 / max(n_valid, 1))
// over all R targets (the bits cs_xent_fwd_masked's reduction writes; stats[0] = stats[3] = 0);
// cs_xent_fused then turns a chunk of logits [rows, V] in place into its gradient
// (softmax * (1 + 2 z lse) - onehot) * stats[2] and writes loss / lse (full-length [R] arrays) at
// row0 .. row0 + rows - 1 with the arithmetic of cs_xent_fwd_masked, tgt being the full [R] array too;
// cs_xent_reduce, after the last chunk, fills all four stats from the full loss vector.
hipError_t cs_xent_count(const int64_t* tgt, int R, int64_t ignore, double* stats, hipStream_t s);
hipError_t cs_xent_fused(int dt, void* logits, const int64_t* tgt, float* loss, float* lse, const double* stats,
                         int rows, int V, int R, int row0, int64_t ignore, float z, hipStream_t s);
hipError_t cs_xent_reduce(const float* loss, const int64_t* tgt, int R, int64_t ignore, double* stats,
                          hipStream_t s);
hipError_t cs_swiglu_fwd(int dt, const void* a, const void* b, void* out, size_t n, hipStream_t s);
hipError_t cs_swiglu_bwd(int dt, const void* a, const void* b, const void* g, void* da, void* db, size_t n,
                         hipStream_t s);
// x/out: [B, S, H, hd] contiguous; cos/sin: [S, hd/2] fp32; inverse rotates by -angle (backward)
// causal / full grouped-query flash attention, bf16 [B, S, H, D] (attention.hip); lse: f32 [B, Hq, S]
// base-2 row log-sum-exp of the scaled scores; delta: f32 [B, Hq, S] scratch of the backward
hipError_t cs_attn_fwd(const void* q, const void* k, const void* v, void* o, float* lse, int B, int S, int Hq, int Hkv,
                       int D, float scale, int causal, hipStream_t stream);
hipError_t cs_attn_bwd(const void* q, const void* k, const void* v, const void* o, const void* dout, const float* lse,
                       float* delta, void* dq, void* dk, void* dv, int B, int S, int Hq, int Hkv, int D, float scale,
                       int causal, hipStream_t stream);
// the same, causal with a document mask (packed sequences): kstart / qend int32 [B, S], non-decreasing
// along S; query i sees key j iff kstart[b, i] <= j <= i, i.e. j <= i < qend[b, j]. Values are clamped
// in the kernels (kstart into [0, i], qend into [j + 1, S]): no contents can cause an access outside
// the tensors. The forward and the dQ pass read kstart, the dK/dV pass reads qend.
hipError_t cs_attn_fwd_doc(const void* q, const void* k, const void* v, void* o, float* lse, int B, int S, int Hq,
                           int Hkv, int D, float scale, const int* kstart, hipStream_t stream);
hipError_t cs_attn_bwd_doc(const void* q, const void* k, const void* v, const void* o, const void* dout,
                           const float* lse, float* delta, void* dq, void* dk, void* dv, int B, int S, int Hq, int Hkv,
                           int D, float scale, const int* kstart, const int* qend, hipStream_t stream);
// decode attention against a KV cache, split over the keys (attn_decode.hip). q / o: bf16 [B, Hq, D]; kc / vc:
// bf16 [B, Smax, Hkv, D] with row stride Hkv * D and batch stride `batch_stride` elements (% 8 == 0, so a
// [:, :n] slice of a longer cache is an operand); lens: int32 [B] on the device, clamped into [0, Smax] in
// the kernel (a row of length 0 gives zeros). D 64 or 128, Hq / Hkv in {1, 2, 4, 8}, all pointers 16-byte
// aligned, 1 <= nsplit <= cs_attn_decode_max_splits(Smax); ws: cs_attn_decode_ws_floats floats (may be null
// when nsplit == 1). hipErrorInvalidValue on anything else. Splits are combined in split order: no atomics.
int cs_attn_decode_key_tile();
int cs_attn_decode_max_splits(int Smax);            // the key tiles of Smax
int cs_attn_decode_splits(int B, int Hkv, int Smax);  // the default split count, from the shapes alone
size_t cs_attn_decode_ws_floats(int B, int Hq, int D, int nsplit);
hipError_t cs_attn_decode(const void* q, const void* kc, const void* vc, const int* lens, void* o, float* ws, int B,
                          int Smax, int Hq, int Hkv, int D, size_t batch_stride, int nsplit, float scale,
                          hipStream_t stream);
// the same against FP8 caches: kc / vc hold e4m3fn codes [B, Smax, Hkv, D] (batch stride in bytes, % 8 == 0),
// ks / vs fp32 scales [B, Smax, Hkv] with row stride Hkv and batch stride `scale_batch_stride` floats; the
// value of element i of a row is float(code[i]) * scale. Everything else as cs_attn_decode.
hipError_t cs_attn_decode_fp8(const void* q, const void* kc, const void* vc, const float* ks, const float* vs,
                              const int* lens, void* o, float* ws, int B, int Smax, int Hq, int Hkv, int D,
                              size_t batch_stride, size_t scale_batch_stride, int nsplit, float scale,
                              hipStream_t stream);
// quantising append to an FP8 KV cache (kv_append_fp8.hip): k / v bf16 [B, S, Hkv, D] contiguous and 16-byte
// aligned -> codes in kc / vc and one power-of-two fp32 scale per (token, kv head) in ks / vs (layouts as for
// cs_attn_decode_fp8), one launch for both tensors. Token (b, s) goes to position (pos ? pos[b] : 0) + s,
// clamped into [0, Smax - 1] in the kernel; of tokens the clamp folds onto one position the last is stored.
// pos: int32 [B] on the device or null. D 64 or 128. hipErrorInvalidValue on anything else.
hipError_t cs_kv_append_fp8(const void* k, const void* v, const int* pos, void* kc, void* vc, float* ks, float* vs,
                            int B, int S, int Smax, int Hkv, int D, size_t batch_stride, size_t scale_batch_stride,
                            hipStream_t stream);
// decode attention against a paged KV cache (attn_decode.hip, the same kernel template): kp / vp are the pools
// [P, page, Hkv, D] of one layer, bf16 (cs_attn_decode_paged) or e4m3fn codes with ks / vs fp32 [P, page, Hkv]
// (cs_attn_decode_paged_fp8); inner three (two) dimensions contiguous, page_stride elements (% 8 == 0) and
// scale_page_stride floats between pages. table: int32 [B, C] on the device, column stride 1, row stride
// table_stride: key n of sequence b is row n % page of page table[b, n / page]; an entry outside [0, pages)
// masks its keys (never loaded). page: a positive multiple of cs_attn_decode_key_tile(). Smax = C * page is the
// logical capacity: lens is clamped into [0, Smax], 1 <= nsplit <= cs_attn_decode_max_splits(Smax). For equal
// nsplit and lens the result has the bits of cs_attn_decode(_fp8) on the gathered cache. Everything else as
// cs_attn_decode; hipErrorInvalidValue on anything else.
hipError_t cs_attn_decode_paged(const void* q, const void* kp, const void* vp, const int* table, const int* lens,
                                void* o, float* ws, int B, int C, int Hq, int Hkv, int D, int pages, int page,
                                size_t page_stride, size_t table_stride, int nsplit, float scale, hipStream_t stream);
hipError_t cs_attn_decode_paged_fp8(const void* q, const void* kp, const void* vp, const float* ks, const float* vs,
                                    const int* table, const int* lens, void* o, float* ws, int B, int C, int Hq,
                                    int Hkv, int D, int pages, int page, size_t page_stride, size_t scale_page_stride,
                                    size_t table_stride, int nsplit, float scale, hipStream_t stream);
// append to a paged KV cache (kv_append_paged.hip): k / v bf16 [B, S, Hkv, D] contiguous and 16-byte aligned ->
// the pools of one layer (layouts as above), one launch for both tensors. ks == vs == null: bf16 pools, rows
// copied; otherwise FP8 pools, rows quantised as by cs_kv_append_fp8. Token (b, s) goes to logical position
// p = (pos ? pos[b] : 0) + s and is stored only if s < (counts ? counts[b] : S), 0 <= p < C * page and
// table[b, p / page] lies in [0, pages); otherwise it is dropped (never clamped). pos, counts: int32 [B] on
// the device or null. D 64 or 128. hipErrorInvalidValue on anything else.
hipError_t cs_kv_append_paged(const void* k, const void* v, const int* pos, const int* counts, const int* table,
                              void* kp, void* vp, float* ks, float* vs, int B, int S, int C, int Hkv, int D, int pages,
                              int page, size_t page_stride, size_t scale_page_stride, size_t table_stride,
                              hipStream_t stream);
// extend attention (attn_extend.hip): T new tokens per sequence against a cache that already holds their k and v.
// q / o: bf16 [B, T, Hq, D] contiguous, right-padded; start: int32 [B] on the device, row b's length before these
// tokens, clamped into [0, Smax] in the kernel; counts: int32 [B] or null (= T), the real new tokens of row b,
// clamped into [0, min(T, Smax - start)]. Query i < counts[b] sees keys 0 .. start[b] + i; rows i >= counts[b] of o
// are zeros; keys at or past start[b] + counts[b] are never loaded. kc / vc: bf16 [B, Smax, Hkv, D] as for
// cs_attn_decode (batch_stride % 8 == 0). D 64 or 128, any Hq % Hkv == 0, all pointers 16-byte aligned, one
// sequence's rows within 2 GiB. One flash-forward style kernel, no split over the keys: the same bits every run.
// hipErrorInvalidValue on anything else, without a launch.
hipError_t cs_attn_extend(const void* q, const void* kc, const void* vc, const int* start, const int* counts, void* o,
                          int B, int T, int Smax, int Hq, int Hkv, int D, size_t batch_stride, float scale,
                          hipStream_t stream);
// the same against bf16 pools [P, page, Hkv, D] through table int32 [B, C] (layouts as for cs_attn_decode_paged,
// Smax = C * page, page a positive multiple of 64): one table entry per 64-key tile, an entry outside [0, pages)
// masks its tile and is never turned into an address. For equal operands the result has the bits of cs_attn_extend
// on the gathered cache.
hipError_t cs_attn_extend_paged(const void* q, const void* kp, const void* vp, const int* table, const int* start,
                                const int* counts, void* o, int B, int T, int C, int Hq, int Hkv, int D, int pages,
                                int page, size_t page_stride, size_t table_stride, float scale, hipStream_t stream);
// training BatchNorm2d (+ residual add, + ReLU) on NCHW fp32 / bf16 activations (bn_nchw.hip).
// stat: f32 [4, C] = scale, shift, mean, invstd (written by the forward, read by the backward);
// part: f32 scratch of cs_bn_nchw_partials(N, C) floats; coef: f32 [3, C] scratch (backward).
// rm / rv (running stats, updated with `momentum`; nbt += 1), w / b, res, dres, dw, db, nbt may be null.
int cs_bn_nchw_partials(int N, int C);
hipError_t cs_bn_nchw_fwd(int dt, const void* x, const void* res, const float* w, const float* b, float* rm, float* rv,
                          int64_t* nbt, float momentum, float eps, int relu, void* y, float* stat, float* part, int N,
                          int C, int HW, hipStream_t stream);
hipError_t cs_bn_nchw_bwd(int dt, const void* dy, const void* x, const void* res, const float* w, const float* stat,
                          int relu, void* dx, void* dres, float* dw, float* db, float* coef, float* part, int N, int C,
                          int HW, hipStream_t stream);
// 3x3 / stride 2 / pad 1 max-pool on NCHW planes (pool_nchw.hip); pos: uint8 winning window
// position per output (0..8), consumed by the gather-style backward
hipError_t cs_maxpool3s2_fwd(int dt, const void* x, void* y, unsigned char* pos, int64_t planes, int H, int W, int Ho,
                             int Wo, hipStream_t stream);
hipError_t cs_maxpool3s2_bwd(int dt, const void* dy, const unsigned char* pos, void* dx, int64_t planes, int H, int W,
                             int Ho, int Wo, hipStream_t stream);
// bf16 GEMM on the matrix cores (gemm_bf16.hip): C[M, N] (=, +=) sum_k A(m, k) B(n, k), fp32
// accumulate. A is stored K-major ([M][K], row stride lda) or M-major ([K][M]); B K-major ([N][K])
// or N-major ([K][N]). out_mode 0: C bf16, 1: C fp32, 2: C fp32 +=, 3: C bf16 +=. Needs 16-byte aligned
// operands, lda / ldb % 8 == 0, K % 8 == 0 for a K-major operand, N, ldc % 4 == 0.
// splits > 1 (out_mode 1 only): split s of the reduction writes the fp32 slab C + s * slab
// (elements), to be summed by cs_slab_sum; cs_gemm_bf16_splits gives the default count.
// forward product with BatchNorm statistics of its bf16 output C[M, N] (A, B K-major, out bf16):
// stats[tile row t][N][2] = (mean, M2) of the bf16 values of rows [256 t, 256 t + 256)
hipError_t cs_gemm_bf16_bn_stats(const void* A, int64_t lda, const void* B, int64_t ldb, void* C, int64_t ldc, int M,
                                 int N, int K, float* stats, hipStream_t stream);
int cs_gemm_bf16_splits(int M, int N, int K);
hipError_t cs_gemm_bf16(int a_kmajor, const void* A, int64_t lda, int b_kmajor, const void* B, int64_t ldb, void* C,
                        int64_t ldc, int M, int N, int K, int out_mode, int splits, int64_t slab, hipStream_t stream);
// Fused sampler (sample.hip; contract in docs/sampling.md): one token per row of logits [B, V] (dt CS_F32, CS_BF16
// or CS_F16, unit inner stride, row_stride >= V elements) by temperature, top-k, min-p, top-p and an inverse-CDF
// draw at u [B] fp32 in [0, 1), one workgroup per row, no floating-point atomics. Each setting is a device array
// [B] (fp32; top_k int32), clamped on the device, or null with the scalar that follows it: temperature_s >= 0
// (0: argmax), top_k_s >= 1 or 0 for none, 0 < top_p_s <= 1, 0 <= min_p_s <= 1. finished: uint8 [B] or null; a
// row with finished[b] != 0 gets eos_id, any other row that draws eos_id sets it. tokens int64 [B]; kept int32
// [B]: the size of the set the token was drawn from. hipErrorInvalidValue on anything else.
hipError_t cs_sample_logits(int dt, const void* logits, int64_t row_stride, int B, int V, const float* u,
                            const float* temperature, float temperature_s, const int* top_k, int top_k_s,
                            const float* top_p, float top_p_s, const float* min_p, float min_p_s,
                            unsigned char* finished, int64_t eos_id, int64_t* tokens, int* kept, hipStream_t stream);
hipError_t cs_rope(int dt, const void* x, const float* cosv, const float* sinv, void* out, int B, int S, int H, int hd,
                   int inverse, hipStream_t s);
// QK-norm fused with RoPE: per head-row of q [B, S, Hq, hd] and k [B, S, Hkv, hd] (one dtype dt, hd 64 or
// 128), y = rope(x * rsqrt(mean(x^2) + eps) * w) with the fp32 gain wq / wk [hd] and the fp32 tables
// cos / sin [>= S, hd / 2], rounded once; one launch for both projections. hipErrorInvalidValue on another
// hd or dtype, on B * S * (Hq + Hkv) > INT_MAX, and on a null or not 16-byte aligned pointer.
hipError_t cs_qk_norm_rope_fwd(int dt, const void* q, const void* k, const float* wq, const float* wk,
                               const float* cosv, const float* sinv, void* yq, void* yk, int B, int S, int Hq, int Hkv,
                               int hd, float eps, hipStream_t s);
// its backward from the saved inputs (the row statistics are recomputed): dq, dk in dt and dw = [dwq | dwk]
// (2 * hd floats), summed in a fixed order from part, [cs_qk_norm_rope_partials(rows, hd)][2 * hd] floats of
// scratch with rows = B * S * (Hq + Hkv): two launches, no atomics
hipError_t cs_qk_norm_rope_bwd(int dt, const void* q, const void* k, const float* wq, const float* wk,
                               const float* cosv, const float* sinv, const void* gq, const void* gk, void* dq,
                               void* dk, float* dw, float* part, int B, int S, int Hq, int Hkv, int hd, float eps,
                               hipStream_t s);
// head-rows a block holds at a time (0: unsupported hd), the grid cap, and the blocks (= partial rows) of a launch
int cs_qk_norm_rope_rows_per_block(int hd);
int cs_qk_norm_rope_max_blocks();
int cs_qk_norm_rope_partials(int64_t rows, int hd);
// channels-last (NHWC) CNN kernels (cnn_nhwc.hip), fp32 / bf16 activations, M = B*H*W rows of C.
// BatchNorm: stat / coef / part exactly as the NCHW kernels above (part: cs_bn_nhwc_partials floats).
// mask (optional, M*C/V bytes, V = cs_bn_nhwc_vec): the forward writes each V-channel vector's
// pre-activation > 0 bits; the backward then takes the ReLU mask from it instead of recomputing it
// from x and the residual (one activation-sized read fewer per pass for a residual BatchNorm).
int cs_bn_nhwc_partials(int64_t M, int C, int dt);
int cs_bn_nhwc_vec(int C, int dt);
hipError_t cs_bn_nhwc_fwd(int dt, const void* x, const void* res, const float* w, const float* b, float* rm, float* rv,
                          int64_t* nbt, float momentum, float eps, int relu, void* y, float* stat, float* part,
                          int64_t M, int C, hipStream_t stream, unsigned char* mask = nullptr);
// the same from per-tile (mean, M2) partials of R-row tiles ([T][C][2], cs_gemm_bf16_bn_stats)
// instead of a statistics pass over x: finalize (Chan, f64, fixed order) + apply
hipError_t cs_bn_nhwc_fwd_tiles(int dt, const void* x, const void* res, const float* w, const float* b, float* rm,
                                float* rv, int64_t* nbt, float momentum, float eps, int relu, void* y, float* stat,
                                const float* tiles, int T, int R, int64_t M, int C, hipStream_t stream,
                                unsigned char* mask);
hipError_t cs_bn_nhwc_bwd(int dt, const void* dy, const void* x, const void* res, const float* w, const float* stat,
                          int relu, void* dx, void* dres, float* dw, float* db, float* coef, float* part, int64_t M,
                          int C, hipStream_t stream, const unsigned char* mask = nullptr,
                          const unsigned char* pool_pos = nullptr, int H = 0, int W = 0, int Ho = 0, int Wo = 0);
// (pool_pos: the BatchNorm's output was 3x3/2 max-pooled (cs_maxpool3s2_nhwc_fwd's window positions
// for the [B, Ho, Wo, C] output; x is [B, H, W, C]) and dy is the pooled gradient — the pool's
// backward gather is fused into both BatchNorm backward passes)
// stat (optional, a BatchNorm's [4][C] from cs_bn_nhwc_fwd with y == nullptr = statistics only):
// pool relu(BN(x)) — the BatchNorm apply fused into the pool's window loads
hipError_t cs_maxpool3s2_nhwc_fwd(int dt, const void* x, void* y, unsigned char* pos, int B, int H, int W, int C,
                                  int Ho, int Wo, hipStream_t stream, const float* stat = nullptr);
hipError_t cs_maxpool3s2_nhwc_bwd(int dt, const void* dy, const unsigned char* pos, void* dx, int B, int H, int W,
                                  int C, int Ho, int Wo, hipStream_t stream);
// bf16 NHWC implicit-GEMM convolution (conv_nhwc.hip; C, Co % 32 == 0, any R x S / stride / pad):
// FWD y[B,Ho,Wo,Co] = conv(x, w [Co][R][S][C]); DGRAD dx = y-shaped dy through wt [C][R][S][Co]
// (the weight transposed by the caller), written to y; WGRAD: split-K fp32 slabs in dw
// ([splits][Co][R*S*C], cs_conv_nhwc_splits) summed in split order into dw_out [Co][R*S*C] fp32.
struct CsConvNhwcArgs {
  const void* x;   // FWD / WGRAD: bf16 [B, H, W, C]
  const void* w;   // FWD: bf16 [Co][R][S][C]; DGRAD: bf16 [C][R][S][Co]
  const void* dy;  // DGRAD / WGRAD: bf16 [B, Ho, Wo, Co]
  void* y;         // FWD: y; DGRAD: dx (bf16 [B, H, W, C])
  float* dw;       // WGRAD: slab workspace
  float* dw_out;   // WGRAD: fp32 [Co][R*S*C]
  int B, H, W, C, Co, R, S, st, pad;
  // filled by the launcher
  int Ho, Wo, M, N, K, ksteps, ksteps_per_split;
};
// out[n] = deterministic sum of part[z][n] over z < splits (fp32; n % 4 == 0)
hipError_t cs_slab_sum(const float* part, int splits, int64_t n, float* out, hipStream_t stream);
int cs_conv_nhwc_splits(int mode, int B, int H, int W, int C, int Co, int R, int S, int st, int pad);
hipError_t cs_conv_nhwc(int mode, const CsConvNhwcArgs& a, int splits, hipStream_t stream);
// col: [B*Ho*Wo, Kp], columns (r*S + s)*C + c, zero for k >= R*S*C; col2im is its adjoint (gather)
hipError_t cs_im2col_nhwc(int dt, const void* x, void* col, int B, int H, int W, int C, int R, int S, int stride,
                          int pad, int Ho, int Wo, int Kp, hipStream_t stream);
hipError_t cs_col2im_nhwc(int dt, const void* dcol, void* dx, int B, int H, int W, int C, int R, int S, int stride,
                          int pad, int Ho, int Wo, int Kp, hipStream_t stream);
