// torch bindings of the decoder-LM kernels (csrc/kernels/lm.hip); shapes/dtypes validated on the host.
#include <algorithm>
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstdint>

#include "binding/torch_util.h"
#include "kernels/launchers.h"

namespace {

using csb::cur_stream;
using csb::DevGuard;

int dt_of(const torch::Tensor& t) {
  if (t.scalar_type() == at::kFloat) return CS_F32;
  if (t.scalar_type() == at::kBFloat16) return CS_BF16;
  TORCH_CHECK(false, "LM kernels support float32 / bfloat16, got ", t.scalar_type());
  return -1;
}

void check(const torch::Tensor& t, const char* n) {
  TORCH_CHECK(t.is_cuda() && t.is_contiguous(), n, " must be a contiguous GPU tensor");
}

// operands of the 16-byte (fp32 x4) / 8-byte (bf16 x4) vector accesses of the RMSNorm 4-wide and the
// cross-entropy kernels: a contiguous view at an odd storage offset passes check() but not this
// (ops/lm.py re-materialises such a view before the call)
void check_aligned(const torch::Tensor& t, const char* n) {
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, n, " must be 16-byte aligned");
}

// out_bf16: write y in bf16 whatever x's dtype (the fp32 residual stream feeding bf16 GEMMs)
std::vector<torch::Tensor> rmsnorm_fwd(torch::Tensor x, torch::Tensor w, double eps, bool out_bf16) {
  check(x, "x"); check(w, "w");
  const int64_t D = w.numel();
  TORCH_CHECK(x.size(-1) == D, "rmsnorm: last dim must match the weight");
  const bool vec4 = cs_rmsnorm_vec4((int)D);
  TORCH_CHECK(!out_bf16 || x.scalar_type() == at::kBFloat16 || vec4,
              "rmsnorm: bf16 output of fp32 input needs D % 4 == 0 and D <= 8192");
  const int64_t rows = x.numel() / D;
  DevGuard g(x.device());
  auto y = out_bf16 ? torch::empty_like(x, x.options().dtype(at::kBFloat16)) : torch::empty_like(x);
  auto rstd = torch::empty({rows}, x.options().dtype(at::kFloat));
  if (vec4) { check_aligned(x, "x"); check_aligned(w, "w"); check_aligned(y, "y"); }
  CS_LAUNCH(cs_rmsnorm_fwd(dt_of(x), dt_of(w), dt_of(y), x.data_ptr(), w.data_ptr(), y.data_ptr(),
                           rstd.data_ptr<float>(), (int)rows, (int)D, (float)eps, cur_stream()));
  return {y, rstd};
}

std::vector<torch::Tensor> rmsnorm_bwd(torch::Tensor x, torch::Tensor w, torch::Tensor rstd, torch::Tensor gy) {
  check(x, "x"); check(w, "w"); check(rstd, "rstd"); check(gy, "gy");
  const int64_t D = w.numel(), rows = x.numel() / D;
  TORCH_CHECK(gy.sizes() == x.sizes() && rstd.numel() == rows, "rmsnorm_bwd: shapes");
  const bool vec4 = cs_rmsnorm_vec4((int)D);
  TORCH_CHECK(gy.scalar_type() == x.scalar_type() || vec4, "rmsnorm_bwd: mixed dtypes need D % 4 == 0 and D <= 8192");
  DevGuard g(x.device());
  auto dx = torch::empty_like(x);
  auto dw = torch::empty_like(w);
  auto part = torch::empty({(int64_t)cs_rmsnorm_bwd_partials((int)rows, (int)D), D}, x.options().dtype(at::kFloat));
  if (vec4) {
    check_aligned(x, "x"); check_aligned(w, "w"); check_aligned(gy, "gy");
    check_aligned(dx, "dx"); check_aligned(dw, "dw"); check_aligned(part, "part");
  }
  CS_LAUNCH(cs_rmsnorm_bwd(dt_of(x), dt_of(w), dt_of(gy), x.data_ptr(), w.data_ptr(), rstd.data_ptr<float>(),
                           gy.data_ptr(), dx.data_ptr(), dw.data_ptr(), part.data_ptr<float>(), (int)rows, (int)D,
                           cur_stream()));
  return {dx, dw};
}

// h = x + delta in x's dtype, y = rms_norm(h, w) (bf16 when out_bf16), rstd of h -> {h, y, rstd}
std::vector<torch::Tensor> add_rmsnorm_fwd(torch::Tensor x, torch::Tensor delta, torch::Tensor w, double eps,
                                           bool out_bf16) {
  check(x, "x"); check(delta, "delta"); check(w, "w");
  const int64_t D = w.numel();
  TORCH_CHECK(D > 0 && D <= INT_MAX && x.dim() >= 1 && x.size(-1) == D, "add_rmsnorm: last dim must match the weight");
  TORCH_CHECK(delta.sizes() == x.sizes(), "add_rmsnorm: x and delta must have one shape");
  const int64_t rows = x.numel() / D;
  TORCH_CHECK(rows <= INT_MAX, "add_rmsnorm: too many rows");
  const bool vec4 = cs_rmsnorm_vec4((int)D);
  TORCH_CHECK(!out_bf16 || x.scalar_type() == at::kBFloat16 || vec4,
              "add_rmsnorm: bf16 output of fp32 input needs D % 4 == 0 and D <= 8192");
  TORCH_CHECK(delta.scalar_type() == x.scalar_type() || vec4,
              "add_rmsnorm: mixed dtypes need D % 4 == 0 and D <= 8192");
  DevGuard g(x.device());
  auto h = torch::empty_like(x);
  auto y = out_bf16 ? torch::empty_like(x, x.options().dtype(at::kBFloat16)) : torch::empty_like(x);
  auto rstd = torch::empty({rows}, x.options().dtype(at::kFloat));
  if (rows == 0) return {h, y, rstd};
  if (vec4) {
    check_aligned(x, "x"); check_aligned(delta, "delta"); check_aligned(w, "w");
    check_aligned(h, "h"); check_aligned(y, "y");
  }
  CS_LAUNCH(cs_add_rmsnorm_fwd(dt_of(x), dt_of(delta), dt_of(w), dt_of(y), x.data_ptr(), delta.data_ptr(),
                               w.data_ptr(), h.data_ptr(), y.data_ptr(), rstd.data_ptr<float>(), (int)rows, (int)D,
                               (float)eps, cur_stream()));
  return {h, y, rstd};
}

// d = gh + (the norm's input gradient of gy), gh absent = zero and not read -> {dx, ddelta, dw}: dx = d in h's
// dtype when need_dx, ddelta = d in delta_dtype when need_ddelta (one tensor serves both when the dtypes
// agree), an output nobody asked for is undefined (None) and not stored
std::vector<torch::Tensor> add_rmsnorm_bwd(torch::Tensor h, torch::Tensor w, torch::Tensor rstd, torch::Tensor gy,
                                           c10::optional<torch::Tensor> gh, at::ScalarType delta_dtype, bool need_dx,
                                           bool need_ddelta) {
  check(h, "h"); check(w, "w"); check(rstd, "rstd"); check(gy, "gy");
  const int64_t D = w.numel();
  TORCH_CHECK(D > 0 && D <= INT_MAX && h.dim() >= 1 && h.size(-1) == D, "add_rmsnorm_bwd: last dim must match the weight");
  const int64_t rows = h.numel() / D;
  TORCH_CHECK(rows <= INT_MAX && gy.sizes() == h.sizes() && rstd.numel() == rows &&
              rstd.scalar_type() == at::kFloat, "add_rmsnorm_bwd: shapes");
  TORCH_CHECK(delta_dtype == at::kFloat || delta_dtype == at::kBFloat16, "add_rmsnorm_bwd: delta dtype float32 / bfloat16");
  const bool has_gh = gh.has_value() && gh->defined();
  if (has_gh) {
    check(*gh, "gh");
    TORCH_CHECK(gh->sizes() == h.sizes() && gh->scalar_type() == h.scalar_type(), "add_rmsnorm_bwd: gh must match h");
  }
  const bool vec4 = cs_rmsnorm_vec4((int)D);
  TORCH_CHECK((gy.scalar_type() == h.scalar_type() && delta_dtype == h.scalar_type()) || vec4,
              "add_rmsnorm_bwd: mixed dtypes need D % 4 == 0 and D <= 8192");
  DevGuard g(h.device());
  const bool same = delta_dtype == h.scalar_type();
  torch::Tensor dx, dd;
  if (need_dx || (need_ddelta && same)) dx = torch::empty_like(h);
  if (need_ddelta && !same) dd = torch::empty_like(h, h.options().dtype(delta_dtype));
  // no rows: the weight gradient is the empty sum
  auto dw = rows == 0 ? torch::zeros_like(w) : torch::empty_like(w);
  if (rows > 0) {
    auto part = torch::empty({(int64_t)cs_rmsnorm_bwd_partials((int)rows, (int)D), D}, h.options().dtype(at::kFloat));
    if (vec4) {
      check_aligned(h, "h"); check_aligned(w, "w"); check_aligned(gy, "gy"); check_aligned(dw, "dw");
      check_aligned(part, "part");
      if (has_gh) check_aligned(*gh, "gh");
      if (dx.defined()) check_aligned(dx, "dx");
      if (dd.defined()) check_aligned(dd, "ddelta");
    }
    CS_LAUNCH(cs_add_rmsnorm_bwd(dt_of(h), dt_of(w), dt_of(gy), dd.defined() ? dt_of(dd) : dt_of(h), h.data_ptr(),
                                 w.data_ptr(), rstd.data_ptr<float>(), gy.data_ptr(), has_gh ? gh->data_ptr() : nullptr,
                                 dx.defined() ? dx.data_ptr() : nullptr, dd.defined() ? dd.data_ptr() : nullptr,
                                 dw.data_ptr(), part.data_ptr<float>(), (int)rows, (int)D, cur_stream()));
  }
  return {need_dx ? dx : torch::Tensor(), need_ddelta ? (same ? dx : dd) : torch::Tensor(), dw};
}

// logits [R, V], targets [R] int64 -> {loss_rows [R] f32, lse [R] f32}
std::vector<torch::Tensor> xent_fwd(torch::Tensor logits, torch::Tensor tgt) {
  check(logits, "logits");
  TORCH_CHECK(logits.dim() == 2 && logits.size(1) % 8 == 0, "xent: logits [R, V] with V % 8 == 0");
  TORCH_CHECK(tgt.is_cuda() && tgt.is_contiguous() && tgt.scalar_type() == at::kLong && tgt.numel() == logits.size(0),
              "xent: targets [R] int64");
  DevGuard g(logits.device());
  auto fo = logits.options().dtype(at::kFloat);
  auto loss = torch::empty({logits.size(0)}, fo), lse = torch::empty({logits.size(0)}, fo);
  check_aligned(logits, "logits");
  CS_LAUNCH(cs_xent_fwd(dt_of(logits), logits.data_ptr(), tgt.data_ptr<int64_t>(), loss.data_ptr<float>(),
                        lse.data_ptr<float>(), (int)logits.size(0), (int)logits.size(1), cur_stream()));
  return {loss, lse};
}

torch::Tensor xent_bwd(torch::Tensor logits, torch::Tensor tgt, torch::Tensor lse, torch::Tensor gscale, double inv_n) {
  check(logits, "logits");
  check(lse, "lse");
  TORCH_CHECK(logits.dim() == 2 && logits.size(1) % 8 == 0 && lse.numel() == logits.size(0), "xent_bwd: shapes");
  TORCH_CHECK(tgt.is_cuda() && tgt.scalar_type() == at::kLong && tgt.numel() == logits.size(0), "xent_bwd: targets");
  TORCH_CHECK(gscale.is_cuda() && gscale.scalar_type() == at::kFloat && gscale.numel() == 1, "xent_bwd: g");
  DevGuard g(logits.device());
  auto d = torch::empty_like(logits);
  check_aligned(logits, "logits"); check_aligned(d, "dlogits");
  CS_LAUNCH(cs_xent_bwd(dt_of(logits), logits.data_ptr(), tgt.data_ptr<int64_t>(), lse.data_ptr<float>(),
                        gscale.data_ptr<float>(), (float)inv_n, d.data_ptr(), (int)logits.size(0), (int)logits.size(1),
                        cur_stream()));
  return d;
}

// the host checks shared by the masked pair, all before any launch
void xent_masked_check(const torch::Tensor& logits, const torch::Tensor& tgt, double z_loss, const char* fn) {
  check(logits, "logits");
  TORCH_CHECK(logits.dim() == 2 && logits.size(1) > 0 && logits.size(1) % 8 == 0, fn,
              ": logits [R, V] with V % 8 == 0");
  TORCH_CHECK(logits.size(0) <= INT_MAX && logits.size(1) <= INT_MAX, fn, ": dimension too large");
  TORCH_CHECK(tgt.is_cuda() && tgt.device() == logits.device() && tgt.is_contiguous() &&
                  tgt.scalar_type() == at::kLong && tgt.numel() == logits.size(0),
              fn, ": targets [R] int64, contiguous, on the logits' device");
  TORCH_CHECK(std::isfinite(z_loss) && z_loss >= 0.0 && z_loss <= FLT_MAX, fn,
              ": z_loss must be a finite float >= 0, got ", z_loss);
  check_aligned(logits, "logits");
}

void xent_stats_check(const torch::Tensor& stats, const torch::Tensor& logits, const char* fn) {
  TORCH_CHECK(stats.is_cuda() && stats.device() == logits.device(), fn, ": stats must be on the logits' device");
  TORCH_CHECK(stats.scalar_type() == at::kDouble, fn, ": stats must be float64, got ", stats.scalar_type());
  TORCH_CHECK(stats.dim() == 1 && stats.numel() == 4 && stats.is_contiguous(), fn, ": stats must be a contiguous [4]");
}

// logits [R, V], targets [R] int64 -> {loss_rows [R] f32, lse [R] f32, stats [4] f64 = (sum, n_valid, inv, mean)}
std::vector<torch::Tensor> xent_fwd_masked(torch::Tensor logits, torch::Tensor tgt, int64_t ignore_index,
                                           double z_loss) {
  xent_masked_check(logits, tgt, z_loss, "xent_fwd_masked");
  DevGuard g(logits.device());
  auto fo = logits.options().dtype(at::kFloat);
  auto loss = torch::empty({logits.size(0)}, fo), lse = torch::empty({logits.size(0)}, fo);
  auto stats = torch::empty({4}, logits.options().dtype(at::kDouble));
  CS_LAUNCH(cs_xent_fwd_masked(dt_of(logits), logits.data_ptr(), tgt.data_ptr<int64_t>(), loss.data_ptr<float>(),
                               lse.data_ptr<float>(), stats.data_ptr<double>(), (int)logits.size(0),
                               (int)logits.size(1), ignore_index, (float)z_loss, cur_stream()));
  return {loss, lse, stats};
}

torch::Tensor xent_bwd_masked(torch::Tensor logits, torch::Tensor tgt, torch::Tensor lse, torch::Tensor stats,
                              torch::Tensor gscale, int64_t ignore_index, double z_loss) {
  xent_masked_check(logits, tgt, z_loss, "xent_bwd_masked");
  TORCH_CHECK(lse.is_cuda() && lse.device() == logits.device() && lse.is_contiguous() &&
                  lse.scalar_type() == at::kFloat && lse.numel() == logits.size(0),
              "xent_bwd_masked: lse [R] float32");
  xent_stats_check(stats, logits, "xent_bwd_masked");
  TORCH_CHECK(gscale.is_cuda() && gscale.device() == logits.device() && gscale.scalar_type() == at::kFloat &&
                  gscale.numel() == 1, "xent_bwd_masked: g must be one float32 element on the logits' device");
  DevGuard g(logits.device());
  auto d = torch::empty_like(logits);
  check_aligned(d, "dlogits");
  CS_LAUNCH(cs_xent_bwd_masked(dt_of(logits), logits.data_ptr(), tgt.data_ptr<int64_t>(), lse.data_ptr<float>(),
                               gscale.data_ptr<float>(), stats.data_ptr<double>(), d.data_ptr(), (int)logits.size(0),
                               (int)logits.size(1), ignore_index, (float)z_loss, cur_stream()));
  return d;
}

// ---- the chunked LM head (ops/lm.py linear_cross_entropy)
void xent_targets_check(const torch::Tensor& tgt, const char* fn) {
  TORCH_CHECK(tgt.is_cuda() && tgt.is_contiguous() && tgt.scalar_type() == at::kLong && tgt.dim() == 1 &&
                  tgt.numel() <= INT_MAX, fn, ": targets [R] int64, contiguous, on the GPU");
}

// targets [R] int64 -> stats [4] f64 = (0, n_valid, inv, 0), the count and reciprocal of xent_fwd_masked
torch::Tensor xent_count(torch::Tensor tgt, int64_t ignore_index) {
  xent_targets_check(tgt, "xent_count");
  DevGuard g(tgt.device());
  auto stats = torch::empty({4}, tgt.options().dtype(at::kDouble));
  CS_LAUNCH(cs_xent_count(tgt.data_ptr<int64_t>(), (int)tgt.numel(), ignore_index, stats.data_ptr<double>(),
                          cur_stream()));
  return stats;
}

// the final statistics over the full loss vector: stats = (sum, n_valid, inv, mean), in place
void xent_reduce(torch::Tensor loss, torch::Tensor tgt, int64_t ignore_index, torch::Tensor stats) {
  xent_targets_check(tgt, "xent_reduce");
  TORCH_CHECK(loss.is_cuda() && loss.device() == tgt.device() && loss.is_contiguous() &&
                  loss.scalar_type() == at::kFloat && loss.dim() == 1 && loss.numel() == tgt.numel(),
              "xent_reduce: loss [R] float32, contiguous, on the targets' device");
  xent_stats_check(stats, tgt, "xent_reduce");
  DevGuard g(tgt.device());
  CS_LAUNCH(cs_xent_reduce(loss.data_ptr<float>(), tgt.data_ptr<int64_t>(), (int)tgt.numel(), ignore_index,
                           stats.data_ptr<double>(), cur_stream()));
}

// logits_chunk [rows, V] is overwritten with its gradient; loss / lse [R] get rows row0 .. row0 + rows - 1
void xent_fused_(torch::Tensor logits, torch::Tensor tgt, torch::Tensor loss, torch::Tensor lse, torch::Tensor stats,
                 int64_t row0, int64_t ignore_index, double z_loss) {
  const char* fn = "xent_fused_";
  check(logits, "logits");
  TORCH_CHECK(logits.dim() == 2 && logits.size(1) > 0 && logits.size(1) % 8 == 0, fn,
              ": logits [rows, V] with V % 8 == 0");
  TORCH_CHECK(logits.size(0) <= INT_MAX && logits.size(1) <= INT_MAX, fn, ": dimension too large");
  xent_targets_check(tgt, fn);
  TORCH_CHECK(tgt.device() == logits.device(), fn, ": targets must be on the logits' device");
  const int64_t R = tgt.numel();
  for (auto* t : {&loss, &lse})
    TORCH_CHECK(t->is_cuda() && t->device() == logits.device() && t->is_contiguous() &&
                    t->scalar_type() == at::kFloat && t->dim() == 1 && t->numel() == R,
                fn, ": loss / lse [R] float32, contiguous, on the logits' device");
  xent_stats_check(stats, logits, fn);
  TORCH_CHECK(row0 >= 0 && row0 <= R && logits.size(0) <= R - row0, fn, ": rows row0 .. row0 + rows - 1 must lie in [0, R), got row0 ",
              row0, ", rows ", logits.size(0), ", R ", R);
  TORCH_CHECK(std::isfinite(z_loss) && z_loss >= 0.0 && z_loss <= FLT_MAX, fn,
              ": z_loss must be a finite float >= 0, got ", z_loss);
  check_aligned(logits, "logits");
  DevGuard g(logits.device());
  CS_LAUNCH(cs_xent_fused(dt_of(logits), logits.data_ptr(), tgt.data_ptr<int64_t>(), loss.data_ptr<float>(),
                          lse.data_ptr<float>(), stats.data_ptr<double>(), (int)logits.size(0), (int)logits.size(1),
                          (int)R, (int)row0, ignore_index, (float)z_loss, cur_stream()));
}

torch::Tensor swiglu_fwd(torch::Tensor a, torch::Tensor b) {
  check(a, "a"); check(b, "b");
  TORCH_CHECK(a.sizes() == b.sizes() && a.scalar_type() == b.scalar_type(), "swiglu: a/b mismatch");
  DevGuard g(a.device());
  auto out = torch::empty_like(a);
  CS_LAUNCH(cs_swiglu_fwd(dt_of(a), a.data_ptr(), b.data_ptr(), out.data_ptr(), a.numel(), cur_stream()));
  return out;
}

std::vector<torch::Tensor> swiglu_bwd(torch::Tensor a, torch::Tensor b, torch::Tensor gy) {
  check(a, "a"); check(b, "b"); check(gy, "gy");
  TORCH_CHECK(a.sizes() == b.sizes() && gy.sizes() == a.sizes() && gy.scalar_type() == a.scalar_type(),
              "swiglu_bwd: shapes");
  DevGuard g(a.device());
  auto da = torch::empty_like(a);
  auto db = torch::empty_like(b);
  CS_LAUNCH(cs_swiglu_bwd(dt_of(a), a.data_ptr(), b.data_ptr(), gy.data_ptr(), da.data_ptr(), db.data_ptr(),
                          a.numel(), cur_stream()));
  return {da, db};
}

torch::Tensor rope(torch::Tensor x, torch::Tensor cosv, torch::Tensor sinv, bool inverse) {
  check(x, "x"); check(cosv, "cos"); check(sinv, "sin");
  TORCH_CHECK(x.dim() == 4, "rope: x must be [B, S, H, head_dim]");
  const int64_t B = x.size(0), S = x.size(1), H = x.size(2), hd = x.size(3);
  TORCH_CHECK(hd % 2 == 0 && cosv.scalar_type() == at::kFloat && sinv.scalar_type() == at::kFloat &&
                  cosv.numel() == S * hd / 2 && sinv.numel() == S * hd / 2,
              "rope: cos/sin must be fp32 [S, head_dim/2]");
  DevGuard g(x.device());
  auto out = torch::empty_like(x);
  CS_LAUNCH(cs_rope(dt_of(x), x.data_ptr(), cosv.data_ptr<float>(), sinv.data_ptr<float>(), out.data_ptr(), (int)B,
                    (int)S, (int)H, (int)hd, inverse ? 1 : 0, cur_stream()));
  return out;
}

// the host checks shared by qk_norm_rope_fwd / _bwd
void qk_check(const torch::Tensor& q, const torch::Tensor& k, const torch::Tensor& wq, const torch::Tensor& wk,
              const torch::Tensor& cosv, const torch::Tensor& sinv) {
  check(q, "q"); check(k, "k"); check(wq, "wq"); check(wk, "wk"); check(cosv, "cos"); check(sinv, "sin");
  for (auto* t : {&k, &wq, &wk, &cosv, &sinv})
    TORCH_CHECK(t->device() == q.device(), "qk_norm_rope: all tensors must be on one device");
  TORCH_CHECK(q.dim() == 4 && k.dim() == 4, "qk_norm_rope: q and k must be [B, S, H, head_dim]");
  TORCH_CHECK(q.size(0) == k.size(0) && q.size(1) == k.size(1) && q.size(3) == k.size(3),
              "qk_norm_rope: q and k must agree in B, S and head_dim");
  TORCH_CHECK(q.scalar_type() == k.scalar_type(), "qk_norm_rope: q and k must have one dtype");
  TORCH_CHECK(q.scalar_type() == at::kFloat || q.scalar_type() == at::kBFloat16,
              "qk_norm_rope: q and k must be float32 or bfloat16");
  const int64_t S = q.size(1), hd = q.size(3);
  TORCH_CHECK(hd == 64 || hd == 128, "qk_norm_rope: head_dim must be 64 or 128, got ", hd);
  TORCH_CHECK(q.size(2) > 0 && k.size(2) > 0, "qk_norm_rope: q and k need at least one head");
  for (auto* w : {&wq, &wk})
    TORCH_CHECK(w->scalar_type() == at::kFloat && w->dim() == 1 && w->size(0) == hd,
                "qk_norm_rope: the gains must be fp32 [head_dim]");
  for (auto* t : {&cosv, &sinv})
    TORCH_CHECK(t->scalar_type() == at::kFloat && t->dim() == 2 && t->size(0) >= S && t->size(1) == hd / 2,
                "qk_norm_rope: cos / sin must be fp32 [>= S, head_dim / 2]");
  TORCH_CHECK(q.size(0) * S * (q.size(2) + k.size(2)) <= INT_MAX, "qk_norm_rope: too many head-rows");
  check_aligned(q, "q"); check_aligned(k, "k"); check_aligned(wq, "wq"); check_aligned(wk, "wk");
  check_aligned(cosv, "cos"); check_aligned(sinv, "sin");
}

// q [B, S, Hq, hd], k [B, S, Hkv, hd] -> {q', k'}: per-head RMSNorm with the gains wq / wk, then RoPE
std::vector<torch::Tensor> qk_norm_rope_fwd(torch::Tensor q, torch::Tensor k, torch::Tensor wq, torch::Tensor wk,
                                            torch::Tensor cosv, torch::Tensor sinv, double eps) {
  qk_check(q, k, wq, wk, cosv, sinv);
  DevGuard g(q.device());
  auto yq = torch::empty_like(q), yk = torch::empty_like(k);
  if (q.size(0) * q.size(1) == 0) return {yq, yk};  // no rows: no launch
  check_aligned(yq, "q'"); check_aligned(yk, "k'");
  CS_LAUNCH(cs_qk_norm_rope_fwd(dt_of(q), q.data_ptr(), k.data_ptr(), wq.data_ptr<float>(), wk.data_ptr<float>(),
                                cosv.data_ptr<float>(), sinv.data_ptr<float>(), yq.data_ptr(), yk.data_ptr(),
                                (int)q.size(0), (int)q.size(1), (int)q.size(2), (int)k.size(2), (int)q.size(3),
                                (float)eps, cur_stream()));
  return {yq, yk};
}

// the saved inputs and the gradients of q', k' -> {dq, dk, dwq, dwk}; dwq and dwk are the halves of one buffer
std::vector<torch::Tensor> qk_norm_rope_bwd(torch::Tensor q, torch::Tensor k, torch::Tensor wq, torch::Tensor wk,
                                            torch::Tensor cosv, torch::Tensor sinv, torch::Tensor gq, torch::Tensor gk,
                                            double eps) {
  qk_check(q, k, wq, wk, cosv, sinv);
  check(gq, "gq"); check(gk, "gk");
  TORCH_CHECK(gq.device() == q.device() && gk.device() == q.device(),
              "qk_norm_rope: all tensors must be on one device");
  TORCH_CHECK(gq.sizes() == q.sizes() && gq.scalar_type() == q.scalar_type() && gk.sizes() == k.sizes() &&
                  gk.scalar_type() == k.scalar_type(),
              "qk_norm_rope_bwd: the gradients must match q and k in shape and dtype");
  check_aligned(gq, "gq"); check_aligned(gk, "gk");
  DevGuard g(q.device());
  const int64_t hd = q.size(3), rows = q.size(0) * q.size(1) * (q.size(2) + k.size(2));
  auto dq = torch::empty_like(q), dk = torch::empty_like(k);
  if (rows == 0) {  // no rows: the weight gradients are the empty sum, no launch
    auto dw = torch::zeros({2 * hd}, wq.options());
    return {dq, dk, dw.slice(0, 0, hd), dw.slice(0, hd, 2 * hd)};
  }
  auto dw = torch::empty({2 * hd}, wq.options());
  auto part = torch::empty({(int64_t)cs_qk_norm_rope_partials(rows, (int)hd), 2 * hd}, wq.options());
  check_aligned(dq, "dq"); check_aligned(dk, "dk"); check_aligned(dw, "dw"); check_aligned(part, "part");
  CS_LAUNCH(cs_qk_norm_rope_bwd(dt_of(q), q.data_ptr(), k.data_ptr(), wq.data_ptr<float>(), wk.data_ptr<float>(),
                                cosv.data_ptr<float>(), sinv.data_ptr<float>(), gq.data_ptr(), gk.data_ptr(),
                                dq.data_ptr(), dk.data_ptr(), dw.data_ptr<float>(), part.data_ptr<float>(),
                                (int)q.size(0), (int)q.size(1), (int)q.size(2), (int)k.size(2), (int)hd, (float)eps,
                                cur_stream()));
  return {dq, dk, dw.slice(0, 0, hd), dw.slice(0, hd, 2 * hd)};
}

// q [B, S, Hq, D], k/v [B, S, Hkv, D] bf16 contiguous -> {o [B, S, Hq, D], lse f32 [B, Hq, S]}
void attn_check(const torch::Tensor& q, const torch::Tensor& k, const torch::Tensor& v) {
  for (auto* t : {&q, &k, &v}) {
    check(*t, "attention input");
    TORCH_CHECK(t->scalar_type() == at::kBFloat16 && t->dim() == 4, "attention: bf16 [B, S, H, D] tensors");
  }
  TORCH_CHECK(k.sizes() == v.sizes() && q.size(0) == k.size(0) && q.size(1) == k.size(1) && q.size(3) == k.size(3),
              "attention: q/k/v shapes");
  TORCH_CHECK(q.size(3) == 64 || q.size(3) == 128, "attention: head dim 64 or 128");
  TORCH_CHECK(q.size(2) % k.size(2) == 0, "attention: query heads must be a multiple of kv heads");
}

// the document mask of a packed batch (ops/attention.py doc_bounds): both arrays or neither
bool doc_check(const torch::Tensor& q, const c10::optional<torch::Tensor>& kstart,
               const c10::optional<torch::Tensor>& qend, bool causal) {
  TORCH_CHECK(kstart.has_value() == qend.has_value(), "attention: kstart and qend must be given together");
  if (!kstart.has_value()) return false;
  TORCH_CHECK(causal, "attention: a document mask is defined only together with causal=True");
  for (auto* t : {&*kstart, &*qend}) {
    TORCH_CHECK(t->scalar_type() == at::kInt, "attention: kstart / qend must be int32, got ", t->scalar_type());
    TORCH_CHECK(t->is_cuda() && t->device() == q.device(), "attention: kstart / qend must be on q's device");
    TORCH_CHECK(t->is_contiguous(), "attention: kstart / qend must be contiguous");
    TORCH_CHECK(t->dim() == 2 && t->size(0) == q.size(0) && t->size(1) == q.size(1),
                "attention: kstart / qend must be shaped [B, S] = [", q.size(0), ", ", q.size(1), "]");
  }
  return true;
}

std::vector<torch::Tensor> attn_fwd(torch::Tensor q, torch::Tensor k, torch::Tensor v, double scale, bool causal,
                                    c10::optional<torch::Tensor> kstart, c10::optional<torch::Tensor> qend) {
  attn_check(q, k, v);
  const bool doc = doc_check(q, kstart, qend, causal);
  DevGuard g(q.device());
  auto o = torch::empty_like(q);
  auto lse = torch::empty({q.size(0), q.size(2), q.size(1)}, q.options().dtype(at::kFloat));
  if (doc) {
    CS_LAUNCH(cs_attn_fwd_doc(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse.data_ptr<float>(), q.size(0),
                              q.size(1), q.size(2), k.size(2), q.size(3), (float)scale, kstart->data_ptr<int>(),
                              cur_stream()));
    return {o, lse};
  }
  CS_LAUNCH(cs_attn_fwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse.data_ptr<float>(), q.size(0),
                        q.size(1), q.size(2), k.size(2), q.size(3), (float)scale, causal ? 1 : 0, cur_stream()));
  return {o, lse};
}

std::vector<torch::Tensor> attn_bwd(torch::Tensor q, torch::Tensor k, torch::Tensor v, torch::Tensor o,
                                    torch::Tensor lse, torch::Tensor dout, double scale, bool causal,
                                    c10::optional<torch::Tensor> kstart, c10::optional<torch::Tensor> qend) {
  attn_check(q, k, v);
  check(o, "o"); check(dout, "dout"); check(lse, "lse");
  TORCH_CHECK(o.sizes() == q.sizes() && dout.sizes() == q.sizes() && o.scalar_type() == at::kBFloat16 &&
                  dout.scalar_type() == at::kBFloat16, "attn_bwd: o / dout must match q");
  TORCH_CHECK(lse.scalar_type() == at::kFloat && lse.numel() == q.size(0) * q.size(2) * q.size(1), "attn_bwd: lse");
  const bool doc = doc_check(q, kstart, qend, causal);
  DevGuard g(q.device());
  auto dq = torch::empty_like(q), dk = torch::empty_like(k), dv = torch::empty_like(v);
  auto delta = torch::empty_like(lse);
  if (doc) {
    CS_LAUNCH(cs_attn_bwd_doc(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), dout.data_ptr(),
                              lse.data_ptr<float>(), delta.data_ptr<float>(), dq.data_ptr(), dk.data_ptr(),
                              dv.data_ptr(), q.size(0), q.size(1), q.size(2), k.size(2), q.size(3), (float)scale,
                              kstart->data_ptr<int>(), qend->data_ptr<int>(), cur_stream()));
    return {dq, dk, dv};
  }
  CS_LAUNCH(cs_attn_bwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), dout.data_ptr(), lse.data_ptr<float>(),
                        delta.data_ptr<float>(), dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), q.size(0), q.size(1),
                        q.size(2), k.size(2), q.size(3), (float)scale, causal ? 1 : 0, cur_stream()));
  return {dq, dk, dv};
}

// The layout the KV-cache kernels take: kc / vc [B, Smax, Hkv, D] of one shape (checked by the caller), their inner
// three dimensions contiguous, one batch stride that holds Smax rows and is a multiple of 8; and, where there are
// scales (ks / vs not null), ks / vs [B, Smax, Hkv], their inner two dimensions contiguous, one batch stride that
// holds Smax rows. Returns the batch strides of the caches and of the scales (of contiguous ones for B <= 1,
// where torch's stride is free).
std::pair<int64_t, int64_t> check_kv_layout(const char* name, const torch::Tensor& kc, const torch::Tensor& vc,
                                            const torch::Tensor* ks, const torch::Tensor* vs) {
  const int64_t B = kc.size(0), Smax = kc.size(1), Hkv = kc.size(2), D = kc.size(3);
  for (auto* t : {&kc, &vc}) {
    TORCH_CHECK(t->stride(3) == 1 && t->stride(2) == D && t->stride(1) == Hkv * D, name,
                ": the inner three dimensions of the caches must be contiguous");
    TORCH_CHECK(B <= 1 || (t->stride(0) >= Smax * Hkv * D && t->stride(0) % 8 == 0), name,
                ": the batch stride of a cache must be a multiple of 8 and hold Smax rows");
  }
  TORCH_CHECK(B <= 1 || kc.stride(0) == vc.stride(0), name, ": the caches must have one batch stride");
  const int64_t bstride = B > 1 ? kc.stride(0) : Smax * Hkv * D;
  if (ks == nullptr) return {bstride, 0};
  for (auto* t : {ks, vs}) {
    TORCH_CHECK(t->dim() == 3 && t->size(0) == B && t->size(1) == Smax && t->size(2) == Hkv, name,
                ": the scales must be [B, Smax, Hkv]");
    TORCH_CHECK(t->stride(2) == 1 && t->stride(1) == Hkv, name,
                ": the inner two dimensions of the scales must be contiguous");
    TORCH_CHECK(B <= 1 || t->stride(0) >= Smax * Hkv, name, ": the batch stride of a scale must hold Smax rows");
  }
  TORCH_CHECK(B <= 1 || ks->stride(0) == vs->stride(0), name, ": the scales must have one batch stride");
  return {bstride, B > 1 ? ks->stride(0) : Smax * Hkv};
}

// decode attention (attn_decode.hip): q bf16 [B, Hq, D], caches bf16 [B, Smax, Hkv, D] whose inner three
// dimensions are contiguous (the batch stride is free: cache[:, :n] is an operand), lens int32 [B] -> o like q.
// splits: 0 = cs_attn_decode_splits(B, Hkv, Smax); anything else is clamped into [1, key tiles of Smax].
// With ks / vs (attn_decode_fp8) the caches are float8_e4m3fn and ks / vs fp32 [B, Smax, Hkv] their scales,
// contiguous in their inner two dimensions, with one batch stride.
torch::Tensor decode_impl(const char* name, torch::Tensor q, torch::Tensor kc, torch::Tensor vc, const torch::Tensor* ks,
                          const torch::Tensor* vs, torch::Tensor lens, double scale, int64_t splits) {
  const bool fp8 = ks != nullptr;
  for (auto* t : {&q, &kc, &vc, &lens}) TORCH_CHECK(t->is_cuda(), name, ": all tensors must be GPU tensors");
  for (auto* t : {&kc, &vc, &lens})
    TORCH_CHECK(t->device() == q.device(), name, ": all tensors must be on one device");
  if (fp8) {
    TORCH_CHECK(q.scalar_type() == at::kBFloat16, name, ": q must be bfloat16");
    TORCH_CHECK(kc.scalar_type() == at::kFloat8_e4m3fn && vc.scalar_type() == at::kFloat8_e4m3fn, name,
                ": the caches must be float8_e4m3fn");
  } else {
    TORCH_CHECK(q.scalar_type() == at::kBFloat16 && kc.scalar_type() == at::kBFloat16 &&
                    vc.scalar_type() == at::kBFloat16, name, ": q and the caches must be bfloat16");
  }
  TORCH_CHECK(q.dim() == 3, name, ": q must be [B, Hq, D]");
  TORCH_CHECK(kc.dim() == 4 && vc.dim() == 4 && kc.sizes() == vc.sizes(), name,
              ": the caches must be [B, Smax, Hkv, D] of one shape");
  const int64_t B = q.size(0), Hq = q.size(1), D = q.size(2), Smax = kc.size(1), Hkv = kc.size(2);
  TORCH_CHECK(kc.size(0) == B && kc.size(3) == D, name, ": q and the caches must agree in B and D");
  TORCH_CHECK(D == 64 || D == 128, name, ": head_dim must be 64 or 128, got ", D);
  TORCH_CHECK(Hkv > 0 && Hq % Hkv == 0 && (Hq / Hkv == 1 || Hq / Hkv == 2 || Hq / Hkv == 4 || Hq / Hkv == 8), name,
              ": query heads per kv head must be 1, 2, 4 or 8, got Hq ", Hq, ", Hkv ", Hkv);
  TORCH_CHECK(Smax >= 1, name, ": the caches need at least one position");
  TORCH_CHECK(lens.scalar_type() == at::kInt, name, ": lens must be int32, got ", lens.scalar_type());
  TORCH_CHECK(lens.dim() == 1 && lens.size(0) == B && lens.is_contiguous(), name, ": lens must be a contiguous [B]");
  TORCH_CHECK(q.is_contiguous(), name, ": q must be contiguous");
  if (fp8) {
    for (auto* t : {ks, vs})
      TORCH_CHECK(t->is_cuda() && t->device() == q.device() && t->scalar_type() == at::kFloat, name,
                  ": the scales must be fp32 tensors on q's device");
  }
  const auto [bstride, sstride] = check_kv_layout(name, kc, vc, ks, vs);
  TORCH_CHECK(B <= 65535 && Hkv <= 65535 && Smax <= INT_MAX, name, ": B, Hkv or Smax too large");
  check_aligned(q, "q"); check_aligned(kc, "k_cache"); check_aligned(vc, "v_cache");
  DevGuard g(q.device());
  auto o = torch::empty_like(q);
  if (B == 0) return o;
  const int64_t tiles = cs_attn_decode_max_splits((int)Smax);
  const int nsplit = splits == 0 ? cs_attn_decode_splits((int)B, (int)Hkv, (int)Smax)
                                 : (int)std::min<int64_t>(std::max<int64_t>(splits, 1), tiles);
  torch::Tensor ws;
  float* wsp = nullptr;
  if (nsplit > 1) {
    ws = torch::empty({(int64_t)cs_attn_decode_ws_floats((int)B, (int)Hq, (int)D, nsplit)},
                      q.options().dtype(at::kFloat));
    wsp = ws.data_ptr<float>();
  }
  check_aligned(o, "o");
  if (fp8) {
    CS_LAUNCH(cs_attn_decode_fp8(q.data_ptr(), kc.data_ptr(), vc.data_ptr(), ks->data_ptr<float>(),
                                 vs->data_ptr<float>(), lens.data_ptr<int>(), o.data_ptr(), wsp, (int)B, (int)Smax,
                                 (int)Hq, (int)Hkv, (int)D, (size_t)bstride, (size_t)sstride, nsplit, (float)scale,
                                 cur_stream()));
    return o;
  }
  CS_LAUNCH(cs_attn_decode(q.data_ptr(), kc.data_ptr(), vc.data_ptr(), lens.data_ptr<int>(), o.data_ptr(), wsp, (int)B,
                           (int)Smax, (int)Hq, (int)Hkv, (int)D, (size_t)bstride, nsplit, (float)scale, cur_stream()));
  return o;
}

torch::Tensor attn_decode(torch::Tensor q, torch::Tensor kc, torch::Tensor vc, torch::Tensor lens, double scale,
                          int64_t splits) {
  return decode_impl("attn_decode", q, kc, vc, nullptr, nullptr, lens, scale, splits);
}

torch::Tensor attn_decode_fp8(torch::Tensor q, torch::Tensor kc, torch::Tensor vc, torch::Tensor ks, torch::Tensor vs,
                              torch::Tensor lens, double scale, int64_t splits) {
  return decode_impl("attn_decode_fp8", q, kc, vc, &ks, &vs, lens, scale, splits);
}

// quantising append to an FP8 KV cache (kv_append_fp8.hip), in place: k / v bf16 [B, S, Hkv, D] contiguous ->
// codes in kc / vc float8_e4m3fn [B, Smax, Hkv, D] and scales in ks / vs fp32 [B, Smax, Hkv] at positions
// (pos ? pos[b] : 0) + s, clamped into [0, Smax - 1] in the kernel. pos: int32 [B] on the device.
void kv_append_fp8(torch::Tensor kc, torch::Tensor vc, torch::Tensor ks, torch::Tensor vs, torch::Tensor k,
                   torch::Tensor v, c10::optional<torch::Tensor> pos) {
  for (auto* t : {&kc, &vc, &ks, &vs, &k, &v}) {
    TORCH_CHECK(t->is_cuda(), "kv_append_fp8: all tensors must be GPU tensors");
    TORCH_CHECK(t->device() == k.device(), "kv_append_fp8: all tensors must be on one device");
  }
  TORCH_CHECK(k.scalar_type() == at::kBFloat16 && v.scalar_type() == at::kBFloat16,
              "kv_append_fp8: k and v must be bfloat16");
  TORCH_CHECK(kc.scalar_type() == at::kFloat8_e4m3fn && vc.scalar_type() == at::kFloat8_e4m3fn,
              "kv_append_fp8: the caches must be float8_e4m3fn");
  TORCH_CHECK(ks.scalar_type() == at::kFloat && vs.scalar_type() == at::kFloat, "kv_append_fp8: the scales must be fp32");
  TORCH_CHECK(k.dim() == 4 && k.sizes() == v.sizes() && k.is_contiguous() && v.is_contiguous(),
              "kv_append_fp8: k and v must be contiguous [B, S, Hkv, D] of one shape");
  const int64_t B = k.size(0), S = k.size(1), Hkv = k.size(2), D = k.size(3);
  TORCH_CHECK(D == 64 || D == 128, "kv_append_fp8: head_dim must be 64 or 128, got ", D);
  TORCH_CHECK(kc.dim() == 4 && kc.sizes() == vc.sizes() && kc.size(0) == B && kc.size(2) == Hkv && kc.size(3) == D,
              "kv_append_fp8: the caches must be [B, Smax, Hkv, D] of one shape, agreeing with k in B, Hkv and D");
  const int64_t Smax = kc.size(1);
  TORCH_CHECK(Smax >= 1 && Hkv >= 1, "kv_append_fp8: the caches need at least one position and one head");
  const auto [bstride, sstride] = check_kv_layout("kv_append_fp8", kc, vc, &ks, &vs);
  const int* posp = nullptr;
  if (pos.has_value()) {
    TORCH_CHECK(pos->is_cuda() && pos->device() == k.device() && pos->scalar_type() == at::kInt && pos->dim() == 1 &&
                    pos->size(0) == B && pos->is_contiguous(),
                "kv_append_fp8: pos must be a contiguous int32 [B] on k's device");
    posp = pos->data_ptr<int>();
  }
  TORCH_CHECK(B <= INT_MAX && S <= INT_MAX && Smax <= INT_MAX && Hkv <= INT_MAX, "kv_append_fp8: sizes too large");
  check_aligned(k, "k"); check_aligned(v, "v"); check_aligned(kc, "k_cache"); check_aligned(vc, "v_cache");
  if (B == 0 || S == 0) return;
  DevGuard g(k.device());
  CS_LAUNCH(cs_kv_append_fp8(k.data_ptr(), v.data_ptr(), posp, kc.data_ptr(), vc.data_ptr(), ks.data_ptr<float>(),
                             vs.data_ptr<float>(), (int)B, (int)S, (int)Smax, (int)Hkv, (int)D, (size_t)bstride,
                             (size_t)sstride, cur_stream()));
}

// The layout the paged KV-cache kernels take: pools kp / vp [P, page, Hkv, D] of one shape, their inner three
// dimensions contiguous, one page stride that holds a page and is a multiple of 8, page a positive multiple of the
// decode key tile; where there are scales, ks / vs fp32 [P, page, Hkv], their inner two dimensions contiguous, one
// page stride that holds a page; table int32 [B, C] on the pools' device with column stride 1 (table[:, :c] of a
// wider table is an operand).
struct PagedLayout {
  int64_t P, page, Hkv, D, C, page_stride, scale_stride, table_stride;
};

PagedLayout check_paged_layout(const char* name, const torch::Tensor& kp, const torch::Tensor& vp,
                               const torch::Tensor* ks, const torch::Tensor* vs, const torch::Tensor& table,
                               int64_t B) {
  TORCH_CHECK(kp.dim() == 4 && vp.dim() == 4 && kp.sizes() == vp.sizes(), name,
              ": the pools must be [P, page, Hkv, D] of one shape");
  const int64_t P = kp.size(0), page = kp.size(1), Hkv = kp.size(2), D = kp.size(3);
  TORCH_CHECK(P >= 1 && Hkv >= 1, name, ": the pools need at least one page and one head");
  const int64_t tile = cs_attn_decode_key_tile();
  TORCH_CHECK(page >= tile && page % tile == 0, name, ": the page size must be a positive multiple of ", tile,
              ", got ", page);
  for (auto* t : {&kp, &vp}) {
    TORCH_CHECK(t->stride(3) == 1 && t->stride(2) == D && t->stride(1) == Hkv * D, name,
                ": the inner three dimensions of the pools must be contiguous");
    TORCH_CHECK(P <= 1 || (t->stride(0) >= page * Hkv * D && t->stride(0) % 8 == 0), name,
                ": the page stride of a pool must be a multiple of 8 and hold a page");
  }
  TORCH_CHECK(P <= 1 || kp.stride(0) == vp.stride(0), name, ": the pools must have one page stride");
  TORCH_CHECK(table.is_cuda() && table.device() == kp.device(), name, ": block_table must be on the pools' device");
  TORCH_CHECK(table.scalar_type() == at::kInt, name, ": block_table must be int32, got ", table.scalar_type());
  TORCH_CHECK(table.dim() == 2 && table.size(0) == B && table.size(1) >= 1, name,
              ": block_table must be [B, C] with C >= 1");
  const int64_t C = table.size(1);
  TORCH_CHECK(C <= 1 || table.stride(1) == 1, name, ": the column stride of block_table must be 1");
  TORCH_CHECK(B <= 1 || table.stride(0) >= C, name, ": the row stride of block_table must hold C entries");
  TORCH_CHECK(P <= INT_MAX && Hkv <= INT_MAX && C * page <= INT_MAX, name, ": P, Hkv or C * page too large");
  PagedLayout L{P, page, Hkv, D, C, P > 1 ? kp.stride(0) : page * Hkv * D, 0, B > 1 ? table.stride(0) : C};
  if (ks == nullptr) return L;
  for (auto* t : {ks, vs}) {
    TORCH_CHECK(t->is_cuda() && t->device() == kp.device() && t->scalar_type() == at::kFloat, name,
                ": the scales must be fp32 tensors on the pools' device");
    TORCH_CHECK(t->dim() == 3 && t->size(0) == P && t->size(1) == page && t->size(2) == Hkv, name,
                ": the scales must be [P, page, Hkv]");
    TORCH_CHECK(t->stride(2) == 1 && t->stride(1) == Hkv, name,
                ": the inner two dimensions of the scales must be contiguous");
    TORCH_CHECK(P <= 1 || t->stride(0) >= page * Hkv, name, ": the page stride of a scale must hold a page");
  }
  TORCH_CHECK(P <= 1 || ks->stride(0) == vs->stride(0), name, ": the scales must have one page stride");
  L.scale_stride = P > 1 ? ks->stride(0) : page * Hkv;
  return L;
}

// decode attention against a paged KV cache (attn_decode.hip): q bf16 [B, Hq, D], pools [P, page, Hkv, D] bf16, or
// float8_e4m3fn with scales ks / vs fp32 [P, page, Hkv] (attn_decode_paged_fp8), block_table int32 [B, C], lens
// int32 [B] -> o like q. splits: 0 = cs_attn_decode_splits(B, Hkv, C * page); anything else is clamped into
// [1, key tiles of C * page].
torch::Tensor decode_paged_impl(const char* name, torch::Tensor q, torch::Tensor kp, torch::Tensor vp,
                                const torch::Tensor* ks, const torch::Tensor* vs, torch::Tensor table,
                                torch::Tensor lens, double scale, int64_t splits) {
  const bool fp8 = ks != nullptr;
  for (auto* t : {&q, &kp, &vp, &lens}) TORCH_CHECK(t->is_cuda(), name, ": all tensors must be GPU tensors");
  for (auto* t : {&kp, &vp, &lens})
    TORCH_CHECK(t->device() == q.device(), name, ": all tensors must be on one device");
  if (fp8) {
    TORCH_CHECK(q.scalar_type() == at::kBFloat16, name, ": q must be bfloat16");
    TORCH_CHECK(kp.scalar_type() == at::kFloat8_e4m3fn && vp.scalar_type() == at::kFloat8_e4m3fn, name,
                ": the pools must be float8_e4m3fn");
  } else {
    TORCH_CHECK(q.scalar_type() == at::kBFloat16 && kp.scalar_type() == at::kBFloat16 &&
                    vp.scalar_type() == at::kBFloat16, name, ": q and the pools must be bfloat16");
  }
  TORCH_CHECK(q.dim() == 3, name, ": q must be [B, Hq, D]");
  const int64_t B = q.size(0), Hq = q.size(1), D = q.size(2);
  const PagedLayout L = check_paged_layout(name, kp, vp, ks, vs, table, B);
  TORCH_CHECK(L.D == D, name, ": q and the pools must agree in D");
  TORCH_CHECK(D == 64 || D == 128, name, ": head_dim must be 64 or 128, got ", D);
  TORCH_CHECK(Hq % L.Hkv == 0 && (Hq / L.Hkv == 1 || Hq / L.Hkv == 2 || Hq / L.Hkv == 4 || Hq / L.Hkv == 8), name,
              ": query heads per kv head must be 1, 2, 4 or 8, got Hq ", Hq, ", Hkv ", L.Hkv);
  TORCH_CHECK(lens.scalar_type() == at::kInt, name, ": lens must be int32, got ", lens.scalar_type());
  TORCH_CHECK(lens.dim() == 1 && lens.size(0) == B && lens.is_contiguous(), name, ": lens must be a contiguous [B]");
  TORCH_CHECK(q.is_contiguous(), name, ": q must be contiguous");
  TORCH_CHECK(B <= 65535 && L.Hkv <= 65535, name, ": B or Hkv too large");
  check_aligned(q, "q"); check_aligned(kp, "k_pages"); check_aligned(vp, "v_pages");
  DevGuard g(q.device());
  auto o = torch::empty_like(q);
  if (B == 0) return o;
  const int Smax = (int)(L.C * L.page);
  const int64_t tiles = cs_attn_decode_max_splits(Smax);
  const int nsplit = splits == 0 ? cs_attn_decode_splits((int)B, (int)L.Hkv, Smax)
                                 : (int)std::min<int64_t>(std::max<int64_t>(splits, 1), tiles);
  torch::Tensor ws;
  float* wsp = nullptr;
  if (nsplit > 1) {
    ws = torch::empty({(int64_t)cs_attn_decode_ws_floats((int)B, (int)Hq, (int)D, nsplit)},
                      q.options().dtype(at::kFloat));
    wsp = ws.data_ptr<float>();
  }
  check_aligned(o, "o");
  if (fp8) {
    CS_LAUNCH(cs_attn_decode_paged_fp8(q.data_ptr(), kp.data_ptr(), vp.data_ptr(), ks->data_ptr<float>(),
                                       vs->data_ptr<float>(), table.data_ptr<int>(), lens.data_ptr<int>(), o.data_ptr(),
                                       wsp, (int)B, (int)L.C, (int)Hq, (int)L.Hkv, (int)D, (int)L.P, (int)L.page,
                                       (size_t)L.page_stride, (size_t)L.scale_stride, (size_t)L.table_stride, nsplit,
                                       (float)scale, cur_stream()));
    return o;
  }
  CS_LAUNCH(cs_attn_decode_paged(q.data_ptr(), kp.data_ptr(), vp.data_ptr(), table.data_ptr<int>(),
                                 lens.data_ptr<int>(), o.data_ptr(), wsp, (int)B, (int)L.C, (int)Hq, (int)L.Hkv, (int)D,
                                 (int)L.P, (int)L.page, (size_t)L.page_stride, (size_t)L.table_stride, nsplit,
                                 (float)scale, cur_stream()));
  return o;
}

torch::Tensor attn_decode_paged(torch::Tensor q, torch::Tensor kp, torch::Tensor vp, torch::Tensor table,
                                torch::Tensor lens, double scale, int64_t splits) {
  return decode_paged_impl("attn_decode_paged", q, kp, vp, nullptr, nullptr, table, lens, scale, splits);
}

torch::Tensor attn_decode_paged_fp8(torch::Tensor q, torch::Tensor kp, torch::Tensor vp, torch::Tensor ks,
                                    torch::Tensor vs, torch::Tensor table, torch::Tensor lens, double scale,
                                    int64_t splits) {
  return decode_paged_impl("attn_decode_paged_fp8", q, kp, vp, &ks, &vs, table, lens, scale, splits);
}

// append to a paged KV cache (kv_append_paged.hip), in place: k / v bf16 [B, S, Hkv, D] contiguous -> the pools
// [P, page, Hkv, D] through block_table int32 [B, C], at logical positions (pos ? pos[b] : 0) + s; a token with
// s >= counts[b], a position outside [0, C * page) or a table entry outside [0, P) is dropped. With ks / vs the
// pools are float8_e4m3fn and the rows are quantised (scales fp32 [P, page, Hkv]); without, the pools are bf16.
void kv_append_paged(torch::Tensor kp, torch::Tensor vp, torch::Tensor table, torch::Tensor k, torch::Tensor v,
                     c10::optional<torch::Tensor> pos, c10::optional<torch::Tensor> counts,
                     c10::optional<torch::Tensor> ks, c10::optional<torch::Tensor> vs) {
  const char* name = "kv_append_paged";
  TORCH_CHECK(ks.has_value() == vs.has_value(), name, ": k_scale and v_scale go together");
  const bool fp8 = ks.has_value();
  for (auto* t : {&kp, &vp, &k, &v}) {
    TORCH_CHECK(t->is_cuda(), name, ": all tensors must be GPU tensors");
    TORCH_CHECK(t->device() == k.device(), name, ": all tensors must be on one device");
  }
  TORCH_CHECK(k.scalar_type() == at::kBFloat16 && v.scalar_type() == at::kBFloat16, name, ": k and v must be bfloat16");
  if (fp8) {
    TORCH_CHECK(kp.scalar_type() == at::kFloat8_e4m3fn && vp.scalar_type() == at::kFloat8_e4m3fn, name,
                ": pools that come with scales must be float8_e4m3fn");
  } else {
    TORCH_CHECK(kp.scalar_type() == at::kBFloat16 && vp.scalar_type() == at::kBFloat16, name,
                ": pools without scales must be bfloat16");
  }
  TORCH_CHECK(k.dim() == 4 && k.sizes() == v.sizes() && k.is_contiguous() && v.is_contiguous(), name,
              ": k and v must be contiguous [B, S, Hkv, D] of one shape");
  const int64_t B = k.size(0), S = k.size(1), Hkv = k.size(2), D = k.size(3);
  TORCH_CHECK(D == 64 || D == 128, name, ": head_dim must be 64 or 128, got ", D);
  const PagedLayout L = check_paged_layout(name, kp, vp, fp8 ? &*ks : nullptr, fp8 ? &*vs : nullptr, table, B);
  TORCH_CHECK(L.Hkv == Hkv && L.D == D, name, ": the pools must agree with k in Hkv and D");
  const int* ptrs[2] = {nullptr, nullptr};
  int i = 0;
  for (auto* t : {&pos, &counts}) {
    if (t->has_value()) {
      const torch::Tensor& x = **t;
      TORCH_CHECK(x.is_cuda() && x.device() == k.device() && x.scalar_type() == at::kInt && x.dim() == 1 &&
                      x.size(0) == B && x.is_contiguous(),
                  name, i == 0 ? ": pos" : ": counts", " must be a contiguous int32 [B] on k's device");
      ptrs[i] = x.data_ptr<int>();
    }
    ++i;
  }
  TORCH_CHECK(B <= INT_MAX && S <= INT_MAX, name, ": sizes too large");
  check_aligned(k, "k"); check_aligned(v, "v"); check_aligned(kp, "k_pages"); check_aligned(vp, "v_pages");
  if (B == 0 || S == 0) return;
  DevGuard g(k.device());
  CS_LAUNCH(cs_kv_append_paged(k.data_ptr(), v.data_ptr(), ptrs[0], ptrs[1], table.data_ptr<int>(), kp.data_ptr(),
                               vp.data_ptr(), fp8 ? ks->data_ptr<float>() : nullptr,
                               fp8 ? vs->data_ptr<float>() : nullptr, (int)B, (int)S, (int)L.C, (int)Hkv, (int)D,
                               (int)L.P, (int)L.page, (size_t)L.page_stride, (size_t)L.scale_stride,
                               (size_t)L.table_stride, cur_stream()));
}

// start / counts of the extend kernels: a contiguous int32 [B] on q's device (counts may be absent)
const int* extend_index(const char* name, const char* what, const c10::optional<torch::Tensor>& t,
                        const torch::Tensor& q, int64_t B) {
  if (!t.has_value()) return nullptr;
  TORCH_CHECK(t->is_cuda() && t->device() == q.device() && t->scalar_type() == at::kInt && t->dim() == 1 &&
                  t->size(0) == B && t->is_contiguous(),
              name, ": ", what, " must be a contiguous int32 [B] on q's device");
  return t->data_ptr<int>();
}

// extend attention (attn_extend.hip): q bf16 [B, T, Hq, D] contiguous, the T new tokens of every row, against
// caches bf16 [B, Smax, Hkv, D] (layout as for attn_decode) that already hold their k and v; start int32 [B] the
// rows' lengths before these tokens, counts int32 [B] (absent: T) their real new tokens -> o like q.
torch::Tensor attn_extend(torch::Tensor q, torch::Tensor kc, torch::Tensor vc, torch::Tensor start, double scale,
                          c10::optional<torch::Tensor> counts) {
  const char* name = "attn_extend";
  for (auto* t : {&q, &kc, &vc}) {
    TORCH_CHECK(t->is_cuda(), name, ": all tensors must be GPU tensors");
    TORCH_CHECK(t->device() == q.device(), name, ": all tensors must be on one device");
    TORCH_CHECK(t->scalar_type() == at::kBFloat16, name, ": q and the caches must be bfloat16");
  }
  TORCH_CHECK(q.dim() == 4 && q.is_contiguous(), name, ": q must be a contiguous [B, T, Hq, D]");
  TORCH_CHECK(kc.dim() == 4 && vc.dim() == 4 && kc.sizes() == vc.sizes(), name,
              ": the caches must be [B, Smax, Hkv, D] of one shape");
  const int64_t B = q.size(0), T = q.size(1), Hq = q.size(2), D = q.size(3), Smax = kc.size(1), Hkv = kc.size(2);
  TORCH_CHECK(kc.size(0) == B && kc.size(3) == D, name, ": q and the caches must agree in B and D");
  TORCH_CHECK(D == 64 || D == 128, name, ": head_dim must be 64 or 128, got ", D);
  TORCH_CHECK(Hkv > 0 && Hq > 0 && Hq % Hkv == 0, name, ": Hq must be a multiple of Hkv, got Hq ", Hq, ", Hkv ", Hkv);
  TORCH_CHECK(Smax >= 1, name, ": the caches need at least one position");
  const int* startp = extend_index(name, "start", start, q, B);
  const int* countp = extend_index(name, "counts", counts, q, B);
  const auto [bstride, sstride] = check_kv_layout(name, kc, vc, nullptr, nullptr);
  (void)sstride;
  TORCH_CHECK(B <= 65535 && Hq <= 65535 && T <= INT_MAX && Smax <= INT_MAX, name, ": B, Hq, T or Smax too large");
  TORCH_CHECK((Smax - 1) * Hkv * D * 2 + 2 * D <= 0x7ffffff0, name, ": one sequence of the cache must lie within 2 GiB");
  check_aligned(q, "q"); check_aligned(kc, "k_cache"); check_aligned(vc, "v_cache");
  DevGuard g(q.device());
  auto o = torch::empty_like(q);
  if (B == 0 || T == 0) return o;
  check_aligned(o, "o");
  CS_LAUNCH(cs_attn_extend(q.data_ptr(), kc.data_ptr(), vc.data_ptr(), startp, countp, o.data_ptr(), (int)B, (int)T,
                           (int)Smax, (int)Hq, (int)Hkv, (int)D, (size_t)bstride, (float)scale, cur_stream()));
  return o;
}

// the same against bf16 pools [P, page, Hkv, D] through block_table int32 [B, C] (layout as for attn_decode_paged)
torch::Tensor attn_extend_paged(torch::Tensor q, torch::Tensor kp, torch::Tensor vp, torch::Tensor table,
                                torch::Tensor start, double scale, c10::optional<torch::Tensor> counts) {
  const char* name = "attn_extend_paged";
  for (auto* t : {&q, &kp, &vp}) {
    TORCH_CHECK(t->is_cuda(), name, ": all tensors must be GPU tensors");
    TORCH_CHECK(t->device() == q.device(), name, ": all tensors must be on one device");
    TORCH_CHECK(t->scalar_type() == at::kBFloat16, name, ": q and the pools must be bfloat16");
  }
  TORCH_CHECK(q.dim() == 4 && q.is_contiguous(), name, ": q must be a contiguous [B, T, Hq, D]");
  const int64_t B = q.size(0), T = q.size(1), Hq = q.size(2), D = q.size(3);
  const PagedLayout L = check_paged_layout(name, kp, vp, nullptr, nullptr, table, B);
  TORCH_CHECK(L.D == D, name, ": q and the pools must agree in D");
  TORCH_CHECK(D == 64 || D == 128, name, ": head_dim must be 64 or 128, got ", D);
  TORCH_CHECK(Hq > 0 && Hq % L.Hkv == 0, name, ": Hq must be a multiple of Hkv, got Hq ", Hq, ", Hkv ", L.Hkv);
  const int* startp = extend_index(name, "start", start, q, B);
  const int* countp = extend_index(name, "counts", counts, q, B);
  TORCH_CHECK(B <= 65535 && Hq <= 65535 && T <= INT_MAX, name, ": B, Hq or T too large");
  TORCH_CHECK((L.page - 1) * L.Hkv * D * 2 + 2 * D <= 0x7ffffff0, name, ": one page of the pools must lie within 2 GiB");
  check_aligned(q, "q"); check_aligned(kp, "k_pages"); check_aligned(vp, "v_pages");
  DevGuard g(q.device());
  auto o = torch::empty_like(q);
  if (B == 0 || T == 0) return o;
  check_aligned(o, "o");
  CS_LAUNCH(cs_attn_extend_paged(q.data_ptr(), kp.data_ptr(), vp.data_ptr(), table.data_ptr<int>(), startp, countp,
                                 o.data_ptr(), (int)B, (int)T, (int)L.C, (int)Hq, (int)L.Hkv, (int)D, (int)L.P,
                                 (int)L.page, (size_t)L.page_stride, (size_t)L.table_stride, (float)scale,
                                 cur_stream()));
  return o;
}

// fused sampler (sample.hip): logits [B, V] fp32 / bf16 / fp16 with unit inner stride, u fp32 [B] -> {tokens int64
// [B], kept int32 [B]}. Each setting is a scalar, or a tensor [B] (fp32; top_k int32) that overrides it and is
// clamped on the device, never read back; top_k 0: none. finished: uint8 [B], updated in place, with eos_id.
std::vector<torch::Tensor> sample_logits(torch::Tensor logits, torch::Tensor u, double temperature, int64_t top_k,
                                         double top_p, double min_p, c10::optional<torch::Tensor> temperature_t,
                                         c10::optional<torch::Tensor> top_k_t, c10::optional<torch::Tensor> top_p_t,
                                         c10::optional<torch::Tensor> min_p_t, c10::optional<int64_t> eos_id,
                                         c10::optional<torch::Tensor> finished) {
  const char* name = "sample_logits";
  TORCH_CHECK(logits.is_cuda() && logits.dim() == 2, name, ": logits must be a 2-D GPU tensor");
  int dt;
  if (logits.scalar_type() == at::kFloat) dt = CS_F32;
  else if (logits.scalar_type() == at::kBFloat16) dt = CS_BF16;
  else if (logits.scalar_type() == at::kHalf) dt = CS_F16;
  else TORCH_CHECK(false, name, ": logits must be float32, bfloat16 or float16, got ", logits.scalar_type());
  const int64_t B = logits.size(0), V = logits.size(1);
  TORCH_CHECK(V >= 1 && V < (1LL << 31) && B < (1LL << 31), name, ": need 1 <= V < 2^31 and B < 2^31");
  TORCH_CHECK(logits.stride(1) == 1 && (B <= 1 || logits.stride(0) >= V), name,
              ": logits rows must be contiguous (unit inner stride, row stride >= V)");
  auto per_row = [&](const torch::Tensor& t, at::ScalarType st, const char* what) {
    TORCH_CHECK(t.is_cuda() && t.device() == logits.device() && t.scalar_type() == st && t.dim() == 1 &&
                    t.size(0) == B && t.is_contiguous(),
                name, ": ", what, " must be a contiguous ", st, " [B] on the logits' device");
  };
  per_row(u, at::kFloat, "u");
  if (temperature_t) per_row(*temperature_t, at::kFloat, "a per-row temperature");
  if (top_k_t) per_row(*top_k_t, at::kInt, "a per-row top_k");
  if (top_p_t) per_row(*top_p_t, at::kFloat, "a per-row top_p");
  if (min_p_t) per_row(*min_p_t, at::kFloat, "a per-row min_p");
  TORCH_CHECK(finished.has_value() == eos_id.has_value(), name, ": eos_id and finished come together");
  if (finished) per_row(*finished, at::kByte, "finished");
  TORCH_CHECK(temperature >= 0.0 && std::isfinite(temperature), name, ": temperature must be finite and >= 0");
  TORCH_CHECK(top_k >= 0 && top_k <= INT_MAX, name, ": top_k must be >= 1 (0: none)");
  TORCH_CHECK(top_p > 0.0 && top_p <= 1.0, name, ": top_p must lie in (0, 1]");
  TORCH_CHECK(min_p >= 0.0 && min_p <= 1.0, name, ": min_p must lie in [0, 1]");
  // a positive double below the smallest float would round to 0, which means something else
  const float tf = temperature > 0.0 ? std::max((float)temperature, FLT_MIN) : 0.f;
  const float pf = std::max((float)top_p, FLT_MIN);
  DevGuard g(logits.device());
  auto tokens = torch::empty({B}, logits.options().dtype(at::kLong));
  auto kept = torch::empty({B}, logits.options().dtype(at::kInt));
  if (B == 0) return {tokens, kept};
  CS_LAUNCH(cs_sample_logits(dt, logits.data_ptr(), B > 1 ? logits.stride(0) : V, (int)B, (int)V, u.data_ptr<float>(),
                             temperature_t ? temperature_t->data_ptr<float>() : nullptr, tf,
                             top_k_t ? top_k_t->data_ptr<int>() : nullptr, (int)top_k,
                             top_p_t ? top_p_t->data_ptr<float>() : nullptr, pf,
                             min_p_t ? min_p_t->data_ptr<float>() : nullptr, (float)min_p,
                             finished ? finished->data_ptr<uint8_t>() : nullptr, eos_id ? *eos_id : -1,
                             tokens.data_ptr<int64_t>(), kept.data_ptr<int>(), cur_stream()));
  return {tokens, kept};
}

// C = a @ b on the bf16 matrix cores (gemm_bf16.hip). a: [M, K], b: [K, N], bf16, each with unit
// stride along one of its two dimensions (so x @ w.t(), dy @ w and dy.t() @ x all run without a
// copy); out: a new bf16 (out_f32 false) or fp32 [M, N] tensor, or `acc` [M, N] += a @ b (fp32, or
// bf16: summed in fp32 with one rounding).
// splits: reduction splits of an fp32 result (-1: cs_gemm_bf16_splits), summed in fixed order.
bool mode_bf16_acc(const c10::optional<torch::Tensor>& acc) {
  return acc.has_value() && acc->scalar_type() == at::kBFloat16;
}

torch::Tensor mm_bf16(torch::Tensor a, torch::Tensor b, bool out_f32, c10::optional<torch::Tensor> acc,
                      int64_t splits) {
  TORCH_CHECK(a.is_cuda() && b.is_cuda() && a.dim() == 2 && b.dim() == 2, "mm_bf16: 2-D GPU tensors");
  TORCH_CHECK(a.scalar_type() == at::kBFloat16 && b.scalar_type() == at::kBFloat16, "mm_bf16: bf16 operands");
  TORCH_CHECK(a.size(1) == b.size(0), "mm_bf16: inner dimensions differ");
  const int64_t M = a.size(0), K = a.size(1), N = b.size(1);
  TORCH_CHECK(M < (1LL << 31) && N < (1LL << 31) && K < (1LL << 31), "mm_bf16: dimension too large");
  int ak, bk;
  int64_t lda, ldb;
  if (a.stride(1) == 1) { ak = 1; lda = a.stride(0); }
  else if (a.stride(0) == 1) { ak = 0; lda = a.stride(1); }
  else TORCH_CHECK(false, "mm_bf16: a needs a unit stride");
  if (b.stride(0) == 1) { bk = 1; ldb = b.stride(1); }
  else if (b.stride(1) == 1) { bk = 0; ldb = b.stride(0); }
  else TORCH_CHECK(false, "mm_bf16: b needs a unit stride");
  DevGuard g(a.device());
  if (M == 0 || N == 0 || K == 0) {
    // empty reduction: torch.mm semantics (zeros; an accumulator is returned unchanged) without a
    // launch — the kernel would return hipSuccess and leave a fresh output uninitialised
    if (acc.has_value()) return *acc;
    return torch::zeros({M, N}, a.options().dtype(out_f32 ? at::kFloat : at::kBFloat16));
  }
  torch::Tensor c;
  int mode;
  // fp32 results of a reduction too long for the output's tile count are split over K into slabs
  int S = splits >= 0 ? (int)splits : cs_gemm_bf16_splits((int)M, (int)N, (int)K);
  if ((!out_f32 && !acc.has_value()) || mode_bf16_acc(acc)) S = 1;
  TORCH_CHECK(S >= 1 && S <= 256, "mm_bf16: splits out of range");
  if (acc.has_value()) {
    c = *acc;
    TORCH_CHECK(c.is_cuda() && (c.scalar_type() == at::kFloat || c.scalar_type() == at::kBFloat16) && c.dim() == 2 &&
                    c.size(0) == M && c.size(1) == N && c.stride(1) == 1,
                "mm_bf16: acc must be fp32 or bf16 [M, N] with unit column stride");
    mode = c.scalar_type() == at::kFloat ? 2 : 3;
  } else {
    c = torch::empty({M, N}, a.options().dtype(out_f32 ? at::kFloat : at::kBFloat16));
    mode = out_f32 ? 1 : 0;
  }
  if (S > 1) {
    auto part = torch::empty({S + (mode == 2 ? 1 : 0), M, N}, a.options().dtype(at::kFloat));
    CS_LAUNCH(cs_gemm_bf16(ak, a.data_ptr(), lda, bk, b.data_ptr(), ldb, part.data_ptr(), N, (int)M, (int)N, (int)K, 1,
                           S, M * N, cur_stream()));
    if (mode == 2) part[S].copy_(c);  // the accumulator joins the fixed-order sum as the last slab
    if (c.is_contiguous()) {
      CS_LAUNCH(cs_slab_sum(part.data_ptr<float>(), (int)part.size(0), M * N, c.data_ptr<float>(), cur_stream()));
    } else {
      auto sum = torch::empty({M, N}, part.options());
      CS_LAUNCH(cs_slab_sum(part.data_ptr<float>(), (int)part.size(0), M * N, sum.data_ptr<float>(), cur_stream()));
      c.copy_(sum);
    }
    return c;
  }
  CS_LAUNCH(cs_gemm_bf16(ak, a.data_ptr(), lda, bk, b.data_ptr(), ldb, c.data_ptr(), c.stride(0), (int)M, (int)N,
                         (int)K, mode, 1, 0, cur_stream()));
  return c;
}

// y = a @ b (bf16, a [M, K] K-major, b [K, N] with unit stride along K) plus the BatchNorm
// statistics of y per 256-row tile: {y, tiles [ceil(M / 256), N, 2] = (mean, M2)}
std::vector<torch::Tensor> mm_bf16_bn_stats(torch::Tensor a, torch::Tensor b) {
  TORCH_CHECK(a.is_cuda() && b.is_cuda() && a.dim() == 2 && b.dim() == 2 && a.scalar_type() == at::kBFloat16 &&
                  b.scalar_type() == at::kBFloat16, "mm_bf16_bn_stats: 2-D bf16 GPU tensors");
  TORCH_CHECK(a.size(1) == b.size(0) && a.stride(1) == 1 && b.stride(0) == 1,
              "mm_bf16_bn_stats: a [M, K] and b [K, N], both with unit stride along K");
  const int64_t M = a.size(0), K = a.size(1), N = b.size(1);
  TORCH_CHECK(M < (1LL << 31) && N < (1LL << 31) && K < (1LL << 31), "mm_bf16_bn_stats: dimension too large");
  DevGuard g(a.device());
  auto y = torch::empty({M, N}, a.options());
  auto tiles = torch::empty({(M + 255) / 256, N, 2}, a.options().dtype(at::kFloat));
  CS_LAUNCH(cs_gemm_bf16_bn_stats(a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(1), y.data_ptr(), N, (int)M,
                                  (int)N, (int)K, tiles.data_ptr<float>(), cur_stream()));
  return {y, tiles};
}

}  // namespace

void register_lm_ops(pybind11::module& m) {
  m.def("rmsnorm_vec4", [](int64_t D) { return D > 0 && D <= INT_MAX && cs_rmsnorm_vec4((int)D); },
        "whether RMSNorm of width D runs the 4-wide kernels (aligned operands; mixed dtypes allowed)");
  m.def("rmsnorm_fwd", &rmsnorm_fwd);
  m.def("rmsnorm_bwd", &rmsnorm_bwd);
  m.def("add_rmsnorm_fwd", &add_rmsnorm_fwd, "h = x + delta, y = rms_norm(h, w) in one pass -> (h, y, rstd)");
  m.def("add_rmsnorm_bwd", &add_rmsnorm_bwd,
        "(h, w, rstd, gy, gh or None, delta_dtype, need_dx, need_ddelta) -> (dx, ddelta, dw): gh + the norm's input "
        "gradient in h's dtype and in delta's, None where not asked for");
  m.def("xent_fwd", &xent_fwd, "softmax cross-entropy rows -> (loss, lse)");
  m.def("xent_bwd", &xent_bwd, "its backward -> dlogits");
  m.def("xent_fwd_masked", &xent_fwd_masked,
        "softmax cross-entropy rows with an ignore index and a z-loss -> (loss, lse, stats = [sum, n_valid, inv, "
        "mean])");
  m.def("xent_bwd_masked", &xent_bwd_masked, "its backward -> dlogits (scaled by g * stats[2], read on the device)");
  m.def("xent_count", &xent_count, "targets -> stats = [0, n_valid, inv, 0], ahead of the first chunk of the LM head");
  m.def("xent_fused_", &xent_fused_,
        "forward and backward of one chunk of logits in place (-> dlogits scaled by stats[2]); loss / lse rows "
        "row0 .. row0 + rows - 1 are written");
  m.def("xent_reduce", &xent_reduce, "stats = [sum, n_valid, inv, mean] of the full loss vector, in place");
  m.def("swiglu_fwd", &swiglu_fwd);
  m.def("swiglu_bwd", &swiglu_bwd);
  m.def("rope", &rope);
  namespace py = pybind11;
  m.def("qk_norm_rope_fwd", &qk_norm_rope_fwd,
        "per-head RMSNorm of q [B,S,Hq,hd] and k [B,S,Hkv,hd] (fp32 gains [hd]) fused with RoPE -> (q', k')",
        py::arg("q"), py::arg("k"), py::arg("wq"), py::arg("wk"), py::arg("cos"), py::arg("sin"),
        py::arg("eps") = 1e-5);
  m.def("qk_norm_rope_bwd", &qk_norm_rope_bwd, "its backward from the saved inputs -> (dq, dk, dwq, dwk)",
        py::arg("q"), py::arg("k"), py::arg("wq"), py::arg("wk"), py::arg("cos"), py::arg("sin"), py::arg("gq"),
        py::arg("gk"), py::arg("eps") = 1e-5);
  m.def("qk_norm_rope_rows_per_block", [](int64_t hd) { return cs_qk_norm_rope_rows_per_block((int)hd); },
        "head-rows a block of the QK-norm kernels holds at a time (0: unsupported head_dim)");
  m.def("qk_norm_rope_max_blocks", &cs_qk_norm_rope_max_blocks, "the grid cap of the QK-norm kernels");
  m.def("attn_fwd", &attn_fwd, "flash attention forward (bf16 [B,S,H,D], GQA, causal; kstart / qend: document mask)",
        py::arg("q"), py::arg("k"), py::arg("v"), py::arg("scale"), py::arg("causal"),
        py::arg("kstart") = c10::nullopt, py::arg("qend") = c10::nullopt);
  m.def("attn_bwd", &attn_bwd, "flash attention backward -> dq, dk, dv", py::arg("q"), py::arg("k"), py::arg("v"),
        py::arg("o"), py::arg("lse"), py::arg("dout"), py::arg("scale"), py::arg("causal"),
        py::arg("kstart") = c10::nullopt, py::arg("qend") = c10::nullopt);
  m.def("attn_decode", &attn_decode,
        "decode attention: q bf16 [B,Hq,D] against caches bf16 [B,Smax,Hkv,D] up to lens int32 [B] -> o [B,Hq,D]; "
        "splits 0: decode_splits(B, Hkv, Smax), otherwise clamped into [1, key tiles of Smax]",
        py::arg("q"), py::arg("k_cache"), py::arg("v_cache"), py::arg("lens"), py::arg("scale"), py::arg("splits") = 0);
  m.def("attn_decode_fp8", &attn_decode_fp8,
        "attn_decode against float8_e4m3fn caches with fp32 scales [B,Smax,Hkv] per (token, kv head)",
        py::arg("q"), py::arg("k_cache"), py::arg("v_cache"), py::arg("k_scale"), py::arg("v_scale"), py::arg("lens"),
        py::arg("scale"), py::arg("splits") = 0);
  m.def("kv_append_fp8", &kv_append_fp8,
        "quantise k, v bf16 [B,S,Hkv,D] into float8_e4m3fn caches and fp32 scales at pos[b] + s (clamped), in place",
        py::arg("k_cache"), py::arg("v_cache"), py::arg("k_scale"), py::arg("v_scale"), py::arg("k"), py::arg("v"),
        py::arg("pos") = c10::nullopt);
  m.def("attn_decode_paged", &attn_decode_paged,
        "decode attention through a block table: q bf16 [B,Hq,D], pools bf16 [P,page,Hkv,D], block_table int32 [B,C], "
        "lens int32 [B] -> o [B,Hq,D]; splits 0: decode_splits(B, Hkv, C * page), otherwise clamped",
        py::arg("q"), py::arg("k_pages"), py::arg("v_pages"), py::arg("block_table"), py::arg("lens"), py::arg("scale"),
        py::arg("splits") = 0);
  m.def("attn_decode_paged_fp8", &attn_decode_paged_fp8,
        "attn_decode_paged against float8_e4m3fn pools with fp32 scales [P,page,Hkv] per (row, kv head)",
        py::arg("q"), py::arg("k_pages"), py::arg("v_pages"), py::arg("k_scale"), py::arg("v_scale"),
        py::arg("block_table"), py::arg("lens"), py::arg("scale"), py::arg("splits") = 0);
  m.def("kv_append_paged", &kv_append_paged,
        "store k, v bf16 [B,S,Hkv,D] into paged pools at pos[b] + s through block_table (dropped where s >= counts[b], "
        "outside the table or on an invalid page), in place; with scales: float8_e4m3fn pools, quantised",
        py::arg("k_pages"), py::arg("v_pages"), py::arg("block_table"), py::arg("k"), py::arg("v"),
        py::arg("pos") = c10::nullopt, py::arg("counts") = c10::nullopt, py::arg("k_scale") = c10::nullopt,
        py::arg("v_scale") = c10::nullopt);
  m.def("attn_extend", &attn_extend,
        "extend attention: q bf16 [B,T,Hq,D], the T new tokens of every row, against caches bf16 [B,Smax,Hkv,D] that "
        "already hold their k and v; query i < counts[b] sees keys 0 .. start[b] + i, padded rows give zeros",
        py::arg("q"), py::arg("k_cache"), py::arg("v_cache"), py::arg("start"), py::arg("scale"),
        py::arg("counts") = c10::nullopt);
  m.def("attn_extend_paged", &attn_extend_paged,
        "attn_extend against bf16 pools [P,page,Hkv,D] through block_table int32 [B,C]; an entry outside [0,P) masks "
        "its keys", py::arg("q"), py::arg("k_pages"), py::arg("v_pages"), py::arg("block_table"), py::arg("start"),
        py::arg("scale"), py::arg("counts") = c10::nullopt);
  m.def("sample_logits", &sample_logits,
        "fused sampler: one token per row of logits [B,V] by temperature, top-k, min-p, top-p and an inverse-CDF draw at "
        "u fp32 [B] -> (tokens int64 [B], kept int32 [B]); a *_rows tensor [B] overrides its scalar; top_k 0: none",
        py::arg("logits"), py::arg("u"), py::arg("temperature") = 1.0, py::arg("top_k") = 0, py::arg("top_p") = 1.0,
        py::arg("min_p") = 0.0, py::arg("temperature_rows") = c10::nullopt, py::arg("top_k_rows") = c10::nullopt,
        py::arg("top_p_rows") = c10::nullopt, py::arg("min_p_rows") = c10::nullopt, py::arg("eos_id") = c10::nullopt,
        py::arg("finished") = c10::nullopt);
  m.def("decode_key_tile", &cs_attn_decode_key_tile, "keys a workgroup of the decode kernel reads per trip");
  m.def("decode_splits", [](int64_t B, int64_t Hkv, int64_t Smax) {
          TORCH_CHECK(B >= 0 && Hkv >= 0 && Smax >= 0 && B <= INT_MAX && Hkv <= INT_MAX && Smax <= INT_MAX,
                      "decode_splits: sizes out of range");
          return cs_attn_decode_splits((int)B, (int)Hkv, (int)Smax);
        }, "the key splits attn_decode picks for these shapes (never from lens)", py::arg("B"), py::arg("Hkv"),
        py::arg("Smax"));
  m.def("mm_bf16", &mm_bf16, "C = a @ b on the bf16 matrix cores", pybind11::arg("a"), pybind11::arg("b"),
        pybind11::arg("out_f32") = false, pybind11::arg("acc") = c10::nullopt, pybind11::arg("splits") = -1);
  m.def("mm_bf16_bn_stats", &mm_bf16_bn_stats, "a @ b (bf16) plus per-256-row-tile BatchNorm (mean, M2) of the result");
}
