"""Autograd wrappers of the decoder-LM gfx950 kernels (``csrc/kernels/lm.hip``).

On GPU tensors every op runs the hand-written HIP kernel (forward and backward);
on CPU tensors the plain-PyTorch reference below runs instead (this is the
numerics oracle of ``tests/test_lm_gpu.py`` and lets the LM train on CPU in the
multi-process gloo tests).
"""
from __future__ import annotations

import os

import torch

from . import native


# ------------------------------------------------------------------ references
def rms_norm_ref(x: torch.Tensor, w: torch.Tensor, eps: float) -> torch.Tensor:
    xf = x.float()
    y = xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps) * w.float()
    return y.to(x.dtype)


def add_rms_norm_ref(x: torch.Tensor, delta: torch.Tensor, w: torch.Tensor, eps: float):
    """(h, y): the residual sum ``h = x + delta`` and its RMSNorm"""
    h = x + delta
    return h, rms_norm_ref(h, w, eps)


def swiglu_ref(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    return (torch.nn.functional.silu(a.float()) * b.float()).to(a.dtype)


def rope_ref(x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor) -> torch.Tensor:
    """x: [B, S, H, hd], rotate interleaved pairs (2j, 2j+1) by angle table [S, hd/2]."""
    xf = x.float().view(*x.shape[:-1], -1, 2)
    c = cos[None, :, None, :]
    s = sin[None, :, None, :]
    x0, x1 = xf[..., 0], xf[..., 1]
    out = torch.stack([x0 * c - x1 * s, x0 * s + x1 * c], -1)
    return out.view(x.shape).to(x.dtype)


def qk_norm_rope_ref(q: torch.Tensor, k: torch.Tensor, wq: torch.Tensor, wk: torch.Tensor, cos: torch.Tensor,
                     sin: torch.Tensor, eps: float = 1e-5):
    """QK-norm fused with RoPE, in fp32: every head-row ``x`` of q [B, S, Hq, hd] and k [B, S, Hkv, hd] becomes
    ``rope(x * rsqrt(mean(x^2) + eps) * w)`` with ``w = wq`` for q and ``wk`` for k (one [hd] gain shared by the
    heads of a projection) and the pairing of ``rope_ref``; rounded to the input's dtype once. -> (q', k')"""
    S = q.shape[1]
    c, s = cos[:S].float()[None, :, None, :], sin[:S].float()[None, :, None, :]

    def one(x, w):
        xf = x.float()
        n = xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps) * w.float()
        n = n.view(*x.shape[:-1], -1, 2)
        n0, n1 = n[..., 0], n[..., 1]
        return torch.stack([n0 * c - n1 * s, n0 * s + n1 * c], -1).view(x.shape).to(x.dtype)

    return one(q, wq), one(k, wk)


# ------------------------------------------------------------------ autograd functions
def _aligned(t: torch.Tensor) -> torch.Tensor:
    """``t`` contiguous and 16-byte aligned, as the RMSNorm 4-wide and the cross-entropy kernels read
    it (8 / 16-byte vector accesses; the bindings refuse anything else): a contiguous view at an odd
    storage offset is copied into a fresh allocation, everything else is returned as it is."""
    t = t.contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone()


class _RMSNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, eps, out_bf16):
        xc = _aligned(x)
        y, rstd = native.C().rmsnorm_fwd(xc, _aligned(w), eps, out_bf16)
        ctx.save_for_backward(xc, w, rstd)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, w, rstd = ctx.saved_tensors
        if gy.dtype != x.dtype and not native.C().rmsnorm_vec4(x.shape[-1]):
            gy = gy.to(x.dtype)  # the scalar kernels read the gradient in x's dtype
        dx, dw = native.C().rmsnorm_bwd(x, _aligned(w), rstd, _aligned(gy))
        return dx, dw, None, None


class _AddRMSNorm(torch.autograd.Function):
    """(h, y) = (x + delta, rms_norm(x + delta)) in one pass; the backward adds the gradient of ``h``
    to the norm's ``dx`` in the pass that computes it, and writes the copy in ``delta``'s dtype (the
    bf16 branch under an fp32 stream) alongside."""

    @staticmethod
    def forward(ctx, x, delta, w, eps, out_bf16):
        ctx.set_materialize_grads(False)  # an unused output's gradient arrives as None, not as zeros
        ctx.delta_dtype = delta.dtype
        if delta.dtype != x.dtype and not native.C().rmsnorm_vec4(x.shape[-1]):
            delta = delta.to(x.dtype)  # the scalar kernels read every operand in the stream's dtype
        h, y, rstd = native.C().add_rmsnorm_fwd(_aligned(x), _aligned(delta), _aligned(w), eps, out_bf16)
        ctx.save_for_backward(h, w, rstd)
        return h, y

    @staticmethod
    def backward(ctx, gh, gy):
        h, w, rstd = ctx.saved_tensors
        need_dx, need_dd = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if gy is None:  # only h was used: the add alone
            if gh is None:
                return None, None, None, None, None
            return gh if need_dx else None, gh.to(ctx.delta_dtype) if need_dd else None, None, None, None
        vec4 = native.C().rmsnorm_vec4(h.shape[-1])
        if gy.dtype != h.dtype and not vec4:
            gy = gy.to(h.dtype)  # the scalar kernels read the gradient in the stream's dtype
        if gh is not None:
            gh = _aligned(gh.to(h.dtype))
        # same dtype: one stored gradient serves x and delta; the scalar kernels store the stream's only
        ddt = ctx.delta_dtype if vec4 else h.dtype
        dx, dd, dw = native.C().add_rmsnorm_bwd(h, _aligned(w), rstd, _aligned(gy), gh, ddt, need_dx, need_dd)
        if dd is not None and dd.dtype != ctx.delta_dtype:
            dd = dd.to(ctx.delta_dtype)
        return dx, dd, dw, None, None


class _SwiGLU(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        a, b = a.contiguous(), b.contiguous()
        ctx.save_for_backward(a, b)
        return native.C().swiglu_fwd(a, b)

    @staticmethod
    def backward(ctx, gy):
        a, b = ctx.saved_tensors
        da, db = native.C().swiglu_bwd(a, b, gy.contiguous().to(a.dtype))
        return da, db


class _RoPE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, cos, sin):
        cos, sin = cos.float().contiguous(), sin.float().contiguous()
        ctx.save_for_backward(cos, sin)
        return native.C().rope(x.contiguous(), cos, sin, False)

    @staticmethod
    def backward(ctx, gy):
        cos, sin = ctx.saved_tensors
        return native.C().rope(gy.contiguous(), cos, sin, True), None, None


class _QKNormRoPE(torch.autograd.Function):
    """(q', k') in one launch; the backward recomputes the row statistics from the saved q and k (one launch
    plus the fixed-order sum of the gain-gradient partials)."""

    @staticmethod
    def forward(ctx, q, k, wq, wk, cos, sin, eps):
        ctx.set_materialize_grads(False)  # an unused output's gradient arrives as None, not as zeros
        q, k, wq, wk = _aligned(q), _aligned(k), _aligned(wq), _aligned(wk)
        cos, sin = _aligned(cos.float()), _aligned(sin.float())
        yq, yk = native.C().qk_norm_rope_fwd(q, k, wq, wk, cos, sin, eps)
        ctx.save_for_backward(q, k, wq, wk, cos, sin)
        ctx.eps = eps
        return yq, yk

    @staticmethod
    def backward(ctx, gq, gk):
        if gq is None and gk is None:
            return (None,) * 7
        q, k, wq, wk, cos, sin = ctx.saved_tensors
        # the kernel reads both gradients in the inputs' dtype; a missing one is zeros of that output only
        gq = torch.zeros_like(q) if gq is None else _aligned(gq.to(q.dtype))
        gk = torch.zeros_like(k) if gk is None else _aligned(gk.to(k.dtype))
        grads = native.C().qk_norm_rope_bwd(q, k, wq, wk, cos, sin, gq, gk, ctx.eps)
        return tuple(g if need else None for g, need in zip(grads, ctx.needs_input_grad[:4])) + (None,) * 3


def _native_ok(*ts) -> bool:
    return all(t.is_cuda for t in ts) and all(t.dtype in (torch.float32, torch.bfloat16) for t in ts)


def rms_norm(x: torch.Tensor, w: torch.Tensor, eps: float = 1e-5) -> torch.Tensor:
    if _native_ok(x, w):
        # under bf16 autocast the fp32 residual stream is normalised straight into bf16: the
        # projections that follow read it without a cast pass each (5 per block), and their input
        # gradients come back in bf16 into the backward kernel, again without a cast
        out_bf16 = (torch.is_autocast_enabled("cuda") and torch.get_autocast_dtype("cuda") == torch.bfloat16
                    and native.C().rmsnorm_vec4(x.shape[-1]))  # the scalar kernels (D % 4, D > 8192) keep x's dtype
        return _RMSNorm.apply(x, w, eps, out_bf16)
    return rms_norm_ref(x, w, eps)


def add_rms_norm(x: torch.Tensor, delta: torch.Tensor, w: torch.Tensor, eps: float = 1e-5):
    """``(h, y)`` with ``h = x + delta`` (the residual stream after a branch) and ``y = rms_norm(h, w, eps)``
    (what the next branch reads), as one gfx950 pass forward and one backward: ``h`` is written once
    and not read back, and the backward adds the gradient of ``h`` to the norm's input gradient where
    it computes it, writing the bf16 copy for a bf16 branch in the same pass. ``h`` has ``x``'s dtype
    and the statistics are those of ``h`` as stored, so the result is ``rms_norm(x + delta)`` bit for bit;
    ``y`` follows ``rms_norm``'s dtype rule (bf16 under bf16 autocast on the 4-wide path).

    GPU fp32 / bf16 tensors, ``delta`` in ``x``'s dtype or bf16 on an fp32 stream, run the kernels;
    anything else (CPU, other dtypes, an fp32 ``delta`` on a bf16 stream, where torch's sum is fp32)
    runs ``add_rms_norm_ref``."""
    if (_native_ok(x, delta, w) and x.shape == delta.shape and w.numel() > 0
            and (delta.dtype == x.dtype or x.dtype == torch.float32)):
        out_bf16 = (torch.is_autocast_enabled("cuda") and torch.get_autocast_dtype("cuda") == torch.bfloat16
                    and native.C().rmsnorm_vec4(x.shape[-1]))  # the same rule as rms_norm
        return _AddRMSNorm.apply(x, delta, w, eps, out_bf16)
    return add_rms_norm_ref(x, delta, w, eps)


def swiglu(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    if _native_ok(a, b) and a.dtype == b.dtype:
        return _SwiGLU.apply(a, b)
    return swiglu_ref(a, b)


def rope(x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor) -> torch.Tensor:
    if _native_ok(x):
        return _RoPE.apply(x, cos, sin)
    return rope_ref(x, cos, sin)


def qk_norm_rope(q: torch.Tensor, k: torch.Tensor, wq: torch.Tensor, wk: torch.Tensor, cos: torch.Tensor,
                 sin: torch.Tensor, eps: float = 1e-5):
    """QK-norm fused with RoPE -> ``(q', k')``. ``q``: [B, S, Hq, hd], ``k``: [B, S, Hkv, hd]; every head-row
    ``x`` at position ``s`` becomes ``rope(x * rsqrt(mean(x^2) + eps) * w, s)`` with the learned gain
    ``w = wq`` ([hd], shared by the heads of q) or ``wk``, the tables ``cos`` / ``sin`` [>= S, hd/2] and the
    pairing of ``rope``: the per-head norm of Qwen3 / Gemma 3 (not a norm over the whole projection),
    computed in fp32 and rounded to the input's dtype once.

    When every tensor is on the GPU, q and k share fp32 or bf16, hd is 64 or 128 and the gains are fp32,
    one gfx950 launch does both projections forward and one (plus the fixed-order sum of the gain
    gradients' partials, no atomics: the same bits every run) backward. Anything else (CPU, another head
    size, bf16 gains, q and k of different dtypes) runs ``qk_norm_rope_ref``.

    Saved for backward: the pre-norm ``q`` and ``k`` (the row statistics are recomputed from them). Plain
    ``rope`` saves no activation, so QK-norm adds tokens x (Hq + Hkv) x hd saved elements per layer."""
    ts = (q, k, wq, wk, cos, sin)
    if (all(t.is_cuda for t in ts) and q.dim() == 4 and k.dim() == 4 and q.dtype == k.dtype
            and q.dtype in (torch.float32, torch.bfloat16) and q.shape[-1] in (64, 128)
            and q.shape[:2] == k.shape[:2] and q.shape[-1] == k.shape[-1] and q.shape[2] > 0 and k.shape[2] > 0
            and wq.dtype == torch.float32 and wk.dtype == torch.float32
            and wq.shape == q.shape[-1:] and wk.shape == q.shape[-1:]):
        return _QKNormRoPE.apply(q, k, wq, wk, cos, sin, float(eps))
    return qk_norm_rope_ref(q, k, wq, wk, cos, sin, eps)


# ------------------------------------------------------------------ bf16 projections with fp32 masters
# "native": the gfx950 matrix-core GEMM of csrc/kernels/gemm_bf16.hip runs all three products of a
# projection (y = x W^T, dx = dy W, dW = dy^T x, the last two reading the operands transposed in
# LDS, no copies); "wgrad": it runs the fp32 weight gradient dW only (where it measured faster
# than hipBLASLt at every Llama-3-8B shape, profiles/r4_gemm_bench_v2.jsonl); "blas": torch.mm
# (hipBLASLt) for all three. scripts/gemm_bench.py compares them per shape.
_GEMM = os.environ.get("CS_LM_GEMM", "wgrad")
if _GEMM not in ("native", "wgrad", "blas"):
    raise ValueError(f"CS_LM_GEMM must be 'native', 'wgrad' or 'blas', got {_GEMM!r}")


def gemm_operands_ok(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Whether ``native.C().mm_bf16(a, b)`` can run ``a @ b`` in place: the host-side preconditions
    of ``cs_gemm_bf16`` (csrc/kernels/gemm_bf16.hip), checked here so an operand the kernel cannot
    read (no unit stride — e.g. an expanded stride-0 gradient —, a leading dimension or an N that is
    not a multiple of 8 / 4 — an odd vocabulary —, a base pointer off 16 bytes) goes to torch.mm
    instead of raising inside backward."""
    if a.dim() != 2 or b.dim() != 2 or a.dtype != torch.bfloat16 or b.dtype != torch.bfloat16 or not a.is_cuda:
        return False
    M, K = a.shape
    N = b.shape[1]
    if M == 0 or N == 0 or K == 0:
        return True  # mm_bf16 returns zeros without a launch
    if a.stride(1) == 1:
        a_kmajor, lda = True, a.stride(0)
    elif a.stride(0) == 1:
        a_kmajor, lda = False, a.stride(1)
    else:
        return False
    if b.stride(0) == 1:
        b_kmajor, ldb = True, b.stride(1)
    elif b.stride(1) == 1:
        b_kmajor, ldb = False, b.stride(0)
    else:
        return False
    if lda % 8 or ldb % 8 or N % 4:
        return False
    if (a_kmajor or b_kmajor) and K % 8:
        return False
    if (lda < K if a_kmajor else lda < M) or (ldb < K if b_kmajor else ldb < N):
        return False
    # 32-bit buffer offsets: a K-major operand addresses 256 rows (kTile), an M-major one 64 k rows
    # (kBK) per tile; and the tile count fits an int (cs_gemm_bf16's own checks, mirrored)
    if (256 if a_kmajor else 64) * lda * 2 >= 0x7fffffff or (256 if b_kmajor else 64) * ldb * 2 >= 0x7fffffff:
        return False
    if ((M + 255) // 256) * ((N + 255) // 256) > 0x7fffffff:
        return False
    return (a.data_ptr() | b.data_ptr()) % 16 == 0


def _mm(a: torch.Tensor, b: torch.Tensor, out_f32: bool = False) -> torch.Tensor:
    """a @ b for bf16 2-D operands (views allowed), bf16 or fp32 out (fp32: the weight gradient)"""
    if (_GEMM == "native" or (_GEMM == "wgrad" and out_f32)) and gemm_operands_ok(a, b):
        return native.C().mm_bf16(a, b, out_f32)
    if out_f32:
        return torch.mm(a, b, out_dtype=torch.float32)
    return torch.mm(a, b)


class _LinearShadow(torch.autograd.Function):
    """y = x @ W^T on the bf16 shadow of the fp32 master W; dW straight out of the GEMM in fp32"""

    @staticmethod
    def forward(ctx, x, weight, shadow):
        x2 = x.reshape(-1, x.shape[-1])
        with torch.autocast("cuda", enabled=False):
            y = _mm(x2, shadow.t())
        ctx.save_for_backward(x2, shadow)
        ctx.xshape = x.shape
        return y.view(*x.shape[:-1], shadow.shape[0])

    @staticmethod
    def backward(ctx, gy):
        x2, shadow = ctx.saved_tensors
        g2 = gy.reshape(-1, gy.shape[-1])
        if g2.dtype != shadow.dtype:
            g2 = g2.to(shadow.dtype)
        dx = dw = None
        with torch.autocast("cuda", enabled=False):
            if ctx.needs_input_grad[0]:
                dx = _mm(g2, shadow).view(ctx.xshape)
            if ctx.needs_input_grad[1]:
                dw = _mm(g2.t(), x2, out_f32=True)
        return dx, dw, None


class ShadowLinear(torch.nn.Linear):
    """``nn.Linear`` (same parameters and state_dict) whose bf16-autocast forward reads a bf16 copy
    of the fp32 weight kept alongside it instead of casting the weight at every use. ``FusedSGD``
    rewrites the copy in its update pass (``sgd_multi`` shadow column; ``FusedAdamW`` does the same), so a training step spends no
    cast kernel on the weights at all, and the weight gradient leaves the GEMM in fp32 (no bf16
    round trip, no cast back). Any other in-place change of the weight (load_state_dict, a DDP
    broadcast, another optimizer) bumps its version and the copy is re-made on the next forward."""

    def _shadow(self) -> torch.Tensor:
        w = self.weight
        sh = getattr(w, "_cs_bf16_shadow", None)
        if sh is None or getattr(w, "_cs_bf16_shadow_version", -1) != w._version or sh.device != w.device \
                or sh.shape != w.shape:
            with torch.no_grad():
                sh = w.detach().to(torch.bfloat16)
            w._cs_bf16_shadow = sh
            w._cs_bf16_shadow_version = w._version
        return sh

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if (self.bias is None and x.is_cuda and self.weight.dtype == torch.float32 and torch.is_autocast_enabled("cuda")
                and torch.get_autocast_dtype("cuda") == torch.bfloat16):
            return _LinearShadow.apply(x.to(torch.bfloat16), self.weight, self._shadow())
        return super().forward(x)


# ------------------------------------------------------------------ LM loss
class _CrossEntropy(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, targets):
        logits = _aligned(logits)
        loss, lse = native.C().xent_fwd(logits, targets)
        ctx.save_for_backward(logits, targets, lse)
        return loss.sum() / logits.shape[0]

    @staticmethod
    def backward(ctx, g):
        logits, targets, lse = ctx.saved_tensors
        d = native.C().xent_bwd(logits, targets, lse, g.float().reshape(1).contiguous(), 1.0 / logits.shape[0])
        return d, None


# no ignore index: the kernels compare every target with a value no token id takes
_NO_IGNORE = -(1 << 63)


class _CrossEntropyMasked(torch.autograd.Function):
    """The masked / z-regularised kernels. The sum, the valid-row count, its reciprocal and the mean
    are formed on the device (``stats``); the backward reads the reciprocal there: no host read-back."""

    @staticmethod
    def forward(ctx, logits, targets, ignore, z):
        logits = _aligned(logits)
        _, lse, stats = native.C().xent_fwd_masked(logits, targets, ignore, z)
        ctx.save_for_backward(logits, targets, lse, stats)
        ctx.ignore, ctx.z = ignore, z
        return stats[3].float()

    @staticmethod
    def backward(ctx, g):
        logits, targets, lse, stats = ctx.saved_tensors
        d = native.C().xent_bwd_masked(logits, targets, lse, stats, g.float().reshape(1).contiguous(), ctx.ignore,
                                       ctx.z)
        return d, None, None, None


def _xent_native_ok(logits: torch.Tensor) -> bool:
    return (logits.is_cuda and logits.dim() == 2 and logits.shape[1] % 8 == 0
            and logits.dtype in (torch.float32, torch.bfloat16))


def _xent_rows_ref(logits, targets, ignore_index, z_loss):
    """fp32 per-row losses (0 for an ignored row, NaN for any other target outside [0, V)) and the
    mask of the rows that count. An ignored row's logits are replaced before any arithmetic, as the
    kernels never read them: a NaN there reaches neither the loss nor the gradient."""
    x = logits.float()
    V = x.shape[-1]
    valid = torch.ones_like(targets, dtype=torch.bool) if ignore_index is None else targets != ignore_index
    x = torch.where(valid[:, None], x, torch.zeros((), dtype=x.dtype, device=x.device))
    lse = torch.logsumexp(x, -1)
    inside = (targets >= 0) & (targets < V)
    xt = x.gather(1, targets.clamp(0, V - 1)[:, None])[:, 0]
    rows = lse - torch.where(inside, xt, torch.full_like(xt, float("nan")))
    if z_loss != 0.0:
        rows = rows + z_loss * lse * lse
    return torch.where(valid, rows, torch.zeros_like(rows)), valid


def cross_entropy_ref(logits: torch.Tensor, targets: torch.Tensor, ignore_index=None,
                      z_loss: float = 0.0) -> torch.Tensor:
    """Plain-torch ``cross_entropy`` with the semantics of the masked kernels, in fp32: the mean over
    the rows whose target is not ``ignore_index`` of ``(lse - x_t) + z_loss * lse^2``; 0 (and a zero
    gradient) when every row is ignored; NaN when a non-ignored target lies outside [0, V), with the
    gradient of the softmax term alone for that row."""
    rows, valid = _xent_rows_ref(logits, targets, ignore_index, z_loss)
    inv = (1.0 / valid.sum().clamp(min=1).double()).float()  # a double division rounded once, on the device
    return rows.sum() * inv


def cross_entropy(logits: torch.Tensor, targets: torch.Tensor, ignore_index=None,
                  z_loss: float = 0.0) -> torch.Tensor:
    """``F.cross_entropy(logits.float(), targets)`` (mean over rows) for [R, V] logits: on GPU one
    fused gfx950 pass forward and one backward over the logits in their own dtype (no fp32 upcast of
    the [tokens, vocab] matrix, no separate log-softmax / nll / cast kernels).

    ``ignore_index`` (default ``None``: no ignore index, not torch's -100): rows with that target,
    negative or inside the vocabulary (a pad id), are left out of the loss and get a zero gradient;
    the forward kernel does not read their logits. The mean runs over the remaining rows. Unlike
    ``F.cross_entropy``, a batch in which every row is ignored gives loss 0 and an all-zero gradient,
    not 0 / 0 = NaN: an all-padding micro-batch must not poison the weights.
    ``z_loss`` (>= 0) adds ``z_loss * lse^2`` per row, the auxiliary loss that keeps the softmax
    normaliser near 1 (PaLM, OLMo 2); its gradient is one multiply per element in the same backward pass.
    Every other target must lie in [0, V): one outside makes the loss NaN.

    With ``ignore_index=None`` and ``z_loss == 0`` the launches are those of the unmasked kernels,
    unchanged. Otherwise GPU fp32 / bf16 logits with V % 8 == 0 run the masked kernels, anything else
    (CPU, another V or dtype) ``cross_entropy_ref`` with the same semantics.

    Data-parallel runs: every rank's mean is over its own valid rows, and the gradient all-reduce then
    averages the ranks with equal weight (the usual convention, not a global valid-token mean)."""
    z_loss = float(z_loss)
    if ignore_index is None and z_loss == 0.0:
        if _xent_native_ok(logits):
            return _CrossEntropy.apply(logits.contiguous(), targets.contiguous())
        return torch.nn.functional.cross_entropy(logits.float(), targets)
    if not (z_loss >= 0.0 and z_loss != float("inf")):
        raise ValueError(f"z_loss must be finite and >= 0, got {z_loss}")
    if _xent_native_ok(logits) and targets.is_cuda and targets.dtype == torch.int64:
        ignore = _NO_IGNORE if ignore_index is None else int(ignore_index)
        return _CrossEntropyMasked.apply(logits.contiguous(), targets.contiguous(), ignore, z_loss)
    return cross_entropy_ref(logits, targets, ignore_index, z_loss)


@torch.no_grad()
def cross_entropy_sums(logits: torch.Tensor, targets: torch.Tensor, ignore_index=None):
    """Forward only, no z-loss: ``(nll_sum, n_valid)`` as 0-dim device tensors (float64, int64), the
    sum of ``lse - x_t`` over the rows whose target is not ``ignore_index`` and their number. On GPU
    these are the device statistics of the masked forward; nothing is read back. Token-weighted
    evaluation accumulates them over batches and divides once."""
    if _xent_native_ok(logits) and targets.is_cuda and targets.dtype == torch.int64:
        ignore = _NO_IGNORE if ignore_index is None else int(ignore_index)
        stats = native.C().xent_fwd_masked(_aligned(logits), targets.contiguous(), ignore, 0.0)[2]
        return stats[0], stats[1].long()
    rows, valid = _xent_rows_ref(logits, targets, ignore_index, 0.0)
    return rows.double().sum(), valid.sum()


# ------------------------------------------------------------------ chunked LM head: linear + loss
def head_chunk_rows(R: int, V: int, itemsize: int, chunk_rows=None) -> int:
    """Rows of one logits chunk of the fused head. An explicit ``chunk_rows`` is clamped to [1, R];
    otherwise the rows of a chunk of ``CS_LM_HEAD_CHUNK_MB`` MiB (default 1024) of logits, rounded down
    to a multiple of 256 (the GEMM's tile), at least 256 and at most R."""
    R = max(int(R), 1)
    if chunk_rows is not None:
        return min(max(int(chunk_rows), 1), R)
    mb = float(os.environ.get("CS_LM_HEAD_CHUNK_MB", "1024"))
    if not mb > 0:
        raise ValueError(f"CS_LM_HEAD_CHUNK_MB must be > 0, got {mb}")
    rows = int(mb * (1 << 20)) // (int(V) * int(itemsize))
    return min(max(rows // 256 * 256, 256), R)


def linear_cross_entropy_ref(h: torch.Tensor, head: torch.nn.Linear, targets: torch.Tensor, ignore_index=None,
                             z_loss: float = 0.0) -> torch.Tensor:
    """The unfused head: the full logits, then ``cross_entropy`` over them."""
    logits = head(h)
    return cross_entropy(logits.view(-1, logits.shape[-1]), targets.reshape(-1), ignore_index, z_loss)


def _head_mode(h: torch.Tensor, head, targets: torch.Tensor):
    """"bf16" / "fp32": how the chunked loop runs its GEMMs; None: the reference path"""
    w = getattr(head, "weight", None)
    if not isinstance(head, torch.nn.Linear) or head.bias is not None or not (h.is_cuda and w.is_cuda and
                                                                                targets.is_cuda):
        return None
    if w.dtype != torch.float32 or targets.dtype != torch.int64 or w.shape[0] % 8 or h.numel() == 0:
        return None
    if h.shape[-1] != w.shape[1] or targets.numel() != h.numel() // h.shape[-1]:
        return None
    if torch.is_autocast_enabled("cuda"):
        if (torch.get_autocast_dtype("cuda") == torch.bfloat16 and isinstance(head, ShadowLinear)
                and h.dtype in (torch.float32, torch.bfloat16)):
            return "bf16"
        return None
    return "fp32" if h.dtype == torch.float32 else None


def _mm_into(a: torch.Tensor, b: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """out = a @ b, ``out`` a contiguous row block of the result's dtype: the GEMM that ``_mm`` picks
    (CS_LM_GEMM=native: the GEMM makes its own output, which is copied into ``out``)"""
    if _GEMM == "native" and a.dtype == torch.bfloat16 and gemm_operands_ok(a, b):
        return out.copy_(native.C().mm_bf16(a, b))
    return torch.mm(a, b, out=out)


def _head_logits(hc, wmat, buf):
    """hc @ wmat^T for one chunk, in the one reused buffer (CS_LM_GEMM=native: the GEMM's own output,
    freed before the next chunk's is made, so that no copy of the chunk is needed)"""
    if _GEMM == "native" and wmat.dtype == torch.bfloat16 and gemm_operands_ok(hc, wmat.t()):
        return native.C().mm_bf16(hc, wmat.t())
    if buf[0] is None:
        buf[0] = torch.empty(buf[1], wmat.shape[0], dtype=hc.dtype, device=hc.device)
    return torch.mm(hc, wmat.t(), out=buf[0][:hc.shape[0]])


class _LinearCrossEntropy(torch.autograd.Function):
    """The head GEMM, the loss and both gradients over row chunks; only one chunk of logits exists at a
    time. ``xent_fused_`` turns the chunk into its gradient in place (scaled by 1 / n_valid, counted over
    all rows before the first chunk), the chunk then feeds dh_c = dlogits_c W and dW += dlogits_c^T h_c
    (fp32). The gradients are finished in forward; backward multiplies them by the upstream scalar."""

    @staticmethod
    def forward(ctx, h2, weight, shadow, targets, ignore, z, chunk):
        C = native.C()
        wmat = weight.detach() if shadow is None else shadow
        R, D = h2.shape
        V = wmat.shape[0]
        need_h, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        bf16 = wmat.dtype == torch.bfloat16
        with torch.autocast("cuda", enabled=False):
            loss = torch.empty(R, dtype=torch.float32, device=h2.device)
            if need_h or need_w:
                stats = C.xent_count(targets, ignore)  # 1 / n_valid over all rows, before the first chunk
                lse = torch.empty_like(loss)
            else:
                stats = torch.empty(4, dtype=torch.float64, device=h2.device)
            buf = [None, min(chunk, R)]
            dh = torch.empty_like(h2) if need_h else None
            dW = torch.zeros(V, D, dtype=torch.float32, device=h2.device) if need_w else None
            for r0 in range(0, R, chunk):
                hc = h2[r0:r0 + chunk]
                lc = _head_logits(hc, wmat, buf)
                if not (need_h or need_w):  # forward only: the loss rows of this chunk, nothing else
                    loss[r0:r0 + chunk] = C.xent_fwd_masked(lc, targets[r0:r0 + chunk], ignore, z)[0]
                    del lc
                    continue
                C.xent_fused_(lc, targets, loss, lse, stats, r0, ignore, z)
                if need_h:
                    _mm_into(lc, wmat, dh[r0:r0 + chunk])
                if need_w:
                    if not bf16:
                        dW.addmm_(lc.t(), hc)
                    elif _GEMM != "blas" and gemm_operands_ok(lc.t(), hc):
                        C.mm_bf16(lc.t(), hc, True, dW, 1)  # fp32 +=, no reduction split: K is one chunk
                    else:
                        dW += torch.mm(lc.t(), hc, out_dtype=torch.float32)
                del lc
            C.xent_reduce(loss, targets, ignore, stats)
        # plain attributes on purpose, not save_for_backward: they are neither inputs nor outputs, backward
        # scales them in place and hands them out, and a second backward (retain_graph) is refused below
        ctx.dh, ctx.dW = dh, dW
        return stats[3].float()

    @staticmethod
    def backward(ctx, g):
        dh, dW = ctx.dh, ctx.dW
        ctx.dh = ctx.dW = None  # scaled in place: a second backward through this node has nothing to return
        if dh is None and dW is None and any(ctx.needs_input_grad[:2]):
            raise RuntimeError("linear_cross_entropy: backward ran twice; its gradients are scaled in place")
        g = g.float()
        if dh is not None:
            dh.mul_(g)
        if dW is not None:
            dW.mul_(g)
        return dh, dW, None, None, None, None, None


def _head_args(h, head, targets, mode):
    h2 = h.reshape(-1, h.shape[-1])
    if mode == "bf16":
        h2 = h2.to(torch.bfloat16)
    return _aligned(h2), head._shadow() if mode == "bf16" else None, targets.reshape(-1).contiguous()


def linear_cross_entropy(h: torch.Tensor, head: torch.nn.Linear, targets: torch.Tensor, ignore_index=None,
                         z_loss: float = 0.0, chunk_rows=None) -> torch.Tensor:
    """``cross_entropy(head(h).view(-1, V), targets.view(-1), ignore_index, z_loss)`` without the
    [tokens, vocab] logits: the head GEMM, the fused loss kernel and the two gradient GEMMs run over
    chunks of ``head_chunk_rows`` rows, so one chunk of logits (and no saved copy, no separate
    gradient matrix) is alive at a time: in one reused buffer with the library GEMM (CS_LM_GEMM=wgrad,
    the default, or blas), in a fresh allocation per chunk with CS_LM_GEMM=native. ``h``: [..., D]; ``head``: a bias-free ``nn.Linear``;
    ``targets``: int64, one per row of ``h``. Returns the 0-dim fp32 loss; same masking, z-loss,
    all-rows-ignored -> 0 and out-of-range -> NaN rules as ``cross_entropy``, and the same per-rank
    mean under data parallelism.

    On the GPU, under bf16 autocast with a ``ShadowLinear`` the GEMMs read the bf16 shadow and the fp32
    weight gradient is accumulated by the native GEMM's ``+=`` mode; fp32 ``h`` without autocast runs the
    same loop on ``torch.mm``. The gradients of ``h`` and of the weight are complete when forward
    returns (backward only scales them by the upstream gradient, in place), which is what removes the
    saved logits; under ``no_grad`` only the loss is computed. Anything else (CPU, V % 8 != 0, a bias,
    other dtypes) runs ``linear_cross_entropy_ref``."""
    z_loss = float(z_loss)
    if not (z_loss >= 0.0 and z_loss != float("inf")):
        raise ValueError(f"z_loss must be finite and >= 0, got {z_loss}")
    mode = _head_mode(h, head, targets)
    if mode is None:
        return linear_cross_entropy_ref(h, head, targets, ignore_index, z_loss)
    h2, shadow, t = _head_args(h, head, targets, mode)
    chunk = head_chunk_rows(h2.shape[0], head.weight.shape[0], h2.element_size(), chunk_rows)
    ignore = _NO_IGNORE if ignore_index is None else int(ignore_index)
    return _LinearCrossEntropy.apply(h2, head.weight, shadow, t, ignore, z_loss, chunk)


@torch.no_grad()
def linear_cross_entropy_sums(h: torch.Tensor, head: torch.nn.Linear, targets: torch.Tensor, ignore_index=None,
                              chunk_rows=None):
    """``cross_entropy_sums(head(h).view(-1, V), targets.view(-1), ignore_index)``, forward only and
    chunked like ``linear_cross_entropy``: ``(nll_sum, n_valid)`` as 0-dim device tensors."""
    mode = _head_mode(h, head, targets)
    if mode is None:
        logits = head(h)
        return cross_entropy_sums(logits.view(-1, logits.shape[-1]), targets.reshape(-1), ignore_index)
    C = native.C()
    h2, shadow, t = _head_args(h, head, targets, mode)
    wmat = head.weight.detach() if shadow is None else shadow
    R, V = h2.shape[0], wmat.shape[0]
    chunk = head_chunk_rows(R, V, h2.element_size(), chunk_rows)
    ignore = _NO_IGNORE if ignore_index is None else int(ignore_index)
    with torch.autocast("cuda", enabled=False):
        loss = torch.empty(R, dtype=torch.float32, device=h2.device)
        buf = [None, min(chunk, R)]
        for r0 in range(0, R, chunk):
            lc = _head_logits(h2[r0:r0 + chunk], wmat, buf)
            loss[r0:r0 + chunk] = C.xent_fwd_masked(lc, t[r0:r0 + chunk], ignore, 0.0)[0]
            del lc
        stats = torch.empty(4, dtype=torch.float64, device=h2.device)
        C.xent_reduce(loss, t, ignore, stats)
    return stats[0], stats[1].long()


def mask_boundary_targets(inputs: torch.Tensor, targets: torch.Tensor, eos_id: int,
                          ignore_index: int = -100) -> torch.Tensor:
    """The targets of a packed batch with every position whose *input* is ``eos_id`` set to
    ``ignore_index`` (one device op, nothing read back). Convention of ``ops.attention.doc_ids_from_eos``:
    an EOS closes its own document, so the target at an EOS input is the first token of the next
    document, which document-masked attention has made unpredictable."""
    return targets.masked_fill(inputs == eos_id, ignore_index)


# ------------------------------------------------------------------ sampling
def _sample_scalars(temperature, top_k, top_p, min_p):
    """Range checks of the scalar settings (tensors are clamped where they are used, never read back)."""
    if not isinstance(temperature, torch.Tensor) and not (0.0 <= float(temperature) < float("inf")):
        raise ValueError(f"sample_logits: temperature must be finite and >= 0, got {temperature}")
    if top_k is not None and not isinstance(top_k, torch.Tensor) and int(top_k) < 1:
        raise ValueError(f"sample_logits: top_k must be >= 1 or None, got {top_k}")
    if top_p is not None and not isinstance(top_p, torch.Tensor) and not (0.0 < float(top_p) <= 1.0):
        raise ValueError(f"sample_logits: top_p must lie in (0, 1], got {top_p}")
    if min_p is not None and not isinstance(min_p, torch.Tensor) and not (0.0 <= float(min_p) <= 1.0):
        raise ValueError(f"sample_logits: min_p must lie in [0, 1], got {min_p}")


def _sample_rows(x, B, dev, dtype, default):
    """A setting as a tensor [B]: a scalar (None: ``default``) repeated, or the caller's tensor converted."""
    if isinstance(x, torch.Tensor):
        if x.shape != (B,):
            raise ValueError(f"sample_logits: a per-row setting must have shape [{B}], got {tuple(x.shape)}")
        return x.to(device=dev, dtype=dtype)
    return torch.full((B,), default if x is None else x, dtype=dtype, device=dev)


def sample_logits_ref(logits: torch.Tensor, u: torch.Tensor, temperature=1.0, top_k=None, top_p=None, min_p=None,
                      eos_id=None, finished=None, return_kept: bool = False):
    """The contract of ``sample_logits`` in plain torch (the division by the temperature in fp32, weights and
    sums in float64, a sort where the kernel descends by radix). Runs on any device."""
    _sample_scalars(temperature, top_k, top_p, min_p)
    if logits.dim() != 2 or logits.shape[1] < 1:
        raise ValueError("sample_logits: logits must be [B, V] with V >= 1")
    B, V = logits.shape
    dev = logits.device
    if u.shape != (B,):
        raise ValueError(f"sample_logits: u must have shape [{B}]")
    if (eos_id is None) != (finished is None):
        raise ValueError("sample_logits: eos_id and finished come together")
    tokens = torch.empty(B, dtype=torch.int64, device=dev)
    kept = torch.empty(B, dtype=torch.int32, device=dev)
    if B == 0:
        return (tokens, kept) if return_kept else tokens
    T = torch.nan_to_num(_sample_rows(temperature, B, dev, torch.float32, 1.0), nan=0.0).clamp(min=0)
    k = _sample_rows(top_k, B, dev, torch.int64, V).clamp(min=1)
    p = torch.nan_to_num(_sample_rows(top_p, B, dev, torch.float32, 1.0), nan=0.0).clamp(0, 1)
    mp = torch.nan_to_num(_sample_rows(min_p, B, dev, torch.float32, 0.0), nan=0.0).clamp(0, 1)
    ninf = torch.full((), float("-inf"), dtype=torch.float32, device=dev)
    z = logits.float()
    has_nan = torch.isnan(z).any(-1)
    greedy = T == 0
    s = torch.where(torch.isnan(z), ninf, z) / torch.where(greedy, torch.ones_like(T), T)[:, None]  # fp32
    s = torch.where(torch.isnan(s), ninf, s) + 0.0
    smax = s.max(-1).values
    first_max = (s == smax[:, None]).int().argmax(-1)  # the lowest index of the maximum
    plain = greedy | has_nan | ~torch.isfinite(smax)  # rows that get the arg max
    w = torch.exp(s.double() - torch.where(plain, torch.zeros_like(smax), smax).double()[:, None])
    keep = s > ninf
    # top-k: everything >= the k-th largest value
    sorted_s, order = s.sort(dim=-1, descending=True, stable=True)
    kth = sorted_s.gather(1, (k.clamp(max=V) - 1)[:, None])
    keep = keep & ((k >= V)[:, None] | (s >= kth))
    # min-p
    keep = keep & (w >= mp.double()[:, None])
    # top-p: the largest kept value whose upper set holds top_p of the kept mass, ties kept
    wk = torch.where(keep, w, torch.zeros_like(w))
    cum = wk.gather(1, order).cumsum(-1)
    reach = cum >= (p.double() * wk.sum(-1))[:, None]
    cut = sorted_s.gather(1, reach.int().argmax(-1)[:, None])
    keep = keep & (~(reach.any(-1) & (p < 1))[:, None] | (s >= cut))
    # the draw, in vocabulary order
    wk = torch.where(keep, w, torch.zeros_like(w))
    cdf = wk.cumsum(-1)
    hit = keep & (cdf >= (u.to(dev).double() * cdf[:, -1])[:, None])
    last = V - 1 - keep.flip(-1).int().argmax(-1)
    tok = torch.where(hit.any(-1), hit.int().argmax(-1), last)
    tokens = torch.where(plain, first_max, tok)
    kept = torch.where(plain, torch.ones_like(tok), keep.sum(-1)).int()
    if finished is not None:
        done = finished != 0
        tokens = torch.where(done, torch.full_like(tokens, eos_id), tokens)
        kept = torch.where(done, torch.zeros_like(kept), kept)
        finished.copy_((done | (tokens == eos_id)).to(finished.dtype))
    return (tokens, kept) if return_kept else tokens


def sample_logits(logits: torch.Tensor, u: torch.Tensor, temperature=1.0, top_k=None, top_p=None, min_p=None,
                  eos_id=None, finished=None, return_kept: bool = False):
    """One token per row of ``logits`` [B, V]: temperature, top-k, min-p, top-p and the draw, on the GPU in one
    launch (``csrc/kernels/sample.hip``) that holds no random state: ``u`` [B], fp32 in [0, 1), is the caller's.
    Returns ``tokens`` int64 [B], with ``return_kept`` also ``kept`` int32 [B], the size of the set a row drew from.

    With ``s = float(logits) / temperature`` in fp32 and ``smax`` a row's maximum (a ``-inf`` logit is never kept):
    ``top_k`` (1 <= k < V) keeps every ``s >=`` the k-th largest value, ties at that value included; ``min_p``
    (> 0) then keeps ``exp(s - smax) >= min_p``; ``top_p`` (< 1) then keeps ``s >= t*``, the largest kept value
    whose upper set ``{s >= t*}`` holds at least ``top_p`` of the kept mass: the usual nucleus, except that tokens
    tied at the cut are all kept. The token is the smallest kept index whose running mass, in vocabulary order,
    reaches ``u`` times the kept mass; never an index outside the kept set. ``temperature == 0`` is greedy: the
    lowest index of the maximum, ``kept = 1``, the filters ignored. A row with a NaN or without a finite ``s`` gets
    some token in [0, V).

    Each setting is a scalar for all rows or a tensor [B] (``top_k`` integer, ``k >= V`` for none), so one call
    can mix a greedy row with sampled ones. Scalars are range-checked; tensors are clamped to the same ranges
    where they are used, never read back. ``finished`` (uint8 or bool [B], with ``eos_id``) is updated in place:
    a finished row gets ``eos_id`` (and ``kept = 0``), another row that draws ``eos_id`` becomes finished.

    GPU logits in fp32, bf16 or fp16 with unit inner stride run the kernel (the same bits of ``tokens`` and
    ``kept`` every run: integer sums only, no floating-point atomics); anything else ``sample_logits_ref``."""
    if (logits.is_cuda and logits.dim() == 2 and logits.shape[1] >= 1 and logits.stride(1) == 1
            and (logits.shape[0] <= 1 or logits.stride(0) >= logits.shape[1])
            and logits.dtype in (torch.float32, torch.bfloat16, torch.float16) and u.is_cuda
            and u.device == logits.device
            and (finished is None or (finished.is_cuda and finished.dtype in (torch.uint8, torch.bool)
                                      and finished.is_contiguous()))):
        _sample_scalars(temperature, top_k, top_p, min_p)
        B, dev = logits.shape[0], logits.device

        def split(x, dtype, default):
            if isinstance(x, torch.Tensor):
                if x.shape != (B,):
                    raise ValueError(f"sample_logits: a per-row setting must have shape [{B}], got {tuple(x.shape)}")
                return default, x.to(device=dev, dtype=dtype).contiguous()
            return (default if x is None else x), None

        t_s, t_r = split(temperature, torch.float32, 1.0)
        k_s, k_r = split(top_k, torch.int32, 0)
        p_s, p_r = split(top_p, torch.float32, 1.0)
        m_s, m_r = split(min_p, torch.float32, 0.0)
        if (eos_id is None) != (finished is None):
            raise ValueError("sample_logits: eos_id and finished come together")
        fin = finished.view(torch.uint8) if finished is not None and finished.dtype == torch.bool else finished
        tokens, kept = native.C().sample_logits(logits, u.float().contiguous(), float(t_s), min(int(k_s), 2**31 - 1),
                                                float(p_s), float(m_s), t_r, k_r, p_r, m_r, eos_id, fin)
        return (tokens, kept) if return_kept else tokens
    return sample_logits_ref(logits, u, temperature, top_k, top_p, min_p, eos_id, finished, return_kept)
