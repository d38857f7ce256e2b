"""Grouped-query flash attention on gfx950 (``csrc/kernels/attention.hip``) as an autograd op.

``attention(q, k, v, causal)`` takes the Llama model's natural layout — q ``[B, S, Hq, D]``,
k/v ``[B, S, Hkv, D]`` — and returns ``[B, S, Hq, D]``. bf16 GPU tensors with D in {64, 128}
run the native forward (online softmax, row log-sum-exp kept for the backward) and the
deterministic native backward (delta, dQ per query block, dK/dV per key block over the
whole query-head group). Anything else — CPU tensors (the gloo tests), fp32, other head
sizes — runs the plain-PyTorch reference below, which is also the numerics oracle of
``tests/test_attention_gpu.py``.

Packed sequences: several documents in one row, a token attending only inside its own document
(and causally). ``doc_ids_from_eos`` / ``doc_bounds`` turn token ids into the two ``int32 [B, S]``
arrays the kernels read (``DocBounds``: first visible key per query, one past the last seeing
query per key), and ``attention(..., doc=bounds)`` runs the document-masked kernels, which visit
only the key tiles back to a query block's oldest document. Document masks are causal only.

Decoding: ``decode_attention(q, k_cache, v_cache, lens)`` is one query row per head against a ``KVCache``
(``csrc/kernels/attn_decode.hip``: split over the keys, K/V read once per kv head; docs/decode_attention.md).
An FP8 cache (``KVCache.allocate(..., dtype=torch.float8_e4m3fn)``) stores e4m3fn codes and one fp32 scale per
(token, kv head): ``kv_cache_append`` quantises into it (``csrc/kernels/kv_append_fp8.hip``) and
``decode_attention(..., k_scale=, v_scale=)`` reads it.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional

import torch

from . import native


class DocBounds(NamedTuple):
    """Document mask of a packed batch: query i sees key j iff ``kstart[b, i] <= j <= i``, which is
    ``j <= i < qend[b, j]``. Both ``int32 [B, S]``, contiguous, non-decreasing along S."""
    kstart: torch.Tensor
    qend: torch.Tensor


def doc_ids_from_eos(tokens: torch.Tensor, eos_id: int) -> torch.Tensor:
    """``int64 [B, S]`` document index of every position: the number of EOS tokens strictly before
    it in its row (an EOS closes its own document; the next token opens a new one)."""
    eos = (tokens == eos_id).long()
    return eos.cumsum(1) - eos


def doc_bounds(doc_ids: torch.Tensor) -> DocBounds:
    """``DocBounds`` of ``doc_ids`` (any integer dtype, ``[B, S]``, every row non-decreasing: a
    document is one contiguous run of equal ids; rows may differ). Torch ops on ``doc_ids``' device
    only, no host read-back of device data: ids that decrease raise ``ValueError`` when ``doc_ids``
    is a host tensor; on a GPU that check would cost a synchronisation per step and is not made —
    every change of id then starts a new document, so the bounds are still consistent."""
    if doc_ids.dim() != 2 or doc_ids.dtype.is_floating_point or doc_ids.dtype == torch.bool:
        raise ValueError("doc_ids must be an integer [B, S] tensor")
    B, S = doc_ids.shape
    d = doc_ids.long()
    if S > 1:
        step = d[:, 1:] - d[:, :-1]
        if not doc_ids.is_cuda and bool((step < 0).any()):
            raise ValueError("doc_ids must not decrease along a row: documents are contiguous runs")
    pos = torch.arange(S, device=d.device).expand(B, S)
    first = torch.ones(B, S, dtype=torch.bool, device=d.device)
    last = torch.ones(B, S, dtype=torch.bool, device=d.device)
    if S > 1:
        first[:, 1:] = step != 0
        last[:, :-1] = step != 0
    # a run's start carried forward / its end carried backward
    kstart = torch.where(first, pos, pos.new_zeros(())).cummax(1).values
    qend = torch.where(last, pos + 1, pos.new_full((), S)).flip(1).cummin(1).values.flip(1)
    return DocBounds(kstart.int().contiguous(), qend.int().contiguous())


def doc_mask(doc: DocBounds) -> torch.Tensor:
    """bool ``[B, S, S]`` (query, key), True where the query may see the key."""
    S = doc.kstart.shape[1]
    pos = torch.arange(S, device=doc.kstart.device)
    return (pos.view(1, 1, S) >= doc.kstart.long().unsqueeze(2)) & (pos.view(1, 1, S) <= pos.view(1, S, 1))


def attention_ref(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, causal: bool = True,
                  doc: Optional[DocBounds] = None) -> torch.Tensor:
    """Math attention in fp32 on [B, S, H, D] tensors (GQA by head repetition)."""
    if doc is not None and not causal:
        raise ValueError("a document mask is defined only together with causal=True")
    B, S, Hq, D = q.shape
    rep = Hq // k.shape[2]
    qf = q.float().transpose(1, 2)
    kf = k.float().repeat_interleave(rep, dim=2).transpose(1, 2)
    vf = v.float().repeat_interleave(rep, dim=2).transpose(1, 2)
    s = qf @ kf.transpose(-1, -2) / math.sqrt(D)
    if doc is not None:
        s = s.masked_fill(~doc_mask(doc).unsqueeze(1), float("-inf"))
    elif causal:
        mask = torch.ones(S, S, dtype=torch.bool, device=q.device).triu(1)
        s = s.masked_fill(mask, float("-inf"))
    o = torch.softmax(s, -1) @ vf
    return o.transpose(1, 2).to(q.dtype)


class _FlashAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, causal, kstart=None, qend=None):
        q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        scale = 1.0 / math.sqrt(q.shape[-1])
        if kstart is None:
            o, lse = native.C().attn_fwd(q, k, v, scale, causal)
            ctx.save_for_backward(q, k, v, o, lse)
        else:
            o, lse = native.C().attn_fwd(q, k, v, scale, causal, kstart, qend)
            ctx.save_for_backward(q, k, v, o, lse, kstart, qend)
        ctx.causal, ctx.scale = causal, scale
        return o

    @staticmethod
    def backward(ctx, do):
        q, k, v, o, lse, *doc = ctx.saved_tensors
        dq, dk, dv = native.C().attn_bwd(q, k, v, o, lse, do.contiguous().to(q.dtype), ctx.scale, ctx.causal, *doc)
        return dq, dk, dv, None, None, None


def native_ok(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor) -> bool:
    return (q.is_cuda and q.dtype == torch.bfloat16 and k.dtype == q.dtype and v.dtype == q.dtype
            and q.shape[-1] in (64, 128) and q.shape[2] % k.shape[2] == 0)


def attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, causal: bool = True,
              doc: Optional[DocBounds] = None) -> torch.Tensor:
    if doc is None:
        if native_ok(q, k, v):
            return _FlashAttention.apply(q, k, v, causal)
        return attention_ref(q, k, v, causal)
    if not causal:
        raise ValueError("a document mask is defined only together with causal=True")
    if native_ok(q, k, v):
        return _FlashAttention.apply(q, k, v, True, doc.kstart, doc.qend)
    return attention_ref(q, k, v, True, doc)


# ------------------------------------------------------------------ decoding against a KV cache
FP8 = torch.float8_e4m3fn
FP8_MAX = 448.0  # the largest finite e4m3fn value
_SCALE_MIN_EXP = -126  # the scale and its reciprocal stay normal fp32 numbers


class KVCache:
    """The keys and values of every layer for B sequences of up to ``Smax`` positions, in the model's natural
    layout: ``k``, ``v`` ``[n_layers, B, Smax, Hkv, hd]`` (uninitialised past the lengths), ``lens`` int32 ``[B]``
    on the device, and ``bound``, a host-side upper bound of ``lens`` (the prompt length plus the steps
    taken) that sizes the slice a decode step attends over without reading ``lens`` back.

    An FP8 cache (``dtype=torch.float8_e4m3fn``) holds e4m3fn codes in ``k`` and ``v`` and one power-of-two
    fp32 scale per (token, kv head) in ``k_scale`` / ``v_scale`` ``[n_layers, B, Smax, Hkv]`` (``kv_quantize_ref``
    states the format); both are ``None`` for any other dtype."""

    def __init__(self, k: torch.Tensor, v: torch.Tensor, lens: torch.Tensor, bound: int = 0,
                 k_scale: Optional[torch.Tensor] = None, v_scale: Optional[torch.Tensor] = None):
        self.k, self.v, self.lens, self.bound = k, v, lens, bound
        self.k_scale, self.v_scale = k_scale, v_scale

    @classmethod
    def allocate(cls, cfg, B: int, max_len: int, device=None, dtype=torch.bfloat16) -> "KVCache":
        """``cfg``: a ``LlamaConfig``. k and v (and the scales of an FP8 cache) come from ``torch.empty``:
        nothing past ``lens`` is ever read as a value."""
        if max_len < 1 or max_len > cfg.max_seq:
            raise ValueError(f"KVCache: max_len {max_len} outside [1, max_seq {cfg.max_seq}]")
        shape = (cfg.n_layers, B, max_len, cfg.n_kv_heads, cfg.dim // cfg.n_heads)
        scales = (None, None)
        if dtype == FP8:
            scales = tuple(torch.empty(shape[:-1], device=device, dtype=torch.float32) for _ in range(2))
        return cls(torch.empty(shape, device=device, dtype=dtype), torch.empty(shape, device=device, dtype=dtype),
                   torch.zeros(B, dtype=torch.int32, device=device), 0, *scales)


def _no_grad_inputs(name: str, *ts) -> None:
    if any(t.requires_grad for t in ts):
        raise RuntimeError(f"{name} is inference only (no backward): detach the inputs or run the model "
                           "under torch.no_grad()")


def kv_quantize_ref(x: torch.Tensor) -> tuple:
    """The FP8 KV-cache format in plain torch, on any device: ``x`` ``[..., D]`` (fp32, bf16 or fp64) ->
    ``(codes float8_e4m3fn [..., D], scale fp32 [...])``, one scale per row. With ``amax = max|x|`` of a row the
    scale is ``s = 2^e``, ``e`` the smallest integer with ``amax * 2^-e <= 448`` (a non-zero row has ``amax / s``
    in (224, 448]), kept ``>= -126``; ``amax == 0`` gives ``s = 1``. The code of ``x[i]`` is ``x[i] * 2^-e``
    rounded to fp32 (exact for bf16 and fp32 rows) and then to e4m3fn, nearest-even; ``float(code) * s`` is the
    value. A row with a non-finite element gets unspecified codes. The CPU path and the fallback of
    ``kv_cache_append``; ``csrc/kernels/kv_append_fp8.hip`` gives the same bytes."""
    ct = torch.float64 if x.dtype == torch.float64 else torch.float32
    with torch.no_grad():
        xf = x.to(ct)
        amax = xf.abs().amax(-1)
        m, ex = torch.frexp(amax)  # amax = m * 2^ex, m in [0.5, 1); 448 = 0.875 * 2^9
        e = torch.where(m <= 0.875, ex - 9, ex - 8).clamp(_SCALE_MIN_EXP, 127)
        e = torch.where(amax > 0, e, torch.zeros_like(e))
        one = torch.ones((), dtype=ct, device=x.device)
        y = (xf * torch.ldexp(one, -e).unsqueeze(-1)).float().clamp(-FP8_MAX, FP8_MAX)
        return y.to(FP8), torch.ldexp(one, e).float()


def kv_dequantize(codes: torch.Tensor, scale: torch.Tensor, dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """``float(code) * scale`` of every row: ``codes`` float8_e4m3fn ``[..., D]``, ``scale`` fp32 ``[...]`` ->
    ``dtype`` ``[..., D]``. The product is exact in fp32 and, for a scale ``kv_quantize_ref`` made, in bf16."""
    return (codes.float() * scale.unsqueeze(-1)).to(dtype)


def kv_append_native_ok(k_cache: torch.Tensor, v_cache: torch.Tensor, k_scale: torch.Tensor, v_scale: torch.Tensor,
                        k: torch.Tensor, v: torch.Tensor, pos: Optional[torch.Tensor] = None) -> bool:
    """Whether ``kv_append_fp8_kernel`` takes these operands: everything on one GPU, k / v bf16 contiguous and
    16-byte aligned with D in {64, 128}, the caches contiguous in their inner three and the scales in their
    inner two dimensions, each pair with one batch stride, ``pos`` a contiguous int32 [B] on the device."""
    ts = (k_cache, v_cache, k_scale, v_scale, k, v) + (() if pos is None else (pos,))
    if not all(t.is_cuda and t.device == k.device for t in ts):
        return False
    if not (k.dtype == v.dtype == torch.bfloat16 and k.is_contiguous() and v.is_contiguous()):
        return False
    B, _, Hkv, D = k.shape
    Smax = k_cache.shape[1]
    if D not in (64, 128):
        return False
    for c, sc in ((k_cache, k_scale), (v_cache, v_scale)):
        if c.stride()[1:] != (Hkv * D, D, 1) or sc.stride()[1:] != (Hkv, 1):
            return False
        if B > 1 and (c.stride(0) % 8 != 0 or c.stride(0) < Smax * Hkv * D or sc.stride(0) < Smax * Hkv):
            return False
    if B > 1 and (k_cache.stride(0) != v_cache.stride(0) or k_scale.stride(0) != v_scale.stride(0)):
        return False
    if pos is not None and not (pos.dtype == torch.int32 and pos.is_contiguous()):
        return False
    return all(t.data_ptr() % 16 == 0 for t in (k, v, k_cache, v_cache))


def kv_cache_append(k_cache: torch.Tensor, v_cache: torch.Tensor, k_scale: torch.Tensor, v_scale: torch.Tensor,
                    k: torch.Tensor, v: torch.Tensor, pos: Optional[torch.Tensor] = None) -> None:
    """Quantise ``k`` and ``v`` ``[B, S, Hkv, D]`` into an FP8 cache, in place: the caches float8_e4m3fn
    ``[B, Smax, Hkv, D]``, the scales fp32 ``[B, Smax, Hkv]``. Token ``(b, s)`` goes to position
    ``(pos[b] if pos is not None else 0) + s``, clamped into ``[0, Smax - 1]`` (on the GPU inside the kernel: no
    value of ``pos``, an int32 ``[B]`` device tensor, moves a store out of the cache); of several tokens of one
    sequence that the clamp folds onto one position, the last is stored. One launch of ``kv_append_fp8_kernel``
    for both tensors when ``kv_append_native_ok`` holds, ``kv_quantize_ref`` and index copies otherwise."""
    _no_grad_inputs("kv_cache_append", k, v)
    if k_cache.dtype != FP8 or v_cache.dtype != FP8:
        raise ValueError("kv_cache_append: the caches must be float8_e4m3fn")
    if k_scale is None or v_scale is None or k_scale.dtype != torch.float32 or v_scale.dtype != torch.float32:
        raise ValueError("kv_cache_append: an FP8 cache needs its fp32 scales")
    if k.dim() != 4 or k.shape != v.shape or k_cache.dim() != 4 or k_cache.shape != v_cache.shape:
        raise ValueError("kv_cache_append: k, v must be [B, S, Hkv, D] and the caches [B, Smax, Hkv, D]")
    B, S, Hkv, D = k.shape
    Smax = k_cache.shape[1]
    if (k_cache.shape[0], k_cache.shape[2], k_cache.shape[3]) != (B, Hkv, D) or Smax < 1:
        raise ValueError(f"kv_cache_append: caches {tuple(k_cache.shape)} do not take k {tuple(k.shape)}")
    if k_scale.shape != (B, Smax, Hkv) or v_scale.shape != (B, Smax, Hkv):
        raise ValueError(f"kv_cache_append: the scales must be [{B}, {Smax}, {Hkv}]")
    if pos is not None and (pos.shape != (B,) or pos.dtype.is_floating_point):
        raise ValueError("kv_cache_append: pos must be an integer [B] tensor")
    if B == 0 or S == 0:
        return
    with torch.no_grad():
        if kv_append_native_ok(k_cache, v_cache, k_scale, v_scale, k, v, pos):
            native.C().kv_append_fp8(k_cache, v_cache, k_scale, v_scale, k, v, pos)
            return
        dev = k.device
        s = torch.arange(S, device=dev).view(1, S)
        base = torch.zeros(B, 1, dtype=torch.int64, device=dev) if pos is None else pos.to(dev).long().view(B, 1)
        p = base + s
        # folded tokens take the data of the one that wins, so every duplicate write carries the same bytes
        src = torch.where(p >= Smax - 1, S - 1, torch.where(p <= 0, (-base).clamp(0, S - 1), s.expand(B, S)))
        rows = (torch.arange(B, device=dev).view(B, 1) * S + src).reshape(-1)
        for x, cache, scale in ((k, k_cache, k_scale), (v, v_cache, v_scale)):
            codes, sc = kv_quantize_ref(x.reshape(B * S, Hkv, D).index_select(0, rows))
            pc = p.clamp(0, Smax - 1)
            for b in range(B):  # per sequence: a cache may carry a batch stride (cache[:, :n])
                cache[b].view(torch.uint8).index_copy_(0, pc[b], codes[b * S:(b + 1) * S].view(torch.uint8))
                scale[b].index_copy_(0, pc[b], sc[b * S:(b + 1) * S])


def _check_cache_args(name: str, k_cache, v_cache, k_scale, v_scale) -> bool:
    """-> whether the caches are FP8; ValueError when dtype and scales do not go together"""
    fp8 = k_cache.dtype == FP8 or v_cache.dtype == FP8
    if fp8:
        if k_cache.dtype != v_cache.dtype:
            raise ValueError(f"{name}: one cache is float8_e4m3fn and the other {v_cache.dtype}")
        if k_scale is None or v_scale is None:
            raise ValueError(f"{name}: float8_e4m3fn caches need k_scale and v_scale")
        if k_scale.dtype != torch.float32 or v_scale.dtype != torch.float32:
            raise ValueError(f"{name}: k_scale and v_scale must be fp32")
        if k_scale.shape != k_cache.shape[:-1] or v_scale.shape != v_cache.shape[:-1]:
            raise ValueError(f"{name}: the scales must be [B, Smax, Hkv] like the caches")
    elif k_scale is not None or v_scale is not None:
        raise ValueError(f"{name}: k_scale / v_scale go with float8_e4m3fn caches only, got {k_cache.dtype}")
    return fp8


def decode_attention_ref(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, lens: torch.Tensor,
                         scale: Optional[float] = None, k_scale: Optional[torch.Tensor] = None,
                         v_scale: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Decode attention in plain torch: q ``[B, Hq, D]`` against ``k_cache`` / ``v_cache`` ``[B, Smax, Hkv, D]``,
    row b seeing keys ``0 .. lens[b] - 1`` (``lens`` clamped into [0, Smax]) -> ``[B, Hq, D]`` in q's dtype.
    fp32 math (fp64 for fp64 inputs), GQA by head repetition. Keys past the length are removed with
    ``torch.where`` from both the scores and V, so whatever the cache holds there (NaN, Inf) cannot leak; a
    row with no visible key gives zeros. FP8 caches (with ``k_scale`` / ``v_scale`` fp32 ``[B, Smax, Hkv]``) are
    dequantised first. The CPU path and the fallback of ``decode_attention``."""
    _no_grad_inputs("decode_attention_ref", q, k_cache, v_cache)
    fp8 = _check_cache_args("decode_attention_ref", k_cache, v_cache, k_scale, v_scale)
    B, Hq, D = q.shape
    Smax, Hkv = k_cache.shape[1], k_cache.shape[2]
    rep = Hq // Hkv
    ct = torch.float64 if q.dtype == torch.float64 else torch.float32
    scale = 1.0 / math.sqrt(D) if scale is None else scale
    with torch.no_grad():
        if fp8:
            k_cache, v_cache = kv_dequantize(k_cache, k_scale, ct), kv_dequantize(v_cache, v_scale, ct)
        vis = torch.arange(Smax, device=q.device).view(1, Smax) < lens.to(q.device).long().clamp(0, Smax).view(B, 1)
        kf = k_cache.to(ct).repeat_interleave(rep, dim=2)  # [B, Smax, Hq, D]
        vf = torch.where(vis.view(B, Smax, 1, 1), v_cache.to(ct), 0.0).repeat_interleave(rep, dim=2)
        s = torch.einsum("bhd,bshd->bhs", q.to(ct), kf) * scale
        s = torch.where(vis.view(B, 1, Smax), s, float("-inf"))
        mx = s.amax(-1, keepdim=True)
        p = torch.exp(s - torch.where(torch.isinf(mx), 0.0, mx))  # a masked key: exp(-inf) = 0
        l = p.sum(-1, keepdim=True)
        o = torch.einsum("bhs,bshd->bhd", p, vf) / torch.where(l > 0, l, 1.0)
    return o.to(q.dtype)


def decode_native_ok(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, lens: torch.Tensor,
                     k_scale: Optional[torch.Tensor] = None, v_scale: Optional[torch.Tensor] = None) -> bool:
    """Whether a gfx950 kernel takes these operands: GPU, bf16 q, D in {64, 128}, Hq / Hkv in {1, 2, 4, 8},
    int32 contiguous ``lens``, q contiguous, the caches contiguous in their inner three dimensions with one
    batch stride that is a multiple of 8, everything 16-byte aligned; the caches bf16 without scales, or
    float8_e4m3fn with fp32 scales ``[B, Smax, Hkv]`` on the same GPU, contiguous in their inner two dimensions
    with one batch stride."""
    if not (q.is_cuda and k_cache.is_cuda and v_cache.is_cuda and lens.is_cuda):
        return False
    fp8 = k_scale is not None or v_scale is not None
    if fp8 and (k_scale is None or v_scale is None):
        return False
    kv_dtype = FP8 if fp8 else torch.bfloat16
    if not (q.dtype == torch.bfloat16 and k_cache.dtype == v_cache.dtype == kv_dtype and lens.dtype == torch.int32):
        return False
    if q.dim() != 3 or k_cache.dim() != 4 or k_cache.shape != v_cache.shape:
        return False
    B, Hq, D = q.shape
    Smax, Hkv = k_cache.shape[1], k_cache.shape[2]
    if k_cache.shape[0] != B or k_cache.shape[3] != D or D not in (64, 128) or Smax < 1 or B > 65535:
        return False
    if Hkv < 1 or Hq % Hkv != 0 or Hq // Hkv not in (1, 2, 4, 8) or lens.shape != (B,) or not lens.is_contiguous():
        return False
    for c in (k_cache, v_cache):
        if c.stride()[1:] != (Hkv * D, D, 1) or (B > 1 and (c.stride(0) % 8 != 0 or c.stride(0) < Smax * Hkv * D)):
            return False
    if B > 1 and k_cache.stride(0) != v_cache.stride(0):
        return False
    if fp8:
        for sc in (k_scale, v_scale):
            if not (sc.is_cuda and sc.device == q.device and sc.dtype == torch.float32 and sc.shape == (B, Smax, Hkv)):
                return False
            if sc.stride()[1:] != (Hkv, 1) or (B > 1 and sc.stride(0) < Smax * Hkv):
                return False
        if B > 1 and k_scale.stride(0) != v_scale.stride(0):
            return False
    return q.is_contiguous() and all(t.data_ptr() % 16 == 0 for t in (q, k_cache, v_cache))


def decode_attention(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, lens: torch.Tensor,
                     scale: Optional[float] = None, splits: Optional[int] = None,
                     k_scale: Optional[torch.Tensor] = None, v_scale: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One query row per head against a KV cache: q ``[B, Hq, D]``, caches ``[B, Smax, Hkv, D]`` (a ``[:, :n]``
    slice of a longer cache is fine), ``lens`` int32 ``[B]`` -> ``[B, Hq, D]``. Row b sees keys
    ``0 .. lens[b] - 1``; ``lens`` is clamped into [0, Smax] and a row of length 0 gives zeros. Stale cache
    rows past the length contribute exactly nothing.

    The gfx950 split-KV kernel runs when ``decode_native_ok`` holds, ``decode_attention_ref`` otherwise.
    ``splits``: the number of key slices per (sequence, kv head); ``None`` picks it from B, Hkv and Smax
    (``decode_splits``), any other value is clamped into [1, key tiles of Smax]. Inference only.

    FP8 caches: float8_e4m3fn ``k_cache`` / ``v_cache`` with ``k_scale`` / ``v_scale`` fp32 ``[B, Smax, Hkv]``
    (``kv_cache_append`` fills them) run the FP8 kernel, which reads the codes and applies each scale once per
    key; stale codes and stale scales (NaN) contribute nothing. A cache dtype and scales that do not go
    together (an FP8 cache without scales, scales with a bf16 cache) raise ``ValueError``."""
    _no_grad_inputs("decode_attention", q, k_cache, v_cache)
    fp8 = _check_cache_args("decode_attention", k_cache, v_cache, k_scale, v_scale)
    if decode_native_ok(q, k_cache, v_cache, lens, k_scale, v_scale):
        scale = 1.0 / math.sqrt(q.shape[-1]) if scale is None else scale
        nsplit = 0 if splits is None else max(int(splits), 1)
        with torch.no_grad():
            if fp8:
                return native.C().attn_decode_fp8(q, k_cache, v_cache, k_scale, v_scale, lens, float(scale), nsplit)
            return native.C().attn_decode(q, k_cache, v_cache, lens, float(scale), nsplit)
    return decode_attention_ref(q, k_cache, v_cache, lens, scale, k_scale, v_scale)


def decode_key_tile() -> int:
    """Keys a workgroup of the decode kernel reads per trip (slices are whole tiles)."""
    return native.C().decode_key_tile()


def decode_splits(B: int, Hkv: int, Smax: int) -> int:
    """The key splits the kernel picks for these shapes: from B, Hkv and Smax only, never from ``lens``."""
    return native.C().decode_splits(B, Hkv, Smax)
