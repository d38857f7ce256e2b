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

Paged cache: ``PagedKVCache`` keeps K/V in a pool of fixed-size pages shared by all sequences, with a block table
per sequence; ``kv_cache_append_paged`` (``csrc/kernels/kv_append_paged.hip``) and ``decode_attention_paged`` (the
paged instantiations of the decode kernel) write and read through the table, in bf16 and FP8.

Extend: ``extend_attention(q, k_cache, v_cache, start, counts)`` and ``extend_attention_paged`` run T new tokens per
row against a cache that already holds their k and v behind the row's earlier keys (``csrc/kernels/attn_extend.hip``,
the flash forward's tile loop with a bottom-right aligned causal mask; docs/extend_attention.md): continuing a
sequence, chunked prefill, verifying several proposed tokens at once. FP8 caches are dequantised into a bf16 scratch
first (the slow path).
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
    B, D = q.shape[0], q.shape[2]
    Smax = k_cache.shape[1]
    ct = torch.float64 if q.dtype == torch.float64 else torch.float32
    scale = 1.0 / math.sqrt(D) if scale is None else scale
    with torch.no_grad():
        if fp8:
            k_cache, v_cache = kv_dequantize(k_cache, k_scale, ct), kv_dequantize(v_cache, v_scale, ct)
        vis = torch.arange(Smax, device=q.device).view(1, Smax) < lens.to(q.device).long().clamp(0, Smax).view(B, 1)
        return _decode_math(q, k_cache, v_cache, vis, scale, ct)


def _decode_math(q, k_cache, v_cache, vis, scale, ct) -> torch.Tensor:
    """softmax(q k^T * scale) v over the keys where ``vis`` bool ``[B, Smax]`` holds, in dtype ``ct``; everything
    else is removed with ``torch.where`` from both the scores and V. -> ``[B, Hq, D]`` in q's dtype."""
    B, Hq, D = q.shape
    Smax, Hkv = k_cache.shape[1], k_cache.shape[2]
    rep = Hq // Hkv
    with torch.no_grad():
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


# ------------------------------------------------------------------ the paged KV cache
PAGE_TILE = 64  # decode_key_tile(): a page is whole key tiles, so a tile of the decode kernel has one table entry


def _bytes_view(t: torch.Tensor) -> torch.Tensor:
    """FP8 tensors are indexed through their bytes (torch indexes float8 on no device reliably)"""
    return t.view(torch.uint8) if t.dtype == FP8 else t


def paged_gather(pages: torch.Tensor, block_table: torch.Tensor, n: Optional[int] = None) -> torch.Tensor:
    """The logical view of a paged tensor, in plain torch on any device: ``pages`` ``[P, page, ...]``,
    ``block_table`` integer ``[B, C]`` -> ``[B, n, ...]`` (``n`` defaults to ``C * page``), row ``i`` of sequence b
    being row ``i % page`` of page ``block_table[b, i // page]``. Rows of an invalid page (an entry outside
    ``[0, P)``, ``-1`` included) come back as zeros. A copy; for the references and the tests."""
    P, page = pages.shape[0], pages.shape[1]
    B, C = block_table.shape
    n = C * page if n is None else n
    if n < 0 or n > C * page:
        raise ValueError(f"paged_gather: n {n} outside [0, {C} * {page}]")
    cols = -(-n // page)
    t = block_table[:, :cols].to(pages.device).long()
    valid = (t >= 0) & (t < P)
    src = _bytes_view(pages)
    out = src[t.clamp(0, P - 1).reshape(-1)].reshape(B, cols, *src.shape[1:])
    out = torch.where(valid.view(B, cols, *([1] * (src.dim() - 1))), out, torch.zeros((), dtype=src.dtype,
                                                                                       device=src.device))
    return out.reshape(B, cols * page, *src.shape[2:])[:, :n].view(pages.dtype)


def _paged_visible(block_table: torch.Tensor, lens: torch.Tensor, P: int, page: int, device) -> torch.Tensor:
    """bool [B, C * page]: key n of sequence b is visible iff n < lens[b] (clamped into [0, C * page]) and its
    table entry lies in [0, P)"""
    B, C = block_table.shape
    Smax = C * page
    t = block_table.to(device).long()
    valid = ((t >= 0) & (t < P)).repeat_interleave(page, dim=1)
    return valid & (torch.arange(Smax, device=device).view(1, Smax) < lens.to(device).long().clamp(0, Smax).view(B, 1))


def _check_paged_args(name: str, k_pages, v_pages, block_table, k_scale, v_scale) -> bool:
    """-> whether the pools are FP8; ValueError for shapes, a bad page size, or a dtype and scales that do not go
    together"""
    if k_pages.dim() != 4 or k_pages.shape != v_pages.shape:
        raise ValueError(f"{name}: the pools must be [P, page, Hkv, D] of one shape")
    page = k_pages.shape[1]
    if page < PAGE_TILE or page % PAGE_TILE != 0:
        raise ValueError(f"{name}: the page size must be a positive multiple of {PAGE_TILE}, got {page}")
    if block_table.dim() != 2 or block_table.dtype.is_floating_point or block_table.dtype == torch.bool:
        raise ValueError(f"{name}: block_table must be an integer [B, C] tensor")
    fp8 = k_pages.dtype == FP8 or v_pages.dtype == FP8
    if fp8:
        if k_pages.dtype != v_pages.dtype:
            raise ValueError(f"{name}: one pool is float8_e4m3fn and the other {v_pages.dtype}")
        if k_scale is None or v_scale is None:
            raise ValueError(f"{name}: float8_e4m3fn pools need k_scale and v_scale")
        if k_scale.dtype != torch.float32 or v_scale.dtype != torch.float32:
            raise ValueError(f"{name}: k_scale and v_scale must be fp32")
        if k_scale.shape != k_pages.shape[:-1] or v_scale.shape != v_pages.shape[:-1]:
            raise ValueError(f"{name}: the scales must be [P, page, Hkv] like the pools")
    elif k_scale is not None or v_scale is not None:
        raise ValueError(f"{name}: k_scale / v_scale go with float8_e4m3fn pools only, got {k_pages.dtype}")
    return fp8


def _paged_layout_ok(k_pages, v_pages, block_table, k_scale, v_scale, B: int) -> bool:
    """the layout kv_append_paged.hip and the paged decode kernels take (check_paged_layout in the binding)"""
    P, page, Hkv, D = k_pages.shape
    fp8 = k_scale is not None
    ts = (k_pages, v_pages, block_table) + ((k_scale, v_scale) if fp8 else ())
    if not all(t.is_cuda and t.device == k_pages.device for t in ts):
        return False
    if k_pages.dtype != v_pages.dtype or k_pages.dtype != (FP8 if fp8 else torch.bfloat16):
        return False
    if k_pages.shape != v_pages.shape or P < 1 or Hkv < 1 or page < PAGE_TILE or page % PAGE_TILE != 0:
        return False
    if block_table.dtype != torch.int32 or block_table.dim() != 2 or block_table.shape[0] != B:
        return False
    C = block_table.shape[1]
    if C < 1 or (C > 1 and block_table.stride(1) != 1) or (B > 1 and block_table.stride(0) < C):
        return False
    if C * page > 2 ** 31 - 1:
        return False
    for c in (k_pages, v_pages):
        if c.stride()[1:] != (Hkv * D, D, 1) or (P > 1 and (c.stride(0) % 8 != 0 or c.stride(0) < page * Hkv * D)):
            return False
    if P > 1 and k_pages.stride(0) != v_pages.stride(0):
        return False
    if fp8:
        for sc in (k_scale, v_scale):
            if sc.dtype != torch.float32 or sc.shape != (P, page, Hkv):
                return False
            if sc.stride()[1:] != (Hkv, 1) or (P > 1 and sc.stride(0) < page * Hkv):
                return False
        if P > 1 and k_scale.stride(0) != v_scale.stride(0):
            return False
    return all(t.data_ptr() % 16 == 0 for t in (k_pages, v_pages))


def decode_attention_paged_ref(q: torch.Tensor, k_pages: torch.Tensor, v_pages: torch.Tensor,
                               block_table: torch.Tensor, lens: torch.Tensor, scale: Optional[float] = None,
                               k_scale: Optional[torch.Tensor] = None,
                               v_scale: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Paged decode attention in plain torch: gather the pools through the table (``paged_gather``), dequantise an
    FP8 pool, and run the math of ``decode_attention_ref`` over the keys that are below the length *and* on a
    valid page. Whatever a stale row, an unowned page or an invalid entry's page holds cannot leak; a sequence with
    no visible key gives zeros. The CPU path and the fallback of ``decode_attention_paged``."""
    _no_grad_inputs("decode_attention_paged_ref", q, k_pages, v_pages)
    fp8 = _check_paged_args("decode_attention_paged_ref", k_pages, v_pages, block_table, k_scale, v_scale)
    P, page = k_pages.shape[0], k_pages.shape[1]
    ct = torch.float64 if q.dtype == torch.float64 else torch.float32
    scale = 1.0 / math.sqrt(q.shape[-1]) if scale is None else scale
    with torch.no_grad():
        table = block_table.to(q.device)
        kc, vc = paged_gather(k_pages, table), paged_gather(v_pages, table)
        if fp8:
            kc = kv_dequantize(kc, paged_gather(k_scale, table), ct)
            vc = kv_dequantize(vc, paged_gather(v_scale, table), ct)
        vis = _paged_visible(table, lens, P, page, q.device)
        # the scores of masked keys are replaced, but a NaN row times q must not meet them on the way: zero K too
        kc = torch.where(vis.view(*vis.shape, 1, 1), kc.to(ct), 0.0)
        return _decode_math(q, kc, vc, vis, scale, ct)


def decode_paged_native_ok(q: torch.Tensor, k_pages: torch.Tensor, v_pages: torch.Tensor, block_table: torch.Tensor,
                           lens: torch.Tensor, k_scale: Optional[torch.Tensor] = None,
                           v_scale: Optional[torch.Tensor] = None) -> bool:
    """Whether the paged gfx950 decode kernel takes these operands: GPU, bf16 q ``[B, Hq, D]`` contiguous, D in
    {64, 128}, Hq / Hkv in {1, 2, 4, 8}, int32 contiguous ``lens``, pools ``[P, page, Hkv, D]`` contiguous in their
    inner three dimensions with one page stride that is a multiple of 8, page a multiple of 64, an int32
    ``block_table`` ``[B, C]`` on the same GPU with column stride 1, everything 16-byte aligned; the pools bf16
    without scales, or float8_e4m3fn with fp32 scales ``[P, page, Hkv]``."""
    if (k_scale is None) != (v_scale is None) or q.dim() != 3 or k_pages.dim() != 4:
        return False
    B, Hq, D = q.shape
    if not (q.is_cuda and lens.is_cuda and lens.device == q.device and k_pages.device == q.device):
        return False
    if not _paged_layout_ok(k_pages, v_pages, block_table, k_scale, v_scale, B):
        return False
    Hkv = k_pages.shape[2]
    if q.dtype != torch.bfloat16 or lens.dtype != torch.int32 or k_pages.shape[3] != D or D not in (64, 128):
        return False
    if B > 65535 or Hq % Hkv != 0 or Hq // Hkv not in (1, 2, 4, 8) or lens.shape != (B,) or not lens.is_contiguous():
        return False
    return q.is_contiguous() and q.data_ptr() % 16 == 0


def decode_attention_paged(q: torch.Tensor, k_pages: torch.Tensor, v_pages: torch.Tensor, block_table: torch.Tensor,
                           lens: torch.Tensor, scale: Optional[float] = None, splits: Optional[int] = None,
                           k_scale: Optional[torch.Tensor] = None,
                           v_scale: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One query row per head against a paged KV cache: q ``[B, Hq, D]``, pools ``[P, page, Hkv, D]`` shared by all
    sequences, ``block_table`` int32 ``[B, C]`` (``table[:, :c]`` of a wider table is fine), ``lens`` int32 ``[B]``
    -> ``[B, Hq, D]``. Key ``n`` of sequence b is row ``n % page`` of page ``block_table[b, n // page]``; it is
    visible iff ``n < lens[b]`` (clamped into ``[0, C * page]``) and the entry lies in ``[0, P)``. An entry outside
    that range (``-1``: no page) masks its keys; it is never folded onto another page. Invisible rows are never
    loaded and contribute exactly nothing; a sequence with no visible key gives zeros.

    The paged instantiation of the gfx950 split-KV kernel runs when ``decode_paged_native_ok`` holds,
    ``decode_attention_paged_ref`` otherwise. ``splits`` as in ``decode_attention``, with ``Smax = C * page``. For
    equal ``splits`` the result has the bits of ``decode_attention`` on ``paged_gather`` of the pools. FP8 pools
    come with ``k_scale`` / ``v_scale`` fp32 ``[P, page, Hkv]``; a dtype and scales that do not go together raise
    ``ValueError``. Inference only."""
    _no_grad_inputs("decode_attention_paged", q, k_pages, v_pages)
    fp8 = _check_paged_args("decode_attention_paged", k_pages, v_pages, block_table, k_scale, v_scale)
    if decode_paged_native_ok(q, k_pages, v_pages, block_table, lens, k_scale, v_scale):
        scale = 1.0 / math.sqrt(q.shape[-1]) if scale is None else scale
        nsplit = 0 if splits is None else max(int(splits), 1)
        with torch.no_grad():
            if fp8:
                return native.C().attn_decode_paged_fp8(q, k_pages, v_pages, k_scale, v_scale, block_table, lens,
                                                        float(scale), nsplit)
            return native.C().attn_decode_paged(q, k_pages, v_pages, block_table, lens, float(scale), nsplit)
    return decode_attention_paged_ref(q, k_pages, v_pages, block_table, lens, scale, k_scale, v_scale)


def kv_append_paged_native_ok(k_pages: torch.Tensor, v_pages: torch.Tensor, block_table: torch.Tensor,
                              k: torch.Tensor, v: torch.Tensor, pos: Optional[torch.Tensor] = None,
                              counts: Optional[torch.Tensor] = None, k_scale: Optional[torch.Tensor] = None,
                              v_scale: Optional[torch.Tensor] = None) -> bool:
    """Whether ``kv_append_paged_kernel`` takes these operands: everything on one GPU, k / v bf16 contiguous and
    16-byte aligned with D in {64, 128}, the pools in the layout of ``decode_paged_native_ok`` (bf16 without
    scales, float8_e4m3fn with them), ``pos`` and ``counts`` contiguous int32 [B] on the device."""
    if (k_scale is None) != (v_scale is None) or k.dim() != 4 or k_pages.dim() != 4:
        return False
    B, _, Hkv, D = k.shape
    if not (k.is_cuda and v.is_cuda and k.device == v.device == k_pages.device):
        return False
    if not (k.dtype == v.dtype == torch.bfloat16 and k.is_contiguous() and v.is_contiguous() and D in (64, 128)):
        return False
    if not _paged_layout_ok(k_pages, v_pages, block_table, k_scale, v_scale, B):
        return False
    if k_pages.shape[2:] != (Hkv, D):
        return False
    for t in (pos, counts):
        if t is not None and not (t.is_cuda and t.device == k.device and t.dtype == torch.int32 and t.shape == (B,)
                                  and t.is_contiguous()):
            return False
    return k.data_ptr() % 16 == 0 and v.data_ptr() % 16 == 0


def kv_cache_append_paged_ref(k_pages: torch.Tensor, v_pages: torch.Tensor, block_table: torch.Tensor,
                              k: torch.Tensor, v: torch.Tensor, pos: Optional[torch.Tensor] = None,
                              counts: Optional[torch.Tensor] = None, k_scale: Optional[torch.Tensor] = None,
                              v_scale: Optional[torch.Tensor] = None) -> None:
    """``kv_cache_append_paged`` in plain torch on any device: the store predicate per token, then index copies of
    the stored tokens (``kv_quantize_ref`` first for an FP8 pool, a cast to the pool's dtype otherwise). The
    boolean selection reads a count back from a GPU; the native path does not."""
    P, page = k_pages.shape[0], k_pages.shape[1]
    B, S, Hkv, D = k.shape
    C = block_table.shape[1]
    dev = k.device
    with torch.no_grad():
        s = torch.arange(S, device=dev).view(1, S)
        base = torch.zeros(B, 1, dtype=torch.int64, device=dev) if pos is None else pos.to(dev).long().view(B, 1)
        p = base + s
        ok = (p >= 0) & (p < C * page)
        if counts is not None:
            ok = ok & (s < counts.to(dev).long().view(B, 1))
        col = torch.div(p.clamp(0, C * page - 1), page, rounding_mode="floor")
        entry = block_table.to(dev).long().gather(1, col)
        ok = (ok & (entry >= 0) & (entry < P)).reshape(-1)
        entry, prow = entry.reshape(-1)[ok], (p.clamp(min=0) % page).reshape(-1)[ok]
        for x, pool, scale in ((k, k_pages, k_scale), (v, v_pages, v_scale)):
            rows = x.reshape(B * S, Hkv, D)[ok]
            if scale is not None:
                codes, sc = kv_quantize_ref(rows)
                pool.view(torch.uint8)[entry, prow] = codes.view(torch.uint8)
                scale[entry, prow] = sc
            else:
                pool[entry, prow] = rows.to(pool.dtype)


def kv_cache_append_paged(k_pages: torch.Tensor, v_pages: torch.Tensor, block_table: torch.Tensor, k: torch.Tensor,
                          v: torch.Tensor, pos: Optional[torch.Tensor] = None, counts: Optional[torch.Tensor] = None,
                          k_scale: Optional[torch.Tensor] = None, v_scale: Optional[torch.Tensor] = None) -> None:
    """Store ``k`` and ``v`` ``[B, S, Hkv, D]`` into the page pools ``[P, page, Hkv, D]`` of one layer, in place,
    through ``block_table`` int32 ``[B, C]``. Token ``(b, s)`` goes to logical position
    ``p = (pos[b] if pos is not None else 0) + s``, row ``p % page`` of page ``block_table[b, p // page]``, and is
    stored only if ``s < counts[b]`` (``counts`` int32 ``[B]``; absent means S), ``0 <= p < C * page`` and the
    table entry lies in ``[0, P)``. Otherwise it is *dropped*: unlike ``kv_cache_append`` nothing is clamped, since
    in a shared pool a folded write would land in live data. ``counts`` keeps the right-padding of a ragged prefill
    out of the pool. Two table rows that name one page are the caller's error (unspecified there, in bounds).

    FP8 pools (float8_e4m3fn with ``k_scale`` / ``v_scale`` fp32 ``[P, page, Hkv]``) take codes and scales in the
    format of ``kv_quantize_ref``; any other pool takes the rows cast to its dtype. One launch of
    ``kv_append_paged_kernel`` for both tensors when ``kv_append_paged_native_ok`` holds,
    ``kv_cache_append_paged_ref`` otherwise."""
    _no_grad_inputs("kv_cache_append_paged", k, v)
    _check_paged_args("kv_cache_append_paged", k_pages, v_pages, block_table, k_scale, v_scale)
    if k.dim() != 4 or k.shape != v.shape:
        raise ValueError("kv_cache_append_paged: k, v must be [B, S, Hkv, D] of one shape")
    B, S, Hkv, D = k.shape
    if k_pages.shape[2:] != (Hkv, D) or block_table.shape[0] != B or block_table.shape[1] < 1:
        raise ValueError(f"kv_cache_append_paged: pools {tuple(k_pages.shape)} and a table {tuple(block_table.shape)} "
                         f"do not take k {tuple(k.shape)}")
    for name, t in (("pos", pos), ("counts", counts)):
        if t is not None and (t.shape != (B,) or t.dtype.is_floating_point):
            raise ValueError(f"kv_cache_append_paged: {name} must be an integer [B] tensor")
    if B == 0 or S == 0:
        return
    with torch.no_grad():
        if kv_append_paged_native_ok(k_pages, v_pages, block_table, k, v, pos, counts, k_scale, v_scale):
            native.C().kv_append_paged(k_pages, v_pages, block_table, k, v, pos, counts, k_scale, v_scale)
            return
    kv_cache_append_paged_ref(k_pages, v_pages, block_table, k, v, pos, counts, k_scale, v_scale)


class PagedLayer(NamedTuple):
    """One layer of a ``PagedKVCache`` as ``Attention.forward``'s ``kv_out``: the pools, the table, the rows'
    token counts (a ragged prefill's lengths) and the scales of an FP8 pool."""
    k: torch.Tensor
    v: torch.Tensor
    block_table: torch.Tensor
    counts: Optional[torch.Tensor]
    k_scale: Optional[torch.Tensor]
    v_scale: Optional[torch.Tensor]


class PagedKVCache:
    """The keys and values of every layer in a pool of ``num_pages`` pages of ``page_size`` positions, shared by B
    sequence slots: ``k``, ``v`` ``[n_layers, P, page, Hkv, hd]`` (uninitialised), ``k_scale`` / ``v_scale``
    ``[n_layers, P, page, Hkv]`` for an FP8 pool (``None`` otherwise), one ``block_table`` int32 ``[B, Cmax]`` on the
    device shared by all layers (``-1``: no page), ``lens`` int32 ``[B]`` on the device and ``bound``, the host
    upper bound of ``lens``, as in ``KVCache``. Logical position n of slot b is row ``n % page`` of page
    ``block_table[b, n // page]`` in every layer.

    The allocator lives on the host: a free list and the page list of every slot (``reserve`` / ``free``), mirrored
    in a host copy of the table that ``commit`` uploads when it has changed. ``row_bound[b]`` is the host upper
    bound of ``lens[b]`` alone (``Llama.prefill`` sets it, ``decode_step`` advances it), which is what a slot's
    capacity is checked against. No reference counts, no prefix sharing or copy-on-write, no scheduler."""

    def __init__(self, k, v, block_table, lens, page_size: int, k_scale=None, v_scale=None):
        self.k, self.v, self.k_scale, self.v_scale = k, v, k_scale, v_scale
        self.block_table, self.lens, self.bound = block_table, lens, 0
        self.page_size, self.num_pages = page_size, k.shape[1]
        B, Cmax = block_table.shape
        self.row_bound = [0] * B
        self._host_table = torch.full((B, Cmax), -1, dtype=torch.int32)
        self._rows = [[] for _ in range(B)]
        self._free = list(range(self.num_pages - 1, -1, -1))  # a stack: page 0 is handed out first
        self._dirty = False

    @classmethod
    def allocate(cls, cfg, B: int, num_pages: int, page_size: int = PAGE_TILE, max_len: Optional[int] = None,
                 device=None, dtype=torch.bfloat16) -> "PagedKVCache":
        """``cfg``: a ``LlamaConfig``; ``max_len``: the longest a sequence may grow (default ``cfg.max_seq``), which
        sizes the table: ``Cmax = ceil(max_len / page_size)`` columns. The pools come from ``torch.empty``: no row
        outside a sequence's length and pages is ever read as a value."""
        if page_size < PAGE_TILE or page_size % PAGE_TILE != 0:
            raise ValueError(f"PagedKVCache: page_size must be a positive multiple of {PAGE_TILE}, got {page_size}")
        max_len = cfg.max_seq if max_len is None else max_len
        if max_len < 1 or max_len > cfg.max_seq:
            raise ValueError(f"PagedKVCache: max_len {max_len} outside [1, max_seq {cfg.max_seq}]")
        if B < 1 or num_pages < 1:
            raise ValueError("PagedKVCache: B and num_pages must be at least 1")
        shape = (cfg.n_layers, num_pages, page_size, cfg.n_kv_heads, cfg.dim // cfg.n_heads)
        scales = (None, None)
        if dtype == FP8:
            scales = tuple(torch.empty(shape[:-1], device=device, dtype=torch.float32) for _ in range(2))
        table = torch.full((B, -(-max_len // page_size)), -1, dtype=torch.int32, device=device)
        return cls(torch.empty(shape, device=device, dtype=dtype), torch.empty(shape, device=device, dtype=dtype),
                   table, torch.zeros(B, dtype=torch.int32, device=device), page_size, *scales)

    @staticmethod
    def pages_needed(lens, extra: int, page: int = PAGE_TILE) -> int:
        """The pages that sequences of ``lens`` tokens growing by ``extra`` tokens each take:
        ``sum_b ceil((lens[b] + extra) / page)``. Host arithmetic, to size a pool."""
        return sum(-(-(int(n) + extra) // page) for n in lens)

    @property
    def pages_free(self) -> int:
        return len(self._free)

    @property
    def pages_in_use(self) -> int:
        return self.num_pages - len(self._free)

    @property
    def max_len(self) -> int:
        return self.block_table.shape[1] * self.page_size

    def capacity(self, b: int) -> int:
        """the positions slot b's pages hold"""
        return len(self._rows[b]) * self.page_size

    def pages_of(self, b: int) -> list:
        return list(self._rows[b])

    def reserve(self, b: int, n_tokens: int) -> None:
        """Grow slot b to ``ceil(n_tokens / page)`` pages (never shrinks). ``RuntimeError``, with nothing changed,
        when the free pages do not cover the request; ``ValueError`` when the table has no such column. Host only:
        ``commit`` uploads the table."""
        need = -(-n_tokens // self.page_size) - len(self._rows[b])
        if need <= 0:
            return
        if len(self._rows[b]) + need > self._host_table.shape[1]:
            raise ValueError(f"PagedKVCache.reserve: {n_tokens} tokens exceed the table's {self.max_len} positions")
        if need > len(self._free):
            raise RuntimeError(f"PagedKVCache.reserve: slot {b} needs {need} more pages, {len(self._free)} are free")
        for _ in range(need):
            page = self._free.pop()
            self._host_table[b, len(self._rows[b])] = page
            self._rows[b].append(page)
        self._dirty = True

    def free(self, b: int) -> None:
        """Return slot b's pages to the free list; its table row becomes -1 (uploaded by ``commit``) and ``lens[b]``
        0, by a device op without a read-back."""
        if self._rows[b]:
            self._free.extend(reversed(self._rows[b]))
            self._rows[b] = []
            self._host_table[b].fill_(-1)
            self._dirty = True
        self.row_bound[b] = 0
        self.lens[b:b + 1].zero_()

    def commit(self) -> None:
        """Upload the host table when it has changed. The copy is staged through a freshly allocated pinned tensor
        and is asynchronous: torch's pinned allocator keeps that block alive until the copy has run, so two
        commits in a row need no host synchronisation and cannot tear."""
        if not self._dirty:
            return
        if self.block_table.is_cuda:
            stage = torch.empty(self._host_table.shape, dtype=torch.int32, pin_memory=True)
            stage.copy_(self._host_table)
            self.block_table.copy_(stage, non_blocking=True)
        else:
            self.block_table.copy_(self._host_table)
        self._dirty = False

    def layer(self, l: int, counts: Optional[torch.Tensor] = None, cols: Optional[int] = None) -> PagedLayer:
        """layer l's pools with the first ``cols`` table columns (all by default)"""
        table = self.block_table if cols is None else self.block_table[:, :cols]
        fp8 = self.k_scale is not None
        return PagedLayer(self.k[l], self.v[l], table, counts, self.k_scale[l] if fp8 else None,
                          self.v_scale[l] if fp8 else None)


# ------------------------------------------------------------------ extend: T new tokens against a filled cache
_EXT_RANGE = 0x7ffffff0  # bytes one buffer resource of the extend kernel may span (a sequence's rows / one page)


def _extend_bounds(start: torch.Tensor, counts, B: int, T: int, Smax: int, device) -> tuple:
    """-> (start clamped into [0, Smax], counts clamped into [0, min(T, Smax - start)]), int64 [B] on ``device``"""
    st = start.to(device).long().clamp(0, Smax)
    cnt = torch.full((B,), T, dtype=torch.int64, device=device) if counts is None else counts.to(device).long()
    return st, torch.minimum(cnt.clamp(0, T), Smax - st)


def _check_extend_args(name: str, q, B_cache: int, D_cache: int, Hkv: int, start, counts) -> None:
    if q.dim() != 4:
        raise ValueError(f"{name}: q must be [B, T, Hq, D]")
    B, _, Hq, D = q.shape
    if B_cache != B or D_cache != D or Hkv < 1 or Hq % Hkv != 0:
        raise ValueError(f"{name}: q {tuple(q.shape)} does not go with a cache of {B_cache} sequences, {Hkv} kv heads "
                         f"and head size {D_cache}")
    for what, t in (("start", start), ("counts", counts)):
        if t is not None and (t.shape != (B,) or t.dtype.is_floating_point or t.dtype == torch.bool):
            raise ValueError(f"{name}: {what} must be an integer [B] tensor")
    if start is None:
        raise ValueError(f"{name}: start is required")


def _extend_math(q, kc, vc, keyvis, st, cnt, scale, ct) -> torch.Tensor:
    """softmax(q k^T * scale) v, query i of row b over the keys n <= st[b] + i where ``keyvis`` bool [B, Smax] holds,
    for i < cnt[b]; in dtype ``ct``. Everything else is removed with ``torch.where`` from K, the scores and V. ->
    ``[B, T, Hq, D]`` in q's dtype, zeros where a query sees no key."""
    B, T, Hq, D = q.shape
    Smax, Hkv = kc.shape[1], kc.shape[2]
    rep = Hq // Hkv
    dev = q.device
    i = torch.arange(T, device=dev).view(1, T, 1)
    n = torch.arange(Smax, device=dev).view(1, 1, Smax)
    vis = (i < cnt.view(B, 1, 1)) & (n <= st.view(B, 1, 1) + i) & keyvis.view(B, 1, Smax)  # [B, T, Smax]
    anyvis = vis.any(1)  # [B, Smax]: a key no query sees is removed, whatever it holds
    kf = torch.where(anyvis.view(B, Smax, 1, 1), kc.to(ct), 0.0).repeat_interleave(rep, dim=2)
    vf = torch.where(anyvis.view(B, Smax, 1, 1), vc.to(ct), 0.0).repeat_interleave(rep, dim=2)
    s = torch.einsum("bthd,bshd->bhts", q.to(ct), kf) * scale
    s = torch.where(vis.view(B, 1, T, Smax), s, float("-inf"))
    mx = s.amax(-1, keepdim=True)
    p = torch.exp(s - torch.where(torch.isinf(mx), 0.0, mx))
    l = p.sum(-1, keepdim=True)
    o = torch.einsum("bhts,bshd->bthd", p / torch.where(l > 0, l, 1.0), vf)
    return o.to(q.dtype)


def extend_attention_ref(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, start: torch.Tensor,
                         counts: Optional[torch.Tensor] = None, scale: Optional[float] = None,
                         k_scale: Optional[torch.Tensor] = None, v_scale: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Extend attention in plain torch: q ``[B, T, Hq, D]``, the T new tokens of every row (right-padded), against
    ``k_cache`` / ``v_cache`` ``[B, Smax, Hkv, D]`` that already hold their k and v. ``start`` integer ``[B]`` is row
    b's length before these tokens (clamped into [0, Smax]), ``counts`` integer ``[B]`` its real new tokens (default
    T; clamped into [0, min(T, Smax - start)]). Query ``i < counts[b]`` sees keys ``0 .. start[b] + i``; rows
    ``i >= counts[b]`` come back as zeros. fp32 math (fp64 for fp64 inputs), GQA by head repetition; keys no query
    sees are removed with ``torch.where`` from the scores and from V (and K), so whatever the cache holds there
    cannot leak. FP8 caches (with ``k_scale`` / ``v_scale``) are dequantised first. The CPU path and the fallback of
    ``extend_attention``."""
    _no_grad_inputs("extend_attention_ref", q, k_cache, v_cache)
    fp8 = _check_cache_args("extend_attention_ref", k_cache, v_cache, k_scale, v_scale)
    if k_cache.dim() != 4 or k_cache.shape != v_cache.shape:
        raise ValueError("extend_attention_ref: the caches must be [B, Smax, Hkv, D] of one shape")
    _check_extend_args("extend_attention_ref", q, k_cache.shape[0], k_cache.shape[3], k_cache.shape[2], start, counts)
    B, T, _, D = q.shape
    Smax = k_cache.shape[1]
    ct = torch.float64 if q.dtype == torch.float64 else torch.float32
    scale = 1.0 / math.sqrt(D) if scale is None else scale
    with torch.no_grad():
        if fp8:
            k_cache, v_cache = kv_dequantize(k_cache, k_scale, ct), kv_dequantize(v_cache, v_scale, ct)
        st, cnt = _extend_bounds(start, counts, B, T, Smax, q.device)
        keyvis = torch.ones(B, Smax, dtype=torch.bool, device=q.device)
        return _extend_math(q, k_cache, v_cache, keyvis, st, cnt, scale, ct)


def extend_attention_paged_ref(q: torch.Tensor, k_pages: torch.Tensor, v_pages: torch.Tensor,
                               block_table: torch.Tensor, start: torch.Tensor, counts: Optional[torch.Tensor] = None,
                               scale: Optional[float] = None, k_scale: Optional[torch.Tensor] = None,
                               v_scale: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Paged extend attention in plain torch: gather the pools through the table (``paged_gather``), dequantise an
    FP8 pool, and run the math of ``extend_attention_ref`` with ``Smax = C * page`` over the keys that are also on a
    valid page (an entry outside ``[0, P)`` masks its keys). The CPU path and the fallback of
    ``extend_attention_paged``."""
    _no_grad_inputs("extend_attention_paged_ref", q, k_pages, v_pages)
    fp8 = _check_paged_args("extend_attention_paged_ref", k_pages, v_pages, block_table, k_scale, v_scale)
    _check_extend_args("extend_attention_paged_ref", q, block_table.shape[0], k_pages.shape[3], k_pages.shape[2],
                       start, counts)
    P, page = k_pages.shape[0], k_pages.shape[1]
    B, T, _, D = q.shape
    Smax = block_table.shape[1] * page
    ct = torch.float64 if q.dtype == torch.float64 else torch.float32
    scale = 1.0 / math.sqrt(D) if scale is None else scale
    with torch.no_grad():
        table = block_table.to(q.device)
        kc, vc = paged_gather(k_pages, table), paged_gather(v_pages, table)
        if fp8:
            kc = kv_dequantize(kc, paged_gather(k_scale, table), ct)
            vc = kv_dequantize(vc, paged_gather(v_scale, table), ct)
        st, cnt = _extend_bounds(start, counts, B, T, Smax, q.device)
        keyvis = ((table.long() >= 0) & (table.long() < P)).repeat_interleave(page, dim=1)
        return _extend_math(q, kc, vc, keyvis, st, cnt, scale, ct)


def _extend_index_ok(q: torch.Tensor, start: torch.Tensor, counts: Optional[torch.Tensor]) -> bool:
    for t in (start, counts):
        if t is not None and not (t.is_cuda and t.device == q.device and t.dtype == torch.int32
                                  and t.shape == (q.shape[0],) and t.is_contiguous()):
            return False
    return True


def extend_native_ok(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, start: torch.Tensor,
                     counts: Optional[torch.Tensor] = None, k_scale: Optional[torch.Tensor] = None,
                     v_scale: Optional[torch.Tensor] = None) -> bool:
    """Whether ``attn_extend_kernel`` takes these operands: GPU, bf16 q ``[B, T, Hq, D]`` contiguous, D in {64, 128},
    any Hq % Hkv == 0, bf16 caches without scales in the layout of ``decode_native_ok`` (contiguous in their inner
    three dimensions, one batch stride that is a multiple of 8: ``cache[:, :n]`` is fine) with one sequence's rows
    within 2 GiB, ``start`` (and ``counts``) contiguous int32 [B] on the device, everything 16-byte aligned. FP8
    caches are not the kernel's: ``extend_attention`` dequantises them first."""
    if k_scale is not None or v_scale is not None:
        return False
    if not (q.is_cuda and k_cache.is_cuda and v_cache.is_cuda and k_cache.device == v_cache.device == q.device):
        return False
    if not (q.dtype == k_cache.dtype == v_cache.dtype == torch.bfloat16):
        return False
    if q.dim() != 4 or k_cache.dim() != 4 or k_cache.shape != v_cache.shape:
        return False
    B, T, Hq, D = q.shape
    Smax, Hkv = k_cache.shape[1], k_cache.shape[2]
    if k_cache.shape[0] != B or k_cache.shape[3] != D or D not in (64, 128) or Smax < 1 or B > 65535 or Hq > 65535:
        return False
    if Hkv < 1 or Hq < 1 or Hq % Hkv != 0 or T > 2 ** 31 - 1 or not _extend_index_ok(q, start, counts):
        return False
    if (Smax - 1) * Hkv * D * 2 + 2 * D > _EXT_RANGE:
        return False
    for c in (k_cache, v_cache):
        if c.stride()[1:] != (Hkv * D, D, 1) or (B > 1 and (c.stride(0) % 8 != 0 or c.stride(0) < Smax * Hkv * D)):
            return False
    if B > 1 and k_cache.stride(0) != v_cache.stride(0):
        return False
    return q.is_contiguous() and all(t.data_ptr() % 16 == 0 for t in (q, k_cache, v_cache))


def extend_attention(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, start: torch.Tensor,
                     counts: Optional[torch.Tensor] = None, scale: Optional[float] = None,
                     k_scale: Optional[torch.Tensor] = None, v_scale: Optional[torch.Tensor] = None) -> torch.Tensor:
    """T new tokens per row against a KV cache that already holds their k and v (append, then attend): q
    ``[B, T, Hq, D]`` right-padded, caches ``[B, Smax, Hkv, D]`` (a ``[:, :n]`` slice of a longer cache is fine),
    ``start`` int32 ``[B]`` the rows' lengths before these tokens, ``counts`` int32 ``[B]`` their real new tokens
    (default T) -> ``[B, T, Hq, D]``. ``start`` is clamped into [0, Smax] and ``counts`` into
    [0, min(T, Smax - start)]. Query ``i < counts[b]`` sits at position ``start[b] + i`` and sees keys
    ``0 .. start[b] + i`` (the bottom-right aligned causal mask); rows ``i >= counts[b]`` are zeros. Keys at or past
    ``start[b] + counts[b]`` are stale: they are never loaded and contribute exactly nothing, V included.

    The gfx950 kernel (``csrc/kernels/attn_extend.hip``, the flash forward's tile loop against the cache;
    docs/extend_attention.md) runs when ``extend_native_ok`` holds, ``extend_attention_ref`` otherwise. T = 1 works,
    but ``decode_attention`` is the kernel for it. FP8 caches (float8_e4m3fn with ``k_scale`` / ``v_scale``) take
    the slow path: the operand is dequantised into a bf16 scratch (``kv_dequantize``) and the bf16 kernel runs on
    that; a dtype and scales that do not go together raise ``ValueError``. Inference only."""
    _no_grad_inputs("extend_attention", q, k_cache, v_cache)
    fp8 = _check_cache_args("extend_attention", k_cache, v_cache, k_scale, v_scale)
    if k_cache.dim() != 4 or k_cache.shape != v_cache.shape:
        raise ValueError("extend_attention: the caches must be [B, Smax, Hkv, D] of one shape")
    _check_extend_args("extend_attention", q, k_cache.shape[0], k_cache.shape[3], k_cache.shape[2], start, counts)
    if fp8 and q.is_cuda and q.dtype == torch.bfloat16 and k_cache.device == q.device:
        with torch.no_grad():  # the slow path: a bf16 copy of the operand (stale rows may hold anything: never loaded)
            kd = kv_dequantize(k_cache, k_scale, torch.bfloat16)
            vd = kv_dequantize(v_cache, v_scale, torch.bfloat16)
        if extend_native_ok(q, kd, vd, start, counts):
            return extend_attention(q, kd, vd, start, counts, scale)
    if extend_native_ok(q, k_cache, v_cache, start, counts, k_scale, v_scale):
        scale = 1.0 / math.sqrt(q.shape[-1]) if scale is None else scale
        with torch.no_grad():
            return native.C().attn_extend(q, k_cache, v_cache, start, float(scale), counts)
    return extend_attention_ref(q, k_cache, v_cache, start, counts, scale, k_scale, v_scale)


def extend_paged_native_ok(q: torch.Tensor, k_pages: torch.Tensor, v_pages: torch.Tensor, block_table: torch.Tensor,
                           start: torch.Tensor, counts: Optional[torch.Tensor] = None,
                           k_scale: Optional[torch.Tensor] = None, v_scale: Optional[torch.Tensor] = None) -> bool:
    """Whether the paged ``attn_extend_kernel`` takes these operands: GPU, bf16 q ``[B, T, Hq, D]`` contiguous, D in
    {64, 128}, any Hq % Hkv == 0, bf16 pools without scales and an int32 ``block_table`` in the layout of
    ``decode_paged_native_ok``, one page within 2 GiB, ``start`` (and ``counts``) contiguous int32 [B] on the device,
    everything 16-byte aligned."""
    if k_scale is not None or v_scale is not None or q.dim() != 4 or k_pages.dim() != 4:
        return False
    B, T, Hq, D = q.shape
    if not (q.is_cuda and k_pages.device == q.device):
        return False
    if not _paged_layout_ok(k_pages, v_pages, block_table, None, None, B):
        return False
    page, Hkv = k_pages.shape[1], k_pages.shape[2]
    if q.dtype != torch.bfloat16 or k_pages.shape[3] != D or D not in (64, 128):
        return False
    if B > 65535 or Hq > 65535 or Hq < 1 or Hq % Hkv != 0 or T > 2 ** 31 - 1 or not _extend_index_ok(q, start, counts):
        return False
    if (page - 1) * Hkv * D * 2 + 2 * D > _EXT_RANGE:
        return False
    return q.is_contiguous() and q.data_ptr() % 16 == 0


def extend_attention_paged(q: torch.Tensor, k_pages: torch.Tensor, v_pages: torch.Tensor, block_table: torch.Tensor,
                           start: torch.Tensor, counts: Optional[torch.Tensor] = None, scale: Optional[float] = None,
                           k_scale: Optional[torch.Tensor] = None,
                           v_scale: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``extend_attention`` against a paged KV cache: pools ``[P, page, Hkv, D]``, ``block_table`` int32 ``[B, C]``
    (``table[:, :c]`` of a wider table is fine), ``Smax = C * page``. Key ``n`` of sequence b is row ``n % page`` of
    page ``block_table[b, n // page]``; an entry outside ``[0, P)`` masks its keys and is never turned into an
    address. A 64-key tile of the kernel has one table entry, read once per tile. For equal operands the result has
    the bits of ``extend_attention`` on ``paged_gather`` of the pools.

    The paged gfx950 kernel runs when ``extend_paged_native_ok`` holds, ``extend_attention_paged_ref`` otherwise. FP8
    pools take the slow path: the pages the table names are gathered and dequantised into a bf16 scratch
    (``paged_gather``, ``kv_dequantize``), which the kernel reads as a pool of its own through a table that keeps
    the invalid entries invalid. Inference only."""
    _no_grad_inputs("extend_attention_paged", q, k_pages, v_pages)
    fp8 = _check_paged_args("extend_attention_paged", k_pages, v_pages, block_table, k_scale, v_scale)
    _check_extend_args("extend_attention_paged", q, block_table.shape[0], k_pages.shape[3], k_pages.shape[2], start,
                       counts)
    if fp8 and q.is_cuda and q.dtype == torch.bfloat16 and k_pages.device == q.device and block_table.is_cuda:
        P, page = k_pages.shape[0], k_pages.shape[1]
        B, C = block_table.shape
        with torch.no_grad():  # the slow path: row b's pages become pages b * C .. b * C + C - 1 of a bf16 scratch
            kd = kv_dequantize(paged_gather(k_pages, block_table), paged_gather(k_scale, block_table), torch.bfloat16)
            vd = kv_dequantize(paged_gather(v_pages, block_table), paged_gather(v_scale, block_table), torch.bfloat16)
            kd, vd = kd.view(B * C, page, *kd.shape[2:]), vd.view(B * C, page, *vd.shape[2:])
            own = torch.arange(B * C, dtype=torch.int32, device=q.device).view(B, C)
            table = torch.where((block_table >= 0) & (block_table < P), own, own.new_full((), -1))
        if extend_paged_native_ok(q, kd, vd, table, start, counts):
            return extend_attention_paged(q, kd, vd, table, start, counts, scale)
    if extend_paged_native_ok(q, k_pages, v_pages, block_table, start, counts, k_scale, v_scale):
        scale = 1.0 / math.sqrt(q.shape[-1]) if scale is None else scale
        with torch.no_grad():
            return native.C().attn_extend_paged(q, k_pages, v_pages, block_table, start, float(scale), counts)
    return extend_attention_paged_ref(q, k_pages, v_pages, block_table, start, counts, scale, k_scale, v_scale)
