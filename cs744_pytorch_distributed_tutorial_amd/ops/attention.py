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
class KVCache:
    """The keys and values of every layer for B sequences of up to ``Smax`` positions, in the model's natural
    layout: ``k``, ``v`` ``[n_layers, B, Smax, Hkv, hd]`` (uninitialised past the lengths), ``lens`` int32 ``[B]``
    on the device, and ``bound``, a host-side upper bound of ``lens`` (the prompt length plus the steps
    taken) that sizes the slice a decode step attends over without reading ``lens`` back."""

    def __init__(self, k: torch.Tensor, v: torch.Tensor, lens: torch.Tensor, bound: int = 0):
        self.k, self.v, self.lens, self.bound = k, v, lens, bound

    @classmethod
    def allocate(cls, cfg, B: int, max_len: int, device=None, dtype=torch.bfloat16) -> "KVCache":
        """``cfg``: a ``LlamaConfig``. k and v come from ``torch.empty``: nothing past ``lens`` is ever read
        as a value."""
        if max_len < 1 or max_len > cfg.max_seq:
            raise ValueError(f"KVCache: max_len {max_len} outside [1, max_seq {cfg.max_seq}]")
        shape = (cfg.n_layers, B, max_len, cfg.n_kv_heads, cfg.dim // cfg.n_heads)
        return cls(torch.empty(shape, device=device, dtype=dtype), torch.empty(shape, device=device, dtype=dtype),
                   torch.zeros(B, dtype=torch.int32, device=device), 0)


def _no_grad_inputs(name: str, *ts) -> None:
    if any(t.requires_grad for t in ts):
        raise RuntimeError(f"{name} is inference only (no backward): detach the inputs or run the model "
                           "under torch.no_grad()")


def decode_attention_ref(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, lens: torch.Tensor,
                         scale: Optional[float] = None) -> torch.Tensor:
    """Decode attention in plain torch: q ``[B, Hq, D]`` against ``k_cache`` / ``v_cache`` ``[B, Smax, Hkv, D]``,
    row b seeing keys ``0 .. lens[b] - 1`` (``lens`` clamped into [0, Smax]) -> ``[B, Hq, D]`` in q's dtype.
    fp32 math (fp64 for fp64 inputs), GQA by head repetition. Keys past the length are removed with
    ``torch.where`` from both the scores and V, so whatever the cache holds there (NaN, Inf) cannot leak; a
    row with no visible key gives zeros. The CPU path and the fallback of ``decode_attention``."""
    _no_grad_inputs("decode_attention_ref", q, k_cache, v_cache)
    B, Hq, D = q.shape
    Smax, Hkv = k_cache.shape[1], k_cache.shape[2]
    rep = Hq // Hkv
    ct = torch.float64 if q.dtype == torch.float64 else torch.float32
    scale = 1.0 / math.sqrt(D) if scale is None else scale
    with torch.no_grad():
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


def decode_native_ok(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, lens: torch.Tensor) -> bool:
    """Whether the gfx950 kernel takes these operands: GPU, bf16, D in {64, 128}, Hq / Hkv in {1, 2, 4, 8},
    int32 contiguous ``lens``, q contiguous, the caches contiguous in their inner three dimensions with one
    batch stride that is a multiple of 8, everything 16-byte aligned."""
    if not (q.is_cuda and k_cache.is_cuda and v_cache.is_cuda and lens.is_cuda):
        return False
    if not (q.dtype == k_cache.dtype == v_cache.dtype == torch.bfloat16 and lens.dtype == torch.int32):
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
    return q.is_contiguous() and all(t.data_ptr() % 16 == 0 for t in (q, k_cache, v_cache))


def decode_attention(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, lens: torch.Tensor,
                     scale: Optional[float] = None, splits: Optional[int] = None) -> torch.Tensor:
    """One query row per head against a KV cache: q ``[B, Hq, D]``, caches ``[B, Smax, Hkv, D]`` (a ``[:, :n]``
    slice of a longer cache is fine), ``lens`` int32 ``[B]`` -> ``[B, Hq, D]``. Row b sees keys
    ``0 .. lens[b] - 1``; ``lens`` is clamped into [0, Smax] and a row of length 0 gives zeros. Stale cache
    rows past the length contribute exactly nothing.

    The gfx950 split-KV kernel runs when ``decode_native_ok`` holds, ``decode_attention_ref`` otherwise.
    ``splits``: the number of key slices per (sequence, kv head); ``None`` picks it from B, Hkv and Smax
    (``decode_splits``), any other value is clamped into [1, key tiles of Smax]. Inference only."""
    _no_grad_inputs("decode_attention", q, k_cache, v_cache)
    if decode_native_ok(q, k_cache, v_cache, lens):
        scale = 1.0 / math.sqrt(q.shape[-1]) if scale is None else scale
        with torch.no_grad():
            return native.C().attn_decode(q, k_cache, v_cache, lens, float(scale),
                                          0 if splits is None else max(int(splits), 1))
    return decode_attention_ref(q, k_cache, v_cache, lens, scale)


def decode_key_tile() -> int:
    """Keys a workgroup of the decode kernel reads per trip (slices are whole tiles)."""
    return native.C().decode_key_tile()


def decode_splits(B: int, Hkv: int, Smax: int) -> int:
    """The key splits the kernel picks for these shapes: from B, Hkv and Smax only, never from ``lens``."""
    return native.C().decode_splits(B, Hkv, Smax)
