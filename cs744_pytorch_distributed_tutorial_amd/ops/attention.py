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
