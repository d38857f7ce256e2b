"""Decoder-only LM with the Llama-3 architecture (BASELINE.json config "Llama-3 8B
bf16 pure data-parallel grad all-reduce on 8xMI355X" — an extension; the
reference has no language model).

Pre-norm blocks: RMSNorm -> grouped-query attention with rotary position
embeddings (RoPE, theta 500000) -> residual -> RMSNorm -> SwiGLU MLP -> residual;
untied input embedding / output head. Pure data parallelism: every rank holds
the full replica (8.03 B parameters = 16 GB in bf16, fits the 288 GB HBM3E of one
MI355X with gradients and optimizer state), and the step's 16 GB of bf16
gradients is the xGMI all-reduce stress the config names.

Hot ops have hand-written gfx950 kernels used on the GPU: RMSNorm fwd/bwd, SwiGLU
fwd/bwd and RoPE in ``ops.lm``, and causal grouped-query flash attention (forward and a
deterministic backward, bf16, head dim 64/128) in ``ops.attention`` — called on the
[B, S, H, D] projections directly, no transposes. The projection GEMMs are plain library
GEMMs (hipBLASLt), run on bf16 copies of the fp32 master weights that the fused SGD pass
rewrites (``ops.lm.ShadowLinear``): no per-step weight casts, fp32 weight gradients straight out
of the GEMM. With ``LlamaConfig.qk_norm`` (opt-in) q and k get a per-head RMSNorm fused with their RoPE
(``ops.lm.qk_norm_rope``). With ``Llama.fused_residual`` (opt-in) every residual add after the first norm runs
inside the RMSNorm that follows it (``ops.lm.add_rms_norm``).

Inference: ``Llama.generate`` = ``prefill`` (the training blocks, k and v copied into an ``ops.attention.KVCache``)
plus one ``decode_step`` per token (split-KV decode attention, ``ops.attention.decode_attention``; docs/decode_attention.md).
``generate(..., kv_dtype="fp8")`` keeps the cache as e4m3fn codes with one fp32 scale per (token, kv head).
``Llama.extend`` runs T > 1 new tokens per row against a filled cache (``ops.attention.extend_attention``;
docs/extend_attention.md): a second turn on a live cache, several proposed tokens verified in one pass, and
``prefill(..., chunk=n)`` / ``generate(..., prefill_chunk=n)``, the prompt fed n tokens at a time.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, replace

import torch
import torch.nn as nn
import torch.nn.functional as F


@dataclass
class LlamaConfig:
    dim: int = 4096
    n_layers: int = 32
    n_heads: int = 32
    n_kv_heads: int = 8
    ffn_dim: int = 14336
    vocab_size: int = 128256
    max_seq: int = 8192
    rope_theta: float = 500000.0
    norm_eps: float = 1e-5
    eos_id: int = 128001  # <|end_of_text|> of the Llama-3 vocabulary: closes a document of a packed row
    # opt-in QK-norm (Qwen3 / Gemma 3): a per-head RMSNorm of q and k with a learned [head_dim] gain each,
    # applied before RoPE (ops.lm.qk_norm_rope); adds attention.q_norm / k_norm to every layer
    qk_norm: bool = False


CONFIGS = {
    "llama3-8b": LlamaConfig(),
    "llama3-1b": LlamaConfig(dim=2048, n_layers=16, n_heads=32, n_kv_heads=8, ffn_dim=8192, max_seq=2048),
    "llama-tiny": LlamaConfig(dim=256, n_layers=2, n_heads=4, n_kv_heads=2, ffn_dim=512, vocab_size=1024,
                              max_seq=128, eos_id=1023),
}


def _ops():
    from ..ops import lm
    return lm


def _Linear(*args, **kwargs) -> nn.Linear:
    """bias-free projection: ``ops.lm.ShadowLinear`` (nn.Linear with a bf16 weight copy kept in step
    with the fp32 master by the fused optimizer)"""
    from ..ops.lm import ShadowLinear
    return ShadowLinear(*args, **kwargs)


class RMSNorm(nn.Module):
    def __init__(self, dim: int, eps: float = 1e-5):
        super().__init__()
        self.eps = eps
        self.weight = nn.Parameter(torch.ones(dim))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return _ops().rms_norm(x, self.weight, self.eps)

    def add(self, x: torch.Tensor, delta: torch.Tensor) -> tuple:
        """``(h, self(h))`` with ``h = x + delta``: the residual add fused into this norm"""
        return _ops().add_rms_norm(x, delta, self.weight, self.eps)


def rope_tables(seq: int, head_dim: int, theta: float, device) -> tuple:
    inv = 1.0 / (theta ** (torch.arange(0, head_dim, 2, device=device, dtype=torch.float32) / head_dim))
    ang = torch.outer(torch.arange(seq, device=device, dtype=torch.float32), inv)
    return ang.cos(), ang.sin()


class Attention(nn.Module):
    def __init__(self, cfg: LlamaConfig):
        super().__init__()
        self.nh, self.nkv = cfg.n_heads, cfg.n_kv_heads
        self.hd = cfg.dim // cfg.n_heads
        self.wq = _Linear(cfg.dim, self.nh * self.hd, bias=False)
        self.wk = _Linear(cfg.dim, self.nkv * self.hd, bias=False)
        self.wv = _Linear(cfg.dim, self.nkv * self.hd, bias=False)
        self.wo = _Linear(self.nh * self.hd, cfg.dim, bias=False)
        self.qk_norm = cfg.qk_norm
        if self.qk_norm:
            self.q_norm = RMSNorm(self.hd, cfg.norm_eps)
            self.k_norm = RMSNorm(self.hd, cfg.norm_eps)

    def _qkv(self, x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor) -> tuple:
        """The projections of ``x`` [B, S, dim] as [B, S, H, hd], q and k after (QK-norm and) RoPE with the
        table rows ``cos`` / ``sin`` [S, hd/2]: row s of the tables belongs to position s of the S axis."""
        B, S, _ = x.shape
        q = self.wq(x).view(B, S, self.nh, self.hd)
        k = self.wk(x).view(B, S, self.nkv, self.hd)
        v = self.wv(x).view(B, S, self.nkv, self.hd)
        if self.qk_norm:
            q, k = _ops().qk_norm_rope(q, k, self.q_norm.weight, self.k_norm.weight, cos, sin, self.q_norm.eps)
        else:
            q, k = _ops().rope(q, cos, sin), _ops().rope(k, cos, sin)
        return q, k, v

    def forward(self, x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, doc=None, kv_out=None) -> torch.Tensor:
        """``doc``: ``ops.attention.DocBounds`` of a packed batch (attention stays inside a document).
        ``kv_out``: a pair of cache tensors [B, Smax >= S, Hkv, hd] (``Llama.prefill``); the post-RoPE k and v
        are copied into their first S positions. With the scales of an FP8 cache appended, ``(k_cache, v_cache,
        k_scale, v_scale)``, they are quantised into them (``ops.attention.kv_cache_append``). An
        ``ops.attention.PagedLayer`` (a layer of a ``PagedKVCache``) takes them through its block table, the first
        ``counts[b]`` tokens of row b (``ops.attention.kv_cache_append_paged``)."""
        B, S, _ = x.shape
        q, k, v = self._qkv(x, cos, sin)
        from ..ops.attention import PagedLayer
        if isinstance(kv_out, PagedLayer):
            from ..ops.attention import kv_cache_append_paged
            kv_cache_append_paged(kv_out.k, kv_out.v, kv_out.block_table, k, v, counts=kv_out.counts,
                                  k_scale=kv_out.k_scale, v_scale=kv_out.v_scale)
        elif kv_out is not None and len(kv_out) == 4:
            from ..ops.attention import kv_cache_append
            kv_cache_append(*kv_out, k, v)
        elif kv_out is not None:
            kv_out[0][:, :S].copy_(k)
            kv_out[1][:, :S].copy_(v)
        from ..ops.attention import attention, attention_ref, native_ok
        if native_ok(q, k, v):
            o = attention(q, k, v, causal=True, doc=doc)  # [B, S, Hq, hd], gfx950 flash attention
        elif doc is not None:  # CPU / fp32 with a document mask: the math reference (masked weights exactly 0)
            o = attention_ref(q, k, v, True, doc)
        else:  # CPU / fp32: PyTorch's attention
            q, k, v = q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2)
            o = F.scaled_dot_product_attention(q, k, v, is_causal=True, enable_gqa=self.nkv != self.nh).transpose(1, 2)
        return self.wo(o.reshape(B, S, self.nh * self.hd))

    def decode(self, x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, kc: torch.Tensor, vc: torch.Tensor,
               slot: torch.Tensor, lens: torch.Tensor, bound: int, k_scale: torch.Tensor = None,
               v_scale: torch.Tensor = None, pos: torch.Tensor = None) -> torch.Tensor:
        """One new token per row against the cache. ``x``: [B, 1, dim]; ``cos`` / ``sin``: [B, hd/2], the table
        rows of every row's own position; ``kc`` / ``vc``: this layer's caches [B, Smax, Hkv, hd]; ``slot``:
        int64 [B], ``b * Smax + position`` where the new k and v rows go; ``lens``: int32 [B], the lengths
        with the new token counted; ``bound``: a host-known upper bound of ``lens``. An FP8 cache comes with
        this layer's scales ``k_scale`` / ``v_scale`` [B, Smax, Hkv] and ``pos`` int32 [B], the positions
        themselves: the new rows are then quantised into the cache by one ``kv_cache_append``."""
        B = x.shape[0]
        # [B, 1, H, hd] read as [1, B, H, hd]: the batch stands in the sequence axis of the RoPE ops, so
        # row b is rotated by table row b
        q, k, v = self._qkv(x.reshape(1, B, -1), cos, sin)
        from ..ops.attention import decode_attention, kv_cache_append
        if k_scale is not None:
            kv_cache_append(kc, vc, k_scale, v_scale, k.view(B, 1, self.nkv, self.hd), v.view(B, 1, self.nkv, self.hd),
                            pos)
            o = decode_attention(q.view(B, self.nh, self.hd), kc[:, :bound], vc[:, :bound], lens,
                                 k_scale=k_scale[:, :bound], v_scale=v_scale[:, :bound])
            return self.wo(o.reshape(B, 1, self.nh * self.hd))
        kc.view(-1, self.nkv, self.hd).index_copy_(0, slot, k.view(B, self.nkv, self.hd).to(kc.dtype))
        vc.view(-1, self.nkv, self.hd).index_copy_(0, slot, v.view(B, self.nkv, self.hd).to(vc.dtype))
        o = decode_attention(q.view(B, self.nh, self.hd), kc[:, :bound], vc[:, :bound], lens)
        return self.wo(o.reshape(B, 1, self.nh * self.hd))


    def decode_paged(self, x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, layer, pos: torch.Tensor,
                     lens: torch.Tensor) -> torch.Tensor:
        """``decode`` against one layer of a ``PagedKVCache`` (``ops.attention.PagedLayer``, its table cut to the
        columns the lengths can reach): one paged append of the new rows at ``pos`` int32 [B], then paged decode
        attention up to ``lens`` int32 [B]."""
        B = x.shape[0]
        q, k, v = self._qkv(x.reshape(1, B, -1), cos, sin)
        from ..ops.attention import decode_attention_paged, kv_cache_append_paged
        kv_cache_append_paged(layer.k, layer.v, layer.block_table, k.view(B, 1, self.nkv, self.hd),
                              v.view(B, 1, self.nkv, self.hd), pos, k_scale=layer.k_scale, v_scale=layer.v_scale)
        o = decode_attention_paged(q.view(B, self.nh, self.hd), layer.k, layer.v, layer.block_table, lens,
                                   k_scale=layer.k_scale, v_scale=layer.v_scale)
        return self.wo(o.reshape(B, 1, self.nh * self.hd))

    def extend(self, x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, start: torch.Tensor, counts, kc=None,
               vc=None, slot=None, bound: int = 0, k_scale=None, v_scale=None, layer=None) -> torch.Tensor:
        """T new tokens per row against the cache: append, then attend. ``x``: [B, T, dim]; ``cos`` / ``sin``:
        [B * T, hd/2], the table rows of every token's own position ``start[b] + s``; ``start``: int32 [B], the
        rows' lengths before these tokens; ``counts``: int32 [B] or None (all T), their real new tokens. Either
        ``layer`` (an ``ops.attention.PagedLayer``: one paged append at ``start`` that drops the padding, then
        ``extend_attention_paged``), or this layer's slab ``kc`` / ``vc`` [B, Smax, Hkv, hd] with ``bound``, a host
        upper bound of the new lengths with ``bound <= Smax`` (the caller's check, so a padded token lands on a
        stale position past its row's new length, never on live data): an FP8 slab comes with its scales and
        takes one ``kv_cache_append`` at ``start``, any other one a device index copy to ``slot`` int64 [B * T]."""
        B, T, _ = x.shape
        # [B, T, H, hd] read as [1, B * T, H, hd]: token (b, s) is rotated by table row b * T + s
        q, k, v = self._qkv(x.reshape(1, B * T, -1), cos, sin)
        q, k, v = q.view(B, T, self.nh, self.hd), k.view(B, T, self.nkv, self.hd), v.view(B, T, self.nkv, self.hd)
        from ..ops.attention import extend_attention, extend_attention_paged, kv_cache_append, kv_cache_append_paged
        if layer is not None:
            kv_cache_append_paged(layer.k, layer.v, layer.block_table, k, v, start, counts, k_scale=layer.k_scale,
                                  v_scale=layer.v_scale)
            o = extend_attention_paged(q, layer.k, layer.v, layer.block_table, start, counts, k_scale=layer.k_scale,
                                       v_scale=layer.v_scale)
        elif k_scale is not None:
            kv_cache_append(kc, vc, k_scale, v_scale, k, v, start)
            o = extend_attention(q, kc[:, :bound], vc[:, :bound], start, counts, k_scale=k_scale[:, :bound],
                                 v_scale=v_scale[:, :bound])
        else:
            kc.view(-1, self.nkv, self.hd).index_copy_(0, slot, k.reshape(B * T, self.nkv, self.hd).to(kc.dtype))
            vc.view(-1, self.nkv, self.hd).index_copy_(0, slot, v.reshape(B * T, self.nkv, self.hd).to(vc.dtype))
            o = extend_attention(q, kc[:, :bound], vc[:, :bound], start, counts)
        return self.wo(o.reshape(B, T, self.nh * self.hd))


class FeedForward(nn.Module):
    def __init__(self, cfg: LlamaConfig):
        super().__init__()
        self.w1 = _Linear(cfg.dim, cfg.ffn_dim, bias=False)  # gate
        self.w3 = _Linear(cfg.dim, cfg.ffn_dim, bias=False)  # up
        self.w2 = _Linear(cfg.ffn_dim, cfg.dim, bias=False)  # down

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return self.w2(_ops().swiglu(self.w1(x), self.w3(x)))


class Block(nn.Module):
    def __init__(self, cfg: LlamaConfig):
        super().__init__()
        self.attention_norm = RMSNorm(cfg.dim, cfg.norm_eps)
        self.attention = Attention(cfg)
        self.ffn_norm = RMSNorm(cfg.dim, cfg.norm_eps)
        self.feed_forward = FeedForward(cfg)

    def forward(self, x, cos, sin, doc=None):
        x = x + self.attention(self.attention_norm(x), cos, sin, doc)
        return x + self.feed_forward(self.ffn_norm(x))

    def forward_fused(self, h, y, next_norm: RMSNorm, cos, sin, doc=None) -> tuple:
        """The same block with each residual add fused into the norm that follows it
        (``ops.lm.add_rms_norm``). ``h``: the stream entering the block, ``y``: its ``attention_norm``,
        already computed (by the previous block, or plainly for the first one); ``next_norm``: the norm
        that reads this block's output, the next block's ``attention_norm`` or the model's final norm.
        Returns the stream leaving the block and its ``next_norm``."""
        h, y = self.ffn_norm.add(h, self.attention(y, cos, sin, doc))
        return next_norm.add(h, self.feed_forward(y))


class Llama(nn.Module):
    def __init__(self, cfg: LlamaConfig):
        super().__init__()
        self.cfg = cfg
        self.vocab_size, self.max_seq = cfg.vocab_size, cfg.max_seq
        self.tok_embeddings = nn.Embedding(cfg.vocab_size, cfg.dim)
        self.layers = nn.ModuleList(Block(cfg) for _ in range(cfg.n_layers))
        self.norm = RMSNorm(cfg.dim, cfg.norm_eps)
        self.output = _Linear(cfg.dim, cfg.vocab_size, bias=False)
        std = 0.02
        for m in self.modules():
            if isinstance(m, nn.Linear):
                nn.init.normal_(m.weight, 0.0, std)
            elif isinstance(m, nn.Embedding):
                nn.init.normal_(m.weight, 0.0, std)
        for blk in self.layers:  # scaled residual projections
            nn.init.normal_(blk.attention.wo.weight, 0.0, std / math.sqrt(2 * cfg.n_layers))
            nn.init.normal_(blk.feed_forward.w2.weight, 0.0, std / math.sqrt(2 * cfg.n_layers))
        self._rope = None
        # opt-in: fuse every residual add into the RMSNorm that follows it (ops.lm.add_rms_norm);
        # same parameters and state_dict, same results (TorchTrainer(fused_residual=True) sets it)
        self.fused_residual = False

    def _tables(self, S: int, device):
        if self._rope is None or self._rope[0].shape[0] < S or self._rope[0].device != device:
            self._rope = rope_tables(max(S, 1), self.cfg.dim // self.cfg.n_heads, self.cfg.rope_theta, device)
        return self._rope[0][:S], self._rope[1][:S]

    def forward(self, tokens: torch.Tensor, doc_ids: torch.Tensor = None, targets: torch.Tensor = None,
                ignore_index=None, z_loss: float = 0.0) -> torch.Tensor:
        """``doc_ids``: integer [B, S], the document of every token of a packed batch
        (``ops.attention.doc_ids_from_eos``); attention is then confined to a token's own document.
        RoPE positions are NOT reset per document: a RoPE score depends only on ``i - j``, so inside
        a document the result is the same as with positions counted from the document's start.

        Without ``targets`` the logits [B, S, V] are returned. With ``targets`` (int64 [B, S]) the
        result is the loss ``ops.lm.cross_entropy(logits, targets, ignore_index, z_loss)`` computed by
        ``ops.lm.linear_cross_entropy`` over row chunks: the logits are never built whole."""
        h = self.hidden(tokens, doc_ids)
        if targets is None:
            return self.output(h)
        return _ops().linear_cross_entropy(h, self.output, targets, ignore_index=ignore_index, z_loss=z_loss)

    def hidden(self, tokens: torch.Tensor, doc_ids: torch.Tensor = None) -> torch.Tensor:
        """The final-norm hidden states [B, S, D] that the output head reads."""
        S = tokens.shape[1]
        cos, sin = self._tables(S, tokens.device)
        h = self.tok_embeddings(tokens)
        if self.fused_residual and len(self.layers) > 0:
            doc = None
            if doc_ids is not None:
                from ..ops.attention import doc_bounds
                doc = doc_bounds(doc_ids)
            # the first norm is a plain one; every residual add after it runs inside the norm that
            # follows it (2 * n_layers fused sites), the last inside the final norm
            y = self.layers[0].attention_norm(h)
            norms = [blk.attention_norm for blk in self.layers[1:]] + [self.norm]
            for blk, nxt in zip(self.layers, norms):
                h, y = blk.forward_fused(h, y, nxt, cos, sin, doc)
            return y
        if doc_ids is None:
            for blk in self.layers:
                h = blk(h, cos, sin)
        else:
            from ..ops.attention import doc_bounds
            doc = doc_bounds(doc_ids)  # once per forward, shared by every layer
            for blk in self.layers:
                h = blk(h, cos, sin, doc)
        return self.norm(h)

    # ------------------------------------------------------------------ inference with a KV cache
    def cache_dtype(self, device) -> torch.dtype:
        """The dtype the projections come out in on ``device``: the autocast dtype under GPU autocast,
        the parameters' dtype otherwise."""
        if torch.device(device).type == "cuda" and torch.is_autocast_enabled("cuda"):
            return torch.get_autocast_dtype("cuda")
        return self.tok_embeddings.weight.dtype

    @torch.no_grad()
    def prefill(self, tokens: torch.Tensor, cache, prompt_lens=None, doc_ids=None, chunk=None) -> torch.Tensor:
        """Run the prompt through the model and fill ``cache`` (``ops.attention.KVCache``): the logits
        [B, V] of each row's last prompt token. ``tokens``: [B, S], right-padded; ``prompt_lens``: int [B],
        every value in [1, S] (default: all S). The blocks run with causal flash attention, which already
        keeps the padding out of the real positions; each layer's post-RoPE k and v go to ``cache[:, :S]``,
        ``cache.lens`` becomes ``prompt_lens``, and the final norm and the head run on the B last rows only.
        Packed documents (``doc_ids``) have no cached form and are refused.

        With an ``ops.attention.PagedKVCache`` the lengths are read to the host once, before the layers (the only
        read-back; none when ``prompt_lens`` is a list or a host tensor), every row's slot is grown to its own
        length and the table committed; each layer's k and v then go through the table, the first ``lens[b]``
        tokens of row b only, so the padding takes no pages. The prompt's attention runs on the fresh projections
        as before.

        ``chunk=n`` feeds the prompt as ``ceil(S / n)`` ``extend`` calls of at most n tokens from an empty cache
        (whatever ``cache`` held is forgotten), with per-row counts cut from ``prompt_lens``: the activations, the
        attention's working set and the head's inputs scale with n, only the cache with S. The same logits and
        the same cache contents as the one-shot call, up to summation order. For a paged cache each chunk's pages
        are reserved and committed before the chunk runs, so the pool grows chunk by chunk."""
        if doc_ids is not None:
            raise ValueError("prefill: a document mask (doc_ids) cannot be combined with a KV cache")
        if tokens.dim() != 2:
            raise ValueError("prefill: tokens must be [B, S]")
        if chunk is not None:
            return self._prefill_chunked(tokens, cache, prompt_lens, int(chunk))
        from ..ops.attention import PagedKVCache
        if isinstance(cache, PagedKVCache):
            return self._prefill_paged(tokens, cache, prompt_lens)
        B, S = tokens.shape
        if cache.k.shape[0] != len(self.layers) or cache.k.shape[1] != B or cache.k.shape[2] < S or S < 1:
            raise ValueError(f"prefill: the cache {tuple(cache.k.shape)} does not hold {len(self.layers)} layers of "
                             f"[{B}, {S}] tokens")
        dev = tokens.device
        if prompt_lens is None:
            lens = torch.full((B,), S, dtype=torch.int32, device=dev)
        else:
            lens = torch.as_tensor(prompt_lens).to(device=dev, dtype=torch.int32).reshape(B).clamp(0, S)
        self._tables(cache.k.shape[2], dev)  # once, at the cache's length: decode_step gathers from them
        cos, sin = self._tables(S, dev)
        h = self.tok_embeddings(tokens)
        fp8 = cache.k_scale is not None
        for l, blk in enumerate(self.layers):
            kv_out = (cache.k[l], cache.v[l]) + ((cache.k_scale[l], cache.v_scale[l]) if fp8 else ())
            h = h + blk.attention(blk.attention_norm(h), cos, sin, kv_out=kv_out)
            h = h + blk.feed_forward(blk.ffn_norm(h))
        last = (lens.long() - 1).clamp(min=0)
        h = h[torch.arange(B, device=dev), last].unsqueeze(1)  # [B, 1, dim], gathered on the device
        cache.lens, cache.bound = lens, S
        return self.output(self.norm(h)).squeeze(1)

    def _prefill_paged(self, tokens: torch.Tensor, cache, prompt_lens) -> torch.Tensor:
        B, S = tokens.shape
        if cache.k.shape[0] != len(self.layers) or cache.block_table.shape[0] != B or S < 1 or S > cache.max_len:
            raise ValueError(f"prefill: a paged cache of {cache.k.shape[0]} layers, {cache.block_table.shape[0]} slots "
                             f"and {cache.max_len} positions does not hold {len(self.layers)} layers of [{B}, {S}] "
                             "tokens")
        dev = tokens.device
        host = [S] * B if prompt_lens is None else torch.as_tensor(prompt_lens).reshape(B).tolist()
        host = [min(max(int(n), 0), S) for n in host]
        for b, n in enumerate(host):
            cache.reserve(b, n)
        cache.commit()
        lens = torch.tensor(host, dtype=torch.int32).to(dev)
        self._tables(cache.max_len, dev)  # once, at the table's reach: decode_step gathers from them
        cos, sin = self._tables(S, dev)
        h = self.tok_embeddings(tokens)
        for l, blk in enumerate(self.layers):
            h = h + blk.attention(blk.attention_norm(h), cos, sin, kv_out=cache.layer(l, counts=lens))
            h = h + blk.feed_forward(blk.ffn_norm(h))
        last = (lens.long() - 1).clamp(min=0)
        h = h[torch.arange(B, device=dev), last].unsqueeze(1)
        cache.lens, cache.bound, cache.row_bound = lens, max(host), list(host)
        return self.output(self.norm(h)).squeeze(1)

    def _prefill_chunked(self, tokens: torch.Tensor, cache, prompt_lens, chunk: int) -> torch.Tensor:
        from ..ops.attention import PagedKVCache
        B, S = tokens.shape
        paged = isinstance(cache, PagedKVCache)
        if chunk < 1:
            raise ValueError(f"prefill: chunk must be at least 1, got {chunk}")
        slots, room = (cache.block_table.shape[0], cache.max_len) if paged else (cache.k.shape[1], cache.k.shape[2])
        if cache.k.shape[0] != len(self.layers) or slots != B or S < 1 or S > room:
            raise ValueError(f"prefill: a cache of {cache.k.shape[0]} layers, {slots} sequences and {room} positions "
                             f"does not hold {len(self.layers)} layers of [{B}, {S}] tokens")
        dev = tokens.device
        host = lens = None
        if paged:  # the allocator needs the lengths on the host: read once, as in the one-shot paged prefill
            host = [S] * B if prompt_lens is None else torch.as_tensor(prompt_lens).reshape(B).tolist()
            host = [min(max(int(n), 0), S) for n in host]
            cache.row_bound = [0] * B
        elif prompt_lens is not None:
            lens = torch.as_tensor(prompt_lens).to(device=dev, dtype=torch.int32).reshape(B).clamp(0, S)
        cache.lens, cache.bound = torch.zeros(B, dtype=torch.int32, device=dev), 0
        logits = None
        for c0 in range(0, S, chunk):
            n = min(chunk, S - c0)
            if paged:
                for b, m in enumerate(host):
                    cache.reserve(b, min(m, c0 + n))
                cache.commit()
                counts = [min(max(m - c0, 0), n) for m in host]
                took = torch.tensor([m > 0 for m in counts]).to(dev)
            elif lens is None:
                counts, took = None, None
            else:
                counts = (lens - c0).clamp(0, n)  # on the device: no read-back
                took = counts > 0
            lg = self.extend(tokens[:, c0:c0 + n], cache, counts)
            # a row's logits are those of the last chunk that held one of its tokens
            logits = lg if logits is None or took is None else torch.where(took.view(B, 1), lg, logits)
        return logits

    @torch.no_grad()
    def extend(self, tokens: torch.Tensor, cache, counts=None, all_logits: bool = False) -> torch.Tensor:
        """Run T more tokens per row on a cache that ``prefill``, ``decode_step`` or an earlier ``extend`` filled (an
        empty one is fine): ``tokens`` [B, T] right-padded, ``counts`` int [B] the real tokens of every row (default
        all T; clamped into [0, T]). Row b's tokens take the positions ``cache.lens[b] ..``; each layer appends their
        k and v and runs ``ops.attention.extend_attention`` (``_paged``) over the cache. Returns the logits [B, V] of
        each row's last real new token, or [B, T, V] with ``all_logits``. A row with ``counts[b] == 0`` keeps its
        length; its logits are unspecified but finite.

        ``cache.lens += counts`` (a device op), ``cache.bound += T``; a paged cache's ``row_bound[b]`` grows by
        ``counts[b]`` when the counts are known on the host (``None``, a list, a host tensor: nothing is read back)
        and by T when they are a device tensor. A contiguous cache raises ``ValueError`` when ``bound + T`` exceeds
        its positions. A paged cache is checked per slot on the host against the pages it holds (``ValueError``
        naming ``reserve``): nothing is allocated behind the caller's back. Packed documents have no cached form."""
        from ..ops.attention import PagedKVCache
        if tokens.dim() != 2 or tokens.shape[1] < 1:
            raise ValueError("extend: tokens must be [B, T] with T >= 1")
        B, T = tokens.shape
        dev = tokens.device
        paged = isinstance(cache, PagedKVCache)
        slots = cache.block_table.shape[0] if paged else cache.k.shape[1]
        if cache.k.shape[0] != len(self.layers) or slots != B:
            raise ValueError(f"extend: a cache of {cache.k.shape[0]} layers and {slots} sequences does not take "
                             f"{len(self.layers)} layers of [{B}, {T}] tokens")
        host = cnt = None
        if counts is None:
            host = [T] * B
        elif isinstance(counts, torch.Tensor) and counts.device.type != "cpu":
            cnt = counts.to(device=dev, dtype=torch.int32).reshape(B).clamp(0, T)
        else:
            host = [min(max(int(n), 0), T) for n in torch.as_tensor(counts).reshape(B).tolist()]
            cnt = torch.tensor(host, dtype=torch.int32).to(dev)
        start = cache.lens  # int32 [B]
        bound = cache.bound + T
        if paged:
            grow = host if host is not None else [T] * B
            for b in range(B):  # host only; never allocates behind the caller's back
                if cache.capacity(b) < cache.row_bound[b] + grow[b]:
                    raise ValueError(f"extend: slot {b} holds {cache.capacity(b)} positions and needs "
                                     f"{cache.row_bound[b] + grow[b]}: call cache.reserve({b}, n) and cache.commit() "
                                     "first")
            reach = cache.max_len
            cols = min(-(-bound // cache.page_size), cache.block_table.shape[1])
        else:
            reach = cache.k.shape[2]
            if bound > reach:
                raise ValueError(f"extend: {cache.bound} positions in use and {T} new tokens exceed the cache's "
                                 f"{reach} positions")
        cos, sin = self._tables(reach, dev)
        pos = (start.long().view(B, 1) + torch.arange(T, device=dev).view(1, T)).clamp(0, reach - 1)  # [B, T]
        cos, sin = cos[pos.reshape(-1)], sin[pos.reshape(-1)]
        fp8 = cache.k_scale is not None
        slot = None
        if not paged and not fp8:
            slot = (torch.arange(B, device=dev).view(B, 1) * reach + pos).reshape(-1)
        h = self.tok_embeddings(tokens)
        for l, blk in enumerate(self.layers):
            if paged:
                kw = dict(layer=cache.layer(l, cols=cols))
            elif fp8:
                kw = dict(kc=cache.k[l], vc=cache.v[l], bound=bound, k_scale=cache.k_scale[l], v_scale=cache.v_scale[l])
            else:
                kw = dict(kc=cache.k[l], vc=cache.v[l], bound=bound, slot=slot)
            h = h + blk.attention.extend(blk.attention_norm(h), cos, sin, start, cnt, **kw)
            h = h + blk.feed_forward(blk.ffn_norm(h))
        cache.lens = (start + T if cnt is None else start + cnt).clamp(max=reach)
        cache.bound = bound
        if paged:
            cache.row_bound = [n + g for n, g in zip(cache.row_bound, grow)]
        if all_logits:
            return self.output(self.norm(h))
        if cnt is None:
            return self.output(self.norm(h[:, -1:])).squeeze(1)
        last = (cnt.long() - 1).clamp(min=0)
        h = h[torch.arange(B, device=dev), last].unsqueeze(1)  # [B, 1, dim], gathered on the device
        return self.output(self.norm(h)).squeeze(1)

    def _decode_step_paged(self, tok: torch.Tensor, cache) -> torch.Tensor:
        B = tok.shape[0]
        for b in range(B):  # host only; a step never allocates behind the caller's back
            if cache.capacity(b) < cache.row_bound[b] + 1:
                raise ValueError(f"decode_step: slot {b} holds {cache.capacity(b)} positions and needs "
                                 f"{cache.row_bound[b] + 1}: call cache.reserve({b}, n) and cache.commit() first")
        dev = tok.device
        cos, sin = self._tables(cache.max_len, dev)
        pos = cache.lens  # int32 [B]; a position outside the slot's pages is dropped by the append
        rope = pos.long().clamp(0, cache.max_len - 1)
        cos, sin = cos[rope], sin[rope]
        lens = pos + 1
        bound = cache.bound + 1
        cols = -(-bound // cache.page_size)
        h = self.tok_embeddings(tok.view(B, 1))
        for l, blk in enumerate(self.layers):
            h = h + blk.attention.decode_paged(blk.attention_norm(h), cos, sin, cache.layer(l, cols=cols), pos, lens)
            h = h + blk.feed_forward(blk.ffn_norm(h))
        cache.lens, cache.bound = lens, bound
        cache.row_bound = [n + 1 for n in cache.row_bound]
        return self.output(self.norm(h)).squeeze(1)

    @torch.no_grad()
    def decode_step(self, tok: torch.Tensor, cache) -> torch.Tensor:
        """Append one token per row and return the logits [B, V] of the next one. Row b's position is
        ``cache.lens[b]``, so rows may differ; every row must still have room (``lens[b] < Smax``: a full
        row's write is clamped onto its last position). Nothing is read back from the device: the RoPE
        table rows are gathered by position, the new k and v rows are scattered by a device index (an FP8
        cache: quantised and stored by one kernel that takes the positions), and the attention runs over
        ``cache[:, :bound]`` with ``bound`` the host-known prompt length plus steps.

        With an ``ops.attention.PagedKVCache``: a host-only check that every slot's pages hold its own host bound
        plus one (``ValueError`` naming ``reserve`` otherwise), one paged append at the lengths, and paged decode
        attention over ``block_table[:, :ceil(bound / page)]``. No read-back and no table traffic in a step."""
        from ..ops.attention import PagedKVCache
        if isinstance(cache, PagedKVCache):
            return self._decode_step_paged(tok, cache)
        B = tok.shape[0]
        Smax = cache.k.shape[2]
        if cache.bound >= Smax:
            raise ValueError(f"decode_step: the cache of {Smax} positions is full")
        dev = tok.device
        cos, sin = self._tables(Smax, dev)
        pos = cache.lens.long().clamp(max=Smax - 1)
        cos, sin = cos[pos], sin[pos]
        slot = torch.arange(B, device=dev) * Smax + pos
        lens = (pos + 1).int()
        bound = cache.bound + 1
        h = self.tok_embeddings(tok.view(B, 1))
        fp8 = cache.k_scale is not None
        pos32 = pos.int() if fp8 else None
        for l, blk in enumerate(self.layers):
            scales = dict(k_scale=cache.k_scale[l], v_scale=cache.v_scale[l], pos=pos32) if fp8 else {}
            h = h + blk.attention.decode(blk.attention_norm(h), cos, sin, cache.k[l], cache.v[l], slot, lens, bound,
                                         **scales)
            h = h + blk.feed_forward(blk.ffn_norm(h))
        cache.lens, cache.bound = lens, bound
        return self.output(self.norm(h)).squeeze(1)

    @torch.no_grad()
    def generate(self, tokens: torch.Tensor, max_new_tokens: int, prompt_lens=None, temperature: float = 0.0,
                 top_k=None, eos_id=None, generator=None, kv_dtype=None, page_size=None, kv_pool=None,
                 prefill_chunk=None, top_p=None, min_p=None, sampler=None) -> torch.Tensor:
        """``int64 [B, max_new_tokens]``: the continuation of every row of ``tokens`` [B, S] (right-padded,
        ``prompt_lens`` int [B]), one ``prefill`` and then one ``decode_step`` per token. ``temperature == 0``
        is greedy argmax; otherwise a token is drawn (``torch.multinomial`` with ``generator``) from
        ``softmax(logits / temperature)``, restricted to the ``top_k`` largest logits when given. A row that
        has emitted ``eos_id`` keeps emitting it (a device-side mask: no early exit, no synchronisation).

        ``top_p`` (nucleus, 0 < p <= 1), ``min_p`` (0 <= p <= 1), a tensor [B] as ``temperature`` or ``top_k`` (per-row
        settings; a row at temperature 0 is greedy) or ``sampler="fused"`` select the fused sampler instead:
        ``ops.lm.sample_logits``, one launch per step on the GPU. Its filters run top-k, min-p, top-p in that order;
        tokens tied at the k-th value or at the nucleus cut are all kept; the token is drawn by inverse CDF in
        vocabulary order at one ``u = torch.rand(B, generator=generator)`` per step, so ``generator`` (on the tokens'
        device) fixes the tokens, though not to the ones ``torch.multinomial`` would give for the same seed. With none
        of these arguments the path is the one above, unchanged.
        ``kv_dtype``: the cache's dtype; ``None`` is ``cache_dtype``, ``"fp8"`` or ``torch.float8_e4m3fn`` an FP8
        cache (e4m3fn codes and one fp32 scale per token and kv head: about half the bytes of bf16).

        ``page_size``: an int builds a private ``PagedKVCache`` of exactly ``sum_b ceil((len_b + max_new_tokens) /
        page_size)`` pages instead of the ``[B, S + max_new_tokens]`` slab. ``kv_pool``: a caller's
        ``PagedKVCache`` with B slots, all free; ``len_b + max_new_tokens`` positions are reserved per row up front
        (``RuntimeError`` when the pool cannot cover them) and the rows are freed before returning, also on an
        exception; the pool's dtype is the cache's, and ``kv_dtype`` must be ``None`` or agree with it. With
        neither argument the contiguous cache is used as before.

        ``prefill_chunk=n`` feeds the prompt n tokens at a time (``prefill(..., chunk=n)``): the same tokens up to
        summation order, with activations sized by n instead of S. Default: the one-shot prefill, as before.

        Continuing a sequence (a second turn) needs the cache, so it is written with the pieces of this method::

            cache = KVCache.allocate(model.cfg, B, max_len, device, model.cache_dtype(device))
            logits = model.prefill(prompt, cache, prompt_lens)
            answer = model.decode_loop(logits, cache, n_new)          # [B, n_new]
            # decode_loop never feeds its last sampled token: it is not in the cache yet
            turn = torch.cat([answer[:, -1:], next_user_tokens], 1)   # [B, 1 + T2], right-padded
            logits = model.extend(turn, cache, counts=1 + next_lens)  # one pass over the new turn
            answer2 = model.decode_loop(logits, cache, n_new)"""
        from ..ops.attention import KVCache, PagedKVCache
        B, S = tokens.shape
        if max_new_tokens < 0 or S + max_new_tokens > self.cfg.max_seq:
            raise ValueError(f"generate: {S} prompt + {max_new_tokens} new tokens exceed max_seq {self.cfg.max_seq}")
        if (not isinstance(temperature, torch.Tensor) and temperature < 0) or (
                top_k is not None and not isinstance(top_k, torch.Tensor) and top_k < 1):
            raise ValueError("generate: temperature must be >= 0 and top_k >= 1")
        dev = tokens.device
        if max_new_tokens == 0:
            return torch.empty(B, 0, dtype=torch.int64, device=dev)
        pool_any_dtype = kv_dtype is None  # a caller's pool: its own dtype stands unless kv_dtype names one
        if kv_dtype is None:
            kv_dtype = self.cache_dtype(dev)
        elif kv_dtype == "fp8":
            kv_dtype = torch.float8_e4m3fn
        elif not isinstance(kv_dtype, torch.dtype):
            raise ValueError(f"generate: kv_dtype must be None, 'fp8' or a torch dtype, got {kv_dtype!r}")
        if page_size is not None and kv_pool is not None:
            raise ValueError("generate: pass page_size or kv_pool, not both")
        if page_size is None and kv_pool is None:
            cache = KVCache.allocate(self.cfg, B, S + max_new_tokens, dev, kv_dtype)
            logits = self.prefill(tokens, cache, prompt_lens, chunk=prefill_chunk)
            return self.decode_loop(logits, cache, max_new_tokens, temperature, top_k, eos_id, generator, top_p, min_p,
                                    sampler)
        host = [S] * B if prompt_lens is None else torch.as_tensor(prompt_lens).reshape(B).tolist()
        host = [min(max(int(n), 0), S) for n in host]  # read once; prefill gets the host list
        if kv_pool is None:
            pages = PagedKVCache.pages_needed(host, max_new_tokens, page_size)
            cache = PagedKVCache.allocate(self.cfg, B, pages, page_size, S + max_new_tokens, dev, kv_dtype)
        else:
            cache = kv_pool
            if cache.block_table.shape[0] != B or any(cache.capacity(b) for b in range(B)):
                raise ValueError(f"generate: kv_pool must have {B} slots, all free")
            if not pool_any_dtype and kv_dtype != cache.k.dtype:
                raise ValueError(f"generate: kv_dtype {kv_dtype} does not agree with the pool's {cache.k.dtype}")
        try:
            for b, n in enumerate(host):
                cache.reserve(b, n + max_new_tokens)
            logits = self.prefill(tokens, cache, host, chunk=prefill_chunk)
            return self.decode_loop(logits, cache, max_new_tokens, temperature, top_k, eos_id, generator, top_p, min_p,
                                    sampler)
        finally:
            if kv_pool is not None:
                for b in range(B):
                    cache.free(b)
                cache.commit()

    @torch.no_grad()
    def decode_loop(self, logits: torch.Tensor, cache, max_new_tokens: int, temperature: float = 0.0, top_k=None,
                    eos_id=None, generator=None, top_p=None, min_p=None, sampler=None) -> torch.Tensor:
        """The token loop of ``generate`` from the logits of a filled cache (``prefill``): pick a token, mask
        the rows that are finished, ``decode_step``. The greedy loop reads nothing back from the device.

        The last token picked is returned but not fed: the cache holds the prompt and the first
        ``max_new_tokens - 1`` new tokens. To go on with more input, hand it to ``extend`` in front of that input:
        ``model.extend(torch.cat([out[:, -1:], new_turn], 1), cache)`` (``generate``'s docstring has the whole
        sequence of calls); to go on sampling alone, ``decode_loop(model.decode_step(out[:, -1], cache), cache, n)``.

        ``top_p``, ``min_p``, a tensor [B] as ``temperature`` or ``top_k``, or ``sampler="fused"`` run the fused
        sampler (``generate`` has the rules: ties at the k-th value and at the nucleus cut are kept, and the draw's
        ``u`` comes from ``generator``): per step one ``torch.rand(B)`` and one ``sample_logits`` call, which also
        applies the eos mask; nothing is read back. Without them the loop below is the one there has always been."""
        B, dev = logits.shape[0], logits.device
        out = torch.empty(B, max_new_tokens, dtype=torch.int64, device=dev)
        if sampler not in (None, "fused"):
            raise ValueError(f"decode_loop: sampler must be None or 'fused', got {sampler!r}")
        if (sampler == "fused" or top_p is not None or min_p is not None or isinstance(temperature, torch.Tensor)
                or isinstance(top_k, torch.Tensor)):
            from ..ops.lm import sample_logits
            # per-row settings reach their device and dtype once, here; scalars stay scalars
            if isinstance(temperature, torch.Tensor):
                temperature = temperature.to(device=dev, dtype=torch.float32).contiguous()
            if isinstance(top_k, torch.Tensor):
                top_k = top_k.to(device=dev, dtype=torch.int32).contiguous()
            if isinstance(top_p, torch.Tensor):
                top_p = top_p.to(device=dev, dtype=torch.float32).contiguous()
            if isinstance(min_p, torch.Tensor):
                min_p = min_p.to(device=dev, dtype=torch.float32).contiguous()
            done = None if eos_id is None else torch.zeros(B, dtype=torch.uint8, device=dev)
            for i in range(max_new_tokens):
                u = torch.rand(B, generator=generator, device=dev)
                tok = sample_logits(logits, u, temperature, top_k, top_p, min_p, eos_id, done)
                out[:, i] = tok
                if i + 1 < max_new_tokens:
                    logits = self.decode_step(tok, cache)
            return out
        finished = torch.zeros(B, dtype=torch.bool, device=dev)
        eos = None if eos_id is None else torch.full((), eos_id, dtype=torch.int64, device=dev)
        for i in range(max_new_tokens):
            if temperature == 0:
                tok = logits.argmax(-1)
            else:
                z = logits.float() if logits.dtype in (torch.bfloat16, torch.float16) else logits
                if top_k is not None and top_k < z.shape[-1]:
                    kth = z.topk(top_k, dim=-1).values[:, -1:]
                    z = z.masked_fill(z < kth, float("-inf"))
                tok = torch.multinomial(torch.softmax(z / temperature, -1), 1, generator=generator).squeeze(1)
            if eos is not None:
                tok = torch.where(finished, eos, tok)
                finished = finished | (tok == eos)
            out[:, i] = tok
            if i + 1 < max_new_tokens:
                logits = self.decode_step(tok, cache)
        return out


def build(name: str, qk_norm: bool = False) -> Llama:
    key = name.lower().replace("_", "-")
    if key in ("llama3-8b", "llama-3-8b", "llama38b"):
        key = "llama3-8b"
    if key not in CONFIGS:
        raise ValueError(f"unknown LM config {name!r}; choose from {sorted(CONFIGS)}")
    cfg = CONFIGS[key]
    return Llama(replace(cfg, qk_norm=True) if qk_norm else cfg)


def param_count(cfg: LlamaConfig) -> int:
    hd = cfg.dim // cfg.n_heads
    attn = cfg.dim * hd * (cfg.n_heads * 2 + cfg.n_kv_heads * 2)
    ffn = 3 * cfg.dim * cfg.ffn_dim
    qk = 2 * hd if cfg.qk_norm else 0
    return cfg.n_layers * (attn + ffn + 2 * cfg.dim + qk) + 2 * cfg.vocab_size * cfg.dim + cfg.dim
