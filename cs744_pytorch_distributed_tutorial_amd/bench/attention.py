"""Attention throughput on one GPU: the gfx950 flash attention (ops/attention.py) vs
PyTorch's scaled_dot_product_attention, at the Llama-3 8B attention shape (Hq 32, Hkv 8,
D 128, causal, bf16). FLOPs counted as 4*B*Hq*S*S*D (forward, halved for causal) and 3.5x
that for forward+backward (the backward's five products, 2.5x the forward's two).

    python -m cs744_pytorch_distributed_tutorial_amd.bench.attention --seq 2048 4096

``--doc-len N`` packs equal documents of N tokens into every row and adds the document-masked
kernels (``native_doc_*``): their TFLOP/s count only the visible (query, key) pairs, whose share of
the causal triangle is ``visible_fraction``.

    python -m cs744_pytorch_distributed_tutorial_amd.bench.attention --seq 8192 --doc-len 1024
"""
from __future__ import annotations

import argparse
import json

import torch
import torch.nn.functional as F


def _time(fn, iters: int) -> float:
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main(argv=None) -> None:
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=1)
    p.add_argument("--seq", type=int, nargs="+", default=[2048, 4096])
    p.add_argument("--heads", type=int, default=32)
    p.add_argument("--kv-heads", type=int, default=8)
    p.add_argument("--head-dim", type=int, default=128)
    p.add_argument("--iters", type=int, default=20)
    p.add_argument("--doc-len", type=int, default=None, help="also time document-masked attention, documents of N tokens")
    a = p.parse_args(argv)
    from ..ops.attention import attention, doc_bounds
    dev = torch.device("cuda", 0)
    for S in a.seq:
        B, Hq, Hkv, D = a.batch, a.heads, a.kv_heads, a.head_dim
        q = torch.randn(B, S, Hq, D, device=dev, dtype=torch.bfloat16, requires_grad=True)
        k = torch.randn(B, S, Hkv, D, device=dev, dtype=torch.bfloat16, requires_grad=True)
        v = torch.randn(B, S, Hkv, D, device=dev, dtype=torch.bfloat16, requires_grad=True)
        do = torch.randn(B, S, Hq, D, device=dev, dtype=torch.bfloat16)
        flops = 4.0 * B * Hq * S * S * D / 2  # causal

        def ours_f():
            with torch.no_grad():
                attention(q, k, v, True)

        def ours_fb():
            attention(q, k, v, True).backward(do)

        qt, kt, vt = (t.detach().transpose(1, 2).contiguous().requires_grad_() for t in (q, k, v))
        dot = do.transpose(1, 2).contiguous()

        def sdpa_f():
            with torch.no_grad():
                F.scaled_dot_product_attention(qt, kt, vt, is_causal=True, enable_gqa=True)

        def sdpa_fb():
            F.scaled_dot_product_attention(qt, kt, vt, is_causal=True, enable_gqa=True).backward(dot)

        row = {"B": B, "S": S, "Hq": Hq, "Hkv": Hkv, "D": D}
        arms = [("native_fwd", ours_f, flops), ("native_fwd_bwd", ours_fb, 3.5 * flops),
                ("sdpa_fwd", sdpa_f, flops), ("sdpa_fwd_bwd", sdpa_fb, 3.5 * flops)]
        if a.doc_len is not None:
            N = a.doc_len
            doc = doc_bounds((torch.arange(S, device=dev) // N).expand(B, S))
            lens = [min(N, S - s0) for s0 in range(0, S, N)]
            pairs = sum(n * (n + 1) // 2 for n in lens)  # visible (query, key) pairs of one row
            dflops = 4.0 * B * Hq * pairs * D
            row["doc_len"] = N
            row["visible_fraction"] = round(pairs / (S * (S + 1) // 2), 5)

            def doc_f():
                with torch.no_grad():
                    attention(q, k, v, True, doc)

            def doc_fb():
                attention(q, k, v, True, doc).backward(do)

            arms[2:2] = [("native_doc_fwd", doc_f, dflops), ("native_doc_fwd_bwd", doc_fb, 3.5 * dflops)]
        for name, fn, fl in arms:
            try:
                ms = _time(fn, a.iters)
                row[name + "_ms"] = round(ms, 4)
                row[name + "_tflops"] = round(fl / ms / 1e9, 1)
            except RuntimeError as e:  # e.g. an SDPA backend without GQA support
                row[name + "_error"] = str(e)[:120]
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
