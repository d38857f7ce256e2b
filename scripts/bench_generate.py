#!/usr/bin/env python
"""Greedy generation end to end: ``Llama.generate`` (prefill + KV-cache decode steps) against the only way
without a cache, a loop that re-runs the full forward on the growing sequence.

  --arm generate  model.generate(prompt, new) under bf16 autocast
  --arm naive     for every new token: model(tokens)[:, -1].argmax(-1), appended to tokens
  --kv fp8        (generate arm) an FP8 KV cache: model.generate(..., kv_dtype="fp8")
  --page-size N   (generate arm) a paged KV cache of N positions per page: model.generate(..., page_size=N)
  --temperature T --top-k K --top-p P   (generate arm) sampled instead of greedy, a seeded device generator
  --sampler fused (generate arm) the fused sampler (ops.lm.sample_logits) instead of the chain of torch ops

llama3-1b, B 8, prompt 128, 128 new tokens by default; random weights (seeded) and a random prompt. One
process per arm; after one untimed warm-up run, each timed run ends in a device synchronise and the median
and range of --runs runs are printed as one JSON line with tokens/s = B * new / time. Needs a GPU.

  python scripts/bench_generate.py --arm generate
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--arm", choices=["generate", "naive"], required=True)
    ap.add_argument("--kv", choices=["bf16", "fp8"], default="bf16", help="the KV cache format of the generate arm")
    ap.add_argument("--page-size", type=int, default=0, help="page size of a paged KV cache (0: the contiguous cache)")
    ap.add_argument("--model", default="llama3-1b")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--prompt", type=int, default=128)
    ap.add_argument("--new", type=int, default=128)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--temperature", type=float, default=0.0, help="0: greedy")
    ap.add_argument("--top-k", type=int, default=0, help="0: none")
    ap.add_argument("--top-p", type=float, default=0.0, help="0: none (given: the fused sampler runs)")
    ap.add_argument("--sampler", choices=["fused"], default=None)
    a = ap.parse_args()
    if a.arm == "naive" and (a.kv != "bf16" or a.page_size):
        ap.error("--arm naive has no KV cache")
    if a.arm == "naive" and (a.temperature or a.top_k or a.top_p or a.sampler):
        ap.error("--arm naive is greedy")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_generate: needs a GPU")
    import cs744_pytorch_distributed_tutorial_amd as pkg
    pkg.ensure_hw_queues()
    from cs744_pytorch_distributed_tutorial_amd.models import llama
    from cs744_pytorch_distributed_tutorial_amd.ops import native
    native.C()
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = llama.build(a.model).to(dev).eval()
    prompt = torch.randint(0, model.cfg.vocab_size, (a.batch, a.prompt), device=dev)

    def generate():
        return model.generate(prompt, a.new, kv_dtype="fp8" if a.kv == "fp8" else None, page_size=a.page_size or None,
                              temperature=a.temperature, top_k=a.top_k or None, top_p=a.top_p or None,
                              sampler=a.sampler, generator=torch.Generator(device=dev).manual_seed(1))

    def naive():
        tokens = prompt
        for _ in range(a.new):
            tokens = torch.cat([tokens, model(tokens)[:, -1].argmax(-1, keepdim=True)], 1)
        return tokens[:, a.prompt:]

    fn = generate if a.arm == "generate" else naive
    secs = []
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        out = fn()  # warm-up: code objects, GEMM algorithm choices, bf16 weight copies
        torch.cuda.synchronize()
        for _ in range(a.runs):
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            secs.append(time.perf_counter() - t0)
    assert out.shape == (a.batch, a.new)
    med = statistics.median(secs)
    print(json.dumps({"arm": a.arm, "kv": a.kv, "page_size": a.page_size, "model": a.model, "batch": a.batch, "prompt": a.prompt, "new": a.new,
                      "temperature": a.temperature, "top_k": a.top_k, "top_p": a.top_p, "sampler": a.sampler,
                      "runs": a.runs, "s_median": round(med, 4), "s_min": round(min(secs), 4),
                      "s_max": round(max(secs), 4), "tokens_per_s": round(a.batch * a.new / med, 1),
                      "ms_per_token_step": round(med / a.new * 1e3, 3),
                      "first_tokens": out[0, :8].tolist(),
                      "peak_mem_GB": round(torch.cuda.max_memory_allocated() / 2**30, 2)}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
