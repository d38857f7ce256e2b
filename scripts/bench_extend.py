#!/usr/bin/env python
"""Extend attention at the Llama-3 shape (Hq 32, Hkv 8, D 128, bf16): T new tokens per row against a filled KV
cache, ops.attention.extend_attention / extend_attention_paged against what the project and PyTorch offered before.

  --part a   parity with the flash forward: start = 0, T = S = 2048, B 8 (the kernel does the forward's work)
     --arm extend        extend_attention on the contiguous cache
     --arm extend_paged  extend_attention_paged, the same keys in shuffled pages of --page positions
     --arm flash         ops.attention.attention(q, k, v, causal=True) under no_grad
  --part b   the new capability: T = 512 against start in {2048, 7680}, B 8
     --arm extend / extend_paged
     --arm sdpa          F.scaled_dot_product_attention(q, k, v, attn_mask=bottom-right causal [T, start + T],
                         enable_gqa=True) on the same cache slice (transposed views, no copy)
  --part c   end to end: llama3-1b (max_seq raised to 8192) under bf16 autocast, prefill of 1 x 8192 tokens
     --arm oneshot       Llama.prefill(tokens, cache)
     --arm chunked       Llama.prefill(tokens, cache, chunk=--chunk)
             reports the time of a prefill and torch.cuda.max_memory_allocated over it (weights and cache included)

One process per arm runs every shape of its part (run the arms alternately and compare the spread); a call is timed
with device events, the warm-up iterations are dropped, one JSON line is printed. Parts a and b rotate over several
copies of the cache (at least --rotate-mib of K and V) so that no call finds its keys in the last-level cache left by
the call before. Needs a GPU: there is no CPU fallback.

  python scripts/bench_extend.py --part a --arm extend
  python scripts/bench_extend.py --summary results.jsonl   # median and range over the processes, the ratios
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HQ, HKV, D, B = 32, 8, 128, 8
PARTS = {"a": [(2048, 0)], "b": [(512, 2048), (512, 7680)]}  # (T, start)
BASELINE = {"a": "flash", "b": "sdpa", "c": "oneshot"}


def _timed(fns, warmup, iters):
    import torch
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(warmup + iters)]
    for i, (s, e) in enumerate(ev):
        s.record()
        fns[i % len(fns)]()
        e.record()
    torch.cuda.synchronize()
    us = [s.elapsed_time(e) * 1e3 for s, e in ev[warmup:]]
    return statistics.median(us), min(us), max(us)


def summary(path: str) -> int:
    """per part and shape: median and range of the processes' medians per arm, each arm's ratio to the part's
    baseline arm, and for part a the condition: not slower than the flash forward beyond the two arms' run-to-run
    range (the sum of their half-ranges). Part c adds the peak memory."""
    runs = {}
    with open(path) as f:
        for line in f:
            line = line.strip()
            if line.startswith("{"):
                r = json.loads(line)
                if "part" in r:  # the paged arm once per page size
                    arm = r["arm"] + (f"_page{r['page']}" if r.get("page") else "")
                    runs.setdefault(r["part"], {}).setdefault(arm, []).append(r)
    out, ok = [], True
    for part in sorted(runs):
        arms, base = runs[part], BASELINE[part]
        if base not in arms:
            raise SystemExit(f"bench_extend: part {part} needs result lines of the {base} arm")
        for name in [s["name"] for s in arms[base][0]["shapes"]]:
            med = {arm: [next(s for s in r["shapes"] if s["name"] == name)["us_median"] for r in rs]
                   for arm, rs in arms.items()}
            m = {arm: statistics.median(v) for arm, v in med.items()}
            row = {"part": part, "shape": name, "processes": {arm: len(v) for arm, v in med.items()}}
            for arm, v in med.items():
                row[arm] = {"median_us": round(m[arm], 1), "min_us": round(min(v), 1), "max_us": round(max(v), 1)}
                if part == "c":
                    mem = [next(s for s in r["shapes"] if s["name"] == name)["peak_mib"] for r in arms[arm]]
                    row[arm]["peak_mib"] = round(statistics.median(mem), 1)
                if arm != base:
                    row[arm]["time_ratio_over_" + base] = round(m[arm] / m[base], 3)
                    if part == "a":
                        spread = (max(v) - min(v)) / 2 + (max(med[base]) - min(med[base])) / 2
                        row[arm]["spread_us"] = round(spread, 1)
                        row[arm]["gate"] = m[arm] <= m[base] + spread
                        ok = ok and row[arm]["gate"]
            out.append(row)
    print(json.dumps({"gate_part_a": ok, "rows": out}))
    return 0 if ok else 1


def part_c(a) -> int:
    from dataclasses import replace
    import torch
    from cs744_pytorch_distributed_tutorial_amd.models import llama
    from cs744_pytorch_distributed_tutorial_amd.ops import attention
    dev = torch.device("cuda", 0)
    S = 8192
    torch.manual_seed(0)
    with torch.device(dev):
        model = llama.Llama(replace(llama.CONFIGS["llama3-1b"], max_seq=S)).eval()
    tokens = torch.randint(1, model.cfg.vocab_size, (1, S), device=dev)
    chunk = a.chunk if a.arm == "chunked" else None
    times, peak, last = [], 0, None
    with torch.autocast("cuda", dtype=torch.bfloat16):
        cache = attention.KVCache.allocate(model.cfg, 1, S, dev, model.cache_dtype(dev))
        for i in range(a.warmup + a.iters):
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            t0 = time.perf_counter()
            last = model.prefill(tokens, cache, chunk=chunk)
            torch.cuda.synchronize()
            if i >= a.warmup:
                times.append((time.perf_counter() - t0) * 1e6)
                peak = max(peak, torch.cuda.max_memory_allocated())
    assert torch.isfinite(last.float()).all()
    shape = {"name": f"llama3-1b_prefill_{S}", "us_median": round(statistics.median(times), 1),
             "us_min": round(min(times), 1), "us_max": round(max(times), 1), "peak_mib": round(peak / 2 ** 20, 1),
             "resident_mib": round(torch.cuda.memory_allocated() / 2 ** 20, 1), "chunk": chunk,
             "top_token": int(last.argmax(-1)[0]), "top_logit": round(float(last.float().max()), 4)}
    print(json.dumps({"part": "c", "arm": a.arm, "iters": a.iters, "shapes": [shape]}))
    return 0


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["a", "b", "c"])
    ap.add_argument("--arm", choices=["extend", "extend_paged", "flash", "sdpa", "oneshot", "chunked"])
    ap.add_argument("--page", type=int, default=64, help="page size of the extend_paged arm")
    ap.add_argument("--chunk", type=int, default=1024, help="chunk of the chunked arm of part c")
    ap.add_argument("--summary", metavar="JSONL", help="summarise the result lines of several processes")
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rotate-mib", type=int, default=1024)
    a = ap.parse_args()
    if a.summary:
        return summary(a.summary)
    ok = {"a": ("extend", "extend_paged", "flash"), "b": ("extend", "extend_paged", "sdpa"), "c": ("oneshot", "chunked")}
    if a.part is None or a.arm not in ok[a.part]:
        ap.error("--part a|b|c with one of its arms, or --summary")
    if a.page < 64 or a.page % 64:
        ap.error("--page: a positive multiple of 64")
    import torch
    import torch.nn.functional as F
    if not torch.cuda.is_available():
        raise SystemExit("bench_extend: needs a GPU")
    import cs744_pytorch_distributed_tutorial_amd as pkg
    pkg.ensure_hw_queues()
    from cs744_pytorch_distributed_tutorial_amd.ops import attention, native
    native.C()
    if a.part == "c":
        return part_c(a)
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(0)
    scale = 1.0 / math.sqrt(D)
    out = []
    for T, st in PARTS[a.part]:
        n = st + T
        per = 2 * B * n * HKV * D * 2
        copies = max(2, min(32, -(-a.rotate_mib * 2 ** 20 // per)))
        q = torch.randn(B, T, HQ, D, device=dev, generator=gen).bfloat16()
        caches = [(torch.randn(B, n, HKV, D, device=dev, generator=gen).bfloat16(),
                   torch.randn(B, n, HKV, D, device=dev, generator=gen).bfloat16()) for _ in range(copies)]
        start = torch.full((B,), st, dtype=torch.int32, device=dev)
        with torch.no_grad():
            assert attention.extend_native_ok(q, *caches[0], start)
            ref = attention.extend_attention(q, *caches[0], start, None, scale).float()
        if a.arm == "extend":
            def mk(kc, vc):
                return lambda: attention.extend_attention(q, kc, vc, start, None, scale)
        elif a.arm == "extend_paged":
            C = n // a.page
            assert C * a.page == n
            perm = torch.randperm(B * C, generator=torch.Generator().manual_seed(B * C)).to(dev)
            where = torch.empty(B * C, dtype=torch.int64, device=dev)
            where[perm] = torch.arange(B * C, device=dev)  # pool[i] = page perm[i], so page j lies at where[j]
            table = where.view(B, C).int().contiguous()
            caches = [tuple(t.reshape(B * C, a.page, HKV, D)[perm].contiguous() for t in c) for c in caches]
            assert attention.extend_paged_native_ok(q, *caches[0], table, start)

            def mk(kp, vp):
                return lambda: attention.extend_attention_paged(q, kp, vp, table, start, None, scale)
        elif a.arm == "flash":
            def mk(kc, vc):
                return lambda: attention.attention(q, kc, vc, causal=True)
        else:
            q4 = q.transpose(1, 2)
            mask = torch.arange(n, device=dev).view(1, n) <= st + torch.arange(T, device=dev).view(T, 1)  # [T, n]

            def mk(kc, vc):
                k4, v4 = kc.transpose(1, 2), vc.transpose(1, 2)
                return lambda: F.scaled_dot_product_attention(q4, k4, v4, attn_mask=mask, scale=scale,
                                                              enable_gqa=True).transpose(1, 2)
        fns = [mk(*c) for c in caches]
        with torch.no_grad():
            err = (fns[0]().float() - ref).abs().max().item()  # the arms compute the same thing
            assert err < 0.05, f"T {T} start {st}: the arms disagree by {err}"
            med, lo, hi = _timed(fns, a.warmup, a.iters)
        # the lower triangle's share of the T x n score matrix, both products, multiply and add
        flops = 4 * B * HQ * D * (T * st + T * (T + 1) // 2)
        out.append({"name": f"B{B}_T{T}_start{st}", "T": T, "start": st, "copies": copies, "us_median": round(med, 1),
                    "us_min": round(lo, 1), "us_max": round(hi, 1), "TFLOPs": round(flops / med / 1e6, 1),
                    "max_abs_diff": err})
        del caches, fns
    print(json.dumps({"part": a.part, "arm": a.arm, "page": a.page if a.arm == "extend_paged" else 0, "heads": HQ,
                      "kv_heads": HKV, "head_dim": D, "iters": a.iters, "shapes": out}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
