#!/usr/bin/env python
"""The fused FP8 decode projections against the separate launches they replace, at the Llama-3-8B shapes.

Call level (default): q/k/v = 4096 + 1024 + 1024 channels over K 4096 through ``linear_fp8_grouped`` against three
``linear_fp8`` calls, and gate/up = 14336 channels over K 4096 through ``swiglu_linear_fp8`` against two ``linear_fp8``
calls and ``ops.lm.swiglu``. One process; per M the two paths are called alternately inside one timed loop, timed
with device events, after a warm-up; the weights are allocated several times over (at least --rotate-mib of codes)
and the calls walk the copies, as the layers of a model do, so no call finds its weights in the last-level cache.
One JSON line per (case, M) with medians and ranges, then a markdown table. The script asserts that the two paths
agree (to the last bit when they sum the same number of slabs).

End to end (--generate): ``Llama.generate`` on llama3-8b, greedy, 128-token prompt, --new tokens, B 1 and B 8, with
``quantize_weights_()`` against ``quantize_weights_(fused=True)``: one fresh process per arm, the arms alternating,
--runs processes each. Needs a GPU.

  python scripts/linear_fp8_fused_bench.py --iters 40 --warmup 10
  python scripts/linear_fp8_fused_bench.py --generate --runs 2
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MS = [1, 8, 32, 64]
K = 4096
QKV = (4096, 1024, 1024)
FFN = 14336


def _timed(a, torch, fused, separate, copies):
    """medians and ranges (us) of the two callables, alternating in one loop; each takes the copy index"""
    n = a.warmup + a.iters
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(n)]
    with torch.no_grad():
        for i, (e0, e1, e2) in enumerate(ev):
            e0.record()
            fused(i % copies)
            e1.record()
            separate(i % copies)
            e2.record()
    torch.cuda.synchronize()
    f = [e0.elapsed_time(e1) * 1e3 for e0, e1, _ in ev[a.warmup:]]
    s = [e1.elapsed_time(e2) * 1e3 for _, e1, e2 in ev[a.warmup:]]
    out = {}
    for name, v in (("fused", f), ("separate", s)):
        out.update({f"{name}_us": round(statistics.median(v), 1), f"{name}_us_min": round(min(v), 1),
                    f"{name}_us_max": round(max(v), 1)})
    return out


def bench_calls(a, torch, dev) -> None:
    from cs744_pytorch_distributed_tutorial_amd.ops import linear_fp8 as lf, lm
    gen = torch.Generator(device=dev).manual_seed(0)

    def weight(N):
        return lf.quantize_weight_fp8(torch.randn(N, K, device=dev, generator=gen) * 0.02)

    def same(y, ref, exact, what):
        if exact:
            assert torch.equal(y.view(torch.int16), ref.view(torch.int16)), f"{what}: the paths differ"
        else:  # different slab counts: bf16 roundings of fp32 sums in two orders
            err = (y.float() - ref.float()).abs().max().item()
            assert err <= 2.0 ** -6 * ref.float().abs().max().item(), f"{what}: the paths disagree by {err}"

    rows = []
    copies = max(2, min(32, -(-a.rotate_mib * 2**20 // (sum(QKV) * K))))
    qkv = [[weight(N) for N in QKV] for _ in range(copies)]
    for M in MS:
        x = torch.randn(M, K, device=dev, generator=gen).bfloat16()
        slabs = lf.linear_fp8_grouped_splits(M, QKV, K)
        for y, (c, s) in zip(lf.linear_fp8_grouped(x, qkv[0]), qkv[0]):
            same(y, lf.linear_fp8(x, c, s, slabs=slabs), True, f"qkv M {M}")
        row = {"case": "qkv", "M": M, "copies": copies, "fused_slabs": slabs,
               "separate_slabs": [lf.linear_fp8_splits(M, N, K) for N in QKV]}
        row.update(_timed(a, torch, lambda i: lf.linear_fp8_grouped(x, qkv[i]),
                          lambda i: [lf.linear_fp8(x, c, s) for c, s in qkv[i]], copies))
        rows.append(row)
        print(json.dumps(row), flush=True)
    del qkv
    copies = max(2, min(32, -(-a.rotate_mib * 2**20 // (2 * FFN * K))))
    ffn = [(weight(FFN), weight(FFN)) for _ in range(copies)]
    for M in MS:
        x = torch.randn(M, K, device=dev, generator=gen).bfloat16()
        slabs, sep = lf.swiglu_linear_fp8_splits(M, FFN, K), lf.linear_fp8_splits(M, FFN, K)
        (g, sg), (u, su) = ffn[0]
        same(lf.swiglu_linear_fp8(x, g, sg, u, su), lm.swiglu(lf.linear_fp8(x, g, sg), lf.linear_fp8(x, u, su)),
             slabs == sep, f"gate/up M {M}")
        row = {"case": "gate_up_swiglu", "M": M, "copies": copies, "fused_slabs": slabs, "separate_slabs": [sep, sep]}
        row.update(_timed(a, torch, lambda i: lf.swiglu_linear_fp8(x, *ffn[i][0], *ffn[i][1]),
                          lambda i: lm.swiglu(lf.linear_fp8(x, *ffn[i][0]), lf.linear_fp8(x, *ffn[i][1])), copies))
        rows.append(row)
        print(json.dumps(row), flush=True)
    print("\n| case | M | slabs fused / separate | fused us (min - max) | separate us (min - max) | separate / fused |")
    print("|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['case']} | {r['M']} | {r['fused_slabs']} / {r['separate_slabs']} | {r['fused_us']} "
              f"({r['fused_us_min']} - {r['fused_us_max']}) | {r['separate_us']} ({r['separate_us_min']} - "
              f"{r['separate_us_max']}) | {r['separate_us'] / r['fused_us']:.2f} |")


def generate_arm(a, torch, dev) -> None:
    """one arm in this process: build, quantise, one warm-up generate and one timed generate per batch size"""
    from cs744_pytorch_distributed_tutorial_amd.models import llama
    torch.manual_seed(0)
    with torch.device(dev):
        model = llama.build(a.model).eval()
    model.quantize_weights_(fused=a.arm == "fused")
    torch.cuda.empty_cache()
    for B in (1, 8):
        tokens = torch.randint(1, model.cfg.vocab_size, (B, 128), device=dev,
                               generator=torch.Generator(device=dev).manual_seed(B))
        secs = []
        with torch.autocast("cuda", dtype=torch.bfloat16):
            for _ in range(3):  # the first run warms up
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = model.generate(tokens, a.new)
                torch.cuda.synchronize()
                secs.append(time.perf_counter() - t0)
        s = statistics.median(secs[1:])
        print(json.dumps({"model": a.model, "arm": a.arm, "B": B, "new": a.new, "seconds_median": round(s, 4),
                          "seconds_all": [round(v, 4) for v in secs[1:]], "tokens_per_s": round(B * a.new / s, 1),
                          "first_tokens": out[0, :8].tolist()}), flush=True)


def bench_generate(a) -> int:
    """the arms alternate, a fresh process each: this process never opens the GPU"""
    for run in range(a.runs):
        for arm in ("separate", "fused"):
            cmd = [sys.executable, os.path.abspath(__file__), "--arm", arm, "--model", a.model, "--new", str(a.new)]
            r = subprocess.run(cmd, timeout=a.arm_timeout)
            if r.returncode != 0:
                print(f"linear_fp8_fused_bench: run {run} of arm {arm} ended with {r.returncode}", file=sys.stderr)
                return 1
    return 0


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rotate-mib", type=int, default=768)
    ap.add_argument("--generate", action="store_true", help="time Llama.generate, one process per arm")
    ap.add_argument("--arm", choices=("separate", "fused"), help="run one arm of --generate in this process")
    ap.add_argument("--arm-timeout", type=float, default=400.0, help="seconds one arm's process may take")
    ap.add_argument("--model", default="llama3-8b")
    ap.add_argument("--new", type=int, default=128)
    ap.add_argument("--runs", type=int, default=2)
    a = ap.parse_args()
    if a.generate:
        return bench_generate(a)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("linear_fp8_fused_bench: needs a GPU")
    import cs744_pytorch_distributed_tutorial_amd as pkg
    pkg.ensure_hw_queues()
    from cs744_pytorch_distributed_tutorial_amd.ops import native
    native.C()
    dev = torch.device("cuda", 0)
    (generate_arm if a.arm else bench_calls)(a, torch, dev)
    return 0


if __name__ == "__main__":
    sys.exit(main())
