#!/usr/bin/env python
"""The MXFP4 weight-only linear kernel at the Llama-3-8B decode shapes against the FP8 kernel (ops.linear_fp8) and
torch.mm on a bf16 weight.

One process; per shape (N x K) and M the three paths are called alternately inside one timed loop, every shape is
warmed first, a call is timed with device events. A shape's weight is allocated several times over (at least
--rotate-mib of FP8 codes; the other formats the same number of copies) and the calls walk the copies in turn, as
the layers of a model do, so no call finds its weight in the 256 MiB last-level cache left by the call before.
GB/s is over the bytes a call reads: codes + scales + x (N * K / 2 + N * K / 32 + 2 M K for MXFP4). One JSON line
per (shape, M), then one markdown table. Needs a GPU.

  python scripts/linear_mxfp4_bench.py --iters 40 --warmup 10
  python scripts/linear_mxfp4_bench.py --generate        # llama3-8b generate tokens/s, FP8 against MXFP4, both fused
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(4096, 4096), (1024, 4096), (14336, 4096), (4096, 14336), (128256, 4096)]
MS = [1, 8, 32, 64]
HBM_PEAK_GBPS = 8000.0


def bench_shapes(a, torch, dev) -> None:
    from cs744_pytorch_distributed_tutorial_amd.ops import linear_fp8 as lf, linear_mxfp4 as lx
    gen = torch.Generator(device=dev).manual_seed(0)
    rows = []
    for N, K in ([tuple(a.only)] if a.only else SHAPES):
        w = torch.randn(N, K, device=dev, generator=gen) * 0.02
        codes, scales = lx.quantize_weight_mxfp4(w)
        c8, s8 = lf.quantize_weight_fp8(w)
        shadow = lx.dequantize_mxfp4(codes, scales, torch.bfloat16)  # the kernel and torch.mm multiply the same numbers
        del w
        copies = max(2, min(16, -(-a.rotate_mib * 2**20 // (N * K))))
        c4s, c8s = [codes.clone() for _ in range(copies)], [c8.clone() for _ in range(copies)]
        ws = [shadow.clone() for _ in range(copies)]
        for M in MS:
            x = torch.randn(M, K, device=dev, generator=gen).bfloat16()
            assert lx.linear_mxfp4_native_ok(x, codes, scales) and lf.linear_fp8_native_ok(x, c8, s8)
            ref = torch.mm(x, shadow.t()).float()
            err = (lx.linear_mxfp4(x, codes, scales).float() - ref).abs().max().item()
            # both are bf16 roundings of fp32 sums of the same exact products, in different orders
            assert err <= 2.0 ** -6 * ref.abs().max().item(), f"{N}x{K} M {M}: the paths disagree by {err}"
            ev = [[torch.cuda.Event(enable_timing=True) for _ in range(4)] for _ in range(a.warmup + a.iters)]
            with torch.no_grad():
                for i, (e0, e1, e2, e3) in enumerate(ev):
                    e0.record()
                    lx.linear_mxfp4(x, c4s[i % copies], scales)
                    e1.record()
                    lf.linear_fp8(x, c8s[i % copies], s8)
                    e2.record()
                    torch.mm(x, ws[i % copies].t())
                    e3.record()
            torch.cuda.synchronize()
            t = [[e[j].elapsed_time(e[j + 1]) * 1e3 for e in ev[a.warmup:]] for j in range(3)]
            med = [statistics.median(v) for v in t]
            nbytes = [N * K // 2 + N * K // 32 + 2 * M * K, N * K + 4 * N + 2 * M * K, 2 * N * K + 2 * M * K]
            row = {"N": N, "K": K, "M": M, "copies": copies, "slabs": lx.linear_mxfp4_splits(M, N, K),
                   "fp8_slabs": lf.linear_fp8_splits(M, N, K), "max_abs_diff": err}
            for name, v, m, nb in zip(("mxfp4", "fp8", "bf16"), t, med, nbytes):
                row.update({f"{name}_us": round(m, 1), f"{name}_us_min": round(min(v), 1), f"{name}_us_max": round(max(v), 1),
                            f"{name}_GBps": round(nb / m / 1e3, 1)})
            rows.append(row)
            print(json.dumps(row), flush=True)
        del c4s, c8s, ws, codes, c8, shadow
    print("\n| N x K | M | slabs | MXFP4 us (min..max) | FP8 us | torch.mm bf16 us | MXFP4 / FP8 | MXFP4 GB/s (share of 8 TB/s) | FP8 GB/s |")
    print("|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['N']} x {r['K']} | {r['M']} | {r['slabs']} | {r['mxfp4_us']} ({r['mxfp4_us_min']}..{r['mxfp4_us_max']}) | "
              f"{r['fp8_us']} | {r['bf16_us']} | {r['mxfp4_us'] / r['fp8_us']:.2f} | "
              f"{r['mxfp4_GBps']} ({r['mxfp4_GBps'] / HBM_PEAK_GBPS:.0%}) | {r['fp8_GBps']} |")


def bench_generate(a, torch, dev) -> None:
    """llama3-8b, greedy, 128-token prompt, --new tokens: tokens/s of generate with FP8 and with MXFP4 weights, both
    fused=True. Quantising drops the masters, so the model is built once per format and each is run --runs times."""
    from cs744_pytorch_distributed_tutorial_amd.models import llama
    for fmt in ("fp8", "mxfp4"):
        torch.manual_seed(0)
        with torch.device(dev):
            model = llama.build(a.model).eval()
        model.quantize_weights_(dtype=fmt, fused=True)
        torch.cuda.empty_cache()
        weight_bytes = sum(b.numel() * b.element_size() for n, b in model.named_buffers()
                           if n.endswith(".weight") or n.endswith(".weight_scale"))
        for B in (1, 8):
            tokens = torch.randint(1, model.cfg.vocab_size, (B, 128), device=dev,
                                   generator=torch.Generator(device=dev).manual_seed(B))
            secs = []
            with torch.autocast("cuda", dtype=torch.bfloat16):
                for _ in range(a.runs + 1):  # the first run warms up
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    model.generate(tokens, a.new)
                    torch.cuda.synchronize()
                    secs.append(time.perf_counter() - t0)
            s = statistics.median(secs[1:])
            print(json.dumps({"model": a.model, "weights": fmt, "fused": True, "B": B, "new": a.new,
                              "seconds_median": round(s, 4), "seconds_all": [round(v, 4) for v in secs[1:]],
                              "tokens_per_s": round(B * a.new / s, 1), "projection_weight_GB": round(weight_bytes / 1e9, 3),
                              "allocated_GB": round(torch.cuda.memory_allocated() / 1e9, 3)}), flush=True)
        del model
        torch.cuda.empty_cache()


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rotate-mib", type=int, default=768)
    ap.add_argument("--only", type=int, nargs=2, metavar=("N", "K"), help="one shape (for a profiler run)")
    ap.add_argument("--generate", action="store_true", help="time Llama.generate instead of the shapes")
    ap.add_argument("--model", default="llama3-8b")
    ap.add_argument("--new", type=int, default=128)
    ap.add_argument("--runs", type=int, default=3)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("linear_mxfp4_bench: needs a GPU")
    import cs744_pytorch_distributed_tutorial_amd as pkg
    pkg.ensure_hw_queues()
    from cs744_pytorch_distributed_tutorial_amd.ops import native
    native.C()
    dev = torch.device("cuda", 0)
    (bench_generate if a.generate else bench_shapes)(a, torch, dev)
    return 0


if __name__ == "__main__":
    sys.exit(main())
