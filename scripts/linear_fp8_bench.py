#!/usr/bin/env python
"""The FP8 weight-only linear kernel at the Llama-3-8B decode shapes against torch.mm on the bf16 shadow (what a
decode step runs without quantised weights).

One process; per shape (N x K) and M the two paths are called alternately inside one timed loop, every shape is
warmed first, a call is timed with device events. A shape's weight is allocated several times over (at least
--rotate-mib of FP8 codes, the bf16 copies twice that) and the calls walk the copies in turn, as the layers of a
model do, so no call finds its weight in the 256 MiB last-level cache left by the call before. Both paths are
bound by bytes: the weight is read once (N * K bytes of codes, 2 * N * K of bf16); x, y, the scales and the fp32
partials of the split are small beside it and are not counted. The share of peak is weight bytes per second over
the HBM peak of 8 TB/s. One JSON line per (shape, M), then one markdown table. Needs a GPU.

  python scripts/linear_fp8_bench.py --iters 40 --warmup 10
  python scripts/linear_fp8_bench.py --generate          # llama3-8b generate tokens/s, bf16 against FP8 weights
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
    from cs744_pytorch_distributed_tutorial_amd.ops import linear_fp8 as lf
    gen = torch.Generator(device=dev).manual_seed(0)
    rows = []
    for N, K in ([tuple(a.only)] if a.only else SHAPES):
        w = torch.randn(N, K, device=dev, generator=gen) * 0.02
        codes, scale = lf.quantize_weight_fp8(w)
        shadow = lf.kv_dequantize(codes, scale, torch.bfloat16)  # both paths multiply by the same numbers
        del w
        copies = max(2, min(16, -(-a.rotate_mib * 2**20 // (N * K))))
        cs = [codes.clone() for _ in range(copies)]
        ws = [shadow.clone() for _ in range(copies)]
        for M in MS:
            x = torch.randn(M, K, device=dev, generator=gen).bfloat16()
            assert lf.linear_fp8_native_ok(x, codes, scale)
            ref = torch.mm(x, shadow.t()).float()
            err = (lf.linear_fp8(x, codes, scale).float() - ref).abs().max().item()
            # both are bf16 roundings of fp32 sums of the same exact products, in different orders
            assert err <= 2.0 ** -6 * ref.abs().max().item(), f"{N}x{K} M {M}: the paths disagree by {err}"
            n = a.warmup + a.iters
            ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(n)]
            with torch.no_grad():
                for i, (e0, e1, e2) in enumerate(ev):
                    e0.record()
                    lf.linear_fp8(x, cs[i % copies], scale)
                    e1.record()
                    torch.mm(x, ws[i % copies].t())
                    e2.record()
            torch.cuda.synchronize()
            fp8 = [e0.elapsed_time(e1) * 1e3 for e0, e1, _ in ev[a.warmup:]]
            bf = [e1.elapsed_time(e2) * 1e3 for _, e1, e2 in ev[a.warmup:]]
            f, b = statistics.median(fp8), statistics.median(bf)
            row = {"N": N, "K": K, "M": M, "copies": copies, "slabs": lf.linear_fp8_splits(M, N, K),
                   "fp8_us": round(f, 1), "fp8_us_min": round(min(fp8), 1), "fp8_us_max": round(max(fp8), 1),
                   "bf16_us": round(b, 1), "bf16_us_min": round(min(bf), 1), "bf16_us_max": round(max(bf), 1),
                   "fp8_GBps": round(N * K / f / 1e3, 1), "bf16_GBps": round(2 * N * K / b / 1e3, 1),
                   "max_abs_diff": err}
            rows.append(row)
            print(json.dumps(row), flush=True)
        del cs, ws, codes, shadow
    print("\n| N x K | M | slabs | FP8 kernel us | torch.mm bf16 us | speed-up | FP8 GB/s (share of 8 TB/s) | bf16 GB/s (share) |")
    print("|---|---|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['N']} x {r['K']} | {r['M']} | {r['slabs']} | {r['fp8_us']} | {r['bf16_us']} | "
              f"{r['bf16_us'] / r['fp8_us']:.2f} | {r['fp8_GBps']} ({r['fp8_GBps'] / HBM_PEAK_GBPS:.0%}) | "
              f"{r['bf16_GBps']} ({r['bf16_GBps'] / HBM_PEAK_GBPS:.0%}) |")


def bench_generate(a, torch, dev) -> None:
    """llama3-8b, greedy, 128-token prompt, --new tokens: tokens/s of generate with the bf16 shadows, then with
    FP8 weights, the two alternating is not possible (quantising drops the masters), so each is run --runs times"""
    from cs744_pytorch_distributed_tutorial_amd.models import llama
    torch.manual_seed(0)
    with torch.device(dev):
        model = llama.build(a.model).eval()
    for quantised in (False, True):
        if quantised:
            model.quantize_weights_()
            torch.cuda.empty_cache()
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
            print(json.dumps({"model": a.model, "weights": "fp8" if quantised else "bf16", "B": B, "new": a.new,
                              "seconds_median": round(s, 4), "seconds_all": [round(v, 4) for v in secs[1:]],
                              "tokens_per_s": round(B * a.new / s, 1)}), flush=True)


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
        raise SystemExit("linear_fp8_bench: needs a GPU")
    import cs744_pytorch_distributed_tutorial_amd as pkg
    pkg.ensure_hw_queues()
    from cs744_pytorch_distributed_tutorial_amd.ops import native
    native.C()
    dev = torch.device("cuda", 0)
    (bench_generate if a.generate else bench_shapes)(a, torch, dev)
    return 0


if __name__ == "__main__":
    sys.exit(main())
