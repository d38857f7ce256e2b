#!/usr/bin/env python
"""The MXFP4 weight-only GEMM for M > 64 (linear_mxfp4_gemm.hip) at the Llama-3-8B projection shapes against what
ran there before it, ``_dequant_mm`` (the weight dequantised to bf16 by ``dequantize_mxfp4`` in plain torch, then the
bf16 GEMM), and for information against the FP8 GEMM on the same shape and torch.mm on a bf16 copy of the weight.

One process; every shape and M is warmed first, then the paths are called alternately inside one timed loop and each
call is timed with device events. A shape's weight is allocated several times over (at least --rotate-mib of codes)
and the calls walk the copies in turn, as the layers of a model do, so no call finds its weight in the 256 MiB
last-level cache left by the call before. Per (shape, M): the medians, the new kernel's TFLOP/s (2 M N K) and weight
GB/s (N K / 2 + N K / 32 bytes), and which of its two lower bounds is the larger: FLOPs at --peak-tflops or bytes
(codes, scales, x and y once) at 8 TB/s. At M = 64 the skinny kernel is timed too. ``_dequant_mm`` is skipped where
its int64 index tensor alone (8 N K bytes) would pass --max-slow-gib, and the head where y alone would pass 1 GiB.
One JSON line per (shape, M), then one markdown table. Needs a GPU.

  python scripts/linear_mxfp4_gemm_bench.py --iters 20 --warmup 5
  python scripts/linear_mxfp4_gemm_bench.py --generate   # llama3-8b, B 8, prompt 512: generate with and without the GEMM
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(4096, 4096), (1024, 4096), (14336, 4096), (4096, 14336), (128256, 4096)]
MS = [64, 128, 256, 512, 2048, 8192]
HBM_PEAK_GBPS = 8000.0
MAX_Y_BYTES = 1 << 30


def bench_shapes(a, torch, dev) -> None:
    from cs744_pytorch_distributed_tutorial_amd.ops import linear_fp8 as lf
    from cs744_pytorch_distributed_tutorial_amd.ops import linear_mxfp4 as lx
    from cs744_pytorch_distributed_tutorial_amd.ops import native
    gen = torch.Generator(device=dev).manual_seed(0)
    rows = []
    for N, K in ([tuple(a.only)] if a.only else SHAPES):
        w = torch.randn(N, K, device=dev, generator=gen) * 0.02
        codes, scales = lx.quantize_weight_mxfp4(w)
        del w
        shadow = torch.cat([lx.dequantize_mxfp4(codes[i:i + 8192], scales[i:i + 8192]) for i in range(0, N, 8192)])
        c8, s8 = lf.quantize_weight_fp8(shadow)  # every path multiplies by the same numbers: e2m1 * 2^e fits e4m3
        wbytes = N * K // 2 + N * K // 32
        copies = max(2, min(16, -(-a.rotate_mib * 2**20 // wbytes)))
        cs, ss = [codes.clone() for _ in range(copies)], [scales.clone() for _ in range(copies)]
        nb = max(2, min(copies, -(-a.rotate_mib * 2**20 // (2 * N * K))))  # 4x the bytes: fewer copies do
        ws = [shadow.clone() for _ in range(nb)]
        c8s = [c8.clone() for _ in range(max(2, min(copies, -(-a.rotate_mib * 2**20 // (N * K)))))]
        slow = 8 * N * K <= a.max_slow_gib * 2**30
        for M in (a.m or MS):
            if M * N * 2 > MAX_Y_BYTES:
                continue
            x = torch.randn(M, K, device=dev, generator=gen).bfloat16()
            paths = [("gemm", lambda i: native.C().linear_mxfp4_gemm(x, cs[i % copies], ss[i % copies], 0))]
            if slow:
                paths.append(("dequant_mm", lambda i: lx._dequant_mm(x, cs[i % copies], ss[i % copies])))
            paths += [("fp8_gemm", lambda i: native.C().linear_fp8_gemm(x, c8s[i % len(c8s)], s8, 0)),
                      ("bf16_mm", lambda i: torch.mm(x, ws[i % nb].t()))]
            if M <= lx.linear_mxfp4_max_m():
                paths.append(("skinny", lambda i: lx.linear_mxfp4(x, cs[i % copies], ss[i % copies])))
            ref = torch.mm(x, shadow.t()).float()
            tol = 2.0 ** -6 * ref.abs().max().item()
            for name, f in paths:  # bf16 roundings of fp32 sums of the same exact products, in different orders
                err = (f(0).float() - ref).abs().max().item()
                assert err <= tol, f"{N}x{K} M {M}: {name} is off by {err}"
            del ref
            n = a.warmup + a.iters
            ev = [[torch.cuda.Event(enable_timing=True) for _ in range(len(paths) + 1)] for _ in range(n)]
            with torch.no_grad():
                for i, e in enumerate(ev):
                    e[0].record()
                    for j, (_, f) in enumerate(paths):
                        f(i)
                        e[j + 1].record()
            torch.cuda.synchronize()
            row = {"N": N, "K": K, "M": M, "copies": copies, "slabs": lx.linear_mxfp4_gemm_splits(M, N, K),
                   "linear_mxfp4_routes_here": lx.linear_mxfp4_gemm_ok(x, codes, scales)}
            for j, (name, _) in enumerate(paths):
                us = [e[j].elapsed_time(e[j + 1]) * 1e3 for e in ev[a.warmup:]]
                row.update({f"{name}_us": round(statistics.median(us), 1), f"{name}_us_min": round(min(us), 1),
                            f"{name}_us_max": round(max(us), 1)})
            g = row["gemm_us"]
            t_flops = 2.0 * M * N * K / (a.peak_tflops * 1e6)                     # us
            t_bytes = (wbytes + 2.0 * M * K + 2.0 * M * N) / (HBM_PEAK_GBPS * 1e3)  # us
            row.update({"gemm_TFLOPs": round(2.0 * M * N * K / g / 1e6, 1), "gemm_weight_GBps": round(wbytes / g / 1e3, 1),
                        "bound": "flops" if t_flops > t_bytes else "bytes", "bound_us": round(max(t_flops, t_bytes), 1)})
            rows.append(row)
            print(json.dumps(row), flush=True)
        del cs, ss, ws, c8s, codes, scales, shadow, c8, s8
        torch.cuda.empty_cache()
    print("\n| N x K | M | slabs | GEMM us | dequant + mm us | speed-up | FP8 GEMM us | torch.mm bf16 us | skinny us | "
          "GEMM TFLOP/s | weight GB/s | larger bound (us) |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        d = r.get("dequant_mm_us")
        speedup = "%.2f" % (d / r["gemm_us"]) if d else ""
        print(f"| {r['N']} x {r['K']} | {r['M']} | {r['slabs']} | {r['gemm_us']} | {d or 'skipped'} | "
              f"{speedup} | {r['fp8_gemm_us']} | {r['bf16_mm_us']} | "
              f"{r.get('skinny_us', '')} | {r['gemm_TFLOPs']} | {r['gemm_weight_GBps']} | {r['bound']} ({r['bound_us']}) |")


def bench_generate(a, torch, dev) -> None:
    """llama3-8b with MXFP4 weights, greedy, B 8, a 512-token prompt (a prefill of 4096 rows) and --new tokens:
    seconds and peak allocated memory of generate with the GEMM and with it switched off (every M > 64 on
    ``_dequant_mm``, the behaviour before the kernel), the two alternating"""
    from cs744_pytorch_distributed_tutorial_amd.models import llama
    from cs744_pytorch_distributed_tutorial_amd.ops import linear_mxfp4 as lx
    torch.manual_seed(0)
    with torch.device(dev):
        model = llama.build(a.model).eval()
    model.quantize_weights_(dtype="mxfp4")
    torch.cuda.empty_cache()
    tokens = torch.randint(1, model.cfg.vocab_size, (a.batch, a.prompt), device=dev,
                           generator=torch.Generator(device=dev).manual_seed(1))
    gemm_ok = lx.linear_mxfp4_gemm_ok
    res = {"gemm": [], "dequant_mm": []}
    peak = {}
    with torch.autocast("cuda", dtype=torch.bfloat16):
        for run in range(a.runs + 1):  # the first run of each warms up
            for name in res:
                lx.linear_mxfp4_gemm_ok = gemm_ok if name == "gemm" else (lambda *t: False)
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                t0 = time.perf_counter()
                model.generate(tokens, a.new)
                torch.cuda.synchronize()
                if run:
                    res[name].append(time.perf_counter() - t0)
                peak[name] = torch.cuda.max_memory_allocated()
    lx.linear_mxfp4_gemm_ok = gemm_ok
    for name, secs in res.items():
        print(json.dumps({"model": a.model, "path": name, "B": a.batch, "prompt": a.prompt, "new": a.new,
                          "seconds_median": round(statistics.median(secs), 4), "seconds_all": [round(v, 4) for v in secs],
                          "peak_allocated_GiB": round(peak[name] / 2**30, 3)}), flush=True)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rotate-mib", type=int, default=768)
    ap.add_argument("--peak-tflops", type=float, default=2500.0, help="dense bf16 matrix peak the FLOP bound uses")
    ap.add_argument("--max-slow-gib", type=float, default=8.0, help="skip _dequant_mm where its index tensor is larger")
    ap.add_argument("--only", type=int, nargs=2, metavar=("N", "K"), help="one shape (for a profiler run)")
    ap.add_argument("--m", type=int, nargs="+", help="the M values (default: 64 to 8192)")
    ap.add_argument("--generate", action="store_true", help="time Llama.generate instead of the shapes")
    ap.add_argument("--model", default="llama3-8b")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--prompt", type=int, default=512)
    ap.add_argument("--new", type=int, default=16)
    ap.add_argument("--runs", type=int, default=3)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("linear_mxfp4_gemm_bench: needs a GPU")
    import cs744_pytorch_distributed_tutorial_amd as pkg
    pkg.ensure_hw_queues()
    from cs744_pytorch_distributed_tutorial_amd.ops import native
    native.C()
    dev = torch.device("cuda", 0)
    (bench_generate if a.generate else bench_shapes)(a, torch, dev)
    return 0


if __name__ == "__main__":
    sys.exit(main())
