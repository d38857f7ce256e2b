#!/usr/bin/env python
"""The residual add + RMSNorm of one site of the LM residual stream at the Llama-3-8B shape: what the
step runs without and with ``fused_residual``.

  --arm unfused  torch add (fp32 stream + bf16 branch output) then ops.lm.rms_norm; backward through
                 autograd: rmsnorm_bwd4_kernel + the column sum, the accumulation add of the norm's dx and
                 the pass-through gradient, the cast of the stream gradient to bf16 for the branch
  --arm fused    ops.lm.add_rms_norm: add_rmsnorm_fwd4_kernel; add_rmsnorm_bwd4_kernel + the column sum

fp32 stream, bf16 delta, bf16 y (bf16 autocast), bf16 gy, fp32 gh. One process per arm (run the arms
alternately and compare the spread); forward (under no_grad) and forward + backward are timed with
device events, the warm-up iterations are dropped, one JSON line is printed. Bytes are counted from
the shapes, per element: forward 4 + 2 read, 4 written by the add and 4 read, 2 written by the norm
(16) against x, delta read and h, y written (12); backward 4 + 2 read, 4 written by the norm, 4 + 4
read, 4 written by the accumulation, 4 read, 2 written by the cast (28) against h, gy, gh read and dx
and its bf16 copy written (16). Needs a GPU: there is no CPU fallback.

  python scripts/bench_add_rmsnorm.py --arm fused --iters 20 --warmup 5
  python scripts/bench_add_rmsnorm.py --summary results.jsonl   # median and range over the processes
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FWD_BYTES = {"unfused": 16, "fused": 12}
BWD_BYTES = {"unfused": 28, "fused": 16}


def _timed(fn, warmup, iters):
    import torch
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(warmup + iters)]
    for s, e in ev:
        s.record()
        fn()
        e.record()
    torch.cuda.synchronize()
    us = [s.elapsed_time(e) * 1e3 for s, e in ev[warmup:]]
    return statistics.median(us), min(us), max(us)


def summary(path: str) -> int:
    """median and range of the processes' medians per arm, the achieved ratios and the gate: the fused
    medians below the unfused arm's lowest process median by more than the unfused arm's own range"""
    runs = {"unfused": [], "fused": []}
    with open(path) as f:
        for line in f:
            line = line.strip()
            if line.startswith("{"):
                r = json.loads(line)
                runs[r["arm"]].append(r)
    if not runs["unfused"] or not runs["fused"]:
        raise SystemExit("bench_add_rmsnorm: the summary needs result lines of both arms")
    out = {"processes": {k: len(v) for k, v in runs.items()}}
    ok = True
    for key, nbytes in (("fwd", FWD_BYTES), ("fwd_bwd", {k: FWD_BYTES[k] + BWD_BYTES[k] for k in FWD_BYTES})):
        med = {arm: [r[f"{key}_us_median"] for r in runs[arm]] for arm in runs}
        u_lo, u_range = min(med["unfused"]), max(med["unfused"]) - min(med["unfused"])
        gate = all(m < u_lo - u_range for m in med["fused"])
        ok = ok and gate
        n = runs["fused"][0]["rows"] * runs["fused"][0]["dim"]
        out[key] = {arm: {"median_us": round(statistics.median(med[arm]), 1), "min_us": min(med[arm]),
                          "max_us": max(med[arm]),
                          "GBps": round(n * nbytes[arm] / statistics.median(med[arm]) / 1e3, 1)} for arm in runs}
        out[key]["time_ratio_fused_over_unfused"] = round(statistics.median(med["fused"]) /
                                                          statistics.median(med["unfused"]), 3)
        out[key]["byte_ratio_expected"] = round(nbytes["fused"] / nbytes["unfused"], 3)
        out[key]["gate"] = gate
    out["gate"] = ok
    print(json.dumps(out))
    return 0 if ok else 1


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--arm", choices=["unfused", "fused"])
    ap.add_argument("--summary", metavar="JSONL", help="summarise the result lines of several processes")
    ap.add_argument("--rows", type=int, default=16384)
    ap.add_argument("--dim", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    if a.summary:
        return summary(a.summary)
    if a.arm is None:
        ap.error("--arm or --summary")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_add_rmsnorm: needs a GPU")
    import cs744_pytorch_distributed_tutorial_amd as pkg
    pkg.ensure_hw_queues()
    from cs744_pytorch_distributed_tutorial_amd.ops import lm, native
    native.C()
    dev = torch.device("cuda", 0)
    R, D = a.rows, a.dim
    gen = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(R, D, device=dev, generator=gen).requires_grad_()
    d = torch.randn(R, D, device=dev, generator=gen).bfloat16().requires_grad_()
    w = (torch.rand(D, device=dev, generator=gen) + 0.5).requires_grad_()
    gy = torch.randn(R, D, device=dev, generator=gen).bfloat16()
    gh = torch.randn(R, D, device=dev, generator=gen)

    if a.arm == "unfused":
        def op():
            h = x + d
            return h, lm.rms_norm(h, w, 1e-5)
    else:
        def op():
            return lm.add_rms_norm(x, d, w, 1e-5)

    def fwd():
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            return op()

    def fwd_bwd():
        x.grad = d.grad = w.grad = None
        with torch.autocast("cuda", dtype=torch.bfloat16):
            h, y = op()
        torch.autograd.backward([h, y], [gh, gy])

    h, y = fwd()
    assert h.dtype == torch.float32 and y.dtype == torch.bfloat16
    del h, y
    f_med, f_min, f_max = _timed(fwd, a.warmup, a.iters)
    fb_med, fb_min, fb_max = _timed(fwd_bwd, a.warmup, a.iters)
    assert x.grad.dtype == torch.float32 and d.grad.dtype == torch.bfloat16
    n = R * D
    fwd_bytes, bwd_bytes = n * FWD_BYTES[a.arm], n * BWD_BYTES[a.arm]
    print(json.dumps({"arm": a.arm, "rows": R, "dim": D, "iters": a.iters, "fwd_us_median": round(f_med, 1),
                      "fwd_us_min": round(f_min, 1), "fwd_us_max": round(f_max, 1),
                      "fwd_bwd_us_median": round(fb_med, 1), "fwd_bwd_us_min": round(fb_min, 1),
                      "fwd_bwd_us_max": round(fb_max, 1), "fwd_bytes": fwd_bytes, "bwd_bytes": bwd_bytes,
                      "fwd_GBps": round(fwd_bytes / f_med / 1e3, 1),
                      "fwd_bwd_GBps": round((fwd_bytes + bwd_bytes) / fb_med / 1e3, 1),
                      "peak_mem_GB": round(torch.cuda.max_memory_allocated() / 2**30, 2)}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
