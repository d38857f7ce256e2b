#!/usr/bin/env python
"""QK-norm + RoPE of one attention layer at the Llama-3-8B shape (16384 tokens, Hq 32, Hkv 8, hd 128, bf16):
the fused op against the composition of the existing ops.

  --arm composed  ops.lm.rms_norm on the [-1, hd] views of q and k, then ops.lm.rope on each: four launches
                  forward (one 256-thread block per head-row in the norm), rope's inverse and
                  rmsnorm_bwd4_kernel + the column sum for each projection backward
  --arm fused     ops.lm.qk_norm_rope: qk_norm_rope_fwd_kernel; qk_norm_rope_bwd_kernel + the column sum

bf16 q, k and gradients, fp32 gains. One process per arm (run the arms alternately and compare the
spread); forward (under no_grad) and forward + backward are timed with device events, the warm-up
iterations are dropped, one JSON line is printed. Bytes are counted from the shapes, per element of q and
k: forward 2 read + 2 written by the norm and again by the rotation (8) against one read and one write (4);
backward 2 + 2 by the inverse rotation, then x and g read and dx written by the norm's backward (10)
against x and g read and dx written (6). Needs a GPU: there is no CPU fallback.

  python scripts/bench_qk_norm.py --arm fused --iters 20 --warmup 5
  python scripts/bench_qk_norm.py --summary results.jsonl   # median and range over the processes
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FWD_BYTES = {"composed": 8, "fused": 4}
BWD_BYTES = {"composed": 10, "fused": 6}


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
    """median and range of the processes' medians per arm, the achieved rates and the gate: the fused arm
    is not slower than the composition (its median of the process medians at or below the composed arm's)"""
    runs = {"composed": [], "fused": []}
    with open(path) as f:
        for line in f:
            line = line.strip()
            if line.startswith("{"):
                r = json.loads(line)
                runs[r["arm"]].append(r)
    if not runs["composed"] or not runs["fused"]:
        raise SystemExit("bench_qk_norm: the summary needs result lines of both arms")
    out = {"processes": {k: len(v) for k, v in runs.items()}}
    ok = True
    n = runs["fused"][0]["elements"]
    for key, nbytes in (("fwd", FWD_BYTES), ("fwd_bwd", {k: FWD_BYTES[k] + BWD_BYTES[k] for k in FWD_BYTES})):
        med = {arm: [r[f"{key}_us_median"] for r in runs[arm]] for arm in runs}
        gate = statistics.median(med["fused"]) <= statistics.median(med["composed"])
        ok = ok and gate
        out[key] = {arm: {"median_us": round(statistics.median(med[arm]), 1), "min_us": min(med[arm]),
                          "max_us": max(med[arm]),
                          "GBps": round(n * nbytes[arm] / statistics.median(med[arm]) / 1e3, 1)} for arm in runs}
        out[key]["time_ratio_fused_over_composed"] = round(statistics.median(med["fused"]) /
                                                           statistics.median(med["composed"]), 3)
        out[key]["byte_ratio_expected"] = round(nbytes["fused"] / nbytes["composed"], 3)
        out[key]["gate"] = gate
    out["gate"] = ok
    print(json.dumps(out))
    return 0 if ok else 1


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--arm", choices=["composed", "fused"])
    ap.add_argument("--summary", metavar="JSONL", help="summarise the result lines of several processes")
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--seq", type=int, default=8192)
    ap.add_argument("--heads", type=int, default=32)
    ap.add_argument("--kv-heads", type=int, default=8)
    ap.add_argument("--head-dim", type=int, default=128)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    if a.summary:
        return summary(a.summary)
    if a.arm is None:
        ap.error("--arm or --summary")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_qk_norm: needs a GPU")
    import cs744_pytorch_distributed_tutorial_amd as pkg
    pkg.ensure_hw_queues()
    from cs744_pytorch_distributed_tutorial_amd.models.llama import rope_tables
    from cs744_pytorch_distributed_tutorial_amd.ops import lm, native
    native.C()
    dev = torch.device("cuda", 0)
    B, S, Hq, Hkv, hd = a.batch, a.seq, a.heads, a.kv_heads, a.head_dim
    gen = torch.Generator(device=dev).manual_seed(0)
    q = torch.randn(B, S, Hq, hd, device=dev, generator=gen).bfloat16().requires_grad_()
    k = torch.randn(B, S, Hkv, hd, device=dev, generator=gen).bfloat16().requires_grad_()
    wq = (torch.rand(hd, device=dev, generator=gen) + 0.5).requires_grad_()
    wk = (torch.rand(hd, device=dev, generator=gen) + 0.5).requires_grad_()
    gq = torch.randn(B, S, Hq, hd, device=dev, generator=gen).bfloat16()
    gk = torch.randn(B, S, Hkv, hd, device=dev, generator=gen).bfloat16()
    cos, sin = rope_tables(S, hd, 500000.0, dev)

    if a.arm == "composed":
        def op():
            yq = lm.rope(lm.rms_norm(q.view(-1, hd), wq, 1e-5).view_as(q), cos, sin)
            yk = lm.rope(lm.rms_norm(k.view(-1, hd), wk, 1e-5).view_as(k), cos, sin)
            return yq, yk
    else:
        def op():
            return lm.qk_norm_rope(q, k, wq, wk, cos, sin, 1e-5)

    def fwd():
        with torch.no_grad():
            return op()

    def fwd_bwd():
        q.grad = k.grad = wq.grad = wk.grad = None
        yq, yk = op()
        torch.autograd.backward([yq, yk], [gq, gk])

    yq, yk = fwd()
    assert yq.dtype == torch.bfloat16 and yq.shape == q.shape and yk.shape == k.shape
    del yq, yk
    f_med, f_min, f_max = _timed(fwd, a.warmup, a.iters)
    fb_med, fb_min, fb_max = _timed(fwd_bwd, a.warmup, a.iters)
    assert q.grad.dtype == torch.bfloat16 and wq.grad.dtype == torch.float32 and wk.grad.shape == (hd,)
    n = B * S * (Hq + Hkv) * hd
    fwd_bytes, bwd_bytes = n * FWD_BYTES[a.arm], n * BWD_BYTES[a.arm]
    print(json.dumps({"arm": a.arm, "tokens": B * S, "heads": Hq, "kv_heads": Hkv, "head_dim": hd, "elements": n,
                      "iters": a.iters, "fwd_us_median": round(f_med, 1), "fwd_us_min": round(f_min, 1),
                      "fwd_us_max": round(f_max, 1), "fwd_bwd_us_median": round(fb_med, 1),
                      "fwd_bwd_us_min": round(fb_min, 1), "fwd_bwd_us_max": round(fb_max, 1),
                      "fwd_bytes": fwd_bytes, "bwd_bytes": bwd_bytes, "fwd_GBps": round(fwd_bytes / f_med / 1e3, 1),
                      "fwd_bwd_GBps": round((fwd_bytes + bwd_bytes) / fb_med / 1e3, 1),
                      "peak_mem_GB": round(torch.cuda.max_memory_allocated() / 2**30, 2)}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
