#!/usr/bin/env python
"""The fused softmax cross-entropy alone at the Llama-3 logits shape: the masked / z-loss kernels
against the unmasked ones.

  --arm unmasked  _C.xent_fwd + _C.xent_bwd (xent_fwd_kernel / xent_bwd_kernel, as before)
  --arm masked    _C.xent_fwd_masked + _C.xent_bwd_masked with ignore index -100 on a fraction
                  --ignored of the rows (seeded, scattered) and z-loss --z; its forward time includes
                  the one-block reduction that forms the sum / count / mean on the device

One process per arm (run the arms alternately and compare the spread); forward and forward + backward
are timed with device events over the binding calls, the warm-up iterations are dropped, one JSON line
is printed. Bytes are counted from the shapes: the forward reads the logits of the rows it does not
skip, the backward reads those again and writes every row. "op_*" times ops.lm.cross_entropy through
autograd instead (for the unmasked arm that adds the torch sum and division that form its mean).
Needs a GPU: there is no CPU fallback.

  python scripts/bench_xent.py --arm masked --ignored 0.125 --z 1e-4 --iters 20 --warmup 5
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def _timed(fn, warmup, iters):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(warmup + iters)]
    for s, e in ev:
        s.record()
        fn()
        e.record()
    torch.cuda.synchronize()
    us = [s.elapsed_time(e) * 1e3 for s, e in ev[warmup:]]
    return statistics.median(us), min(us), max(us)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--arm", choices=["unmasked", "masked"], required=True)
    ap.add_argument("--rows", type=int, default=16384)
    ap.add_argument("--vocab", type=int, default=128256)
    ap.add_argument("--dtype", choices=["bf16", "fp32"], default="bf16")
    ap.add_argument("--ignored", type=float, default=0.0,
                    help="fraction of rows carrying the ignore index (masked arm)")
    ap.add_argument("--z", type=float, default=0.0, help="z-loss coefficient (masked arm)")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_xent: needs a GPU")
    if a.arm == "unmasked" and (a.ignored or a.z):
        raise SystemExit("bench_xent: --ignored / --z belong to the masked arm")
    import cs744_pytorch_distributed_tutorial_amd as pkg
    pkg.ensure_hw_queues()
    from cs744_pytorch_distributed_tutorial_amd import _C
    from cs744_pytorch_distributed_tutorial_amd.ops import lm
    dev = torch.device("cuda", 0)
    dtype = torch.bfloat16 if a.dtype == "bf16" else torch.float32
    R, V = a.rows, a.vocab
    gen = torch.Generator(device=dev).manual_seed(0)
    x = torch.empty(R, V, dtype=dtype, device=dev)
    for lo in range(0, R, 1024):  # filled a slab at a time: no fp32 copy of the whole matrix
        x[lo:lo + 1024] = (torch.randn(min(1024, R - lo), V, device=dev, generator=gen) * 3).to(dtype)
    t = torch.randint(0, V, (R,), device=dev, generator=gen)
    n_ign = int(round(a.ignored * R))
    if n_ign:
        t[torch.randperm(R, device=dev, generator=gen)[:n_ign]] = -100
    g = torch.ones(1, device=dev)
    if a.arm == "unmasked":
        def fwd():
            return _C.xent_fwd(x, t)

        def fwd_bwd():
            _, lse = _C.xent_fwd(x, t)
            return _C.xent_bwd(x, t, lse, g, 1.0 / R)

        def op(xa):
            return lm.cross_entropy(xa, t)
    else:
        def fwd():
            return _C.xent_fwd_masked(x, t, -100, a.z)

        def fwd_bwd():
            _, lse, stats = _C.xent_fwd_masked(x, t, -100, a.z)
            return _C.xent_bwd_masked(x, t, lse, stats, g, -100, a.z)

        def op(xa):
            return lm.cross_entropy(xa, t, ignore_index=-100, z_loss=a.z)

    xa = x.detach().requires_grad_()

    def op_fwd_bwd():
        xa.grad = None
        op(xa).backward()

    f_med, f_min, f_max = _timed(fwd, a.warmup, a.iters)
    fb_med, fb_min, fb_max = _timed(fwd_bwd, a.warmup, a.iters)
    with torch.no_grad():
        o_med, _, _ = _timed(lambda: op(x), a.warmup, a.iters)
    ob_med, _, _ = _timed(op_fwd_bwd, a.warmup, a.iters)
    esz = x.element_size()
    read = (R - n_ign) * V * esz
    fwd_bytes, bwd_bytes = read, read + R * V * esz
    print(json.dumps({"arm": a.arm, "rows": R, "vocab": V, "dtype": a.dtype, "ignored_rows": n_ign, "z": a.z,
                      "iters": a.iters, "fwd_us_median": round(f_med, 1), "fwd_us_min": round(f_min, 1),
                      "fwd_us_max": round(f_max, 1), "fwd_bwd_us_median": round(fb_med, 1),
                      "fwd_bwd_us_min": round(fb_min, 1), "fwd_bwd_us_max": round(fb_max, 1),
                      "op_fwd_us_median": round(o_med, 1), "op_fwd_bwd_us_median": round(ob_med, 1),
                      "fwd_bytes": fwd_bytes, "bwd_bytes": bwd_bytes,
                      "fwd_GBps": round(fwd_bytes / f_med / 1e3, 1),
                      "fwd_bwd_GBps": round((fwd_bytes + bwd_bytes) / fb_med / 1e3, 1),
                      "peak_mem_GB": round(torch.cuda.max_memory_allocated() / 2**30, 2)}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
