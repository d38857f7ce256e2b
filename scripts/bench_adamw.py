#!/usr/bin/env python
"""The optimizer pass alone on Llama-3-8B's parameter shapes cut down to a few layers: FusedAdamW with
global-norm clipping against what stock PyTorch needs for the same step.

  --arm fused   ops.optim.FusedAdamW(max_grad_norm=1): one norm launch + one update launch per group,
                the bf16 shadows of the ShadowLinear weights rewritten by the update
  --arm torch   clip_grad_norm_ + torch.optim.AdamW(fused=True) + a fresh bf16 cast of every ShadowLinear
                weight (what ShadowLinear does at its next use after a foreign optimizer)

One process per arm (run the arms alternately and compare the spread); each step is timed with device
events, the warm-up steps are dropped, and one JSON line is printed. Bytes per step are counted from the
shapes: 16 B read + 12 B written per parameter, 2 B per shadowed parameter, 4 B per parameter for the
norm pass. Needs a GPU: there is no CPU fallback.

  python scripts/bench_adamw.py --arm fused --layers 4 --steps 30 --warmup 10
"""
import argparse
import dataclasses
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--arm", choices=["fused", "torch"], required=True)
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--max-grad-norm", type=float, default=1.0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_adamw: needs a GPU")
    import cs744_pytorch_distributed_tutorial_amd as pkg
    pkg.ensure_hw_queues()
    from cs744_pytorch_distributed_tutorial_amd.models import llama
    from cs744_pytorch_distributed_tutorial_amd.ops.lm import ShadowLinear
    from cs744_pytorch_distributed_tutorial_amd.ops.optim import FusedAdamW
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    with torch.device(dev):
        model = llama.Llama(dataclasses.replace(llama.CONFIGS["llama3-8b"], n_layers=a.layers))
    params = list(model.parameters())
    shadowed = [m for m in model.modules() if isinstance(m, ShadowLinear)]
    for m in shadowed:
        m._shadow()  # live bf16 copies, as after a bf16-autocast forward
    for p in params:
        p.grad = torch.randn_like(p) * 1e-3
    groups = [{"params": [p for p in params if p.dim() >= 2], "weight_decay": 0.1},
              {"params": [p for p in params if p.dim() < 2], "weight_decay": 0.0}]
    kw = dict(lr=3e-4, betas=(0.9, 0.95), eps=1e-8, weight_decay=0.1)
    if a.arm == "fused":
        opt = FusedAdamW(groups, max_grad_norm=a.max_grad_norm, **kw)

        def step():
            opt.step()
    else:
        opt = torch.optim.AdamW(groups, fused=True, **kw)

        def step():
            torch.nn.utils.clip_grad_norm_(params, a.max_grad_norm)
            opt.step()
            for m in shadowed:
                m._shadow()
    n = sum(p.numel() for p in params)
    nsh = sum(m.weight.numel() for m in shadowed)
    nbytes = 28 * n + 2 * nsh + 4 * n
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
          for _ in range(a.warmup + a.steps)]
    for s, e in ev:
        s.record()
        step()
        e.record()
    torch.cuda.synchronize()
    us = [s.elapsed_time(e) * 1e3 for s, e in ev[a.warmup:]]
    if a.arm == "fused":
        assert all(m.weight._cs_bf16_shadow_version == m.weight._version for m in shadowed)
    med = statistics.median(us)
    print(json.dumps({"arm": a.arm, "layers": a.layers, "params": n, "shadowed_params": nsh, "steps": a.steps,
                      "us_per_step_median": round(med, 1), "us_min": round(min(us), 1), "us_max": round(max(us), 1),
                      "bytes_per_step": nbytes, "GBps_median": round(nbytes / med / 1e3, 1),
                      "peak_mem_GB": round(torch.cuda.max_memory_allocated() / 2**30, 2)}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
