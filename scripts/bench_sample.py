#!/usr/bin/env python
"""The fused sampler against the chain of torch ops it replaces, on logits of Llama-3's vocabulary.

  --arm fused   u = torch.rand(B); ops.lm.sample_logits(logits, u, ...) with the eos mask inside the kernel
  --arm torch   the chain of Llama.decode_loop before the fused sampler existed: cast to fp32, topk, compare,
                masked_fill, divide, softmax, multinomial, and the eos mask (where, |, ==). For top_p, which that
                loop never had, the usual sort-based nucleus: softmax, sort, cumsum, compare, masked_fill,
                multinomial over the sorted probabilities, gather
  --all         the driver: --rounds times, one fresh process per arm, the arms alternating; prints their lines

Every process times all of: logits [8, 128256] and [64, 128256] in bf16 (seeded, randn * 2.5), with top_k = 50,
with top_p = 0.9, and with both, at temperature 0.8. Per case: --warmup untimed calls, then device events around
--iters calls, one JSON line with the microseconds per call and the number of kernel launches of one call (counted
from a torch.profiler trace taken after the timing). Needs a GPU.

  python scripts/bench_sample.py --all
"""
import argparse
import json
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

V = 128256
CASES = [(B, s) for B in (8, 64) for s in ("top_k", "top_p", "both")]
T, K, P, EOS = 0.8, 50, 0.9, 2


def torch_chain(torch, logits, setting, finished, eos, gen):
    z = logits.float()
    if setting in ("top_k", "both"):
        kth = z.topk(K, dim=-1).values[:, -1:]
        z = z.masked_fill(z < kth, float("-inf"))
    probs = torch.softmax(z / T, -1)
    if setting in ("top_p", "both"):
        sp, si = probs.sort(-1, descending=True)
        sp = sp.masked_fill(sp.cumsum(-1) - sp >= P, 0.0)
        tok = si.gather(1, torch.multinomial(sp, 1, generator=gen)).squeeze(1)
    else:
        tok = torch.multinomial(probs, 1, generator=gen).squeeze(1)
    tok = torch.where(finished, eos, tok)
    return tok, finished | (tok == eos)


def run_arm(a) -> int:
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_sample: needs a GPU")
    from cs744_pytorch_distributed_tutorial_amd.ops import lm, native
    native.C()
    dev = torch.device("cuda", 0)
    for B, setting in CASES:
        logits = (torch.randn(B, V, generator=torch.Generator().manual_seed(B)) * 2.5).to(torch.bfloat16).to(dev)
        gen = torch.Generator(device=dev).manual_seed(1)
        kw = dict(top_k=K if setting != "top_p" else None, top_p=P if setting != "top_k" else None)
        state = {"fin8": torch.zeros(B, dtype=torch.uint8, device=dev),
                 "fin": torch.zeros(B, dtype=torch.bool, device=dev)}
        eos = torch.full((), EOS, dtype=torch.int64, device=dev)

        def call():
            if a.arm == "fused":
                u = torch.rand(B, generator=gen, device=dev)
                return lm.sample_logits(logits, u, T, eos_id=EOS, finished=state["fin8"], **kw)
            tok, state["fin"] = torch_chain(torch, logits, setting, state["fin"], eos, gen)
            return tok

        for _ in range(a.warmup):
            tok = call()
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(a.iters):
            tok = call()
        t1.record()
        torch.cuda.synchronize()
        us = t0.elapsed_time(t1) * 1e3 / a.iters
        assert tok.shape == (B,) and int(tok.min()) >= 0 and int(tok.max()) < V
        launches = None
        try:
            from torch.profiler import ProfilerActivity, profile
            with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
                call()
                torch.cuda.synchronize()
            launches = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA
                           and "memcpy" not in e.name.lower() and "memset" not in e.name.lower())
        except Exception as e:  # noqa: BLE001 - the count is extra; the timing above stands without it
            print(f"bench_sample: launch count not taken: {e}", file=sys.stderr)
        print(json.dumps({"arm": a.arm, "B": B, "V": V, "dtype": "bf16", "setting": setting, "temperature": T,
                          "top_k": kw["top_k"], "top_p": kw["top_p"], "iters": a.iters,
                          "us_per_call": round(us, 1), "launches_per_call": launches}), flush=True)
    return 0


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--arm", choices=["fused", "torch"])
    ap.add_argument("--all", action="store_true")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    if a.all:
        for _ in range(a.rounds):
            for arm in ("torch", "fused"):
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--arm", arm, "--iters", str(a.iters),
                                    "--warmup", str(a.warmup)], timeout=300)
                if r.returncode != 0:
                    return r.returncode
        return 0
    if a.arm is None:
        ap.error("--arm or --all")
    return run_arm(a)


if __name__ == "__main__":
    sys.exit(main())
