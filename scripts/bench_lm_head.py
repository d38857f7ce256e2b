#!/usr/bin/env python
"""The LM head (output projection + cross-entropy) at the Llama-3 shape, unfused against the chunked
head of ops.lm.linear_cross_entropy: time of forward + backward and peak allocated bytes.

  --arm unfused        head(h) + ops.lm.cross_entropy: the full [rows, vocab] logits and their gradient
  --arm fused          ops.lm.linear_cross_entropy with --chunk-mb MiB of logits per chunk
  --arm kernel-pair    _C.xent_fwd_masked + _C.xent_bwd_masked over --chunk-mb chunks of one logits matrix
  --arm kernel-fused   _C.xent_count + _C.xent_fused_ (in place) + _C.xent_reduce over the same chunks;
                       both kernel arms move the same bytes: two reads and one write of the matrix
  --arm step           TorchTrainer(--model, bf16) steps with --fused-head 0 / 1: step time and peak
                       memory of the whole training step

One process per arm. ``--all`` (the head arms) and ``--all-kernels`` start one fresh child process per
arm, the arms alternating over --rounds rounds, stop at the first child that fails, and print per arm
the median of the process medians and their range. Times are device events around work ending in a
synchronise, warm-up iterations dropped; bytes are counted from the shapes. Needs a GPU.

  python scripts/bench_lm_head.py --all --rounds 3
  python scripts/bench_lm_head.py --arm fused --chunk-mb 256
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _timed(fn, warmup, iters, prep=None):
    """``prep`` runs before every iteration, outside its pair of events"""
    import torch
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(warmup + iters)]
    for i, (s, e) in enumerate(ev):
        if i == warmup:
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
        if prep is not None:
            prep()
        s.record()
        fn()
        e.record()
    torch.cuda.synchronize()
    ms = [s.elapsed_time(e) for s, e in ev[warmup:]]
    return statistics.median(ms), min(ms), max(ms)


def _head_arm(a):
    import torch
    from cs744_pytorch_distributed_tutorial_amd.ops import lm
    dev = torch.device("cuda", 0)
    R, D, V = a.rows, a.dim, a.vocab
    gen = torch.Generator(device=dev).manual_seed(0)
    h = torch.randn(R, D, device=dev, generator=gen).bfloat16()
    t = torch.randint(0, V, (R,), device=dev, generator=gen)
    head = lm.ShadowLinear(D, V, bias=False).to(dev)
    torch.nn.init.normal_(head.weight, 0.0, 0.02)
    head._shadow()
    base = torch.cuda.memory_allocated()
    chunk = lm.head_chunk_rows(R, V, 2)
    hf = h.detach().requires_grad_()
    out = {}

    def run():
        hf.grad = None
        head.weight.grad = None
        with torch.autocast("cuda", dtype=torch.bfloat16):
            if a.arm == "fused":
                loss = lm.linear_cross_entropy(hf, head, t, chunk_rows=chunk)
            else:
                loss = lm.cross_entropy(head(hf).view(-1, V), t)
        loss.backward()
        out["loss"] = loss.detach()

    med, lo, hi = _timed(run, a.warmup, a.iters)
    peak = torch.cuda.max_memory_allocated() - base
    return {"arm": a.arm, "rows": R, "dim": D, "vocab": V, "chunk_mb": a.chunk_mb if a.arm == "fused" else None,
            "chunk_rows": chunk if a.arm == "fused" else None, "iters": a.iters, "fwd_bwd_ms_median": round(med, 3),
            "fwd_bwd_ms_min": round(lo, 3), "fwd_bwd_ms_max": round(hi, 3), "peak_alloc_GB": round(peak / 1e9, 3),
            "loss": round(float(out["loss"]), 6)}


def _kernel_arm(a):
    import torch
    from cs744_pytorch_distributed_tutorial_amd import _C
    dev = torch.device("cuda", 0)
    R, V = a.rows, a.vocab
    gen = torch.Generator(device=dev).manual_seed(0)
    x = torch.empty(R, V, dtype=torch.bfloat16, device=dev)
    for lo in range(0, R, 1024):  # filled a slab at a time: no fp32 copy of the whole matrix
        x[lo:lo + 1024] = (torch.randn(min(1024, R - lo), V, device=dev, generator=gen) * 3).bfloat16()
    t = torch.randint(0, V, (R,), device=dev, generator=gen)
    from cs744_pytorch_distributed_tutorial_amd.ops import lm
    chunk = lm.head_chunk_rows(R, V, 2)
    g = torch.ones(1, device=dev)
    work = x.clone()  # the fused kernel overwrites its input: restored from x before every iteration, untimed
    loss, lse = torch.empty(R, device=dev), torch.empty(R, device=dev)

    if a.arm == "kernel-pair":
        def run():
            for r0 in range(0, R, chunk):
                xc = x[r0:r0 + chunk]
                _, l, st = _C.xent_fwd_masked(xc, t[r0:r0 + chunk], -100, a.z)
                _C.xent_bwd_masked(xc, t[r0:r0 + chunk], l, st, g, -100, a.z)
    else:
        def run():
            st = _C.xent_count(t, -100)
            for r0 in range(0, R, chunk):
                _C.xent_fused_(work[r0:r0 + chunk], t, loss, lse, st, r0, -100, a.z)
            _C.xent_reduce(loss, t, -100, st)

    # both arms read the same logits in every iteration (and both follow a full write of a matrix of that size)
    med, lo, hi = _timed(run, a.warmup, a.iters, prep=lambda: work.copy_(x))
    nbytes = 3 * R * V * 2
    return {"arm": a.arm, "rows": R, "vocab": V, "chunk_rows": chunk, "z": a.z, "iters": a.iters,
            "ms_median": round(med, 3), "ms_min": round(lo, 3), "ms_max": round(hi, 3), "bytes": nbytes,
            "GBps": round(nbytes / med / 1e6, 1)}


def _step_arm(a):
    import torch
    from cs744_pytorch_distributed_tutorial_amd.runtime.torch_trainer import TorchTrainer
    dev = torch.device("cuda", 0)
    tr = TorchTrainer(a.model, a.batch_size, dev, dtype="bf16", seq_len=a.seq_len, fused_head=bool(a.fused_head))
    med, lo, hi = _timed(tr.step, a.warmup, a.iters)
    return {"arm": "step", "model": a.model, "batch": a.batch_size, "seq_len": a.seq_len, "fused_head": bool(a.fused_head),
            "chunk_mb": os.environ.get("CS_LM_HEAD_CHUNK_MB"), "step_ms_median": round(med, 2),
            "step_ms_min": round(lo, 2), "step_ms_max": round(hi, 2),
            "peak_alloc_GB": round(torch.cuda.max_memory_allocated() / 1e9, 3), "loss": round(tr.last_loss(), 4)}


def _drive(a, arms, key):
    """one fresh child per arm and round, alternating; stops at the first failure"""
    runs = {}
    for rnd in range(a.rounds):
        for name, extra in arms:
            cmd = [sys.executable, os.path.abspath(__file__), "--rows", str(a.rows), "--dim", str(a.dim), "--vocab",
                   str(a.vocab), "--iters", str(a.iters), "--warmup", str(a.warmup), "--z", str(a.z), *extra]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.child_timeout)
            if r.returncode != 0:
                print(r.stdout + r.stderr, file=sys.stderr)
                raise SystemExit(f"bench_lm_head: arm {name} failed with exit code {r.returncode}; stopping")
            rec = json.loads(r.stdout.strip().splitlines()[-1])
            rec["round"] = rnd
            print(json.dumps(rec), flush=True)
            runs.setdefault(name, []).append(rec)
    for name, recs in runs.items():
        meds = [r[key] for r in recs]
        line = {"summary": name, "median_of_process_medians_ms": round(statistics.median(meds), 3),
                "range_ms": [min(meds), max(meds)]}
        if "peak_alloc_GB" in recs[0]:
            line["peak_alloc_GB"] = recs[0]["peak_alloc_GB"]
        print(json.dumps(line), flush=True)
    return 0


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--arm", choices=["unfused", "fused", "kernel-pair", "kernel-fused", "step"])
    ap.add_argument("--all", action="store_true", help="unfused and fused at 128 / 256 / 512 / 1024 MiB chunks")
    ap.add_argument("--all-kernels", action="store_true", help="kernel-pair and kernel-fused")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--rows", type=int, default=16384)
    ap.add_argument("--dim", type=int, default=4096)
    ap.add_argument("--vocab", type=int, default=128256)
    ap.add_argument("--chunk-mb", type=float, default=None, help="MiB of logits per chunk (default: CS_LM_HEAD_CHUNK_MB)")
    ap.add_argument("--z", type=float, default=0.0)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--model", type=str, default="llama3-8b")
    ap.add_argument("--batch-size", type=int, default=8)
    ap.add_argument("--seq-len", type=int, default=2048)
    ap.add_argument("--fused-head", type=int, default=0)
    ap.add_argument("--child-timeout", type=float, default=300.0)
    a = ap.parse_args()
    if a.all or a.all_kernels:  # the parent never touches the GPU: every arm is a fresh process
        if a.all:
            arms = [("unfused", ["--arm", "unfused"])] + [(f"fused-{mb}", ["--arm", "fused", "--chunk-mb", str(mb)])
                                                          for mb in (128, 256, 512, 1024)]
            return _drive(a, arms, "fwd_bwd_ms_median")
        arms = [("kernel-pair", ["--arm", "kernel-pair", "--chunk-mb", str(a.chunk_mb or 256)]),
                ("kernel-fused", ["--arm", "kernel-fused", "--chunk-mb", str(a.chunk_mb or 256)])]
        return _drive(a, arms, "ms_median")
    if a.arm is None:
        ap.error("give --arm, --all or --all-kernels")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_lm_head: needs a GPU")
    import cs744_pytorch_distributed_tutorial_amd as pkg
    pkg.ensure_hw_queues()
    if a.chunk_mb is not None:  # the library's own rule turns it into rows (ops.lm.head_chunk_rows)
        os.environ["CS_LM_HEAD_CHUNK_MB"] = str(a.chunk_mb)
    fn = {"unfused": _head_arm, "fused": _head_arm, "kernel-pair": _kernel_arm, "kernel-fused": _kernel_arm,
          "step": _step_arm}[a.arm]
    print(json.dumps(fn(a)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
