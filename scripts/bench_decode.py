#!/usr/bin/env python
"""Decode attention at the Llama-3 shape (Hq 32, Hkv 8, D 128, bf16): one query row per head against a KV
cache, the split-KV kernel against what PyTorch offers.

  --arm native  ops.attention.decode_attention on cache[:, :len] with the device-side lengths
  --arm sdpa    F.scaled_dot_product_attention(q [B, Hq, 1, D], k, v [B, Hkv, len, D], enable_gqa=True) on the
                same slice of the same cache (a strided view, no copy); the ragged shape passes a boolean
                padding mask [B, 1, 1, Smax]

Shapes: B in {1, 8, 64} x uniform length in {2048, 8192}, and one ragged batch (B 64, lengths uniform in
[1, 8192], seeded). One process per arm runs every shape (run the arms alternately and compare the spread);
a call is timed with device events, the warm-up iterations are dropped, one JSON line is printed. A shape's
caches are allocated several times over (at least --rotate-mib of K and V together) and the calls walk them
in turn, as the layers of a model do, so no call finds its keys in the 256 MiB last-level cache left by the
call before. Bytes are counted from the lengths: K and V read once per kv head, 2 * sum(lens) * Hkv * D * 2.
Needs a GPU: there is no CPU fallback.

  --kv fp8      (native arm) the caches are FP8: e4m3fn codes plus one fp32 scale per (token, kv head), written by
                ops.attention.kv_cache_append; bytes are then 2 * sum(lens) * Hkv * (D + 4)
  --arm append  the cache write of one decode step (one new token per row) at B in {1, 8, 64}, cache length 2048:
                --kv bf16 times what Attention.decode does for a bf16 cache (.to and index_copy_ for k and for
                v), --kv fp8 the one quantising kv_cache_append that replaces them

  --paged PAGE  (native and append arms) the same keys in a paged cache of PAGE positions per page: every cache is
                cut into pages, the pages are stored in a seeded shuffled order (consecutive logical pages are not
                adjacent in memory) and reached through a block table: ops.attention.decode_attention_paged /
                kv_cache_append_paged. --arm append --kv bf16 --paged times the paged bf16 append kernel.

  python scripts/bench_decode.py --arm native --iters 50 --warmup 10
  python scripts/bench_decode.py --arm native --kv fp8
  python scripts/bench_decode.py --summary results.jsonl   # median and range over the processes, the gate
"""
import argparse
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HQ, HKV, D = 32, 8, 128
UNIFORM = [(b, n) for b in (1, 8, 64) for n in (2048, 8192)]
RAGGED = (64, 8192)
HBM_GBPS = 6300.0  # the achievable HBM rate the fractions are quoted against


def kv_bytes(lens, kv="bf16") -> int:
    return 2 * int(sum(lens)) * HKV * (D * 2 if kv == "bf16" else D + 4)


def _timed(fns, warmup, iters):
    import torch
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(warmup + iters)]
    for i, (s, e) in enumerate(ev):
        s.record()
        fns[i % len(fns)]()
        e.record()
    torch.cuda.synchronize()
    us = [s.elapsed_time(e) * 1e3 for s, e in ev[warmup:]]
    return statistics.median(us), min(us), max(us)


def summary(path: str) -> int:
    """per shape: median and range of the processes' medians per arm, GB/s and the fraction of the HBM rate,
    and the gate at the uniform shapes: the native median is not above SDPA's by more than the run-to-run
    range of the two arms (the sum of their half-ranges)"""
    runs = {"native": [], "sdpa": []}
    with open(path) as f:
        for line in f:
            line = line.strip()
            if line.startswith("{"):
                r = json.loads(line)
                runs[r["arm"]].append(r)
    if not runs["native"] or not runs["sdpa"]:
        raise SystemExit("bench_decode: the summary needs result lines of both arms")
    ok = True
    rows = []
    for name in [s["name"] for s in runs["native"][0]["shapes"]]:
        med = {arm: [next(s for s in r["shapes"] if s["name"] == name)["us_median"] for r in runs[arm]] for arm in runs}
        nbytes = next(s for s in runs["native"][0]["shapes"] if s["name"] == name)["kv_bytes"]
        m = {arm: statistics.median(v) for arm, v in med.items()}
        spread = sum((max(v) - min(v)) / 2 for v in med.values())
        gate = m["native"] <= m["sdpa"] + spread
        if not name.startswith("ragged"):
            ok = ok and gate
        row = {"shape": name, "kv_bytes": nbytes, "gate": gate, "time_ratio_native_over_sdpa": round(m["native"] / m["sdpa"], 3)}
        for arm in runs:
            gbps = nbytes / m[arm] / 1e3
            row[arm] = {"median_us": round(m[arm], 1), "min_us": round(min(med[arm]), 1), "max_us": round(max(med[arm]), 1),
                        "GBps": round(gbps, 1), "hbm_fraction": round(gbps / HBM_GBPS, 3)}
        rows.append(row)
    print(json.dumps({"processes": {k: len(v) for k, v in runs.items()}, "gate_uniform": ok, "shapes": rows}))
    return 0 if ok else 1


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--arm", choices=["native", "sdpa", "append"])
    ap.add_argument("--kv", choices=["bf16", "fp8"], default="bf16", help="the cache format (native and append arms)")
    ap.add_argument("--paged", type=int, default=0, metavar="PAGE", help="page size of a paged cache (0: contiguous)")
    ap.add_argument("--summary", metavar="JSONL", help="summarise the result lines of several processes")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rotate-mib", type=int, default=1024)
    a = ap.parse_args()
    if a.summary:
        return summary(a.summary)
    if a.arm is None:
        ap.error("--arm or --summary")
    if a.arm == "sdpa" and (a.kv != "bf16" or a.paged):
        ap.error("--arm sdpa reads contiguous bf16 caches only")
    if a.paged and (a.paged < 64 or a.paged % 64):
        ap.error("--paged: a positive multiple of 64")
    import torch
    import torch.nn.functional as F
    if not torch.cuda.is_available():
        raise SystemExit("bench_decode: needs a GPU")
    import cs744_pytorch_distributed_tutorial_amd as pkg
    pkg.ensure_hw_queues()
    from cs744_pytorch_distributed_tutorial_amd.ops import attention, native
    native.C()
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(0)
    scale = 1.0 / math.sqrt(D)
    out = []
    fp8 = a.kv == "fp8"

    def quantised(kc, vc):
        """(k codes, v codes, k scales, v scales) of a bf16 cache pair, through the append kernel"""
        B, n = kc.shape[:2]
        bufs = (torch.empty_like(kc, dtype=attention.FP8), torch.empty_like(vc, dtype=attention.FP8),
                torch.empty(B, n, HKV, device=dev), torch.empty(B, n, HKV, device=dev))
        attention.kv_cache_append(*bufs, kc, vc)
        return bufs

    def paged(bufs, table_out):
        """the tensors of one cache [B, n, ...] as pools [B * n / PAGE, PAGE, ...] in a shuffled page order; the
        block table int32 [B, n / PAGE] is written to table_out once (every cache of a shape shares it)"""
        B, n = bufs[0].shape[:2]
        C = n // a.paged
        perm = torch.randperm(B * C, generator=torch.Generator().manual_seed(B * C)).to(dev)
        if not table_out:
            where = torch.empty(B * C, dtype=torch.int64, device=dev)
            where[perm] = torch.arange(B * C, device=dev)  # pool[i] = page perm[i], so page j lies at where[j]
            table_out.append(where.view(B, C).int().contiguous())
        return tuple(t.reshape(B * C, a.paged, *t.shape[2:]).view(torch.uint8)[perm].view(t.dtype) for t in bufs)

    if a.arm == "append":
        n = 2048
        for B in (1, 8, 64):
            copies = 16  # the layers of a model: every call writes another cache
            k = torch.randn(B, 1, HKV, D, device=dev, generator=gen).bfloat16()
            v = torch.randn(B, 1, HKV, D, device=dev, generator=gen).bfloat16()
            pos = torch.randint(0, n, (B,), device=dev, generator=gen).int()
            slot = torch.arange(B, device=dev) * n + pos.long()
            caches = [(torch.zeros(B, n, HKV, D, device=dev).bfloat16(), torch.zeros(B, n, HKV, D, device=dev).bfloat16())
                      for _ in range(copies)]
            if fp8:
                caches = [quantised(kc, vc) for kc, vc in caches]
            if a.paged:
                table = []
                caches = [paged(c, table) for c in caches]
                table = table[0]
                assert attention.kv_append_paged_native_ok(*caches[0][:2], table, k, v, pos, None, *caches[0][2:])

                def mk(bufs):
                    sc = dict(k_scale=bufs[2], v_scale=bufs[3]) if fp8 else {}
                    return lambda: attention.kv_cache_append_paged(bufs[0], bufs[1], table, k, v, pos, **sc)
            elif fp8:
                assert attention.kv_append_native_ok(*caches[0], k, v, pos)

                def mk(bufs):
                    return lambda: attention.kv_cache_append(*bufs, k, v, pos)
            else:
                def mk(bufs):
                    kc, vc = bufs

                    def write():  # the cache write of models.llama.Attention.decode
                        kc.view(-1, HKV, D).index_copy_(0, slot, k.view(B, HKV, D).to(kc.dtype))
                        vc.view(-1, HKV, D).index_copy_(0, slot, v.view(B, HKV, D).to(vc.dtype))
                    return write
            with torch.no_grad():
                med, lo, hi = _timed([mk(c) for c in caches], a.warmup, a.iters)
            out.append({"name": f"append_B{B}", "B": B, "us_median": round(med, 1), "us_min": round(lo, 1),
                        "us_max": round(hi, 1)})
        print(json.dumps({"arm": a.arm, "kv": a.kv, "paged": a.paged, "kv_heads": HKV, "head_dim": D, "iters": a.iters,
                          "shapes": out}))
        return 0
    shapes = [(f"B{b}_L{n}", b, n, None) for b, n in UNIFORM]
    rag = torch.randint(1, RAGGED[1] + 1, (RAGGED[0],), generator=torch.Generator().manual_seed(1))
    shapes.append((f"ragged_B{RAGGED[0]}_L1..{RAGGED[1]}", RAGGED[0], RAGGED[1], rag))
    for name, B, n, ragged in shapes:
        per = kv_bytes([n] * B, a.kv)
        copies = max(1, min(64, -(-a.rotate_mib * 2**20 // per)))
        q = torch.randn(B, HQ, D, device=dev, generator=gen).bfloat16()
        caches = [(torch.randn(B, n, HKV, D, device=dev, generator=gen).bfloat16(),
                   torch.randn(B, n, HKV, D, device=dev, generator=gen).bfloat16()) for _ in range(copies)]
        host_lens = [n] * B if ragged is None else ragged.tolist()
        lens = torch.tensor(host_lens, dtype=torch.int32, device=dev)
        assert attention.decode_native_ok(q, *caches[0], lens)
        with torch.no_grad():  # the bf16 kernel's result: what every arm is compared with
            if fp8:  # on the dequantised first cache (its values are bf16 numbers), then the bf16 caches go
                ref = None
                for i, (kc, vc) in enumerate(caches):
                    caches[i] = quantised(kc, vc)
                    if ref is None:
                        deq = [attention.kv_dequantize(caches[0][j], caches[0][j + 2], torch.bfloat16) for j in (0, 1)]
                        ref = attention.decode_attention(q, *deq, lens, scale).float()
                        del deq
                    del kc, vc
                assert attention.decode_native_ok(q, *caches[0][:2], lens, *caches[0][2:])
            else:
                ref = attention.decode_attention(q, *caches[0], lens, scale).float()
        if a.arm == "native" and a.paged:
            table = []
            for i in range(len(caches)):
                caches[i] = paged(caches[i], table)
            table = table[0]
            assert attention.decode_paged_native_ok(q, *caches[0][:2], table, lens, *caches[0][2:])

            def mk(kp, vp, ks=None, vs=None):
                return lambda: attention.decode_attention_paged(q, kp, vp, table, lens, scale, k_scale=ks, v_scale=vs)
        elif a.arm == "native" and fp8:
            def mk(kc, vc, ks, vs):
                return lambda: attention.decode_attention(q, kc, vc, lens, scale, k_scale=ks, v_scale=vs)
        elif a.arm == "native":
            def mk(kc, vc):
                return lambda: attention.decode_attention(q, kc, vc, lens, scale)
        else:
            q4 = q.view(B, HQ, 1, D)
            mask = None
            if ragged is not None:
                mask = (torch.arange(n, device=dev).view(1, n) < lens.view(B, 1)).view(B, 1, 1, n)

            def mk(kc, vc):
                k4, v4 = kc.transpose(1, 2), vc.transpose(1, 2)
                return lambda: F.scaled_dot_product_attention(q4, k4, v4, attn_mask=mask, scale=scale, enable_gqa=True)
        fns = [mk(*c) for c in caches]
        with torch.no_grad():
            # the arms compute the same thing
            got = fns[0]().reshape(B, HQ, D).float()
            err = (got - ref).abs().max().item()
            assert err < 0.05, f"{name}: the arms disagree by {err}"
            med, lo, hi = _timed(fns, a.warmup, a.iters)
        nbytes = kv_bytes(host_lens, a.kv)
        out.append({"name": name, "B": B, "len": n, "ragged": ragged is not None, "copies": copies,
                    "splits": native.C().decode_splits(B, HKV, n), "us_median": round(med, 1), "us_min": round(lo, 1),
                    "us_max": round(hi, 1), "kv_bytes": nbytes, "GBps": round(nbytes / med / 1e3, 1), "max_abs_diff": err})
        del caches, fns
    print(json.dumps({"arm": a.arm, "kv": a.kv, "paged": a.paged, "heads": HQ, "kv_heads": HKV, "head_dim": D, "iters": a.iters, "shapes": out}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
