"""Extend attention off the GPU: ops.attention.extend_attention_ref / extend_attention_paged_ref against the float64
loop of tests/extend_oracle.py with NaN at every stale position, on every unowned page and behind an invalid table
entry inside the visible range; Llama.extend, prefill(chunk=) and generate(prefill_chunk=) on llama-tiny against the
full forward and the one-shot prefill, through a slab, an FP8 slab, a paged pool and a paged FP8 pool; and the host
bookkeeping and refusals of Llama.extend."""
import copy
import functools

import pytest
import torch

from extend_oracle import (clamp_bounds, extend_oracle64, model_scenarios, nan_stale_, paged_case, stale_, worst)
from kv_paged_oracle import scatter_to_pages

CPU = torch.device("cpu")
F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
KINDS = ["slab", "slab_fp8", "paged", "paged_fp8"]


def _att():
    from cs744_pytorch_distributed_tutorial_amd.ops import attention
    return attention


# ------------------------------------------------------------------ the reference ops
B, T, HQ, HKV, D, PAGE, SMAX = 5, 7, 4, 2, 64, 64, 128
START = [0, 3, 60, 125, 64]   # row 3: start + T > Smax, its counts are clamped to 3
COUNTS = [7, 0, 5, 7, 1]      # row 1 takes nothing; row 4 one token on the first row of its second page


@functools.lru_cache(maxsize=None)
def _ref_case(cache_kind):
    """q fp64, the caches' values fp64 (bf16-rounded, or what an FP8 cache dequantises to) with NaN where stale, the
    caches as the ops take them, and the pools / tables without and with an invalid entry in row 2's visible range"""
    att = _att()
    g = torch.Generator().manual_seed(21)
    q = torch.randn(B, T, HQ, D, generator=g, dtype=F64)
    k = torch.randn(B, SMAX, HKV, D, generator=g).to(BF16)
    v = (torch.randn(B, SMAX, HKV, D, generator=g) * 2).to(BF16)
    if cache_kind == "fp8":
        (kc, ks), (vc, vs) = att.kv_quantize_ref(k), att.kv_quantize_ref(v)
        k64, v64 = att.kv_dequantize(kc, ks, F64), att.kv_dequantize(vc, vs, F64)
        st, cn = clamp_bounds(START, COUNTS, T, SMAX)
        for b in range(B):  # stale: the NaN code and a NaN scale
            kc.view(torch.uint8)[b, st[b] + cn[b]:] = 0x7F
            vc.view(torch.uint8)[b, st[b] + cn[b]:] = 0x7F
        nan_stale_(ks, vs, START, COUNTS, T)
        slab = (kc, vc, ks, vs)
    else:
        k64, v64 = k.double(), v.double()
        nan_stale_(k, v, START, COUNTS, T)
        slab = (k, v)
    pools = {}
    for name, hole in (("whole", None), ("hole", (2, 0))):
        kp, vp, table, key_ok = paged_case(slab[0], slab[1], START, COUNTS, T, PAGE, seed=5, hole=hole)
        sc = ()
        if cache_kind == "fp8":
            lens = [s + c for s, c in zip(*clamp_bounds(START, COUNTS, T, SMAX))]
            P = kp.shape[0]
            sc = (scatter_to_pages(slab[2], table, lens, P, PAGE), scatter_to_pages(slab[3], table, lens, P, PAGE))
        pools[name] = (kp, vp, table, key_ok, sc)
    return q, k64, v64, slab, pools


@pytest.mark.parametrize("ct", [F32, F64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("cache_kind", ["bf16", "fp8"])
def test_refs_against_float64_loop(cache_kind, ct):
    """The references round like any ct matmul: a score is a D-term sum, an output a sum over at most Smax keys of
    weights that add up to one, so the error is within (Smax + D) ulp of the largest visible |v|."""
    att = _att()
    q, k64, v64, slab, pools = _ref_case(cache_kind)
    start, counts = torch.tensor(START, dtype=torch.int32), torch.tensor(COUNTS, dtype=torch.int32)
    st, cn = clamp_bounds(START, COUNTS, T, SMAX)
    assert cn == [7, 0, 5, 3, 1]
    vmax = max(v64[b, :st[b] + cn[b]].abs().max().item() for b in range(B) if cn[b])
    tol = (SMAX + D) * (2.0 ** -24 if ct == F32 else 2.0 ** -53) * vmax
    sc = dict(k_scale=slab[2], v_scale=slab[3]) if cache_kind == "fp8" else {}
    qc = q.to(ct)

    def check(o, o64, what):
        assert o.dtype == ct and o.shape == (B, T, HQ, D)
        assert torch.isfinite(o).all(), what
        for b in range(B):
            assert torch.equal(o[b, cn[b]:], torch.zeros(T - cn[b], HQ, D, dtype=ct)), f"{what}: padded rows of {b}"
        err = (o.double() - o64).abs().max().item()
        print(f"{what} ({cache_kind}, {ct}): max err {err:.3e}, bound {tol:.3e}")
        assert err <= tol, what

    o64 = extend_oracle64(qc, k64, v64, START, COUNTS)
    check(att.extend_attention_ref(qc, slab[0], slab[1], start, counts, **sc), o64, "contiguous")
    # the public op off the GPU is the reference
    assert not att.extend_native_ok(qc, slab[0], slab[1], start, counts, **sc)
    assert torch.equal(att.extend_attention(qc, slab[0], slab[1], start, counts, **sc),
                       att.extend_attention_ref(qc, slab[0], slab[1], start, counts, **sc))
    for name in ("whole", "hole"):
        kp, vp, table, key_ok, psc = pools[name]
        kw = dict(k_scale=psc[0], v_scale=psc[1]) if psc else {}
        want = o64 if name == "whole" else extend_oracle64(qc, k64, v64, START, COUNTS, key_ok=key_ok)
        got = att.extend_attention_paged_ref(qc, kp, vp, table, start, counts, **kw)
        check(got, want, f"paged, {name}")
        assert not att.extend_paged_native_ok(qc, kp, vp, table, start, counts, **kw)
        assert torch.equal(att.extend_attention_paged(qc, kp, vp, table, start, counts, **kw), got)
    # the hole hides keys 0 .. 63 of row 2: its queries at positions 60 .. 63 see nothing, the one at 64 one key
    hole = att.extend_attention_paged_ref(qc, *pools["hole"][:3], start, counts,
                                          **(dict(k_scale=pools["hole"][4][0], v_scale=pools["hole"][4][1])
                                             if cache_kind == "fp8" else {}))
    assert torch.equal(hole[2, :4], torch.zeros(4, HQ, D, dtype=ct))
    assert torch.equal(hole[2, 4].double(), v64[2, 64].repeat_interleave(HQ // HKV, dim=0).to(ct).double())


def test_counts_default_clamps_and_scale():
    att = _att()
    q, k64, v64, slab, _ = _ref_case("bf16")
    k, v = slab
    start = torch.tensor(START, dtype=torch.int32)
    # counts=None is T, clamped by Smax - start: stale NaN rows are in range now, so use a clean cache
    kc, vc = torch.nan_to_num(k.double()), torch.nan_to_num(v.double())
    a = att.extend_attention_ref(q, kc, vc, start)
    b = att.extend_attention_ref(q, kc, vc, start, torch.full((B,), T + 100))
    assert torch.equal(a, b)
    assert (a - extend_oracle64(q, kc, vc, START, None)).abs().max() < 1e-13
    # start outside [0, Smax] is clamped: below to 0, above to Smax (no live query)
    wild = torch.tensor([-5, SMAX + 9, 60, 125, 64], dtype=torch.int32)
    c = att.extend_attention_ref(q, kc, vc, wild)
    assert torch.equal(c[0], a[0]) and torch.equal(c[1], torch.zeros_like(c[1]))
    s = att.extend_attention_ref(q, kc, vc, start, scale=0.3)
    assert (s - extend_oracle64(q, kc, vc, START, None, scale=0.3)).abs().max() < 1e-13


def test_refusals():
    att = _att()
    q, _, _, slab, pools = _ref_case("bf16")
    f8 = _ref_case("fp8")[3]
    start = torch.tensor(START, dtype=torch.int32)
    k, v = slab
    with pytest.raises(ValueError, match="need k_scale and v_scale"):
        att.extend_attention(q, f8[0], f8[1], start)
    with pytest.raises(ValueError, match="float8_e4m3fn caches only"):
        att.extend_attention(q, k, v, start, k_scale=f8[2], v_scale=f8[3])
    with pytest.raises(ValueError, match="does not go with"):
        att.extend_attention(q[:, :, :3], k, v, start)  # Hq 3 against Hkv 2
    with pytest.raises(ValueError, match="does not go with"):
        att.extend_attention(q[:3], k, v, start[:3])
    with pytest.raises(ValueError, match="start must be an integer"):
        att.extend_attention(q, k, v, start.float())
    with pytest.raises(ValueError, match="counts must be an integer"):
        att.extend_attention(q, k, v, start, torch.ones(B + 1, dtype=torch.int32))
    kp, vp, table = pools["whole"][:3]
    with pytest.raises(ValueError, match="multiple of 64"):
        att.extend_attention_paged(q, kp[:, :48], vp[:, :48], table, start)
    with pytest.raises(ValueError, match="block_table must be an integer"):
        att.extend_attention_paged(q, kp, vp, table.float(), start)
    for i in range(3):
        ts = [q.clone(), torch.nan_to_num(k.float()), torch.nan_to_num(v.float())]
        ts[i].requires_grad_()
        with pytest.raises(RuntimeError, match="inference only"):
            att.extend_attention(*ts, start)
        with pytest.raises(RuntimeError, match="inference only"):
            att.extend_attention_ref(*ts, start)


# ------------------------------------------------------------------ the model
BM, S, LENS, CHUNKS = 2, 24, (5, 11), (1, 5, 24)


def _tiny(qk_norm=False, seed=0, dtype=F32):
    from cs744_pytorch_distributed_tutorial_amd.models import llama
    torch.manual_seed(seed)
    m = llama.build("llama-tiny", qk_norm=qk_norm).to(dtype).eval()
    if qk_norm:  # gains away from 1, so a norm that is skipped on one path shows
        with torch.no_grad():
            for blk in m.layers:
                blk.attention.q_norm.weight.uniform_(0.5, 1.5)
                blk.attention.k_norm.weight.uniform_(0.5, 1.5)
    return m


def _maker(att, cfg, kind, dtype, Bn=BM, max_len=S, pages=None):
    fp8 = kind.endswith("fp8")
    dt = att.FP8 if fp8 else dtype

    def make():
        if kind.startswith("slab"):
            return stale_(att.KVCache.allocate(cfg, Bn, max_len, CPU, dt))
        return stale_(att.PagedKVCache.allocate(cfg, Bn, Bn + 1 if pages is None else pages, 64, None, CPU, dt))
    return make


@functools.lru_cache(maxsize=None)
def _model_case(qk_norm, kind):
    """the scenarios of tests/extend_oracle.py through the fp32 model, the float64 copy's full forward, the fp32
    model's, and for an FP8 cache e_q per scenario: what the float64 copy itself loses through such a cache"""
    att = _att()
    m = _tiny(qk_norm)
    m64 = copy.deepcopy(m).double()
    tokens = torch.randint(1, m.cfg.vocab_size, (BM, S), generator=torch.Generator().manual_seed(4))
    with torch.no_grad():
        ref, full = m64(tokens), m(tokens)
    got = model_scenarios(m, tokens, LENS, _maker(att, m.cfg, kind, F32), CHUNKS)
    e_q = {}
    if kind.endswith("fp8"):
        got64 = model_scenarios(m64, tokens, LENS, _maker(att, m.cfg, kind, F64), CHUNKS)
        e_q = {name: worst(rows, ref) for name, (rows, _) in got64.items() if rows}
    return m, ref, full, got, e_q


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("qk_norm", [False, True], ids=["plain", "qk_norm"])
def test_model_logits(qk_norm, kind):
    """Every cached path's logits against the full forward's, both measured against a float64 copy of the model: the
    fp32 paths differ only in summation order, so a cached path may err at most 4x what the full forward errs (the
    bound of tests/test_decode_cpu.py). An FP8 cache adds its quantisation, for which no tolerance can be derived
    (tests/test_kv_fp8_gpu.py): the yardstick is e_q, what the float64 copy loses through the same cache on the
    same path, counted twice for codes that a rounding ahead of the quantiser moves by a step."""
    m, ref, full, got, e_q = _model_case(qk_norm, kind)
    for name in [f"chunk{n}" for n in CHUNKS] + ["extend_all", "second_turn"]:
        rows, _ = got[name]
        e = worst(rows, ref)
        e_full = max((full[b, t].double() - ref[b, t]).abs().max().item() for b, t, _ in rows)
        print(f"{name} ({kind}, qk_norm={qk_norm}): cached {e:.3e}, full forward {e_full:.3e}, "
              f"e_q {e_q.get(name, 0.0):.3e}")
        assert e_full > 0
        assert torch.isfinite(torch.stack([lg for _, _, lg in rows])).all()
        assert e <= 4 * e_full + 2 * e_q.get(name, 0.0), name
    want = sorted((b, t) for b in range(BM) for t in range(min(LENS), S))
    assert sorted((b, t) for b, t, _ in got["extend_all"][0]) == want


def _visible_kv(att, cache, lens):
    """[(k, v)] per row: the visible positions of every layer, dequantised, [n_layers, len, Hkv, hd] float64"""
    out = []
    paged = hasattr(cache, "block_table")
    for b, n in enumerate(lens):
        per = []
        for t, sc in ((cache.k, cache.k_scale), (cache.v, cache.v_scale)):
            layers = []
            for l in range(t.shape[0]):
                x = att.paged_gather(t[l], cache.block_table)[b, :n] if paged else t[l, b, :n]
                if sc is not None:
                    s = att.paged_gather(sc[l], cache.block_table)[b, :n] if paged else sc[l, b, :n]
                    x = att.kv_dequantize(x, s, F64)
                layers.append(x.double())
            per.append(torch.stack(layers))
        out.append(tuple(per))
    return out


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("qk_norm", [False, True], ids=["plain", "qk_norm"])
def test_chunked_prefill_cache_and_state(qk_norm, kind):
    """prefill(chunk=n) leaves what the one-shot prefill leaves: the lengths and bounds exactly, the visible k and v
    within fp32 GEMM rounding: a projection is a sum of dim = 256 products, so 256 ulp of the largest entry (layer 0
    sees the same inputs on both paths; layer 1's differ by the attention's summation order). An FP8 cache may in
    addition hold a neighbouring code where that rounding crosses a boundary of the quantiser: one step of e4m3,
    2^-3 of the row's largest entry."""
    att = _att()
    m, _, _, got, _ = _model_case(qk_norm, kind)
    one = got["one_shot"][1]
    want = _visible_kv(att, one, LENS)
    for n in CHUNKS:
        cache = got[f"chunk{n}"][1]
        assert cache.lens.tolist() == list(LENS) and cache.lens.dtype == torch.int32
        assert cache.bound == max(LENS) == one.bound
        if kind.startswith("paged"):
            assert cache.row_bound == list(LENS) == one.row_bound
            assert cache.pages_in_use == att.PagedKVCache.pages_needed(LENS, 0, 64) == one.pages_in_use
        for (k, v), (k1, v1) in zip(_visible_kv(att, cache, LENS), want):
            for a, b in ((k, k1), (v, v1)):
                assert torch.isfinite(a).all()
                top = b.abs().max().item()
                tol = 2.0 ** -16 * top + (2.0 ** -3 * top if kind.endswith("fp8") else 0.0)
                err = (a - b).abs().max().item()
                assert err <= tol, f"chunk {n}: cache differs by {err:.3e} (bound {tol:.3e})"


@pytest.mark.parametrize("kind", KINDS)
def test_state_after_extend(kind):
    att = _att()
    m, _, _, got, _ = _model_case(False, kind)
    cache = got["second_turn"][1]
    lens, bound = got["second_turn_state"][1]
    assert cache.lens.tolist() == lens and cache.lens.dtype == torch.int32 and cache.bound == bound
    if kind.startswith("paged"):
        assert cache.row_bound == lens  # host counts: the rows' own growth
    cache = got["extend_all"][1]
    assert cache.lens.tolist() == [S] * BM and cache.bound == S
    # counts as a list, as a host tensor and absent agree; a row with counts 0 keeps its length and stays finite
    tokens = torch.randint(1, m.cfg.vocab_size, (BM, 4), generator=torch.Generator().manual_seed(8))
    outs = []
    for counts in ([4, 4], torch.tensor([4, 4]), None):
        c = _maker(att, m.cfg, kind, F32)()
        m.prefill(tokens, c)
        outs.append(m.extend(tokens, c, counts))
        assert c.lens.tolist() == [8, 8] and c.bound == 8
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    c = _maker(att, m.cfg, kind, F32)()
    m.prefill(tokens, c)
    lg = m.extend(tokens, c, [0, 3])
    assert lg.shape == (BM, m.cfg.vocab_size) and torch.isfinite(lg).all()
    assert c.lens.tolist() == [4, 7] and c.bound == 8
    if kind.startswith("paged"):
        assert c.row_bound == [4, 7]
    # an empty cache is allowed: extend from nothing is a prefill
    c = _maker(att, m.cfg, kind, F32)()
    if kind.startswith("paged"):
        for b in range(BM):
            c.reserve(b, 4)
        c.commit()
    lg = m.extend(tokens, c)
    if not kind.endswith("fp8"):
        with torch.no_grad():
            assert (lg - m(tokens)[:, -1]).abs().max() < 1e-4
    assert c.lens.tolist() == [4, 4]


def test_refusals_of_llama_extend():
    att = _att()
    m = _tiny()
    tokens = torch.randint(1, m.cfg.vocab_size, (BM, 6), generator=torch.Generator().manual_seed(9))
    slab = att.KVCache.allocate(m.cfg, BM, 10, CPU, F32)
    m.prefill(tokens, slab)
    with pytest.raises(ValueError, match="exceed the cache's 10 positions"):
        m.extend(tokens[:, :5], slab)
    assert slab.bound == 6 and slab.lens.tolist() == [6, 6]  # nothing happened
    m.extend(tokens[:, :4], slab)
    assert slab.bound == 10
    with pytest.raises(ValueError, match=r"\[B, T\]"):
        m.extend(tokens[0], slab)
    with pytest.raises(ValueError, match="does not take"):
        m.extend(tokens[:1], slab)
    pool = att.PagedKVCache.allocate(m.cfg, BM, 4, 64, None, CPU, F32)
    m.prefill(torch.cat([tokens] * 10, 1), pool, [60, 20])  # one page each
    with pytest.raises(ValueError, match=r"slot 0 holds 64 positions and needs 66: call cache.reserve\(0, n\)"):
        m.extend(tokens, pool)
    assert pool.pages_in_use == 2 and pool.row_bound == [60, 20]  # never allocates behind the caller's back
    m.extend(tokens, pool, [4, 6])  # 64 and 26: fits
    assert pool.row_bound == [64, 26] and pool.lens.tolist() == [64, 26] and pool.bound == 66
    pool.reserve(0, 70)
    pool.commit()
    m.extend(tokens, pool)
    assert pool.row_bound == [70, 32] and pool.pages_in_use == 3
    with pytest.raises(ValueError, match="chunk must be at least 1"):
        m.prefill(tokens, slab, chunk=0)
    with pytest.raises(ValueError, match="doc_ids"):
        m.prefill(tokens, slab, doc_ids=torch.zeros_like(tokens), chunk=2)


def test_generate_with_prefill_chunk():
    """greedy tokens in fp32 on the CPU: the chunked prefill changes the summation order only"""
    m = _tiny(seed=6)
    tokens = torch.randint(1, m.cfg.vocab_size, (3, 9), generator=torch.Generator().manual_seed(9))
    lens = torch.tensor([4, 9, 7])
    with torch.no_grad():  # a near-tie would make the comparison meaningless: an input failure, shown, not skipped
        top = m(tokens)[torch.arange(3), lens - 1].topk(2).values
    assert (top[:, 0] - top[:, 1]).min() > 1e-4
    want = m.generate(tokens, 7, prompt_lens=lens)
    for n in (1, 4, 9, 50):
        assert torch.equal(m.generate(tokens, 7, prompt_lens=lens, prefill_chunk=n), want)
    assert torch.equal(m.generate(tokens, 7, prompt_lens=lens, page_size=64, prefill_chunk=4),
                       m.generate(tokens, 7, prompt_lens=lens, page_size=64))
    assert torch.equal(m.generate(tokens, 7, prompt_lens=lens, page_size=64, prefill_chunk=4), want)


def test_chunked_paged_prefill_takes_exactly_the_pages_needed():
    att = _att()
    m = _tiny()
    lens = [1, 64, 65, 100]
    tokens = torch.randint(1, m.cfg.vocab_size, (4, 100), generator=torch.Generator().manual_seed(10))
    pool = att.PagedKVCache.allocate(m.cfg, 4, 9, 64, None, CPU, F32)
    seen = []
    reserve = pool.reserve
    pool.reserve = lambda b, n: (reserve(b, n), seen.append(pool.pages_in_use))[0]
    m.prefill(tokens, pool, lens, chunk=48)
    need = att.PagedKVCache.pages_needed(lens, 0, 64)
    assert need == 6 and pool.pages_in_use == need
    assert pool.row_bound == lens and pool.lens.tolist() == lens and pool.bound == 100
    # the pool grew chunk by chunk: after the first chunk's reservations one page per row
    assert seen[3] == 4 and seen[-1] == need
