"""Extend attention on the GPU (attn_extend, ops.attention.extend_attention / extend_attention_paged) against the
float64 loop of tests/extend_oracle.py on the bf16-rounded inputs: ragged starts around the key tile and counts with
padding, NaN at every stale position, on every unowned page and in every last page's tail, a row that overflows the
cache, sliced caches, pages of one and two key tiles, an invalid table entry inside the visible range, the paged
kernel's bits against the contiguous kernel's, determinism, the flash forward and the decode kernel as cross-checks,
FP8 caches through the public op, the bindings' host checks, and Llama.extend / prefill(chunk=) under bf16 autocast
(MI355X only)."""
import copy
import functools

import pytest
import torch

from decode_oracle import decode_oracle64
from extend_oracle import (clamp_bounds, extend_oracle64, model_scenarios, nan_stale_, paged_case, rel_l2, stale_,
                           worst)
from kv_paged_oracle import scatter_to_pages

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
O_TOL = 8e-3  # the flash forward's bound (tests/test_attention_gpu.py): bf16 P, fp32 accumulate, bf16 out
HEADS = [(4, 4), (4, 2), (8, 1)]
TS = [1, 33, 128, 129]
STARTS = [0, 1, 63, 64, 65, 191]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cs744_pytorch_distributed_tutorial_amd.ops import native
    native.C()
    return torch.device("cuda", 0)


def _C():
    from cs744_pytorch_distributed_tutorial_amd import _C
    return _C


def _att():
    from cs744_pytorch_distributed_tutorial_amd.ops import attention
    return attention


@pytest.fixture
def no_ref(monkeypatch):
    """the native paths must run: the references raise"""
    def boom(*a, **kw):
        raise AssertionError("extend attention fell back to the reference")
    monkeypatch.setattr(_att(), "extend_attention_ref", boom)
    monkeypatch.setattr(_att(), "extend_attention_paged_ref", boom)
    return monkeypatch


@functools.lru_cache(maxsize=None)
def _case(D, Hq, Hkv, T):
    """Host operands, computed once and never changed: four rows, three with starts from STARTS (rotating with the
    case) and counts from {0, 1, T - 1, T}, the fourth at Smax - T // 2 with counts T (start + T > Smax: clamped);
    bf16 q, k, v with NaN at every stale position; the float64 oracle."""
    idx = TS.index(T) + 4 * HEADS.index((Hq, Hkv)) + (12 if D == 128 else 0)
    Smax = 384 if T >= 128 else 256
    start = [STARTS[(idx + j) % 6] for j in (0, 2, 3)] + [Smax - T // 2]
    pick = [T, T - 1, 1, 0]
    counts = [pick[(idx + j) % 4] for j in range(3)] + [T]
    if T not in counts[:3]:
        counts[0] = T
    g = torch.Generator().manual_seed(7000 + idx)
    q = torch.randn(4, T, Hq, D, generator=g).to(BF16)
    k = torch.randn(4, Smax, Hkv, D, generator=g).to(BF16)
    v = (torch.randn(4, Smax, Hkv, D, generator=g) * 2).to(BF16)
    o64 = extend_oracle64(q, k, v, start, counts)
    nan_stale_(k, v, start, counts, T)
    return q, k, v, start, counts, Smax, o64


def _check(o, o64, start, counts, T, Smax, what):
    assert o.dtype == BF16 and o.shape == o64.shape
    o = o.cpu()
    assert torch.isfinite(o.float()).all(), f"{what}: not finite"
    st, cn = clamp_bounds(start, counts, T, Smax)
    for b in range(len(st)):
        assert torch.equal(o[b, cn[b]:], torch.zeros_like(o[b, cn[b]:])), f"{what}: padded rows of row {b} not zero"
    err = rel_l2(o, o64)
    print(f"{what}: worst relative L2 {err.max().item():.3e} (bound {O_TOL:.0e})")
    assert (err <= O_TOL).all(), f"{what}: relative L2 {err.max().item():.3e}"


def _i32(x, dev):
    return torch.tensor(x, dtype=torch.int32, device=dev)


@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("heads", HEADS, ids=lambda h: f"hq{h[0]}_hkv{h[1]}")
@pytest.mark.parametrize("D", [64, 128])
def test_kernel_against_float64(dev, no_ref, D, heads, T):
    att = _att()
    q, k, v, start, counts, Smax, o64 = _case(D, *heads, T)
    qd, st, cn = q.to(dev), _i32(start, dev), _i32(counts, dev)
    kd, vd = k.to(dev), v.to(dev)
    assert att.extend_native_ok(qd, kd, vd, st, cn)
    _check(att.extend_attention(qd, kd, vd, st, cn), o64, start, counts, T, Smax, "contiguous")
    # a [:, :Smax] slice of a longer cache (a batch stride), NaN behind it
    longer = [torch.full((4, Smax + 37, heads[1], D), float("nan"), dtype=BF16, device=dev) for _ in range(2)]
    longer[0][:, :Smax], longer[1][:, :Smax] = kd, vd
    ks, vs = longer[0][:, :Smax], longer[1][:, :Smax]
    assert not ks.is_contiguous() and att.extend_native_ok(qd, ks, vs, st, cn)
    _check(att.extend_attention(qd, ks, vs, st, cn), o64, start, counts, T, Smax, "slice")
    for page in (64, 128):
        kp, vp, table, _ = paged_case(k, v, start, counts, T, page, seed=D + T + page)
        kp, vp, tb = kp.to(dev), vp.to(dev), table.to(dev)
        assert att.extend_paged_native_ok(qd, kp, vp, tb, st, cn)
        _check(att.extend_attention_paged(qd, kp, vp, tb, st, cn), o64, start, counts, T, Smax, f"paged, page {page}")


@pytest.mark.parametrize("page", [64, 128])
def test_invalid_page_inside_the_visible_range(dev, no_ref, page):
    att = _att()
    D, heads, T = 128, (4, 2), 33
    q, k, v, start, counts, Smax, _ = _case(D, *heads, T)
    st, cn = clamp_bounds(start, counts, T, Smax)
    b = max(range(4), key=lambda i: st[i] + cn[i])  # the longest row loses its first page
    assert st[b] + cn[b] > page
    kp, vp, table, key_ok = paged_case(k, v, start, counts, T, page, seed=3, hole=(b, 0))
    assert not key_ok[b, :page].any() and key_ok[b, page]
    k64 = torch.nan_to_num(k.double())  # the oracle never reads what key_ok hides; NaN would poison its indexing
    o64 = extend_oracle64(q, k64, torch.nan_to_num(v.double()), start, counts, key_ok=key_ok)
    o = att.extend_attention_paged(q.to(dev), kp.to(dev), vp.to(dev), table.to(dev), _i32(start, dev), _i32(counts, dev))
    _check(o, o64, start, counts, T, Smax, f"hole in row {b}, page {page}")


@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("D", [64, 128])
def test_paged_bits_and_determinism(dev, no_ref, D, T):
    """equal operands: the paged kernel on the pool and the contiguous kernel on paged_gather of the pool give the
    same bits (the table is valid wherever a row is visible); two runs give the same bits"""
    att = _att()
    q, k, v, start, counts, Smax, _ = _case(D, 8, 1, T)
    qd, st, cn = q.to(dev), _i32(start, dev), _i32(counts, dev)
    for page in (64, 128):
        kp, vp, table, _ = paged_case(k, v, start, counts, T, page, seed=11 + page)
        kp, vp, tb = kp.to(dev), vp.to(dev), table.to(dev)
        a = att.extend_attention_paged(qd, kp, vp, tb, st, cn)
        assert torch.equal(a.view(torch.int16), att.extend_attention_paged(qd, kp, vp, tb, st, cn).view(torch.int16))
        kg, vg = att.paged_gather(kp, tb), att.paged_gather(vp, tb)
        c = att.extend_attention(qd, kg, vg, st, cn)
        assert torch.equal(a.view(torch.int16), c.view(torch.int16)), f"page {page}"
        assert torch.equal(c.view(torch.int16), att.extend_attention(qd, kg, vg, st, cn).view(torch.int16))


@pytest.mark.parametrize("D", [64, 128])
def test_against_the_flash_forward(dev, no_ref, D):
    """start = 0, counts = T: the flash forward's problem. Both sides within O_TOL of the oracle."""
    att = _att()
    Bn, S, Hq, Hkv = 2, 200, 4, 2
    g = torch.Generator().manual_seed(31 + D)
    q = torch.randn(Bn, S, Hq, D, generator=g).to(BF16)
    k = torch.randn(Bn, S, Hkv, D, generator=g).to(BF16)
    v = (torch.randn(Bn, S, Hkv, D, generator=g) * 2).to(BF16)
    o64 = extend_oracle64(q, k, v, [0] * Bn, None)
    qd, kd, vd = q.to(dev), k.to(dev), v.to(dev)
    zero = torch.zeros(Bn, dtype=torch.int32, device=dev)
    for counts in (None, _i32([S] * Bn, dev)):
        _check(att.extend_attention(qd, kd, vd, zero, counts), o64, [0] * Bn, None, S, S, "extend at start 0")
    flash = att.attention(qd, kd, vd, causal=True)
    assert (rel_l2(flash, o64) <= O_TOL).all()


@pytest.mark.parametrize("D", [64, 128])
def test_one_token_against_decode_attention(dev, no_ref, D):
    """T = 1: decode attention's problem with lens = start + 1. Both sides within O_TOL of the oracle."""
    att = _att()
    q, k, v, start, counts, Smax, o64 = _case(D, 8, 1, 1)
    st, cn = clamp_bounds(start, counts, 1, Smax)
    lens = [s + c for s, c in zip(st, cn)]
    live = [b for b in range(4) if cn[b]]
    assert live
    o = att.extend_attention(q.to(dev), k.to(dev), v.to(dev), _i32(start, dev), _i32(counts, dev))
    _check(o, o64, start, counts, 1, Smax, "extend, T = 1")
    dec = att.decode_attention(q[:, 0].contiguous().to(dev), k.to(dev), v.to(dev), _i32(lens, dev))
    d64, _ = decode_oracle64(q[:, 0], torch.nan_to_num(k.float()), torch.nan_to_num(v.float()), lens)
    for b in live:
        assert (d64[b] - o64[b, 0]).abs().max() < 1e-12  # one oracle
        assert (rel_l2(dec[b:b + 1].unsqueeze(1), o64[b:b + 1]) <= O_TOL).all()


@pytest.mark.parametrize("T", [33, 129])
def test_fp8_caches_through_the_public_op(dev, no_ref, T):
    """an FP8 slab and an FP8 pool take the slow path (a bf16 scratch, then the bf16 kernel): against the oracle on
    the dequantised cache, whose values are exact in bf16, with the bf16 kernel's bound"""
    att = _att()
    D, Hq, Hkv = 128, 4, 2
    q, k, v, start, counts, Smax, _ = _case(D, Hq, Hkv, T)
    st, cn = clamp_bounds(start, counts, T, Smax)
    lens = [s + c for s, c in zip(st, cn)]
    (kc, ks), (vc, vs) = att.kv_quantize_ref(torch.nan_to_num(k.float())), att.kv_quantize_ref(torch.nan_to_num(v.float()))
    o64 = extend_oracle64(q, att.kv_dequantize(kc, ks, torch.float64), att.kv_dequantize(vc, vs, torch.float64),
                          start, counts)
    for b in range(4):  # stale: the NaN code and NaN scales
        kc.view(torch.uint8)[b, lens[b]:] = 0x7F
        vc.view(torch.uint8)[b, lens[b]:] = 0x7F
    nan_stale_(ks, vs, start, counts, T)
    qd, sd, cd = q.to(dev), _i32(start, dev), _i32(counts, dev)
    assert not att.extend_native_ok(qd, kc.to(dev), vc.to(dev), sd, cd, ks.to(dev), vs.to(dev))
    o = att.extend_attention(qd, kc.to(dev), vc.to(dev), sd, cd, k_scale=ks.to(dev), v_scale=vs.to(dev))
    _check(o, o64, start, counts, T, Smax, "FP8 slab")
    kp, vp, table, _ = paged_case(kc, vc, start, counts, T, 64, seed=17)
    P = kp.shape[0]
    ksp, vsp = scatter_to_pages(ks, table, lens, P, 64), scatter_to_pages(vs, table, lens, P, 64)
    o = att.extend_attention_paged(qd, kp.to(dev), vp.to(dev), table.to(dev), sd, cd, k_scale=ksp.to(dev),
                                   v_scale=vsp.to(dev))
    _check(o, o64, start, counts, T, Smax, "FP8 pool")


def test_host_checks_of_the_bindings(dev):
    """a misaligned pointer, a page that is no multiple of 64 and D = 96 are refused before any launch, and the
    public ops then run the reference without raising"""
    att, C = _att(), _C()
    T, Hq, Hkv, D, Smax, page = 5, 4, 2, 64, 128, 64
    g = torch.Generator().manual_seed(41)

    def mk(D=D, page=page):
        q = torch.randn(2, T, Hq, D, generator=g).to(BF16).to(dev)
        kc, vc = (torch.randn(2, Smax, Hkv, D, generator=g).to(BF16).to(dev) for _ in range(2))
        kp, vp = (torch.randn(4, page, Hkv, D, generator=g).to(BF16).to(dev) for _ in range(2))
        return q, kc, vc, kp, vp

    start, table = _i32([3, 70], dev), _i32([[0, 1], [2, 3]], dev)
    q, kc, vc, kp, vp = mk()
    buf = torch.zeros(q.numel() + 8, dtype=BF16, device=dev)
    off = buf[1:1 + q.numel()].view_as(q).copy_(q)
    assert off.is_contiguous() and off.data_ptr() % 16 != 0
    q96, kc96, vc96, kp96, vp96 = mk(D=96)
    slab = [("16-byte aligned", (off, kc, vc, start)), ("head_dim must be 64 or 128", (q96, kc96, vc96, start)),
            ("start must be a contiguous int32", (q, kc, vc, start.long())),
            ("Hq must be a multiple of Hkv", (q[:, :, :3].contiguous(), kc, vc, start))]
    for msg, args in slab:
        with pytest.raises(RuntimeError, match=msg):
            C.attn_extend(*args, 0.125)
        assert not att.extend_native_ok(*args)
    pools = [("16-byte aligned", (off, kp, vp, table, start)), ("head_dim must be 64 or 128", (q96, kp96, vp96, table, start)),
             ("block_table must be int32", (q, kp, vp, table.long(), start))]
    for msg, args in pools:
        with pytest.raises(RuntimeError, match=msg):
            C.attn_extend_paged(*args, 0.125)
        assert not att.extend_paged_native_ok(*args)
    kp48, vp48 = mk(page=48)[3:]
    with pytest.raises(RuntimeError, match="page size must be a positive multiple of 64, got 48"):
        C.attn_extend_paged(q, kp48, vp48, table, start, 0.125)
    with pytest.raises(ValueError, match="multiple of 64"):
        att.extend_attention_paged(q, kp48, vp48, table, start)
    # the fall-back: the misaligned q through the public ops, against the oracle
    want = extend_oracle64(q.cpu(), kc.cpu(), vc.cpu(), [3, 70], None)
    assert (rel_l2(att.extend_attention(off, kc, vc, start), want) <= O_TOL).all()
    assert att.extend_native_ok(q, kc, vc, start) and att.extend_paged_native_ok(q, kp, vp, table, start)
    a, b = C.attn_extend(q, kc, vc, start, 0.125), att.extend_attention(q, kc, vc, start)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))  # the default scale is 1 / sqrt(D)


# ------------------------------------------------------------------ the model
BM, S, LENS, CHUNKS = 2, 24, (5, 11), (1, 5, 24)


def _tiny(dev, qk_norm):
    from cs744_pytorch_distributed_tutorial_amd.models import llama
    torch.manual_seed(11)
    m = llama.build("llama-tiny", qk_norm=qk_norm).eval()
    if qk_norm:
        with torch.no_grad():
            for blk in m.layers:
                blk.attention.q_norm.weight.uniform_(0.5, 1.5)
                blk.attention.k_norm.weight.uniform_(0.5, 1.5)
    m64 = copy.deepcopy(m).double()  # stays on the host
    return m.to(dev), m64


def _maker(att, cfg, kind, device, dtype):
    dt = att.FP8 if kind.endswith("fp8") else dtype

    def make():
        if kind.startswith("slab"):
            return stale_(att.KVCache.allocate(cfg, BM, S, device, dt))
        return stale_(att.PagedKVCache.allocate(cfg, BM, BM + 1, 64, None, device, dt))
    return make


@pytest.mark.parametrize("kind", ["slab", "slab_fp8", "paged", "paged_fp8"])
@pytest.mark.parametrize("qk_norm", [False, True], ids=["plain", "qk_norm"])
def test_model_under_autocast(dev, monkeypatch, qk_norm, kind):
    """llama-tiny (hd 64, G 2) under bf16 autocast, the scenarios of tests/extend_oracle.py (prefill(chunk=n) for
    n in {1, 5, S}, one extend of all the rest with all_logits, a second turn after decode steps): a cached path's
    logits against a float64 CPU copy of the same weights may err at most 2x what the GPU's own full forward errs
    against it, plus 2^-8 max|logits| (the bound form of tests/test_decode_gpu.py: the paths do not share the
    attention's rounding). An FP8 cache adds 2 * e_q, what the float64 copy loses through the same cache on the CPU
    reference path (tests/test_kv_fp8_gpu.py). No sampled tokens are compared: random weights give near-tied bf16
    logits."""
    att = _att()
    m, m64 = _tiny(dev, qk_norm)
    tokens = torch.randint(1, m.cfg.vocab_size, (BM, S), generator=torch.Generator().manual_seed(4))
    with torch.no_grad():
        ref = m64(tokens)
    e_q = {}
    if kind.endswith("fp8"):
        got64 = model_scenarios(m64, tokens, LENS, _maker(att, m.cfg, kind, torch.device("cpu"), torch.float64), CHUNKS)
        e_q = {name: worst(rows, ref) for name, (rows, _) in got64.items() if rows}

    def boom(*a, **kw):
        raise AssertionError("extend attention fell back to the reference")
    monkeypatch.setattr(att, "extend_attention_ref", boom)  # from here on the native paths must run
    monkeypatch.setattr(att, "extend_attention_paged_ref", boom)
    with torch.autocast("cuda", dtype=BF16):
        with torch.no_grad():
            full = m(tokens.to(dev)).double().cpu()
        got = model_scenarios(m, tokens.to(dev), LENS, _maker(att, m.cfg, kind, dev, m.cache_dtype(dev)), CHUNKS)
    top = ref.abs().max().item()
    for name in [f"chunk{n}" for n in CHUNKS] + ["extend_all", "second_turn"]:
        rows, cache = got[name]
        e = worst(rows, ref)
        e_full = max((full[b, t] - ref[b, t]).abs().max().item() for b, t, _ in rows)
        print(f"{name} ({kind}, qk_norm={qk_norm}): cached {e:.3e}, full forward {e_full:.3e}, max|logits| {top:.3e}, "
              f"e_q {e_q.get(name, 0.0):.3e}")
        assert torch.isfinite(torch.stack([lg.float() for _, _, lg in rows])).all()
        assert e <= 2 * e_full + 2.0 ** -8 * top + 2 * e_q.get(name, 0.0), name
    lens, bound = got["second_turn_state"][1]
    cache = got["second_turn"][1]
    assert cache.lens.tolist() == lens and cache.bound == bound
    for n in CHUNKS:
        assert got[f"chunk{n}"][1].lens.tolist() == list(LENS)
