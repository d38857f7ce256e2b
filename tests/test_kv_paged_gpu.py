"""The paged KV cache on the GPU (attn_decode_paged, attn_decode_paged_fp8, kv_append_paged; ops.attention
decode_attention_paged / kv_cache_append_paged / PagedKVCache): paged decode attention bit for bit against the
contiguous kernel on the gathered cache and against the float64 oracle, with every unreachable datum of the pool in
the kernel's way (NaN pages, NaN tails, invalid table entries); table safety; the append byte for byte against a host
loop; the host checks; and Llama.prefill / decode_step / generate on a PagedKVCache under bf16 autocast (MI355X only)."""
import copy
import functools

import pytest
import torch

from decode_oracle import decode_oracle64, teacher_forced
from kv_fp8_oracle import FP8, quantize_oracle
from kv_paged_oracle import (bytes_of, deal_pages, dequant, expected_append, gather_nan, oracle_visible64,
                             reachable_rows, scatter_to_pages, visible)

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
HEADS = [(4, 4), (4, 2), (8, 1), (32, 8)]
B = 6
EXTRA = 5  # pages nobody owns


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


def _forbid_refs(monkeypatch):
    def boom(what):
        def f(*a, **kw):
            raise AssertionError(f"{what} fell back to the reference")
        return f
    att = _att()
    monkeypatch.setattr(att, "decode_attention_ref", boom("decode_attention"))
    monkeypatch.setattr(att, "decode_attention_paged_ref", boom("decode_attention_paged"))
    monkeypatch.setattr(att, "kv_cache_append_paged_ref", boom("kv_cache_append_paged"))
    monkeypatch.setattr(att, "kv_quantize_ref", boom("a quantising append"))


@pytest.fixture
def no_ref(monkeypatch):
    """the native paths must run: every reference raises"""
    _forbid_refs(monkeypatch)
    return monkeypatch


def _on(dev, *ts):
    return tuple(None if t is None else t.to(dev) for t in ts)


def test_page_tile_is_the_kernels_key_tile(dev):
    assert _att().PAGE_TILE == _C().decode_key_tile() == _att().decode_key_tile() == 64


# ------------------------------------------------------------------ decode attention through the table
def _columns(page):
    return 4 if page == 64 else 3  # Smax 256 / 384: four / six key tiles


@functools.lru_cache(maxsize=None)
def _case(D, Hq, Hkv, page, fp8):
    """One pool on the host, computed once and never changed: more pages than needed, the rows' pages dealt from a
    seeded permutation, NaN (FP8: code 0x7F and NaN scales) in every unowned page and every tail, the table's unused
    columns -1 / P + 5. With it the gathered cache (NaN where invisible), the float64 oracle on the gathered
    (dequantised) cache and the bound 2^-7 * max|v| per (sequence, kv head), expanded to the query heads."""
    C = _columns(page)
    Smax = C * page
    seed = 1000 * D + 10 * Hq + Hkv + page + (7 if fp8 else 0)
    g = torch.Generator().manual_seed(seed)
    pick = [0, 1, 63, 64, 65, 127, 128, 129]
    rot = (D // 64 + Hq + Hkv + page // 64 + fp8) % len(pick)
    lens = torch.tensor([Smax] + (pick[rot:] + pick[:rot])[:B - 1])[torch.randperm(B, generator=g)].int()
    need = [-(-int(n) // page) for n in lens]
    P = sum(need) + EXTRA
    table = deal_pages(need, C, P, seed)
    q = torch.randn(B, Hq, D, generator=g).to(BF16)
    mag = torch.logspace(-2, 2, Smax)[torch.randperm(Smax, generator=g)].view(1, Smax, 1, 1)
    k = torch.randn(B, Smax, Hkv, D, generator=g) * mag.sqrt()
    v = torch.randn(B, Smax, Hkv, D, generator=g) * 2 * mag.flip(1)
    if fp8:
        (kc, ks), (vc, vs) = quantize_oracle(k), quantize_oracle(v)
        pools = tuple(scatter_to_pages(t, table, lens, P, page) for t in (kc, vc, ks, vs))
        o64, vmax = decode_oracle64(q, dequant(kc, ks), dequant(vc, vs), lens)
    else:
        kc, vc = k.to(BF16), v.to(BF16)
        pools = tuple(scatter_to_pages(t, table, lens, P, page) for t in (kc, vc)) + (None, None)
        o64, vmax = decode_oracle64(q, kc, vc, lens)
    gathered = tuple(None if t is None else gather_nan(t, table, lens, page) for t in pools)
    bound = (2.0 ** -7 * vmax).repeat_interleave(Hq // Hkv, dim=1).unsqueeze(-1)  # [B, Hq, 1]
    return q, pools, table, lens, gathered, o64, bound


def _check(o, lens, o64, bound, what):
    assert o.dtype == BF16 and o.shape == o64.shape
    o = o.double().cpu()
    assert not torch.isnan(o).any(), what
    err = (o - o64).abs()
    print(f"{what}: max err {err.max().item():.3e}, worst err - bound {(err - bound).max().item():.3e}")
    assert (err <= bound).all(), f"{what}: error exceeds 2^-7 max|v| by {(err - bound).max().item():.3e}"
    for b in range(len(lens)):
        if int(lens[b]) <= 0:
            assert torch.equal(o[b], torch.zeros_like(o[b])), f"{what}: a row of length 0 is not exactly zero"


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("page", [64, 128])
@pytest.mark.parametrize("heads", HEADS, ids=lambda h: f"hq{h[0]}_hkv{h[1]}")
@pytest.mark.parametrize("D", [64, 128])
def test_bits_of_the_contiguous_kernel_and_float64(dev, no_ref, D, heads, page, fp8):
    """decode_attention_paged == decode_attention(splits=same) on the gathered cache, bit for bit (the arithmetic per
    key is the same code), and both inside 2^-7 * max|v| of the float64 oracle. The gathered cache holds NaN wherever
    the pool does."""
    att = _att()
    q, pools, table, lens, gathered, o64, bound = _case(D, *heads, page, fp8)
    assert torch.isnan(gathered[0].float()).any() and torch.isnan(pools[0].float()).any()
    qd, td, ld = _on(dev, q, table, lens)
    kp, vp, ks, vs = _on(dev, *pools)
    gk, gv, gks, gvs = _on(dev, *gathered)
    assert att.decode_paged_native_ok(qd, kp, vp, td, ld, ks, vs)
    tiles = table.shape[1] * page // 64
    outs = []
    for s in (1, 2, 3, tiles, 1000):
        o = att.decode_attention_paged(qd, kp, vp, td, ld, splits=s, k_scale=ks, v_scale=vs)
        ref = att.decode_attention(qd, gk, gv, ld, splits=s, k_scale=gks, v_scale=gvs)
        what = f"{'FP8' if fp8 else 'bf16'} D{D} {heads} page {page} splits {s}"
        assert torch.equal(o, ref), f"{what}: paged and contiguous kernels differ in bits"
        _check(o, lens, o64, bound, what)
        outs.append(o)
    assert torch.equal(outs[-1], outs[-2])  # 1000 splits is clamped to the number of tiles
    o = att.decode_attention_paged(qd, kp, vp, td, ld, k_scale=ks, v_scale=vs)
    assert torch.equal(o, att.decode_attention(qd, gk, gv, ld, k_scale=gks, v_scale=gvs))
    _check(o, lens, o64, bound, "default splits")
    # a wider table cut to its first C columns is an operand as it is
    wide = torch.full((B, table.shape[1] + 3), 2, dtype=torch.int32, device=dev)
    wide[:, :table.shape[1]] = td
    cut = wide[:, :table.shape[1]]
    assert not cut.is_contiguous() and att.decode_paged_native_ok(qd, kp, vp, cut, ld, ks, vs)
    assert torch.equal(att.decode_attention_paged(qd, kp, vp, cut, ld, splits=2, k_scale=ks, v_scale=vs), outs[1])


def test_binding_scale_argument(dev):
    q, pools, table, lens, gathered, _, bound = _case(128, 32, 8, 64, False)
    o64, _ = decode_oracle64(q, gathered[0], gathered[1], lens, scale=0.3)
    o = _C().attn_decode_paged(*_on(dev, q, pools[0], pools[1], table, lens), 0.3)
    _check(o, lens, o64, bound, "bf16 scale 0.3, default splits")


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("splits", [1, 3])
def test_table_safety(dev, no_ref, splits, fp8):
    """Invalid entries inside a length mask their keys (the oracle's result over the remaining keys), lens are
    clamped, other garbage in every unreachable byte changes no bit, two runs agree."""
    att = _att()
    D, Hq, Hkv, page = 128, 8, 2, 64
    q, pools, table, lens, _, _, _ = _case(D, Hq, Hkv, page, fp8)
    C, P = table.shape[1], pools[0].shape[0]
    Smax = C * page
    # holes: -1 / P + 5 in the middle of the two longest rows; lens below zero and far past the end
    table, lens = table.clone(), lens.clone()
    order = lens.argsort(descending=True)
    full, second, short = int(order[0]), int(order[1]), int(order[-1])
    table[full, 1], table[full, 2] = -1, P + 5
    table[second, 0] = P + 5
    lens[full], lens[short] = Smax + 100, -5
    # the logical cache the pool stands for, rebuilt from the pool itself
    tame = lens.clamp(0, Smax)
    vis = visible(table, tame, P, page)
    assert vis[full].sum() == 2 * page and not vis[short].any() and int(lens[second]) > page
    gath = [None if t is None else gather_nan(t, table, tame, page) for t in pools]
    if fp8:
        k64, v64 = dequant(gath[0], gath[2]), dequant(gath[1], gath[3])
    else:
        k64, v64 = gath[0].double(), gath[1].double()
    o64, vmax = oracle_visible64(q, torch.nan_to_num(k64), torch.nan_to_num(v64), vis)
    bound = (2.0 ** -7 * vmax).repeat_interleave(Hq // Hkv, dim=1).unsqueeze(-1)
    qd, td, ld = _on(dev, q, table, lens)
    kp, vp, ks, vs = _on(dev, *pools)
    a = att.decode_attention_paged(qd, kp, vp, td, ld, splits=splits, k_scale=ks, v_scale=vs)
    _check(a, tame, o64, bound, f"holes, {'FP8' if fp8 else 'bf16'} splits {splits}")
    assert torch.equal(a, att.decode_attention_paged(qd, kp, vp, td, ld, splits=splits, k_scale=ks, v_scale=vs))
    assert torch.equal(a, att.decode_attention_paged(qd, kp, vp, td, tame.to(dev), splits=splits, k_scale=ks,
                                                     v_scale=vs))
    assert torch.equal(a[short], torch.zeros_like(a[short]))
    reach = reachable_rows(table, tame, P, page)
    assert not reach.all()
    for code, junk in ((0x00, float("inf")), (0x7E, 0.0), (0xFF, 3.0e38)):
        k2, v2 = pools[0].clone(), pools[1].clone()
        bytes_of(k2)[~reach], bytes_of(v2)[~reach] = code, code
        sc = (None, None)
        if fp8:
            sc = (pools[2].clone(), pools[3].clone())
            sc[0][~reach], sc[1][~reach] = junk, junk
        got = att.decode_attention_paged(qd, *_on(dev, k2, v2), td, ld, splits=splits, k_scale=_on(dev, sc[0])[0],
                                         v_scale=_on(dev, sc[1])[0])
        assert torch.equal(a, got), f"garbage {code:#x} in the unreachable bytes changed the output"
    # other garbage in the table's unused columns too
    t2 = table.clone()
    for b in range(B):
        t2[b, -(-int(tame[b]) // page):] = 2 ** 31 - 1 if b % 2 else -(2 ** 31)
    assert torch.equal(a, att.decode_attention_paged(qd, kp, vp, t2.to(dev), ld, splits=splits, k_scale=ks, v_scale=vs))


# ------------------------------------------------------------------ the append
def _pattern(P, page, Hkv, D, fp8, dev):
    """pools (and scales) holding a pattern that no append writes"""
    dt = FP8 if fp8 else BF16
    n = D * (1 if fp8 else 2)
    kp = torch.full((P, page, Hkv, n), 0x5A, dtype=torch.uint8, device=dev).view(dt)
    vp = torch.full((P, page, Hkv, n), 0xA5, dtype=torch.uint8, device=dev).view(dt)
    if not fp8:
        return kp, vp
    return kp, vp, torch.full((P, page, Hkv), -7.0, device=dev), torch.full((P, page, Hkv), -9.0, device=dev)


def _same_bytes(got, want, what):
    for name, a, b in zip(("k pool", "v pool", "k scales", "v scales"), got, want):
        assert torch.equal(bytes_of(a.cpu()), bytes_of(b)), f"{what}: {name} differ from the host loop"


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("S", [1, 3, 70])
@pytest.mark.parametrize("Hkv", [1, 2, 8])
@pytest.mark.parametrize("D", [64, 128])
def test_append_bytes_and_drops(dev, no_ref, D, Hkv, S, fp8):
    """B 5, page 64, C 3 (192 positions): rows starting at 0, just before a page boundary, two short of the end
    (the rest is dropped), below zero (the negative positions are dropped) and far past the end; one row with a
    -1 column and one with a P + 5 column in its way; counts absent or ragged with a 0. Every byte no stored token
    owns keeps the pattern."""
    att = _att()
    Bn, page, C = 5, 64, 3
    P = Bn * C + 4
    table = deal_pages([C] * Bn, C, P, seed=D + Hkv + S)
    table[1, 1], table[3, 0] = -1, P + 5
    g = torch.Generator().manual_seed(100 * D + 10 * Hkv + S)
    k = (torch.randn(Bn, S, Hkv, D, generator=g) * 3).to(BF16)
    v = (torch.randn(Bn, S, Hkv, D, generator=g) * 0.01).to(BF16)
    pos_list = (None, (0, 60, C * page - 2, -2, C * page + 1000))
    counts_list = (None, (S, max(S - 1, 0), 0, S, 1))
    total = 0
    for pos in pos_list:
        for counts in counts_list:
            bufs = _pattern(P, page, Hkv, D, fp8, dev)
            want, stored = expected_append(bufs, table, k, v, pos, counts, page)
            total += stored
            posd = None if pos is None else torch.tensor(pos, dtype=torch.int32, device=dev)
            cntd = None if counts is None else torch.tensor(counts, dtype=torch.int32, device=dev)
            kw = dict(k_scale=bufs[2], v_scale=bufs[3]) if fp8 else {}
            assert att.kv_append_paged_native_ok(bufs[0], bufs[1], table.to(dev), k.to(dev), v.to(dev), posd, cntd, **kw)
            att.kv_cache_append_paged(bufs[0], bufs[1], table.to(dev), k.to(dev), v.to(dev), posd, cntd, **kw)
            _same_bytes(bufs, want, f"D{D} Hkv{Hkv} S{S} pos {pos} counts {counts}")
            again = _pattern(P, page, Hkv, D, fp8, dev)
            kw = dict(k_scale=again[2], v_scale=again[3]) if fp8 else {}
            att.kv_cache_append_paged(again[0], again[1], table.to(dev), k.to(dev), v.to(dev), posd, cntd, **kw)
            for a, b in zip(bufs, again):
                assert torch.equal(bytes_of(a), bytes_of(b))
    assert total > 0


def test_append_everything_dropped_writes_nothing(dev, no_ref):
    att = _att()
    P, page, C, Hkv, D = 4, 64, 2, 2, 64
    g = torch.Generator().manual_seed(3)
    k, v = (torch.randn(4, 3, Hkv, D, generator=g).to(BF16).to(dev) for _ in range(2))
    table = torch.tensor([[0, 1], [-1, P + 5], [2, 3], [2, 3]], dtype=torch.int32, device=dev)
    pos = torch.tensor([-3, 0, C * page, 5], dtype=torch.int32, device=dev)  # below zero, no pages, past the end
    counts = torch.tensor([3, 3, 3, 0], dtype=torch.int32, device=dev)  # and a row of no tokens
    for fp8 in (False, True):
        bufs = _pattern(P, page, Hkv, D, fp8, dev)
        want = [t.cpu().clone() for t in bufs]
        kw = dict(k_scale=bufs[2], v_scale=bufs[3]) if fp8 else {}
        att.kv_cache_append_paged(bufs[0], bufs[1], table, k, v, pos, counts, **kw)
        _same_bytes(bufs, want, "all dropped")


def test_append_then_attend_round_trip(dev, no_ref):
    """what the append stores is what the attention reads: a ragged prefill and one step, against the contiguous
    kernel on the same rows"""
    att = _att()
    Bn, S, Hq, Hkv, D, page, C = 3, 70, 8, 2, 128, 64, 3
    g = torch.Generator().manual_seed(9)
    k, v = (torch.randn(Bn, S + 1, Hkv, D, generator=g).to(BF16).to(dev) for _ in range(2))
    q = torch.randn(Bn, Hq, D, generator=g).to(BF16).to(dev)
    counts = torch.tensor([70, 1, 64], dtype=torch.int32, device=dev)
    table = deal_pages([2, 1, 2], C, 9, seed=1).to(dev)
    kp = torch.full((9, page, Hkv, D), float("nan"), dtype=BF16, device=dev)
    vp = kp.clone()
    att.kv_cache_append_paged(kp, vp, table, k[:, :S].contiguous(), v[:, :S].contiguous(), counts=counts)
    step_k = torch.stack([k[b, int(counts[b])] for b in range(Bn)]).unsqueeze(1).contiguous()
    step_v = torch.stack([v[b, int(counts[b])] for b in range(Bn)]).unsqueeze(1).contiguous()
    att.kv_cache_append_paged(kp, vp, table, step_k, step_v, pos=counts)
    lens = counts + 1
    o = att.decode_attention_paged(q, kp, vp, table[:, :2], lens, splits=2)
    assert torch.equal(o, att.decode_attention(q, k.contiguous(), v.contiguous(), lens, splits=2))


# ------------------------------------------------------------------ the host checks
def test_host_checks_and_fallback(dev):
    att, C = _att(), _C()
    P, page, Cn, Hq, Hkv, D = 5, 64, 2, 4, 2, 64
    g = torch.Generator().manual_seed(6)
    lens = torch.tensor([100, 4], dtype=torch.int32)
    table = torch.tensor([[3, 1], [0, -1]], dtype=torch.int32)

    def mk(Hq=Hq, Hkv=Hkv, D=D, page=page, fp8=False):
        q = torch.randn(2, Hq, D, generator=g).to(BF16).to(dev)
        k, v = torch.randn(P, page, Hkv, D, generator=g), torch.randn(P, page, Hkv, D, generator=g)
        if fp8:
            (kp, ks), (vp, vs) = (_on(dev, *quantize_oracle(t)) for t in (k, v))
            return [q, kp, vp, ks, vs, table.to(dev), lens.to(dev)]
        return [q, k.to(BF16).to(dev), v.to(BF16).to(dev), table.to(dev), lens.to(dev)]

    def oracle(args):
        q, kp, vp = args[0], args[1], args[2]
        tb, ln = args[-2].cpu(), args[-1].cpu()
        if len(args) == 7:
            k64, v64 = dequant(kp, args[3]), dequant(vp, args[4])
        else:
            k64, v64 = kp.double().cpu(), vp.double().cpu()
        pg = kp.shape[1]
        gk, gv = (gather_nan(t, tb, ln, pg) for t in (k64, v64))
        return oracle_visible64(q, torch.nan_to_num(gk), torch.nan_to_num(gv), visible(tb, ln, kp.shape[0], pg))

    q, kp, vp, tb, ln = mk()
    cases = []
    cases.append(("block_table must be int32", [q, kp, vp, tb.long(), ln]))
    cases.append(("block_table must be on the pools' device", [q, kp, vp, tb.cpu(), ln]))
    wide = torch.zeros(2, 2 * Cn, dtype=torch.int32, device=dev)
    wide[:, ::2] = tb
    cases.append(("column stride of block_table must be 1", [q, kp, vp, wide[:, ::2], ln]))
    cases.append(("query heads per kv head", mk(Hq=6)))
    cases.append(("head_dim must be 64 or 128", mk(D=96)))
    cases.append(("lens must be int32", [q, kp, vp, tb, ln.long()]))
    buf = torch.zeros(q.numel() + 8, dtype=BF16, device=dev)
    off = buf[1:1 + q.numel()].view_as(q).copy_(q)
    assert off.is_contiguous() and off.data_ptr() % 16 != 0
    cases.append(("16-byte aligned", [off, kp, vp, tb, ln]))
    big = torch.zeros(P, page, Hkv, 2 * D, dtype=BF16, device=dev)
    big[..., ::2] = kp
    cases.append(("inner three dimensions of the pools", [q, big[..., ::2], vp, tb, ln]))
    odd = torch.zeros(P, page * Hkv * D + 4, dtype=BF16, device=dev)[:, :page * Hkv * D].view(P, page, Hkv, D)
    cases.append(("page stride of a pool must be a multiple of 8", [q, odd, odd, tb, ln]))
    for msg, args in cases:
        with pytest.raises(RuntimeError, match=msg):
            C.attn_decode_paged(*args, 0.125)
        assert not att.decode_paged_native_ok(*args)
        o = att.decode_attention_paged(*args)  # the reference, without raising
        o64, vmax = oracle(args)
        assert o.dtype == args[0].dtype and o.device == args[0].device
        assert (o.double().cpu() - o64).abs().max() <= 2.0 ** -7 * vmax.max(), msg
    # FP8 pools
    q8, kp8, vp8, ks8, vs8, tb8, ln8 = mk(fp8=True)
    wides = torch.zeros(P, page, 2 * Hkv, device=dev)
    wides[..., ::2] = ks8
    for msg, args in (("inner two dimensions of the scales", [q8, kp8, vp8, wides[..., ::2], vs8, tb8, ln8]),
                      ("block_table must be int32", [q8, kp8, vp8, ks8, vs8, tb8.long(), ln8])):
        with pytest.raises(RuntimeError, match=msg):
            C.attn_decode_paged_fp8(*args, 0.125)
        qa, ka, va, ksa, vsa, ta, la = args
        assert not att.decode_paged_native_ok(qa, ka, va, ta, la, ksa, vsa)
        o = att.decode_attention_paged(qa, ka, va, ta, la, k_scale=ksa, v_scale=vsa)
        o64, vmax = oracle(args)
        assert (o.double().cpu() - o64).abs().max() <= 2.0 ** -7 * vmax.max(), msg
    assert att.decode_paged_native_ok(q8, kp8, vp8, tb8, ln8, ks8, vs8)
    # what is refused outright: the page size, and a dtype and scales that do not go together
    p48 = mk(page=48)
    with pytest.raises(RuntimeError, match="page size must be a positive multiple of 64, got 48"):
        C.attn_decode_paged(*p48, 0.125)
    with pytest.raises(ValueError, match="page size must be a positive multiple of 64, got 48"):
        att.decode_attention_paged(*p48)
    with pytest.raises(RuntimeError, match="q and the pools must be bfloat16"):
        C.attn_decode_paged(q8, kp8, vp8, tb8, ln8, 0.125)
    with pytest.raises(RuntimeError, match="pools must be float8_e4m3fn"):
        C.attn_decode_paged_fp8(q, kp, vp, ks8, vs8, tb, ln, 0.125)
    with pytest.raises(RuntimeError, match=r"scales must be \[P, page, Hkv\]"):
        C.attn_decode_paged_fp8(q8, kp8, vp8, ks8[:, :32], vs8, tb8, ln8, 0.125)
    with pytest.raises(ValueError, match="need k_scale and v_scale"):
        att.decode_attention_paged(q8, kp8, vp8, tb8, ln8)
    with pytest.raises(ValueError, match="float8_e4m3fn pools only"):
        att.decode_attention_paged(q, kp, vp, tb, ln, k_scale=ks8, v_scale=vs8)
    with pytest.raises(RuntimeError, match="inference only"):
        att.decode_attention_paged(q.clone().requires_grad_(), kp, vp, tb, ln)
    assert att.decode_paged_native_ok(q, kp, vp, tb, ln)


def test_append_host_checks_and_fallback(dev):
    att, C = _att(), _C()
    P, page, Hkv, D = 4, 64, 2, 64
    g = torch.Generator().manual_seed(8)
    table = torch.tensor([[2, 0], [3, -1]], dtype=torch.int32, device=dev)
    pos = torch.tensor([62, 1], dtype=torch.int32, device=dev)
    k = torch.randn(2, 3, Hkv, D, generator=g).to(BF16).to(dev)
    v = torch.randn(2, 3, Hkv, D, generator=g).to(BF16).to(dev)

    def run_c(kp, vp, tb, kk, vv, ps=None, cnt=None, ks=None, vs=None):
        C.kv_append_paged(kp, vp, tb, kk, vv, ps, cnt, ks, vs)

    for fp8 in (False, True):
        base = _pattern(P, page, Hkv, D, fp8, dev)
        sc = dict(ks=base[2], vs=base[3]) if fp8 else {}
        scales = dict(k_scale=base[2], v_scale=base[3]) if fp8 else {}
        cases = [("k and v must be bfloat16", dict(kk=k.float(), vv=v.float())),
                 ("block_table must be int32", dict(tb=table.long())),
                 ("block_table must be on the pools' device", dict(tb=table.cpu())),
                 ("pos must be a contiguous int32", dict(ps=pos.long())),
                 ("counts must be a contiguous int32", dict(cnt=torch.ones(2, dtype=torch.int64, device=dev)))]
        for msg, change in cases:
            args = dict(kp=base[0], vp=base[1], tb=table, kk=k, vv=v, ps=pos, cnt=None, **sc)
            args.update(change)
            with pytest.raises(RuntimeError, match=msg):
                run_c(**args)
            # the ops function takes the same operands through the reference, to the host loop's bytes
            bufs = _pattern(P, page, Hkv, D, fp8, dev)
            want, stored = expected_append(bufs, table.cpu(), args["kk"].to(BF16), args["vv"].to(BF16), pos.cpu(),
                                           args["cnt"], page)
            assert stored > 0
            kw = dict(k_scale=bufs[2], v_scale=bufs[3]) if fp8 else {}
            assert not att.kv_append_paged_native_ok(bufs[0], bufs[1], args["tb"], args["kk"], args["vv"], args["ps"],
                                                     args["cnt"], **kw)
            att.kv_cache_append_paged(bufs[0], bufs[1], args["tb"], args["kk"], args["vv"], args["ps"], args["cnt"], **kw)
            _same_bytes(bufs, want, f"fallback, {msg}")
        run_c(base[0], base[1], table, k, v, pos, None, **sc)  # and the base case is accepted
        with pytest.raises(RuntimeError, match="head_dim must be 64 or 128"):
            k96 = torch.zeros(2, 3, Hkv, 96, dtype=BF16, device=dev)
            run_c(*_pattern(P, page, Hkv, 96, False, dev), table, k96, k96)
    bf, f8 = _pattern(P, page, Hkv, D, False, dev), _pattern(P, page, Hkv, D, True, dev)
    with pytest.raises(RuntimeError, match="pools without scales must be bfloat16"):
        run_c(f8[0], f8[1], table, k, v)
    with pytest.raises(RuntimeError, match="pools that come with scales must be float8_e4m3fn"):
        run_c(bf[0], bf[1], table, k, v, ks=f8[2], vs=f8[3])
    with pytest.raises(RuntimeError, match="page size must be a positive multiple of 64, got 48"):
        run_c(*_pattern(P, 48, Hkv, D, False, dev), table, k, v)
    with pytest.raises(ValueError, match="need k_scale and v_scale"):
        att.kv_cache_append_paged(f8[0], f8[1], table, k, v)
    with pytest.raises(ValueError, match="float8_e4m3fn pools only"):
        att.kv_cache_append_paged(bf[0], bf[1], table, k, v, k_scale=f8[2], v_scale=f8[3])
    with pytest.raises(ValueError, match="page size must be a positive multiple of 64, got 48"):
        att.kv_cache_append_paged(*_pattern(P, 48, Hkv, D, False, dev), table, k, v)


# ------------------------------------------------------------------ the model
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


def _stale_pool(att, cfg, Bm, pages, dev, dtype):
    pool = att.PagedKVCache.allocate(cfg, Bm, pages, 64, device=dev, dtype=dtype)
    if dtype == FP8:
        bytes_of(pool.k).fill_(0x7F)
        bytes_of(pool.v).fill_(0x7F)
        pool.k_scale.fill_(float("nan"))
        pool.v_scale.fill_(float("nan"))
    else:
        pool.k.fill_(float("nan"))
        pool.v.fill_(float("nan"))
    return pool


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("qk_norm", [False, True], ids=["plain", "qk_norm"])
def test_model_teacher_forced(dev, monkeypatch, qk_norm, fp8):
    """llama-tiny under bf16 autocast, teacher-forced through a PagedKVCache of page 64 with ragged prompts (5, 11)
    and S 24, against a float64 CPU copy of the weights. The bounds are those of the contiguous caches, computed the
    same way: 2 * e_full + 2^-8 * top for the bf16 pool (tests/test_decode_gpu.py), plus 2 * e_q for the FP8 pool
    (tests/test_kv_fp8_gpu.py), e_q being m64's own error through an FP8 pool on the CPU reference path. The prefill
    logits equal the contiguous cache's bit for bit: the same code up to the cache write."""
    att = _att()
    m, m64 = _tiny(dev, qk_norm)
    Bm, S, lens = 2, 24, (5, 11)
    n = S + max(lens) - min(lens)
    dtype = FP8 if fp8 else BF16
    tokens = torch.randint(1, m.cfg.vocab_size, (Bm, S), generator=torch.Generator().manual_seed(4))
    with torch.no_grad():
        ref = m64(tokens)
    e_q = 0.0
    if fp8:
        got64 = teacher_forced(m64, tokens, lens, _stale_pool(att, m64.cfg, Bm, 4, torch.device("cpu"), FP8))
        e_q = max((lg - ref[b, t]).abs().max().item() for b, t, lg in got64)
    _forbid_refs(monkeypatch)  # from here on the native paths must run
    with torch.autocast("cuda", dtype=BF16):
        with torch.no_grad():
            full = m(tokens.to(dev)).double().cpu()
        pool = _stale_pool(att, m.cfg, Bm, 4, dev, dtype)
        for b in range(Bm):
            pool.reserve(b, n)
        got = teacher_forced(m, tokens.to(dev), lens, pool)
        contiguous = att.KVCache.allocate(m.cfg, Bm, n, dev, dtype)
        prompt = tokens[:, :max(lens)].clone()
        prompt[0, lens[0]:] = 0
        first = m.prefill(prompt.to(dev), contiguous, torch.tensor(lens))
    for b in range(Bm):
        assert torch.equal(got[b][2], first[b]), "the prefill logits differ from the contiguous cache's"
    assert sorted((b, t) for b, t, _ in got) == sorted((b, t) for b in range(Bm) for t in range(lens[b] - 1, S))
    e_dec = max((lg.double().cpu() - ref[b, t]).abs().max().item() for b, t, lg in got)
    e_full = max((full[b, t] - ref[b, t]).abs().max().item() for b, t, _ in got)
    top = ref.abs().max().item()
    print(f"model teacher-forced, paged {'FP8' if fp8 else 'bf16'} pool (qk_norm={qk_norm}): decode {e_dec:.3e}, "
          f"full forward {e_full:.3e}, max|logits| {top:.3e}, e_q {e_q:.3e}")
    assert e_dec <= 2 * e_full + 2.0 ** -8 * top + 2 * e_q
    assert pool.lens.tolist() == [x + S - min(lens) for x in lens] and pool.bound == n


def test_model_generate(dev, no_ref):
    att = _att()
    m, _ = _tiny(dev, False)
    tokens = torch.randint(1, m.cfg.vocab_size, (3, 9), generator=torch.Generator().manual_seed(12)).to(dev)
    plens = torch.tensor([4, 9, 9])
    made = []
    allocate = att.PagedKVCache.allocate.__func__
    no_ref.setattr(att.PagedKVCache, "allocate",
                   classmethod(lambda cls, *a, **kw: made.append(allocate(cls, *a, **kw)) or made[-1]))
    with torch.autocast("cuda", dtype=BF16):
        flat = m.generate(tokens, 70, prompt_lens=plens)
        out = m.generate(tokens, 70, prompt_lens=plens, page_size=64)
        out8 = m.generate(tokens, 12, prompt_lens=plens, page_size=64, kv_dtype="fp8")
        smp = m.generate(tokens, 12, prompt_lens=plens, temperature=0.8, top_k=20, eos_id=m.cfg.eos_id, page_size=128,
                         generator=torch.Generator(device=dev).manual_seed(1))
        eos = int(out[1, 3])
        at = int((out[1] == eos).nonzero()[0])  # where row 1 first emits it
        stop = m.generate(tokens, 12, prompt_lens=plens, eos_id=eos, page_size=64)
    for t, n in ((out, 70), (out8, 12), (smp, 12), (stop, 12)):
        assert t.dtype == torch.int64 and t.shape == (3, n) and t.device.type == "cuda"
        assert int(t.min()) >= 0 and int(t.max()) < m.cfg.vocab_size
    assert torch.equal(out[:, 0], flat[:, 0])  # the first token comes from the prefill: the same code
    assert torch.equal(stop[1, :at + 1], out[1, :at + 1]) and (stop[1, at:] == eos).all()  # EOS, then EOS for good
    assert [c.num_pages for c in made] == [6, 3, 3, 3]  # ceil((4 + 70) / 64) + 2 * ceil((9 + 70) / 64), ...
    assert made[0].k.dtype == BF16 and made[1].k.dtype == FP8 and made[1].k_scale.shape == made[1].k.shape[:-1]
    assert made[2].page_size == 128 and made[2].block_table.shape == (3, 1)


def test_generate_from_a_shared_pool(dev, no_ref):
    att = _att()
    m, _ = _tiny(dev, False)
    tokens = torch.randint(1, m.cfg.vocab_size, (3, 9), generator=torch.Generator().manual_seed(12)).to(dev)
    pool = att.PagedKVCache.allocate(m.cfg, 3, 5, 64, device=dev, dtype=BF16)  # 1 + 2 + 2 pages: exactly enough
    seen = []
    reserve = pool.reserve

    def spy(b, n):
        reserve(b, n)
        seen.append((b, tuple(pool.pages_of(b))))
    pool.reserve = spy
    with torch.autocast("cuda", dtype=BF16):
        a = m.generate(tokens, 60, prompt_lens=[4, 9, 9], kv_pool=pool)
        assert pool.pages_in_use == 0 and pool.pages_free == 5 and pool.lens.tolist() == [0, 0, 0]
        first = {p for _, pages in seen for p in pages}
        del seen[:]
        b = m.generate(tokens, 60, prompt_lens=[4, 9, 9], kv_pool=pool)
        assert pool.pages_in_use == 0 and (pool.block_table == -1).all()
        assert first & {p for _, pages in seen for p in pages}, "the second call reuses pages of the first"
        assert torch.equal(a, b) and torch.equal(a, m.generate(tokens, 60, prompt_lens=[4, 9, 9], page_size=64))
        with pytest.raises(RuntimeError, match="more pages"):
            m.generate(tokens, 100, prompt_lens=[4, 9, 9], kv_pool=pool)  # 3 * 2 pages > 5
        assert pool.pages_in_use == 0  # freed on the exception too


def test_no_host_sync_in_decode(dev, no_ref):
    att = _att()
    m, _ = _tiny(dev, True)
    tokens = torch.randint(1, m.cfg.vocab_size, (3, 9), generator=torch.Generator().manual_seed(13)).to(dev)
    for dtype in (BF16, FP8):
        with torch.autocast("cuda", dtype=BF16):
            pool = att.PagedKVCache.allocate(m.cfg, 3, 8, 64, device=dev, dtype=dtype)
            logits = m.prefill(tokens, pool, torch.tensor([4, 9, 9]))
            assert [pool.capacity(b) for b in range(3)] == [64, 64, 64]
            logits = m.decode_step(logits.argmax(-1), pool)  # warm: tables, bf16 weight copies, library handles
            for b in (1, 2):
                pool.reserve(b, 9 + 62)  # a second page for rows 1 and 2 before the debug mode
            pool.commit()
            torch.cuda.synchronize()
            prev = torch.cuda.get_sync_debug_mode()
            torch.cuda.set_sync_debug_mode("error")
            try:
                logits = m.decode_step(logits.argmax(-1), pool)
                out = m.decode_loop(logits, pool, 56, eos_id=m.cfg.eos_id)  # rows 1 and 2 cross into page two
            finally:
                torch.cuda.set_sync_debug_mode(prev)
        assert out.shape == (3, 56) and pool.bound == 9 + 1 + 1 + 55
        assert pool.lens.tolist() == [4 + 57, 9 + 57, 9 + 57]
        with torch.autocast("cuda", dtype=BF16), pytest.raises(ValueError, match="reserve"):
            for _ in range(8):  # row 0 has one page: its 65th position is refused, on the host
                m.decode_step(out[:, -1], pool)
