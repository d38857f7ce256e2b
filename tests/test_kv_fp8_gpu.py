"""The FP8 KV cache on the GPU (kv_append_fp8, attn_decode_fp8; ops.attention.kv_cache_append / decode_attention):
the quantising append byte for byte against the independent quantiser of tests/kv_fp8_oracle.py (positions, the
clamp, untouched bytes, determinism), FP8 decode attention against the float64 oracle of the dequantised caches on
the grid of tests/test_decode_gpu.py with NaN codes and NaN scales in the stale region, the host checks, and
Llama.prefill / decode_step / generate with an FP8 cache under bf16 autocast (MI355X only)."""
import copy
import functools

import pytest
import torch

from decode_oracle import teacher_forced
from kv_fp8_oracle import FP8, attention_oracle, magnitude_rows, quantize_oracle, stale_tail_

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
HEADS = [(4, 4), (4, 2), (8, 1), (32, 8)]
B = 6


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
    def boom_attn(*a, **kw):
        raise AssertionError("decode_attention fell back to the reference")

    def boom_quant(*a, **kw):
        raise AssertionError("kv_cache_append fell back to the reference")
    monkeypatch.setattr(_att(), "decode_attention_ref", boom_attn)
    monkeypatch.setattr(_att(), "kv_quantize_ref", boom_quant)


@pytest.fixture
def no_ref(monkeypatch):
    """the native paths must run: both references raise"""
    _forbid_refs(monkeypatch)
    return monkeypatch


def _bytes(t):
    return t.view(torch.uint8)


def _tile():
    return _C().decode_key_tile()


# ------------------------------------------------------------------ the append
def _pattern(Bn, Smax, Hkv, D, dev):
    """caches and scales holding a pattern that no append writes"""
    kc = torch.full((Bn, Smax, Hkv, D), 0x5A, dtype=torch.uint8, device=dev).view(FP8)
    vc = torch.full((Bn, Smax, Hkv, D), 0xA5, dtype=torch.uint8, device=dev).view(FP8)
    ks = torch.full((Bn, Smax, Hkv), -7.0, device=dev)
    vs = torch.full((Bn, Smax, Hkv), -9.0, device=dev)
    return kc, vc, ks, vs


def _expected(bufs, k, v, pos):
    """the host's copy of `bufs` after appending k, v at pos: the oracle's bytes, tokens of a row in order (of
    tokens the clamp folds onto one position the last stays)"""
    want = [t.cpu().clone() for t in bufs]
    Smax = want[0].shape[1]
    (qk, sk), (qv, sv) = quantize_oracle(k), quantize_oracle(v)
    for b in range(k.shape[0]):
        for s in range(k.shape[1]):
            p = min(max((0 if pos is None else int(pos[b])) + s, 0), Smax - 1)
            _bytes(want[0])[b, p], _bytes(want[1])[b, p] = _bytes(qk)[b, s], _bytes(qv)[b, s]
            want[2][b, p], want[3][b, p] = sk[b, s], sv[b, s]
    return want


def _same_bytes(got, want, what):
    for name, a, b in zip(("k codes", "v codes", "k scales", "v scales"), got, want):
        assert torch.equal(_bytes(a.cpu()), _bytes(b)), f"{what}: {name} differ from the oracle"


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("Hkv", [1, 2, 8])
@pytest.mark.parametrize("D", [64, 128])
def test_append_positions(dev, no_ref, D, Hkv, S):
    """Smax 11, B 5: no pos; ragged pos with a row that ends exactly at the end, one at Smax - 1 (S 3: its tokens
    fold onto the last position), one far past the end and one below zero"""
    att = _att()
    Bn, Smax = 5, 11
    g = torch.Generator().manual_seed(100 * D + 10 * Hkv + S)
    k = (torch.randn(Bn, S, Hkv, D, generator=g) * 3).to(BF16)
    v = (torch.randn(Bn, S, Hkv, D, generator=g) * 0.01).to(BF16)
    for pos in (None, (0, Smax - S, Smax - 1, Smax + 1000, -2)):
        bufs = _pattern(Bn, Smax, Hkv, D, dev)
        want = _expected(bufs, k, v, pos)
        posd = None if pos is None else torch.tensor(pos, dtype=torch.int32, device=dev)
        att.kv_cache_append(*bufs, k.to(dev), v.to(dev), posd)
        _same_bytes(bufs, want, f"D{D} Hkv{Hkv} S{S} pos {pos}")  # the pattern everywhere else included
        again = _pattern(Bn, Smax, Hkv, D, dev)
        att.kv_cache_append(*again, k.to(dev), v.to(dev), posd)
        for a, b in zip(bufs, again):
            assert torch.equal(_bytes(a), _bytes(b))


@pytest.mark.parametrize("D", [64, 128])
def test_append_magnitudes_and_edge_rows(dev, no_ref, D):
    """rows of magnitude 1e-6 .. 1e6, the zero row, the one-element row, amax at 448 * 2^k and just above: more
    than one workgroup, a row count that is no multiple of the rows per workgroup"""
    att = _att()
    rows = magnitude_rows(1000, D, seed=D)
    n = rows.shape[0] // 2
    k, v = rows[:2 * n].view(2, n, 1, D).contiguous(), rows[:2 * n].flip(0).view(2, n, 1, D).contiguous()
    bufs = _pattern(2, n + 3, 1, D, dev)
    want = _expected(bufs, k, v, None)
    att.kv_cache_append(*bufs, k.to(dev), v.to(dev))
    _same_bytes(bufs, want, f"D{D} magnitudes")


def test_append_into_a_slice_and_fallback(dev):
    """cache[:, :n] of a longer cache is an operand of the kernel; fp32 rows go through the reference, on the
    GPU, to the same bytes"""
    att = _att()
    g = torch.Generator().manual_seed(7)
    k, v = torch.randn(3, 2, 2, 64, generator=g).to(BF16), torch.randn(3, 2, 2, 64, generator=g).to(BF16)
    pos = (0, 3, 9)
    for dtype in (BF16, F32):
        long_ = _pattern(3, 12, 2, 64, dev)
        part = tuple(t[:, :5] for t in long_)
        want = [t.cpu().clone() for t in long_]  # the pattern, then the slice's positions (9 is clamped to 4)
        for w, r in zip(want, _expected(part, k, v, pos)):
            _bytes(w)[:, :5] = _bytes(r)
        kd, vd, posd = k.to(dev, dtype), v.to(dev, dtype), torch.tensor(pos, dtype=torch.int32, device=dev)
        assert att.kv_append_native_ok(*part, kd, vd, posd) == (dtype == BF16)
        att.kv_cache_append(*part, kd, vd, posd)
        _same_bytes(long_, want, f"slice, {dtype}")


def test_append_host_checks(dev):
    C = _C()
    g = torch.Generator().manual_seed(8)

    def mk(D=64, Hkv=2):
        k = torch.randn(2, 1, Hkv, D, generator=g).to(BF16).to(dev)
        return list(_pattern(2, 4, Hkv, D, dev)) + [k, k.clone()]

    base = mk()
    cases = []
    cases.append(("k and v must be bfloat16", base[:4] + [base[4].float(), base[5]], None))
    cases.append(("caches must be float8_e4m3fn", [_bytes(base[0])] + base[1:], None))
    cases.append(("scales must be fp32", base[:2] + [base[2].double()] + base[3:], None))
    cases.append(("head_dim must be 64 or 128", mk(D=96), None))
    wide = torch.randn(2, 1, 2, 128, generator=g).to(BF16).to(dev)
    cases.append(("contiguous", base[:4] + [wide[..., ::2], base[5]], None))
    cases.append(("scales must be", base[:2] + [base[2][:, :3], base[3]] + base[4:], None))
    cases.append(("pos must be", base, torch.zeros(2, dtype=torch.int64, device=dev)))
    cases.append(("pos must be", base, torch.zeros(3, dtype=torch.int32, device=dev)))
    cases.append(("pos must be", base, torch.zeros(2, dtype=torch.int32)))
    for msg, args, pos in cases:
        with pytest.raises(RuntimeError, match=msg):
            C.kv_append_fp8(*args, pos)
    C.kv_append_fp8(*base, torch.zeros(2, dtype=torch.int32, device=dev))  # and the base case is accepted


# ------------------------------------------------------------------ attention on an FP8 cache
def _smax(which):
    T = _tile()
    return {"1": 1, "T-1": T - 1, "T": T, "T+1": T + 1, "4T+3": 4 * T + 3}[which]


@functools.lru_cache(maxsize=None)
def _case(D, Hq, Hkv, Smax):
    """bf16 q and caches from the oracle quantiser on the host, every stale position holding NaN codes (0x7F) and
    NaN scales, the float64 oracle of the dequantised visible part and the bound 2^-7 * max|v_deq| per (sequence,
    kv head), expanded to the query heads. Computed once, never changed."""
    T = _tile()
    g = torch.Generator().manual_seed(1000 * D + 10 * Hq + Hkv + Smax)
    lens = torch.tensor([0, 1, T - 1, T, T + 1, Smax]).clamp(max=Smax)[torch.randperm(B, generator=g)].int()
    q = torch.randn(B, Hq, D, generator=g).to(BF16)
    # rows of different magnitudes, so the scales differ from key to key
    mag = torch.logspace(-2, 2, Smax)[torch.randperm(Smax, generator=g)].view(1, Smax, 1, 1)
    kc, ks = quantize_oracle(torch.randn(B, Smax, Hkv, D, generator=g) * mag.sqrt())
    vc, vs = quantize_oracle(torch.randn(B, Smax, Hkv, D, generator=g) * 2 * mag.flip(1))
    o64, vmax = attention_oracle(q, kc, vc, ks, vs, lens)
    stale_tail_(kc, vc, ks, vs, lens)
    bound = (2.0 ** -7 * vmax).repeat_interleave(Hq // Hkv, dim=1).unsqueeze(-1)  # [B, Hq, 1]
    return q, kc, vc, ks, vs, lens, o64, bound


def _on(dev, *ts):
    return tuple(t.to(dev) for t in ts)


def _check(o, lens, o64, bound, what):
    assert o.dtype == BF16 and o.shape == o64.shape
    o = o.double().cpu()
    assert not torch.isnan(o).any(), what
    err = (o - o64).abs()
    worst = (err - bound).max().item()
    print(f"{what}: max err {err.max().item():.3e}, tightest bound {bound[bound > 0].min().item() if (bound > 0).any() else 0:.3e}")
    assert (err <= bound).all(), f"{what}: error exceeds 2^-7 max|v| by {worst:.3e}"
    for b in range(len(lens)):
        if int(lens[b]) <= 0:
            assert torch.equal(o[b], torch.zeros_like(o[b])), f"{what}: a row of length 0 is not exactly zero"


@pytest.mark.parametrize("smax", ["1", "T-1", "T", "T+1", "4T+3"])
@pytest.mark.parametrize("heads", HEADS, ids=lambda h: f"hq{h[0]}_hkv{h[1]}")
@pytest.mark.parametrize("D", [64, 128])
def test_kernel_against_float64(dev, no_ref, D, heads, smax):
    att = _att()
    Smax = _smax(smax)
    q, kc, vc, ks, vs, lens, o64, bound = _case(D, *heads, Smax)
    qd, kd, vd, ksd, vsd, ld = _on(dev, q, kc, vc, ks, vs, lens)
    assert att.decode_native_ok(qd, kd, vd, ld, ksd, vsd)
    tiles = -(-Smax // _tile())
    outs = []
    for s in (1, 2, 3, tiles, 1000):
        o = att.decode_attention(qd, kd, vd, ld, splits=s, k_scale=ksd, v_scale=vsd)
        _check(o, lens, o64, bound, f"FP8 D{D} {heads} Smax {Smax} splits {s}")
        outs.append(o.double().cpu())
    assert torch.equal(outs[-1], outs[-2])  # 1000 splits is clamped to the number of tiles
    for o in outs[1:]:
        assert ((o - outs[0]).abs() <= bound).all()
    _check(att.decode_attention(qd, kd, vd, ld, k_scale=ksd, v_scale=vsd), lens, o64, bound,
           f"FP8 D{D} {heads} Smax {Smax} default splits")


def test_binding_scale_argument(dev):
    q, kc, vc, ks, vs, lens, _, bound = _case(128, 32, 8, _smax("4T+3"))
    o64, _ = attention_oracle(q, kc, vc, ks, vs, lens, scale=0.3)  # the oracle touches the visible keys only
    o = _C().attn_decode_fp8(*_on(dev, q, kc, vc, ks, vs, lens), 0.3)
    _check(o, lens, o64, bound, "FP8 scale 0.3, default splits")


@pytest.mark.parametrize("D", [64, 128])
def test_lens_are_clamped(dev, no_ref, D):
    att = _att()
    Smax = _smax("T+1")
    g = torch.Generator().manual_seed(5)
    q = torch.randn(3, 8, D, generator=g).to(BF16).to(dev)
    (kc, ks), (vc, vs) = (_on(dev, *quantize_oracle(torch.randn(3, Smax, 2, D, generator=g))) for _ in range(2))
    wild = torch.tensor([-5, Smax + 100, 7], dtype=torch.int32, device=dev)
    tame = torch.tensor([0, Smax, 7], dtype=torch.int32, device=dev)
    for s in (1, 2):
        a = att.decode_attention(q, kc, vc, wild, splits=s, k_scale=ks, v_scale=vs)
        b = att.decode_attention(q, kc, vc, tame, splits=s, k_scale=ks, v_scale=vs)
        assert torch.equal(a, b) and not torch.isnan(a).any()
        assert torch.equal(a[0], torch.zeros_like(a[0]))


@pytest.mark.parametrize("splits", [1, 3])
def test_determinism_garbage_and_slices(dev, no_ref, splits):
    att = _att()
    q, kc, vc, ks, vs, lens, _, _ = _case(128, 32, 8, _smax("4T+3"))
    qd, kd, vd, ksd, vsd, ld = _on(dev, q, kc, vc, ks, vs, lens)
    a = att.decode_attention(qd, kd, vd, ld, splits=splits, k_scale=ksd, v_scale=vsd)
    assert torch.equal(a, att.decode_attention(qd, kd, vd, ld, splits=splits, k_scale=ksd, v_scale=vsd))
    # other garbage in the stale region (codes 0, 0x7E = 448, 0xFF = NaN; scales inf, 0, huge): the same bits
    for code, junk in ((0x00, float("inf")), (0x7E, 0.0), (0xFF, 3.0e38)):
        k2, v2, ks2, vs2 = (t.clone() for t in (kc, vc, ks, vs))
        for b in range(B):
            n = int(lens[b])
            _bytes(k2)[b, n:], _bytes(v2)[b, n:] = code, code
            ks2[b, n:], vs2[b, n:] = junk, junk
        got = att.decode_attention(qd, *_on(dev, k2, v2), ld, splits=splits, k_scale=ks2.to(dev), v_scale=vs2.to(dev))
        assert torch.equal(a, got)
    # cache[:, :n] of a longer cache (NaN codes and scales behind it) against a contiguous copy of the slice
    n = kc.shape[1]
    longk = torch.full((B, n + 37, *kc.shape[2:]), 0x7F, dtype=torch.uint8, device=dev).view(FP8)
    longv = longk.clone()
    longks = torch.full((B, n + 37, kc.shape[2]), float("nan"), device=dev)
    longvs = longks.clone()
    _bytes(longk)[:, :n], _bytes(longv)[:, :n] = _bytes(kd), _bytes(vd)
    longks[:, :n], longvs[:, :n] = ksd, vsd
    assert not longk[:, :n].is_contiguous() and not longks[:, :n].is_contiguous()
    got = att.decode_attention(qd, longk[:, :n], longv[:, :n], ld, splits=splits, k_scale=longks[:, :n],
                               v_scale=longvs[:, :n])
    assert torch.equal(a, got)


@pytest.mark.parametrize("splits", [1, 3])
@pytest.mark.parametrize("heads", [(4, 4), (32, 8)], ids=lambda h: f"hq{h[0]}_hkv{h[1]}")
@pytest.mark.parametrize("D", [64, 128])
def test_same_bits_as_bf16_on_the_dequantised_cache(dev, no_ref, D, heads, splits):
    """The two cache formats are instantiations of one kernel and the scales are powers of two, so a scale moves
    only exponents: (q . k8) * ks is q . (k8 * ks) and p * vs * v8 is p * (v8 * vs), rounding for rounding. The
    FP8 kernel therefore returns the bits of the bf16 kernel on the dequantised cache. Rows from randn keep every
    intermediate far from the denormal range, where the two could part."""
    att = _att()
    Hq, Hkv = heads
    T = _tile()
    Smax = 4 * T + 3
    g = torch.Generator().manual_seed(10 * D + Hq)
    lens = torch.tensor([0, 1, T - 1, T, T + 1, Smax])[torch.randperm(B, generator=g)].int().to(dev)
    q = torch.randn(B, Hq, D, generator=g).to(BF16).to(dev)
    k, v = (torch.randn(B, Smax, Hkv, D, generator=g).to(BF16).to(dev) for _ in range(2))
    kc, vc = torch.empty_like(k, dtype=FP8), torch.empty_like(v, dtype=FP8)
    ks, vs = torch.empty(B, Smax, Hkv, device=dev), torch.empty(B, Smax, Hkv, device=dev)
    att.kv_cache_append(kc, vc, ks, vs, k, v)
    o8 = att.decode_attention(q, kc, vc, lens, splits=splits, k_scale=ks, v_scale=vs)
    o16 = att.decode_attention(q, att.kv_dequantize(kc, ks, BF16), att.kv_dequantize(vc, vs, BF16), lens, splits=splits)
    assert not torch.isnan(o8).any() and o8.abs().max() > 0
    assert torch.equal(o8, o16)


def test_host_checks_and_fallback(dev):
    att, C = _att(), _C()
    Smax, Hq, Hkv, D = 9, 4, 2, 64
    g = torch.Generator().manual_seed(6)

    def mk(Hq=Hq, Hkv=Hkv, D=D):
        q = torch.randn(2, Hq, D, generator=g).to(BF16).to(dev)
        (kc, ks), (vc, vs) = (_on(dev, *quantize_oracle(torch.randn(2, Smax, Hkv, D, generator=g))) for _ in range(2))
        return [q, kc, vc, ks, vs, torch.tensor([9, 4], dtype=torch.int32, device=dev)]

    q, kc, vc, ks, vs, lens = mk()
    cases = []
    cases.append(("q must be bfloat16", [q.float(), kc, vc, ks, vs, lens]))
    cases.append(("head_dim must be 64 or 128", mk(D=96)))
    cases.append(("query heads per kv head", mk(Hq=6)))
    cases.append(("lens must be int32", [q, kc, vc, ks, vs, lens.long()]))
    buf = torch.zeros(q.numel() + 8, dtype=BF16, device=dev)
    off = buf[1:1 + q.numel()].view_as(q).copy_(q)
    assert off.is_contiguous() and off.data_ptr() % 16 != 0
    cases.append(("16-byte aligned", [off, kc, vc, ks, vs, lens]))
    wide = torch.zeros(2, Smax, 2 * Hkv, device=dev)
    wide[..., ::2] = ks
    cases.append(("inner two dimensions of the scales", [q, kc, vc, wide[..., ::2], vs, lens]))
    for msg, args in cases:
        with pytest.raises(RuntimeError, match=msg):
            C.attn_decode_fp8(*args, 0.125)
        qa, ka, va, ksa, vsa, la = args
        assert not att.decode_native_ok(qa, ka, va, la, ksa, vsa)
        o = att.decode_attention(qa, ka, va, la, k_scale=ksa, v_scale=vsa)  # the reference, without raising
        o64, vmax = attention_oracle(qa, ka, va, ksa, vsa, la)
        assert o.dtype == qa.dtype
        assert (o.double().cpu() - o64).abs().max() <= 2.0 ** -7 * vmax.max()
    # what the binding alone refuses (decode_attention raises ValueError for these before it gets there)
    for msg, args in (("caches must be float8_e4m3fn", [q, kc.to(BF16), vc.to(BF16), ks, vs, lens]),
                      ("scales must be fp32", [q, kc, vc, ks.double(), vs, lens]),
                      (r"scales must be \[B, Smax, Hkv\]", [q, kc, vc, ks[:, :5], vs, lens])):
        with pytest.raises(RuntimeError, match=msg):
            C.attn_decode_fp8(*args, 0.125)
    assert att.decode_native_ok(q, kc, vc, lens, ks, vs)
    with pytest.raises(ValueError, match="need k_scale and v_scale"):
        att.decode_attention(q, kc, vc, lens)
    with pytest.raises(ValueError, match="float8_e4m3fn caches only"):
        att.decode_attention(q, kc.to(BF16), vc.to(BF16), lens, k_scale=ks, v_scale=vs)
    with pytest.raises(RuntimeError, match="inference only"):
        att.decode_attention(q.clone().requires_grad_(), kc, vc, lens, k_scale=ks, v_scale=vs)


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


def _stale_cache(att, cfg, Bm, n, dev):
    cache = att.KVCache.allocate(cfg, Bm, n, dev, FP8)
    assert cache.k.dtype == FP8 and cache.k.element_size() == 1 and cache.k_scale.dtype == F32
    _bytes(cache.k).fill_(0x7F)
    _bytes(cache.v).fill_(0x7F)
    cache.k_scale.fill_(float("nan"))
    cache.v_scale.fill_(float("nan"))
    return cache


@pytest.mark.parametrize("qk_norm", [False, True], ids=["plain", "qk_norm"])
def test_model_teacher_forced(dev, monkeypatch, qk_norm):
    """llama-tiny (hd 64, G 2) under bf16 autocast, teacher-forced through an FP8 cache, against a float64 CPU
    copy of the same weights (m64). No tolerance can be derived for the quantised path: a bf16 rounding ahead of
    the quantiser can move a code by a whole step. The yardstick is therefore computed here from the reference:
    e_q, the largest logit difference between m64 teacher-forced through an FP8 cache on the CPU reference path
    (whose quantiser tests/test_kv_fp8_cpu.py ties byte for byte to the oracle) and m64's own full forward. The
    GPU path may err by 2 * e_full + 2^-8 * top, as the bf16-cache test allows, plus 2 * e_q, the factor 2 for
    the moved codes. Measured figures are in docs/decode_attention.md."""
    att = _att()
    m, m64 = _tiny(dev, qk_norm)
    Bm, S, lens = 2, 24, (5, 11)
    n = S + max(lens) - min(lens)
    tokens = torch.randint(1, m.cfg.vocab_size, (Bm, S), generator=torch.Generator().manual_seed(4))
    with torch.no_grad():
        ref = m64(tokens)
    got64 = teacher_forced(m64, tokens, lens, _stale_cache(att, m64.cfg, Bm, n, torch.device("cpu")))
    e_q = max((lg - ref[b, t]).abs().max().item() for b, t, lg in got64)
    _forbid_refs(monkeypatch)  # from here on the native paths must run
    with torch.autocast("cuda", dtype=BF16):
        with torch.no_grad():
            full = m(tokens.to(dev)).double().cpu()
        got = teacher_forced(m, tokens.to(dev), lens, _stale_cache(att, m.cfg, Bm, n, dev))
    assert sorted((b, t) for b, t, _ in got) == sorted((b, t) for b in range(Bm) for t in range(lens[b] - 1, S))
    e_dec8 = max((lg.double().cpu() - ref[b, t]).abs().max().item() for b, t, lg in got)
    e_full = max((full[b, t] - ref[b, t]).abs().max().item() for b, t, _ in got)
    top = ref.abs().max().item()
    print(f"model teacher-forced, FP8 cache (qk_norm={qk_norm}): decode {e_dec8:.3e}, full forward {e_full:.3e}, "
          f"max|logits| {top:.3e}, e_q {e_q:.3e}")
    assert e_dec8 <= 2 * e_full + 2.0 ** -8 * top + 2 * e_q


def test_model_generate(dev, no_ref):
    att = _att()
    m, _ = _tiny(dev, False)
    made = []
    allocate = att.KVCache.allocate
    no_ref.setattr(att.KVCache, "allocate", lambda *a, **kw: made.append(allocate(*a, **kw)) or made[-1])
    tokens = torch.randint(1, m.cfg.vocab_size, (3, 9), generator=torch.Generator().manual_seed(12)).to(dev)
    with torch.autocast("cuda", dtype=BF16):
        out = m.generate(tokens, 12, prompt_lens=torch.tensor([4, 9, 9]), kv_dtype="fp8")
        smp = m.generate(tokens, 12, temperature=0.8, top_k=20, eos_id=m.cfg.eos_id, kv_dtype=FP8,
                         generator=torch.Generator(device=dev).manual_seed(1))
    for t in (out, smp):
        assert t.dtype == torch.int64 and t.shape == (3, 12) and t.device.type == "cuda"
        assert int(t.min()) >= 0 and int(t.max()) < m.cfg.vocab_size
    assert len(made) == 2
    for cache in made:
        assert cache.k.dtype == FP8 and cache.k.element_size() == 1 and cache.v.element_size() == 1
        assert cache.k_scale.shape == cache.k.shape[:-1] and cache.k_scale.dtype == F32


def test_no_host_sync_in_decode(dev, no_ref):
    att = _att()
    m, _ = _tiny(dev, True)
    tokens = torch.randint(1, m.cfg.vocab_size, (3, 9), generator=torch.Generator().manual_seed(13)).to(dev)
    with torch.autocast("cuda", dtype=BF16):
        cache = att.KVCache.allocate(m.cfg, 3, 9 + 8, dev, FP8)
        logits = m.prefill(tokens, cache, torch.tensor([4, 9, 9]))
        logits = m.decode_step(logits.argmax(-1), cache)  # warm: tables, bf16 weight copies, library handles
        torch.cuda.synchronize()
        prev = torch.cuda.get_sync_debug_mode()
        torch.cuda.set_sync_debug_mode("error")
        try:
            logits = m.decode_step(logits.argmax(-1), cache)
            out = m.decode_loop(logits, cache, 6, eos_id=m.cfg.eos_id)
        finally:
            torch.cuda.set_sync_debug_mode(prev)
    assert out.shape == (3, 6) and cache.bound == 9 + 1 + 1 + 5
    assert cache.lens.tolist() == [4 + 7, 9 + 7, 9 + 7]
