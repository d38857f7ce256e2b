"""Split-KV decode attention on the GPU (attn_decode, ops.attention.decode_attention) against the float64 oracle
of tests/decode_oracle.py on the bf16-rounded inputs: NaN-filled stale keys, lengths around the key tile, every
split count including empty splits, clamped lens, determinism, sliced caches, the host checks, and
Llama.prefill / decode_step / generate under bf16 autocast with no host synchronisation in a step (MI355X only)."""
import copy
import functools

import pytest
import torch

from decode_oracle import decode_oracle64, nan_tail_, teacher_forced

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
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


@pytest.fixture
def no_ref(monkeypatch):
    """the native path must run: the reference raises"""
    def boom(*a, **kw):
        raise AssertionError("decode_attention fell back to the reference")
    monkeypatch.setattr(_att(), "decode_attention_ref", boom)
    return monkeypatch


def _tile():
    return _C().decode_key_tile()


def _smax(which):
    T = _tile()
    return {"1": 1, "T-1": T - 1, "T": T, "T+1": T + 1, "4T+3": 4 * T + 3}[which]


@functools.lru_cache(maxsize=None)
def _case(D, Hq, Hkv, Smax):
    """bf16 inputs on the host with every stale position NaN, the float64 oracle of the visible part and the
    bound 2^-7 * max|v| per (sequence, kv head), expanded to the query heads. Computed once, never changed."""
    T = _tile()
    g = torch.Generator().manual_seed(1000 * D + 10 * Hq + Hkv + Smax)
    lens = torch.tensor([0, 1, T - 1, T, T + 1, Smax]).clamp(max=Smax)[torch.randperm(B, generator=g)].int()
    q = torch.randn(B, Hq, D, generator=g).to(BF16)
    kc = torch.randn(B, Smax, Hkv, D, generator=g).to(BF16)
    vc = (torch.randn(B, Smax, Hkv, D, generator=g) * 2).to(BF16)
    o64, vmax = decode_oracle64(q, kc, vc, lens)
    nan_tail_(kc, vc, lens)
    bound = (2.0 ** -7 * vmax).repeat_interleave(Hq // Hkv, dim=1).unsqueeze(-1)  # [B, Hq, 1]
    return q, kc, vc, lens, o64, bound


def _splits():
    return (1, 2, 3, None, 1000)  # None: the number of key tiles of Smax; 1000 is clamped to it


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
    q, kc, vc, lens, o64, bound = _case(D, *heads, Smax)
    qd, kd, vd, ld = q.to(dev), kc.to(dev), vc.to(dev), lens.to(dev)
    tiles = -(-Smax // _tile())
    outs = []
    for s in _splits():
        s = tiles if s is None else s
        o = att.decode_attention(qd, kd, vd, ld, splits=s)
        _check(o, lens, o64, bound, f"D{D} {heads} Smax {Smax} splits {s}")
        outs.append(o.double().cpu())
    # the clamp: 1000 splits is the number of tiles, bit for bit
    assert torch.equal(outs[-1], outs[-2])
    # split invariance: any two split counts agree within the bound (not bitwise)
    for o in outs[1:]:
        assert ((o - outs[0]).abs() <= bound).all()
    # the heuristic's own choice
    _check(att.decode_attention(qd, kd, vd, ld), lens, o64, bound, f"D{D} {heads} Smax {Smax} default splits")


def test_binding_default_and_explicit_scale(dev):
    q, kc, vc, lens, _, bound = _case(128, 32, 8, _smax("4T+3"))
    o64, _ = decode_oracle64(q, kc, vc, lens, scale=0.3)  # the oracle touches the visible keys only
    o = _C().attn_decode(q.to(dev), kc.to(dev), vc.to(dev), lens.to(dev), 0.3)
    _check(o, lens, o64, bound, "scale 0.3, default splits")
    o = _att().decode_attention(q.to(dev), kc.to(dev), vc.to(dev), lens.to(dev), scale=0.3, splits=2)
    _check(o, lens, o64, bound, "scale 0.3, 2 splits")


def test_split_heuristic():
    C, T = _C(), _tile()
    assert T >= 1 and C.decode_splits(64, 8, 8192) >= 1
    for Bq, Hkv, Smax in ((1, 8, 8192), (8, 8, 2048), (64, 8, 8192), (1, 1, 1), (3, 2, T + 1), (1, 8, 100000)):
        s = C.decode_splits(Bq, Hkv, Smax)
        assert 1 <= s <= max(1, -(-Smax // T))
    assert C.decode_splits(1, 8, 8192) > C.decode_splits(64, 8, 8192)  # fewer (batch, head) pairs: more splits
    assert C.decode_splits(1, 8, T) == 1  # one tile cannot be split


@pytest.mark.parametrize("D", [64, 128])
def test_lens_are_clamped(dev, no_ref, D):
    att = _att()
    Smax = _smax("T+1")
    g = torch.Generator().manual_seed(5)
    q = torch.randn(3, 8, D, generator=g).to(BF16).to(dev)
    kc = torch.randn(3, Smax, 2, D, generator=g).to(BF16).to(dev)
    vc = torch.randn(3, Smax, 2, D, generator=g).to(BF16).to(dev)
    wild = torch.tensor([-5, Smax + 100, 7], dtype=torch.int32, device=dev)
    tame = torch.tensor([0, Smax, 7], dtype=torch.int32, device=dev)
    for s in (1, 2):
        a, b = att.decode_attention(q, kc, vc, wild, splits=s), att.decode_attention(q, kc, vc, tame, splits=s)
        assert torch.equal(a, b) and not torch.isnan(a).any()
        assert torch.equal(a[0], torch.zeros_like(a[0]))


@pytest.mark.parametrize("splits", [1, 3])
def test_determinism_garbage_and_slices(dev, no_ref, splits):
    att = _att()
    q, kc, vc, lens, _, _ = _case(128, 32, 8, _smax("4T+3"))
    qd, ld = q.to(dev), lens.to(dev)
    a = att.decode_attention(qd, kc.to(dev), vc.to(dev), ld, splits=splits)
    assert torch.equal(a, att.decode_attention(qd, kc.to(dev), vc.to(dev), ld, splits=splits))
    for junk in (float("inf"), -3.0e38, 0.0):  # other garbage in the stale region: the same bits
        k2, v2 = nan_tail_(kc.clone(), vc.clone(), lens, junk)
        assert torch.equal(a, att.decode_attention(qd, k2.to(dev), v2.to(dev), ld, splits=splits))
    # cache[:, :n] of a longer cache (NaN behind it) against a contiguous copy of the slice
    n = kc.shape[1]
    longk = torch.full((B, n + 37, *kc.shape[2:]), float("nan"), dtype=BF16, device=dev)
    longv = longk.clone()
    longk[:, :n], longv[:, :n] = kc.to(dev), vc.to(dev)
    assert not longk[:, :n].is_contiguous()
    assert torch.equal(a, att.decode_attention(qd, longk[:, :n], longv[:, :n], ld, splits=splits))


def test_host_checks_and_fallback(dev):
    att, C = _att(), _C()
    Smax, Hq, Hkv, D = 9, 4, 2, 64
    g = torch.Generator().manual_seed(6)

    def mk(Hq=Hq, Hkv=Hkv, D=D):
        return (torch.randn(2, Hq, D, generator=g).to(BF16).to(dev), torch.randn(2, Smax, Hkv, D, generator=g).to(BF16).to(dev),
                torch.randn(2, Smax, Hkv, D, generator=g).to(BF16).to(dev), torch.tensor([9, 4], dtype=torch.int32, device=dev))

    q, kc, vc, lens = mk()
    cases = []
    cases.append(("bfloat16", (q.float(), kc, vc, lens)))
    cases.append(("head_dim must be 64 or 128", mk(D=96)))
    cases.append(("query heads per kv head", mk(Hq=6)))
    cases.append(("lens must be int32", (q, kc, vc, lens.long())))
    buf = torch.zeros(q.numel() + 8, dtype=BF16, device=dev)
    off = buf[1:1 + q.numel()].view_as(q).copy_(q)
    assert off.is_contiguous() and off.data_ptr() % 16 != 0
    cases.append(("16-byte aligned", (off, kc, vc, lens)))
    wide = torch.randn(2, Smax, Hkv, 2 * D, generator=g).to(BF16).to(dev)
    cases.append(("inner three dimensions", (q, wide[..., ::2], vc, lens)))
    for msg, args in cases:
        with pytest.raises(RuntimeError, match=msg):
            C.attn_decode(*args, 0.125)
        assert not att.decode_native_ok(*args)
        o = att.decode_attention(*args)  # the reference, without raising
        o64, vmax = decode_oracle64(*[t.cpu() for t in args])
        assert o.dtype == args[0].dtype
        assert ((o.double().cpu() - o64).abs().max() <= 2.0 ** -7 * vmax.max())
    assert att.decode_native_ok(q, kc, vc, lens)
    for t in (q, kc, vc):
        with pytest.raises(RuntimeError, match="inference only"):
            t.requires_grad_()
            try:
                att.decode_attention(q, kc, vc, lens)
            finally:
                t.requires_grad_(False)


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


@pytest.mark.parametrize("qk_norm", [False, True], ids=["plain", "qk_norm"])
def test_model_teacher_forced(dev, no_ref, qk_norm):
    """llama-tiny (hd 64, G 2) under bf16 autocast: the decode path's logits against a float64 CPU copy of the
    same weights may err at most 2x what the GPU's own full forward errs against it, plus 2^-8 max|logits|
    (the two paths do not share the attention's rounding). Measured figures are in docs/decode_attention.md."""
    att = _att()
    m, m64 = _tiny(dev, qk_norm)
    Bm, S, lens = 2, 24, (5, 11)
    tokens = torch.randint(1, m.cfg.vocab_size, (Bm, S), generator=torch.Generator().manual_seed(4))
    with torch.no_grad():
        ref = m64(tokens)
    with torch.autocast("cuda", dtype=BF16):
        with torch.no_grad():
            full = m(tokens.to(dev)).double().cpu()
        cache = att.KVCache.allocate(m.cfg, Bm, S + max(lens) - min(lens), dev, m.cache_dtype(dev))
        assert cache.k.dtype == BF16
        cache.k.fill_(float("nan"))
        cache.v.fill_(float("nan"))
        got = teacher_forced(m, tokens.to(dev), lens, cache)
    assert sorted((b, t) for b, t, _ in got) == sorted((b, t) for b in range(Bm) for t in range(lens[b] - 1, S))
    e_dec = max((lg.double().cpu() - ref[b, t]).abs().max().item() for b, t, lg in got)
    e_full = max((full[b, t] - ref[b, t]).abs().max().item() for b, t, _ in got)
    top = ref.abs().max().item()
    print(f"model teacher-forced (qk_norm={qk_norm}): decode {e_dec:.3e}, full forward {e_full:.3e}, max|logits| {top:.3e}")
    assert e_dec <= 2 * e_full + 2.0 ** -8 * top


def test_model_generate(dev, no_ref):
    m, _ = _tiny(dev, False)
    tokens = torch.randint(1, m.cfg.vocab_size, (3, 9), generator=torch.Generator().manual_seed(12)).to(dev)
    with torch.autocast("cuda", dtype=BF16):
        out = m.generate(tokens, 12, prompt_lens=torch.tensor([4, 9, 9]))
        smp = m.generate(tokens, 12, temperature=0.8, top_k=20, eos_id=m.cfg.eos_id,
                         generator=torch.Generator(device=dev).manual_seed(1))
    for t in (out, smp):
        assert t.dtype == torch.int64 and t.shape == (3, 12) and t.device.type == "cuda"
        assert int(t.min()) >= 0 and int(t.max()) < m.cfg.vocab_size


def test_no_host_sync_in_decode(dev, no_ref):
    att = _att()
    m, _ = _tiny(dev, True)
    tokens = torch.randint(1, m.cfg.vocab_size, (3, 9), generator=torch.Generator().manual_seed(13)).to(dev)
    with torch.autocast("cuda", dtype=BF16):
        cache = att.KVCache.allocate(m.cfg, 3, 9 + 8, dev, m.cache_dtype(dev))
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
