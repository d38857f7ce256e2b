"""The FP8 KV cache off the GPU: ops.attention.kv_quantize_ref byte for byte against the independent quantiser of
tests/kv_fp8_oracle.py, the bounds the format implies, kv_cache_append (positions, clamping, untouched bytes),
decode_attention on an FP8 cache against the float64 oracle of the dequantised values, Llama.generate with an FP8
cache, and the refusals."""
import pytest
import torch

from decode_oracle import teacher_forced
from kv_fp8_oracle import (FP8, attention_oracle, dequantize_oracle, magnitude_rows, quantize_oracle, stale_tail_)

CPU = torch.device("cpu")
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64


def _att():
    from cs744_pytorch_distributed_tutorial_amd.ops import attention
    return attention


def _tiny(seed=0, dtype=F32):
    from cs744_pytorch_distributed_tutorial_amd.models import llama
    torch.manual_seed(seed)
    return llama.build("llama-tiny").to(dtype).eval()


def _bytes(t):
    return t.view(torch.uint8)


# ------------------------------------------------------------------ the format
@pytest.mark.parametrize("dtype", [BF16, F32, F64], ids=["bf16", "fp32", "fp64"])
@pytest.mark.parametrize("D", [64, 128])
def test_quantize_ref_is_the_oracle_byte_for_byte(dtype, D):
    x = magnitude_rows(1000, D, seed=D, dtype=dtype)
    codes, scale = _att().kv_quantize_ref(x)
    want_codes, want_scale = quantize_oracle(x)
    assert codes.dtype == FP8 and codes.shape == x.shape and scale.dtype == F32 and scale.shape == x.shape[:-1]
    assert torch.equal(_bytes(scale), _bytes(want_scale))
    assert torch.equal(_bytes(codes), _bytes(want_codes))


def test_format_bounds():
    """what section 1 of the format implies, on bf16 rows of magnitude 1e-6 .. 1e6 and the edge rows"""
    att = _att()
    x = magnitude_rows(1000, 128, seed=1)
    codes, scale = att.kv_quantize_ref(x)
    x64, amax = x.double(), x.double().abs().amax(-1)
    # the scale: a power of two, 1 for a zero row, amax / s in (224, 448] otherwise
    m, _ = torch.frexp(scale)
    assert (m == 0.5).all()
    assert (scale[amax == 0] == 1).all() and (amax == 0).sum() == 1
    r = (amax / scale.double())[amax > 0]
    assert (r > 224).all() and (r <= 448).all()
    # no code beyond +-448, none NaN (torch's cast does not saturate: 0x7F would be a NaN)
    c = codes.float()
    assert not torch.isnan(c).any() and c.abs().max() <= 448
    assert (c.abs().amax(-1)[amax > 0] >= 224).all()  # 225 rounds to the code 224
    # |deq - x| <= max(2^-4 |x|, 2^-10 s): half an ulp of a 3-bit mantissa, or half the subnormal step 2^-9 s
    deq = dequantize_oracle(codes, scale)
    err = (deq - x64).abs()
    bound = torch.maximum(2.0 ** -4 * x64.abs(), 2.0 ** -10 * scale.double().unsqueeze(-1))
    print(f"quantisation: worst err / bound {(err / bound).max().item():.4f}")
    assert (err <= bound).all()
    # a dequantised value is a bf16 number, and kv_dequantize gives it in any dtype
    for dt in (BF16, F32, F64):
        assert torch.equal(att.kv_dequantize(codes, scale, dt).double(), deq)
    # the single non-zero element of its row survives, the zeros stay zeros
    one = (x64 != 0).sum(-1) == 1
    assert one.sum() == 1 and ((deq[one] != 0).sum() == 1)


def test_allocate():
    att = _att()
    m = _tiny()
    c = att.KVCache.allocate(m.cfg, 3, 17, CPU, FP8)
    assert c.k.shape == c.v.shape == (2, 3, 17, 2, 64) and c.k.dtype == c.v.dtype == FP8 and c.k.element_size() == 1
    assert c.k_scale.shape == c.v_scale.shape == (2, 3, 17, 2) and c.k_scale.dtype == c.v_scale.dtype == F32
    assert c.k_scale.data_ptr() != c.v_scale.data_ptr()
    b = att.KVCache.allocate(m.cfg, 3, 17, CPU, F32)
    assert b.k_scale is None and b.v_scale is None


# ------------------------------------------------------------------ the append
def _append_case(S, pos, Smax=9, B=3, Hkv=2, D=64, seed=2):
    """-> caches pre-filled with a pattern, after the append, and what every position must hold"""
    att = _att()
    g = torch.Generator().manual_seed(seed + S)
    k = (torch.randn(B, S, Hkv, D, generator=g) * 3).to(BF16)
    v = (torch.randn(B, S, Hkv, D, generator=g) * 0.01).to(BF16)
    kc = torch.full((B, Smax, Hkv, D), 0x5A, dtype=torch.uint8).view(FP8)
    vc = torch.full((B, Smax, Hkv, D), 0xA5, dtype=torch.uint8).view(FP8)
    ks, vs = torch.full((B, Smax, Hkv), -7.0), torch.full((B, Smax, Hkv), -9.0)
    want = [t.clone() for t in (kc, vc, ks, vs)]
    (qk, sk), (qv, sv) = quantize_oracle(k), quantize_oracle(v)
    for b in range(B):
        for s in range(S):  # in order: of tokens folded onto one position the last one stays
            p = min(max((0 if pos is None else int(pos[b])) + s, 0), Smax - 1)
            _bytes(want[0])[b, p], _bytes(want[1])[b, p] = _bytes(qk)[b, s], _bytes(qv)[b, s]
            want[2][b, p], want[3][b, p] = sk[b, s], sv[b, s]
    att.kv_cache_append(kc, vc, ks, vs, k, v, None if pos is None else torch.tensor(pos, dtype=torch.int32))
    return (kc, vc, ks, vs), want


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("pos", [None, (0, 4, 6), (8, 7, 100), (-2, 0, 5)], ids=["none", "ragged", "past_end", "negative"])
def test_append_cpu(S, pos):
    """Smax 9: (8, 7, 100) runs rows past the end (clamped onto position 8), (-2, ..) below 0"""
    got, want = _append_case(S, pos)
    for a, b in zip(got, want):
        assert torch.equal(_bytes(a), _bytes(b))
    written = (got[2] != -7.0).sum().item()
    assert 0 < written <= 3 * S * 2  # everything else still holds the pattern (compared above, counted here)


def test_append_into_a_slice_of_a_longer_cache():
    att = _att()
    g = torch.Generator().manual_seed(3)
    k, v = torch.randn(2, 3, 2, 64, generator=g).to(BF16), torch.randn(2, 3, 2, 64, generator=g).to(BF16)
    longk, longv = torch.zeros(2, 12, 2, 64).to(FP8), torch.zeros(2, 12, 2, 64).to(FP8)
    lks, lvs = torch.zeros(2, 12, 2), torch.zeros(2, 12, 2)
    att.kv_cache_append(longk[:, :5], longv[:, :5], lks[:, :5], lvs[:, :5], k, v, torch.tensor([1, 4], dtype=torch.int32))
    (qk, sk), (qv, sv) = quantize_oracle(k), quantize_oracle(v)
    assert torch.equal(_bytes(longk[0, 1:4]), _bytes(qk[0])) and torch.equal(lvs[0, 1:4], sv[0])
    assert torch.equal(_bytes(longv[1, 4]), _bytes(qv[1, 2])) and torch.equal(lks[1, 4], sk[1, 2])  # clamped at 4
    assert (lks[:, 5:] == 0).all() and (_bytes(longk[:, 5:]) == 0).all()


# ------------------------------------------------------------------ attention on an FP8 cache
@pytest.mark.parametrize("heads", [(4, 4), (4, 2), (8, 1)], ids=lambda h: f"hq{h[0]}_hkv{h[1]}")
def test_decode_attention_fp8_cpu_against_float64(heads):
    att = _att()
    Hq, Hkv = heads
    B, Smax, D = 5, 19, 64
    lens = torch.tensor([0, 1, 7, 18, 19], dtype=torch.int32)
    g = torch.Generator().manual_seed(4)
    q = torch.randn(B, Hq, D, generator=g)
    (kc, ks), (vc, vs) = (quantize_oracle(torch.randn(B, Smax, Hkv, D, generator=g) * m) for m in (1.0, 2.0))
    o64, vmax = attention_oracle(q, kc, vc, ks, vs, lens)
    stale_tail_(kc, vc, ks, vs, lens)
    assert not att.decode_native_ok(q, kc, vc, lens, ks, vs)
    o = att.decode_attention(q, kc, vc, lens, splits=3, k_scale=ks, v_scale=vs)
    assert o.dtype == F32 and o.shape == (B, Hq, D) and not torch.isnan(o).any()
    assert torch.equal(o, att.decode_attention_ref(q, kc, vc, lens, k_scale=ks, v_scale=vs))
    assert torch.equal(o[0], torch.zeros(Hq, D))
    assert torch.equal(o[1].double(), dequantize_oracle(vc, vs)[1, 0].repeat_interleave(Hq // Hkv, dim=0))
    # the reference's own fp32 accuracy, as in test_decode_cpu.test_ref_against_float64_loop
    err = (o.double() - o64).abs().max().item()
    print(f"decode_attention (FP8 cache, CPU) vs float64: max err {err:.3e}")
    assert err <= 64 * 2.0 ** -24 * vmax.max().item()
    # fp64 queries: fp64 math on the dequantised cache
    o = att.decode_attention(q.double(), kc, vc, lens, k_scale=ks, v_scale=vs)
    assert o.dtype == F64 and (o - o64).abs().max() < 1e-13
    # a [:, :n] slice of the cache and its scales
    a = att.decode_attention(q, kc[:, :7], vc[:, :7], lens, k_scale=ks[:, :7], v_scale=vs[:, :7])
    b = att.decode_attention(q, kc[:, :7].contiguous(), vc[:, :7].contiguous(), lens, k_scale=ks[:, :7].contiguous(),
                             v_scale=vs[:, :7].contiguous())
    assert torch.equal(a, b)
    o7, _ = attention_oracle(q, kc[:, :7], vc[:, :7], ks[:, :7], vs[:, :7], lens)
    assert (a.double() - o7).abs().max().item() <= 64 * 2.0 ** -24 * vmax.max().item()


def test_mismatched_arguments_raise():
    att = _att()
    q, kc, vc = torch.randn(2, 4, 64), torch.randn(2, 5, 2, 64), torch.randn(2, 5, 2, 64)
    lens = torch.tensor([5, 2], dtype=torch.int32)
    (k8, ks), (v8, vs) = att.kv_quantize_ref(kc), att.kv_quantize_ref(vc)
    for fn in (att.decode_attention, att.decode_attention_ref):
        with pytest.raises(ValueError, match="need k_scale and v_scale"):
            fn(q, k8, v8, lens)
        with pytest.raises(ValueError, match="need k_scale and v_scale"):
            fn(q, k8, v8, lens, k_scale=ks)
        with pytest.raises(ValueError, match="float8_e4m3fn caches only"):
            fn(q, kc, vc, lens, k_scale=ks, v_scale=vs)
        with pytest.raises(ValueError, match="one cache is float8_e4m3fn"):
            fn(q, k8, vc, lens, k_scale=ks, v_scale=vs)
        with pytest.raises(ValueError, match="must be fp32"):
            fn(q, k8, v8, lens, k_scale=ks.double(), v_scale=vs)
        with pytest.raises(ValueError, match=r"\[B, Smax, Hkv\]"):
            fn(q, k8, v8, lens, k_scale=ks[:, :3], v_scale=vs)
    k, v = kc[:, :1].contiguous(), vc[:, :1].contiguous()
    with pytest.raises(ValueError, match="must be float8_e4m3fn"):
        att.kv_cache_append(kc, vc, ks, vs, k, v)
    with pytest.raises(ValueError, match="needs its fp32 scales"):
        att.kv_cache_append(k8, v8, None, vs, k, v)
    with pytest.raises(ValueError, match="do not take"):
        att.kv_cache_append(k8, v8, ks, vs, k[:1], v[:1])
    with pytest.raises(ValueError, match="the scales must be"):
        att.kv_cache_append(k8, v8, ks[:, :2], vs[:, :2], k, v)
    with pytest.raises(ValueError, match="pos must be"):
        att.kv_cache_append(k8, v8, ks, vs, k, v, torch.zeros(3, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="inference only"):
        att.kv_cache_append(k8, v8, ks, vs, k.clone().requires_grad_(), v)


# ------------------------------------------------------------------ the model
def test_model_teacher_forced_fp8_cache_cpu():
    """float64 llama-tiny teacher-forced through an FP8 cache on the reference path: every position is reported,
    the cache ends at the right lengths, and the logits stay near the full forward's. How near is e_q of
    tests/test_kv_fp8_gpu.py's model test, a figure and not a derived bound (measured here: 2.7e-2 at
    max|logits| 1.3); the assertion only separates a working cache from a broken one, whose logits are off by
    the size of the logits themselves."""
    att = _att()
    m64 = _tiny(dtype=F64)
    B, S, lens = 2, 24, (5, 11)
    tokens = torch.randint(1, m64.cfg.vocab_size, (B, S), generator=torch.Generator().manual_seed(4))
    with torch.no_grad():
        ref = m64(tokens)
    cache = att.KVCache.allocate(m64.cfg, B, S + max(lens) - min(lens), CPU, FP8)
    _bytes(cache.k).fill_(0x7F)
    _bytes(cache.v).fill_(0x7F)
    cache.k_scale.fill_(float("nan"))
    cache.v_scale.fill_(float("nan"))
    got = teacher_forced(m64, tokens, lens, cache)
    assert sorted((b, t) for b, t, _ in got) == sorted((b, t) for b in range(B) for t in range(lens[b] - 1, S))
    assert cache.lens.tolist() == [n + S - min(lens) for n in lens] and cache.bound == max(lens) + S - min(lens)
    e_q = max((lg - ref[b, t]).abs().max().item() for b, t, lg in got)
    top = ref.abs().max().item()
    print(f"float64 model through an FP8 cache: e_q {e_q:.3e} at max|logits| {top:.3e}")
    assert 0 < e_q < 0.25 * top
    # the cache holds the oracle's bytes of what the model wrote (prefill through kv_cache_append)
    assert not torch.isnan(cache.k_scale[:, 0, :lens[0]]).any() and torch.isnan(cache.k_scale[:, 0, -1]).all()


def test_generate_fp8_cpu():
    m = _tiny(seed=6)
    tokens = torch.randint(1, m.cfg.vocab_size, (2, 6), generator=torch.Generator().manual_seed(9))
    for kv in ("fp8", FP8):
        out = m.generate(tokens, 5, kv_dtype=kv)
        with torch.no_grad():
            first = m(tokens)[:, -1].argmax(-1)  # the first token comes from the prefill, which reads no cache
        assert out.dtype == torch.int64 and out.shape == (2, 5) and torch.equal(out[:, 0], first)
        assert int(out.min()) >= 0 and int(out.max()) < m.cfg.vocab_size
    assert torch.equal(m.generate(tokens, 5, kv_dtype=None), m.generate(tokens, 5))
    assert torch.equal(m.generate(tokens, 5, kv_dtype=torch.float32), m.generate(tokens, 5))
    with pytest.raises(ValueError, match="kv_dtype"):
        m.generate(tokens, 5, kv_dtype="int4")
