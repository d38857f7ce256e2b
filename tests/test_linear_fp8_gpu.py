"""The FP8 weight-only linear kernel (csrc/kernels/linear_fp8.hip) against float64, bit-exact one-hot rows, the
same bits for every split, dispatch, and llama-tiny with quantised weights (MI355X only)."""
import pytest
import torch

from decode_oracle import teacher_forced

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
SHAPES = [(16, 64), (24, 64), (8, 128), (272, 320), (48, 1024)]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cs744_pytorch_distributed_tutorial_amd.ops import native
    native.C()
    return torch.device("cuda", 0)


def _lf():
    from cs744_pytorch_distributed_tutorial_amd.ops import linear_fp8
    return linear_fp8


@pytest.fixture
def no_ref(monkeypatch):
    """the kernel must run: the reference and the dequantise-and-mm path raise"""
    def boom(*a, **kw):
        raise AssertionError("linear_fp8 left the kernel")
    monkeypatch.setattr(_lf(), "linear_fp8_ref", boom)
    monkeypatch.setattr(_lf(), "_dequant_mm", boom)
    return monkeypatch


def _weights(N, K, dev, seed=0):
    """rows of magnitude 2^-12 .. 2^4, some elements small enough for subnormal and zero codes of both signs"""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(N, K, generator=g) * torch.exp2(torch.linspace(-12, 4, N)).unsqueeze(1)
    w[:, 1::5] *= 2.0 ** -14  # subnormal codes
    w[:, 2::7] *= 2.0 ** -22  # +-0 codes
    codes, scale = _lf().quantize_weight_fp8(w)
    b = codes.view(torch.uint8)
    assert (((b & 0x78) == 0) & ((b & 7) != 0)).any() and (b == 0x80).any() and (b == 0).any()
    assert scale.unique().numel() > 1
    return codes.to(dev), scale.to(dev)


# slabs of 9 and more chunks, as every Llama-3-8B shape has: a wave takes two chunks per trip, makes a second trip
# and ends on an odd chunk. (M, N, K, slabs): 16 chunks in one slab, 13 in one, 19 in two (10 + 9), and a shape whose
# slab count the heuristic itself sets to 1 on 256 CUs (13 chunks)
LONG = [(1, 48, 1024, 1), (17, 272, 832, 1), (64, 24, 1216, 2), (17, 16384, 832, None)]


def _check_float64(x, codes, scale, y):
    """|y - ref| <= 2^-8 |ref| + K 2^-23 (|x| @ |w|): products are exact in fp32, so this is twice the first-order
    bound of a K-term fp32 sum in any order plus the bf16 rounding of the output."""
    K = x.shape[1]
    assert y.shape == (x.shape[0], codes.shape[0]) and y.dtype == BF16
    w = codes.double() * scale.double()[:, None]
    ref = x.double() @ w.T
    bound = 2.0 ** -8 * ref.abs() + K * 2.0 ** -23 * (x.double().abs() @ w.abs().T)
    err = (y.double() - ref).abs()
    print(f"M {x.shape[0]} N {codes.shape[0]} K {K}: max error {err.max().item():.3e}, "
          f"max (error - bound) {(err - bound).max().item():.3e}")
    assert (err <= bound).all()


def _check_one_hot(codes, scale, ks, **kw):
    """x row i is 2^a at k = ks[i]: y[i] must be column k of the dequantised weight times 2^a, bit for bit (a zero
    with the sign of the sum, +0: a -0 code gives +0). Pins the K order of the two MFMA fragments, chunk by chunk,
    and the channel <-> scale pairing."""
    lf, dev = _lf(), codes.device
    x = torch.zeros(len(ks), codes.shape[1], dtype=BF16, device=dev)
    amp = torch.exp2(torch.arange(len(ks), device=dev) % 8 - 3.0)
    x[torch.arange(len(ks)), ks] = amp.to(BF16)
    want = (lf.kv_dequantize(codes, scale, BF16)[:, ks].float() * amp).T.to(BF16) + 0.0
    y = lf.linear_fp8(x, codes, scale, **kw)
    assert not (y == 0).logical_and(y.view(torch.int16) != 0).any()  # the kernel's zeros are +0
    assert torch.equal(y.view(torch.int16), want.view(torch.int16))


@pytest.mark.parametrize("splits", [None, 1, 3])
@pytest.mark.parametrize("N,K", SHAPES)
@pytest.mark.parametrize("M", [1, 3, 16, 17, 33, 64])
def test_against_float64(dev, no_ref, M, N, K, splits):
    codes, scale = _weights(N, K, dev)
    x = torch.randn(M, K, generator=torch.Generator().manual_seed(M)).to(BF16).to(dev)
    _check_float64(x, codes, scale, _lf().linear_fp8(x, codes, scale, splits))


@pytest.mark.parametrize("N,K", SHAPES)
def test_one_hot_rows_are_exact(dev, no_ref, N, K):
    codes, scale = _weights(N, K, dev, seed=1)
    ks = sorted({k for k in (0, 7, 8, 15, 16, 31, 32, 63, 64, K - 1) if k < K})
    for splits in (None, 2):
        _check_one_hot(codes, scale, ks, splits=splits)


@pytest.mark.parametrize("M,N,K,slabs", LONG)
def test_long_slabs(dev, no_ref, M, N, K, slabs):
    """the steady state of the K loop: both checks above where a wave holds 3 to 4 chunks of a slab"""
    chunks = K // 64 // (slabs or _lf().linear_fp8_splits(M, N, K))
    assert chunks >= 9 or torch.cuda.get_device_properties(dev).multi_processor_count != 256
    codes, scale = _weights(N, K, dev, seed=3)
    x = torch.randn(M, K, generator=torch.Generator().manual_seed(M)).to(BF16).to(dev)
    _check_float64(x, codes, scale, _lf().linear_fp8(x, codes, scale, slabs=slabs))
    ks = [0, 63, 64, 255, 256, 257, 300, 511, 512, 519, 575, 576, 640, 767, 768, 831, K - 9, K - 1]
    _check_one_hot(codes, scale, ks, slabs=slabs)


def test_same_bits_for_every_split(dev, no_ref):
    lf = _lf()
    M, N, K = 33, 48, 1024
    assert lf.linear_fp8_splits(M, N, K) > 1  # the slabs are shared by 1, 2, 3 and 5 workgroups below
    codes, scale = _weights(N, K, dev, seed=2)
    x = torch.randn(M, K, generator=torch.Generator().manual_seed(5)).to(BF16).to(dev)
    ys = [lf.linear_fp8(x, codes, scale, s) for s in (None, 1, 2, 3, 5, 1, 5)]
    assert all(torch.equal(y.view(torch.int16), ys[0].view(torch.int16)) for y in ys)


def test_dispatch(dev, monkeypatch):
    lf = _lf()
    codes, scale = _weights(48, 128, dev)
    g = torch.Generator().manual_seed(9)
    wide = torch.randn(8, 136, generator=g).to(BF16).to(dev)
    c96, s96 = _weights(48, 96, dev)
    slow = [(torch.randn(65, 128, generator=g).to(BF16).to(dev), codes, scale),   # M past the kernel
            (torch.randn(4, 96, generator=g).to(BF16).to(dev), c96, s96),        # K % 64 != 0
            (torch.randn(4, 128, generator=g).to(dev), codes, scale),            # fp32 x
            (wide[:, 4:132], codes, scale)]                                      # rows off 16 bytes
    for x, c, s in slow:
        assert not lf.linear_fp8_native_ok(x, c, s)
        y, ref = lf.linear_fp8(x, c, s), lf.linear_fp8_ref(x, c, s)
        tol = 2.0 ** -7 * ref.abs().max().item() if x.dtype == BF16 else 1e-5 * ref.abs().max().item()
        assert y.dtype == x.dtype and (y.float() - ref.float()).abs().max().item() <= tol
    assert lf.linear_fp8_native_ok(wide[:, :128], codes, scale)  # a row stride of 136 is fine
    monkeypatch.setattr(lf, "_dequant_mm", None)
    monkeypatch.setattr(lf, "linear_fp8_ref", None)
    assert torch.equal(lf.linear_fp8(wide[:, :128], codes, scale), lf.linear_fp8(wide[:, :128].contiguous(), codes, scale))
    assert lf.linear_fp8(torch.empty(0, 128, dtype=BF16, device=dev), codes, scale).shape == (0, 48)
    assert lf.linear_fp8(torch.empty(2, 0, 128, dtype=BF16, device=dev), codes, scale).shape == (2, 0, 48)
    with pytest.raises(RuntimeError, match="inference only"):
        lf.linear_fp8(wide[:, :128].clone().requires_grad_(), codes, scale)


def _tiny(dev):
    from cs744_pytorch_distributed_tutorial_amd.models import llama
    torch.manual_seed(11)
    return llama.build("llama-tiny").eval().to(dev)


def test_model_teacher_forced(dev, monkeypatch):
    """llama-tiny with FP8 weights under bf16 autocast: teacher-forced decode_step logits through the kernel
    against the same quantised model with every Fp8Linear on linear_fp8_ref. The two differ in the order of the
    fp32 sums only, so the yardstick is the one tests/test_kv_fp8_gpu.py uses for bf16-level differences of the
    logits: 2 * e_full + 2^-8 * top, e_full the gap between the un-quantised bf16 model and its float64 copy on
    the same tokens. Measured figures are in docs/linear_fp8.md."""
    import copy
    from cs744_pytorch_distributed_tutorial_amd.ops import attention as att
    lf = _lf()
    m = _tiny(torch.device("cpu"))
    m64 = copy.deepcopy(m).double()  # stays on the host
    m = m.to(dev)
    Bm, S, lens = 2, 24, (5, 11)
    n = S + max(lens) - min(lens)
    tokens = torch.randint(1, m.cfg.vocab_size, (Bm, S), generator=torch.Generator().manual_seed(4))
    with torch.no_grad():
        ref64 = m64(tokens)
        with torch.autocast("cuda", dtype=BF16):
            full = m(tokens.to(dev)).double().cpu()
    m.quantize_weights_()
    kernel = lf.linear_fp8
    with torch.autocast("cuda", dtype=BF16):
        monkeypatch.setattr(lf, "linear_fp8", lambda x, c, s, splits=None: lf.linear_fp8_ref(x, c, s))
        want = teacher_forced(m, tokens.to(dev), lens, att.KVCache.allocate(m.cfg, Bm, n, dev))
        monkeypatch.setattr(lf, "linear_fp8", kernel)
        monkeypatch.setattr(lf, "linear_fp8_ref", None)  # the prefill (22 rows) and the decode steps run the kernel
        got = teacher_forced(m, tokens.to(dev), lens, att.KVCache.allocate(m.cfg, Bm, n, dev))
    assert [(b, t) for b, t, _ in got] == [(b, t) for b, t, _ in want]
    err = max((a.double() - b.double()).abs().max().item() for (_, _, a), (_, _, b) in zip(got, want))
    e_full = max((full[b, t] - ref64[b, t]).abs().max().item() for b, t, _ in got)
    top = ref64.abs().max().item()
    print(f"FP8 weights, kernel vs reference: {err:.3e}; bf16 model vs float64: {e_full:.3e}; max|logits| {top:.3e}")
    assert err <= 2 * e_full + 2.0 ** -8 * top


@pytest.mark.parametrize("paged", [False, True], ids=["slab", "paged"])
def test_model_generate(dev, no_ref, paged):
    """greedy generate with FP8 weights: the prefill (27 rows) and every decode step run the kernel, since both
    slow paths raise"""
    m = _tiny(dev).quantize_weights_()
    tokens = torch.randint(1, m.cfg.vocab_size, (3, 9), generator=torch.Generator().manual_seed(12)).to(dev)
    with torch.autocast("cuda", dtype=BF16):
        out = m.generate(tokens, 8, page_size=64 if paged else None)
    assert out.shape == (3, 8) and int(out.min()) >= 0 and int(out.max()) < m.cfg.vocab_size
