"""The MXFP4 weight-only linear kernel (csrc/kernels/linear_mxfp4.hip) against float64, bit-exact one-hot rows, the
same bits for every split, the grouped and paired entries against the composition, dispatch, and llama-tiny with
MXFP4 weights (MI355X only)."""
import pytest
import torch

from decode_oracle import teacher_forced

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
SHAPES = [(16, 128), (24, 128), (8, 256), (272, 384), (48, 1024)]
# slabs of 9 and more chunks of 128: a wave takes chunks w, w + 4, ..., two per trip of its loop, so with 9 to 15
# chunks it makes a second trip and some wave ends on an odd chunk. (M, N, K, slabs): 16 chunks in one slab (two
# full trips), 13 in one (waves 1 to 3 end odd), 19 in two (10 + 9)
LONG = [(1, 48, 2048, 1), (17, 272, 1664, 1), (64, 24, 2432, 2)]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cs744_pytorch_distributed_tutorial_amd.ops import native
    native.C()
    return torch.device("cuda", 0)


def _lx():
    from cs744_pytorch_distributed_tutorial_amd.ops import linear_mxfp4
    return linear_mxfp4


@pytest.fixture
def no_ref(monkeypatch):
    """the kernel must run: the reference and the dequantise-and-mm path raise"""
    def boom(*a, **kw):
        raise AssertionError("linear_mxfp4 left the kernel")
    monkeypatch.setattr(_lx(), "linear_mxfp4_ref", boom)
    monkeypatch.setattr(_lx(), "_dequant_mm", boom)
    return monkeypatch


def _weights(N, K, dev, seed=0):
    """blocks of magnitude 2^-10 .. 2^6 (the scales differ inside a row), one all-zero block per row, and some
    elements small enough for the zero codes of both signs"""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(N, K // 32, 32, generator=g) * torch.exp2(torch.randint(-10, 7, (N, K // 32, 1), generator=g).float())
    w[torch.arange(N), torch.arange(N) % (K // 32)] = 0.0
    w = w.view(N, K)
    w[:, 2::7] *= 2.0 ** -10
    codes, scales = _lx().quantize_weight_mxfp4(w)
    assert torch.cat((codes & 15, codes >> 4)).unique().numel() == 16 and scales.unique().numel() >= 2
    return codes.to(dev), scales.to(dev)


def _x(M, K, dev):
    return torch.randn(M, K, generator=torch.Generator().manual_seed(M)).to(BF16).to(dev)


def _check_float64(x, codes, scales, y):
    """|y - ref| <= 2^-8 |ref| + K 2^-23 (|x| @ |W|^T): products of two bf16 numbers are exact in fp32, so this
    covers the fp32 sum in any order plus the bf16 rounding of the output."""
    K = x.shape[1]
    assert y.shape == (x.shape[0], codes.shape[0]) and y.dtype == BF16
    w = _lx().dequantize_mxfp4(codes, scales, torch.float64)
    ref = x.double() @ w.T
    bound = 2.0 ** -8 * ref.abs() + K * 2.0 ** -23 * (x.double().abs() @ w.abs().T)
    err = (y.double() - ref).abs()
    print(f"M {x.shape[0]} N {codes.shape[0]} K {K}: max error {err.max().item():.3e}, "
          f"max (error - bound) {(err - bound).max().item():.3e}")
    assert (err <= bound).all()


def _check_one_hot(codes, scales, ks, **kw):
    """x row i is 2^a at k = ks[i]: y[i] must be column k of the dequantised weight times 2^a, bit for bit, zeros as
    +0. Pins the nibble order, the k of every MFMA K-step and lane group, and the block <-> scale pairing."""
    lx, dev = _lx(), codes.device
    x = torch.zeros(len(ks), codes.shape[1] * 2, dtype=BF16, device=dev)
    amp = torch.exp2(torch.arange(len(ks), device=dev) % 8 - 3.0)
    x[torch.arange(len(ks)), ks] = amp.to(BF16)
    want = (lx.dequantize_mxfp4(codes, scales, torch.float32)[:, ks] * amp).T.to(BF16) + 0.0
    y = lx.linear_mxfp4(x, codes, scales, **kw)
    assert not (y == 0).logical_and(y.view(torch.int16) != 0).any()  # the kernel's zeros are +0
    assert torch.equal(y.view(torch.int16), want.view(torch.int16))


@pytest.mark.parametrize("splits", [None, 1, 3])
@pytest.mark.parametrize("N,K", SHAPES)
@pytest.mark.parametrize("M", [1, 3, 16, 17, 33, 64])
def test_against_float64(dev, no_ref, M, N, K, splits):
    codes, scales = _weights(N, K, dev)
    x = _x(M, K, dev)
    _check_float64(x, codes, scales, _lx().linear_mxfp4(x, codes, scales, splits))


@pytest.mark.parametrize("N,K", SHAPES)
def test_one_hot_rows_are_exact(dev, no_ref, N, K):
    codes, scales = _weights(N, K, dev, seed=1)
    ks = sorted({k for k in (0, 1, 7, 8, 15, 16, 31, 32, 33, 63, 64, 127, 128, K - 1) if k < K})
    for splits in (None, 2):
        _check_one_hot(codes, scales, ks, splits=splits)


@pytest.mark.parametrize("M,N,K,slabs", LONG)
def test_long_slabs(dev, no_ref, M, N, K, slabs):
    """the steady state of the K loop: both checks above where a wave holds 3 to 4 chunks of a slab"""
    codes, scales = _weights(N, K, dev, seed=3)
    x = _x(M, K, dev)
    _check_float64(x, codes, scales, _lx().linear_mxfp4(x, codes, scales, slabs=slabs))
    ks = [0, 127, 128, 511, 512, 513, 600, 1023, 1024, 1039, 1151, 1152, 1280, 1535, 1536, 1663, K - 33, K - 1]
    _check_one_hot(codes, scales, ks, slabs=slabs)


def test_same_bits_for_every_split(dev, no_ref):
    lx = _lx()
    M, N, K = 33, 48, 1024
    assert lx.linear_mxfp4_splits(M, N, K) > 1  # the slabs are shared by 1, 2, 3 and 5 (clamped) workgroups below
    codes, scales = _weights(N, K, dev, seed=2)
    x = _x(M, K, dev)
    ys = [lx.linear_mxfp4(x, codes, scales, s) for s in (None, 1, 2, 3, 5, 1, 5)]
    assert all(torch.equal(y.view(torch.int16), ys[0].view(torch.int16)) for y in ys)


@pytest.mark.parametrize("slabs", [1, None])
@pytest.mark.parametrize("M", [1, 17])
def test_grouped_has_the_bits_of_the_separate_calls(dev, no_ref, M, slabs):
    lx = _lx()
    Ns, K = (64, 16, 16), 1024
    ws = [_weights(N, K, dev, seed=4 + i) for i, N in enumerate(Ns)]
    x = _x(M, K, dev)
    n = slabs or lx.linear_mxfp4_grouped_splits(M, Ns, K)
    assert slabs == 1 or n > 1
    ys = lx.linear_mxfp4_grouped(x, ws, slabs=slabs)
    for (c, s), y in zip(ws, ys):
        assert torch.equal(y.view(torch.int16), lx.linear_mxfp4(x, c, s, slabs=n).view(torch.int16))
        _check_float64(x, c, s, y)


@pytest.mark.parametrize("N,K", [(24, 256), (24, 1024)])  # one slab only, and a K the default splits: the combine
@pytest.mark.parametrize("M", [1, 17])
def test_swiglu_has_the_bits_of_the_composition(dev, no_ref, M, N, K):
    from cs744_pytorch_distributed_tutorial_amd.ops import lm
    lx = _lx()
    (gc, gs), (uc, us) = _weights(N, K, dev, seed=7), _weights(N, K, dev, seed=8)
    x = _x(M, K, dev)
    n = lx.swiglu_linear_mxfp4_splits(M, N, K)
    assert (n > 1) == (K == 1024)
    g, u = lx.linear_mxfp4(x, gc, gs, slabs=n), lx.linear_mxfp4(x, uc, us, slabs=n)
    _check_float64(x, gc, gs, g)
    y = lx.swiglu_linear_mxfp4(x, gc, gs, uc, us)
    assert torch.equal(y.view(torch.int16), lm.swiglu(g, u).view(torch.int16))
    assert torch.equal(y, lx.swiglu_linear_mxfp4(x, gc, gs, uc, us, splits=2, slabs=n))


def test_dispatch(dev, monkeypatch):
    lx = _lx()
    codes, scales = _weights(48, 256, dev)
    g = torch.Generator().manual_seed(9)
    wide = torch.randn(8, 264, generator=g).to(BF16).to(dev)
    c96, s96 = _weights(48, 96, dev)
    slow = [(torch.randn(65, 256, generator=g).to(BF16).to(dev), codes, scales),   # M past the kernel
            (torch.randn(4, 96, generator=g).to(BF16).to(dev), c96, s96),         # K % 128 != 0
            (torch.randn(4, 256, generator=g).to(dev), codes, scales),            # fp32 x
            (wide[:, 4:260], codes, scales)]                                      # rows off 16 bytes
    for x, c, s in slow:
        assert not lx.linear_mxfp4_native_ok(x, c, s)
        y, ref = lx.linear_mxfp4(x, c, s), lx.linear_mxfp4_ref(x, c, s)
        tol = 2.0 ** -7 * ref.abs().max().item() if x.dtype == BF16 else 1e-5 * ref.abs().max().item()
        assert y.dtype == x.dtype and (y.float() - ref.float()).abs().max().item() <= tol
    assert lx.linear_mxfp4_native_ok(wide[:, :256], codes, scales)  # a row stride of K + 8 is fine
    monkeypatch.setattr(lx, "_dequant_mm", None)
    monkeypatch.setattr(lx, "linear_mxfp4_ref", None)
    assert torch.equal(lx.linear_mxfp4(wide[:, :256], codes, scales), lx.linear_mxfp4(wide[:, :256].contiguous(), codes, scales))
    assert lx.linear_mxfp4(torch.empty(0, 256, dtype=BF16, device=dev), codes, scales).shape == (0, 48)
    assert lx.linear_mxfp4(torch.empty(2, 0, 256, dtype=BF16, device=dev), codes, scales).shape == (2, 0, 48)
    with pytest.raises(RuntimeError, match="inference only"):
        lx.linear_mxfp4(wide[:, :256].clone().requires_grad_(), codes, scales)


def _tiny(dev):
    from cs744_pytorch_distributed_tutorial_amd.models import llama
    torch.manual_seed(11)
    return llama.build("llama-tiny").eval().to(dev)


@pytest.mark.parametrize("fused", [False, True], ids=["plain", "fused"])
def test_model_teacher_forced(dev, monkeypatch, fused):
    """llama-tiny with MXFP4 weights under bf16 autocast: teacher-forced decode_step logits through the kernel
    against the same quantised model with every Mxfp4Linear on linear_mxfp4_ref. The two differ in the order of the
    fp32 sums only, so the yardstick is tests/test_linear_fp8_gpu.py's: 2 * e_full + 2^-8 * top, e_full the gap
    between the un-quantised bf16 model and its float64 copy on the same tokens."""
    import copy
    from cs744_pytorch_distributed_tutorial_amd.ops import attention as att
    lx = _lx()
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
    m.quantize_weights_(dtype="mxfp4")
    kernel = lx.linear_mxfp4
    with torch.autocast("cuda", dtype=BF16):
        monkeypatch.setattr(lx, "linear_mxfp4", lambda x, c, s, splits=None, slabs=None: lx.linear_mxfp4_ref(x, c, s))
        want = teacher_forced(m, tokens.to(dev), lens, att.KVCache.allocate(m.cfg, Bm, n, dev))
        monkeypatch.setattr(lx, "linear_mxfp4", kernel)
        monkeypatch.setattr(lx, "linear_mxfp4_ref", None)  # the prefill (22 rows) and the decode steps run the kernel
        monkeypatch.setattr(lx, "_dequant_mm", None)
        m.quantize_weights_(dtype="mxfp4", fused=fused)
        got = teacher_forced(m, tokens.to(dev), lens, att.KVCache.allocate(m.cfg, Bm, n, dev))
    assert [(b, t) for b, t, _ in got] == [(b, t) for b, t, _ in want]
    err = max((a.double() - b.double()).abs().max().item() for (_, _, a), (_, _, b) in zip(got, want))
    e_full = max((full[b, t] - ref64[b, t]).abs().max().item() for b, t, _ in got)
    top = ref64.abs().max().item()
    print(f"MXFP4 weights, kernel vs reference: {err:.3e}; bf16 model vs float64: {e_full:.3e}; max|logits| {top:.3e}")
    assert err <= 2 * e_full + 2.0 ** -8 * top


@pytest.mark.parametrize("paged", [False, True], ids=["slab", "paged"])
@pytest.mark.parametrize("fused", [False, True], ids=["plain", "fused"])
def test_model_generate(dev, no_ref, fused, paged):
    """greedy generate with MXFP4 weights: the prefill (27 rows) and every decode step run the kernel, since both
    slow paths raise"""
    m = _tiny(dev).quantize_weights_(dtype="mxfp4", fused=fused)
    tokens = torch.randint(1, m.cfg.vocab_size, (3, 9), generator=torch.Generator().manual_seed(12)).to(dev)
    with torch.autocast("cuda", dtype=BF16):
        out = m.generate(tokens, 8, page_size=64 if paged else None)
    assert out.shape == (3, 8) and int(out.min()) >= 0 and int(out.max()) < m.cfg.vocab_size
