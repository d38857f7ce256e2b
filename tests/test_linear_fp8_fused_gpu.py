"""The fused FP8 decode projections (csrc/kernels/linear_fp8.hip): the grouped launch and the paired SwiGLU launch,
bit for bit against the separate linear_fp8 calls at the same slab count, against float64, and in llama-tiny
(MI355X only)."""
import functools

import pytest
import torch

from decode_oracle import teacher_forced

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16


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


@pytest.fixture(autouse=True)
def no_composition(monkeypatch):
    """the fused kernels must run: falling back to the separate calls raises"""
    def boom(*a, **kw):
        raise AssertionError("the fused FP8 projection fell back to the composition")
    monkeypatch.setattr(_lf(), "_grouped_composition", boom)
    monkeypatch.setattr(_lf(), "_swiglu_composition", boom)


@functools.lru_cache(maxsize=None)
def _weights(N, K, seed):
    """the recipe of test_linear_fp8_gpu.py: rows of magnitude 2^-12 .. 2^4 with subnormal and +-0 codes; one seed per
    segment, so a wrong segment <-> scale or gate <-> up pairing shows"""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(N, K, generator=g) * torch.exp2(torch.linspace(-12, 4, N)).unsqueeze(1)
    w[:, 1::5] *= 2.0 ** -14
    w[:, 2::7] *= 2.0 ** -22
    codes, scale = _lf().quantize_weight_fp8(w)
    return codes.cuda(), scale.cuda()


@functools.lru_cache(maxsize=None)
def _x(M, K):
    return torch.randn(M, K, generator=torch.Generator().manual_seed(M)).to(BF16).cuda()


def _bits(t):
    return t.view(torch.int16)


def _linear64(x, codes, scale):
    """the float64 product and the bound test_linear_fp8_gpu.py uses: 2^-8 |ref| + K 2^-23 (|x| @ |w|^T)"""
    w = codes.double() * scale.double()[:, None]
    ref = x.double() @ w.T
    return ref, 2.0 ** -8 * ref.abs() + x.shape[1] * 2.0 ** -23 * (x.double().abs() @ w.abs().T)


def _check_grouped(x, ws, ys, slabs):
    assert len(ys) == len(ws)
    for i, ((codes, scale), y) in enumerate(zip(ws, ys)):
        assert y.shape == (x.shape[0], codes.shape[0]) and y.dtype == BF16
        assert torch.equal(_bits(y), _bits(_lf().linear_fp8(x, codes, scale, slabs=slabs))), f"segment {i}"
        ref, bound = _linear64(x, codes, scale)
        assert ((y.double() - ref).abs() <= bound).all(), f"segment {i}"


def _check_swiglu(x, gate, up, y, slabs):
    from cs744_pytorch_distributed_tutorial_amd.ops import lm
    lf = _lf()
    assert y.shape == (x.shape[0], gate[0].shape[0]) and y.dtype == BF16
    assert torch.equal(_bits(y), _bits(lm.swiglu(lf.linear_fp8(x, *gate, slabs=slabs), lf.linear_fp8(x, *up, slabs=slabs))))
    (g, e_g), (u, e_u) = _linear64(x, *gate), _linear64(x, *up)
    silu = g * torch.sigmoid(g)
    # |silu'| <= 1.1; the last term covers the output rounding and the fast exponential
    bound = 1.1 * e_g * (u.abs() + e_u) + silu.abs() * e_u + 2.0 ** -7 * (silu * u).abs()
    err = (y.double() - silu * u).abs()
    print(f"M {x.shape[0]} N {y.shape[1]} K {x.shape[1]}: max error {err.max().item():.3e}, "
          f"max (error - bound) {(err - bound).max().item():.3e}")
    assert (err <= bound).all()


@pytest.mark.parametrize("splits", [None, 1])
@pytest.mark.parametrize("slabs", [1, 2])
@pytest.mark.parametrize("M", [1, 17, 64])
@pytest.mark.parametrize("K", [128, 1024])
@pytest.mark.parametrize("Ns", [(48,), (48, 16), (48, 16, 24), (272, 8, 40)])
def test_grouped(dev, Ns, K, M, slabs, splits):
    ws = [_weights(N, K, 10 + i) for i, N in enumerate(Ns)]
    _check_grouped(_x(M, K), ws, _lf().linear_fp8_grouped(_x(M, K), ws, splits, slabs), slabs)


@pytest.mark.parametrize("M", [1, 17, 33, 64])
@pytest.mark.parametrize("K,slabs", [(64, 1), (1024, 1), (1024, 2)])  # 2 slabs need K >= 256
@pytest.mark.parametrize("N", [16, 24, 272])
def test_swiglu(dev, N, K, slabs, M):
    gate, up = _weights(N, K, 20), _weights(N, K, 21)
    _check_swiglu(_x(M, K), gate, up, _lf().swiglu_linear_fp8(_x(M, K), *gate, *up, slabs=slabs), slabs)


def test_same_bits_for_every_split(dev):
    lf = _lf()
    M, K, Ns = 33, 1024, (48, 16, 24)
    assert lf.linear_fp8_grouped_splits(M, Ns, K) > 1 and lf.swiglu_linear_fp8_splits(M, 48, K) > 1
    x, ws = _x(M, K), [_weights(N, K, 10 + i) for i, N in enumerate(Ns)]
    gate, up = _weights(48, K, 20), _weights(48, K, 21)
    first = lf.linear_fp8_grouped(x, ws), lf.swiglu_linear_fp8(x, *gate, *up)
    for s in (1, 2, 3, 5):
        ys = lf.linear_fp8_grouped(x, ws, s)
        assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(ys, first[0]))
        assert torch.equal(_bits(lf.swiglu_linear_fp8(x, *gate, *up, splits=s)), _bits(first[1]))
    _check_grouped(x, ws, first[0], lf.linear_fp8_grouped_splits(M, Ns, K))
    _check_swiglu(x, gate, up, first[1], lf.swiglu_linear_fp8_splits(M, 48, K))


def test_long_slabs(dev):
    """19 chunks in two slabs (10 + 9): a wave makes a second trip of its two-chunk loop and ends on an odd chunk"""
    lf, K = _lf(), 1216
    ws = [_weights(N, K, 10 + i) for i, N in enumerate((48, 16, 24))]
    _check_grouped(_x(64, K), ws, lf.linear_fp8_grouped(_x(64, K), ws, slabs=2), 2)
    gate, up = _weights(24, K, 20), _weights(24, K, 21)
    _check_swiglu(_x(17, K), gate, up, lf.swiglu_linear_fp8(_x(17, K), *gate, *up, slabs=2), 2)


def _tiny(dev):
    from cs744_pytorch_distributed_tutorial_amd.models import llama
    torch.manual_seed(11)
    return llama.build("llama-tiny").eval().to(dev)


def test_model_teacher_forced(dev):
    """llama-tiny under bf16 autocast, teacher-forced decode_step logits: quantize_weights_(fused=True) against
    quantize_weights_() on the same weights. The two differ as two slab counts differ (the grouped launch picks its
    count from the summed tiles), so the yardstick is test_linear_fp8_gpu.py::test_model_teacher_forced's:
    2 * e_full + 2^-8 * top. Measured figures are in docs/linear_fp8.md."""
    import copy
    from cs744_pytorch_distributed_tutorial_amd.ops import attention as att
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
    with torch.autocast("cuda", dtype=BF16):
        want = teacher_forced(m.quantize_weights_(), tokens.to(dev), lens, att.KVCache.allocate(m.cfg, Bm, n, dev))
        got = teacher_forced(m.quantize_weights_(fused=True), tokens.to(dev), lens,
                             att.KVCache.allocate(m.cfg, Bm, n, dev))
    assert [(b, t) for b, t, _ in got] == [(b, t) for b, t, _ in want]
    err = max((a.double() - b.double()).abs().max().item() for (_, _, a), (_, _, b) in zip(got, want))
    e_full = max((full[b, t] - ref64[b, t]).abs().max().item() for b, t, _ in got)
    top = ref64.abs().max().item()
    print(f"FP8 weights, fused vs separate launches: {err:.3e}; bf16 model vs float64: {e_full:.3e}; "
          f"max|logits| {top:.3e}")
    assert err <= 2 * e_full + 2.0 ** -8 * top


@pytest.mark.parametrize("paged", [False, True], ids=["slab", "paged"])
def test_model_generate(dev, paged):
    """greedy generate with the fused flag: the prefill (27 rows) and every decode step run the fused kernels"""
    m = _tiny(dev).quantize_weights_(fused=True)
    tokens = torch.randint(1, m.cfg.vocab_size, (3, 9), generator=torch.Generator().manual_seed(12)).to(dev)
    with torch.autocast("cuda", dtype=BF16):
        out = m.generate(tokens, 8, page_size=64 if paged else None)
    assert out.shape == (3, 8) and int(out.min()) >= 0 and int(out.max()) < m.cfg.vocab_size
