"""The FP8 weight-only GEMM for M > 64 (csrc/kernels/linear_fp8_gemm.hip) through ``linear_fp8``: against float64,
bit-exact one-hot rows, rows whose bits do not depend on the call they arrive in, strided operands, and a
llama-tiny prefill (MI355X only). Both slow paths raise, so every case needs the kernel."""
import copy

import pytest
import torch

from decode_oracle import teacher_forced
from test_linear_fp8_gpu import BF16, _check_float64, _check_one_hot, _lf, _tiny, _weights, dev, no_ref  # noqa: F401

pytestmark = pytest.mark.gpu

# a lone partial row tile, a row tile with one live row (129, 257), N below one MFMA tile, N straddling a workgroup
# tile (136, 272), one K-tile, an odd number of K-tiles (5), slabs that do not divide the K-tiles (16 into 3)
SHAPES = [(8, 64), (24, 64), (136, 128), (272, 320), (48, 1024)]


def _x(M, K, dev, seed):
    return torch.randn(M, K, generator=torch.Generator().manual_seed(seed)).to(BF16).to(dev)


def _bits(t):
    return t.view(torch.int16)


@pytest.mark.parametrize("slabs", [None, 1, 3])
@pytest.mark.parametrize("N,K", SHAPES)
@pytest.mark.parametrize("M", [65, 128, 129, 200, 257])
def test_against_float64(dev, no_ref, M, N, K, slabs):
    codes, scale = _weights(N, K, dev)
    x = _x(M, K, dev, M)
    assert _lf().linear_fp8_gemm_ok(x, codes, scale)
    _check_float64(x, codes, scale, _lf().linear_fp8(x, codes, scale, slabs=slabs))


@pytest.mark.parametrize("slabs", [None, 2])
@pytest.mark.parametrize("K", [320, 1024])
def test_one_hot_rows_are_exact(dev, no_ref, K, slabs):
    """80 rows, each 2^a at one k: pins the K map of both fragments, both LDS buffers, the swizzles and the
    channel <-> scale pairing, in the first and the last K-tile of a slab"""
    codes, scale = _weights(136, K, dev, seed=1)
    ks = [0, 7, 8, 15, 16, 31, 32, 63, 64, 65, 127, 128, 191, 192, K - 9, K - 1] * 5
    _check_one_hot(codes, scale, ks, slabs=slabs)


@pytest.mark.parametrize("slabs", [1, 2])
def test_rows_do_not_depend_on_the_call(dev, no_ref, slabs):
    """for a fixed slab count a row has the same bits in a call of 70 rows and of 300, first or last in it, and
    from operands with padded rows"""
    lf, (N, K) = _lf(), (136, 320)
    codes, scale = _weights(N, K, dev, seed=2)
    x = _x(300, K, dev, 7)
    y = lf.linear_fp8(x, codes, scale, slabs=slabs)
    assert torch.equal(_bits(lf.linear_fp8(x[:70], codes, scale, slabs=slabs)), _bits(y[:70]))
    assert torch.equal(_bits(lf.linear_fp8(x[230:], codes, scale, slabs=slabs)), _bits(y[230:]))
    assert torch.equal(_bits(lf.linear_fp8(x, codes, scale, slabs=slabs)), _bits(y))  # and from run to run
    xw = torch.full((300, K + 8), float("nan"), dtype=BF16, device=dev)
    cw = torch.full((N, K + 16), 0x7F, dtype=torch.uint8, device=dev).view(codes.dtype)  # NaN codes in the padding
    xw[:, :K], cw[:, :K] = x, codes
    xv, cv = xw[:, :K], cw[:, :K]
    assert xv.stride(0) == K + 8 and cv.stride(0) == K + 16 and lf.linear_fp8_gemm_ok(xv, cv, scale)
    assert torch.equal(_bits(lf.linear_fp8(xv, cv, scale, slabs=slabs)), _bits(y))


@pytest.mark.parametrize("fused", [False, True], ids=["plain", "fused"])
def test_model_prefill(dev, monkeypatch, fused):
    """llama-tiny with FP8 weights under bf16 autocast: a prefill of 3 x 40 = 120 rows runs the GEMM (both slow
    paths raise), the head and the decode steps the skinny kernel; the logits against the same quantised model with
    every projection on linear_fp8_ref. Yardstick of test_linear_fp8_gpu.test_model_teacher_forced:
    2 * e_full + 2^-8 * top. Measured figures are in docs/linear_fp8.md."""
    from cs744_pytorch_distributed_tutorial_amd.ops import attention as att
    lf = _lf()
    m = _tiny(torch.device("cpu"))
    m64 = copy.deepcopy(m).double()  # stays on the host
    m = m.to(dev)
    Bm, S, lens = 3, 44, (40, 40, 40)
    tokens = torch.randint(1, m.cfg.vocab_size, (Bm, S), generator=torch.Generator().manual_seed(4))
    with torch.no_grad():
        ref64 = m64(tokens)
        with torch.autocast("cuda", dtype=BF16):
            full = m(tokens.to(dev)).double().cpu()
    m.quantize_weights_()
    kernel = lf.linear_fp8
    with torch.autocast("cuda", dtype=BF16):
        monkeypatch.setattr(lf, "linear_fp8", lambda x, c, s, splits=None, slabs=None: lf.linear_fp8_ref(x, c, s))
        want = teacher_forced(m, tokens.to(dev), lens, att.KVCache.allocate(m.cfg, Bm, S, dev))
        monkeypatch.setattr(lf, "linear_fp8", kernel)
        monkeypatch.setattr(lf, "linear_fp8_ref", None)
        monkeypatch.setattr(lf, "_dequant_mm", None)
        for blk in m.layers:
            blk.attention.fused_fp8 = blk.feed_forward.fused_fp8 = fused
        got = teacher_forced(m, tokens.to(dev), lens, att.KVCache.allocate(m.cfg, Bm, S, dev))
    assert [(b, t) for b, t, _ in got] == [(b, t) for b, t, _ in want]
    err = max((a.double() - b.double()).abs().max().item() for (_, _, a), (_, _, b) in zip(got, want))
    e_full = max((full[b, t] - ref64[b, t]).abs().max().item() for b, t, _ in got)
    top = ref64.abs().max().item()
    print(f"FP8 weights, GEMM prefill vs reference: {err:.3e}; bf16 model vs float64: {e_full:.3e}; max|logits| {top:.3e}")
    assert err <= 2 * e_full + 2.0 ** -8 * top
