"""The MXFP4 weight-only GEMM for M > 64 (csrc/kernels/linear_mxfp4_gemm.hip) through ``linear_mxfp4``: against
float64, bit-exact one-hot rows, rows whose bits do not depend on the call they arrive in, strided operands inside
poisoned parents, and a llama-tiny prefill (MI355X only). Both slow paths raise, so every case needs the kernel."""
import copy

import pytest
import torch

from decode_oracle import teacher_forced
from test_linear_mxfp4_gpu import BF16, _check_float64, _check_one_hot, _lx, _tiny, _weights, dev, no_ref  # noqa: F401

pytestmark = pytest.mark.gpu

# a lone partial row tile, a row tile with one live row (129, 257), N below one MFMA tile, N straddling a workgroup
# tile (136, 272), one chunk, an odd chunk count (5), slabs that do not divide the chunks (3 into 5 and into 8)
SHAPES = [(8, 128), (24, 128), (136, 256), (272, 640), (48, 1024)]


def _x(M, K, dev, seed):
    return torch.randn(M, K, generator=torch.Generator().manual_seed(seed)).to(BF16).to(dev)


def _bits(t):
    return t.view(torch.int16)


@pytest.mark.parametrize("slabs", [None, 1, 3])
@pytest.mark.parametrize("N,K", SHAPES)
@pytest.mark.parametrize("M", [65, 128, 129, 200, 257])
def test_against_float64(dev, no_ref, M, N, K, slabs):
    codes, scales = _weights(N, K, dev)
    x = _x(M, K, dev, M)
    assert _lx().linear_mxfp4_gemm_ok(x, codes, scales)
    _check_float64(x, codes, scales, _lx().linear_mxfp4(x, codes, scales, slabs=slabs))


@pytest.mark.parametrize("slabs", [None, 2])
@pytest.mark.parametrize("K", [640, 1024])
def test_one_hot_rows_are_exact(dev, no_ref, K, slabs):
    """80 rows, each 2^a at one k: pins the nibble order, the K map of both K-steps and all lane groups, the scale
    byte for both halves of both K-tiles of a chunk, both buffers and the swizzles"""
    codes, scales = _weights(136, K, dev, seed=1)
    ks = [0, 7, 8, 15, 16, 31, 32, 47, 48, 63, 64, 95, 96, 127, K - 33, K - 1] * 5
    _check_one_hot(codes, scales, ks, slabs=slabs)


@pytest.mark.parametrize("slabs", [1, 2])
def test_rows_do_not_depend_on_the_call(dev, no_ref, slabs):
    """for a fixed slab count a row has the same bits in a call of 70 rows and of 300, first or last in it, and
    from operands that are views inside poisoned parents"""
    lx, (N, K) = _lx(), (136, 640)
    codes, scales = _weights(N, K, dev, seed=2)
    x = _x(300, K, dev, 7)
    y = lx.linear_mxfp4(x, codes, scales, slabs=slabs)
    assert torch.equal(_bits(lx.linear_mxfp4(x[:70], codes, scales, slabs=slabs)), _bits(y[:70]))
    assert torch.equal(_bits(lx.linear_mxfp4(x[230:], codes, scales, slabs=slabs)), _bits(y[230:]))
    assert torch.equal(_bits(lx.linear_mxfp4(x, codes, scales, slabs=slabs)), _bits(y))  # and from run to run
    xw = torch.full((300, K + 8), float("nan"), dtype=BF16, device=dev)
    cw = torch.full((N, K // 2 + 16), 0xFF, dtype=torch.uint8, device=dev)
    sw = torch.full((N, K // 32 + 4), 0xFF, dtype=torch.uint8, device=dev)
    xw[:, :K], cw[:, :K // 2], sw[:, :K // 32] = x, codes, scales
    xv, cv, sv = xw[:, :K], cw[:, :K // 2], sw[:, :K // 32]
    assert (xv.stride(0), cv.stride(0), sv.stride(0)) == (K + 8, K // 2 + 16, K // 32 + 4)
    assert lx.linear_mxfp4_gemm_ok(xv, cv, sv)
    assert torch.equal(_bits(lx.linear_mxfp4(xv, cv, sv, slabs=slabs)), _bits(y))


@pytest.mark.parametrize("fused", [False, True], ids=["plain", "fused"])
def test_model_prefill(dev, monkeypatch, fused):
    """llama-tiny with MXFP4 weights under bf16 autocast: a prefill of 3 x 40 = 120 rows runs the GEMM (both slow
    paths are None), the head and the decode steps the skinny kernel; the logits against the same quantised model
    with every projection on linear_mxfp4_ref. Yardstick of test_linear_fp8_gemm_gpu.test_model_prefill:
    2 * e_full + 2^-8 * top."""
    from cs744_pytorch_distributed_tutorial_amd.ops import attention as att
    lx = _lx()
    m = _tiny(torch.device("cpu"))
    m64 = copy.deepcopy(m).double()  # stays on the host
    m = m.to(dev)
    Bm, S, lens = 3, 44, (40, 40, 40)
    tokens = torch.randint(1, m.cfg.vocab_size, (Bm, S), generator=torch.Generator().manual_seed(4))
    with torch.no_grad():
        ref64 = m64(tokens)
        with torch.autocast("cuda", dtype=BF16):
            full = m(tokens.to(dev)).double().cpu()
    m.quantize_weights_(dtype="mxfp4")
    kernel = lx.linear_mxfp4
    with torch.autocast("cuda", dtype=BF16):
        monkeypatch.setattr(lx, "linear_mxfp4", lambda x, c, s, splits=None, slabs=None: lx.linear_mxfp4_ref(x, c, s))
        want = teacher_forced(m, tokens.to(dev), lens, att.KVCache.allocate(m.cfg, Bm, S, dev))
        monkeypatch.setattr(lx, "linear_mxfp4", kernel)
        monkeypatch.setattr(lx, "linear_mxfp4_ref", None)
        monkeypatch.setattr(lx, "_dequant_mm", None)
        for blk in m.layers:
            blk.attention.fused_fp8 = blk.feed_forward.fused_fp8 = fused
        got = teacher_forced(m, tokens.to(dev), lens, att.KVCache.allocate(m.cfg, Bm, S, dev))
    assert [(b, t) for b, t, _ in got] == [(b, t) for b, t, _ in want]
    err = max((a.double() - b.double()).abs().max().item() for (_, _, a), (_, _, b) in zip(got, want))
    e_full = max((full[b, t] - ref64[b, t]).abs().max().item() for b, t, _ in got)
    top = ref64.abs().max().item()
    print(f"MXFP4 weights, GEMM prefill vs reference: {err:.3e}; bf16 model vs float64: {e_full:.3e}; max|logits| {top:.3e}")
    assert err <= 2 * e_full + 2.0 ** -8 * top
