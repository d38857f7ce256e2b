"""The dispatch of the FP8 weight-only GEMM for M > 64 as far as it can be checked without a GPU."""
import pytest
import torch

from cs744_pytorch_distributed_tutorial_amd.ops import linear_fp8 as lf


def _meta(M, K, N=16, ldx=None, ldw=None):
    x = torch.empty_strided((M, K), (ldx or K, 1), dtype=torch.bfloat16, device="meta")
    codes = torch.empty_strided((N, K), (ldw or K, 1), dtype=lf.FP8, device="meta")
    return x, codes, torch.empty(N, device="meta")


# the 32-bit offsets of a tile's buffer descriptor: 128 rows of x (2 bytes an element) and 128 of codes stay below
# 0x7ffffff0, so ldx <= 8388607 elements and ldw <= 16777215 bytes (rounded down to the strides' multiples)
@pytest.mark.parametrize("kw,ok", [(dict(M=65, K=128), True), (dict(M=64, K=128), False), (dict(M=65, K=96), False),
                                   (dict(M=65, K=128, N=12), False), (dict(M=65, K=128, ldx=8388600), True),
                                   (dict(M=65, K=128, ldx=8388608), False), (dict(M=65, K=128, ldw=16777200), True),
                                   (dict(M=65, K=128, ldw=16777216), False), (dict(M=6144, K=128), True),
                                   (dict(M=6145, K=128), False)])
def test_gemm_layout(kw, ok):
    assert lf._gemm_layout_ok(*_meta(**kw)) == ok
    assert not lf.linear_fp8_gemm_ok(*_meta(**kw))  # not on a GPU


def test_linear_fp8_on_the_cpu_at_65_rows_is_the_reference():
    g = torch.Generator().manual_seed(0)
    codes, scale = lf.quantize_weight_fp8(torch.randn(16, 128, generator=g))
    x = torch.randn(65, 128, generator=g).bfloat16()
    assert not lf.linear_fp8_gemm_ok(x, codes, scale)
    assert torch.equal(lf.linear_fp8(x, codes, scale), lf.linear_fp8_ref(x, codes, scale))
