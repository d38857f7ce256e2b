"""The dispatch of the MXFP4 weight-only GEMM for M > 64 as far as it can be checked without a GPU."""
import pytest
import torch

from cs744_pytorch_distributed_tutorial_amd.ops import linear_mxfp4 as lx


def _meta(M, K, N=16, ldx=None, ldw=None, lds=None):
    x = torch.empty_strided((M, K), (ldx or K, 1), dtype=torch.bfloat16, device="meta")
    codes = torch.empty_strided((N, K // 2), (ldw or K // 2, 1), dtype=torch.uint8, device="meta")
    return x, codes, torch.empty_strided((N, K // 32), (lds or K // 32, 1), dtype=torch.uint8, device="meta")


# the 32-bit offsets of a tile's buffer descriptor: 128 rows of x (2 bytes an element), of codes and of scales stay
# below 0x7ffffff0, so ldx <= 8388607 elements and ldw, lds <= 16777215 bytes (rounded down to the strides'
# multiples: 8 elements, 16 bytes, 4 bytes). No row cap is set.
@pytest.mark.parametrize("kw,ok", [(dict(M=65, K=128), True), (dict(M=64, K=128), False), (dict(M=65, K=192), False),
                                   (dict(M=65, K=128, N=12), False), (dict(M=65, K=128, lds=6), False),
                                   (dict(M=65, K=128, lds=8), True), (dict(M=65, K=128, ldx=8388600), True),
                                   (dict(M=65, K=128, ldx=8388608), False), (dict(M=65, K=128, ldw=16777200), True),
                                   (dict(M=65, K=128, ldw=16777216), False), (dict(M=65, K=128, lds=16777212), True),
                                   (dict(M=65, K=128, lds=16777216), False), (dict(M=1 << 20, K=128), True)])
def test_gemm_layout(kw, ok):
    assert lx._gemm_layout_ok(*_meta(**kw)) == ok
    assert not lx.linear_mxfp4_gemm_ok(*_meta(**kw))  # not on a GPU


def test_linear_mxfp4_on_the_cpu_at_65_rows_is_the_reference():
    g = torch.Generator().manual_seed(0)
    codes, scales = lx.quantize_weight_mxfp4(torch.randn(16, 128, generator=g))
    x = torch.randn(65, 128, generator=g).bfloat16()
    assert not lx.linear_mxfp4_gemm_ok(x, codes, scales)
    assert torch.equal(lx.linear_mxfp4(x, codes, scales), lx.linear_mxfp4_ref(x, codes, scales))
