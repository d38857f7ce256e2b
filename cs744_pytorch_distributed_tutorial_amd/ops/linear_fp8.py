"""FP8 weight-only projections (W8A16): ``csrc/kernels/linear_fp8.hip`` for decoding (up to 64 rows) and
``csrc/kernels/linear_fp8_gemm.hip`` for prefills and larger batches.

A weight ``[N, K]`` is stored as float8_e4m3fn codes plus one power-of-two fp32 scale per output channel, the
format ``ops.attention.kv_quantize_ref`` defines, applied to the rows of the weight. Every code is exactly a
bf16 number and ``float(code) * scale`` is the weight, so the kernel's only roundings are its fp32 sums and
the bf16 store. At decode batch sizes a projection is bound by its weight bytes, which this halves against
the bf16 shadow. Inference only. ``docs/linear_fp8.md`` has the design and the measurements."""
from __future__ import annotations

from typing import Optional

import torch

from . import native
from .attention import FP8, _no_grad_inputs, kv_dequantize, kv_quantize_ref


def quantize_weight_fp8(w: torch.Tensor) -> tuple:
    """``w`` ``[N, K]`` (fp32, bf16 or fp64, any device) -> ``(codes float8_e4m3fn [N, K], scale fp32 [N])``:
    ``kv_quantize_ref`` on the rows, one scale per output channel."""
    if w.dim() != 2:
        raise ValueError(f"quantize_weight_fp8: the weight must be [N, K], got {tuple(w.shape)}")
    return kv_quantize_ref(w.detach())


def linear_fp8_ref(x: torch.Tensor, codes: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """``x @ (codes * scale[:, None])^T`` in plain torch: fp32 math (fp64 for an fp64 ``x``), the result in
    ``x``'s dtype. ``x`` ``[..., K]``."""
    ct = torch.float64 if x.dtype == torch.float64 else torch.float32
    w = codes.to(ct) * scale.to(ct).unsqueeze(-1)
    return (x.to(ct) @ w.t()).to(x.dtype)


def linear_fp8_max_m() -> int:
    """The most rows of ``x`` the kernel takes."""
    return native.C().linear_fp8_max_m()


def linear_fp8_splits(M: int, N: int, K: int) -> int:
    """The K slabs the kernel splits K into, and sums in order, for these shapes: from M, N, K and the CU count
    only, never from data. (``linear_fp8``'s ``splits`` argument does not change this count: see there.)"""
    return native.C().linear_fp8_splits(M, N, K)


def linear_fp8_native_ok(x2: torch.Tensor, codes: torch.Tensor, scale: torch.Tensor) -> bool:
    """Whether ``linear_fp8_kernel`` takes these operands: everything on one GPU, ``x2`` bf16 ``[M, K]`` with
    unit inner stride and M at most ``linear_fp8_max_m()``, ``codes`` float8_e4m3fn ``[N, K]`` K-contiguous,
    ``scale`` fp32 ``[N]`` contiguous, K a multiple of 64, N a multiple of 8, row strides that keep every row
    16-byte aligned, and 16-byte aligned base pointers."""
    if not (x2.is_cuda and codes.is_cuda and scale.is_cuda and codes.device == x2.device == scale.device):
        return False
    if x2.dtype != torch.bfloat16 or codes.dtype != FP8 or scale.dtype != torch.float32:
        return False
    if x2.dim() != 2 or codes.dim() != 2 or scale.dim() != 1:
        return False
    (M, K), N = x2.shape, codes.shape[0]
    if codes.shape[1] != K or scale.shape[0] != N or M > linear_fp8_max_m():
        return False
    if M == 0 or N == 0:
        return True  # an empty result, no launch
    if K < 64 or K % 64 != 0 or N % 8 != 0:
        return False
    if x2.stride(1) != 1 or (M > 1 and (x2.stride(0) < K or x2.stride(0) % 8 != 0)):
        return False
    if codes.stride(1) != 1 or (N > 1 and (codes.stride(0) < K or codes.stride(0) % 16 != 0)):
        return False
    return scale.is_contiguous() and all(t.data_ptr() % 16 == 0 for t in (x2, codes, scale))


def linear_fp8_gemm_splits(M: int, N: int, K: int) -> int:
    """The K slabs the large-M kernel (``linear_fp8_gemm.hip``) cuts K into for these shapes: from M, N, K and the
    CU count only, never from data, and 1 whenever the fp32 partials would pass 256 MiB."""
    return native.C().linear_fp8_gemm_splits(M, N, K)


# cs_linear_fp8_gemm (csrc/kernels/launchers.h): offsets inside a tile's buffer descriptor are 32-bit. A tile
# addresses 128 rows, at most 128 * 2 * ldx bytes of x and 128 * ldw bytes of codes, and both stay below 0x7ffffff0
_GEMM_OOB = 0x7FFFFFF0
_GEMM_TILE_ROWS = 128
# The most rows linear_fp8 sends to the GEMM. docs/linear_fp8.md, "Measurements, M > 64": up to 6144 rows the kernel
# beats the dequantise-and-multiply path on all five Llama-3-8B shapes by more than the run-to-run spread (1.09x to
# 1.5x at 3072 to 6144 rows); at 8192 rows the slow path wins on 4096 x 4096 (0.97x) and ties on 4096 x 14336, and
# generate with a prefill of 8192 rows is 1.2 % slower on the kernel. The kernel itself takes any M.
_GEMM_MAX_M = 6144


def _gemm_layout_ok(x2: torch.Tensor, codes: torch.Tensor, scale: torch.Tensor) -> bool:
    """the host-side arithmetic of ``linear_fp8_gemm_ok``: types, shapes and strides, whatever device holds them"""
    if x2.dtype != torch.bfloat16 or codes.dtype != FP8 or scale.dtype != torch.float32:
        return False
    if x2.dim() != 2 or codes.dim() != 2 or scale.dim() != 1:
        return False
    (M, K), N = x2.shape, codes.shape[0]
    if codes.shape[1] != K or scale.shape[0] != N or not linear_fp8_max_m() < M <= _GEMM_MAX_M or max(N, K) >= 2**31:
        return False
    if N == 0:
        return True  # an empty result, no launch
    if K < 64 or K % 64 != 0 or N % 8 != 0:
        return False
    ldx, ldw = x2.stride(0), codes.stride(0) if N > 1 else K
    if x2.stride(1) != 1 or ldx < K or ldx % 8 != 0 or codes.stride(1) != 1 or ldw < K or ldw % 16 != 0:
        return False
    return _GEMM_TILE_ROWS * 2 * ldx < _GEMM_OOB and _GEMM_TILE_ROWS * ldw < _GEMM_OOB and scale.is_contiguous()


def linear_fp8_gemm_ok(x2: torch.Tensor, codes: torch.Tensor, scale: torch.Tensor) -> bool:
    """Whether ``linear_fp8_gemm_kernel`` takes these operands and ``linear_fp8`` sends them there: the conditions of
    ``linear_fp8_native_ok`` with ``linear_fp8_max_m()`` < M <= 6144 in place of the cap on M (above 6144 rows the
    slow path measured no slower: ``_GEMM_MAX_M``), and row strides whose 32-bit offsets fit a tile's buffer
    descriptor (x up to 8388607 elements, codes up to 16777215 bytes). The tensors themselves may pass 2^31 bytes."""
    if not (x2.is_cuda and codes.is_cuda and scale.is_cuda and codes.device == x2.device == scale.device):
        return False
    return _gemm_layout_ok(x2, codes, scale) and all(t.data_ptr() % 16 == 0 for t in (x2, codes, scale))


def _dequant_mm(x2: torch.Tensor, codes: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """The slow path on the GPU for bf16 ``x2``: the weight dequantised to bf16 (exact), then the bf16 GEMM"""
    from .lm import _mm
    with torch.autocast("cuda", enabled=False):
        return _mm(x2, kv_dequantize(codes, scale, torch.bfloat16).t())


def linear_fp8(x: torch.Tensor, codes: torch.Tensor, scale: torch.Tensor, splits: Optional[int] = None,
               slabs: Optional[int] = None) -> torch.Tensor:
    """``y[..., N] = x[..., K] @ (codes[N, K] * scale[N, None])^T`` in ``x``'s dtype.

    Two gfx950 kernels serve ``x`` flattened to ``[M, K]``. When ``linear_fp8_native_ok`` holds the skinny kernel
    runs: decode steps and short extends (M up to ``linear_fp8_max_m()``). Otherwise, when ``linear_fp8_gemm_ok``
    holds, the LDS-tiled GEMM of ``linear_fp8_gemm.hip`` runs: prefills, chunks of a chunked prefill, long extends
    and decode batches above ``linear_fp8_max_m()`` and up to 6144 rows; it reads the codes once and never
    materialises a bf16 weight. Anything else takes the slow path: on the GPU with a bf16 ``x`` the weight is dequantised to bf16 and
    multiplied by the bf16 GEMM of ``ops.lm``, and everywhere else ``linear_fp8_ref`` runs.

    Both kernels cut K into slabs and sum them in a fixed order. ``slabs`` is their number; it fixes the summation
    order and so the last bits of the result. On the skinny kernel ``None`` is ``linear_fp8_splits(M, N, K)`` and
    anything else is clamped into [1, K / 128]; on the GEMM ``None`` is ``linear_fp8_gemm_splits(M, N, K)`` and
    anything else is clamped into [1, K / 64], and for a fixed ``slabs`` a row's bits do not depend on M or on where
    the row stands, so chunking a prefill differently changes nothing. The two kernels sum in different orders:
    their results agree to rounding, not bit for bit. ``splits`` is a workgroup count of the skinny kernel, not a
    slab count: how many workgroups share the slabs of a channel tile (``None``: one per slab; otherwise clamped
    into [1, slabs]). It moves work and changes no bit of the result; the GEMM ignores it. Both are ignored off
    the kernels. Inference only."""
    _no_grad_inputs("linear_fp8", x, scale)
    K = x.shape[-1]
    x2 = x.reshape(-1, K)
    if linear_fp8_native_ok(x2, codes, scale):
        with torch.no_grad():
            y = native.C().linear_fp8(x2, codes, scale, 0 if splits is None else max(int(splits), 1),
                                      0 if slabs is None else max(int(slabs), 1))
    elif linear_fp8_gemm_ok(x2, codes, scale):
        with torch.no_grad():
            y = native.C().linear_fp8_gemm(x2, codes, scale, 0 if slabs is None else max(int(slabs), 1))
    elif x2.is_cuda and x2.dtype == torch.bfloat16 and codes.is_cuda:
        y = _dequant_mm(x2, codes, scale)
    else:
        y = linear_fp8_ref(x2, codes, scale)
    return y.view(*x.shape[:-1], codes.shape[0])


def linear_fp8_grouped_splits(M: int, Ns, K: int) -> int:
    """The K slabs ``linear_fp8_grouped`` sums for weights of ``Ns`` output channels: ``linear_fp8_splits``'s rule on
    the summed 32-channel tiles of all weights, from the shapes and the CU count only."""
    return native.C().linear_fp8_grouped_splits(M, [int(n) for n in Ns], K)


def swiglu_linear_fp8_splits(M: int, N: int, K: int) -> int:
    """The K slabs ``swiglu_linear_fp8`` sums: the same rule on its ``ceil(N / 16)`` workgroups per slab."""
    return native.C().swiglu_linear_fp8_splits(M, N, K)


def _fused_ok(x2: torch.Tensor, weights) -> bool:
    """every operand passes ``linear_fp8_native_ok`` and nothing is empty (an empty result needs no kernel)"""
    return x2.shape[0] > 0 and all(c.dim() == 2 and c.shape[0] > 0 and linear_fp8_native_ok(x2, c, s)
                                   for c, s in weights)


def _grouped_composition(x, weights, splits, slabs) -> tuple:
    return tuple(linear_fp8(x, c, s, splits, slabs) for c, s in weights)


def _swiglu_composition(x, gate_codes, gate_scale, up_codes, up_scale, splits, slabs) -> torch.Tensor:
    from .lm import swiglu
    return swiglu(linear_fp8(x, gate_codes, gate_scale, splits, slabs), linear_fp8(x, up_codes, up_scale, splits, slabs))


def linear_fp8_grouped(x: torch.Tensor, weights, splits: Optional[int] = None, slabs: Optional[int] = None) -> tuple:
    """``linear_fp8(x, codes_i, scale_i)`` for 1 to 3 ``(codes, scale)`` pairs that share ``x`` (q, k and v), as a
    tuple. When every pair passes ``linear_fp8_native_ok`` one grouped launch of the gfx950 kernel computes all of
    them (and one combine, when K is split): every weight stays its own tensor, and the narrow ones ride in the grid
    of the wide one. Each result has the bits ``linear_fp8`` gives at the same ``slabs``; ``None`` is
    ``linear_fp8_grouped_splits``, picked from the summed tiles, so it can differ from what the separate calls
    pick. ``splits`` as in ``linear_fp8``. Anything the kernel does not take is ``linear_fp8`` per weight."""
    weights = [tuple(w) for w in weights]
    if not 1 <= len(weights) <= 3 or any(len(w) != 2 for w in weights):
        raise ValueError(f"linear_fp8_grouped: 1 to 3 (codes, scale) pairs, got {len(weights)}")
    K = x.shape[-1]
    for codes, scale in weights:
        if codes.dim() != 2 or codes.shape[1] != K or scale.shape != codes.shape[:1]:
            raise ValueError(f"linear_fp8_grouped: codes {tuple(codes.shape)} and scale {tuple(scale.shape)} do not "
                             f"match x [..., {K}]")
    _no_grad_inputs("linear_fp8_grouped", x, *(s for _, s in weights))
    x2 = x.reshape(-1, K)
    if not _fused_ok(x2, weights):
        return _grouped_composition(x, weights, splits, slabs)
    with torch.no_grad():
        ys = native.C().linear_fp8_grouped(x2, [c for c, _ in weights], [s for _, s in weights],
                                           0 if splits is None else max(int(splits), 1),
                                           0 if slabs is None else max(int(slabs), 1))
    return tuple(y.view(*x.shape[:-1], y.shape[1]) for y in ys)


def swiglu_linear_fp8(x: torch.Tensor, gate_codes: torch.Tensor, gate_scale: torch.Tensor, up_codes: torch.Tensor,
                      up_scale: torch.Tensor, splits: Optional[int] = None, slabs: Optional[int] = None) -> torch.Tensor:
    """``ops.lm.swiglu(linear_fp8(x, gate), linear_fp8(x, up))`` for two weights ``[N, K]``. When both pass
    ``linear_fp8_native_ok`` one launch of the gfx950 kernel computes it (and one combine, when K is split): a
    workgroup owns 16 gate channels and the same 16 up channels, rounds both sums to bf16 as the separate calls
    would and applies SwiGLU in its epilogue, so neither ``[M, N]`` intermediate is written or read and the bits
    are the composition's at the same ``slabs`` (``None``: ``swiglu_linear_fp8_splits``). Anything else is that
    composition."""
    if gate_codes.dim() != 2 or gate_codes.shape != up_codes.shape or gate_codes.shape[1] != x.shape[-1]:
        raise ValueError(f"swiglu_linear_fp8: gate {tuple(gate_codes.shape)} and up {tuple(up_codes.shape)} must be one "
                         f"shape [N, {x.shape[-1]}]")
    if gate_scale.shape != gate_codes.shape[:1] or up_scale.shape != up_codes.shape[:1]:
        raise ValueError("swiglu_linear_fp8: a scale must be [N]")
    _no_grad_inputs("swiglu_linear_fp8", x, gate_scale, up_scale)
    x2 = x.reshape(-1, x.shape[-1])
    if not _fused_ok(x2, ((gate_codes, gate_scale), (up_codes, up_scale))):
        return _swiglu_composition(x, gate_codes, gate_scale, up_codes, up_scale, splits, slabs)
    with torch.no_grad():
        y = native.C().swiglu_linear_fp8(x2, gate_codes, gate_scale, up_codes, up_scale,
                                         0 if splits is None else max(int(splits), 1),
                                         0 if slabs is None else max(int(slabs), 1))
    return y.view(*x.shape[:-1], gate_codes.shape[0])


def autocast_input(x: torch.Tensor) -> torch.Tensor:
    """``x`` as an ``Fp8Linear`` reads it: cast to bf16 under bf16 GPU autocast, untouched otherwise"""
    if x.is_cuda and torch.is_autocast_enabled("cuda") and torch.get_autocast_dtype("cuda") == torch.bfloat16:
        return x.to(torch.bfloat16)
    return x


class Fp8Linear(torch.nn.Module):
    """A bias-free projection whose weight is FP8 codes (buffer ``weight`` ``[out, in]``) and per-channel scales
    (buffer ``weight_scale`` ``[out]``). Inference only: an input that requires grad raises. Under bf16 GPU
    autocast the input is cast to bf16, as ``ShadowLinear`` does, and the result is bf16."""

    def __init__(self, in_features: int, out_features: int, device=None):
        super().__init__()
        self.in_features, self.out_features = in_features, out_features
        self.register_buffer("weight", torch.zeros(out_features, in_features, dtype=torch.uint8, device=device).view(FP8))
        self.register_buffer("weight_scale", torch.ones(out_features, device=device))

    @classmethod
    def from_linear(cls, lin: torch.nn.Linear) -> "Fp8Linear":
        if lin.bias is not None:
            raise ValueError("Fp8Linear.from_linear: the projection must be bias-free")
        m = cls(lin.in_features, lin.out_features, device=lin.weight.device)
        m.weight, m.weight_scale = quantize_weight_fp8(lin.weight)
        return m

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return linear_fp8(autocast_input(x), self.weight, self.weight_scale)

    def extra_repr(self) -> str:
        return f"in_features={self.in_features}, out_features={self.out_features}, weight=float8_e4m3fn"
