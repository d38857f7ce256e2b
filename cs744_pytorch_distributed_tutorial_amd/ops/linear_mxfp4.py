"""MXFP4 weight-only projections (W4A16): ``csrc/kernels/linear_mxfp4.hip`` for decoding (up to 64 rows) and
``csrc/kernels/linear_mxfp4_gemm.hip`` for prefills and larger batches.

A weight ``[N, K]`` is stored in the OCP microscaling format: ``codes`` uint8 ``[N, K/2]``, two e2m1 codes per byte
(element ``2i`` in the low nibble, ``2i+1`` in the high one; values +-{0, 0.5, 1, 1.5, 2, 3, 4, 6}), and ``scales``
uint8 ``[N, K/32]``, one e8m0 exponent per block of 32 consecutive k of a row: the weight is
``code * 2^(scale - 127)``. A code has 2 significant bits and a scale is a power of two, so every dequantised
weight is exactly a bf16 number and the kernel's only roundings are its fp32 sums and the bf16 store. A decode
projection is bound by its weight bytes: 0.53 of the FP8 format's (``ops.linear_fp8``), 0.27 of the bf16
shadow's. Inference only. ``docs/linear_mxfp4.md`` has the design and the measurements."""
from __future__ import annotations

from typing import Optional

import torch

from . import native
from .attention import _no_grad_inputs
from .linear_fp8 import autocast_input

BLOCK = 32  # k per scale
_GRID = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)  # the value of magnitude code 0..7; bit 3 of a code is the sign
_E_MIN, _E_MAX = -125, 125  # block exponents kept: every dequantised value is a normal bf16 number


def quantize_weight_mxfp4(w: torch.Tensor) -> tuple:
    """``w`` ``[N, K]`` (fp32, bf16 or fp64, any device, K a multiple of 32) -> ``(codes uint8 [N, K/2], scales
    uint8 [N, K/32])``. Per block of 32 the exponent ``e`` is the smallest integer with ``amax * 2^-e <= 6`` (nothing
    saturates: the rule of the FP8 formats here), clamped into [-125, 125], 0 for an all-zero block; the elements
    are rounded to the nearest e2m1 value, ties to the even code, in float64."""
    if w.dim() != 2 or w.shape[1] % BLOCK != 0:
        raise ValueError(f"quantize_weight_mxfp4: the weight must be [N, K] with K a multiple of {BLOCK}, got {tuple(w.shape)}")
    N, K = w.shape
    b = w.detach().to(torch.float64).view(N, K // BLOCK, BLOCK)
    # amax = m * 2^x with m in [0.5, 1): amax <= 6 * 2^e = 0.75 * 2^(e + 3), so e = x - 3 when m <= 0.75, x - 2 above
    m, x = torch.frexp(b.abs().amax(dim=-1))
    e = torch.where(m <= 0.75, x - 3, x - 2)
    e = torch.where(m == 0, torch.zeros_like(e), e).clamp(_E_MIN, _E_MAX)
    inv = ((1023 - e.to(torch.int64)) << 52).view(torch.float64)  # 2^-e, bit for bit
    v = (b.abs() * inv.unsqueeze(-1)).clamp(max=6.0)  # exact; the clamp acts only where e was clamped down
    grid = torch.tensor(_GRID, dtype=torch.float64, device=w.device)
    mids = (grid[:-1] + grid[1:]) / 2
    lo, hi = torch.bucketize(v, mids), torch.bucketize(v, mids, right=True)  # they differ exactly on a tie
    mag = torch.where(lo == hi, lo, lo + (lo & 1))
    code = (mag | (torch.signbit(b).to(mag.dtype) << 3)).to(torch.uint8).view(N, K)
    return code[:, 0::2] | (code[:, 1::2] << 4), (e + 127).to(torch.uint8)


def dequantize_mxfp4(codes: torch.Tensor, scales: torch.Tensor, dtype: torch.dtype = torch.bfloat16) -> torch.Tensor:
    """``(codes [N, K/2], scales [N, K/32])`` -> the weight ``[N, K]`` in ``dtype`` (bf16, fp32 or fp64): exact"""
    N, K = codes.shape[0], codes.shape[1] * 2
    grid = torch.tensor(_GRID + tuple(-g for g in _GRID), dtype=torch.float32, device=codes.device)
    nib = torch.stack((codes & 15, codes >> 4), dim=-1).view(N, K // BLOCK, BLOCK)
    two_e = (scales.to(torch.int32) << 23).view(torch.float32)  # 2^(scale - 127), bit for bit
    return (grid[nib.long()] * two_e.unsqueeze(-1)).view(N, K).to(dtype)


def linear_mxfp4_ref(x: torch.Tensor, codes: torch.Tensor, scales: torch.Tensor) -> torch.Tensor:
    """``x @ dequantize_mxfp4(codes, scales)^T`` in plain torch: fp32 math (fp64 for an fp64 ``x``), the result in
    ``x``'s dtype. ``x`` ``[..., K]``."""
    ct = torch.float64 if x.dtype == torch.float64 else torch.float32
    return (x.to(ct) @ dequantize_mxfp4(codes, scales, ct).t()).to(x.dtype)


def linear_mxfp4_max_m() -> int:
    """The most rows of ``x`` the kernel takes."""
    return native.C().linear_mxfp4_max_m()


def linear_mxfp4_splits(M: int, N: int, K: int) -> int:
    """The K slabs the kernel splits K into, and sums in order, for these shapes: from M, N, K and the CU count
    only, never from data."""
    return native.C().linear_mxfp4_splits(M, [int(N)], K)


def linear_mxfp4_grouped_splits(M: int, Ns, K: int) -> int:
    """The K slabs ``linear_mxfp4_grouped`` sums: the same rule on the summed 32-channel tiles of all weights."""
    Ns = [int(n) for n in Ns]
    return native.C().linear_mxfp4_splits(M, Ns, K) if len(Ns) > 1 else linear_mxfp4_splits(M, Ns[0], K)


def swiglu_linear_mxfp4_splits(M: int, N: int, K: int) -> int:
    """The K slabs ``swiglu_linear_mxfp4`` sums: the same rule on its ``ceil(N / 16)`` workgroups per slab."""
    return native.C().linear_mxfp4_splits(M, [int(N)], K, True)


def linear_mxfp4_native_ok(x2: torch.Tensor, codes: torch.Tensor, scales: torch.Tensor) -> bool:
    """Whether ``linear_mxfp4_kernel`` takes these operands: everything on one GPU, ``x2`` bf16 ``[M, K]`` with unit
    inner stride and M at most ``linear_mxfp4_max_m()``, ``codes`` uint8 ``[N, K/2]`` and ``scales`` uint8
    ``[N, K/32]`` with unit inner stride, K a multiple of 128, N a multiple of 8, row strides that keep the rows of
    ``x2`` and ``codes`` 16-byte aligned, and 16-byte aligned base pointers."""
    if not (x2.is_cuda and codes.is_cuda and scales.is_cuda and codes.device == x2.device == scales.device):
        return False
    if x2.dtype != torch.bfloat16 or codes.dtype != torch.uint8 or scales.dtype != torch.uint8:
        return False
    if x2.dim() != 2 or codes.dim() != 2 or scales.dim() != 2:
        return False
    (M, K), N = x2.shape, codes.shape[0]
    if codes.shape[1] * 2 != K or scales.shape != (N, K // BLOCK) or K % BLOCK != 0 or M > linear_mxfp4_max_m():
        return False
    if M == 0 or N == 0:
        return True  # an empty result, no launch
    if K < 128 or K % 128 != 0 or N % 8 != 0:
        return False
    if x2.stride(1) != 1 or (M > 1 and (x2.stride(0) < K or x2.stride(0) % 8 != 0)):
        return False
    if codes.stride(1) != 1 or codes.stride(0) < K // 2 or codes.stride(0) % 16 != 0:
        return False
    if scales.stride(1) != 1 or scales.stride(0) < K // BLOCK:
        return False
    return all(t.data_ptr() % 16 == 0 for t in (x2, codes, scales))


def linear_mxfp4_gemm_splits(M: int, N: int, K: int) -> int:
    """The K slabs the large-M kernel (``linear_mxfp4_gemm.hip``) cuts K into for these shapes: from M, N, K and the
    CU count only, never from data, and 1 whenever the fp32 partials would pass 256 MiB."""
    return native.C().linear_mxfp4_gemm_splits(M, N, K)


# cs_linear_mxfp4_gemm (csrc/kernels/launchers.h): offsets inside a tile's buffer descriptor are 32-bit. A tile
# addresses 128 rows, at most 128 * 2 * ldx bytes of x, 128 * ldw of codes and 128 * lds of scales, all below 0x7ffffff0
_GEMM_OOB = 0x7FFFFFF0
_GEMM_TILE_ROWS = 128
# The most rows linear_mxfp4 sends to the GEMM: no cap. docs/linear_mxfp4.md, "Measurements, M > 64": from 64 to 8192
# rows the kernel beats the dequantise-and-multiply path on all five Llama-3-8B shapes (1.31x at worst, 4096 x 14336
# at 8192 rows) where the two runs differ by 1 % there and 7 % at most
_GEMM_MAX_M = 2**31 - 1


def _gemm_layout_ok(x2: torch.Tensor, codes: torch.Tensor, scales: torch.Tensor) -> bool:
    """the host-side arithmetic of ``linear_mxfp4_gemm_ok``: types, shapes and strides, whatever device holds them"""
    if x2.dtype != torch.bfloat16 or codes.dtype != torch.uint8 or scales.dtype != torch.uint8:
        return False
    if x2.dim() != 2 or codes.dim() != 2 or scales.dim() != 2:
        return False
    (M, K), N = x2.shape, codes.shape[0]
    if K % BLOCK != 0 or codes.shape[1] * 2 != K or scales.shape != (N, K // BLOCK) or max(N, K) >= 2**31:
        return False
    if not linear_mxfp4_max_m() < M <= _GEMM_MAX_M:
        return False
    if N == 0:
        return True  # an empty result, no launch
    if K < 128 or K % 128 != 0 or N % 8 != 0:
        return False
    ldx = x2.stride(0)
    ldw, lds = (codes.stride(0), scales.stride(0)) if N > 1 else (K // 2, K // BLOCK)
    if x2.stride(1) != 1 or ldx < K or ldx % 8 != 0 or codes.stride(1) != 1 or ldw < K // 2 or ldw % 16 != 0:
        return False
    if scales.stride(1) != 1 or lds < K // BLOCK or lds % 4 != 0:
        return False
    return max(2 * ldx, ldw, lds) * _GEMM_TILE_ROWS < _GEMM_OOB


def linear_mxfp4_gemm_ok(x2: torch.Tensor, codes: torch.Tensor, scales: torch.Tensor) -> bool:
    """Whether ``linear_mxfp4_gemm_kernel`` takes these operands and ``linear_mxfp4`` sends them there: the
    conditions of ``linear_mxfp4_native_ok`` with M above ``linear_mxfp4_max_m()`` in place of the cap on M, scale
    rows a multiple of 4 bytes apart from a 4-byte aligned base (they are staged four bytes at a time), and row
    strides whose 32-bit offsets fit a tile's buffer descriptor (x up to 8388607 elements, codes and scales up to
    16777215 bytes). The tensors themselves may pass 2^31 bytes."""
    if not (x2.is_cuda and codes.is_cuda and scales.is_cuda and codes.device == x2.device == scales.device):
        return False
    if not _gemm_layout_ok(x2, codes, scales):
        return False
    return x2.data_ptr() % 16 == 0 and codes.data_ptr() % 16 == 0 and scales.data_ptr() % 4 == 0


def _dequant_mm(x2: torch.Tensor, codes: torch.Tensor, scales: torch.Tensor) -> torch.Tensor:
    """The slow path on the GPU for bf16 ``x2``: the weight dequantised to bf16 (exact), then the bf16 GEMM"""
    from .lm import _mm
    with torch.autocast("cuda", enabled=False):
        return _mm(x2, dequantize_mxfp4(codes, scales, torch.bfloat16).t())


def _arg(v: Optional[int]) -> int:
    return 0 if v is None else max(int(v), 1)


def _check_weight(fn: str, K: int, codes: torch.Tensor, scales: torch.Tensor) -> None:
    if codes.dim() != 2 or codes.shape[1] * 2 != K or K % BLOCK != 0 or scales.shape != (codes.shape[0], K // BLOCK):
        raise ValueError(f"{fn}: codes {tuple(codes.shape)} and scales {tuple(scales.shape)} do not match x [..., {K}]: "
                         f"[N, K/2] and [N, K/{BLOCK}]")


def linear_mxfp4(x: torch.Tensor, codes: torch.Tensor, scales: torch.Tensor, splits: Optional[int] = None,
                 slabs: Optional[int] = None) -> torch.Tensor:
    """``y[..., N] = x[..., K] @ dequantize_mxfp4(codes, scales)^T`` in ``x``'s dtype.

    Two gfx950 kernels serve ``x`` flattened to ``[M, K]``. When ``linear_mxfp4_native_ok`` holds the skinny kernel
    runs: decode steps and short extends (M up to ``linear_mxfp4_max_m()``). Otherwise, when
    ``linear_mxfp4_gemm_ok`` holds, the LDS-tiled GEMM of ``linear_mxfp4_gemm.hip`` runs: prefills, chunks of a
    chunked prefill, long extends and decode batches above ``linear_mxfp4_max_m()`` rows; it reads the codes once
    and never materialises a bf16 weight. Anything else takes the slow path: on the GPU with a bf16 ``x`` the weight
    is dequantised to bf16 and multiplied by the bf16 GEMM of ``ops.lm``, and everywhere else ``linear_mxfp4_ref``
    runs.

    Both kernels cut K into slabs and sum them in a fixed order. ``slabs`` is their number; it fixes the summation
    order and so the last bits of the result. On the skinny kernel ``None`` is ``linear_mxfp4_splits(M, N, K)`` and
    anything else is clamped into [1, K / 256]; on the GEMM ``None`` is ``linear_mxfp4_gemm_splits(M, N, K)`` and
    anything else is clamped into [1, K / 128], and for a fixed ``slabs`` a row's bits do not depend on M or on
    where the row stands, so chunking a prefill differently changes nothing. The two kernels sum in different
    orders: their results agree to rounding, not bit for bit. ``splits`` is how many workgroups of the skinny kernel
    share the slabs of a channel tile (``None``: one per slab; otherwise clamped into [1, slabs]); it moves work
    and changes no bit, and the GEMM ignores it. Both are ignored off the kernels. Inference only."""
    _check_weight("linear_mxfp4", x.shape[-1], codes, scales)
    _no_grad_inputs("linear_mxfp4", x)
    x2 = x.reshape(-1, x.shape[-1])
    if linear_mxfp4_native_ok(x2, codes, scales):
        if x2.shape[0] == 0 or codes.shape[0] == 0:
            y = x2.new_empty(x2.shape[0], codes.shape[0])
        else:
            with torch.no_grad():
                y = native.C().linear_mxfp4(x2, codes, scales, _arg(splits), _arg(slabs))
    elif linear_mxfp4_gemm_ok(x2, codes, scales):
        with torch.no_grad():
            y = native.C().linear_mxfp4_gemm(x2, codes, scales, _arg(slabs))
    elif x2.is_cuda and x2.dtype == torch.bfloat16 and codes.is_cuda:
        y = _dequant_mm(x2, codes, scales)
    else:
        y = linear_mxfp4_ref(x2, codes, scales)
    return y.view(*x.shape[:-1], codes.shape[0])


def _fused_ok(x2: torch.Tensor, weights) -> bool:
    """every operand passes ``linear_mxfp4_native_ok`` and nothing is empty (an empty result needs no kernel)"""
    return x2.shape[0] > 0 and all(c.shape[0] > 0 and linear_mxfp4_native_ok(x2, c, s) for c, s in weights)


def linear_mxfp4_grouped(x: torch.Tensor, weights, splits: Optional[int] = None, slabs: Optional[int] = None) -> tuple:
    """``linear_mxfp4(x, codes_i, scales_i)`` for 1 to 3 ``(codes, scales)`` pairs that share ``x`` (q, k and v), as a
    tuple. When every pair passes ``linear_mxfp4_native_ok`` one launch of the gfx950 kernel computes all of them
    (and one combine, when K is split). Each result has the bits ``linear_mxfp4`` gives at the same ``slabs``;
    ``None`` is ``linear_mxfp4_grouped_splits``, picked from the summed tiles. Anything the kernel does not take is
    ``linear_mxfp4`` per weight."""
    weights = [tuple(w) for w in weights]
    if not 1 <= len(weights) <= 3 or any(len(w) != 2 for w in weights):
        raise ValueError(f"linear_mxfp4_grouped: 1 to 3 (codes, scales) pairs, got {len(weights)}")
    for codes, scales in weights:
        _check_weight("linear_mxfp4_grouped", x.shape[-1], codes, scales)
    _no_grad_inputs("linear_mxfp4_grouped", x)
    x2 = x.reshape(-1, x.shape[-1])
    if not _fused_ok(x2, weights):
        return tuple(linear_mxfp4(x, c, s, splits, slabs) for c, s in weights)
    with torch.no_grad():
        ys = native.C().linear_mxfp4_grouped(x2, [c for c, _ in weights], [s for _, s in weights], _arg(splits), _arg(slabs))
    return tuple(y.view(*x.shape[:-1], y.shape[1]) for y in ys)


def swiglu_linear_mxfp4(x: torch.Tensor, gate_codes: torch.Tensor, gate_scales: torch.Tensor, up_codes: torch.Tensor,
                        up_scales: torch.Tensor, splits: Optional[int] = None, slabs: Optional[int] = None) -> torch.Tensor:
    """``ops.lm.swiglu(linear_mxfp4(x, gate), linear_mxfp4(x, up))`` for two weights ``[N, K]``. When both pass
    ``linear_mxfp4_native_ok`` one launch of the gfx950 kernel computes it (and one combine, when K is split): a
    workgroup owns 16 gate channels and the same 16 up channels, rounds both sums to bf16 as the separate calls
    would and applies SwiGLU in its epilogue, so the bits are the composition's at the same ``slabs`` (``None``:
    ``swiglu_linear_mxfp4_splits``). Anything else is that composition."""
    _check_weight("swiglu_linear_mxfp4", x.shape[-1], gate_codes, gate_scales)
    _check_weight("swiglu_linear_mxfp4", x.shape[-1], up_codes, up_scales)
    if gate_codes.shape != up_codes.shape:
        raise ValueError(f"swiglu_linear_mxfp4: gate {tuple(gate_codes.shape)} and up {tuple(up_codes.shape)} must be one shape")
    _no_grad_inputs("swiglu_linear_mxfp4", x)
    x2 = x.reshape(-1, x.shape[-1])
    if not _fused_ok(x2, ((gate_codes, gate_scales), (up_codes, up_scales))):
        from .lm import swiglu
        return swiglu(linear_mxfp4(x, gate_codes, gate_scales, splits, slabs),
                      linear_mxfp4(x, up_codes, up_scales, splits, slabs))
    with torch.no_grad():
        y = native.C().swiglu_linear_mxfp4(x2, gate_codes, gate_scales, up_codes, up_scales, _arg(splits), _arg(slabs))
    return y.view(*x.shape[:-1], gate_codes.shape[0])


class Mxfp4Linear(torch.nn.Module):
    """A bias-free projection whose weight is MXFP4: buffers ``weight`` (uint8 ``[out, in/2]``, e2m1 codes) and
    ``weight_scale`` (uint8 ``[out, in/32]``, e8m0 block exponents). Inference only: an input that requires grad
    raises. Under bf16 GPU autocast the input is cast to bf16, as ``Fp8Linear`` does, and the result is bf16."""

    def __init__(self, in_features: int, out_features: int, device=None):
        super().__init__()
        if in_features % BLOCK != 0:
            raise ValueError(f"Mxfp4Linear: in_features must be a multiple of {BLOCK}, got {in_features}")
        self.in_features, self.out_features = in_features, out_features
        self.register_buffer("weight", torch.zeros(out_features, in_features // 2, dtype=torch.uint8, device=device))
        self.register_buffer("weight_scale", torch.full((out_features, in_features // BLOCK), 127, dtype=torch.uint8,
                                                        device=device))

    @classmethod
    def from_linear(cls, lin: torch.nn.Linear) -> "Mxfp4Linear":
        if lin.bias is not None:
            raise ValueError("Mxfp4Linear.from_linear: the projection must be bias-free")
        m = cls(lin.in_features, lin.out_features, device=lin.weight.device)
        m.weight, m.weight_scale = quantize_weight_mxfp4(lin.weight)
        return m

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return linear_mxfp4(autocast_input(x), self.weight, self.weight_scale)

    def extra_repr(self) -> str:
        return f"in_features={self.in_features}, out_features={self.out_features}, weight=mxfp4"
