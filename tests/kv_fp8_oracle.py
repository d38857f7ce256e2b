"""Oracle of the FP8 KV-cache format for tests/test_kv_fp8_cpu.py and tests/test_kv_fp8_gpu.py, written
independently of ops.attention.kv_quantize_ref: the exponent comes from float64 ``frexp`` of amax / 448 (not
from amax with a mantissa threshold), the scaling is a float64 product, and the only rounding to e4m3fn is
torch's CPU cast of the fp32 value. The attention oracle is decode_oracle64 on the dequantised caches."""
import torch

from decode_oracle import decode_oracle64

FP8 = torch.float8_e4m3fn


def quantize_oracle(x):
    """x [..., D] (any float dtype, any device) -> (codes float8_e4m3fn [..., D], scale fp32 [...]) on the host.
    s = 2^e, e the smallest integer with amax * 2^-e <= 448, e >= -126; amax == 0 -> s = 1."""
    x64 = x.detach().double().cpu()
    amax = x64.abs().amax(-1)
    # amax / 448 = m * 2^ex with m in [0.5, 1): 2^ex >= amax / 448 always, 2^(ex-1) only when m == 0.5
    m, ex = torch.frexp(amax / 448.0)
    e = torch.where(m == 0.5, ex - 1, ex).clamp(min=-126).long()
    e = torch.where(amax > 0, e, torch.zeros_like(e))
    scaled = x64 * torch.pow(torch.tensor(2.0, dtype=torch.float64), -e.double()).unsqueeze(-1)
    assert not (scaled.abs() > 448).any(), "the format never needs saturation"
    return scaled.float().to(FP8), torch.pow(torch.tensor(2.0, dtype=torch.float64), e.double()).float()


def dequantize_oracle(codes, scale):
    """-> float64 [..., D]: float(code) * scale, exact"""
    return codes.cpu().float().double() * scale.cpu().double().unsqueeze(-1)


def attention_oracle(q, k_codes, v_codes, k_scale, v_scale, lens, scale=None):
    """decode_oracle64 on the dequantised caches: exactly the values an FP8 kernel sees. -> (o float64
    [B, Hq, D], vmax float64 [B, Hkv] of the dequantised visible values)"""
    return decode_oracle64(q, dequantize_oracle(k_codes, k_scale), dequantize_oracle(v_codes, v_scale), lens, scale)


def stale_tail_(k_codes, v_codes, k_scale, v_scale, lens):
    """every position >= lens[b]: codes 0x7F (NaN) and scales NaN, in place"""
    for b in range(k_codes.shape[0]):
        n = min(max(int(lens[b]), 0), k_codes.shape[1])
        k_codes[b, n:].view(torch.uint8).fill_(0x7F)
        v_codes[b, n:].view(torch.uint8).fill_(0x7F)
        k_scale[b, n:] = float("nan")
        v_scale[b, n:] = float("nan")
    return k_codes, v_codes, k_scale, v_scale


def magnitude_rows(n=1000, D=128, seed=0, dtype=torch.bfloat16):
    """n rows of D values with row magnitudes from 1e-6 to 1e6, plus the edge rows: all zero, one non-zero
    element, amax exactly 448 * 2^k and the next bf16 above it (k = -20, -1, 0, 1, 7, 20)."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(n, D, generator=g) * torch.logspace(-6, 6, n).view(n, 1)).to(dtype)
    edge = [torch.zeros(D), torch.zeros(D)]
    edge[1][D // 3] = -3.0e-3
    for k in (-20, -1, 0, 1, 7, 20):
        at = 448.0 * 2.0 ** k
        above = at + 2.0 ** (k + 1)  # 448 = 1.75 * 2^8 and bf16 has 7 fraction bits: the next bf16 is 450 * 2^k
        for amax in (at, above):
            row = torch.rand(D, generator=g) * at * 0.99
            row[5] = -amax
            edge.append(row)
    return torch.cat([x, torch.stack(edge).to(dtype)])
