"""MXFP4 weight-only projections on the CPU: the quantiser, the reference, Mxfp4Linear and Llama.quantize_weights_."""
import pytest
import torch

from cs744_pytorch_distributed_tutorial_amd.models import llama
from cs744_pytorch_distributed_tutorial_amd.ops import linear_fp8, linear_mxfp4 as lx

GRID = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0], dtype=torch.float64)


def _w(N=24, K=128, seed=0):
    """blocks of magnitude 2^-10 .. 2^6, so the scales differ inside a row"""
    g = torch.Generator().manual_seed(seed)
    mag = torch.exp2(torch.randint(-10, 7, (N, K // 32, 1), generator=g).double())
    return (torch.randn(N, K // 32, 32, generator=g).double() * mag).view(N, K).float()


def _nibbles(codes):
    return torch.stack((codes & 15, codes >> 4), dim=-1).flatten(1)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float64])
def test_representable_inputs_round_trip(dtype):
    """every code under scales from both ends of the kept range: the format's own values come back bit for bit,
    the top of the grid in every block so that the block exponent is the one the value was built with"""
    g = torch.Generator().manual_seed(1)
    e = torch.tensor([[-125, -3, 0, 17], [125, -60, 1, -1]]).repeat(4, 1)                 # [8, 4] block exponents
    mag = GRID[torch.randint(0, 8, (8, 4, 32), generator=g)]
    mag[:, :, 0] = 6.0
    sign = 1.0 - 2.0 * torch.randint(0, 2, (8, 4, 32), generator=g).double()
    w = (mag * sign * torch.exp2(e.double())[:, :, None]).view(8, 128).to(dtype)
    codes, scales = lx.quantize_weight_mxfp4(w)
    assert codes.dtype == scales.dtype == torch.uint8 and codes.shape == (8, 64) and scales.shape == (8, 4)
    assert torch.equal(scales.long(), e + 127)
    assert torch.equal(lx.dequantize_mxfp4(codes, scales, dtype), w)
    assert torch.equal(_nibbles(codes)[:, 0::32] & 7, torch.full((8, 4), 7, dtype=torch.uint8))  # element 2i: low nibble


def test_quantiser_error_bound_and_idempotence():
    w = _w(seed=2)
    w[:, 32:64] = 0.0                                   # a zero block
    w[:2, :32] = 0.0
    w[0, 0], w[0, 1] = 6.0, 6.0 * (1 + 2.0 ** -20)      # amax just above the top of the grid: the next exponent
    w[1, 0] = 6.0                                       # amax on the top: e = 0, and every tie of the grid
    w[1, 5:12] = torch.tensor([-2.5, 0.25, 0.75, 1.25, 1.75, 3.5, 5.0])
    codes, scales = lx.quantize_weight_mxfp4(w)
    deq = lx.dequantize_mxfp4(codes, scales, torch.float64)
    two_e = ((scales.long() + (1023 - 127)) << 52).view(torch.float64).repeat_interleave(32, dim=1)
    v = w.double().abs() / two_e
    assert v.max() <= 6.0 and (v.view(24, 4, 32).amax(-1)[:, [0, 2, 3]] > 3.0).all()   # nothing saturates; e is the smallest
    # half the local grid step: the distance to the nearer neighbour of the grid interval v lies in
    i = torch.bucketize(v, GRID[1:], right=True).clamp(max=6)
    half_step = (GRID[i + 1] - GRID[i]) / 2
    assert ((w.double() - deq).abs() <= half_step * two_e).all()
    assert (scales[:, 1] == 127).all() and (codes[:, 16:32] == 0).all()
    assert scales[0, 0] == 128 and _nibbles(codes)[0, :2].tolist() == [5, 5]      # 6 / 2 and 6 (1 + 2^-20) / 2 -> 3
    assert scales[1, 0] == 127 and _nibbles(codes)[1, 5:12].tolist() == [12, 0, 2, 2, 4, 6, 6]  # ties to the even code
    # quantising the dequantised weight again: the same values everywhere, and the same codes and scales wherever
    # the largest code of the block is 4 or 6. (A block whose amax rounded down to 3 * 2^e is stored as 6 * 2^(e-1)
    # the second time, by the smallest-exponent rule: other codes, the same numbers.)
    again = lx.quantize_weight_mxfp4(deq)
    assert torch.equal(lx.dequantize_mxfp4(*again, torch.float64), deq)
    keeps = ((_nibbles(codes) & 7).view(24, 4, 32).amax(-1) >= 6) | (scales == 127) & (deq.view(24, 4, 32) == 0).all(-1)
    assert keeps.sum() > keeps.numel() // 2 and not keeps[0, 0]
    assert torch.equal(again[1][keeps], scales[keeps])
    assert torch.equal(again[0].view(24, 4, 16)[keeps], codes.view(24, 4, 16)[keeps])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float64])
def test_reference_against_float64(dtype):
    codes, scales = lx.quantize_weight_mxfp4(_w(seed=3))
    w = lx.dequantize_mxfp4(codes, scales, torch.float64)
    x = torch.randn(2, 5, 128, generator=torch.Generator().manual_seed(1)).to(dtype)
    y, ref = lx.linear_mxfp4_ref(x, codes, scales), x.double() @ w.T
    eps = {torch.float32: 2.0 ** -24, torch.bfloat16: 2.0 ** -8, torch.float64: 2.0 ** -53}[dtype]
    sums = 128 * (2.0 ** -53 if dtype == torch.float64 else 2.0 ** -24) * (x.double().abs() @ w.abs().T)
    assert y.dtype == dtype and y.shape == (2, 5, 24)
    assert ((y.double() - ref).abs() <= eps * ref.abs() + sums).all()
    assert torch.equal(lx.linear_mxfp4(x, codes, scales), y)  # the CPU path of the public entry is the reference


def test_mxfp4linear_from_linear_and_state_dict():
    lin = torch.nn.Linear(128, 24, bias=False)
    with torch.no_grad():
        lin.weight.copy_(_w(seed=4))
    q = lx.Mxfp4Linear.from_linear(lin)
    codes, scales = lx.quantize_weight_mxfp4(lin.weight)
    assert set(q.state_dict()) == {"weight", "weight_scale"} and not list(q.parameters())
    assert torch.equal(q.weight, codes) and torch.equal(q.weight_scale, scales)
    x = torch.randn(3, 128, generator=torch.Generator().manual_seed(3))
    fresh = lx.Mxfp4Linear(128, 24)
    fresh.load_state_dict(q.state_dict())
    assert torch.equal(fresh.weight, codes) and torch.equal(fresh(x), lx.linear_mxfp4_ref(x, codes, scales))
    with pytest.raises(RuntimeError, match="inference only"):
        q(x.clone().requires_grad_())
    with pytest.raises(ValueError, match="bias-free"):
        lx.Mxfp4Linear.from_linear(torch.nn.Linear(128, 24))


@pytest.mark.parametrize("head,fused", [(True, False), (False, True)])
def test_quantize_weights_mxfp4(head, fused):
    torch.manual_seed(0)
    m = llama.build("llama-tiny").eval()
    before = {k: v.clone() for k, v in m.state_dict().items()}
    assert m.quantize_weights_(dtype="mxfp4", head=head, fused=fused) is m
    swapped = {n for n, mod in m.named_modules() if isinstance(mod, lx.Mxfp4Linear)}
    want = {f"layers.{i}.{p}" for i in range(m.cfg.n_layers)
            for p in ("attention.wq", "attention.wk", "attention.wv", "attention.wo", "feed_forward.w1",
                      "feed_forward.w3", "feed_forward.w2")} | ({"output"} if head else set())
    assert swapped == want and not any(isinstance(mod, linear_fp8.Fp8Linear) for mod in m.modules())
    kept = {k for k in before if not any(k.startswith(w + ".") for w in want)}
    assert {n for n, _ in m.named_parameters()} == kept
    assert set(m.state_dict()) == kept | {f"{w}.{b}" for w in want for b in ("weight", "weight_scale")}
    tokens = torch.randint(1, m.cfg.vocab_size, (2, 6), generator=torch.Generator().manual_seed(1))
    out = m.generate(tokens, 4)
    assert out.shape == (2, 4) and int(out.min()) >= 0 and int(out.max()) < m.cfg.vocab_size
    with pytest.raises(ValueError, match="fp8"):
        m.quantize_weights_(dtype="int4")
    with pytest.raises(ValueError, match="another format"):
        m.quantize_weights_(dtype="fp8")
    assert m.quantize_weights_(dtype="mxfp4", head=head, fused=fused) is m  # idempotent
