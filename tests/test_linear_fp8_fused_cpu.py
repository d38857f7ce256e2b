"""The fused FP8 projections off the GPU: linear_fp8_grouped and swiglu_linear_fp8 are the composition of the public
functions, malformed arguments raise, and quantize_weights_(fused=True) changes neither logits nor state_dict."""
import pytest
import torch

from cs744_pytorch_distributed_tutorial_amd.models import llama
from cs744_pytorch_distributed_tutorial_amd.ops import linear_fp8 as lf, lm


def _w(N, K=64, seed=0):
    w = torch.randn(N, K, generator=torch.Generator().manual_seed(seed)) * torch.exp2(torch.linspace(-12, 4, N))[:, None]
    return lf.quantize_weight_fp8(w)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_cpu_is_the_composition(dtype):
    x = torch.randn(2, 3, 64, generator=torch.Generator().manual_seed(1)).to(dtype)
    ws = [_w(24, seed=1), _w(8, seed=2), _w(16, seed=3)]
    for G in (1, 2, 3):
        ys = lf.linear_fp8_grouped(x, ws[:G])
        assert isinstance(ys, tuple) and len(ys) == G
        assert all(torch.equal(y, lf.linear_fp8_ref(x, c, s)) for y, (c, s) in zip(ys, ws))
    (g, sg), (u, su) = _w(24, seed=4), _w(24, seed=5)
    want = lm.swiglu(lf.linear_fp8_ref(x, g, sg), lf.linear_fp8_ref(x, u, su))
    assert torch.equal(lf.swiglu_linear_fp8(x, g, sg, u, su), want) and want.shape == (2, 3, 24)


def test_malformed_arguments_raise():
    x = torch.randn(3, 64)
    w = _w(24)
    with pytest.raises(ValueError, match="1 to 3"):
        lf.linear_fp8_grouped(x, [])
    with pytest.raises(ValueError, match="1 to 3"):
        lf.linear_fp8_grouped(x, [w] * 4)
    with pytest.raises(ValueError, match="do not match"):
        lf.linear_fp8_grouped(x, [w, _w(24, K=128)])
    with pytest.raises(ValueError, match="one shape"):
        lf.swiglu_linear_fp8(x, *w, *_w(16))
    with pytest.raises(ValueError, match="one shape"):
        lf.swiglu_linear_fp8(x, *_w(24, K=128), *_w(24, K=128))
    with pytest.raises(RuntimeError, match="inference only"):
        lf.linear_fp8_grouped(x.clone().requires_grad_(), [w])
    with pytest.raises(RuntimeError, match="inference only"):
        lf.swiglu_linear_fp8(x.clone().requires_grad_(), *w, *w)


def test_model_fused_flag_changes_nothing_on_the_cpu():
    torch.manual_seed(0)
    plain = llama.build("llama-tiny").eval()
    fused = llama.build("llama-tiny").eval()
    fused.load_state_dict(plain.state_dict())
    plain.quantize_weights_()
    assert fused.quantize_weights_(fused=True) is fused
    assert all(b.attention.fused_fp8 and b.feed_forward.fused_fp8 for b in fused.layers)
    assert not any(b.attention.fused_fp8 or b.feed_forward.fused_fp8 for b in plain.layers)
    sd, want = fused.state_dict(), plain.state_dict()
    assert list(sd) == list(want)
    assert all(torch.equal(sd[k].view(torch.uint8) if sd[k].dtype == lf.FP8 else sd[k],
                           want[k].view(torch.uint8) if want[k].dtype == lf.FP8 else want[k]) for k in want)
    tokens = torch.randint(1, plain.cfg.vocab_size, (2, 7), generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        assert torch.equal(fused(tokens), plain(tokens))
    assert torch.equal(fused.generate(tokens, 3), plain.generate(tokens, 3))
