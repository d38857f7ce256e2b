"""FP8 weight-only projections on the CPU: the quantiser, the reference, Fp8Linear and Llama.quantize_weights_."""
import pytest
import torch

from cs744_pytorch_distributed_tutorial_amd.models import llama
from cs744_pytorch_distributed_tutorial_amd.ops import attention, linear_fp8 as lf


def _w(N=24, K=64, seed=0):
    return torch.randn(N, K, generator=torch.Generator().manual_seed(seed)) * torch.exp2(torch.linspace(-12, 4, N))[:, None]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float64])
def test_quantiser_and_reference(dtype):
    w = _w().to(dtype)
    codes, scale = lf.quantize_weight_fp8(w)
    want_codes, want_scale = attention.kv_quantize_ref(w)
    assert codes.dtype == attention.FP8 and codes.shape == w.shape and scale.shape == (24,) and scale.dtype == torch.float32
    assert torch.equal(codes.view(torch.uint8), want_codes.view(torch.uint8)) and torch.equal(scale, want_scale)
    x = torch.randn(2, 5, 64, generator=torch.Generator().manual_seed(1)).to(dtype)
    y = lf.linear_fp8_ref(x, codes, scale)
    ref = x.double() @ (codes.double() * scale.double()[:, None]).T
    eps = {torch.float32: 2.0 ** -24, torch.bfloat16: 2.0 ** -8, torch.float64: 2.0 ** -53}[dtype]
    sums = 64 * (2.0 ** -53 if dtype == torch.float64 else 2.0 ** -24) * (x.double().abs() @ (codes.double().abs() * scale.double()[:, None]).T)
    assert y.dtype == dtype and y.shape == (2, 5, 24)
    assert ((y.double() - ref).abs() <= eps * ref.abs() + sums).all()
    assert torch.equal(lf.linear_fp8(x, codes, scale), y)  # the CPU path of the public entry is the reference


def test_fp8linear_from_linear_and_state_dict():
    lin = torch.nn.Linear(64, 24, bias=False)
    with torch.no_grad():
        lin.weight.copy_(_w(seed=2))
    q = lf.Fp8Linear.from_linear(lin)
    codes, scale = lf.quantize_weight_fp8(lin.weight)
    assert set(q.state_dict()) == {"weight", "weight_scale"} and not list(q.parameters())
    assert torch.equal(q.weight.view(torch.uint8), codes.view(torch.uint8)) and torch.equal(q.weight_scale, scale)
    x = torch.randn(3, 64, generator=torch.Generator().manual_seed(3))
    assert torch.equal(q(x), lf.linear_fp8_ref(x, codes, scale))
    fresh = lf.Fp8Linear(64, 24)
    fresh.load_state_dict(q.state_dict())
    assert torch.equal(fresh.weight.view(torch.uint8), codes.view(torch.uint8)) and torch.equal(fresh(x), q(x))
    with pytest.raises(RuntimeError, match="inference only"):
        q(x.clone().requires_grad_())
    with pytest.raises(ValueError, match="bias-free"):
        lf.Fp8Linear.from_linear(torch.nn.Linear(64, 24))


@pytest.mark.parametrize("head", [True, False])
def test_quantize_weights_replaces_the_projections(head):
    torch.manual_seed(0)
    m = llama.build("llama-tiny").eval()
    before = {k: v.clone() for k, v in m.state_dict().items()}
    assert m.quantize_weights_(head=head) is m
    swapped = {n for n, mod in m.named_modules() if isinstance(mod, lf.Fp8Linear)}
    want = {f"layers.{i}.{p}" for i in range(m.cfg.n_layers)
            for p in ("attention.wq", "attention.wk", "attention.wv", "attention.wo", "feed_forward.w1",
                      "feed_forward.w3", "feed_forward.w2")} | ({"output"} if head else set())
    assert swapped == want and any(isinstance(mod, torch.nn.Linear) for mod in m.modules()) == (not head)
    assert {n for n, _ in m.named_parameters()} == {k for k in before if not any(k.startswith(w + ".") for w in want)}
    assert all(torch.equal(p, before[n]) for n, p in m.named_parameters())  # embeddings, norms (and head) untouched
    tokens = torch.randint(1, m.cfg.vocab_size, (2, 6), generator=torch.Generator().manual_seed(1))
    out = m.generate(tokens, 4)
    assert out.shape == (2, 4) and int(out.min()) >= 0 and int(out.max()) < m.cfg.vocab_size
    with pytest.raises(ValueError, match="fp8"):
        m.quantize_weights_(dtype="int4")
