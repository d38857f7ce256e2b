"""QK-norm off the GPU: ops.lm.qk_norm_rope_ref against the composition it fuses and against the float64
oracle (tests/qk_norm_oracle.py), the oracle's hand-written backward against float64 autograd, and the
model / trainer option (LlamaConfig.qk_norm, TorchTrainer(qk_norm=...), CS744_QK_NORM)."""
import pytest
import torch

import qk_norm_oracle as orc
from qk_norm_oracle import CASES, EPS

CPU = torch.device("cpu")
F32, BF16 = torch.float32, torch.bfloat16
ENV = ("CS744_OPTIMIZER", "CS744_LR", "CS744_WEIGHT_DECAY", "CS744_MAX_GRAD_NORM", "CS744_DOC_LEN", "CS744_LOSS_MASK",
       "CS744_Z_LOSS", "CS744_FUSED_HEAD", "CS744_FUSED_RESIDUAL", "CS744_QK_NORM", "CS_LM_HEAD_CHUNK_MB")


@pytest.fixture
def clean_env(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def _trainer(**kw):
    from cs744_pytorch_distributed_tutorial_amd.runtime.torch_trainer import TorchTrainer
    return TorchTrainer("llama-tiny", 2, CPU, seq_len=32, fused_sgd=False, **kw)


def _ref_run(inp):
    """qk_norm_rope through the public op on CPU tensors (the reference path) -> outs, grads"""
    from cs744_pytorch_distributed_tutorial_amd.ops import lm
    q, k, wq, wk, cos, sin, gq, gk = inp
    a = [t.detach().clone().requires_grad_() for t in (q, k, wq, wk)]
    yq, yk = lm.qk_norm_rope(*a, cos, sin, EPS)
    torch.autograd.backward([yq, yk], [gq, gk])
    return (yq.detach(), yk.detach()), tuple(t.grad for t in a)


# ------------------------------------------------------------------ the reference
@pytest.mark.parametrize("case", CASES[:3], ids=str)
def test_ref_is_rms_norm_then_rope(case):
    """fp32, q and k with their own head counts: the composition of the two existing references"""
    from cs744_pytorch_distributed_tutorial_amd.ops import lm
    q, k, wq, wk, cos, sin, _, _ = orc.make_inputs(case, F32, CPU)
    hd = q.shape[-1]
    yq, yk = lm.qk_norm_rope_ref(q, k, wq, wk, cos, sin, EPS)
    for x, w, y in ((q, wq, yq), (k, wk, yk)):
        want = lm.rope_ref(lm.rms_norm_ref(x.view(-1, hd), w, EPS).view_as(x), cos, sin)
        assert y.shape == x.shape and y.dtype == x.dtype
        torch.testing.assert_close(y, want, rtol=1e-6, atol=1e-6)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=str)
def test_ref_meets_the_oracle_bounds(case, dtype):
    inp = orc.make_inputs(case, dtype, CPU)
    outs, grads = _ref_run(inp)
    orc.check_against_oracle(inp, outs, grads, dtype, tag=f"cpu ref {case}")


@pytest.mark.parametrize("case", [CASES[0], CASES[1], CASES[4], CASES[5]], ids=str)
def test_oracle_backward_is_float64_autograd_of_its_forward(case):
    inp = orc.make_inputs(case, F32, CPU)
    q, k, wq, wk, cos, sin, gq, gk = inp
    a = [t.double().requires_grad_() for t in (q, k, wq, wk)]
    yq, yk = orc.forward(*a, cos, sin, EPS)
    assert yq.requires_grad
    torch.autograd.backward([yq, yk], [gq.double(), gk.double()])
    want = orc.backward(*inp, EPS)[:4]
    for got, w in zip((t.grad for t in a), want):
        scale = float(w.abs().max())
        assert float((got - w).abs().max()) <= 1e-10 * max(scale, 1.0)


def test_zero_row_gives_zero_output_and_finite_gradients():
    inp = list(orc.make_inputs(CASES[4], F32, CPU))
    inp[0] = inp[0].clone()
    inp[0][1, 7, 2] = 0.0
    inp[1] = inp[1].clone()
    inp[1][0, 0, 0] = 0.0
    (yq, yk), grads = _ref_run(inp)
    assert float(yq[1, 7, 2].abs().max()) == 0.0 and float(yk[0, 0, 0].abs().max()) == 0.0
    for t in (yq, yk) + grads:
        assert bool(torch.isfinite(t).all())
    orc.check_against_oracle(inp, (yq, yk), grads, F32, tag="cpu zero rows")


# ------------------------------------------------------------------ the model
def _tiny_keys(cfg, qk_norm):
    keys = ["tok_embeddings.weight"]
    for i in range(cfg.n_layers):
        keys += [f"layers.{i}.attention_norm.weight"]
        keys += [f"layers.{i}.attention.{n}.weight" for n in ("wq", "wk", "wv", "wo")]
        if qk_norm:
            keys += [f"layers.{i}.attention.q_norm.weight", f"layers.{i}.attention.k_norm.weight"]
        keys += [f"layers.{i}.ffn_norm.weight"]
        keys += [f"layers.{i}.feed_forward.{n}.weight" for n in ("w1", "w3", "w2")]
    return keys + ["norm.weight", "output.weight"]


def _tiny_params(cfg):
    hd = cfg.dim // cfg.n_heads
    layer = cfg.dim * hd * (2 * cfg.n_heads + 2 * cfg.n_kv_heads) + 3 * cfg.dim * cfg.ffn_dim + 2 * cfg.dim
    return cfg.n_layers * layer + 2 * cfg.vocab_size * cfg.dim + cfg.dim


def test_default_model_is_unchanged():
    from cs744_pytorch_distributed_tutorial_amd.models import llama
    m = llama.build("llama-tiny")
    cfg = m.cfg
    assert cfg.qk_norm is False and llama.LlamaConfig().qk_norm is False
    assert (cfg.dim, cfg.n_layers, cfg.n_heads, cfg.n_kv_heads, cfg.ffn_dim, cfg.vocab_size) == (256, 2, 4, 2, 512, 1024)
    assert list(m.state_dict().keys()) == _tiny_keys(cfg, False)
    assert llama.param_count(cfg) == _tiny_params(cfg) == sum(p.numel() for p in m.parameters())
    assert not hasattr(m.layers[0].attention, "q_norm")


def test_qk_norm_model_adds_exactly_the_gains():
    from cs744_pytorch_distributed_tutorial_amd.models import llama
    torch.manual_seed(0)
    base = llama.build("llama-tiny")
    torch.manual_seed(0)
    m = llama.build("llama-tiny", qk_norm=True)
    cfg = m.cfg
    assert cfg.qk_norm is True and llama.CONFIGS["llama-tiny"].qk_norm is False
    sd = m.state_dict()
    assert list(sd.keys()) == _tiny_keys(cfg, True)
    new = [k for k in sd if k not in base.state_dict()]
    assert len(new) == 2 * cfg.n_layers
    for k in new:
        assert k.endswith(("q_norm.weight", "k_norm.weight"))
        assert tuple(sd[k].shape) == (64,) and bool((sd[k] == 1).all())
    for k, v in base.state_dict().items():  # the gains draw nothing from the generator
        assert torch.equal(sd[k], v), k
    n = _tiny_params(cfg) + cfg.n_layers * 2 * 64
    assert llama.param_count(cfg) == n == sum(p.numel() for p in m.parameters())


# ------------------------------------------------------------------ the trainer
@pytest.mark.parametrize("doc_len", [None, 32])
def test_cpu_trainer_step_with_qk_norm(clean_env, doc_len):
    tr = _trainer(qk_norm=True, doc_len=doc_len)
    assert tr.qk_norm is True and tr.module.cfg.qk_norm is True
    tr.step()
    assert bool(torch.isfinite(tr.loss))
    for blk in tr.module.layers:
        for norm in (blk.attention.q_norm, blk.attention.k_norm):
            assert norm.weight.grad is not None and float(norm.weight.grad.abs().sum()) > 0


def test_trainer_argument_and_environment(clean_env):
    from cs744_pytorch_distributed_tutorial_amd.runtime.torch_trainer import TorchTrainer
    tr = _trainer()
    assert tr.qk_norm is False and tr.module.cfg.qk_norm is False
    clean_env.setenv("CS744_QK_NORM", "1")
    tr = _trainer()
    assert tr.qk_norm is True and hasattr(tr.module.layers[0].attention, "q_norm")
    assert _trainer(qk_norm=False).qk_norm is False  # the argument wins
    clean_env.setenv("CS744_QK_NORM", "0")
    assert _trainer().qk_norm is False
    clean_env.delenv("CS744_QK_NORM")
    with pytest.raises(ValueError, match="qk_norm"):
        TorchTrainer("vgg11", 2, CPU, fused_sgd=False, qk_norm=True)
