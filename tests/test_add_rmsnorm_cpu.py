"""The fused residual add + RMSNorm off the GPU: ops.lm.add_rms_norm on CPU tensors is the two-op
reference, Llama.fused_residual computes what the plain blocks compute bit for bit (same ops in
the same order on CPU), and the trainer's fused_residual switch."""
import pytest
import torch

CPU = torch.device("cpu")
ENV = ("CS744_OPTIMIZER", "CS744_LR", "CS744_WEIGHT_DECAY", "CS744_MAX_GRAD_NORM", "CS744_DOC_LEN", "CS744_LOSS_MASK",
       "CS744_Z_LOSS", "CS744_FUSED_HEAD", "CS744_FUSED_RESIDUAL", "CS_LM_HEAD_CHUNK_MB")


@pytest.fixture
def clean_env(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def _trainer(**kw):
    from cs744_pytorch_distributed_tutorial_amd.runtime.torch_trainer import TorchTrainer
    return TorchTrainer("llama-tiny", 4, CPU, seq_len=32, fused_sgd=False, **kw)


# ------------------------------------------------------------------ the op
@pytest.mark.parametrize("shape", [(3, 8), (2, 5, 9)])
def test_cpu_op_is_the_two_op_composition(shape):
    from cs744_pytorch_distributed_tutorial_amd.ops import lm
    g = torch.Generator().manual_seed(0)
    x0, d0 = torch.randn(*shape, generator=g), torch.randn(*shape, generator=g)
    w0 = torch.rand(shape[-1], generator=g) + 0.5
    gh, gy = torch.randn(*shape, generator=g), torch.randn(*shape, generator=g)
    grads = []
    for fused in (True, False):
        x, d, w = (t.clone().requires_grad_() for t in (x0, d0, w0))
        if fused:
            h, y = lm.add_rms_norm(x, d, w, 1e-5)
            rh, ry = lm.add_rms_norm_ref(x0, d0, w0, 1e-5)
            assert torch.equal(h, x0 + d0) and torch.equal(y, lm.rms_norm_ref(x0 + d0, w0, 1e-5))
            assert torch.equal(h, rh) and torch.equal(y, ry)
        else:
            h = x + d
            y = lm.rms_norm_ref(h, w, 1e-5)
        torch.autograd.backward([h, y], [gh, gy])
        grads.append((x.grad, d.grad, w.grad))
    for a, b in zip(*grads):
        assert torch.equal(a, b)


# ------------------------------------------------------------------ the model
def _model_run(fused, doc, with_targets, state=None):
    from cs744_pytorch_distributed_tutorial_amd.models import llama
    from cs744_pytorch_distributed_tutorial_amd.ops import lm
    from cs744_pytorch_distributed_tutorial_amd.ops.attention import doc_ids_from_eos
    torch.manual_seed(0)
    m = llama.build("llama-tiny")
    if state is not None:
        m.load_state_dict(state)
    assert m.fused_residual is False  # off by default
    m.fused_residual = fused
    g = torch.Generator().manual_seed(1)
    tok = torch.randint(0, m.vocab_size - 1, (2, 24), generator=g)
    tok[0, 7] = tok[1, 15] = m.cfg.eos_id
    tgt = torch.randint(0, m.vocab_size, (2, 24), generator=g)
    doc_ids = doc_ids_from_eos(tok, m.cfg.eos_id) if doc else None
    if with_targets:
        loss = m(tok, doc_ids=doc_ids, targets=tgt)
    else:
        logits = m(tok, doc_ids=doc_ids)
        loss = lm.cross_entropy(logits.view(-1, logits.shape[-1]), tgt.view(-1))
    loss.backward()
    return m, loss.detach(), {n: p.grad for n, p in m.named_parameters()}


@pytest.mark.parametrize("with_targets", [False, True], ids=["logits", "targets"])
@pytest.mark.parametrize("doc", [False, True], ids=["nodoc", "doc"])
def test_llama_tiny_fused_residual_bit_equal_on_cpu(doc, with_targets):
    m0, l0, g0 = _model_run(False, doc, with_targets)
    m1, l1, g1 = _model_run(True, doc, with_targets, m0.state_dict())
    assert list(m0.state_dict().keys()) == list(m1.state_dict().keys())
    assert torch.equal(l0, l1) and torch.isfinite(l0)
    assert g0.keys() == g1.keys()
    for n in g0:
        assert g0[n] is not None and torch.equal(g0[n], g1[n]), n


# ------------------------------------------------------------------ the trainer
def test_trainer_fused_residual_argument_and_environment(clean_env):
    assert _trainer().fused_residual is False
    assert _trainer().module.fused_residual is False
    tr = _trainer(fused_residual=True)
    assert tr.fused_residual is True and tr.module.fused_residual is True
    clean_env.setenv("CS744_FUSED_RESIDUAL", "1")
    tr = _trainer()
    assert tr.fused_residual is True and tr.module.fused_residual is True
    tr = _trainer(fused_residual=False)  # the argument wins
    assert tr.fused_residual is False and tr.module.fused_residual is False
    clean_env.setenv("CS744_FUSED_RESIDUAL", "0")
    assert _trainer().fused_residual is False
    from cs744_pytorch_distributed_tutorial_amd.runtime.torch_trainer import TorchTrainer
    with pytest.raises(ValueError, match="fused_residual"):
        TorchTrainer("vgg11", 2, CPU, fused_sgd=False, fused_residual=True)


def test_cpu_three_steps_bit_equal(clean_env):
    outs = []
    for fused in (False, True):
        tr = _trainer(fused_residual=fused)
        p0 = torch.cat([p.detach().reshape(-1) for p in tr.module.parameters()]).clone()
        for _ in range(3):
            tr.step()
        outs.append((tr.loss.clone(), torch.cat([p.detach().reshape(-1) for p in tr.module.parameters()]), p0))
    assert torch.equal(outs[0][2], outs[1][2]) and not torch.equal(outs[0][1], outs[0][2])
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
