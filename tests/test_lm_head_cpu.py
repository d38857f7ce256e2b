"""The chunked LM head off the GPU: ops.lm.linear_cross_entropy_ref (the path every CPU tensor, odd
vocabulary, bias or other dtype takes) against F.linear + F.cross_entropy in float64 autograd,
head_chunk_rows, the trainer's fused_head switch, and fused_head=True training bit for bit like
fused_head=False on CPU, where both run the same ops: one process and a 2-rank gloo DDP world."""
import math

import pytest
import torch
import torch.nn.functional as F

from mp_util import run_world

CPU = torch.device("cpu")
ENV = ("CS744_OPTIMIZER", "CS744_LR", "CS744_WEIGHT_DECAY", "CS744_MAX_GRAD_NORM", "CS744_DOC_LEN", "CS744_LOSS_MASK",
       "CS744_Z_LOSS", "CS744_FUSED_HEAD", "CS_LM_HEAD_CHUNK_MB")


@pytest.fixture
def clean_env(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def _trainer(**kw):
    from cs744_pytorch_distributed_tutorial_amd.runtime.torch_trainer import TorchTrainer
    return TorchTrainer("llama-tiny", 4, CPU, seq_len=32, fused_sgd=False, **kw)


# ------------------------------------------------------------------ the reference path
def _case(seed=0, R=(3, 7), D=16, V=50):
    g = torch.Generator().manual_seed(seed)
    h = torch.randn(*R, D, generator=g)
    head = torch.nn.Linear(D, V, bias=False)
    with torch.no_grad():
        head.weight.copy_(torch.randn(V, D, generator=g) * 0.5)
    t = torch.randint(0, V, R, generator=g)
    return h, head, t


@pytest.mark.parametrize("ignore,z", [(None, 0.0), (-100, 0.0), (7, 0.0), (None, 1e-2), (-100, 0.5)])
def test_ref_against_float64_autograd(ignore, z):
    from cs744_pytorch_distributed_tutorial_amd.ops import lm
    h, head, t = _case()
    if ignore is not None:
        t[0, 1], t[2, 5], t[1, 0] = ignore, ignore, ignore
    h.requires_grad_()
    loss = lm.linear_cross_entropy(h, head, t, ignore_index=ignore, z_loss=z)
    assert loss.dim() == 0 and loss.dtype == torch.float32
    (2.5 * loss).backward()
    h64 = h.detach().double().requires_grad_()
    w64 = head.weight.detach().double().requires_grad_()
    logits = F.linear(h64, w64).view(-1, w64.shape[0])
    tt = t.view(-1)
    nll = F.cross_entropy(logits, tt, ignore_index=-(1 << 40) if ignore is None else ignore, reduction="none")
    valid = torch.ones_like(tt, dtype=torch.bool) if ignore is None else tt != ignore
    lse = torch.logsumexp(logits, -1)
    ref = ((nll + z * lse * lse) * valid).sum() / valid.sum()
    (2.5 * ref).backward()
    assert float(loss.detach()) == pytest.approx(float(ref.detach()), rel=1e-5, abs=1e-6)
    torch.testing.assert_close(h.grad.double(), h64.grad, rtol=1e-4, atol=1e-6)
    torch.testing.assert_close(head.weight.grad.double(), w64.grad, rtol=1e-4, atol=1e-6)
    if ignore is not None:
        assert bool((h.grad[t == ignore] == 0).all())
    # the wrapper took the reference path, and the reference is cross_entropy over the full logits
    l2 = lm.linear_cross_entropy_ref(h.detach(), head, t, ignore, z)
    l3 = lm.cross_entropy(head(h.detach()).view(-1, 50), t.view(-1), ignore, z)
    assert torch.equal(l2, loss.detach()) and torch.equal(l3, loss.detach())


def test_ref_edge_rules():
    from cs744_pytorch_distributed_tutorial_amd.ops import lm
    h, head, t = _case(1)
    h.requires_grad_()
    loss = lm.linear_cross_entropy(h, head, torch.full_like(t, -100), ignore_index=-100, z_loss=0.5)
    loss.backward()
    assert float(loss.detach()) == 0.0 and bool((h.grad == 0).all()) and bool((head.weight.grad == 0).all())
    tb = t.clone()
    tb[1, 1] = 50  # outside [0, V) and not the ignore index: NaN
    assert math.isnan(float(lm.linear_cross_entropy(h, head, tb, ignore_index=-100)))
    for z in (-1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            lm.linear_cross_entropy(h, head, t, z_loss=z)
    nll, n = lm.linear_cross_entropy_sums(h, head, t, ignore_index=int(t[0, 0]))
    valid = t != t[0, 0]
    assert int(n) == int(valid.sum()) and nll.dtype == torch.float64
    ref = F.cross_entropy(head(h).double().view(-1, 50), t.view(-1), reduction="none")[valid.view(-1)].sum()
    assert float(nll) == pytest.approx(float(ref), rel=1e-5)
    hb = torch.nn.Linear(16, 50, bias=True)  # a bias: the reference path applies it
    lb = lm.linear_cross_entropy(h, hb, t)
    assert torch.equal(lb, lm.cross_entropy(hb(h).view(-1, 50), t.view(-1)))


# ------------------------------------------------------------------ head_chunk_rows
def test_head_chunk_rows(clean_env):
    from cs744_pytorch_distributed_tutorial_amd.ops.lm import head_chunk_rows
    # explicit values, clamped to [1, R]
    assert head_chunk_rows(37, 1024, 2, 8) == 8
    assert head_chunk_rows(37, 1024, 2, 37) == 37
    assert head_chunk_rows(37, 1024, 2, 64) == 37
    assert head_chunk_rows(37, 1024, 2, 0) == 1
    assert head_chunk_rows(37, 1024, 2, -5) == 1
    # the default: 1024 MiB of logits, a multiple of 256 rows
    assert head_chunk_rows(16384, 128256, 2) == (1024 << 20) // (128256 * 2) // 256 * 256 == 4096
    assert head_chunk_rows(16384, 128256, 4) == 2048
    assert head_chunk_rows(4096, 32768, 2) == 4096  # one chunk covers every row
    assert head_chunk_rows(100, 1024, 2) == 100  # R smaller than one chunk
    assert head_chunk_rows(16384, 1 << 24, 4) == 256  # never under one GEMM tile of rows
    clean_env.setenv("CS_LM_HEAD_CHUNK_MB", "256")
    assert head_chunk_rows(16384, 128256, 2) == 1024
    clean_env.setenv("CS_LM_HEAD_CHUNK_MB", "128")
    assert head_chunk_rows(16384, 128256, 2) == 512
    assert head_chunk_rows(16384, 128256, 2, 300) == 300  # an explicit value wins
    clean_env.setenv("CS_LM_HEAD_CHUNK_MB", "0")
    with pytest.raises(ValueError):
        head_chunk_rows(16384, 128256, 2)


# ------------------------------------------------------------------ trainer
def test_trainer_fused_head_argument_and_environment(clean_env):
    assert _trainer().fused_head is False
    assert _trainer(fused_head=True).fused_head is True
    clean_env.setenv("CS744_FUSED_HEAD", "1")
    assert _trainer().fused_head is True
    assert _trainer(fused_head=False).fused_head is False  # the argument wins
    clean_env.setenv("CS744_FUSED_HEAD", "0")
    assert _trainer().fused_head is False
    from cs744_pytorch_distributed_tutorial_amd.runtime.torch_trainer import TorchTrainer
    with pytest.raises(ValueError, match="fused_head"):
        TorchTrainer("vgg11", 2, CPU, fused_sgd=False, fused_head=True)


@pytest.mark.parametrize("kw", [dict(), dict(doc_len=8, loss_mask="doc", z_loss=1e-4, optimizer="adamw", lr=1e-3)],
                         ids=["plain", "doc+mask+z+adamw"])
def test_cpu_step_and_evaluate_bit_equal(clean_env, kw):
    outs = []
    for fused in (False, True):
        tr = _trainer(fused_head=fused, **kw)
        tr.step()
        ev = tr.evaluate(1)
        outs.append((tr.loss.clone(), torch.cat([p.detach().reshape(-1) for p in tr.module.parameters()]), ev))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert outs[0][2] == outs[1][2] and outs[0][2]["tokens"] > 0


def _lm_ddp(rank, world, fused):
    from cs744_pytorch_distributed_tutorial_amd.runtime.torch_trainer import TorchTrainer
    torch.set_num_threads(1)
    tr = TorchTrainer("llama-tiny", 4, torch.device("cpu"), rank, world, sync="ddp", comm="torch", bucket_mb=0.5,
                      optimizer="adamw", lr=1e-3, weight_decay=0.1, max_grad_norm=1.0, seq_len=32, fused_sgd=False,
                      doc_len=8, loss_mask="doc", z_loss=1e-4, fused_head=fused)
    p0 = torch.cat([p.detach().reshape(-1) for p in tr.module.parameters()]).clone()
    for _ in range(2):
        tr.step()
    return {"p": torch.cat([p.detach().reshape(-1) for p in tr.module.parameters()]), "p0": p0, "loss": tr.loss}


def test_ddp_world2_bit_equal_to_unfused(clean_env):
    fused, plain = run_world(_lm_ddp, 2, True), run_world(_lm_ddp, 2, False)
    assert torch.equal(fused[0]["p"], fused[1]["p"])
    assert not torch.equal(fused[0]["p"], fused[0]["p0"])
    for r in range(2):
        assert torch.equal(fused[r]["p"], plain[r]["p"]) and torch.equal(fused[r]["loss"], plain[r]["loss"])
