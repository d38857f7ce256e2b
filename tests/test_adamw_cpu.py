"""AdamW on the autograd-path trainer without a GPU: the trainer's optimizer switch (argument and
``CS744_OPTIMIZER``), the two parameter groups, ``FusedAdamW``'s CPU path against
``clip_grad_norm_`` + ``torch.optim.AdamW`` (bitwise), and 2-rank gloo DDP replicas staying bitwise
equal under clipped AdamW."""
import pytest
import torch

from mp_util import run_world

CPU = torch.device("cpu")
ENV = ("CS744_OPTIMIZER", "CS744_LR", "CS744_WEIGHT_DECAY", "CS744_MAX_GRAD_NORM")


@pytest.fixture
def clean_env(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def _trainer(**kw):
    from cs744_pytorch_distributed_tutorial_amd.runtime.torch_trainer import TorchTrainer
    return TorchTrainer("llama-tiny", 4, CPU, seq_len=32, fused_sgd=False, **kw)


def _check_adamw(tr, lr, wd):
    assert type(tr.opt) is torch.optim.AdamW
    groups = tr.opt.param_groups
    assert len(groups) == 2
    assert all(p.dim() >= 2 for p in groups[0]["params"]) and groups[0]["weight_decay"] == wd
    assert all(p.dim() < 2 for p in groups[1]["params"]) and groups[1]["weight_decay"] == 0
    assert len(groups[1]["params"]) > 0  # the RMSNorm weights
    assert sum(len(g["params"]) for g in groups) == len(list(tr.module.parameters()))
    assert all(g["lr"] == lr and g["betas"] == (0.9, 0.95) for g in groups)


def test_trainer_adamw_argument(clean_env):
    tr = _trainer(optimizer="adamw", lr=1e-3, weight_decay=0.1, max_grad_norm=1.0)
    _check_adamw(tr, 1e-3, 0.1)
    assert tr.clip_norm == 1.0
    p0 = [p.detach().clone() for p in tr.module.parameters()]
    losses = []
    for _ in range(3):
        tr.step()
        losses.append(tr.last_loss())
    assert all(torch.isfinite(torch.tensor(losses)))
    assert all(not torch.equal(a, b) for a, b in zip(p0, tr.module.parameters()))
    assert all(int(tr.opt.state[p]["step"]) == 3 for p in tr.module.parameters())


def test_trainer_adamw_from_environment(clean_env):
    clean_env.setenv("CS744_OPTIMIZER", "adamw")
    clean_env.setenv("CS744_LR", "3e-4")
    clean_env.setenv("CS744_WEIGHT_DECAY", "0.1")
    clean_env.setenv("CS744_MAX_GRAD_NORM", "1")
    tr = _trainer()
    _check_adamw(tr, 3e-4, 0.1)
    assert tr.clip_norm == 1.0
    tr.step()
    # an explicit argument wins over the environment, hyper-parameters included
    tr = _trainer(optimizer="sgd")
    assert type(tr.opt) is torch.optim.SGD and tr.opt.param_groups[0]["lr"] == 0.1 and tr.clip_norm is None


def test_trainer_unknown_optimizer_raises(clean_env):
    with pytest.raises(ValueError):
        _trainer(optimizer="lion")
    clean_env.setenv("CS744_OPTIMIZER", "adam")
    with pytest.raises(ValueError):
        _trainer()


def test_trainer_default_is_sgd_as_before(clean_env):
    # the hyper-parameter variables alone change nothing: they count only beside CS744_OPTIMIZER
    clean_env.setenv("CS744_LR", "3e-4")
    clean_env.setenv("CS744_MAX_GRAD_NORM", "1")
    tr = _trainer()
    assert type(tr.opt) is torch.optim.SGD
    assert len(tr.opt.param_groups) == 1
    g = tr.opt.param_groups[0]
    assert g["lr"] == 0.1 and g["momentum"] == 0.9 and g["weight_decay"] == 1e-4
    assert tr.clip_norm is None and tr.optimizer == "sgd"


def _model_and_grads(seed):
    torch.manual_seed(seed)
    m = torch.nn.Sequential(torch.nn.Linear(33, 17), torch.nn.LayerNorm(17), torch.nn.Linear(17, 5))
    gen = torch.Generator().manual_seed(seed + 1)
    grads = [[torch.randn(p.shape, generator=gen) * 3 for p in m.parameters()] for _ in range(3)]
    return m, grads


@pytest.mark.parametrize("max_norm,scale", [(None, 1.0), (1.0, 1.0), (1.0, 0.5)])
def test_fused_adamw_cpu_equals_torch_bitwise(max_norm, scale):
    from cs744_pytorch_distributed_tutorial_amd.ops.optim import FusedAdamW
    a, grads = _model_and_grads(7)
    b, _ = _model_and_grads(7)

    def groups(m):
        ps = list(m.parameters())
        return [{"params": [p for p in ps if p.dim() >= 2], "weight_decay": 0.1},
                {"params": [p for p in ps if p.dim() < 2], "weight_decay": 0.0}]
    oa = FusedAdamW(groups(a), lr=1e-2, betas=(0.9, 0.95), max_grad_norm=max_norm, grad_scale=scale)
    ob = torch.optim.AdamW(groups(b), lr=1e-2, betas=(0.9, 0.95))
    assert oa.last_grad_norm() is None
    for gs in grads:
        for m in (a, b):
            for p, g in zip(m.parameters(), gs):
                p.grad = g.clone()
        oa.step()
        if scale != 1.0:
            for p in b.parameters():
                p.grad.mul_(scale)
        norm = torch.nn.utils.clip_grad_norm_(list(b.parameters()), max_norm) if max_norm is not None else None
        ob.step()
        if norm is None:
            assert oa.last_grad_norm() is None
        else:
            assert torch.equal(oa.last_grad_norm(), norm)
    for p, q in zip(a.parameters(), b.parameters()):
        assert torch.equal(p, q)
    # torch's state, both ways
    sa, sb = oa.state_dict(), ob.state_dict()
    assert set(sa["state"][0]) == {"step", "exp_avg", "exp_avg_sq"} and torch.is_tensor(sa["state"][0]["step"])
    ob.load_state_dict(sa)
    oa.load_state_dict(sb)


@pytest.mark.parametrize("opt", ["amsgrad", "maximize", "capturable"])
def test_fused_adamw_refuses(opt):
    from cs744_pytorch_distributed_tutorial_amd.ops.optim import FusedAdamW
    with pytest.raises(ValueError):
        FusedAdamW([torch.nn.Parameter(torch.zeros(3))], **{opt: True})


def _lm_ddp_adamw(rank, world):
    from cs744_pytorch_distributed_tutorial_amd.runtime.torch_trainer import TorchTrainer
    torch.set_num_threads(1)
    tr = TorchTrainer("llama-tiny", 4, torch.device("cpu"), rank, world, sync="ddp", comm="torch", bucket_mb=0.5,
                      optimizer="adamw", lr=1e-3, weight_decay=0.1, max_grad_norm=1.0, seq_len=32, fused_sgd=False)
    p0 = torch.cat([p.detach().reshape(-1) for p in tr.module.parameters()]).clone()
    for _ in range(3):
        tr.step()
    return {"p": torch.cat([p.detach().reshape(-1) for p in tr.module.parameters()]), "p0": p0}


@pytest.mark.slow
def test_lm_ddp_adamw_replicas_identical(clean_env):
    outs = run_world(_lm_ddp_adamw, 2)
    assert torch.equal(outs[0]["p"], outs[1]["p"])
    assert not torch.equal(outs[0]["p"], outs[0]["p0"])
