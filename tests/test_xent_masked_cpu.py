"""The torch side of the masked, z-regularised cross-entropy on CPU tensors: ops.lm.cross_entropy_ref
against F.cross_entropy and against autograd of the formula in float64, its edge rules (every row
ignored -> 0, an out-of-range target -> NaN), the float64 oracle of tests/test_xent_masked_gpu.py
against it, mask_boundary_targets on hand-written rows, cross_entropy_sums, and the trainer's
loss_mask / z_loss / evaluate() with llama-tiny."""
import math

import pytest
import torch
import torch.nn.functional as F

import test_xent_masked_gpu as xm

CPU = torch.device("cpu")
REF_TOL = dict(rtol=1e-4, atol=1e-5)  # fp32 rounding of the reference itself
ENV = ("CS744_OPTIMIZER", "CS744_LR", "CS744_WEIGHT_DECAY", "CS744_MAX_GRAD_NORM", "CS744_GRAD_COMM_DTYPE",
       "CS744_DOC_LEN", "CS744_LOSS_MASK", "CS744_Z_LOSS")


def _inputs(R, V, dtype=torch.float32, seed=0):
    g_ = torch.Generator(device="cpu").manual_seed(seed + R * 1009 + V)
    x = (torch.randn(R, V, generator=g_) * 3).to(dtype)
    t = torch.randint(0, V, (R,), generator=g_)
    return x, t


def _ref(x, t, ignore, z, g=1.0):
    from cs744_pytorch_distributed_tutorial_amd.ops import lm
    xa = x.clone().requires_grad_()
    mean = lm.cross_entropy_ref(xa, t, ignore, z)
    (g * mean).backward()
    return mean.detach(), xa.grad


@pytest.mark.parametrize("ignore", [-100, 3, None])
@pytest.mark.parametrize("R,V", [(5, 8), (7, 1001), (9, 1024)])
def test_ref_against_torch(R, V, ignore):
    x, t = _inputs(R, V)
    if ignore is not None:
        t[1::3] = ignore
    assert ignore is None or int((t != ignore).sum()) >= 1
    mean, grad = _ref(x, t, ignore, 0.0, 2.5)
    xd = x.double().requires_grad_()
    want = F.cross_entropy(xd, t, ignore_index=-100 if ignore is None else ignore)
    (2.5 * want).backward()
    torch.testing.assert_close(mean.double(), want.detach(), **REF_TOL)
    torch.testing.assert_close(grad.double(), xd.grad, **REF_TOL)


@pytest.mark.parametrize("z", [1e-4, 0.5])
@pytest.mark.parametrize("ignore", [-100, 3, None])
def test_ref_z_loss_against_float64_autograd(ignore, z):
    R, V = 9, 1024
    x, t = _inputs(R, V, seed=1)
    if ignore is not None:
        t[::2] = ignore
    valid = torch.ones(R, dtype=torch.bool) if ignore is None else t != ignore
    mean, grad = _ref(x, t, ignore, z, 2.5)
    xd = x.double().requires_grad_()
    lse = torch.logsumexp(xd, -1)
    rows = lse - xd.gather(1, t.clamp(0, V - 1)[:, None])[:, 0] + z * lse ** 2
    want = rows[valid].sum() / int(valid.sum())
    (2.5 * want).backward()
    k = 1 + 2 * z * float(lse.detach().abs().max())
    torch.testing.assert_close(mean.double(), want.detach(), rtol=1e-4 * k, atol=1e-5 * k)
    torch.testing.assert_close(grad.double(), xd.grad, rtol=1e-4 * k, atol=1e-5 * k)
    assert bool((grad[~valid] == 0).all())


@pytest.mark.parametrize("z", [0.0, 0.5])
def test_ref_edge_rules(z):
    from cs744_pytorch_distributed_tutorial_amd.ops import lm
    x, t = _inputs(3, 16)
    for ignore in (-100, 5):
        mean, grad = _ref(x, torch.full((3,), ignore), ignore, z)
        assert float(mean) == 0.0 and bool((grad == 0).all())
    # ignored rows may hold anything
    xb = x.clone()
    xb[1] = float("nan")
    tb = t.clone()
    tb[1] = -100
    m0, g0 = _ref(x, tb, -100, z)
    m1, g1 = _ref(xb, tb, -100, z)
    assert torch.equal(m0, m1) and torch.equal(g0, g1) and bool((g1[1] == 0).all())
    for bad in (16, -1):
        tb = t.clone()
        tb[0], tb[2] = -100, bad
        mean, grad = _ref(x, tb, -100, z)
        assert math.isnan(float(mean)) and bool(torch.isfinite(grad).all()) and bool((grad[0] == 0).all())
    # -100 is a target like any other unless it is named as the ignore index
    tb = t.clone()
    tb[0] = -100
    assert math.isnan(float(lm.cross_entropy_ref(x, tb, None, z)))
    if z > 0:  # (z = 0 without an ignore index is the unmasked path: F.cross_entropy on CPU, as before)
        assert math.isnan(float(lm.cross_entropy(x, tb, z_loss=z)))
    with pytest.raises(ValueError):
        lm.cross_entropy(x, t, z_loss=-1.0)


def test_default_arguments_take_the_unmasked_path():
    """ignore_index=None, z_loss=0: F.cross_entropy on CPU as before, bit for bit"""
    from cs744_pytorch_distributed_tutorial_amd.ops import lm
    x, t = _inputs(7, 1001)
    assert torch.equal(lm.cross_entropy(x, t), F.cross_entropy(x.float(), t))
    assert torch.equal(lm.cross_entropy(x, t, None, 0.0), F.cross_entropy(x.float(), t))


@pytest.mark.parametrize("z", xm.ZS)
@pytest.mark.parametrize("pattern", xm.PATTERNS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_oracle_against_ref(dtype, pattern, z):
    R, V = 7, 1024
    x, t0 = _inputs(R, V, dtype, seed=2)
    for ignore in (-100, int(t0[R // 2])):
        t = xm._masked_targets(t0, V, pattern, ignore)
        loss, lse, d, mean, n = xm.xent_masked_oracle(x, t, ignore, z, 2.5)
        assert n == int((t != ignore).sum())
        rmean, rgrad = _ref(x.float(), t, ignore, z, 2.5)
        k = 1 + 2 * z * float(lse.abs().max())
        torch.testing.assert_close(mean, rmean.double(), rtol=1e-4 * k, atol=1e-5 * k)
        torch.testing.assert_close(d, rgrad.double(), rtol=1e-4 * k, atol=1e-5 * k)
        ign = t == ignore
        assert bool((loss[ign] == 0).all()) and bool((lse[ign] == 0).all()) and bool((d[ign] == 0).all())
    # with nothing ignored and z = 0 it is the unmasked oracle of tests/test_lm_edges_gpu.py
    loss, lse, d, mean, n = xm.xent_masked_oracle(x, t0, None, 0.0, 2.5)
    uloss, ulse, ud = xm.xent_oracle(x, t0, 2.5)
    assert n == R and torch.equal(loss, uloss) and torch.equal(lse, ulse)
    torch.testing.assert_close(d, ud, rtol=1e-14, atol=0)


def test_oracle_edge_rules():
    x, t = _inputs(4, 16)
    t[0], t[1], t[2] = -100, 16, -1
    loss, lse, d, mean, n = xm.xent_masked_oracle(x, t, -100, 0.5, 1.0)
    assert n == 3 and math.isnan(float(mean))
    assert torch.isnan(loss).tolist() == [False, True, True, False] and float(loss[0]) == 0
    assert bool(torch.isfinite(d).all()) and bool((d[0] == 0).all())
    _, _, d, mean, n = xm.xent_masked_oracle(x, torch.full((4,), 7), 7, 0.5, 1.0)
    assert n == 0 and float(mean) == 0 and bool((d == 0).all())


def test_mask_boundary_targets():
    from cs744_pytorch_distributed_tutorial_amd.ops import lm
    from cs744_pytorch_distributed_tutorial_amd.ops.attention import doc_ids_from_eos
    E = 9
    x = torch.tensor([[E, 1, 2, 3, 4, 5],    # EOS at the first position
                      [1, 2, 3, 4, 5, E],    # at the last
                      [1, E, E, 2, E, 3],    # adjacent ones
                      [1, 2, 3, 4, 5, 6]])   # none
    y = torch.tensor([[1, 2, 3, 4, 5, 6],
                      [2, 3, 4, 5, E, 7],
                      [E, E, 2, E, 3, 4],
                      [2, 3, 4, 5, 6, 7]])
    want = torch.tensor([[-100, 2, 3, 4, 5, 6],
                         [2, 3, 4, 5, E, -100],
                         [E, -100, -100, E, -100, 4],
                         [2, 3, 4, 5, 6, 7]])
    got = lm.mask_boundary_targets(x, y, E)
    assert torch.equal(got, want) and got is not y and y[0, 0] == 1
    assert torch.equal(lm.mask_boundary_targets(x, y, E, ignore_index=-1), want.masked_fill(want == -100, -1))
    # what is masked is exactly the targets that belong to another document than their input: with
    # y[i] = x[i + 1], the positions where the document index of doc_ids_from_eos steps up
    full = torch.cat([x, y[:, -1:]], 1)
    ids = doc_ids_from_eos(full, E)
    assert torch.equal(got == -100, ids[:, 1:] != ids[:, :-1])


@pytest.mark.parametrize("ignore", [-100, None])
def test_cross_entropy_sums_torch_path(ignore):
    from cs744_pytorch_distributed_tutorial_amd.ops import lm
    R, V = 9, 1001
    x, t = _inputs(R, V, seed=3)
    if ignore is not None:
        t[::4] = ignore
    xa = x.clone().requires_grad_()
    nll, n = lm.cross_entropy_sums(xa, t, ignore_index=ignore)
    assert not nll.requires_grad and nll.dtype == torch.float64 and n.dtype == torch.int64 and nll.dim() == 0
    valid = torch.ones(R, dtype=torch.bool) if ignore is None else t != ignore
    assert int(n) == int(valid.sum())
    want = F.cross_entropy(x.double()[valid], t[valid], reduction="sum")
    torch.testing.assert_close(nll, want, **REF_TOL)
    nll, n = lm.cross_entropy_sums(x, torch.full((R,), -100), ignore_index=-100)
    assert float(nll) == 0.0 and int(n) == 0


def _trainer(monkeypatch, model="llama-tiny", **kw):
    from cs744_pytorch_distributed_tutorial_amd.runtime.torch_trainer import TorchTrainer
    args = dict(batch_size=2, device=CPU, optimizer="adamw", lr=3e-4, weight_decay=0.1, fused_sgd=False, seq_len=64)
    args.update(kw)
    return TorchTrainer(model, **args)


def test_trainer_arguments(monkeypatch):
    for key in ENV:
        monkeypatch.delenv(key, raising=False)
    with pytest.raises(ValueError, match="doc_len"):
        _trainer(monkeypatch, loss_mask="doc")
    with pytest.raises(ValueError, match="loss_mask"):
        _trainer(monkeypatch, loss_mask="eos", doc_len=16)
    with pytest.raises(ValueError, match="z_loss"):
        _trainer(monkeypatch, z_loss=-1.0)
    for kw in (dict(loss_mask="doc"), dict(z_loss=1e-4)):
        with pytest.raises(ValueError, match="LM"):
            _trainer(monkeypatch, model="vgg11", seq_len=0, optimizer="sgd", **kw)
    tr = _trainer(monkeypatch)
    assert tr.loss_mask is None and tr.z_loss == 0.0
    # the environment counts only where the argument is None
    monkeypatch.setenv("CS744_LOSS_MASK", "doc")
    monkeypatch.setenv("CS744_Z_LOSS", "1e-3")
    tr = _trainer(monkeypatch, doc_len=16)
    assert tr.loss_mask == "doc" and tr.z_loss == 1e-3
    tr = _trainer(monkeypatch, doc_len=16, z_loss=0.0)
    assert tr.loss_mask == "doc" and tr.z_loss == 0.0
    tr = _trainer(monkeypatch, doc_len=16, z_loss=0.25)
    assert tr.z_loss == 0.25
    with pytest.raises(ValueError, match="doc_len"):
        _trainer(monkeypatch)  # CS744_LOSS_MASK=doc without a doc_len
    monkeypatch.setenv("CS744_LOSS_MASK", "eos")
    with pytest.raises(ValueError, match="loss_mask"):
        _trainer(monkeypatch, doc_len=16)
    tr = _trainer(monkeypatch, doc_len=16, loss_mask="doc")
    assert tr.loss_mask == "doc"


def test_trainer_step_and_evaluate(monkeypatch):
    for key in ENV:
        monkeypatch.delenv(key, raising=False)
    tr = _trainer(monkeypatch, doc_len=16, loss_mask="doc", z_loss=1e-4)
    assert tr.tokens_per_step() == 2 * 64
    tr.step()
    assert math.isfinite(tr.last_loss())
    state = tr.data.gen.get_state()
    ev = tr.evaluate(1)
    tr.data.gen.set_state(state)
    x, _ = tr.data.next()
    assert ev["tokens"] == int((x != tr.eos_id).sum()) and 0 < ev["tokens"] < 2 * 64
    assert math.isfinite(ev["nll"]) and ev["ppl"] == pytest.approx(math.exp(ev["nll"]))
    assert tr.net.training
    # without a mask every token counts, and the z-free nll is what plain cross-entropy gives
    tr = _trainer(monkeypatch)
    assert tr.evaluate(2)["tokens"] == 2 * 2 * 64
