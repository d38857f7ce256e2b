"""QK-norm fused with RoPE on the GPU (qk_norm_rope_fwd / qk_norm_rope_bwd, ops.lm.qk_norm_rope) against the
float64 oracle of tests/qk_norm_oracle.py with its derived bounds, the launch's partition into row blocks and
into the q and k segments, positions, determinism, the host checks, and the model / trainer option (MI355X only)."""
import pytest
import torch

import qk_norm_oracle as orc
from qk_norm_oracle import CASES, EPS

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
DTYPES = pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
HOLES = (2, 33, 4, 2, 64, 1.0)
ENV = ("CS744_OPTIMIZER", "CS744_LR", "CS744_WEIGHT_DECAY", "CS744_MAX_GRAD_NORM", "CS744_GRAD_COMM_DTYPE",
       "CS744_DOC_LEN", "CS744_LOSS_MASK", "CS744_Z_LOSS", "CS744_FUSED_HEAD", "CS744_FUSED_RESIDUAL",
       "CS744_QK_NORM", "CS_LM_HEAD_CHUNK_MB")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cs744_pytorch_distributed_tutorial_amd.ops import native
    native.C()
    return torch.device("cuda", 0)


@pytest.fixture
def clean_env(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def _C():
    from cs744_pytorch_distributed_tutorial_amd import _C
    return _C


def _op_run(inp, need=(True, True, True, True), grads_in=None):
    """ops.lm.qk_norm_rope forward and backward -> (q', k'), (dq, dk, dwq, dwk)"""
    from cs744_pytorch_distributed_tutorial_amd.ops import lm
    q, k, wq, wk, cos, sin, gq, gk = inp
    # detach, not clone: an offset view stays the view it is
    a = [t.detach().requires_grad_(n) for t, n in zip((q, k, wq, wk), need)]
    yq, yk = lm.qk_norm_rope(*a, cos, sin, EPS)
    torch.autograd.backward([yq, yk], [gq, gk] if grads_in is None else grads_in)
    return (yq.detach(), yk.detach()), tuple(t.grad for t in a)


def _no_ref(monkeypatch):
    """the native path must run: the reference raises"""
    from cs744_pytorch_distributed_tutorial_amd.ops import lm

    def boom(*a, **kw):
        raise AssertionError("qk_norm_rope fell back to the reference")
    monkeypatch.setattr(lm, "qk_norm_rope_ref", boom)


# ------------------------------------------------------------------ forward and backward against the oracle
@DTYPES
@pytest.mark.parametrize("case", CASES, ids=str)
def test_op_against_oracle(dev, monkeypatch, case, dtype):
    _no_ref(monkeypatch)
    inp = orc.make_inputs(case, dtype, dev)
    outs, grads = _op_run(inp)
    orc.check_against_oracle(inp, outs, grads, dtype, tag=f"op {case}")


@DTYPES
@pytest.mark.parametrize("case", CASES, ids=str)
def test_bindings_against_oracle(dev, case, dtype):
    inp = orc.make_inputs(case, dtype, dev)
    q, k, wq, wk, cos, sin, gq, gk = inp
    outs = _C().qk_norm_rope_fwd(q, k, wq, wk, cos, sin, EPS)
    grads = _C().qk_norm_rope_bwd(q, k, wq, wk, cos, sin, gq, gk, EPS)
    assert len(outs) == 2 and len(grads) == 4
    orc.check_against_oracle(inp, outs, grads, dtype, tag=f"binding {case}")


@DTYPES
def test_bindings_past_the_grid_cap(dev, dtype):
    """more q rows than kQKMaxBlocks blocks hold at once: the last rows are reached by the grid's stride"""
    C = _C()
    rpb, cap = C.qk_norm_rope_rows_per_block(64), C.qk_norm_rope_max_blocks()
    assert rpb == 2 * C.qk_norm_rope_rows_per_block(128) > 0 and C.qk_norm_rope_rows_per_block(32) == 0
    Hq = 8
    S = (cap * rpb) // Hq + 4  # 32 q rows past the cap; k (Hkv = 1) lies wholly in the second trip
    case = (1, S, Hq, 1, 64, 1.0)
    assert S * Hq > cap * rpb and S * Hq * 64 * 4 < 16 << 20
    inp = orc.make_inputs(case, dtype, dev)
    q, k, wq, wk, cos, sin, gq, gk = inp
    outs = C.qk_norm_rope_fwd(q, k, wq, wk, cos, sin, EPS)
    grads = C.qk_norm_rope_bwd(q, k, wq, wk, cos, sin, gq, gk, EPS)
    orc.check_against_oracle(inp, outs, grads[:2], dtype, tag=f"cap {case}")  # y and dx only: > MAX_ROWS rows
    assert bool(torch.isfinite(grads[2]).all()) and bool(torch.isfinite(grads[3]).all())


# ------------------------------------------------------------------ partition holes
def _hole_rows(dev):
    """(projection, head-row) of the hot rows: the ends of each segment and both sides of the first block
    boundary inside each (the k segment starts at launch row nq, in the middle of a block)"""
    B, S, Hq, Hkv, hd, _ = HOLES
    rpb = _C().qk_norm_rope_rows_per_block(hd)
    nq, nk = B * S * Hq, B * S * Hkv
    kb = rpb - nq % rpb  # first k row that opens a block
    assert 0 < kb < nk and rpb < nq
    return [("q", 0), ("q", nq - 1), ("k", 0), ("k", nk - 1), ("q", rpb - 1), ("q", rpb), ("k", kb - 1), ("k", kb)]


@pytest.mark.parametrize("i", range(8))
def test_partition_holes(dev, i):
    """one hot head-row of incoming gradient: nothing leaks into another row or the other projection"""
    proj, row = _hole_rows(dev)[i]
    inp = orc.make_inputs(HOLES, BF16, dev)
    q, k, wq, wk, cos, sin, gq, gk = inp
    hd = q.shape[-1]
    hq, hk = torch.zeros_like(gq), torch.zeros_like(gk)
    hot, src = (hq, gq) if proj == "q" else (hk, gk)
    hot.view(-1, hd)[row] = src.view(-1, hd)[row]
    dq, dk, dwq, dwk = _C().qk_norm_rope_bwd(q, k, wq, wk, cos, sin, hq, hk, EPS)
    want = orc.backward(q, k, wq, wk, cos, sin, hq, hk, EPS)
    dx, dx_other = (dq, dk) if proj == "q" else (dk, dq)
    dw, dw_other = (dwq, dwk) if proj == "q" else (dwk, dwq)
    t, tabs = (want[2], want[4]) if proj == "q" else (want[3], want[5])  # the hot row's t: every other row's is 0
    mask = torch.ones(dx.numel() // hd, dtype=torch.bool, device=dev)
    mask[row] = False
    assert float(dx.view(-1, hd)[mask].abs().max()) == 0.0
    assert float(dx_other.abs().max()) == 0.0 and float(dw_other.abs().max()) == 0.0
    assert float(dx.view(-1, hd)[row].abs().max()) > 0.0
    assert orc.row_err(dx, want[0] if proj == "q" else want[1]) <= orc.ROW_TOL[BF16]
    err = (dw.double().cpu() - t).abs()
    print(f"[qk-norm] hole {proj}{row}: max |dw - t| / |t| = {float((err / tabs.clamp_min(1e-300)).max()):.3e}")
    assert bool((err <= 1e-5 * tabs).all())


# ------------------------------------------------------------------ positions
@pytest.mark.parametrize("hd", [64, 128])
def test_positions_follow_the_projections_own_head_count(dev, hd):
    C = _C()
    q, k, wq, wk, cos, sin, _, _ = orc.make_inputs((2, 33, 4, 2, hd, 1.0), BF16, dev)
    yq, yk = C.qk_norm_rope_fwd(q, k, wq, wk, cos, sin, EPS)
    # batch 1 alone starts again at s = 0
    yq1, yk1 = C.qk_norm_rope_fwd(q[1:].contiguous(), k[1:].contiguous(), wq, wk, cos, sin, EPS)
    assert torch.equal(yq[1:], yq1) and torch.equal(yk[1:], yk1)
    # another Hkv moves the k segment, not q's positions; each k head keeps its own
    yq2, yk2 = C.qk_norm_rope_fwd(q, k[:, :, :1].contiguous(), wq, wk, cos, sin, EPS)
    assert torch.equal(yq2, yq) and torch.equal(yk2, yk[:, :, :1])
    k4 = torch.cat([k, k], 2).contiguous()
    yq3, yk3 = C.qk_norm_rope_fwd(q, k4, wq, wk, cos, sin, EPS)
    assert torch.equal(yq3, yq) and torch.equal(yk3[:, :, :2], yk) and torch.equal(yk3[:, :, 2:], yk)


# ------------------------------------------------------------------ other checks
@DTYPES
def test_backward_is_deterministic(dev, dtype):
    q, k, wq, wk, cos, sin, gq, gk = orc.make_inputs(CASES[0], dtype, dev)
    a = _C().qk_norm_rope_bwd(q, k, wq, wk, cos, sin, gq, gk, EPS)
    b = _C().qk_norm_rope_bwd(q, k, wq, wk, cos, sin, gq, gk, EPS)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


@DTYPES
def test_zero_rows(dev, monkeypatch, dtype):
    _no_ref(monkeypatch)
    inp = list(orc.make_inputs(CASES[4], dtype, dev))
    inp[0] = inp[0].clone()
    inp[0][1, 7, 2] = 0.0
    inp[0][0, 0, 0] = 0.0
    inp[1] = inp[1].clone()
    inp[1][1, 32, 1] = 0.0
    (yq, yk), grads = _op_run(inp)
    assert float(yq[1, 7, 2].abs().max()) == 0.0 and float(yq[0, 0, 0].abs().max()) == 0.0
    assert float(yk[1, 32, 1].abs().max()) == 0.0
    for t in (yq, yk) + grads:
        assert bool(torch.isfinite(t).all())
    orc.check_against_oracle(inp, (yq, yk), grads, dtype, tag="zero rows")


@DTYPES
def test_odd_offset_views(dev, monkeypatch, dtype):
    """contiguous views one element into their storage: the op re-materialises them (bitwise the aligned
    result), the binding refuses the pointer"""
    _no_ref(monkeypatch)
    inp = orc.make_inputs(CASES[4], dtype, dev)

    def off(t):
        buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
        v = buf[1:].view(t.shape)
        v.copy_(t)
        assert v.is_contiguous() and v.data_ptr() % 16 != 0
        return v

    outs, grads = _op_run(inp)
    shifted = tuple(off(t) for t in inp)
    outs2, grads2 = _op_run(shifted)
    for a, b in zip(outs + grads, outs2 + grads2):
        assert torch.equal(a, b)
    q, k, wq, wk, cos, sin, gq, gk = inp
    for j in range(6):
        args = [q, k, wq, wk, cos, sin]
        args[j] = shifted[j]
        with pytest.raises(RuntimeError, match="16-byte aligned"):
            _C().qk_norm_rope_fwd(*args, EPS)
    for j in (6, 7):
        args = list(inp)
        args[j] = shifted[j]
        with pytest.raises(RuntimeError, match="16-byte aligned"):
            _C().qk_norm_rope_bwd(*args, EPS)
    torch.cuda.synchronize()


def test_host_checks(dev):
    C = _C()
    q, k, wq, wk, cos, sin, gq, gk = orc.make_inputs(CASES[4], F32, dev)
    B, S, Hq, hd = q.shape

    def fwd(**kw):
        a = dict(q=q, k=k, wq=wq, wk=wk, cos=cos, sin=sin)
        a.update(kw)
        return C.qk_norm_rope_fwd(a["q"], a["k"], a["wq"], a["wk"], a["cos"], a["sin"], EPS)

    def bwd(**kw):
        a = dict(q=q, k=k, wq=wq, wk=wk, cos=cos, sin=sin, gq=gq, gk=gk)
        a.update(kw)
        return C.qk_norm_rope_bwd(a["q"], a["k"], a["wq"], a["wk"], a["cos"], a["sin"], a["gq"], a["gk"], EPS)

    for name in ("q", "k", "wq", "wk", "cos", "sin"):  # one device
        with pytest.raises(RuntimeError, match="GPU tensor"):
            fwd(**{name: dict(q=q, k=k, wq=wq, wk=wk, cos=cos, sin=sin)[name].cpu()})
    with pytest.raises(RuntimeError, match="GPU tensor"):
        bwd(gq=gq.cpu())
    with pytest.raises(RuntimeError, match="contiguous"):
        fwd(q=q.transpose(1, 2).contiguous().transpose(1, 2))
    with pytest.raises(RuntimeError, match="contiguous"):
        fwd(cos=torch.cat([cos, cos], 1)[:, ::2])
    with pytest.raises(RuntimeError, match="contiguous"):
        bwd(gk=gk.transpose(1, 2).contiguous().transpose(1, 2))
    with pytest.raises(RuntimeError, match=r"\[B, S, H, head_dim\]"):
        fwd(q=q.view(B, S, Hq * hd))
    with pytest.raises(RuntimeError, match="agree in B, S and head_dim"):
        fwd(k=k[:1].contiguous())
    with pytest.raises(RuntimeError, match="agree in B, S and head_dim"):
        fwd(k=k[:, :-1].contiguous())
    with pytest.raises(RuntimeError, match="agree in B, S and head_dim"):
        fwd(k=torch.cat([k, k], 3).contiguous())
    with pytest.raises(RuntimeError, match="one dtype"):
        fwd(k=k.bfloat16())
    with pytest.raises(RuntimeError, match="float32 or bfloat16"):
        fwd(q=q.half(), k=k.half())
    with pytest.raises(RuntimeError, match="head_dim must be 64 or 128"):
        fwd(q=q[..., :32].contiguous(), k=k[..., :32].contiguous(), wq=wq[:32].contiguous(),
            wk=wk[:32].contiguous(), cos=cos[:, :16].contiguous(), sin=sin[:, :16].contiguous())
    with pytest.raises(RuntimeError, match="gains must be fp32"):
        fwd(wq=wq.bfloat16())
    with pytest.raises(RuntimeError, match="gains must be fp32"):
        fwd(wk=torch.cat([wk, wk]))
    with pytest.raises(RuntimeError, match="gains must be fp32"):
        fwd(wk=wk.view(1, hd))
    with pytest.raises(RuntimeError, match="cos / sin must be fp32"):
        fwd(cos=cos[:-1].contiguous())
    with pytest.raises(RuntimeError, match="cos / sin must be fp32"):
        fwd(sin=sin.double())
    with pytest.raises(RuntimeError, match="cos / sin must be fp32"):
        fwd(sin=torch.cat([sin, sin], 1))
    with pytest.raises(RuntimeError, match="match q and k in shape and dtype"):
        bwd(gq=gq[:1].contiguous())
    with pytest.raises(RuntimeError, match="match q and k in shape and dtype"):
        bwd(gk=gk.bfloat16())
    # tables longer than S are fine: the first S rows are read
    long_cos, long_sin = torch.cat([cos, cos]), torch.cat([sin, sin])
    a = fwd(cos=long_cos, sin=long_sin)
    b = fwd()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    # no rows: empty outputs (and zero weight gradients), no launch
    for e in (dict(q=q[:0], k=k[:0], gq=gq[:0], gk=gk[:0]),
              dict(q=q[:, :0], k=k[:, :0], gq=gq[:, :0], gk=gk[:, :0])):
        e = {n: t.contiguous() for n, t in e.items()}
        yq, yk = fwd(q=e["q"], k=e["k"])
        assert yq.shape == e["q"].shape and yk.shape == e["k"].shape
        dq, dk, dwq, dwk = bwd(**e)
        assert dq.shape == e["q"].shape and dk.shape == e["k"].shape
        assert float(dwq.abs().sum()) == 0.0 and float(dwk.abs().sum()) == 0.0 and dwq.shape == (hd,)
    torch.cuda.synchronize()


@DTYPES
@pytest.mark.parametrize("what", ["hd32", "bf16_gains"])
def test_fallback_runs_the_reference_on_the_gpu(dev, monkeypatch, what, dtype):
    from cs744_pytorch_distributed_tutorial_amd.ops import lm
    calls = []
    ref = lm.qk_norm_rope_ref
    monkeypatch.setattr(lm, "qk_norm_rope_ref", lambda *a, **kw: calls.append(1) or ref(*a, **kw))
    inp = list(orc.make_inputs((2, 33, 4, 2, 32 if what == "hd32" else 64, 1.0), dtype, dev))
    if what == "bf16_gains":
        inp[2], inp[3] = inp[2].bfloat16(), inp[3].bfloat16()
    outs, grads = _op_run(inp)
    assert calls == [1]
    # bf16 gains get bf16 gradients: the fp32 bound of dw is not theirs
    orc.check_against_oracle(inp, outs, grads[:2] if what == "bf16_gains" else grads, dtype, tag=f"fallback {what}")


def test_one_missing_output_gradient_is_zeros_of_that_output(dev, monkeypatch):
    _no_ref(monkeypatch)
    from cs744_pytorch_distributed_tutorial_amd.ops import lm
    inp = orc.make_inputs(CASES[4], BF16, dev)
    q, k, wq, wk, cos, sin, gq, gk = inp
    a = [t.detach().requires_grad_() for t in (q, k, wq, wk)]
    yq, _ = lm.qk_norm_rope(*a, cos, sin, EPS)
    yq.backward(gq)  # k' unused: its gradient arrives as None
    _, want = _op_run(inp, grads_in=[gq, torch.zeros_like(gk)])
    for t, w in zip(a, want):
        assert torch.equal(t.grad, w)
    assert float(a[1].grad.abs().max()) == 0.0 and float(a[3].grad.abs().max()) == 0.0
    # inputs that need no gradient get none
    _, g = _op_run(inp, need=(True, False, False, True))
    assert g[1] is None and g[2] is None and torch.equal(g[0], _op_run(inp)[1][0])


# ------------------------------------------------------------------ model and trainer
def test_llama_tiny_qk_norm_gpu_matches_cpu_reference(dev, monkeypatch):
    """fp32: attention runs the reference on both devices, so the difference is the new op's"""
    from cs744_pytorch_distributed_tutorial_amd.models import llama
    torch.manual_seed(0)
    cpu = llama.build("llama-tiny", qk_norm=True)
    with torch.no_grad():
        g = torch.Generator().manual_seed(5)
        for blk in cpu.layers:  # gains off their initial ones
            for n in (blk.attention.q_norm, blk.attention.k_norm):
                n.weight.copy_(torch.rand(64, generator=g) + 0.5)
    gpu = llama.build("llama-tiny", qk_norm=True).to(dev)
    gpu.load_state_dict(cpu.state_dict())
    g = torch.Generator().manual_seed(1)
    tok = torch.randint(0, 1024, (2, 33), generator=g)
    tgt = torch.randint(0, 1024, (2, 33), generator=g)
    lc = cpu(tok, targets=tgt)
    lc.backward()
    _no_ref(monkeypatch)
    lg = gpu(tok.to(dev), targets=tgt.to(dev))
    lg.backward()
    lg, lc = float(lg.detach()), float(lc.detach())
    print(f"[qk-norm] llama-tiny fp32 loss gpu {lg:.6f} cpu {lc:.6f}")
    assert abs(lg - lc) <= 1e-4
    pc = dict(cpu.named_parameters())
    n_checked = 0
    for name, p in gpu.named_parameters():
        if "q_norm" in name or "k_norm" in name:
            want = pc[name].grad
            assert float(want.abs().max()) > 0
            err = float((p.grad.cpu() - want).abs().max()) / float(want.abs().max())
            print(f"[qk-norm] {name} grad err / max {err:.3e}")
            assert err <= 1e-3, name
            n_checked += 1
    assert n_checked == 4


def test_trainer_bf16_with_every_lm_option(dev, clean_env):
    from cs744_pytorch_distributed_tutorial_amd.ops.lm import ShadowLinear
    from cs744_pytorch_distributed_tutorial_amd.runtime.torch_trainer import SyntheticBatches, TorchTrainer
    tr = TorchTrainer("llama-tiny", 8, dev, dtype="bf16", optimizer="adamw", lr=1e-3, weight_decay=0.1, seed=7,
                      fused_residual=True, doc_len=32, fused_head=True, qk_norm=True)
    assert tr.qk_norm and tr.fused_residual and tr.fused_head and tr.doc_len == 32
    seq = tr.data.tokens.shape[1] - 1
    tr.data = SyntheticBatches("tokens", 8, dev, seq=seq, vocab=1024, pool=8, seed=7, doc_len=32, eos_id=tr.eos_id)
    gains = [p for n, p in tr.module.named_parameters() if "q_norm" in n or "k_norm" in n]
    no_decay = tr.opt.param_groups[1]["params"]
    assert len(gains) == 4 and all(any(p is x for x in no_decay) for p in gains)
    assert tr.opt.param_groups[1]["weight_decay"] == 0
    losses = []
    for _ in range(30):
        tr.step()
        losses.append(tr.last_loss())
    print(f"[qk-norm] trainer losses first {losses[:3]} last {losses[-5:]}")
    assert all(v == v and abs(v) != float("inf") for v in losses)
    assert sum(losses[-5:]) / 5 < sum(losses[:3]) / 3
    assert all(not bool((p == 1).all()) for p in gains)  # the gains train
    n = 0
    for m in tr.module.modules():
        if isinstance(m, ShadowLinear):
            assert torch.equal(m.weight._cs_bf16_shadow, m.weight.detach().to(torch.bfloat16))
            n += 1
    assert n == 2 * 7 + 1


def test_trainer_without_qk_norm_is_unchanged(dev, clean_env):
    from cs744_pytorch_distributed_tutorial_amd.runtime.torch_trainer import TorchTrainer
    runs = []
    for kw in ({}, {"qk_norm": False}):
        tr = TorchTrainer("llama-tiny", 8, dev, dtype="bf16", optimizer="adamw", lr=1e-3, seq_len=32, **kw)
        assert tr.qk_norm is False and not any("q_norm" in n for n in tr.module.state_dict())
        losses = []
        for _ in range(3):
            tr.step()
            losses.append(tr.loss)
        runs.append(torch.stack(losses).float().cpu())
    print(f"[qk-norm] trainer losses without the argument {runs[0].tolist()} with qk_norm=False {runs[1].tolist()}")
    assert bool(torch.isfinite(runs[0]).all()) and torch.equal(runs[0], runs[1])
