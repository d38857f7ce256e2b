"""The masked, z-regularised fused cross-entropy (xent_fwd_masked_kernel / xent_reduce_kernel /
xent_bwd_masked_kernel of csrc/kernels/lm.hip, ops.lm.cross_entropy(ignore_index=, z_loss=)) up to the
trainer's loss_mask / z_loss / evaluate().

Oracle: xent_masked_oracle below, the formula in float64 on the same input values. Tolerances: those
of tests/test_lm_edges_gpu.py for the unmasked kernels; with z > 0 scaled by 1 + 2 z max|lse|, the
derivative of the added term z lse^2 with respect to lse: the most the lse error already allowed can
add. docs/lm_edge_tests.md lists the branch each case enters and the errors measured.
The oracle takes any device and is checked on CPU by tests/test_xent_masked_cpu.py.
"""
import math

import pytest
import torch

from test_lm_edges_gpu import Report, XENT_GRAD_TOL, XENT_LOSS_TOL, offset_view, xent_oracle

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
G = 2.5  # the upstream gradient of every backward here


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cs744_pytorch_distributed_tutorial_amd.ops import native
    native.C()
    return torch.device("cuda", 0)


def _dt(d):
    return "bf16" if d == BF16 else "fp32"


# ------------------------------------------------------------------ float64 oracle
def xent_masked_oracle(x, t, ignore, z, g=1.0):
    """-> per-row loss, lse, dlogits, mean, n_valid; all float64 (n_valid an int).
    Rows with t == ignore (None: no row): loss = lse = 0, a zero dlogits row, whatever their logits hold.
    Other rows: lse = log sum exp, loss = (lse - x_t) + z lse^2, or NaN for t outside [0, V);
    dlogits = (softmax (1 + 2 z lse) - onehot) g / max(n_valid, 1), without the one-hot for such a t.
    mean = sum of the losses / max(n_valid, 1): 0 when every row is ignored."""
    xd = x.detach().double()
    R, V = xd.shape
    valid = torch.ones(R, dtype=torch.bool, device=x.device) if ignore is None else t != ignore
    xd = torch.where(valid[:, None], xd, torch.zeros_like(xd))
    lse = torch.logsumexp(xd, -1)
    ok = (t >= 0) & (t < V)
    tc = t.clamp(0, V - 1)
    loss = torch.where(ok, lse - xd.gather(1, tc[:, None])[:, 0] + z * lse * lse, torch.full_like(lse, float("nan")))
    d = torch.exp(xd - lse[:, None]) * (1 + 2 * z * lse)[:, None]
    d[torch.arange(R, device=x.device)[ok], tc[ok]] -= 1.0
    n = int(valid.sum())
    zero = torch.zeros_like(lse)
    loss, lse = torch.where(valid, loss, zero), torch.where(valid, lse, zero)
    d = torch.where(valid[:, None], d, torch.zeros_like(d)) * (g / max(n, 1))
    return loss, lse, d, loss.sum() / max(n, 1), n


def _scaled(tol, z, lse):
    """tol times 1 + 2 z max|lse| (z = 0: tol itself)"""
    k = 1.0 + 2.0 * z * float(lse.abs().max()) if z > 0 else 1.0
    return dict(rtol=tol["rtol"] * k, atol=tol["atol"] * k)


# ------------------------------------------------------------------ inputs, built once
SHAPES = [(5, 8), (3, 2048), (2, 2056), (7, 1024)]
PATTERNS = ["none", "first", "last", "alternate", "all_but_one"]
ZS = [0.0, 1e-4, 0.5]
_CACHE = {}


def _pattern(R, pattern):
    m = torch.zeros(R, dtype=torch.bool)
    if pattern == "first":
        m[0] = True
    elif pattern == "last":
        m[-1] = True
    elif pattern == "alternate":
        m[::2] = True
    elif pattern == "all_but_one":
        m[:] = True
        m[R // 2] = False
    return m


def _inputs(R, V, dtype, dev):
    """logits and in-range targets of a shape; the same tensors for every case that uses it"""
    key = (R, V, dtype)
    if key not in _CACHE:
        g_ = torch.Generator(device="cpu").manual_seed(V * 31 + R)
        x = (torch.randn(R, V, generator=g_) * 3).to(dtype).to(dev)
        t = torch.randint(0, V, (R,), generator=g_).to(dev)
        _CACHE[key] = (x, t)
    return _CACHE[key]


def _masked_targets(t, V, pattern, ignore):
    """t with the pattern's rows set to `ignore`. An in-vocabulary ignore id (a pad id) is also put
    where it cannot be told from a real target: any row that already carries it is ignored too."""
    t = t.clone()
    t[_pattern(t.numel(), pattern).to(t.device)] = ignore
    return t


def _run(x, t, ignore, z, g=G):
    from cs744_pytorch_distributed_tutorial_amd import _C
    loss, lse, stats = _C.xent_fwd_masked(x, t, ignore, z)
    gs = torch.full((1,), g, device=x.device)
    return loss, lse, stats, _C.xent_bwd_masked(x, t, lse, stats, gs, ignore, z)


# ------------------------------------------------------------------ 1. against the oracle
@pytest.mark.parametrize("z", ZS)
@pytest.mark.parametrize("ignore", [-100, "pad"])
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("R,V", SHAPES)
@pytest.mark.parametrize("dtype", [F32, BF16], ids=_dt)
def test_masked_against_oracle(dev, dtype, R, V, pattern, ignore, z):
    from cs744_pytorch_distributed_tutorial_amd.ops import lm
    x, t0 = _inputs(R, V, dtype, dev)
    if ignore == "pad":  # an id that some unmasked row also has as its genuine target: that row is ignored too
        keep = (~_pattern(R, pattern)).nonzero().flatten()
        ignore = int(t0[keep[0]])
    t = _masked_targets(t0, V, pattern, ignore)
    rloss, rlse, rd, rmean, n = xent_masked_oracle(x, t, ignore, z, G)
    assert n == int((t != ignore).sum()) and n <= R - int(_pattern(R, pattern).sum())
    loss, lse, stats, d = _run(x, t, ignore, z)
    ltol, gtol = _scaled(XENT_LOSS_TOL, z, rlse), _scaled(XENT_GRAD_TOL[dtype], z, rlse)
    rep = Report(f"xent masked ({R}, {V}) {_dt(dtype)} {pattern} ignore {ignore} z {z} n_valid {n}")
    rep.add("loss", loss, rloss, **ltol)
    rep.add("lse", lse, rlse, **XENT_LOSS_TOL)
    rep.add("dlogits", d, rd, **gtol)
    assert int(stats[1]) == n
    rep.add("sum", stats[0], rloss.sum(), **ltol)
    xa = x.clone().requires_grad_()
    mean = lm.cross_entropy(xa, t, ignore_index=ignore, z_loss=z)
    (G * mean).backward()
    assert mean.dtype == F32 and mean.dim() == 0 and xa.grad.dtype == dtype
    rep.add("mean", mean, rmean, **ltol)
    rep.add("autograd", xa.grad, rd, **gtol)
    rep.done()
    ign = t == ignore
    assert bool((d[ign] == 0).all()) and bool((loss[ign] == 0).all()) and bool((lse[ign] == 0).all())


@pytest.mark.parametrize("z", [1e-4, 0.5])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=_dt)
def test_z_loss_without_ignore_index(dev, dtype, z):
    """ignore_index=None with z > 0: the masked kernels with no row ignored; a -100 target still poisons"""
    from cs744_pytorch_distributed_tutorial_amd.ops import lm
    x, t = _inputs(7, 1024, dtype, dev)
    rloss, rlse, rd, rmean, n = xent_masked_oracle(x, t, None, z, G)
    assert n == 7
    xa = x.clone().requires_grad_()
    mean = lm.cross_entropy(xa, t, z_loss=z)
    (G * mean).backward()
    rep = Report(f"xent z-loss only {_dt(dtype)} z {z}")
    rep.add("mean", mean, rmean, **_scaled(XENT_LOSS_TOL, z, rlse))
    rep.add("autograd", xa.grad, rd, **_scaled(XENT_GRAD_TOL[dtype], z, rlse))
    rep.done()
    tb = t.clone()
    tb[2] = -100
    assert bool(torch.isnan(lm.cross_entropy(x, tb, z_loss=z)))


# ------------------------------------------------------------------ 2. bitwise against the unmasked kernels
@pytest.mark.parametrize("pattern", ["none", "first", "alternate", "all_but_one"])
@pytest.mark.parametrize("R,V", SHAPES)
@pytest.mark.parametrize("dtype", [F32, BF16], ids=_dt)
def test_z0_bitwise_equal_to_unmasked_kernels(dev, dtype, R, V, pattern):
    from cs744_pytorch_distributed_tutorial_amd import _C
    x, t0 = _inputs(R, V, dtype, dev)
    t = _masked_targets(t0, V, pattern, -100)
    valid = t != -100
    n = int(valid.sum())
    assert n == (R if pattern == "none" else R - int(_pattern(R, pattern).sum())) and n >= 1
    loss, lse, stats, d = _run(x, t, -100, 0.0)
    uloss, ulse = _C.xent_fwd(x, t0)  # the unmasked kernel on the same logits, every target in range
    ud = _C.xent_bwd(x, t0, ulse, torch.full((1,), G, device=dev), 1.0 / n)
    assert torch.equal(loss[valid], uloss[valid]) and torch.equal(lse[valid], ulse[valid])
    assert torch.equal(d[valid], ud[valid])
    assert int(stats[1]) == n
    inv = torch.tensor(1.0 / n, dtype=torch.float64).float().double()  # the double quotient rounded once
    assert float(stats[2]) == float(inv)
    assert bool((d[~valid] == 0).all())


# ------------------------------------------------------------------ 3. ignored rows are not read
@pytest.mark.parametrize("fill", [float("nan"), float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("z", [0.0, 1e-4])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=_dt)
def test_ignored_rows_are_not_read(dev, dtype, z, fill):
    from cs744_pytorch_distributed_tutorial_amd.ops import lm
    R, V = 7, 1024
    x, t0 = _inputs(R, V, dtype, dev)
    t = _masked_targets(t0, V, "alternate", -100)
    ign = t == -100
    xb = x.clone()
    xb[ign] = fill
    outs = []
    for inp in (x, xb):
        xa = inp.clone().requires_grad_()
        mean = lm.cross_entropy(xa, t, ignore_index=-100, z_loss=z)
        (G * mean).backward()
        outs.append((mean.detach(), xa.grad))
    (m0, d0), (m1, d1) = outs
    assert bool(torch.isfinite(m1)) and torch.equal(m0, m1)
    assert not bool(torch.isnan(d1.float()).any()) and bool((d1[ign] == 0).all())
    assert torch.equal(d0, d1)


# ------------------------------------------------------------------ 4. every row ignored
@pytest.mark.parametrize("ignore", [-100, 5])
@pytest.mark.parametrize("z", [0.0, 0.5])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=_dt)
def test_all_rows_ignored_gives_zero(dev, dtype, z, ignore):
    from cs744_pytorch_distributed_tutorial_amd.ops import lm
    x, _ = _inputs(3, 2048, dtype, dev)
    t = torch.full((3,), ignore, device=dev)
    xa = x.clone().requires_grad_()
    mean = lm.cross_entropy(xa, t, ignore_index=ignore, z_loss=z)
    (G * mean).backward()
    assert float(mean.detach()) == 0.0
    assert bool((xa.grad == 0).all())
    loss, lse, stats, d = _run(x, t, ignore, z)
    assert stats.tolist() == [0.0, 0.0, 1.0, 0.0]
    assert bool((loss == 0).all()) and bool((lse == 0).all()) and bool((d == 0).all())


# ------------------------------------------------------------------ 5. the poison rule is kept
@pytest.mark.parametrize("z", [0.0, 1e-4])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=_dt)
def test_out_of_range_targets_still_poison(dev, dtype, z):
    from cs744_pytorch_distributed_tutorial_amd.ops import lm
    R, V = 7, 1024
    x, t0 = _inputs(R, V, dtype, dev)
    t = t0.clone()
    t[1], t[3], t[4], t[6] = V, -100, -1, -100
    rloss, rlse, rd, rmean, n = xent_masked_oracle(x, t, -100, z, G)
    assert n == 5 and bool(torch.isnan(rmean))
    loss, lse, stats, d = _run(x, t, -100, z)
    bad = torch.tensor([False, True, False, False, True, False, False], device=dev)
    assert torch.equal(torch.isnan(loss), bad) and int(stats[1]) == 5 and math.isnan(float(stats[3]))
    assert bool(torch.isfinite(d.float()).all())
    assert bool((d[t == -100] == 0).all())
    rep = Report(f"xent masked poison {_dt(dtype)} z {z}")
    rep.add("lse", lse, rlse, **XENT_LOSS_TOL)
    rep.add("dlogits", d, rd, **_scaled(XENT_GRAD_TOL[dtype], z, rlse))  # bad rows: softmax term alone
    rep.done()
    xa = x.clone().requires_grad_()
    mean = lm.cross_entropy(xa, t, ignore_index=-100, z_loss=z)
    mean.backward()
    assert bool(torch.isnan(mean)) and bool(torch.isfinite(xa.grad.float()).all())


# ------------------------------------------------------------------ 6. the reduction
# xent_reduce_kernel: one block of 1024 threads, thread i takes rows i, i + 1024, ..., eight of them per
# trip. R = 1 one busy thread; 255 / 257; 1023 one idle thread; 1025 thread 0 alone has a second row;
# 4099 four rows each and three threads a fifth; 8192 exactly one full trip; 8193 thread 0 alone takes a
# second trip
@pytest.mark.parametrize("R", [1, 255, 257, 1023, 1025, 4099, 8192, 8193])
def test_reduction_counts_and_is_deterministic(dev, R):
    from cs744_pytorch_distributed_tutorial_amd.ops import lm
    V = 8
    g_ = torch.Generator(device="cpu").manual_seed(R)
    x = (torch.randn(R, V, generator=g_) * 3).to(dev)
    t = torch.randint(0, V, (R,), generator=g_)
    t[torch.rand(R, generator=g_) < 0.3] = -100
    t = t.to(dev)
    rloss, _, rd, rmean, n = xent_masked_oracle(x, t, -100, 0.0, G)
    runs = []
    for _ in range(2):
        xa = x.clone().requires_grad_()
        mean = lm.cross_entropy(xa, t, ignore_index=-100)
        (G * mean).backward()
        runs.append((mean.detach(), xa.grad))
    _, _, stats, _ = _run(x, t, -100, 0.0)
    assert int(stats[1]) == n == int((t != -100).sum())
    nll, cnt = lm.cross_entropy_sums(x, t, ignore_index=-100)
    assert int(cnt) == n and cnt.dtype == torch.int64 and nll.dtype == torch.float64
    rep = Report(f"xent reduce R {R} n_valid {n}")
    rep.add("mean", runs[0][0], rmean, **XENT_LOSS_TOL)
    rep.add("sum", nll, rloss.sum(), **XENT_LOSS_TOL)
    rep.add("autograd", runs[0][1], rd, **XENT_GRAD_TOL[F32])
    rep.done()
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


# ------------------------------------------------------------------ 7. fallback and offset views
@pytest.mark.parametrize("z", [0.0, 0.5])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=_dt)
def test_odd_vocabulary_runs_the_reference(dev, dtype, z, monkeypatch):
    """V = 1001 on the GPU: cross_entropy_ref (fp32 torch ops), never the bindings"""
    from cs744_pytorch_distributed_tutorial_amd.ops import lm
    R, V = 6, 1001
    g_ = torch.Generator(device="cpu").manual_seed(77)
    x = (torch.randn(R, V, generator=g_) * 3).to(dtype).to(dev)
    t = torch.randint(0, V, (R,), generator=g_).to(dev)
    t[0], t[4] = -100, -100
    calls = []
    ref = lm.cross_entropy_ref
    monkeypatch.setattr(lm, "cross_entropy_ref", lambda *a, **k: (calls.append(1), ref(*a, **k))[1])
    xa = x.clone().requires_grad_()
    mean = lm.cross_entropy(xa, t, ignore_index=-100, z_loss=z)
    (G * mean).backward()
    assert calls == [1]
    _, rlse, rd, rmean, n = xent_masked_oracle(x, t, -100, z, G)
    rep = Report(f"xent masked V = 1001 {_dt(dtype)} z {z}")
    rep.add("mean", mean, rmean, **_scaled(XENT_LOSS_TOL, z, rlse))
    rep.add("autograd", xa.grad, rd, **_scaled(XENT_GRAD_TOL[dtype], z, rlse))
    rep.done()
    nll, cnt = lm.cross_entropy_sums(x, t, ignore_index=-100)
    assert int(cnt) == n == 4
    # everything ignored, and an out-of-range target, on this path too
    ta = torch.full((R,), -100, device=dev)
    xa = x.clone().requires_grad_()
    m0 = lm.cross_entropy(xa, ta, ignore_index=-100, z_loss=z)
    m0.backward()
    assert float(m0.detach()) == 0.0 and bool((xa.grad == 0).all())
    t[1] = V
    assert bool(torch.isnan(lm.cross_entropy(x, t, ignore_index=-100, z_loss=z)))


@pytest.mark.parametrize("dtype", [F32, BF16], ids=_dt)
def test_offset_view(dev, dtype):
    from cs744_pytorch_distributed_tutorial_amd import _C
    from cs744_pytorch_distributed_tutorial_amd.ops import lm
    R, V = 2, 2056
    x, t0 = _inputs(R, V, dtype, dev)
    t = _masked_targets(t0, V, "first", -100)
    outs = []
    for view in (False, True):
        xv = (offset_view(x) if view else x.clone()).requires_grad_()
        mean = lm.cross_entropy(xv, t, ignore_index=-100, z_loss=1e-4)
        (G * mean).backward()
        outs.append((mean.detach(), xv.grad))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    xo = offset_view(x)
    _, lse, stats = _C.xent_fwd_masked(x, t, -100, 1e-4)
    with pytest.raises(RuntimeError, match="aligned"):
        _C.xent_fwd_masked(xo, t, -100, 1e-4)
    with pytest.raises(RuntimeError, match="aligned"):
        _C.xent_bwd_masked(xo, t, lse, stats, torch.ones(1, device=dev), -100, 1e-4)
    torch.cuda.synchronize()


# ------------------------------------------------------------------ 8. host checks
def test_host_checks(dev):
    from cs744_pytorch_distributed_tutorial_amd import _C
    x, t0 = _inputs(7, 1024, F32, dev)
    t = _masked_targets(t0, 1024, "first", -100)
    _, lse, stats = _C.xent_fwd_masked(x, t, -100, 0.0)
    g = torch.ones(1, device=dev)

    def fwd(x=x, t=t, z=0.0):
        return _C.xent_fwd_masked(x, t, -100, z)

    def bwd(x=x, t=t, lse=lse, stats=stats, g=g, z=0.0):
        return _C.xent_bwd_masked(x, t, lse, stats, g, -100, z)

    bad_stats = [stats[:3].clone(), stats.reshape(2, 2), stats.float(), stats.cpu(),
                 torch.zeros(8, dtype=torch.float64, device=dev)[::2]]
    for s in bad_stats:
        with pytest.raises(RuntimeError, match="stats"):
            bwd(stats=s)
    for f in (fwd, bwd):
        with pytest.raises(RuntimeError, match="int64"):
            f(t=t.int())
        with pytest.raises(RuntimeError, match="int64"):
            f(t=t[:-1].contiguous())
        for z in (-1e-4, float("inf"), float("nan")):
            with pytest.raises(RuntimeError, match="z_loss"):
                f(z=z)
        with pytest.raises(RuntimeError, match="V % 8"):
            f(x=x[:, :1001].contiguous())
        with pytest.raises(RuntimeError):
            f(x=x.half())
        with pytest.raises(RuntimeError):
            f(x=x.cpu())
    for gbad in (torch.ones(2, device=dev), torch.ones(1, device=dev, dtype=torch.float64), torch.ones(1)):
        with pytest.raises(RuntimeError, match="g must be"):
            bwd(g=gbad)
    with pytest.raises(RuntimeError, match="lse"):
        bwd(lse=lse.double())
    torch.cuda.synchronize()
    # the wrapper refuses a bad z before anything else
    from cs744_pytorch_distributed_tutorial_amd.ops import lm
    for z in (-1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            lm.cross_entropy(x, t, ignore_index=-100, z_loss=z)


# ------------------------------------------------------------------ 9. model level
def test_model_boundary_targets_take_no_gradient(dev):
    from cs744_pytorch_distributed_tutorial_amd.models import llama
    from cs744_pytorch_distributed_tutorial_amd.ops import lm
    from cs744_pytorch_distributed_tutorial_amd.ops.attention import doc_ids_from_eos
    from cs744_pytorch_distributed_tutorial_amd.runtime.torch_trainer import SyntheticBatches
    torch.manual_seed(0)
    model = llama.build("llama-tiny").to(dev)
    eos = model.cfg.eos_id
    data = SyntheticBatches("tokens", 4, dev, seq=128, vocab=1024, pool=4, seed=3, doc_len=32, eos_id=eos)
    x, y = data.next()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        logits = model(x, doc_ids=doc_ids_from_eos(x, eos))
        logits.retain_grad()
        tm = lm.mask_boundary_targets(x, y, eos)
        loss = lm.cross_entropy(logits.view(-1, logits.shape[-1]), tm.view(-1), ignore_index=-100, z_loss=1e-4)
    loss.backward()
    at_eos = (x == eos)
    assert int(at_eos.sum()) >= 4 and int((tm == -100).sum()) == int(at_eos.sum())
    assert logits.dtype == BF16 and bool(torch.isfinite(loss))
    gr = logits.grad
    assert bool((gr[at_eos] == 0).all())
    assert bool((gr[~at_eos] != 0).any(-1).all())  # every other row carries a gradient


# ------------------------------------------------------------------ 10. trainer
def test_trainer_learns_with_loss_mask_and_z_loss(dev, monkeypatch):
    """The configuration of test_trainer_learns_on_packed_documents (tests/test_attention_docmask_gpu.py)
    plus loss_mask="doc", z_loss=1e-4, and that test's own conditions; then evaluate()."""
    from cs744_pytorch_distributed_tutorial_amd.runtime.torch_trainer import SyntheticBatches, TorchTrainer
    for key in ("CS744_OPTIMIZER", "CS744_LR", "CS744_WEIGHT_DECAY", "CS744_MAX_GRAD_NORM", "CS744_GRAD_COMM_DTYPE",
                "CS744_DOC_LEN", "CS744_LOSS_MASK", "CS744_Z_LOSS"):
        monkeypatch.delenv(key, raising=False)
    seed = 5000
    tr = TorchTrainer("llama-tiny", batch_size=8, device=dev, dtype="bf16", optimizer="adamw", lr=3e-4,
                      weight_decay=0.1, max_grad_norm=1.0, doc_len=32, seed=seed, loss_mask="doc", z_loss=1e-4)
    assert tr.loss_mask == "doc" and tr.z_loss == 1e-4
    seq = tr.data.tokens.shape[1] - 1
    tr.data = SyntheticBatches("tokens", 8, dev, seq=seq, vocab=1024, pool=8, seed=seed, doc_len=32, eos_id=tr.eos_id)
    assert tr.tokens_per_step() == 8 * seq
    losses = []
    for _ in range(50):
        tr.step()
        losses.append(tr.loss)
    losses = torch.stack(losses).float().cpu()
    print(f"[xent-masked] trainer: first {float(losses[0]):.3f} last {float(losses[-1]):.3f}")
    assert bool(torch.isfinite(losses).all())
    assert float(losses[-1]) < float(losses[0])
    assert float(losses[-1]) < math.log(1024)
    # evaluate() draws its batches from the pool with the data generator: replay the draw
    state = tr.data.gen.get_state()
    ev = tr.evaluate(2)
    tr.data.gen.set_state(state)
    want = sum(int((tr.data.next()[0] != tr.eos_id).sum()) for _ in range(2))
    print(f"[xent-masked] evaluate: {ev}")
    assert ev["tokens"] == want and 0 < want < 2 * 8 * seq
    assert math.isfinite(ev["nll"]) and ev["nll"] < math.log(1024)
    assert ev["ppl"] == pytest.approx(math.exp(ev["nll"]))
    assert tr.net.training
