"""The chunked LM head: xent_fused_kernel / xent_count_kernel of csrc/kernels/lm.hip, their bindings,
ops.lm.linear_cross_entropy / linear_cross_entropy_sums, Llama.forward(targets=) and
TorchTrainer(fused_head=True).

Yardsticks. The kernel: the existing pair xent_fwd_masked + xent_bwd_masked with g = 1, bit for bit.
linear_cross_entropy and the model: a float64 oracle on the values the GEMMs read, with the rule of
tests/test_adamw_gpu.py: e(x) = max|x - x64| / max|x64| per tensor, and the fused path may have at
most 2 e(today's unfused path) plus one rounding of the output dtype (eps / 2). The factor 2 allows
another, equally valid summation order over the chunks; the extra rounding is the multiplication by the
upstream gradient, which the unfused path folds into the kernel's scale. Nothing in a bound comes from
the fused code. Loss tolerances: XENT_LOSS_TOL of tests/test_lm_edges_gpu.py, scaled for z as
tests/test_xent_masked_gpu.py does.
"""
import copy
import math

import pytest
import torch

from test_lm_edges_gpu import Report, XENT_GRAD_TOL, XENT_LOSS_TOL, offset_view
from test_xent_masked_gpu import PATTERNS, SHAPES, ZS, _inputs, _masked_targets, _pattern, _scaled, xent_masked_oracle

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
G = 2.5  # the upstream gradient of the linear_cross_entropy cases
NO_IGNORE = -(1 << 63)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cs744_pytorch_distributed_tutorial_amd.ops import native
    native.C()
    return torch.device("cuda", 0)


def _dt(d):
    return "bf16" if d == BF16 else "fp32"


def _pair(x, t, ignore, z):
    """the existing kernels with g = 1 -> loss, lse, stats, dlogits"""
    from cs744_pytorch_distributed_tutorial_amd import _C
    loss, lse, stats = _C.xent_fwd_masked(x, t, ignore, z)
    d = _C.xent_bwd_masked(x, t, lse, stats, torch.ones(1, device=x.device), ignore, z)
    return loss, lse, stats, d


def _fused(x, t, stats, ignore, z, R=None, row0=0, fill=7.0):
    """xent_fused_ on a clone of x -> loss, lse (length R, pre-filled), the overwritten clone"""
    from cs744_pytorch_distributed_tutorial_amd import _C
    R = t.numel() if R is None else R
    xc = x.clone()
    loss = torch.full((R,), fill, device=x.device)
    lse = torch.full((R,), fill, device=x.device)
    _C.xent_fused_(xc, t, loss, lse, stats, row0, ignore, z)
    return loss, lse, xc


def _bits(a, b):
    """equal bit for bit (NaNs of the same payload included)"""
    if a.dtype == BF16:
        return torch.equal(a.view(torch.int16), b.view(torch.int16))
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


# ------------------------------------------------------------------ 1. the kernel against the pair, bitwise
@pytest.mark.parametrize("z", ZS)
@pytest.mark.parametrize("ignore", [-100, "pad"])
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("R,V", SHAPES)
@pytest.mark.parametrize("dtype", [F32, BF16], ids=_dt)
def test_fused_kernel_bitwise_equal_to_pair(dev, dtype, R, V, pattern, ignore, z):
    from cs744_pytorch_distributed_tutorial_amd import _C
    x, t0 = _inputs(R, V, dtype, dev)
    if ignore == "pad":
        keep = (~_pattern(R, pattern)).nonzero().flatten()
        ignore = int(t0[keep[0]])
    t = _masked_targets(t0, V, pattern, ignore)
    loss, lse, stats, d = _pair(x, t, ignore, z)
    cnt = _C.xent_count(t, ignore)
    assert torch.equal(cnt[1:3], stats[1:3]) and cnt[0] == 0 and cnt[3] == 0
    floss, flse, fd = _fused(x, t, cnt, ignore, z)
    assert _bits(floss, loss) and _bits(flse, lse)
    assert _bits(fd, d)
    red = torch.empty(4, dtype=torch.float64, device=dev)
    _C.xent_reduce(floss, t, ignore, red)
    assert torch.equal(red, stats)


@pytest.mark.parametrize("z", [0.0, 0.5])
@pytest.mark.parametrize("V", [8, 1024, 2048, 2056])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=_dt)
def test_target_is_read_before_its_vector_is_overwritten(dev, dtype, V, z):
    """targets in column 0, 7 (the ends of thread 0's first vector), 8 (thread 1), 512 (another wave),
    2048 (V = 2056: thread 0's second trip) and V - 1: x[t] comes out of the registers of pass 2"""
    cols = [c for c in (0, 7, 8, 512, 2048, V - 1) if c < V]
    g_ = torch.Generator(device="cpu").manual_seed(V)
    x = (torch.randn(len(cols), V, generator=g_) * 3).to(dtype).to(dev)
    t = torch.tensor(cols, device=dev)
    loss, lse, stats, d = _pair(x, t, -100, z)
    floss, flse, fd = _fused(x, t, stats, -100, z)
    assert _bits(floss, loss) and _bits(flse, lse) and _bits(fd, d)
    rloss, _, rd, _, _ = xent_masked_oracle(x, t, -100, z)
    rep = Report(f"xent fused hazard V {V} {_dt(dtype)} z {z}")
    rep.add("loss", floss, rloss, **_scaled(XENT_LOSS_TOL, z, lse))
    rep.add("dlogits", fd, rd, **_scaled(XENT_GRAD_TOL[dtype], z, lse))
    rep.done()


@pytest.mark.parametrize("dtype", [F32, BF16], ids=_dt)
def test_row0_writes_the_middle_of_longer_arrays(dev, dtype):
    R, V, r0, n = 11, 1024, 4, 5
    g_ = torch.Generator(device="cpu").manual_seed(5)
    x = (torch.randn(R, V, generator=g_) * 3).to(dtype).to(dev)
    t = torch.randint(0, V, (R,), generator=g_).to(dev)
    t[5], t[9] = -100, -100
    loss, lse, stats, d = _pair(x, t, -100, 1e-4)
    floss, flse, fd = _fused(x[r0:r0 + n], t, stats, -100, 1e-4, R=R, row0=r0)
    assert _bits(floss[r0:r0 + n], loss[r0:r0 + n]) and _bits(flse[r0:r0 + n], lse[r0:r0 + n])
    assert _bits(fd, d[r0:r0 + n])
    outside = torch.ones(R, dtype=torch.bool, device=dev)
    outside[r0:r0 + n] = False
    assert bool((floss[outside] == 7.0).all()) and bool((flse[outside] == 7.0).all())
    # the last rows, and the host check on row0 + rows <= R
    floss, flse, fd = _fused(x[R - 2:], t, stats, -100, 1e-4, R=R, row0=R - 2)
    assert _bits(floss[R - 2:], loss[R - 2:]) and _bits(fd, d[R - 2:]) and bool((floss[:R - 2] == 7.0).all())
    from cs744_pytorch_distributed_tutorial_amd import _C
    for bad in (R - 1, -1, R + 1):
        with pytest.raises(RuntimeError, match="row0"):
            _C.xent_fused_(x[:2].clone(), t, floss, flse, stats, bad, -100, 0.0)
    with pytest.raises(RuntimeError, match="aligned"):
        _C.xent_fused_(offset_view(x[:2]), t, floss, flse, stats, 0, -100, 0.0)
    with pytest.raises(RuntimeError, match="V % 8"):
        _C.xent_fused_(x[:2, :1001].contiguous(), t, floss, flse, stats, 0, -100, 0.0)
    with pytest.raises(RuntimeError, match="int64"):
        _C.xent_fused_(x[:2].clone(), t.int(), floss, flse, stats, 0, -100, 0.0)
    with pytest.raises(RuntimeError, match="loss / lse"):
        _C.xent_fused_(x[:2].clone(), t, floss[:-1], flse, stats, 0, -100, 0.0)
    with pytest.raises(RuntimeError, match="stats"):
        _C.xent_fused_(x[:2].clone(), t, floss, flse, stats.float(), 0, -100, 0.0)
    with pytest.raises(RuntimeError, match="z_loss"):
        _C.xent_fused_(x[:2].clone(), t, floss, flse, stats, 0, -100, -1.0)
    torch.cuda.synchronize()


# ------------------------------------------------------------------ 2. ignored rows, out-of-range targets
@pytest.mark.parametrize("fill", [float("nan"), float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("z", [0.0, 1e-4])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=_dt)
def test_ignored_rows_are_not_read(dev, dtype, z, fill):
    R, V = 7, 1024
    x, t0 = _inputs(R, V, dtype, dev)
    t = _masked_targets(t0, V, "alternate", -100)
    ign = t == -100
    xb = x.clone()
    xb[ign] = fill
    _, _, stats, _ = _pair(x, t, -100, z)
    l0, s0, d0 = _fused(x, t, stats, -100, z)
    l1, s1, d1 = _fused(xb, t, stats, -100, z)
    assert bool(torch.isfinite(l1).all()) and bool(torch.isfinite(s1).all()) and bool(torch.isfinite(d1.float()).all())
    assert bool((d1[ign] == 0).all()) and bool((l1[ign] == 0).all()) and bool((s1[ign] == 0).all())
    assert _bits(l0, l1) and _bits(s0, s1) and _bits(d0, d1)


@pytest.mark.parametrize("z", [0.0, 1e-4])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=_dt)
def test_out_of_range_targets_poison_the_loss_only(dev, dtype, z):
    R, V = 7, 1024
    x, t0 = _inputs(R, V, dtype, dev)
    t = t0.clone()
    t[1], t[3], t[4], t[6] = V, -100, -1, -100
    loss, lse, stats, d = _pair(x, t, -100, z)
    floss, flse, fd = _fused(x, t, stats, -100, z)
    bad = torch.tensor([False, True, False, False, True, False, False], device=dev)
    assert torch.equal(torch.isnan(floss), bad)
    assert torch.equal(floss[~bad], loss[~bad]) and _bits(flse, lse) and _bits(fd, d)
    assert bool(torch.isfinite(fd.float()).all())
    _, rlse, rd, _, n = xent_masked_oracle(x, t, -100, z)
    assert n == 5
    rep = Report(f"xent fused poison {_dt(dtype)} z {z}")
    rep.add("lse", flse, rlse, **XENT_LOSS_TOL)
    rep.add("dlogits", fd, rd, **_scaled(XENT_GRAD_TOL[dtype], z, rlse))  # bad rows: softmax term alone
    rep.done()


@pytest.mark.parametrize("ignore", [-100, 5])
@pytest.mark.parametrize("z", [0.0, 0.5])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=_dt)
def test_every_row_ignored(dev, dtype, z, ignore):
    from cs744_pytorch_distributed_tutorial_amd import _C
    x, _ = _inputs(3, 2048, dtype, dev)
    t = torch.full((3,), ignore, device=dev)
    stats = _C.xent_count(t, ignore)
    assert stats.tolist() == [0.0, 0.0, 1.0, 0.0]
    floss, flse, fd = _fused(x, t, stats, ignore, z)
    assert bool((floss == 0).all()) and bool((flse == 0).all()) and bool((fd == 0).all())
    _C.xent_reduce(floss, t, ignore, stats)
    assert stats.tolist() == [0.0, 0.0, 1.0, 0.0]


# ------------------------------------------------------------------ 3. xent_count
@pytest.mark.parametrize("masked", [False, True], ids=["all-valid", "masked"])
@pytest.mark.parametrize("R", [1, 1023, 1024, 1025, 8192, 8193])
def test_count_matches_the_masked_forward(dev, R, masked):
    from cs744_pytorch_distributed_tutorial_amd import _C
    V = 8
    g_ = torch.Generator(device="cpu").manual_seed(R)
    x = torch.randn(R, V, generator=g_).to(dev)
    t = torch.randint(0, V, (R,), generator=g_)
    if masked:
        t[torch.rand(R, generator=g_) < 0.3] = -100
        t[R - 1] = -100
    t = t.to(dev)
    stats = _C.xent_fwd_masked(x, t, -100, 0.0)[2]
    a, b = _C.xent_count(t, -100), _C.xent_count(t, -100)
    assert int(a[1]) == int((t != -100).sum())
    assert torch.equal(a[1:3].view(torch.int64), stats[1:3].view(torch.int64))
    assert torch.equal(a.view(torch.int64), b.view(torch.int64))


# ------------------------------------------------------------------ 4. linear_cross_entropy against float64
D_, V_, R_ = 64, 1024, 37
CONFIGS = {"plain": (None, 0.0), "z+ignore": (-100, 1e-4)}
_HEAD = {}


def _head_case(mode, cfg, dev, exact_logits=False):
    """h, W (bf16-representable in the bf16 mode), targets, the float64 oracle and today's unfused path
    with its errors against the oracle; built once per (mode, cfg, exact_logits).

    exact_logits: h in {-2 .. 2} and W in {-1/4, 0, 1/4}. Every logit is then a multiple of 1/4 of
    magnitude at most 64 * 2 / 4 = 32, which has at most 8 significant bits: the bf16 head GEMM (exact
    products, fp32 sums, bf16 output) writes it without a rounding, so the logits the loss kernel reads
    are the oracle's own (standard deviation 2.3, about that of the random case)."""
    from cs744_pytorch_distributed_tutorial_amd.ops import lm
    key = (mode, cfg, exact_logits)
    if key in _HEAD:
        return _HEAD[key]
    ignore, z = CONFIGS[cfg]
    g_ = torch.Generator(device="cpu").manual_seed(21)
    h = torch.randn(R_, D_, generator=g_)
    W = torch.randn(V_, D_, generator=g_) * 0.3
    t = torch.randint(0, V_, (R_,), generator=g_)
    if ignore is not None:
        t[torch.rand(R_, generator=g_) < 0.3] = ignore
        t[8:16] = ignore  # with chunk_rows = 8 the second chunk holds ignored rows only
        t[36] = ignore  # and with chunk_rows = 36 so does the last, one-row chunk
    if exact_logits:
        h = torch.randint(-2, 3, (R_, D_), generator=g_).float()
        W = torch.randint(-1, 2, (V_, D_), generator=g_).float() / 4
    if mode == "bf16":
        h, W = h.bfloat16().float(), W.bfloat16().float()
    h, W, t = h.to(dev), W.to(dev), t.to(dev)
    rloss, rlse, rd, rmean, n = xent_masked_oracle(h.double() @ W.double().t(), t, ignore, z, G)
    ref = dict(loss=rmean, dh=rd @ W.double(), dW=rd.t() @ h.double(), lse=rlse, n=n)
    head = lm.ShadowLinear(D_, V_, bias=False).to(dev)
    with torch.no_grad():
        head.weight.copy_(W)
    hu = h.clone().requires_grad_()
    with _autocast(mode):
        loss = lm.cross_entropy(head(hu).view(-1, V_), t, ignore_index=ignore, z_loss=z)
    (G * loss).backward()
    unfused = dict(loss=loss.detach(), dh=hu.grad, dW=head.weight.grad.clone())
    head.weight.grad = None
    _HEAD[key] = (h, head, t, ref, unfused)
    return _HEAD[key]


def _autocast(mode):
    return torch.autocast("cuda", dtype=BF16, enabled=mode == "bf16")


def _err(x, ref):
    return float((x.double() - ref).abs().max() / ref.abs().max().clamp_min(1e-300))


def _run_fused(h, head, t, mode, ignore, z, chunk_rows, grad_h=True, grad_w=True):
    from cs744_pytorch_distributed_tutorial_amd.ops import lm
    hf = h.clone().requires_grad_(grad_h)
    head.weight.grad = None
    head.weight.requires_grad_(grad_w)
    try:
        with _autocast(mode):
            loss = lm.linear_cross_entropy(hf, head, t, ignore_index=ignore, z_loss=z, chunk_rows=chunk_rows)
        assert loss.dtype == F32 and loss.dim() == 0
        (G * loss).backward()
        dW = None if head.weight.grad is None else head.weight.grad.clone()
    finally:
        head.weight.grad = None
        head.weight.requires_grad_(True)
    return loss.detach(), hf.grad, dW


def _check_rule(tag, mode, got, ref, unfused, lse, z):
    loss, dh, dW = got
    bad = []
    # the loss by the same rule (test_linear_cross_entropy_loss_against_float64 asserts the absolute bound)
    tol = _scaled(XENT_LOSS_TOL, z, lse)
    lf, lu = abs(float(loss) - float(ref["loss"])), abs(float(unfused["loss"]) - float(ref["loss"]))
    if not lf <= 2 * lu + tol["atol"] + tol["rtol"] * abs(float(ref["loss"])):
        bad.append(("loss", lf, lu))
    # one rounding of the output dtype: dh leaves the bf16 GEMM in bf16 (fp32 mode: fp32), dW in fp32
    floors = {"dh": torch.finfo(BF16 if mode == "bf16" else F32).eps / 2, "dW": torch.finfo(F32).eps / 2}
    for name, x in (("dh", dh), ("dW", dW)):
        ef, eu = _err(x, ref[name]), _err(unfused[name], ref[name])
        print(f"[lm-head] {tag} {name}: fused {ef:.3e} unfused {eu:.3e} floor {floors[name]:.3e}")
        if not ef <= 2 * eu + floors[name]:
            bad.append((name, ef, eu))
    assert not bad, (tag, bad)


@pytest.mark.parametrize("chunk_rows", [1, 8, 36, 37, 64])
@pytest.mark.parametrize("cfg", list(CONFIGS))
@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_linear_cross_entropy_against_float64(dev, mode, cfg, chunk_rows):
    ignore, z = CONFIGS[cfg]
    h, head, t, ref, unfused = _head_case(mode, cfg, dev)
    got = _run_fused(h, head, t, mode, ignore, z, chunk_rows)
    assert got[1].dtype == F32 and got[1].shape == h.shape and got[2].dtype == F32 and got[2].shape == (V_, D_)
    _check_rule(f"linear_xent {mode} {cfg} chunk {chunk_rows}", mode, got, ref, unfused, ref["lse"], z)
    if ignore is not None:  # ignored rows take no gradient at all
        assert bool((got[1][t == ignore] == 0).all())
    again = _run_fused(h, head, t, mode, ignore, z, chunk_rows)
    assert all(torch.equal(a, b) for a, b in zip(got, again))  # two runs, the same bits


@pytest.mark.parametrize("chunk_rows", [1, 8, 36, 37, 64])
@pytest.mark.parametrize("cfg", list(CONFIGS))
@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_linear_cross_entropy_loss_against_float64(dev, mode, cfg, chunk_rows):
    """The loss of forward + backward (upstream gradient 2.5: xent_count, xent_fused_ per chunk,
    xent_reduce) within XENT_LOSS_TOL (scaled for z) of the float64 oracle: h and W as the kernels read
    them, the product and the loss in double. The forward-only path must give the same bits.

    In the bf16 mode the loss kernel reads the head GEMM's bf16 output, so the inputs are those whose
    logits bf16 holds exactly (_head_case(exact_logits=True)): the oracle's logits and the kernel's are
    then the same numbers, and the bound measures the loss arithmetic and the reduction over chunks, as it
    does in fp32. With random inputs the bf16 rounding of the logits alone (relative 2^-9 of values near
    +-7) moves the loss by 1.1e-3, for today's unfused path exactly as for the chunked one (measured on
    the MI355X: 1.109e-03 both, 1.384e-03 both with z and ignore); that rounding is covered by
    test_linear_cross_entropy_against_float64, which holds the chunked loss to twice the unfused path's
    error on random inputs."""
    from cs744_pytorch_distributed_tutorial_amd.ops import lm
    ignore, z = CONFIGS[cfg]
    h, head, t, ref, unfused = _head_case(mode, cfg, dev, exact_logits=mode == "bf16")
    if mode == "bf16":  # the premise: the bf16 logits are the oracle's
        with torch.no_grad(), _autocast(mode):
            assert head(h).dtype == BF16 and torch.equal(head(h).double(), h.double() @ head.weight.double().t())
    # forward + backward with the upstream gradient: the loss of xent_count + xent_fused_ + xent_reduce
    loss, dh, dW = _run_fused(h, head, t, mode, ignore, z, chunk_rows)
    assert dh is not None and dW is not None
    with torch.no_grad(), _autocast(mode):  # and the forward-only path (xent_fwd_masked per chunk): the same bits
        assert torch.equal(lm.linear_cross_entropy(h, head, t, ignore_index=ignore, z_loss=z, chunk_rows=chunk_rows),
                           loss)
    print(f"[lm-head] loss {mode} {cfg} chunk {chunk_rows}: |fused - f64| {abs(float(loss) - float(ref['loss'])):.3e} "
          f"|unfused - f64| {abs(float(unfused['loss']) - float(ref['loss'])):.3e}")
    rep = Report(f"linear_xent loss {mode} {cfg} chunk {chunk_rows}")
    rep.add("loss", loss, ref["loss"], **_scaled(XENT_LOSS_TOL, z, ref["lse"]))
    rep.done()


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_linear_cross_entropy_all_rows_ignored(dev, mode):
    h, head, t, _, _ = _head_case(mode, "z+ignore", dev)
    ta = torch.full_like(t, -100)
    loss, dh, dW = _run_fused(h, head, ta, mode, -100, 1e-4, 8)
    assert float(loss) == 0.0 and bool((dh == 0).all()) and bool((dW == 0).all())


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_linear_cross_entropy_views_and_partial_grads(dev, mode):
    from cs744_pytorch_distributed_tutorial_amd.ops import lm
    ignore, z = CONFIGS["z+ignore"]
    h, head, t, ref, unfused = _head_case(mode, "z+ignore", dev)
    base = _run_fused(h, head, t, mode, ignore, z, 8)
    # h as a contiguous view off the allocation's alignment, and as a column slice of a wider tensor
    wide = torch.zeros(R_, D_ + 8, device=dev)
    wide[:, 4:4 + D_] = h
    for hv in (offset_view(h), wide[:, 4:4 + D_], h.view(1, R_, D_)):
        assert hv.data_ptr() % 16 != 0 or not hv.is_contiguous() or hv.dim() == 3
        tv = t.view(1, R_) if hv.dim() == 3 else t
        hf = hv.detach().requires_grad_()
        head.weight.grad = None
        with _autocast(mode):
            loss = lm.linear_cross_entropy(hf, head, tv, ignore_index=ignore, z_loss=z, chunk_rows=8)
        (G * loss).backward()
        assert hf.grad.shape == hv.shape
        assert torch.equal(loss.detach(), base[0]) and torch.equal(hf.grad.reshape(R_, D_), base[1])
        assert torch.equal(head.weight.grad, base[2])
    head.weight.grad = None
    # only one of the two gradients asked for
    loss, dh, dW = _run_fused(h, head, t, mode, ignore, z, 8, grad_w=False)
    assert dW is None and torch.equal(loss, base[0]) and torch.equal(dh, base[1])
    loss, dh, dW = _run_fused(h, head, t, mode, ignore, z, 8, grad_h=False)
    assert dh is None and torch.equal(loss, base[0]) and torch.equal(dW, base[2])
    # no_grad: the loss alone, the same bits
    with torch.no_grad(), _autocast(mode):
        l0 = lm.linear_cross_entropy(h, head, t, ignore_index=ignore, z_loss=z, chunk_rows=8)
        nll, cnt = lm.linear_cross_entropy_sums(h, head, t, ignore_index=ignore, chunk_rows=8)
        logits = head(h)
        unll, ucnt = lm.cross_entropy_sums(logits.view(-1, V_), t, ignore_index=ignore)
    assert not l0.requires_grad and torch.equal(l0, base[0])
    assert int(cnt) == int(ucnt) == ref["n"] and cnt.dtype == torch.int64 and nll.dtype == torch.float64
    rep = Report(f"linear_xent sums {mode}")
    rep.add("nll_sum", nll, unll, **XENT_LOSS_TOL)
    rep.done()


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_odd_vocabulary_runs_the_reference(dev, mode, monkeypatch):
    from cs744_pytorch_distributed_tutorial_amd.ops import lm
    V = 1001
    g_ = torch.Generator(device="cpu").manual_seed(77)
    h = torch.randn(6, D_, generator=g_).to(dev)
    t = torch.randint(0, V, (6,), generator=g_).to(dev)
    t[0], t[4] = -100, -100
    head = lm.ShadowLinear(D_, V, bias=False).to(dev)
    calls = []
    ref = lm.linear_cross_entropy_ref
    monkeypatch.setattr(lm, "linear_cross_entropy_ref", lambda *a, **k: (calls.append(1), ref(*a, **k))[1])
    outs = []
    for fn in (lm.linear_cross_entropy, ref):
        hf = h.clone().requires_grad_()
        head.weight.grad = None
        with _autocast(mode):
            loss = fn(hf, head, t, ignore_index=-100, z_loss=1e-4)
        (G * loss).backward()
        outs.append((loss.detach(), hf.grad, head.weight.grad.clone()))
    assert calls == [1]
    assert all(torch.equal(a, b) for a, b in zip(*outs))
    # a bias goes the same way
    hb = torch.nn.Linear(D_, 1024, bias=True).to(dev)
    lm.linear_cross_entropy(h, hb, t, ignore_index=-100)
    assert calls == [1, 1]


# ------------------------------------------------------------------ 5. memory
def _peak_growth(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - before


def test_fused_head_never_holds_the_full_logits(dev):
    """D = 256, V = 32768, R = 4096 under bf16 autocast: the full logits are 268 MB. The fused path (a
    17 MB chunk, a 34 MB fp32 dW, dh) stays below one full logits matrix; today's path, the control
    that the meter works, holds the logits and their gradient: more than two."""
    from cs744_pytorch_distributed_tutorial_amd.ops import lm
    D, V, R = 256, 32768, 4096
    g_ = torch.Generator(device=dev).manual_seed(3)
    h = torch.randn(R, D, device=dev, generator=g_).bfloat16()
    t = torch.randint(0, V, (R,), device=dev, generator=g_)
    head = lm.ShadowLinear(D, V, bias=False).to(dev)
    head._shadow()
    full = R * V * 2

    def run(fused):
        hf = h.clone().requires_grad_()
        head.weight.grad = None
        with torch.autocast("cuda", dtype=BF16):
            if fused:
                loss = lm.linear_cross_entropy(hf, head, t, chunk_rows=256)
            else:
                loss = lm.cross_entropy(head(hf).view(-1, V), t)
        loss.backward()
        return loss.detach()

    losses, peaks = {}, {}
    for fused in (True, False):
        run(fused)  # warm-up: library workspaces are allocated once, outside the measurement
        head.weight.grad = None
        peaks[fused] = _peak_growth(lambda: losses.__setitem__(fused, run(fused)))
    print(f"[lm-head] memory: full logits {full / 1e6:.0f} MB, fused peak {peaks[True] / 1e6:.0f} MB, "
          f"unfused peak {peaks[False] / 1e6:.0f} MB")
    assert peaks[True] < full
    assert peaks[False] > 2 * full
    assert abs(float(losses[True]) - float(losses[False])) <= 1e-5 + 1e-5 * abs(float(losses[False]))


# ------------------------------------------------------------------ 6. model and trainer
def _loss64(logits, t, ignore, z):
    """the loss of xent_masked_oracle, differentiable, in float64"""
    V = logits.shape[-1]
    x, t = logits.reshape(-1, V), t.reshape(-1)
    valid = torch.ones_like(t, dtype=torch.bool) if ignore is None else t != ignore
    lse = torch.logsumexp(x, -1)
    rows = lse - x.gather(1, t.clamp(0, V - 1)[:, None])[:, 0] + z * lse * lse
    return torch.where(valid, rows, torch.zeros_like(rows)).sum() / max(int(valid.sum()), 1)


def _model64(model, monkeypatch):
    """a float64 copy of the model whose ops keep float64 (the package's CPU references compute in fp32)"""
    from cs744_pytorch_distributed_tutorial_amd.ops import attention, lm

    def rms(x, w, eps=1e-5):
        return x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps) * w

    theta = model.cfg.rope_theta

    def rope(x, cos, sin):  # the angle table again, in float64 (the model's is fp32)
        S, hd = x.shape[1], x.shape[-1]
        inv = 1.0 / (theta ** (torch.arange(0, hd, 2, device=x.device, dtype=torch.float64) / hd))
        ang = torch.outer(torch.arange(S, device=x.device, dtype=torch.float64), inv)
        xf = x.view(*x.shape[:-1], -1, 2)
        c, s = ang.cos()[None, :, None, :], ang.sin()[None, :, None, :]
        x0, x1 = xf[..., 0], xf[..., 1]
        return torch.stack([x0 * c - x1 * s, x0 * s + x1 * c], -1).view(x.shape)

    def attn(q, k, v, causal=True, doc=None):
        rep = q.shape[2] // k.shape[2]
        qf = q.transpose(1, 2)
        kf = k.repeat_interleave(rep, dim=2).transpose(1, 2)
        vf = v.repeat_interleave(rep, dim=2).transpose(1, 2)
        s = qf @ kf.transpose(-1, -2) / math.sqrt(q.shape[-1])
        s = s.masked_fill(~attention.doc_mask(doc).unsqueeze(1), float("-inf"))
        return (torch.softmax(s, -1) @ vf).transpose(1, 2)

    monkeypatch.setattr(lm, "rms_norm", rms)
    monkeypatch.setattr(lm, "swiglu", lambda a, b: torch.nn.functional.silu(a) * b)
    monkeypatch.setattr(lm, "rope", rope)
    monkeypatch.setattr(attention, "attention_ref", attn)
    m = copy.deepcopy(model).double()
    m._rope = None
    return m


MODEL_CASES = {"plain": (False, False, 0.0), "doc": (True, False, 0.0), "doc+mask+z": (True, True, 1e-4)}


@pytest.mark.parametrize("case", list(MODEL_CASES))
@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_model_loss_and_gradients(dev, mode, case, monkeypatch):
    from cs744_pytorch_distributed_tutorial_amd.models import llama
    from cs744_pytorch_distributed_tutorial_amd.ops import lm
    from cs744_pytorch_distributed_tutorial_amd.ops.attention import doc_ids_from_eos
    from cs744_pytorch_distributed_tutorial_amd.runtime.torch_trainer import SyntheticBatches
    use_doc, use_mask, z = MODEL_CASES[case]
    torch.manual_seed(0)
    model = llama.build("llama-tiny").to(dev)
    eos = model.cfg.eos_id
    data = SyntheticBatches("tokens", 4, dev, seq=64, vocab=1024, pool=4, seed=3, doc_len=16 if use_doc else None,
                            eos_id=eos if use_doc else None)
    x, y = data.next()
    doc_ids = doc_ids_from_eos(x, eos) if use_doc else None
    ignore = -100 if use_mask else None
    tm = lm.mask_boundary_targets(x, y, eos) if use_mask else y
    V = model.vocab_size
    names = [n for n, _ in model.named_parameters()]

    def grads():
        out = [p.grad.clone() for p in model.parameters()]
        model.zero_grad(set_to_none=True)
        return out

    with _autocast(mode):
        logits = model(x, doc_ids=doc_ids)
        lu = lm.cross_entropy(logits.view(-1, V), tm.view(-1), ignore_index=ignore, z_loss=z)
    lu.backward()
    gu = grads()
    with _autocast(mode):
        lf = model(x, doc_ids=doc_ids, targets=tm, ignore_index=ignore, z_loss=z)
    assert lf.dim() == 0 and lf.dtype == F32
    lf.backward()
    gf = grads()
    m64 = _model64(model, monkeypatch)
    l64 = _loss64(m64(x, doc_ids=doc_ids), tm, ignore, z)
    l64.backward()
    g64 = [p.grad for p in m64.parameters()]
    monkeypatch.undo()
    lu, lf, l64 = lu.detach(), lf.detach(), l64.detach()
    eu, ef = abs(float(lu) - float(l64)), abs(float(lf) - float(l64))
    tol = XENT_LOSS_TOL["atol"] + XENT_LOSS_TOL["rtol"] * abs(float(l64))
    print(f"[lm-head] model {mode} {case}: loss fused {float(lf):.6f} unfused {float(lu):.6f} float64 {float(l64):.6f}")
    assert ef <= 2 * eu + tol
    bad = []
    floor = torch.finfo(F32).eps / 2  # the parameters' gradients are fp32
    worst = None
    for n, a, b, r in zip(names, gf, gu, g64):
        e_f, e_u = _err(a, r), _err(b, r)
        if worst is None or e_f - 2 * e_u > worst[0] - 2 * worst[1]:
            worst = (e_f, e_u, n)
        if not e_f <= 2 * e_u + floor:
            bad.append((n, e_f, e_u))
    print(f"[lm-head] model {mode} {case}: closest to the bound {worst[2]}: fused {worst[0]:.3e} unfused {worst[1]:.3e}")
    assert not bad, bad


def _clear_env(monkeypatch):
    for k in ("CS744_OPTIMIZER", "CS744_LR", "CS744_WEIGHT_DECAY", "CS744_MAX_GRAD_NORM", "CS744_GRAD_COMM_DTYPE",
              "CS744_DOC_LEN", "CS744_LOSS_MASK", "CS744_Z_LOSS", "CS744_FUSED_HEAD", "CS_LM_HEAD_CHUNK_MB"):
        monkeypatch.delenv(k, raising=False)


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_trainer_with_fused_head(dev, dt, monkeypatch):
    """the 50-step AdamW case of tests/test_adamw_gpu.py test_llama_tiny_trains_with_adamw with the fused
    head, next to the unfused trainer at the same seed: first loss, that test's bound on the last
    losses, and evaluate()"""
    from cs744_pytorch_distributed_tutorial_amd.runtime.torch_trainer import SyntheticBatches, TorchTrainer
    _clear_env(monkeypatch)
    seed = 5000
    first, evals = {}, {}
    for fused in (True, False):
        tr = TorchTrainer("llama-tiny", 8, dev, dtype=dt, optimizer="adamw", lr=1e-3, weight_decay=0.1,
                          max_grad_norm=1.0, seq_len=32, seed=seed, fused_head=fused)
        assert tr.fused_head is fused
        tr.data = SyntheticBatches("tokens", 8, dev, seq=32, vocab=1024, pool=8, seed=seed)
        losses = []
        for _ in range(50 if fused else 1):
            tr.step()
            losses.append(tr.loss)
        losses = torch.stack(losses).float().cpu()
        first[fused] = float(losses[0])
        assert bool(torch.isfinite(losses).all())
        if fused:
            print(f"[lm-head] trainer {dt}: first {first[fused]:.4f} max(last 10) {float(losses[-10:].max()):.4f}")
            assert float(losses[-10:].max()) < 1.0
            assert float(tr.opt.last_grad_norm()) > 0
            # the same weights and the same batches through both evaluate() paths
            state = tr.data.gen.get_state()
            evals[True] = tr.evaluate(2)
            tr.data.gen.set_state(state)
            tr.fused_head = False
            evals[False] = tr.evaluate(2)
            tr.fused_head = True
    print(f"[lm-head] trainer {dt}: first loss fused {first[True]:.6f} unfused {first[False]:.6f}; evaluate {evals}")
    assert abs(first[True] - first[False]) <= XENT_LOSS_TOL["atol"] + XENT_LOSS_TOL["rtol"] * abs(first[False])
    assert evals[True]["tokens"] == evals[False]["tokens"] == 2 * 8 * 32
    assert abs(evals[True]["nll"] - evals[False]["nll"]) <= \
        XENT_LOSS_TOL["atol"] + XENT_LOSS_TOL["rtol"] * abs(evals[False]["nll"])


def test_trainer_switches(dev, monkeypatch):
    from cs744_pytorch_distributed_tutorial_amd.runtime.torch_trainer import TorchTrainer
    _clear_env(monkeypatch)
    assert TorchTrainer("llama-tiny", 2, dev, seq_len=16).fused_head is False
    monkeypatch.setenv("CS744_FUSED_HEAD", "1")
    tr = TorchTrainer("llama-tiny", 2, dev, dtype="bf16", seq_len=16, doc_len=8, loss_mask="doc", z_loss=1e-4)
    assert tr.fused_head is True
    tr.step()
    assert bool(torch.isfinite(tr.loss))
    assert TorchTrainer("llama-tiny", 2, dev, seq_len=16, fused_head=False).fused_head is False
    monkeypatch.delenv("CS744_FUSED_HEAD")
    for name in ("vgg11", "resnet18"):
        with pytest.raises(ValueError, match="fused_head"):
            TorchTrainer(name, 2, dev, fused_head=True)
