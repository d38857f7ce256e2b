"""The fused residual add + RMSNorm kernels (add_rmsnorm_fwd / add_rmsnorm_bwd, ops.lm.add_rms_norm)
against the two-kernel composition they replace, bit for bit where both round alike, and
Llama.fused_residual / TorchTrainer(fused_residual=True) against the plain blocks (MI355X only)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

EPS = 1e-5
# rows x D. 4-wide: the smallest row; DQ = 250 < 256 (idle lanes) and two backward blocks, the second
# with one row; the model's D with three backward blocks; kMaxQ full. Scalar: D % 4 != 0, and
# D % 4 == 0 above 8192
SHAPES_4 = [(1, 8), (17, 1000), (33, 4096), (5, 8192)]
SHAPES_S = [(3, 9), (4, 1002), (2, 8196)]
SHAPES = SHAPES_4 + SHAPES_S
# (x dtype, delta dtype, bf16 autocast): (a) the model's case, (b) all fp32, (c) all bf16
F32, BF16 = torch.float32, torch.bfloat16
CASES = {"a": (F32, BF16, True), "b": (F32, F32, False), "c": (BF16, BF16, False)}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cs744_pytorch_distributed_tutorial_amd.ops import native
    native.C()
    return torch.device("cuda", 0)


def _ctx(autocast):
    return torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast)


def _inputs(dev, rows, D, case, seed=0):
    xdt, ddt, autocast = CASES[case]
    g = torch.Generator(device=dev).manual_seed(seed)
    x = torch.randn(rows, D, device=dev, generator=g).to(xdt)
    d = torch.randn(rows, D, device=dev, generator=g).to(ddt)
    w = torch.rand(D, device=dev, generator=g) + 0.5
    gh = torch.randn(rows, D, device=dev, generator=g).to(xdt)
    gy = torch.randn(rows, D, device=dev, generator=g)  # cast to y's dtype by the caller
    return x, d, w, gh, gy, autocast


def _run(x, d, w, autocast, gh, gy, req=(True, True)):
    """ops.lm.add_rms_norm forward and backward -> h, y, (dx, ddelta, dw)"""
    from cs744_pytorch_distributed_tutorial_amd.ops import lm
    # detach, not clone: an offset view stays the view it is
    xa, da, wa = x.detach().requires_grad_(req[0]), d.detach().requires_grad_(req[1]), w.detach().requires_grad_()
    with _ctx(autocast):
        h, y = lm.add_rms_norm(xa, da, wa, EPS)
    outs, grads = ([y], [gy.to(y.dtype)]) if gh is None else ([h, y], [gh, gy.to(y.dtype)])
    torch.autograd.backward(outs, grads)
    return h.detach(), y.detach(), (xa.grad, da.grad, wa.grad)


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("rows,D", SHAPES)
def test_forward_is_add_then_rms_norm(dev, rows, D, case):
    from cs744_pytorch_distributed_tutorial_amd import _C
    from cs744_pytorch_distributed_tutorial_amd.ops import lm
    x, d, w, _, _, autocast = _inputs(dev, rows, D, case)
    with _ctx(autocast):
        h, y = lm.add_rms_norm(x, d, w, EPS)
        ry = lm.rms_norm(x + d, w, EPS)
    assert h.dtype == x.dtype and torch.equal(h, x + d)
    vec4 = _C.rmsnorm_vec4(D)
    assert y.dtype == (BF16 if autocast and vec4 else x.dtype)
    assert y.dtype == ry.dtype and torch.equal(y, ry)
    # rstd through the bindings (the scalar kernels take delta in x's dtype)
    out_bf16 = y.dtype == BF16
    h2, y2, rstd = _C.add_rmsnorm_fwd(x, d if vec4 else d.to(x.dtype), w, EPS, out_bf16)
    ry2, rrstd = _C.rmsnorm_fwd(h, w, EPS, out_bf16)
    assert rstd.shape == (rows,) and torch.equal(rstd, rrstd)
    assert torch.equal(h2, h) and torch.equal(y2, y) and torch.equal(y2, ry2)


@pytest.mark.parametrize("case", ["a", "b"])
@pytest.mark.parametrize("rows,D", SHAPES)
def test_backward_fp32_stream_bit_equal_to_the_composition(dev, rows, D, case):
    from cs744_pytorch_distributed_tutorial_amd import _C
    x, d, w, gh, gy, autocast = _inputs(dev, rows, D, case, seed=1)
    h, y, (dx, dd, dw) = _run(x, d, w, autocast, gh, gy)
    _, rstd = _C.rmsnorm_fwd(h, w, EPS, y.dtype == BF16)
    rdx, rdw = _C.rmsnorm_bwd(h, w, rstd, gy.to(y.dtype))
    assert dx.dtype == F32 and dd.dtype == d.dtype and dw.dtype == F32
    assert torch.equal(dw, rdw)
    assert torch.equal(dx, gh + rdx)
    assert torch.equal(dd, dx.to(d.dtype))
    if _C.rmsnorm_vec4(D):  # the binding itself, both copies written by the kernel
        bdx, bdd, bdw = _C.add_rmsnorm_bwd(h, w, rstd, gy.to(y.dtype), gh, d.dtype, True, True)
        assert torch.equal(bdx, dx) and torch.equal(bdd, dd) and torch.equal(bdw, dw) and bdd.dtype == d.dtype
        assert (bdd.data_ptr() == bdx.data_ptr()) == (d.dtype == F32)  # one stored gradient where the dtypes agree
        only_dd = _C.add_rmsnorm_bwd(h, w, rstd, gy.to(y.dtype), gh, d.dtype, False, True)
        assert only_dd[0] is None and torch.equal(only_dd[1], dd) and torch.equal(only_dd[2], dw)
        only_dw = _C.add_rmsnorm_bwd(h, w, rstd, gy.to(y.dtype), gh, d.dtype, False, False)
        assert only_dw[0] is None and only_dw[1] is None and torch.equal(only_dw[2], dw)


@pytest.mark.parametrize("rows,D", SHAPES)
def test_backward_bf16_stream(dev, rows, D):
    """the fused kernel rounds gh + dx once, the composition twice: against the fp32 autograd gradients
    of the reference at the bf16 tolerances of tests/test_lm_gpu.py::test_rmsnorm; dw stays bit-equal
    to the unfused kernel's"""
    from cs744_pytorch_distributed_tutorial_amd import _C
    from cs744_pytorch_distributed_tutorial_amd.ops import lm
    x, d, w, gh, gy, autocast = _inputs(dev, rows, D, "c", seed=2)
    h, y, (dx, dd, dw) = _run(x, d, w, autocast, gh, gy)
    assert dx.dtype == BF16 and dd.dtype == BF16 and torch.equal(dx, dd)
    _, rstd = _C.rmsnorm_fwd(h, w, EPS, True)
    assert torch.equal(dw, _C.rmsnorm_bwd(h, w, rstd, gy.to(BF16))[1])
    ins = [t.detach().float().requires_grad_() for t in (x, d, w)]
    rh, ry = lm.add_rms_norm_ref(*ins, EPS)
    torch.autograd.backward([rh, ry], [gh.float(), gy.to(BF16).float()])
    torch.testing.assert_close(dx.float(), ins[0].grad, rtol=2e-2, atol=2e-2)
    torch.testing.assert_close(dd.float(), ins[1].grad, rtol=2e-2, atol=2e-2)
    torch.testing.assert_close(dw.float(), ins[2].grad, rtol=2e-2, atol=5e-2)


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("rows,D", [(17, 1000), (4, 1002)])
def test_absent_gh_and_inputs_without_grad(dev, rows, D, case):
    x, d, w, gh, gy, autocast = _inputs(dev, rows, D, case, seed=3)
    h, y, full = _run(x, d, w, autocast, gh, gy)
    # only y used: the same gradients as a zero gradient of h
    _, _, none = _run(x, d, w, autocast, None, gy)
    _, _, zero = _run(x, d, w, autocast, torch.zeros_like(gh), gy)
    for a, b in zip(none, zero):
        assert a is not None and torch.equal(a, b)
    # an input that asks for no gradient gets none, the others are what they were
    _, _, no_d = _run(x, d, w, autocast, gh, gy, req=(True, False))
    assert no_d[1] is None and torch.equal(no_d[0], full[0]) and torch.equal(no_d[2], full[2])
    _, _, no_x = _run(x, d, w, autocast, gh, gy, req=(False, True))
    assert no_x[0] is None and torch.equal(no_x[1], full[1]) and torch.equal(no_x[2], full[2])
    _, _, no_xd = _run(x, d, w, autocast, gh, gy, req=(False, False))
    assert no_xd[0] is None and no_xd[1] is None and torch.equal(no_xd[2], full[2])


def _offset_view(t):
    """the same values as a contiguous view one element into a fresh allocation: not 16-byte aligned"""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 != 0
    return v


@pytest.mark.parametrize("case", list(CASES))
def test_offset_views(dev, case):
    from cs744_pytorch_distributed_tutorial_amd import _C
    rows, D = 17, 1000
    x, d, w, gh, gy, autocast = _inputs(dev, rows, D, case, seed=4)
    h, y, grads = _run(x, d, w, autocast, gh, gy)
    gyc = gy.to(y.dtype)
    oh, oy, ograds = _run(_offset_view(x), _offset_view(d), _offset_view(w), autocast, _offset_view(gh),
                          _offset_view(gyc))
    assert torch.equal(oh, h) and torch.equal(oy, y)
    for a, b in zip(ograds, grads):
        assert torch.equal(a, b)
    # the bindings refuse what the 4-wide kernels cannot read
    _, rstd = _C.rmsnorm_fwd(h, w, EPS, y.dtype == BF16)
    for i in range(3):
        args = [x, d, w]
        args[i] = _offset_view(args[i])
        with pytest.raises(RuntimeError, match="aligned"):
            _C.add_rmsnorm_fwd(*args, EPS, y.dtype == BF16)
    for i in (0, 1, 3, 4):
        args = [h, w, rstd, gyc, gh]
        args[i] = _offset_view(args[i])
        with pytest.raises(RuntimeError, match="aligned"):
            _C.add_rmsnorm_bwd(*args, d.dtype, True, True)


@pytest.mark.parametrize("D", [8, 9])
def test_no_rows(dev, D):
    from cs744_pytorch_distributed_tutorial_amd import _C
    x = torch.empty(0, D, device=dev)
    w = torch.ones(D, device=dev)
    h, y, rstd = _C.add_rmsnorm_fwd(x, x, w, EPS, False)
    assert h.shape == (0, D) and y.shape == (0, D) and rstd.shape == (0,)
    dx, dd, dw = _C.add_rmsnorm_bwd(h, w, rstd, y, None, F32, True, True)
    assert dx.shape == (0, D) and dd.shape == (0, D) and torch.equal(dw, torch.zeros_like(w))
    oh, oy, (gx, gd, gw) = _run(x, x, w, False, x, x)
    assert oh.shape == (0, D) and oy.shape == (0, D) and gx.shape == (0, D) and gd.shape == (0, D)
    assert torch.equal(gw, torch.zeros_like(w))


@pytest.mark.parametrize("D", [9, 8196])
def test_binding_refuses_mixed_dtypes_on_scalar_path(dev, D):
    from cs744_pytorch_distributed_tutorial_amd import _C
    x = torch.randn(2, D, device=dev)
    w = torch.ones(D, device=dev)
    assert not _C.rmsnorm_vec4(D)
    with pytest.raises(RuntimeError, match="mixed dtypes"):
        _C.add_rmsnorm_fwd(x, x.bfloat16(), w, EPS, False)
    with pytest.raises(RuntimeError, match="bf16 output"):
        _C.add_rmsnorm_fwd(x, x, w, EPS, True)
    h, y, rstd = _C.add_rmsnorm_fwd(x, x, w, EPS, False)
    with pytest.raises(RuntimeError, match="mixed dtypes"):
        _C.add_rmsnorm_bwd(h, w, rstd, y.bfloat16(), None, F32, True, True)
    with pytest.raises(RuntimeError, match="mixed dtypes"):
        _C.add_rmsnorm_bwd(h, w, rstd, y, None, BF16, True, True)
    with pytest.raises(RuntimeError, match="gh must match"):
        _C.add_rmsnorm_bwd(h, w, rstd, y, x.bfloat16(), F32, True, True)
    with pytest.raises(RuntimeError, match="one shape"):
        _C.add_rmsnorm_fwd(x, x[:1], w, EPS, False)
    torch.cuda.synchronize()


# ------------------------------------------------------------------ model and trainer
def _model_grads(model, fused, mode, tok, tgt, doc_ids):
    from cs744_pytorch_distributed_tutorial_amd.ops import lm
    model.fused_residual = fused
    model.zero_grad(set_to_none=True)
    with _ctx(True):
        if mode == "targets":
            loss = model(tok, targets=tgt)
        else:
            logits = model(tok, doc_ids=doc_ids if mode == "doc_ids" else None)
            loss = lm.cross_entropy(logits.view(-1, logits.shape[-1]), tgt.view(-1))
    loss.backward()
    return loss.detach().clone(), {n: p.grad.clone() for n, p in model.named_parameters()}


@pytest.mark.parametrize("mode", ["logits", "doc_ids", "targets"])
def test_llama_tiny_fused_residual_bit_equal(dev, mode):
    """llama-tiny under bf16 autocast, 2 x 32 tokens, the same weights: the switch changes no bit of the
    loss or of a parameter gradient. A gradient that two unfused runs do not reproduce bit for bit is
    compared at rtol 1e-5, atol 1e-6 instead (and named in the output)."""
    from cs744_pytorch_distributed_tutorial_amd.models import llama
    from cs744_pytorch_distributed_tutorial_amd.ops.attention import doc_ids_from_eos
    torch.manual_seed(0)
    model = llama.build("llama-tiny").to(dev)
    g = torch.Generator(device=dev).manual_seed(1)
    tok = torch.randint(0, model.vocab_size - 1, (2, 32), device=dev, generator=g)
    tok[0, 9] = tok[1, 20] = model.cfg.eos_id
    tgt = torch.randint(0, model.vocab_size, (2, 32), device=dev, generator=g)
    doc_ids = doc_ids_from_eos(tok, model.cfg.eos_id)
    keys = list(model.state_dict().keys())
    l0, g0 = _model_grads(model, False, mode, tok, tgt, doc_ids)
    l1, g1 = _model_grads(model, False, mode, tok, tgt, doc_ids)
    lf, gf = _model_grads(model, True, mode, tok, tgt, doc_ids)
    assert list(model.state_dict().keys()) == keys
    assert torch.isfinite(lf) and torch.equal(l0, l1) and torch.equal(lf, l0)
    loose = [n for n in g0 if not torch.equal(g0[n], g1[n])]
    print(f"[add-rmsnorm] model {mode}: loss {float(lf):.6f}; not bit-reproducible between two unfused runs: {loose}")
    for n in g0:
        if n in loose:
            torch.testing.assert_close(gf[n], g0[n], rtol=1e-5, atol=1e-6)
        else:
            assert torch.equal(gf[n], g0[n]), n
    assert float(gf["layers.0.ffn_norm.weight"].abs().sum()) > 0 and float(gf["norm.weight"].abs().sum()) > 0


def test_trainer_with_fused_residual(dev, monkeypatch):
    """three AdamW steps with the switch on and off at the same seed: the same losses step by step (exactly
    where two unfused runs agree exactly, else at rtol 1e-5, atol 1e-6), and a falling loss. lr is set:
    at the trainer's default, SGD's 0.1, AdamW's loss rises from the first step on either path."""
    from cs744_pytorch_distributed_tutorial_amd.runtime.torch_trainer import TorchTrainer
    for k in ("CS744_OPTIMIZER", "CS744_LR", "CS744_WEIGHT_DECAY", "CS744_MAX_GRAD_NORM", "CS744_GRAD_COMM_DTYPE",
              "CS744_DOC_LEN", "CS744_LOSS_MASK", "CS744_Z_LOSS", "CS744_FUSED_HEAD", "CS744_FUSED_RESIDUAL",
              "CS_LM_HEAD_CHUNK_MB"):
        monkeypatch.delenv(k, raising=False)
    runs = []
    for fused in (False, False, True):
        tr = TorchTrainer("llama-tiny", 8, dev, dtype="bf16", optimizer="adamw", lr=1e-3, seq_len=32,
                          fused_residual=fused)
        assert tr.fused_residual is fused and tr.module.fused_residual is fused
        losses = []
        for _ in range(3):
            tr.step()
            losses.append(tr.loss)
        runs.append(torch.stack(losses).float().cpu())
    a, b, f = runs
    print(f"[add-rmsnorm] trainer losses unfused {a.tolist()} again {b.tolist()} fused {f.tolist()}")
    assert bool(torch.isfinite(f).all())
    for i in range(3):
        if torch.equal(a[i], b[i]):
            assert torch.equal(f[i], a[i]), i
        else:
            torch.testing.assert_close(f[i], a[i], rtol=1e-5, atol=1e-6)
    assert float(f[2]) < float(f[0])
