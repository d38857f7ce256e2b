"""``ops.optim.FusedAdamW`` (adamw.hip: multi-tensor AdamW + deterministic global-norm clipping) on
the MI355X: against ``torch.optim.AdamW`` in float64 with torch's own float32 AdamW on the same
device as the yardstick, clipping against ``clip_grad_norm_``, determinism, bf16 shadows, ``lr``
changes, a short training run through the trainer, and the table builder's host checks.

The yardstick rule (every numeric comparison here): with e(x) the maximum over a tensor of
``|p - p64| / lr``, ``|m - m64| / max|m64|`` and ``|v - v64| / max|v64|``, the fused result must have
e <= 2 * e(torch float32 arm), plus one ulp of the largest parameter over ``lr`` for ``p``. The factor 2
allows a different but equally valid rounding order; nothing in the bound comes from the fused code."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

LR, BETAS, EPS, WD = 1e-3, (0.9, 0.95), 1e-8, 0.1


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cs744_pytorch_distributed_tutorial_amd.ops import native
    native.C()
    return torch.device("cuda", 0)


def _fused(groups, **kw):
    from cs744_pytorch_distributed_tutorial_amd.ops.optim import FusedAdamW
    return FusedAdamW(groups, lr=LR, betas=BETAS, eps=EPS, weight_decay=WD, **kw)


def _torch(groups):
    return torch.optim.AdamW(groups, lr=LR, betas=BETAS, eps=EPS, weight_decay=WD)


def _params(init, dtype=torch.float32):
    return [torch.nn.Parameter(t.detach().to(dtype).clone()) for t in init]


def _groups(ps, wd=WD):
    """decay on the matrices only, as the trainer groups them"""
    return [{"params": [p for p in ps if p.dim() >= 2], "weight_decay": wd},
            {"params": [p for p in ps if p.dim() < 2], "weight_decay": 0.0}]


def _grads_like(init, gen, mag=True):
    """randn * 10**randint(-4, 1) per element with about 1 % exact zeros, laid out like the parameter"""
    out = []
    for t in init:
        g = torch.randn(t.shape, generator=gen, device=t.device)
        if mag:
            g = g * 10.0 ** torch.randint(-4, 2, t.shape, generator=gen, device=t.device).float()
        g = g * (torch.rand(t.shape, generator=gen, device=t.device) >= 0.01)
        out.append(torch.empty_like(t).copy_(g))
    return out


def _set_grads(ps, gs, dtype=torch.float32):
    for p, g in zip(ps, gs):
        p.grad = None if g is None else g.to(dtype).clone()


def _steps(opt, ps, grad_steps, dtype=torch.float32, clip=None):
    for gs in grad_steps:
        _set_grads(ps, gs, dtype)
        if clip is not None:
            torch.nn.utils.clip_grad_norm_([p for p in ps if p.grad is not None], clip)
        opt.step()


def _metrics(p, st, p64, st64):
    m64, v64 = st64["exp_avg"], st64["exp_avg_sq"]
    return (float((p.detach().double() - p64.detach()).abs().max()) / LR,
            float((st["exp_avg"].double() - m64).abs().max() / m64.abs().max()),
            float((st["exp_avg_sq"].double() - v64).abs().max() / v64.abs().max()))


def _check_rule(tag, fused, ref32, ref64, names=None):
    """fused / ref32 / ref64: (params, optimizer). The yardstick rule, per parameter tensor."""
    bad = []
    for i, (pf, pt, pd) in enumerate(zip(fused[0], ref32[0], ref64[0])):
        if pd not in ref64[1].state:
            continue
        ef = _metrics(pf, fused[1].state[pf], pd, ref64[1].state[pd])
        et = _metrics(pt, ref32[1].state[pt], pd, ref64[1].state[pd])
        ulp = float(np.spacing(np.float32(float(pd.detach().abs().max())))) / LR
        name = names[i] if names else f"n={pf.numel()}"
        print(f"[adamw-numerics] {tag} {name}: fused p {ef[0]:.3e} m {ef[1]:.3e} v {ef[2]:.3e} | "
              f"torch32 p {et[0]:.3e} m {et[1]:.3e} v {et[2]:.3e} | ulp/lr {ulp:.3e}")
        if not (ef[0] <= 2 * et[0] + ulp and ef[1] <= 2 * et[1] and ef[2] <= 2 * et[2]):
            bad.append((name, ef, et, ulp))
    assert not bad, bad


# ------------------------------------------------------------------ 1. kernel against fp64
SIZES = (1, 7, 4095, 4096, 4097, 1_000_003)


def test_kernel_against_fp64(dev):
    """One table of six tensors whose sizes cover the chunk edges and the vector tails, 5 steps; the rule
    is asserted per tensor."""
    gen = torch.Generator(device=dev).manual_seed(11)
    init = [torch.randn(n, generator=gen, device=dev) for n in SIZES]
    steps = [_grads_like(init, gen) for _ in range(5)]
    arms = []
    for dtype, make in ((torch.float32, lambda ps: _fused([{"params": ps}])),
                        (torch.float32, lambda ps: _torch([{"params": ps}])),
                        (torch.float64, lambda ps: _torch([{"params": ps}]))):
        ps = _params(init, dtype)
        opt = make(ps)
        _steps(opt, ps, steps, dtype)
        arms.append((ps, opt))
    assert all(int(arms[0][1].state[p]["step"]) == 5 for p in arms[0][0])
    _check_rule("kernel", *arms)


def test_unaligned_views_take_the_scalar_loop_with_the_same_bits(dev):
    """a parameter (or only its gradient) that is a view at an odd element offset cannot be read 16 bytes
    at a time: the scalar loop runs for that entry and gives the bits of the vector loop"""
    gen = torch.Generator(device=dev).manual_seed(12)
    n = 4096 + 4099
    init = [torch.randn(n, generator=gen, device=dev) for _ in range(3)]
    steps = [_grads_like(init, gen) for _ in range(2)]
    ref = _params(init)
    opt = _fused([{"params": ref}], max_grad_norm=1.0)
    _steps(opt, ref, steps)
    bufs = [torch.zeros(n + 1, device=dev) for _ in range(3)]
    ps = [torch.nn.Parameter(bufs[0][1:]), torch.nn.Parameter(bufs[1][:n]), torch.nn.Parameter(bufs[2][:n])]
    assert ps[0].data_ptr() % 16 == 4
    with torch.no_grad():
        for p, t in zip(ps, init):
            p.copy_(t)
    opt2 = _fused([{"params": ps}], max_grad_norm=1.0)
    for gs in steps:
        gbuf = torch.zeros(n + 1, device=dev)
        gbuf[1:].copy_(gs[1])
        ps[0].grad, ps[1].grad, ps[2].grad = gs[0].clone(), gbuf[1:], gs[2].clone()  # [1]: only g is unaligned
        opt2.step()
    assert torch.equal(opt.last_grad_norm(), opt2.last_grad_norm())
    for a, b in zip(ref, ps):
        assert torch.equal(a, b)
        assert torch.equal(opt.state[a]["exp_avg"], opt2.state[b]["exp_avg"])
        assert torch.equal(opt.state[a]["exp_avg_sq"], opt2.state[b]["exp_avg_sq"])
    assert float(bufs[0][0]) == 0 and float(bufs[1][n]) == 0  # the neighbours of the views are untouched


# ------------------------------------------------------------------ 2. optimizer against torch, whole model
@pytest.fixture(scope="module")
def model_init(dev):
    """llama-tiny's parameters + one 4-D channels-last tensor + one parameter that never gets a gradient"""
    from cs744_pytorch_distributed_tutorial_amd.models import llama
    torch.manual_seed(21)
    m = llama.build("llama-tiny").to(dev)
    names = [n for n, _ in m.named_parameters()] + ["conv_channels_last", "no_grad"]
    init = [p.detach().clone() for p in m.parameters()]
    init.append(torch.randn(8, 4, 3, 3, device=dev).contiguous(memory_format=torch.channels_last))
    init.append(torch.randn(5, 3, device=dev))
    return names, init


def _model_grads(init, gen, **kw):
    gs = _grads_like(init[:-1], gen, **kw)
    assert gs[-1].stride() == init[-2].stride() and not gs[-1].is_contiguous()
    return gs + [None]


def test_whole_model_against_torch_and_state_dict_both_ways(dev, model_init):
    names, init = model_init
    gen = torch.Generator(device=dev).manual_seed(22)
    steps = [_model_grads(init, gen) for _ in range(4)]
    arms = []
    for dtype, make in ((torch.float32, _fused), (torch.float32, _torch), (torch.float64, _torch)):
        ps = _params(init, dtype)
        opt = make(_groups(ps))
        _steps(opt, ps, steps[:3], dtype)
        arms.append((ps, opt))
    (pf, of), (pt, ot), _ = arms
    assert of.param_groups[1]["weight_decay"] == 0 and of.param_groups[0]["weight_decay"] == WD
    assert torch.equal(pf[-1], init[-1]) and pf[-1] not in of.state  # grad None: untouched, no state
    st = of.state[pf[-2]]
    assert st["exp_avg"].stride() == pf[-2].stride() and torch.is_tensor(st["step"]) and int(st["step"]) == 3
    assert set(st) == {"step", "exp_avg", "exp_avg_sq"}
    _check_rule("model", *arms, names=names)
    # either state loads into the other; one more step from the swapped states agrees the same way
    sf, st_ = of.state_dict(), ot.state_dict()
    assert len(sf["state"]) == len(st_["state"]) == len(init) - 1
    of.load_state_dict(st_)
    ot.load_state_dict(sf)
    for (ps, opt), dtype in zip(arms, (torch.float32, torch.float32, torch.float64)):
        _steps(opt, ps, steps[3:], dtype)
    assert int(of.state[pf[0]]["step"]) == 4 and torch.equal(pf[-1], init[-1])
    _check_rule("model-swapped", *arms, names=names)


# ------------------------------------------------------------------ 3. clipping
MAX_NORM = 1.0


def _scaled_grads(init, gen, norm):
    gs = _model_grads(init, gen, mag=False)
    tot = torch.linalg.vector_norm(torch.cat([g.double().reshape(-1) for g in gs if g is not None]))
    return [None if g is None else (g * (norm / tot).float()) for g in gs]


def _flat(ps, opt):
    out = [p.detach().reshape(-1) for p in ps]
    for p in ps:
        if p in opt.state:
            out += [opt.state[p]["exp_avg"].reshape(-1), opt.state[p]["exp_avg_sq"].reshape(-1)]
    return torch.cat(out)


def test_clip_norm_and_update_against_torch(dev, model_init):
    names, init = model_init
    gen = torch.Generator(device=dev).manual_seed(31)
    steps = [_scaled_grads(init, gen, 50 * MAX_NORM) for _ in range(3)]
    arms = []
    for dtype, make, clip in ((torch.float32, lambda g: _fused(g, max_grad_norm=MAX_NORM), None),
                              (torch.float32, _torch, MAX_NORM), (torch.float64, _torch, MAX_NORM)):
        ps = _params(init, dtype)
        opt = make(_groups(ps))
        _steps(opt, ps, steps, dtype, clip=clip)
        arms.append((ps, opt))
    _check_rule("clip", *arms, names=names)
    cat = torch.cat([g.reshape(-1) for g in steps[-1] if g is not None])
    n64 = float(torch.linalg.vector_norm(cat.double()))
    e32 = abs(float(torch.linalg.vector_norm(cat)) - n64) / n64
    got = arms[0][1].last_grad_norm()
    assert got.is_cuda and got.dtype == torch.float32 and got.numel() == 1
    ef = abs(float(got) - n64) / n64
    print(f"[adamw-numerics] norm: fp64 {n64:.9g} fused rel err {ef:.3e} | torch32 vector_norm rel err {e32:.3e}")
    assert 49 < n64 < 51
    assert ef <= 2 * e32 + 1e-7


def test_clip_is_exact_identity_below_the_bound_and_handles_zero_gradients(dev, model_init):
    _, init = model_init
    gen = torch.Generator(device=dev).manual_seed(32)
    steps = [_scaled_grads(init, gen, 0.5 * MAX_NORM) for _ in range(2)]
    res = []
    for kw in ({"max_grad_norm": MAX_NORM}, {}):
        ps = _params(init)
        opt = _fused(_groups(ps), **kw)
        _steps(opt, ps, steps)
        res.append((_flat(ps, opt), opt.last_grad_norm()))
    assert torch.equal(res[0][0], res[1][0])  # coefficient exactly 1
    assert res[1][1] is None and abs(float(res[0][1]) - 0.5) < 1e-5
    ps = _params(init)
    opt = _fused(_groups(ps), max_grad_norm=MAX_NORM)
    _steps(opt, ps, [[None if g is None else torch.zeros_like(g) for g in steps[0]]])
    assert float(opt.last_grad_norm()) == 0.0
    assert all(bool(torch.isfinite(p).all()) for p in ps)
    # zero gradient: only the decay moves a parameter
    assert torch.equal(ps[0].detach(), init[0] * np.float32(1 - LR * WD)) and torch.equal(ps[-2].detach(), init[-2] * np.float32(1 - LR * WD))


def test_grad_scale_equals_halving_the_gradients(dev, model_init):
    _, init = model_init
    gen = torch.Generator(device=dev).manual_seed(33)
    steps = [_scaled_grads(init, gen, 50 * MAX_NORM) for _ in range(2)]
    half = [[None if g is None else g * 0.5 for g in gs] for gs in steps]
    res = []
    for kw, st in (({"grad_scale": 0.5}, steps), ({}, half)):
        ps = _params(init)
        opt = _fused(_groups(ps), max_grad_norm=MAX_NORM, **kw)
        _steps(opt, ps, st)
        res.append((_flat(ps, opt), opt.last_grad_norm().clone()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    assert abs(float(res[0][1]) - 25.0) < 1e-3  # the norm is reported after grad_scale


def test_clip_is_global_over_groups(dev, model_init):
    """the same parameters in 1, 2 or 3 groups (same order, same hyper-parameters): one norm over all of
    them, so the same bits"""
    _, init = model_init
    gen = torch.Generator(device=dev).manual_seed(34)
    steps = [_scaled_grads(init, gen, 50 * MAX_NORM) for _ in range(2)]
    res = []
    for cuts in ((), (7,), (3, 12)):
        ps = _params(init)
        edges = (0, *cuts, len(ps))
        opt = _fused([{"params": ps[a:b]} for a, b in zip(edges[:-1], edges[1:])], max_grad_norm=MAX_NORM)
        assert len(opt.param_groups) == len(cuts) + 1
        _steps(opt, ps, steps)
        res.append((_flat(ps, opt), opt.last_grad_norm().clone()))
    for r in res[1:]:
        assert torch.equal(r[0], res[0][0]) and torch.equal(r[1], res[0][1])


# ------------------------------------------------------------------ 4. determinism
def test_clipped_steps_are_deterministic(dev, model_init):
    _, init = model_init
    gen = torch.Generator(device=dev).manual_seed(41)
    steps = [_scaled_grads(init, gen, 50 * MAX_NORM) for _ in range(3)]
    res = []
    for _ in range(2):
        ps = _params(init)
        opt = _fused(_groups(ps), max_grad_norm=MAX_NORM)
        norms = []
        for gs in steps:
            _steps(opt, ps, [gs])
            norms.append(opt.last_grad_norm().clone())
        res.append(torch.cat([_flat(ps, opt), torch.stack(norms).reshape(-1)]))
    assert torch.equal(res[0], res[1])


# ------------------------------------------------------------------ 5. shadows
def test_adamw_keeps_bf16_shadows(dev):
    """the AdamW twin of the FusedSGD shadow check: the update rewrites the bf16 copy of a ShadowLinear
    weight (bit-equal to a fresh cast) and the next autocast forward reuses the same object"""
    from cs744_pytorch_distributed_tutorial_amd.ops.lm import ShadowLinear
    torch.manual_seed(5)
    layers = [ShadowLinear(256, 384, bias=False).to(dev) for _ in range(2)]
    x = torch.randn(2, 64, 256, device=dev)
    gy = torch.randn(2, 64, 384, device=dev).bfloat16()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        ys = [l(x) for l in layers]
    for y in ys:
        y.backward(gy)
    w0 = [l.weight.detach().clone() for l in layers]
    opt = _fused([{"params": [l.weight for l in layers]}], max_grad_norm=MAX_NORM)
    opt.step()
    shs = [l.weight._cs_bf16_shadow for l in layers]
    for l, sh, w in zip(layers, shs, w0):
        assert not torch.equal(l.weight.detach(), w)
        assert torch.equal(sh, l.weight.detach().to(torch.bfloat16))
    with torch.autocast("cuda", dtype=torch.bfloat16):
        for l in layers:
            l(x)
    assert all(l.weight._cs_bf16_shadow is sh for l, sh in zip(layers, shs))


# ------------------------------------------------------------------ 6. lr changes apply
def test_group_lr_is_read_every_step_without_a_table_rebuild(dev):
    gen = torch.Generator(device=dev).manual_seed(61)
    init = [torch.randn(300, 70, generator=gen, device=dev), torch.randn(4097, generator=gen, device=dev)]
    ps = _params(init)
    opt = _fused(_groups(ps))
    gs = _grads_like(init, gen)
    _set_grads(ps, gs)  # the same gradient tensors stay attached: the pointer set does not change
    opt.step()
    table = opt._table
    assert table is not None
    p1 = [p.detach().clone() for p in ps]
    mv1 = [(opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone()) for p in ps]
    for g in opt.param_groups:
        g["lr"] = 0.0
    opt.step()
    assert opt._table is table
    for p, q, (m, v) in zip(ps, p1, mv1):
        assert torch.equal(p.detach(), q)  # decay factor 1 - 0*wd = 1, step size 0
        assert not torch.equal(opt.state[p]["exp_avg"], m) and not torch.equal(opt.state[p]["exp_avg_sq"], v)
    for g in opt.param_groups:
        g["lr"] = LR
    opt.step()
    assert opt._table is table and all(not torch.equal(p.detach(), q) for p, q in zip(ps, p1))


# ------------------------------------------------------------------ 7. it trains
@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_llama_tiny_trains_with_adamw(dev, dt, monkeypatch):
    """50 clipped AdamW steps on a pool of 8 sequences, fused arm and torch arm (torch.optim.AdamW +
    clip_grad_norm_): both end below 1.0 (ln 1024 = 6.93 is "did not learn"; the fp32 reference arm on
    CPU ends at 0.05-0.07)."""
    from cs744_pytorch_distributed_tutorial_amd.ops.optim import FusedAdamW
    from cs744_pytorch_distributed_tutorial_amd.runtime.torch_trainer import SyntheticBatches, TorchTrainer
    for k in ("CS744_OPTIMIZER", "CS744_LR", "CS744_WEIGHT_DECAY", "CS744_MAX_GRAD_NORM", "CS744_GRAD_COMM_DTYPE"):
        monkeypatch.delenv(k, raising=False)
    seed = 5000
    for fused in (True, False):
        tr = TorchTrainer("llama-tiny", 8, dev, dtype=dt, optimizer="adamw", lr=1e-3, weight_decay=0.1,
                          max_grad_norm=1.0, seq_len=32, fused_sgd=fused, seed=seed)
        assert type(tr.opt) is (FusedAdamW if fused else torch.optim.AdamW)
        assert len(tr.opt.param_groups) == 2 and tr.opt.param_groups[1]["weight_decay"] == 0
        tr.data = SyntheticBatches("tokens", 8, dev, seq=32, vocab=1024, pool=8, seed=seed)
        losses = []
        for _ in range(50):
            tr.step()
            losses.append(tr.loss)
        losses = torch.stack(losses).float().cpu()
        print(f"[adamw-numerics] trains {dt} {'fused' if fused else 'torch'}: first {float(losses[0]):.3f} "
              f"max(last 10) {float(losses[-10:].max()):.4f}")
        assert bool(torch.isfinite(losses).all())
        assert float(losses[-10:].max()) < 1.0
        if fused:
            assert float(tr.opt.last_grad_norm()) > 0


# ------------------------------------------------------------------ 8. host checks
def test_table_builder_refuses_bad_tensors(dev):
    from cs744_pytorch_distributed_tutorial_amd.ops import native
    C = native.C()
    p = torch.randn(8, 4, 3, 3, device=dev).contiguous(memory_format=torch.channels_last)
    g, m, v = torch.zeros_like(p), torch.zeros_like(p), torch.zeros_like(p)
    none = torch.empty(0, device=dev, dtype=torch.bfloat16)
    t = C.adamw_multi_table([p], [g], [m], [v], [none])
    assert t.is_cuda and t.dtype == torch.int64 and t.numel() == 9 and int(t[-1]) == 1
    with pytest.raises(RuntimeError, match="memory layout"):
        C.adamw_multi_table([p], [g], [m], [v.contiguous()], [none])
    with pytest.raises(RuntimeError, match="bf16"):
        C.adamw_multi_table([p], [g], [m], [v], [torch.zeros_like(p, dtype=torch.float16)])
    with pytest.raises(RuntimeError, match="GPU"):
        C.adamw_multi_table([p], [g.cpu()], [m], [v], [none])
    with pytest.raises(RuntimeError, match="float32"):
        C.adamw_multi_table([p], [g], [m.double()], [v], [none])
    with pytest.raises(RuntimeError):
        C.adamw_multi(t, 2, 1, LR, 0.9, 0.95, EPS, WD, 0.1, 0.05)  # more tensors than the table holds
