"""The float64 oracles, bounds and input builders of tests/ops_oracle.py on the CPU, before
tests/test_ops_edges_gpu.py holds a kernel to them: each oracle against an independent
implementation (torch.optim.SGD, F.cross_entropy with autograd, utils.data.augment_reference,
Tensor.bfloat16), each builder against what its docstring claims, and each derived bound against
a plain fp32 evaluation of the same formula, which a bound must admit."""
import pytest
import torch

import ops_oracle as oo

F32 = torch.float32
CPU = torch.device("cpu")

# the (B, K, C) of the GPU head cases (tests/test_ops_edges_gpu.py) and the peaked variants
HEAD_SHAPES = [(23, 512, 10), (5, 4, 10), (7, 252, 10), (4, 260, 10), (9, 516, 10), (6, 2048, 10),
               (23, 512, 1), (23, 512, 2), (5, 36, 9), (7, 516, 11), (3, 2048, 16)]
PEAK_SHAPES = [(23, 512, 10), (7, 516, 11)]
PEAK_TARGETS = [1e2, 1e4]


# ------------------------------------------------------------------ SGD
@pytest.mark.parametrize("lr,mom,wd,damp", [(0.1, 0.9, 1e-4, 0.0), (0.05, 0.8, 5e-4, 0.25), (0.1, 0.0, 1e-4, 0.0)])
def test_sgd_oracle_matches_torch_sgd(lr, mom, wd, damp):
    torch.manual_seed(0)
    n = 257
    p0 = torch.randn(n, dtype=torch.float64)
    rp = torch.nn.Parameter(p0.clone())
    opt = torch.optim.SGD([rp], lr=lr, momentum=mom, weight_decay=wd, dampening=damp, foreach=False)
    p, m = p0.clone(), torch.full((n,), 123.0, dtype=torch.float64)  # m: not read at the first step
    for i in range(3):
        g = torch.randn(n, dtype=torch.float64)
        rp.grad = g.clone()
        opt.step()
        m_in = m.clone()
        p, m = oo.sgd_oracle(p, g, m, lr, mom, wd, damp, 1.0, i == 0)
        if mom == 0:
            assert torch.equal(m, m_in)
    # the oracle rounds the hyperparameters to fp32 (2^-24 relative each); torch used them unrounded
    torch.testing.assert_close(p, rp.detach(), rtol=1e-6, atol=1e-6)
    if mom != 0:
        torch.testing.assert_close(m, opt.state[rp]["momentum_buffer"], rtol=1e-6, atol=1e-6)


def test_sgd_oracle_scale_is_a_gradient_multiplier():
    p, g, m = oo.sgd_inputs(101, CPU)
    a = oo.sgd_oracle(p, g, m, 0.05, 0.8, 5e-4, 0.25, 0.5, False)
    b = oo.sgd_oracle(p, g.double() * 0.5, m, 0.05, 0.8, 5e-4, 0.25, 1.0, False)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_sgd_inputs_magnitudes():
    for t in oo.sgd_inputs(20000, CPU):
        a = t.abs()
        assert t.dtype == F32 and float(a.min()) >= 0.999e-3 and float(a.max()) <= 1.001e3
        assert float(a.min()) < 2e-3 and float(a.max()) > 500 and 0.4 < float((t > 0).float().mean()) < 0.6


def _sgd_fp32(p, g, m, lr, mom, wd, damp, scale, first):
    """the update in plain fp32 tensor arithmetic: every product and sum rounded once"""
    t = lambda v: torch.tensor(v, dtype=F32)
    d = g * t(scale) + t(wd) * p
    if mom == 0:
        return p - t(lr) * d, m
    buf = d if first else t(mom) * m + (t(1.0) - t(damp)) * d
    return p - t(lr) * buf, buf


@pytest.mark.parametrize("cfg", oo.SGD_CONFIGS, ids=lambda c: "-".join(str(v) for v in c))
def test_sgd_bounds_admit_an_fp32_evaluation(cfg):
    """2,000,000 elements of magnitudes 1e-3 .. 1e3: the fp32 formula stays under the derived bounds
    (it has more roundings than the kernel, which fuses three of the products into fmas)"""
    p, g, m = oo.sgd_inputs(2_000_000, CPU, seed=1)
    rp, rm = oo.sgd_oracle(p, g, m, *cfg)
    bp, bm = oo.sgd_bounds(p, g, m, *cfg)
    fp, fm = _sgd_fp32(p, g, m, *cfg)
    wp = float(((fp.double() - rp).abs() / bp).max())
    wm = float(((fm.double() - rm).abs() / bm).max())
    print(f"[ops-oracles] sgd fp32 {cfg}: p {wp:.2f}x bound, m {wm:.2f}x bound")
    assert wp <= 1.0 and wm <= 1.0
    assert wp > 0.05  # the bound is of the size of the rounding error, not orders above it


# ------------------------------------------------------------------ classifier head
def _head_torch(feat, W, bias, y, gscale):
    f, w, b = (t.double().requires_grad_() for t in (feat, W, bias))
    logits = torch.nn.functional.linear(f, w, b)
    logits.retain_grad()
    loss = torch.nn.functional.cross_entropy(logits, y)
    (loss * gscale).backward()
    return logits.detach(), loss.detach(), logits.grad, w.grad, b.grad, f.grad


HEAD_NAMES = oo.HEAD_NAMES


@pytest.mark.parametrize("B,K,C", HEAD_SHAPES)
@pytest.mark.parametrize("gscale", [1.0, 0.25])
def test_head_oracle_matches_autograd(B, K, C, gscale):
    feat, W, bias, y = oo.head_inputs(B, K, C, CPU)
    assert int(y.min()) >= 0 and int(y.max()) < C
    for n, a, r in zip(HEAD_NAMES, oo.head_oracle(feat, W, bias, y, gscale), _head_torch(feat, W, bias, y, gscale)):
        torch.testing.assert_close(a, r, rtol=1e-10, atol=1e-12, msg=lambda s, n=n: f"{n}: {s}")


def _head_fp32(feat, W, bias, y, gscale):
    """head_oracle's formulas evaluated in fp32"""
    B = feat.shape[0]
    x = feat @ W.t() + bias
    mx = x.max(1, keepdim=True).values
    lse = (x - mx).exp().sum(1).log() + mx[:, 0]
    rows = torch.arange(B)
    loss = (lse - x[rows, y]).mean()
    dl = (x - lse[:, None]).exp()
    dl[rows, y] -= 1.0
    dl = dl * (torch.tensor(gscale, dtype=F32) / B)
    return x, loss, dl, dl.t() @ feat, dl.sum(0), dl @ W


def _head_fp32_worst(feat, W, bias, y, gscale, peaked=False):
    ref = oo.head_oracle(feat, W, bias, y, gscale)
    bound = oo.head_bounds(ref, gscale, (feat, W, bias) if peaked else None)
    worst = {}
    for n, a, r in zip(HEAD_NAMES, _head_fp32(feat, W, bias, y, gscale), ref):
        assert bool(torch.isfinite(a).all()), n
        worst[n] = float(((a.double() - r).abs() / bound[n]).max())
    return worst


@pytest.mark.parametrize("B,K,C", HEAD_SHAPES)
@pytest.mark.parametrize("gscale", [1.0, 0.25])
def test_head_tolerances_admit_an_fp32_evaluation(B, K, C, gscale):
    feat, W, bias, y = oo.head_inputs(B, K, C, CPU)
    worst = _head_fp32_worst(feat, W, bias, y, gscale)
    print(f"[ops-oracles] head fp32 ({B}, {K}, {C}) gscale {gscale}: " + " ".join(f"{n} {w:.2f}x" for n, w in worst.items()))
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("B,K,C", PEAK_SHAPES)
@pytest.mark.parametrize("target", PEAK_TARGETS)
def test_head_tolerances_admit_an_fp32_evaluation_of_peaked_logits(B, K, C, target):
    feat, W, bias, y = oo.head_inputs(B, K, C, CPU, seed=1)
    s = oo.peak_scale(feat, W, bias, target)
    assert s == 2.0 ** round(torch.log2(torch.tensor(s)).item()) and s > 1
    feat = feat * s
    ref = oo.head_oracle(feat, W, bias, y)
    mx = float(ref[0].abs().max())
    assert target / 2 < mx < target * 2 and bool(torch.isfinite(ref[1])) and float(ref[1]) > 1
    # a class far from the row's maximum: its softmax underflows, the gradient is that of the one-hot alone
    far = ref[0] < ref[0].max(1, keepdim=True).values - 110
    assert bool(far.any())
    worst = _head_fp32_worst(feat, W, bias, y, 1.0, peaked=True)
    print(f"[ops-oracles] head fp32 peaked ({B}, {K}, {C}) max|logit| {mx:.3g}: " +
          " ".join(f"{n} {w:.2f}x" for n, w in worst.items()))
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("B,K,C", PEAK_SHAPES)
def test_head_tie_inputs(B, K, C):
    feat, W, bias, y = oo.head_tie_inputs(B, K, C, CPU, "flat")
    lg = oo.head_oracle(feat, W, bias, y)[0]
    assert bool((lg == 0.5).all()) and bool((oo.lowest_argmax(lg) == 0).all())
    feat, W, bias, y = oo.head_tie_inputs(B, K, C, CPU, "pair")
    j0, j1 = oo.TIE_PAIR
    assert torch.equal(W[j0], W[j1]) and float(bias[j0]) == float(bias[j1]) == 50.0
    lg = oo.head_oracle(feat, W, bias, y)[0]
    assert torch.equal(lg[:, j0], lg[:, j1])  # bit-equal
    assert bool((lg[:, j0] == lg.max(1).values).all())
    others = [j for j in range(C) if j not in oo.TIE_PAIR]
    assert float(lg[:, others].max()) < float(lg[:, j0].min()) - 10  # a margin fp32 rounding cannot close
    assert bool((oo.lowest_argmax(lg) == j0).all())


def test_lowest_argmax():
    x = torch.tensor([[1.0, 3.0, 3.0, 2.0], [5.0, 5.0, 5.0, 5.0], [0.0, -1.0, 0.5, 0.5], [2.0, 1.0, 0.0, 2.0]])
    assert oo.lowest_argmax(x).tolist() == [1, 0, 2, 0]


@pytest.mark.parametrize("B", [1, 64, 513, 1000])
@pytest.mark.parametrize("C", [1, 10, 16])
def test_xent_oracle_matches_autograd(B, C):
    x, y = oo.xent_inputs(B, C, CPU)
    xr = x.double().requires_grad_()
    loss = torch.nn.functional.cross_entropy(xr, y)
    (loss * 0.25).backward()
    got = oo.xent_oracle(x, y, 0.25)
    torch.testing.assert_close(got[0], loss.detach(), rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(got[1], xr.grad, rtol=1e-10, atol=1e-14)


# ------------------------------------------------------------------ flat combines and casts
def test_rows_mean_oracle_and_bound():
    torch.manual_seed(1)
    for rows, n in ((1, 5), (3, 1027), (16, 1027)):
        src = torch.randn(rows * n)
        ref, bound = oo.rows_mean_oracle(src, rows)
        torch.testing.assert_close(ref, src.double().view(rows, n).mean(0), rtol=1e-14, atol=0)
        s = src.view(rows, n)[0].clone()
        for r in range(1, rows):  # the kernel's order: rows summed in order, then one division
            s += src.view(rows, n)[r]
        got = s / torch.tensor(float(rows))
        assert bool(((got.double() - ref).abs() <= bound).all())
        if rows == 1:
            assert torch.equal(got, src)


def test_bf16_rne_bits_matches_torch():
    x, built = oo.cast_edge_inputs(2_098_355, CPU)
    assert x.dtype == F32 and x.numel() == 2_098_355
    ref = oo.bits_of(x.bfloat16())
    got = oo.bf16_rne_bits(x)
    nan = torch.isnan(x)
    assert int(nan.sum()) == 4
    assert torch.equal(oo.bf16_bits_isnan(got), nan) and torch.equal(oo.bf16_bits_isnan(ref), nan)
    assert torch.equal(got[~nan], ref[~nan])
    # the listed patterns give the listed results
    ns = len(oo.CAST_SPECIALS)
    assert oo.bits_of(x[:ns]).tolist() == [b for b, _ in oo.CAST_SPECIALS]
    for (b, want), g in zip(oo.CAST_SPECIALS, got[:ns].tolist()):
        assert (want is None and (g & 0x7FFF) > 0x7F80) or g == want, (hex(b), hex(g))
    assert float(oo.f32_from_bits([0x7F7FFFFF], CPU)) == torch.finfo(F32).max
    assert float(oo.bf16_from_bits([0x7F7F], CPU).float()) == torch.finfo(torch.bfloat16).max


def test_cast_edge_inputs_are_ties_of_both_parities():
    x, built = oo.cast_edge_inputs(2_098_355, CPU)
    ns = len(oo.CAST_SPECIALS)
    nt = (built - ns) // 3
    tie, below, above = (oo.bits_of(x[ns + i * nt:ns + (i + 1) * nt]) for i in range(3))
    assert nt == 0x10000 - 2 * 128  # every hi16 but the Inf / NaN exponents
    assert bool(((tie & 0xFFFF) == 0x8000).all())  # exactly half way between two bf16 values
    hi = tie >> 16
    assert int((hi & 1).sum()) == nt // 2  # half with an odd kept bit (round up), half even (round down)
    assert bool((hi & 0x7F80 != 0x7F80).all()) and int((hi & 0x7F80 == 0).sum()) == 256  # finite; subnormals in
    assert torch.equal(below, tie - 1) and torch.equal(above, tie + 1)
    got = oo.bf16_rne_bits(x[ns:built])
    assert torch.equal(got[:nt], hi + (hi & 1))  # to even
    assert torch.equal(got[nt:2 * nt], hi) and torch.equal(got[2 * nt:], hi + 1)
    # a round-half-up conversion differs on every even tie: the sweep tells the two apart
    half_up = (tie + 0x8000) >> 16
    assert int((half_up != got[:nt]).sum()) == nt // 2
    rest = x[built:]
    assert bool(torch.isfinite(rest).all()) and float(rest.abs().max()) > 100


def test_backcast_inputs():
    x, bits = oo.backcast_inputs(2_098_355, CPU)
    assert x.dtype == torch.bfloat16 and torch.equal(oo.bits_of(x), bits)
    assert torch.equal(bits[:0x10000], torch.arange(0x10000))
    f = x.float()
    ok = ~torch.isnan(f)
    assert torch.equal(oo.bits_of(f)[ok], (bits << 16)[ok])


# ------------------------------------------------------------------ augment
def test_augment_dataset_pixels_are_distinguishable():
    data, params = oo.augment_dataset(CPU)
    assert data.dtype == torch.uint8 and data.shape == (18, 32, 32, 3) and params.dtype == torch.int32
    n, y, x, c = 5, 7, 11, 2
    assert int(data[n, y, x, c]) == (7 * n + 3 * (32 * y + x) + c) % 251
    d = data.long()
    assert bool((d[:, 1:] != d[:, :-1]).all()) and bool((d[:, :, 1:] != d[:, :, :-1]).all())  # neighbours
    assert bool((d[..., 1:] != d[..., :-1]).all())  # channels
    assert float((d != d.flip(2)).float().mean()) > 0.99  # mirror image
    off = ~torch.eye(32, dtype=torch.bool)
    assert float((d != d.transpose(1, 2))[:, off].float().mean()) > 0.99  # transpose
    assert bool((d[1:] != d[:-1]).all())  # the next image
    combos = {tuple(r) for r in params.tolist()}
    assert combos == {(dy, dx, fl) for dy in (0, 4, 8) for dx in (0, 4, 8) for fl in (0, 1)} and len(params) == 18


@pytest.mark.parametrize("nhwc,cstride", [(False, 3), (True, 3), (True, 4)])
def test_augment_oracle_matches_reference(nhwc, cstride):
    from cs744_pytorch_distributed_tutorial_amd.utils import data as dm
    ds = dm.SyntheticCIFAR10(train=True, size=40, seed=3)
    params = dm.augment_params(40, 0, 5, True)
    idx = torch.randperm(40, generator=torch.Generator().manual_seed(0))[:13]
    got = oo.augment_oracle(ds.data, idx, params, nhwc, cstride)
    ref = dm.augment_reference(ds.data, idx, params, channels_last=nhwc).double()
    if cstride == 4:
        assert bool((got[..., 3] == 0).all())
        got = got[..., :3]
    torch.testing.assert_close(got, ref, rtol=1e-5, atol=1e-5)
    # and on the fixed dataset, whose crops reach every corner
    data, params = oo.augment_dataset(CPU)
    for idx in oo.AUG_IDX:
        idx = torch.tensor(idx)
        got = oo.augment_oracle(data, idx, params, nhwc, cstride)
        ref = dm.augment_reference(data, idx, params, channels_last=nhwc).double()
        torch.testing.assert_close(got[..., :3] if cstride == 4 else got, ref, rtol=1e-5, atol=1e-5)


def test_augment_oracle_order_of_crop_and_flip():
    """image 1 is (dy, dx, fl) = (0, 0, 1): the window's top-left 4 x 4 is padding BEFORE the mirror, so
    the output's padding is at the top right; mirroring first would put it at the top left"""
    data, params = oo.augment_dataset(CPU)
    assert params[1].tolist() == [0, 0, 1]
    out = oo.augment_oracle(data, torch.tensor([1]), params, True, 3)[0]
    mean = torch.tensor(oo.CIFAR_MEAN_255, dtype=torch.float64) / 255
    std = torch.tensor(oo.CIFAR_STD_255, dtype=torch.float64) / 255
    pad = -mean / std
    assert bool((out[:4] == pad).all()) and bool((out[:, 28:] == pad).all())
    assert bool((out[4:, :28] != pad).any(-1).all())
    # output (y, x) = source (y - 4, 31 - x - 4): (4, 27) is source (0, 0), (31, 0) is source (27, 27)
    px = lambda y, x: (data[1, y, x].double() / 255 - mean) / std
    assert torch.equal(out[4, 27], px(0, 0)) and torch.equal(out[31, 0], px(27, 27)) and torch.equal(out[10, 20], px(6, 7))
