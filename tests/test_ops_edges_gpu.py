"""The kernels bound in csrc/binding/ops.cpp (xent.hip, sgd.hip, flat_ops.hip, augment.hip) on the
branches tests/test_ops_gpu.py never enters: the runtime-C and the uncached classifier row pass, the
eval path, every loop of the column pass, peaked and tied logits; second grid-stride trips of the
element-wise passes, every SGD hyperparameter, the multi-tensor table's binary search; bf16 rounding
at ties, subnormals and the overflow to Inf; the corners of the crop range. docs/ops_edge_tests.md
lists what each case reaches and the measured error over bound.

Oracle: tests/ops_oracle.py, the op written out in float64 on the same values, with bounds derived
from the number of fp32 roundings (checked on the CPU by tests/test_ops_oracles_cpu.py). Where two
results must be the same bits they are compared as bits.
"""
import functools

import pytest
import torch

import ops_oracle as oo
import test_lm_edges_gpu as le
from test_lm_edges_gpu import offset_view

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
BIG = 2_097_152 + 4 * 300 + 3  # 2048 blocks x 256 threads x 4: a second grid-stride trip of 300 float4 and a tail of 3


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cs744_pytorch_distributed_tutorial_amd.ops import native
    native.C()
    return torch.device("cuda", 0)


class Report(le.Report):
    def done(self):
        print(f"[ops-edges] {self.tag}: " + " ".join(f"{n} {e:.3e} ({w:.2f}x bound)" for n, e, w in self.items))
        bad = [(n, e, w) for n, e, w in self.items if not w <= 1.0]
        assert not bad, (self.tag, bad)


def same_bits(a, b):
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if not a.is_floating_point():
        return torch.equal(a, b)
    return torch.equal(oo.bits_of(a.reshape(-1)), oo.bits_of(b.reshape(-1)))


# ------------------------------------------------------------------ classifier head
# C == 10: head_rows_kernel<10>, any other C: head_rows_kernel<0> (runtime C). K4 = K / 4 float4 per row.
HEAD_CASES = [
    (23, 512, 10),   # cols_wave: one 16-unrolled trip, one 4-unrolled trip, 3 remainder rows; cached, both trips full
    (5, 4, 10),      # K4 = 1: one live lane in trip 0, `k < K4` false for all of trip 1
    (7, 252, 10),    # K4 = 63: `k < K4` false in trip 0 for lane 63
    (4, 260, 10),    # K4 = 65: trip 1 with one live lane; K % 64 = 4, so `k >= K` returns in the column pass
    (9, 516, 10),    # K4 = 129 > 128: the first K of the `!cached` loop and of the second W read for dfeat
    (6, 2048, 10),   # `!cached`, 8 trips per lane
    (23, 512, 1), (23, 512, 2), (5, 36, 9), (7, 516, 11), (3, 2048, 16),  # head_rows_kernel<0>
]
PEAK_CASES = [(23, 512, 10), (7, 516, 11)]


def _head(dev, feat, W, bias, y, gscale=1.0, backward=True):
    from cs744_pytorch_distributed_tutorial_amd.ops import native
    return native.linear_xent(feat, W, bias, y, gscale, backward)


def _check_head(tag, out, feat, W, bias, y, gscale, peaked=False):
    l, correct, lg, dW, db, dfeat, pred = out
    ref = dict(zip(oo.HEAD_NAMES, oo.head_oracle(feat, W, bias, y, gscale)))
    bound = oo.head_bounds(tuple(ref.values()), gscale, (feat, W, bias) if peaked else None)
    rep = Report(tag)
    for n, got in (("logits", lg), ("loss", l), ("dW", dW), ("db", db), ("dfeat", dfeat)):
        assert got.dtype == F32 and bool(torch.isfinite(got).all()), n
        rep.add(n, got, ref[n], bound=bound[n])
    # exact: the prediction is the lowest index of the maximum of the logits the kernel returned
    # (themselves held to the oracle above, so a near-tie in float64 cannot fail this)
    assert pred.dtype == torch.int64 and torch.equal(pred, oo.lowest_argmax(lg))
    assert correct.dtype == torch.int32 and int(correct) == int((pred == y).sum())
    rep.done()
    return ref


@pytest.mark.parametrize("B,K,C", HEAD_CASES)
@pytest.mark.parametrize("gscale", [1.0, 0.25])
def test_linear_xent_branches(dev, B, K, C, gscale):
    feat, W, bias, y = oo.head_inputs(B, K, C, dev)
    out = _head(dev, feat, W, bias, y, gscale)
    assert len(out) == 7
    _check_head(f"linear_xent ({B}, {K}, {C}) gscale {gscale}", out, feat, W, bias, y, gscale)
    again = _head(dev, feat, W, bias, y, gscale)  # fixed summation order: run to run the same bits
    assert all(same_bits(a, b) for a, b in zip(out, again))


@pytest.mark.parametrize("B,K,C", PEAK_CASES)
def test_linear_xent_eval_path(dev, B, K, C):
    """backward=False: dfeat == nullptr returns early from the row pass, the column pass runs one piece
    (P = 1: loss and count only); loss, correct, logits and pred are those of the backward call"""
    feat, W, bias, y = oo.head_inputs(B, K, C, dev)
    full = _head(dev, feat, W, bias, y, 1.0, True)
    ev = _head(dev, feat, W, bias, y, 1.0, False)
    assert len(ev) == 4
    for name, a, b in zip(("loss", "correct", "logits", "pred"), ev, (full[0], full[1], full[2], full[6])):
        assert same_bits(a, b), name


@pytest.mark.parametrize("B,K,C", PEAK_CASES)
@pytest.mark.parametrize("target", [1e2, 1e4])
def test_linear_xent_peaked_logits(dev, B, K, C, target):
    """features scaled by a power of two until max |logit| is about `target`: expf underflows for every
    class far from the maximum, the loss is far above 1; all outputs finite and inside the bounds,
    which add the propagated error of fp32 logits of that size (ops_oracle.head_bounds)"""
    feat, W, bias, y = oo.head_inputs(B, K, C, dev, seed=1)
    feat = feat * oo.peak_scale(feat, W, bias, target)
    out = _head(dev, feat, W, bias, y)
    ref = _check_head(f"linear_xent peaked ({B}, {K}, {C}) target {target:g}", out, feat, W, bias, y, 1.0, peaked=True)
    assert target / 2 < float(ref["logits"].abs().max()) < 2 * target and float(ref["loss"]) > 1
    # a class more than 110 below its row's maximum has softmax < 2^-149: the row's dlogits, and so the
    # row's share of db, is that of the other classes alone. With every row's class j that far down
    # and never the label, db[j] is exactly 0.
    far = (ref["logits"] < ref["logits"].max(1, keepdim=True).values - 110)
    onehot = torch.nn.functional.one_hot(y, C).bool()
    dead = (far & ~onehot).all(0)
    assert bool((out[4][dead] == 0).all())


@pytest.mark.parametrize("B,K,C", PEAK_CASES)
@pytest.mark.parametrize("variant", ["flat", "pair"])
def test_linear_xent_ties(dev, B, K, C, variant):
    feat, W, bias, y = oo.head_tie_inputs(B, K, C, dev, variant)
    out = _head(dev, feat, W, bias, y)
    lg, pred = out[2], out[6]
    if variant == "flat":
        assert bool((lg == 0.5).all()) and bool((pred == 0).all())
    else:
        j0, j1 = oo.TIE_PAIR
        assert torch.equal(lg[:, j0], lg[:, j1]) and bool((lg[:, j0] == lg.max(1).values).all())
        assert bool((pred == j0).all())
    _check_head(f"linear_xent ties {variant} ({B}, {K}, {C})", out, feat, W, bias, y, 1.0)
    ev = _head(dev, feat, W, bias, y, 1.0, False)
    assert torch.equal(ev[3], pred) and int(ev[1]) == int((pred == y).sum())


@pytest.mark.parametrize("B", [1, 64, 513, 1000])
@pytest.mark.parametrize("C", [1, 10, 16])
def test_softmax_xent_branches(dev, B, C):
    """one block of 512 threads: B = 513 and 1000 take the `b += blockDim.x` loop a second time (one
    thread, then 488 of them); B = 1 leaves 511 threads with nothing to add"""
    from cs744_pytorch_distributed_tutorial_amd.ops import native
    x, y = oo.xent_inputs(B, C, dev)
    for gscale in (1.0, 0.25):
        l, dl, c = native.softmax_xent(x, y, gscale)
        rl, rdl = oo.xent_oracle(x, y, gscale)
        rep = Report(f"softmax_xent ({B}, {C}) gscale {gscale}")
        rep.add("loss", l, rl, atol=1e-5 * (1 + float(x.abs().max())))
        rep.add("dlogits", dl, rdl, rtol=1e-4, atol=1e-6 * gscale)
        assert c.dtype == torch.int32 and int(c) == int((oo.lowest_argmax(x) == y).sum())
        rep.done()
        l2, dl2, c2 = native.softmax_xent(x, y, gscale)
        assert same_bits(l, l2) and same_bits(dl, dl2) and int(c) == int(c2)


def test_xent_bindings_check_labels_on_the_host(dev):
    """a label outside [0, C) would index past a logits row on the device: both bindings refuse it
    before launching, and still refuse what they refused before"""
    from cs744_pytorch_distributed_tutorial_amd.ops import native
    feat, W, bias, y = oo.head_inputs(4, 8, 3, dev)
    x, _ = oo.xent_inputs(4, 3, dev)
    for bad in (-1, 3, 2 ** 40):
        yb = y.clone()
        yb[2] = bad
        with pytest.raises(RuntimeError, match="label"):
            native.linear_xent(feat, W, bias, yb, 1.0, True)
        with pytest.raises(RuntimeError, match="label"):
            native.linear_xent(feat, W, bias, yb, 1.0, False)
        with pytest.raises(RuntimeError, match="label"):
            native.softmax_xent(x, yb)
    with pytest.raises(RuntimeError):  # C == 0
        native.softmax_xent(torch.empty(4, 0, device=dev), torch.zeros(4, dtype=torch.long, device=dev))
    with pytest.raises(RuntimeError):
        native.linear_xent(feat, torch.empty(0, 8, device=dev), torch.empty(0, device=dev), y, 1.0, True)
    with pytest.raises(RuntimeError):  # K % 4 != 0
        native.linear_xent(feat[:, :6].contiguous(), W[:, :6].contiguous(), bias, y, 1.0, True)
    with pytest.raises(RuntimeError):  # C = 17
        native.linear_xent(feat, torch.zeros(17, 8, device=dev), torch.zeros(17, device=dev), y, 1.0, True)
    with pytest.raises(RuntimeError):
        native.softmax_xent(torch.zeros(4, 17, device=dev), y)
    with pytest.raises(RuntimeError):  # float64
        native.linear_xent(feat.double(), W.double(), bias.double(), y, 1.0, True)
    with pytest.raises(RuntimeError):
        native.softmax_xent(x.double(), y)
    with pytest.raises(RuntimeError):  # int32 labels
        native.linear_xent(feat, W, bias, y.int(), 1.0, True)
    with pytest.raises(RuntimeError):
        native.softmax_xent(x, y.int())
    # a valid call right after still works
    _check_head("linear_xent after refusals", native.linear_xent(feat, W, bias, y, 1.0, True), feat, W, bias, y, 1.0)
    l, dl, c = native.softmax_xent(x, y)
    rl, rdl = oo.xent_oracle(x, y)
    torch.testing.assert_close(l.double(), rl, rtol=0, atol=1e-5 * (1 + float(x.abs().max())))
    torch.testing.assert_close(dl.double(), rdl, rtol=1e-4, atol=1e-6)


# ------------------------------------------------------------------ SGD
SGD_NS = [3, 4, 4099, BIG]  # scalar tail only; one float4; float4 + tail of 3; the second grid-stride trip
_cfg_id = lambda c: "-".join(str(v) for v in c)


@functools.lru_cache(maxsize=None)
def _sgd_data(n, device):
    return oo.sgd_inputs(n, device)


def _sgd_m(m0, cfg):
    """the momentum the case starts from: NaN where the kernel must not read it (first), a sentinel
    where it must not write it (momentum 0)"""
    mom, first = cfg[1], cfg[5]
    if first:
        return torch.full_like(m0, float("nan"))
    if mom == 0:
        return torch.full_like(m0, 1234.5)
    return m0.clone()


def _check_sgd(tag, p, m, p0, g, m_in, cfg):
    mom = cfg[1]
    rp, rm = oo.sgd_oracle(p0, g, m_in, *cfg)
    bp, bm = oo.sgd_bounds(p0, g, m_in, *cfg)
    rep = Report(tag)
    rep.add("p", p, rp, bound=bp)
    if mom == 0:
        assert same_bits(m, m_in)  # left untouched
    else:
        rep.add("m", m, rm, bound=bm)
    rep.done()


@pytest.mark.parametrize("n", SGD_NS)
@pytest.mark.parametrize("cfg", oo.SGD_CONFIGS, ids=_cfg_id)
def test_sgd_flat_branches(dev, n, cfg):
    from cs744_pytorch_distributed_tutorial_amd.ops import native
    p0, g, m0 = _sgd_data(n, dev)
    m_in = _sgd_m(m0, cfg)
    p, m = p0.clone(), m_in.clone()
    native.sgd_flat(p, g, m, *cfg)
    _check_sgd(f"sgd_flat n {n} {cfg}", p, m, p0, g, m_in, cfg)
    # contiguous views one element off the allocation's alignment: the same bits
    po, go, mo = offset_view(p0), offset_view(g), offset_view(m_in)
    native.sgd_flat(po, go, mo, *cfg)
    assert same_bits(po, p) and same_bits(mo, m)


# 1 / 4095 / 4096 / 4097: one chunk short by 4095, short by one, exactly one, one chunk and one element;
# 0: an empty parameter (chunk_start repeats); 3 * 4096 + 5: four chunks of one tensor, the last of 5; 7 tensors, 10 chunks
MULTI_SIZES = [1, 4095, 4096, 4097, 0, 3 * 4096 + 5, 1]
MULTI_SHADOWED = (1, 5)


def _split(t, sizes):
    return [c.clone() for c in torch.split(t, sizes)]


def _run_multi(dev, sizes, cfg, shadowed=()):
    """one sgd_multi step over separate tensors of `sizes` and the same values through sgd_flat"""
    from cs744_pytorch_distributed_tutorial_amd import _C
    from cs744_pytorch_distributed_tutorial_amd.ops import native
    p0, g, m0 = _sgd_data(sum(sizes), dev)
    m_in = _sgd_m(m0, cfg)
    ps, gs, ms = _split(p0, sizes), _split(g, sizes), _split(m_in, sizes)
    none = torch.empty(0, dtype=BF16, device=dev)
    shs = [torch.zeros(s, dtype=BF16, device=dev) if i in shadowed else none for i, s in enumerate(sizes)]
    table = _C.sgd_multi_table(ps, gs, ms, shs)
    nchunks = int(table[-1])
    assert nchunks == sum((s + 4095) // 4096 for s in sizes)
    assert table[len(sizes) * 5:-1].tolist() == [sum((s + 4095) // 4096 for s in sizes[:i]) for i in range(len(sizes))]
    _C.sgd_multi(table, len(sizes), nchunks, *cfg)
    p, m = torch.cat(ps), torch.cat(ms)
    pf, mf = p0.clone(), m_in.clone()
    native.sgd_flat(pf, g, mf, *cfg)
    return p, m, pf, mf, p0, g, m_in, ps, shs


@pytest.mark.parametrize("cfg", oo.SGD_CONFIGS, ids=_cfg_id)
def test_sgd_multi_chunk_search(dev, cfg):
    p, m, pf, mf, p0, g, m_in, ps, shs = _run_multi(dev, MULTI_SIZES, cfg, MULTI_SHADOWED)
    _check_sgd(f"sgd_multi {MULTI_SIZES} {cfg}", p, m, p0, g, m_in, cfg)
    assert same_bits(p, pf) and same_bits(m, mf)  # sgd_device.h: one element update, the same bits
    for i in MULTI_SHADOWED:  # the bf16 shadow is the new value rounded to nearest even
        assert torch.equal(oo.bits_of(shs[i]), oo.bf16_rne_bits(ps[i]))


def test_sgd_multi_more_chunks_than_blocks(dev):
    """2100 one-element tensors: 2100 chunks on 2048 blocks, so blocks 0..51 serve a second chunk, and
    the binary search is 12 levels deep"""
    cfg = oo.SGD_CONFIGS[1]
    p, m, pf, mf, p0, g, m_in, _, _ = _run_multi(dev, [1] * 2100, cfg)
    _check_sgd(f"sgd_multi 2100 x 1 {cfg}", p, m, p0, g, m_in, cfg)
    assert same_bits(p, pf) and same_bits(m, mf)


@pytest.mark.parametrize("damp", [0.0, 0.5])
def test_fused_sgd_first_step_is_per_parameter(dev, damp):
    """a parameter whose first gradient arrives at step 2 starts its own buffer (buf = d) and leaves the
    other parameter's momentum alone, as torch.optim.SGD decides it; the state dict loads into
    torch.optim.SGD and back in the middle of that"""
    from cs744_pytorch_distributed_tutorial_amd.ops.optim import FusedSGD
    g_ = torch.Generator(device="cpu").manual_seed(5)
    a0, b0 = torch.randn(300, generator=g_).to(dev), torch.randn(5000, generator=g_).to(dev)
    ga = [torch.randn(300, generator=g_).to(dev) for _ in range(3)]
    gb = [None] + [torch.randn(5000, generator=g_).to(dev) for _ in range(2)]
    kw = dict(lr=0.1, momentum=0.9, weight_decay=1e-4, dampening=damp)
    ra, rb = torch.nn.Parameter(a0.clone()), torch.nn.Parameter(b0.clone())
    fa, fb = torch.nn.Parameter(a0.clone()), torch.nn.Parameter(b0.clone())
    ref = torch.optim.SGD([ra, rb], foreach=False, **kw)
    opt = FusedSGD([fa, fb], **kw)
    for s in range(3):
        for prm, grads in ((ra, ga), (rb, gb), (fa, ga), (fb, gb)):
            prm.grad = None if grads[s] is None else grads[s].clone()
        ref.step()
        opt.step()
        print(f"[ops-edges] FusedSGD damp {damp} step {s + 1}: max |a - ref| {float((fa - ra).abs().max()):.3e} "
              f"max |b - ref| {float((fb - rb).abs().max()):.3e}")
        torch.testing.assert_close(fa.detach(), ra.detach(), rtol=1e-6, atol=1e-6)
        torch.testing.assert_close(fb.detach(), rb.detach(), rtol=1e-6, atol=1e-6)
        if s == 0:
            assert "momentum_buffer" not in opt.state[fb]
        if s == 1:  # the checkpoint format is torch's: into torch.optim.SGD, and back
            other = torch.optim.SGD([torch.nn.Parameter(fa.detach().clone()), torch.nn.Parameter(fb.detach().clone())],
                                    foreach=False, **kw)
            other.load_state_dict(opt.state_dict())
            for i, rprm in enumerate((ra, rb)):
                torch.testing.assert_close(other.state[other.param_groups[0]["params"][i]]["momentum_buffer"],
                                           ref.state[rprm]["momentum_buffer"], rtol=1e-6, atol=1e-6)
            opt.load_state_dict(other.state_dict())
    for prm, rprm in ((fa, ra), (fb, rb)):
        torch.testing.assert_close(opt.state[prm]["momentum_buffer"], ref.state[rprm]["momentum_buffer"],
                                   rtol=1e-6, atol=1e-6)


# ------------------------------------------------------------------ flat combines and casts
FLAT_BIG = 2_098_355  # = BIG: all four kernels share grid_for's 2048-block cap


@pytest.mark.parametrize("rows,n", [(1, 5), (1, FLAT_BIG), (3, FLAT_BIG), (16, 1027)])
@pytest.mark.parametrize("bcast", [False, True])
def test_rows_mean_branches(dev, rows, n, bcast):
    """rows == 1: the `r = 1..` loops are empty, the mean is x / 1; (1, 5): one float4 and a scalar tail
    of 1; FLAT_BIG: the second grid-stride trip; (16, 1027): 16 rows, tail of 3"""
    from cs744_pytorch_distributed_tutorial_amd import _C
    g_ = torch.Generator(device="cpu").manual_seed(rows * 7919 + n)
    src0 = torch.randn(rows * n, generator=g_).to(dev)
    src, dst = src0.clone(), torch.full((n,), float("nan"), device=dev)
    _C.rows_mean(src, rows, dst, bcast)
    ref, bound = oo.rows_mean_oracle(src0, rows)
    rep = Report(f"rows_mean ({rows}, {n}) bcast {bcast}")
    rep.add("mean", dst, ref, bound=bound)
    rep.done()
    if rows == 1:
        assert same_bits(dst, src0)
    if bcast:
        assert all(same_bits(row, dst) for row in src.view(rows, n))
    else:
        assert same_bits(src, src0)


@pytest.mark.parametrize("n", [3, FLAT_BIG])
@pytest.mark.parametrize("div", [0.0, 3.0])
def test_accumulate_branches(dev, n, div):
    """`add_` then `div_`, bit for bit. The two are done on CPU copies: there `div_` by a number is the
    correctly rounded division, as the kernel's is, while on the GPU ATen multiplies by the fp32
    reciprocal of a scalar divisor ("may lose one bit"): with div = 3 the GPU `div_` is one ulp away
    from the quotient on a third of the elements (measured on an MI355X: 3 of 3 and 699,493 of
    2,098,355) and never more, which is asserted too. The addition alone is also held to the GPU's."""
    from cs744_pytorch_distributed_tutorial_amd import _C
    g_ = torch.Generator(device="cpu").manual_seed(n + int(div))
    g0, t0 = torch.randn(n, generator=g_), torch.randn(n, generator=g_)
    g, t = g0.to(dev), t0.to(dev)
    exp = g0.clone().add_(t0)
    aten = g.clone().add_(t)
    assert torch.equal(aten.cpu(), exp)
    if div > 0:
        exp.div_(div)
        aten.div_(div)
    _C.accumulate(g, t, div)
    assert torch.equal(g.cpu(), exp)
    ulps = (oo.bits_of(g) - oo.bits_of(aten)).abs()
    print(f"[ops-edges] accumulate n {n} div {div}: {int((ulps != 0).sum())} of {n} elements differ from the GPU's "
          f"add_ / div_, by at most {int(ulps.max())} ulp")
    assert int(ulps.max()) <= (1 if div > 0 else 0)


def test_cast_grad_rounds_to_nearest_even(dev):
    """fp32 -> bf16 on +-0, subnormals, the overflow to Inf, Inf, NaN and every exact tie with its
    neighbours (ops_oracle.cast_edge_inputs), at a size that takes the second grid-stride trip"""
    from cs744_pytorch_distributed_tutorial_amd import _C
    x, built = oo.cast_edge_inputs(FLAT_BIG, dev)
    y = torch.zeros(FLAT_BIG, dtype=BF16, device=dev)
    _C.cast_grad(x, y)
    got, ref = oo.bits_of(y), oo.bf16_rne_bits(x)
    nan = torch.isnan(x)
    assert torch.equal(oo.bf16_bits_isnan(got), nan)
    wrong = (got != ref) & ~nan
    assert not bool(wrong.any()), [(hex(int(a)), hex(int(b)), hex(int(c))) for a, b, c in
                                   zip(oo.bits_of(x)[wrong][:8], got[wrong][:8], ref[wrong][:8])]
    for (b, want), g in zip(oo.CAST_SPECIALS, got[:len(oo.CAST_SPECIALS)].tolist()):
        assert want is None or g == want, (hex(b), hex(g))
    yo = torch.zeros(FLAT_BIG, dtype=BF16, device=dev)
    _C.cast_grad(offset_view(x), yo)
    assert torch.equal(oo.bits_of(yo)[~nan], got[~nan]) and torch.equal(oo.bf16_bits_isnan(oo.bits_of(yo)), nan)


def test_cast_grad_back_is_a_shift(dev):
    from cs744_pytorch_distributed_tutorial_amd import _C
    x, bits = oo.backcast_inputs(FLAT_BIG, dev)
    y = torch.zeros(FLAT_BIG, dtype=F32, device=dev)
    _C.cast_grad(x, y)
    assert torch.equal(oo.bits_of(y), bits << 16)


# ------------------------------------------------------------------ augment
@pytest.mark.parametrize("nhwc,cstride", [(False, 3), (True, 3), (True, 4)])
def test_augment_crop_corners_and_flip_order(dev, nhwc, cstride):
    """every (dy, dx) in {0, 4, 8}^2 x flip on images whose pixels are all distinguishable: the corners
    of the crop range, crop before flip, the gather through repeated indices and B = 1"""
    from cs744_pytorch_distributed_tutorial_amd.ops import native
    data, params = oo.augment_dataset(dev)
    mean = torch.tensor(oo.CIFAR_MEAN_255, dtype=torch.float64, device=dev) / 255
    std = torch.tensor(oo.CIFAR_STD_255, dtype=torch.float64, device=dev) / 255
    for idx in oo.AUG_IDX:
        idx = torch.tensor(idx, device=dev)
        out = native.augment(data, idx, params, nhwc, cstride)
        ref = oo.augment_oracle(data, idx, params, nhwc, cstride)
        assert out.shape == ref.shape and out.dtype == F32
        if cstride == 4:
            assert bool((out[..., 3] == 0).all())
        rep = Report(f"augment nhwc {nhwc} cstride {cstride} B {len(idx)}")
        rep.add("out", out, ref, rtol=1e-5, atol=1e-5)
        rep.done()
    # image 0 is (dy, dx, fl) = (0, 0, 0): its top-left 4 x 4 is padding, which is -mean / std, not 0
    assert params[0].tolist() == [0, 0, 0]
    out = native.augment(data, torch.tensor([0], device=dev), params, nhwc, cstride)[0]
    corner = out[:, :4, :4] if not nhwc else out[:4, :4, :3].permute(2, 0, 1)
    want = (-mean / std)[:, None, None].expand(3, 4, 4)
    torch.testing.assert_close(corner.double(), want, rtol=1e-5, atol=1e-5)
    assert float(corner.abs().min()) > 1.5
