"""The decoder-LM gfx950 kernels (csrc/kernels/lm.hip) on the dispatch branches tests/test_lm_gpu.py
never enters: the scalar RMSNorm kernels (D % 4 != 0, D > 8192), more than 16 weight-gradient
partial rows, bf16 weights, SwiGLU / RoPE grid-stride loops that take a second trip, contiguous
views at an odd storage offset, saturating SwiGLU gates, and cross-entropy per row (loss, lse,
dlogits) with shifted logits, -inf padding and out-of-range targets.

Oracle: the op written out from its formula in float64 on the same input values (bf16 inputs are
upcast, never re-rounded). Tolerances: the TOL table and weight-gradient / cross-entropy tolerances
of tests/test_lm_gpu.py for the same op and dtype; anything else is derived where it is used.
The oracles and input builders take a device and are checked on CPU by tests/test_lm_oracles_cpu.py.
"""
import math
import types

import pytest
import torch

from test_lm_gpu import TOL

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
EPS = 1e-5
# tests/test_lm_gpu.py: RMSNorm weight gradient by x dtype; cross-entropy loss / dlogits by logits dtype
DW_TOL = {F32: dict(rtol=1e-4, atol=1e-4), BF16: dict(rtol=2e-2, atol=5e-2)}
XENT_LOSS_TOL = dict(rtol=1e-5, atol=1e-5)
XENT_GRAD_TOL = {F32: dict(rtol=1e-4, atol=1e-6), BF16: dict(rtol=1e-2, atol=1e-4)}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cs744_pytorch_distributed_tutorial_amd.ops import native
    native.C()
    return torch.device("cuda", 0)


# ------------------------------------------------------------------ float64 oracles
def _d(t):
    return t.detach().double()


def rmsnorm_oracle(x, w, gy, eps=EPS):
    """y = x r w with r = (mean(x^2) + eps)^-1/2; dx = r w g - (r^3 / D) x sum(w g x); dw = sum_rows g x r"""
    x, w, gy = _d(x), _d(w), _d(gy)
    D = x.shape[-1]
    r = (x.pow(2).mean(-1, keepdim=True) + eps).rsqrt()
    y = x * r * w
    dot = (w * gy * x).sum(-1, keepdim=True)
    dx = r * w * gy - r.pow(3) / D * dot * x
    dw = (gy * x * r).reshape(-1, D).sum(0)
    return y, dx, dw


def swiglu_oracle(a, b, gy):
    """y = a s b with s = sigmoid(a); da = g b s (1 + a (1 - s)); db = g a s. a * sigmoid(a) never
    overflows: sigmoid saturates to exactly 0 / 1 in float64."""
    a, b, gy = _d(a), _d(b), _d(gy)
    s = torch.sigmoid(a)
    return a * s * b, gy * b * s * (1 + a * (1 - s)), gy * a * s


def rope_oracle(x, cos, sin, gy):
    """pairs (2j, 2j + 1) of x [B, S, H, hd] rotated by the angle of (position, j), tables [S, hd/2];
    the backward is the rotation by the negative angle"""
    c, s = _d(cos)[None, :, None, :], _d(sin)[None, :, None, :]

    def rot(t, sn):
        t = _d(t).reshape(*t.shape[:-1], -1, 2)
        t0, t1 = t[..., 0], t[..., 1]
        return torch.stack([t0 * c - t1 * sn, t0 * sn + t1 * c], -1).reshape(*t.shape[:-2], -1)

    return rot(x, s), rot(gy, -s)


def xent_oracle(logits, targets, g=1.0):
    """per row: lse = log sum exp (natural log), loss = lse - logit[target] (NaN for a target outside
    [0, V)), dlogits = (softmax - onehot) g / R, without the one-hot for such a target"""
    x = _d(logits)
    R, V = x.shape
    lse = torch.logsumexp(x, -1)
    ok = (targets >= 0) & (targets < V)
    tc = targets.clamp(0, V - 1)
    loss = torch.where(ok, lse - x.gather(1, tc[:, None])[:, 0], torch.full_like(lse, float("nan")))
    d = torch.exp(x - lse[:, None])
    d[torch.arange(R, device=x.device)[ok], tc[ok]] -= 1.0
    return loss, lse, d * (g / R)


# ------------------------------------------------------------------ input builders
SWIGLU_GATES = [0.0, 1e-3, 20.0, 60.0, 88.0, 90.0, 1e4]
BF16_MAX = float(torch.finfo(BF16).max)


def swiglu_extreme_inputs(dtype, device, k, seed=0):
    """a: every value of +-SWIGLU_GATES (bf16: and +- the largest finite bf16), each k times; b and g
    uniform in [-1, 1] so that the exact a * b and g * a are representable in dtype (with a normal b
    a third of the products of the largest bf16 value would be infinite by definition)."""
    vals = SWIGLU_GATES + ([BF16_MAX] if dtype == BF16 else [])
    vals = [s * v for v in vals for s in (1.0, -1.0)]
    g_ = torch.Generator(device="cpu").manual_seed(seed)
    a = torch.tensor(vals, dtype=torch.float64).to(dtype)[:, None].expand(len(vals), k).contiguous()
    b = (torch.rand(len(vals), k, generator=g_) * 2 - 1).to(dtype)
    gy = (torch.rand(len(vals), k, generator=g_) * 2 - 1).to(dtype)
    return a.to(device), b.to(device), gy.to(device)


def xent_pad_inputs(dtype, device, which):
    """-inf padded logits and targets in the finite columns. 'tail': V = 1008, columns >= 1001 padded
    (an odd vocabulary of 1001 padded to a multiple of 8: the last 8-vector is 1 finite + 7 -inf).
    'half': V = 4096, every thread reads the 8-vectors i and i + 2048; per row
      0: columns >= 2048 padded (the second vector is all -inf: ms_combine's m2 == -inf return),
      1: columns <  2048 padded (the first is: the m == -inf adoption on the second),
      2: columns <  3000 padded (threads 0..118 see nothing finite: wave 0 enters the shuffle and the
         4-wave combine with m == -inf),
      3: nothing padded,
      4: columns >= 8 padded (one finite vector in the whole row)."""
    g_ = torch.Generator(device="cpu").manual_seed(11)
    ninf = float("-inf")
    if which == "tail":
        x = torch.randn(3, 1008, generator=g_) * 3
        x[:, 1001:] = ninf
        t = torch.tensor([0, 1000, 517])
    else:
        x = torch.randn(5, 4096, generator=g_) * 3
        x[0, 2048:] = ninf
        x[1, :2048] = ninf
        x[2, :3000] = ninf
        x[4, 8:] = ninf
        t = torch.tensor([2047, 2048, 4095, 1234, 7])
    return x.to(dtype).to(device), t.to(device)


def xent_oor_inputs(dtype, device):
    """6 rows of V = 1024; rows 1 and 4 carry the out-of-range targets -100 and V"""
    g_ = torch.Generator(device="cpu").manual_seed(12)
    x = (torch.randn(6, 1024, generator=g_) * 3).to(dtype)
    t = torch.randint(0, 1024, (6,), generator=g_)
    t[1], t[4] = -100, 1024
    return x.to(device), t.to(device)


def offset_view(t):
    """the values of t as a contiguous view one element into a fresh buffer: is_contiguous() holds,
    the data pointer is 2 (bf16) / 4 (fp32) bytes off the allocation's alignment"""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 != 0
    return v


# ------------------------------------------------------------------ reporting
class Report:
    """collects max |got - ref| and the worst |got - ref| / (atol + rtol |ref|) of every output of a
    case, prints them all in one line, then asserts"""

    def __init__(self, tag):
        self.tag, self.items = tag, []

    def add(self, name, got, ref, rtol=0.0, atol=0.0, bound=None):
        got, ref = _d(got), _d(ref)
        assert got.shape == ref.shape, (name, got.shape, ref.shape)
        bound = atol + rtol * ref.abs() if bound is None else bound
        diff = (got - ref).abs()
        finite = bool(torch.isfinite(got).all())
        worst = float((diff / bound).max()) if finite and got.numel() else (0.0 if finite else math.inf)
        self.items.append((name, float(diff.max()) if finite and got.numel() else math.inf, worst))

    def merge(self, name, err, worst):
        """fold another chunk of the same output in"""
        for i, (n, e, w) in enumerate(self.items):
            if n == name:
                self.items[i] = (n, max(e, err), max(w, worst))
                return
        self.items.append((name, err, worst))

    def done(self):
        print(f"[lm-edges] {self.tag}: " + " ".join(f"{n} {e:.3e} ({w:.2f}x tol)" for n, e, w in self.items))
        bad = [(n, e, w) for n, e, w in self.items if not w <= 1.0]
        assert not bad, (self.tag, bad)


def _dt(d):
    return "bf16" if d == BF16 else "fp32"


def _sid(shape):
    return "x".join(str(v) for v in shape)


# ------------------------------------------------------------------ RMSNorm
# 4-wide kernels (D % 4 == 0, D <= 8192): (300, 512) gives P = ceil(300 / 16) = 19 partial rows, so
# colsum4's `p += 16` loop takes a second trip for lanes 0..2, and the last block holds 12 of 16 rows;
# (1, 64) one row, 16 of 256 threads busy; (17, 8) two blocks, 2 threads busy.
# scalar kernels (rmsnorm_fwd/bwd_kernel, colsum_kernel): (37, 1002) D % 4 = 2, P = ceil(37 / 8) = 5 with
# a ragged last block; (3, 7) D < one wave; (9, 16384) D % 4 == 0 but D / 4 > 2048, 64 columns per thread.
RMS_SHAPES_4 = [(300, 512), (1, 64), (17, 8)]
RMS_SHAPES_S = [(37, 1002), (3, 7), (9, 16384)]
RMS_CASES = [(r, D, xd, wd) for r, D in RMS_SHAPES_4 for xd, wd in ((F32, F32), (BF16, F32), (BF16, BF16))] + \
            [(r, D, xd, wd) for r, D in RMS_SHAPES_S for xd, wd in ((F32, F32), (BF16, BF16), (F32, BF16))]


def _rms_inputs(rows, D, xdt, wdt, device, seed=0):
    g_ = torch.Generator(device="cpu").manual_seed(seed + rows * 100003 + D)
    x = torch.randn(rows, D, generator=g_).to(xdt).to(device)
    w = (torch.rand(D, generator=g_) + 0.5).to(wdt).to(device)
    gy = torch.randn(rows, D, generator=g_).to(xdt).to(device)
    return x, w, gy


def _rms_check(rep, y, dx, dw, x, w, gy):
    """forward / dx by the TOL of x's dtype; dw by the weight-gradient tolerance of x's dtype, or, for a
    bf16 weight (dw itself rounded to bf16): one bf16 rounding of the exact value, 2^-8 |ref|, plus the
    fp32 atol"""
    ry, rdx, rdw = rmsnorm_oracle(x, w, gy)
    rep.add("y", y, ry, **TOL[x.dtype])
    rep.add("dx", dx, rdx, **TOL[x.dtype])
    if w.dtype == BF16:
        rep.add("dw", dw, rdw, bound=2.0 ** -8 * rdw.abs() + DW_TOL[F32]["atol"])
    else:
        rep.add("dw", dw, rdw, **DW_TOL[x.dtype])


@pytest.mark.parametrize("rows,D,xdt,wdt", RMS_CASES, ids=lambda v: _dt(v) if isinstance(v, torch.dtype) else str(v))
def test_rmsnorm_branches(dev, rows, D, xdt, wdt):
    from cs744_pytorch_distributed_tutorial_amd import _C
    from cs744_pytorch_distributed_tutorial_amd.ops import lm
    assert _C.rmsnorm_vec4(D) == ((rows, D) in RMS_SHAPES_4)
    x, w, gy = _rms_inputs(rows, D, xdt, wdt, dev)
    x.requires_grad_()
    w.requires_grad_()
    y = lm.rms_norm(x, w, EPS)
    assert y.dtype == xdt
    y.backward(gy)
    assert x.grad.dtype == xdt and w.grad.dtype == wdt
    rep = Report(f"rmsnorm ({rows}, {D}) x {_dt(xdt)} w {_dt(wdt)}")
    _rms_check(rep, y, x.grad, w.grad, x, w, gy)
    rep.done()


@pytest.mark.parametrize("D", [1002, 16384])
def test_rmsnorm_autocast_scalar_path(dev, D):
    """bf16 autocast, fp32 residual stream, a width the 4-wide kernels do not take: y stays fp32 (the
    scalar kernels write x's dtype), a bf16 upstream gradient is accepted and recast by
    _RMSNorm.backward, dx and dw match. D = 16384 is a multiple of 4 that still runs the scalar
    kernels (D > 8192)."""
    from cs744_pytorch_distributed_tutorial_amd import _C
    from cs744_pytorch_distributed_tutorial_amd.ops import lm
    rows = 6
    x, w, gy = _rms_inputs(rows, D, F32, F32, dev, seed=1)
    gyb = gy.bfloat16()
    x.requires_grad_()
    w.requires_grad_()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y = lm.rms_norm(x, w, EPS)
    assert y.dtype == F32
    y.backward(gyb)
    assert x.grad.dtype == F32 and w.grad.dtype == F32
    rep = Report(f"rmsnorm autocast ({rows}, {D})")
    _rms_check(rep, y, x.grad, w.grad, x, w, gyb)
    # the recast itself (autograd casts a bf16 gradient of an fp32 output before backward sees it)
    _, rstd = _C.rmsnorm_fwd(x.detach(), w.detach(), EPS, False)
    ctx = types.SimpleNamespace(saved_tensors=(x.detach(), w.detach(), rstd))
    dx, dw, _, _ = lm._RMSNorm.backward(ctx, gyb)
    assert torch.equal(dx, x.grad) and torch.equal(dw, w.grad)
    rep.done()


def test_rmsnorm_binding_refuses_mixed_dtypes_on_scalar_path(dev):
    from cs744_pytorch_distributed_tutorial_amd import _C
    for D in (1002, 16384):
        x, w, gy = _rms_inputs(3, D, F32, F32, dev)
        with pytest.raises(RuntimeError):
            _C.rmsnorm_fwd(x, w, EPS, True)
        _, rstd = _C.rmsnorm_fwd(x, w, EPS, False)
        with pytest.raises(RuntimeError):
            _C.rmsnorm_bwd(x, w, rstd, gy.bfloat16())
    torch.cuda.synchronize()


@pytest.mark.parametrize("dtype", [F32, BF16], ids=_dt)
def test_rmsnorm_offset_views(dev, dtype):
    """x, w and gy as contiguous views at an odd storage offset: the wrapper re-materialises them, the
    result matches the oracle and equals the aligned call bitwise; the binding refuses each of them
    before any launch"""
    from cs744_pytorch_distributed_tutorial_amd import _C
    from cs744_pytorch_distributed_tutorial_amd.ops import lm
    rows, D = 5, 512
    x, w, gy = _rms_inputs(rows, D, dtype, dtype, dev, seed=2)
    outs = []
    for view in (False, True):
        xv, wv, gv = ((offset_view(t) if view else t.clone()) for t in (x, w, gy))
        xv.requires_grad_()
        wv.requires_grad_()
        y = lm.rms_norm(xv, wv, EPS)
        y.backward(gv)
        outs.append((y.detach(), xv.grad, wv.grad))
    rep = Report(f"rmsnorm offset views ({rows}, {D}) {_dt(dtype)}")
    _rms_check(rep, *outs[1], x, w, gy)
    rep.done()
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    xo, wo, go = offset_view(x), offset_view(w), offset_view(gy)
    _, rstd = _C.rmsnorm_fwd(x, w, EPS, False)
    for args in ((xo, w), (x, wo)):
        with pytest.raises(RuntimeError, match="aligned"):
            _C.rmsnorm_fwd(*args, EPS, False)
    for args in ((xo, w, rstd, gy), (x, wo, rstd, gy), (x, w, rstd, go)):
        with pytest.raises(RuntimeError, match="aligned"):
            _C.rmsnorm_bwd(*args)
    # the scalar kernels have no vector access: the same views are fine at D % 4 != 0
    x7, w7, g7 = _rms_inputs(3, 7, dtype, dtype, dev)
    y7, r7 = _C.rmsnorm_fwd(offset_view(x7), offset_view(w7), EPS, False)
    assert torch.equal(y7, _C.rmsnorm_fwd(x7, w7, EPS, False)[0])
    torch.cuda.synchronize()


# ------------------------------------------------------------------ SwiGLU
@pytest.mark.parametrize("path", ["4wide", "scalar"])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=_dt)
def test_swiglu_extreme_gates(dev, dtype, path):
    """saturating gates: exp(-a) overflows to inf (a <= -89), underflows (a >= 88). 64 copies of every
    gate run the 4-wide kernels; the same flattened without its last element (n odd) the scalar ones"""
    from cs744_pytorch_distributed_tutorial_amd import _C
    a, b, gy = swiglu_extreme_inputs(dtype, dev, 64)
    if path == "scalar":
        a, b, gy = (t.flatten()[:-1].clone() for t in (a, b, gy))
    assert (a.numel() % 4 == 0) == (path == "4wide") and a.data_ptr() % 16 == 0
    y = _C.swiglu_fwd(a, b)
    da, db = _C.swiglu_bwd(a, b, gy)
    ry, rda, rdb = swiglu_oracle(a, b, gy)
    rep = Report(f"swiglu extreme gates {_dt(dtype)} n = {a.numel()}")
    for n, got, ref in (("y", y, ry), ("da", da, rda), ("db", db, rdb)):
        assert bool(torch.isfinite(got.float()).all()), n
        rep.add(n, got, ref, **TOL[dtype])
    rep.done()


@pytest.mark.parametrize("shape", [(4100, 4100), (2049, 2049)], ids=["4wide", "scalar"])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=_dt)
def test_swiglu_grid_stride_loop(dev, dtype, shape):
    """grid_for caps the grid at 16384 blocks of 256 threads = 4,194,304 items per sweep.
    (4100, 4100): n / 4 = 4,202,500 quads, the 4-wide loop's second sweep covers the last 8,196;
    (2049, 2049): n = 4,198,401 is odd, the scalar loop's second sweep covers the last 4,097."""
    from cs744_pytorch_distributed_tutorial_amd import _C
    n = shape[0] * shape[1]
    assert (n // 4 if n % 4 == 0 else n) > 16384 * 256
    torch.manual_seed(3)
    a = torch.randn(shape, device=dev).to(dtype)
    b = torch.randn(shape, device=dev).to(dtype)
    gy = torch.randn(shape, device=dev).to(dtype)
    y = _C.swiglu_fwd(a, b)
    da, db = _C.swiglu_bwd(a, b, gy)
    rep = Report(f"swiglu loop {shape} {_dt(dtype)}")
    for lo in range(0, shape[0], 512):  # the fp64 oracle a slab of rows at a time: bounded memory
        sl = slice(lo, min(lo + 512, shape[0]))
        part = Report("")
        for name, got, ref in zip(("y", "da", "db"), (y, da, db), swiglu_oracle(a[sl], b[sl], gy[sl])):
            part.add(name, got[sl], ref, **TOL[dtype])
        for item in part.items:
            rep.merge(*item)
    rep.done()


@pytest.mark.parametrize("dtype", [F32, BF16], ids=_dt)
def test_swiglu_offset_views(dev, dtype):
    """n % 4 == 0 but aligned16() false: the scalar kernels run. They do the same arithmetic per
    element as the 4-wide ones, so the result equals the aligned call bitwise."""
    from cs744_pytorch_distributed_tutorial_amd import _C
    shape = (3, 17, 352)
    torch.manual_seed(4)
    a, b, gy = (torch.randn(shape, device=dev).to(dtype) for _ in range(3))
    av, bv, gv = offset_view(a), offset_view(b), offset_view(gy)
    y, (da, db) = _C.swiglu_fwd(av, bv), _C.swiglu_bwd(av, bv, gv)
    rep = Report(f"swiglu offset views {shape} {_dt(dtype)}")
    for name, got, ref in zip(("y", "da", "db"), (y, da, db), swiglu_oracle(a, b, gy)):
        rep.add(name, got, ref, **TOL[dtype])
    rep.done()
    y4, (da4, db4) = _C.swiglu_fwd(a, b), _C.swiglu_bwd(a, b, gy)
    for name, s, v in (("y", y, y4), ("da", da, da4), ("db", db, db4)):
        assert torch.equal(s, v), (name, int((s != v).sum()), float((s.float() - v.float()).abs().max()))


# ------------------------------------------------------------------ RoPE
def _rope_inputs(shape, dtype, device, seed=5):
    from cs744_pytorch_distributed_tutorial_amd.models.llama import rope_tables
    B, S, H, hd = shape
    cos, sin = rope_tables(S, hd, 500000.0, device)
    g_ = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn(shape, generator=g_).to(dtype).to(device)
    gy = torch.randn(shape, generator=g_).to(dtype).to(device)
    return x, gy, cos, sin


# (2, 5, 3, 128): the model's head dim; (1, 3, 2, 2): half = 1, every pair its own row;
# (2, 33, 8, 128): B > 1, the position index (rowi / H) % S wraps at the batch boundary
ROPE_SHAPES = [(2, 5, 3, 128), (1, 3, 2, 2), (2, 33, 8, 128)]


@pytest.mark.parametrize("shape", ROPE_SHAPES, ids=_sid)
@pytest.mark.parametrize("dtype", [F32, BF16], ids=_dt)
def test_rope_shapes(dev, dtype, shape):
    from cs744_pytorch_distributed_tutorial_amd import _C
    from cs744_pytorch_distributed_tutorial_amd.ops import lm
    x, gy, cos, sin = _rope_inputs(shape, dtype, dev)
    x.requires_grad_()
    y = lm.rope(x, cos, sin)
    y.backward(gy)
    ry, rdx = rope_oracle(x, cos, sin, gy)
    rep = Report(f"rope {shape} {_dt(dtype)}")
    rep.add("y", y, ry, **TOL[dtype])
    rep.add("dx", x.grad, rdx, **TOL[dtype])
    # rope then its inverse returns x. With u = 2^-24 and n the pair's Euclidean norm: a rotation
    # computes each component as fl(fl(p) -+ fl(q)) with |p| + |q| <= sqrt(2) n, error <= 3 u n; the
    # fp32 tables have c^2 + s^2 = 1 + O(4 u); two rotations: (4 + 2 * 3) u n, bound 16 u n.
    # bf16 (8 significant bits, one rounding costs at most ub = 2^-8 of the value) rounds twice:
    # the intermediate pair (each component by <= ub |y_i|, an error vector of norm <= ub n, which the
    # inverse rotation can turn wholly into one component) and the result (ub |x_i|, at most ub n). No
    # bound in |x_i| alone can hold for a component much smaller than its partner; the two roundings
    # give ub (n + |x_i|), asserted with (1 + 2 ub) for the second rounding acting on a value already
    # off by the first.
    back = _C.rope(_C.rope(x.detach(), cos, sin, False), cos, sin, True)
    n = _d(x).reshape(*shape[:-1], -1, 2).norm(dim=-1, keepdim=True).expand(*shape[:-1], shape[-1] // 2, 2).reshape(shape)
    ub = 2.0 ** -8 if dtype == BF16 else 0.0
    rep.add("inverse", back, x, bound=16 * 2.0 ** -24 * n + ub * (1 + 2 * ub) * (n + _d(x).abs()) + 1e-30)
    rep.done()


def test_rope_grid_stride_loop(dev):
    """(1, 2050, 32, 128) bf16: 4,198,400 pairs > 4,194,304, the loop's second sweep covers the last
    4,096 pairs (position 2049)"""
    from cs744_pytorch_distributed_tutorial_amd import _C
    shape = (1, 2050, 32, 128)
    assert shape[1] * shape[2] * shape[3] // 2 > 16384 * 256
    x, gy, cos, sin = _rope_inputs(shape, BF16, dev)
    y, dx = _C.rope(x, cos, sin, False), _C.rope(gy, cos, sin, True)
    rep = Report(f"rope loop {shape} bf16")
    for lo in range(0, shape[1], 256):
        sl = slice(lo, min(lo + 256, shape[1]))
        ry, rdx = rope_oracle(x[:, sl], cos[sl], sin[sl], gy[:, sl])
        part = Report("")
        part.add("y", y[:, sl], ry, **TOL[BF16])
        part.add("dx", dx[:, sl], rdx, **TOL[BF16])
        for item in part.items:
            rep.merge(*item)
    rep.done()


# ------------------------------------------------------------------ cross-entropy
def _xent_run(x, t, g=2.5):
    """_C.xent_fwd / xent_bwd -> per-row loss, lse, dlogits"""
    from cs744_pytorch_distributed_tutorial_amd import _C
    loss, lse = _C.xent_fwd(x, t)
    gs = torch.full((1,), g, device=x.device)
    return loss, lse, _C.xent_bwd(x, t, lse, gs, 1.0 / x.shape[0])


# (5, 8): one 8-vector, one busy thread; (3, 2048): every thread exactly one vector; (2, 2056): thread
# 0 alone takes a second trip; (1, 128256): the Llama-3 vocabulary, 62.6 trips
@pytest.mark.parametrize("R,V", [(5, 8), (3, 2048), (2, 2056), (1, 128256)])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=_dt)
def test_cross_entropy_rows(dev, dtype, R, V):
    from cs744_pytorch_distributed_tutorial_amd.ops import lm
    g_ = torch.Generator(device="cpu").manual_seed(V)
    x = (torch.randn(R, V, generator=g_) * 3).to(dtype).to(dev)
    t = torch.randint(0, V, (R,), generator=g_).to(dev)
    loss, lse, d = _xent_run(x, t)
    rloss, rlse, rd = xent_oracle(x, t, 2.5)
    rep = Report(f"xent rows ({R}, {V}) {_dt(dtype)}")
    rep.add("loss", loss, rloss, **XENT_LOSS_TOL)
    rep.add("lse", lse, rlse, **XENT_LOSS_TOL)
    rep.add("dlogits", d, rd, **XENT_GRAD_TOL[dtype])
    xa = x.clone().requires_grad_()
    mean = lm.cross_entropy(xa, t)
    (2.5 * mean).backward()
    rep.add("mean", mean, rloss.mean(), **XENT_LOSS_TOL)
    rep.add("autograd", xa.grad, rd, **XENT_GRAD_TOL[dtype])
    rep.done()


@pytest.mark.parametrize("c", [95.0, -95.0])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=_dt)
def test_cross_entropy_shifted_logits(dev, dtype, c):
    """logits near +-95: exp(95) = 1.8e41 overflows fp32, exp(-95) = 5e-42 is subnormal, so a sum of
    plain exponentials would give lse = +-inf; the online maximum keeps every exponent <= 0."""
    R, V = 3, 2056
    g_ = torch.Generator(device="cpu").manual_seed(int(c) + 200)
    x = (torch.randn(R, V, generator=g_) * 3 + c).to(dtype).to(dev)
    t = torch.randint(0, V, (R,), generator=g_).to(dev)
    loss, lse, d = _xent_run(x, t)
    rloss, rlse, rd = xent_oracle(x, t, 2.5)
    # The kernel forms l = fl(m + fl(log s)) and loss = fl(l - x_t), all fp32. With M = max |logit| and
    # U = ulp_fp32(M): |l| <= M + ln V may reach the next binade, ulp(l) <= 2 U, so the rounding of l
    # costs <= U, that of the difference (|loss| < |l|) <= U, and log s (s in [1, V], v_log_f32 and a
    # multiply) about 1e-6. 2 U + 1e-6 in all; asserted: 4 U + 1e-5, and not the rtol of the unshifted
    # test, which at |lse| = 100 would allow 1e-3.
    M = float(x.float().abs().max())
    U = 2.0 ** (math.floor(math.log2(M)) - 23)
    rep = Report(f"xent shifted {c:+.0f} {_dt(dtype)} (max |logit| {M:.1f}, bound {4 * U + 1e-5:.2e})")
    rep.add("loss", loss, rloss, atol=4 * U + 1e-5)
    rep.add("lse", lse, rlse, atol=4 * U + 1e-5)
    rep.add("dlogits", d, rd, **XENT_GRAD_TOL[dtype])
    rep.done()


@pytest.mark.parametrize("which", ["tail", "half"])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=_dt)
def test_cross_entropy_neg_inf_padding(dev, dtype, which):
    x, t = xent_pad_inputs(dtype, dev, which)
    loss, lse, d = _xent_run(x, t)
    rloss, rlse, rd = xent_oracle(x, t, 2.5)
    rep = Report(f"xent -inf padding {which} {tuple(x.shape)} {_dt(dtype)}")
    rep.add("loss", loss, rloss, **XENT_LOSS_TOL)
    rep.add("lse", lse, rlse, **XENT_LOSS_TOL)
    rep.add("dlogits", d, rd, **XENT_GRAD_TOL[dtype])
    rep.done()
    pad = torch.isinf(x)
    assert bool(pad.any()) and bool((d[pad] == 0).all())


@pytest.mark.parametrize("dtype", [F32, BF16], ids=_dt)
def test_cross_entropy_out_of_range_targets(dev, dtype):
    x, t = xent_oor_inputs(dtype, dev)
    bad = (t < 0) | (t >= x.shape[1])
    assert int(bad.sum()) == 2
    loss, lse, d = _xent_run(x, t)
    rloss, rlse, rd = xent_oracle(x, t, 2.5)
    assert torch.equal(torch.isnan(loss), bad)
    assert bool(torch.isfinite(d.float()).all())
    rep = Report(f"xent out-of-range targets {tuple(x.shape)} {_dt(dtype)}")
    rep.add("loss", loss[~bad], rloss[~bad], **XENT_LOSS_TOL)
    rep.add("lse", lse, rlse, **XENT_LOSS_TOL)
    rep.add("dlogits", d, rd, **XENT_GRAD_TOL[dtype])  # rd's bad rows: softmax * g / R, no one-hot
    rep.done()


@pytest.mark.parametrize("dtype", [F32, BF16], ids=_dt)
def test_cross_entropy_offset_view(dev, dtype):
    """logits as a contiguous view at an odd storage offset: the wrapper re-materialises them; the
    binding refuses them before any launch"""
    from cs744_pytorch_distributed_tutorial_amd import _C
    from cs744_pytorch_distributed_tutorial_amd.ops import lm
    R, V = 4, 2056
    g_ = torch.Generator(device="cpu").manual_seed(13)
    x = (torch.randn(R, V, generator=g_) * 3).to(dtype).to(dev)
    t = torch.randint(0, V, (R,), generator=g_).to(dev)
    outs = []
    for view in (False, True):
        xv = (offset_view(x) if view else x.clone()).requires_grad_()
        mean = lm.cross_entropy(xv, t)
        (2.5 * mean).backward()
        outs.append((mean.detach(), xv.grad))
    rloss, _, rd = xent_oracle(x, t, 2.5)
    rep = Report(f"xent offset view ({R}, {V}) {_dt(dtype)}")
    rep.add("mean", outs[1][0], rloss.mean(), **XENT_LOSS_TOL)
    rep.add("autograd", outs[1][1], rd, **XENT_GRAD_TOL[dtype])
    rep.done()
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    xo = offset_view(x)
    _, lse = _C.xent_fwd(x, t)
    with pytest.raises(RuntimeError, match="aligned"):
        _C.xent_fwd(xo, t)
    with pytest.raises(RuntimeError, match="aligned"):
        _C.xent_bwd(xo, t, lse, torch.ones(1, device=dev), 1.0 / R)
    torch.cuda.synchronize()
