"""The float64 oracles and input builders of tests/test_lm_edges_gpu.py and
tests/test_attention_edges_gpu.py against the project's own fp32 references (ops.lm.*_ref,
F.cross_entropy, ops.attention.attention_ref with autograd) on CPU tensors: a wrong formula or a
badly built input is found here, before a GPU test compares a kernel with it. The references get the
same values in fp32 (bf16 values are exact in fp32), so the only difference is fp32 rounding."""
import math

import pytest
import torch

import test_attention_edges_gpu as ae
import test_lm_edges_gpu as le

F32, BF16 = torch.float32, torch.bfloat16
CPU = torch.device("cpu")
REF_TOL = dict(rtol=1e-4, atol=1e-5)  # the fp32 references' own rounding


def _autograd(fn, inputs, gy):
    ins = [t.detach().float().requires_grad_() for t in inputs]
    out = fn(*ins)
    out.backward(gy.float())
    return [out.detach()] + [t.grad for t in ins]


def _close(names, got, ref, **tol):
    for n, a, r in zip(names, got, ref):
        torch.testing.assert_close(a, r.double(), **tol, msg=lambda m, n=n: f"{n}: {m}")


@pytest.mark.parametrize("rows,D", [(17, 8), (1, 64), (3, 7), (37, 1002)])
@pytest.mark.parametrize("xdt,wdt", [(F32, F32), (BF16, BF16), (F32, BF16)])
def test_rmsnorm_oracle(rows, D, xdt, wdt):
    from cs744_pytorch_distributed_tutorial_amd.ops import lm
    x, w, gy = le._rms_inputs(rows, D, xdt, wdt, CPU)
    assert x.dtype == xdt and w.dtype == wdt and gy.dtype == xdt and float(w.float().min()) >= 0.5
    ref = _autograd(lambda a, b: lm.rms_norm_ref(a, b, le.EPS), [x, w], gy)
    _close(("y", "dx", "dw"), le.rmsnorm_oracle(x, w, gy), ref, **REF_TOL)


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_swiglu_oracle_and_extreme_inputs(dtype):
    from cs744_pytorch_distributed_tutorial_amd.ops import lm
    a, b, gy = le.swiglu_extreme_inputs(dtype, CPU, 64)
    gates = set(a[:, 0].double().tolist())
    want = {s * float(torch.tensor(v, dtype=torch.float64).to(dtype)) for v in le.SWIGLU_GATES for s in (1.0, -1.0)}
    assert gates == want | ({le.BF16_MAX, -le.BF16_MAX} if dtype == BF16 else set())
    assert bool((a == a[:, :1]).all()) and float(b.float().abs().max()) <= 1 and float(gy.float().abs().max()) <= 1
    got = le.swiglu_oracle(a, b, gy)
    for t in got:  # the exact results are finite and representable in dtype
        assert bool(torch.isfinite(t.to(dtype)).all())
    _close(("y", "da", "db"), got, _autograd(lm.swiglu_ref, [a, b], gy), rtol=1e-5, atol=1e-6)
    torch.manual_seed(0)
    a, b, gy = (torch.randn(5, 7, 9).to(dtype) for _ in range(3))
    _close(("y", "da", "db"), le.swiglu_oracle(a, b, gy), _autograd(lm.swiglu_ref, [a, b], gy), **REF_TOL)


@pytest.mark.parametrize("shape", le.ROPE_SHAPES, ids=le._sid)
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_rope_oracle(dtype, shape):
    from cs744_pytorch_distributed_tutorial_amd.ops import lm
    x, gy, cos, sin = le._rope_inputs(shape, dtype, CPU)
    assert cos.shape == (shape[1], shape[3] // 2) and cos.dtype == F32
    ref = _autograd(lambda t: lm.rope_ref(t, cos, sin), [x], gy)
    _close(("y", "dx"), le.rope_oracle(x, cos, sin, gy), ref, **REF_TOL)


def _xent_torch(x, t, g):
    """F.cross_entropy in float64 per row and the gradient of g * mean"""
    xr = x.detach().double().requires_grad_()
    loss = torch.nn.functional.cross_entropy(xr, t, reduction="none")
    (g * loss.mean()).backward()
    return loss.detach(), xr.grad


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_xent_oracle(dtype):
    tol = dict(rtol=1e-12, atol=1e-12)
    g_ = torch.Generator().manual_seed(1)
    x = (torch.randn(5, 8, generator=g_) * 3 + 95).to(dtype)
    t = torch.randint(0, 8, (5,), generator=g_)
    loss, lse, d = le.xent_oracle(x, t, 2.5)
    rloss, rd = _xent_torch(x, t, 2.5)
    _close(("loss", "lse", "d"), (loss, lse, d), (rloss, rloss + x.double().gather(1, t[:, None])[:, 0], rd), **tol)
    for which, shape, npad in (("tail", (3, 1008), 3 * 7), ("half", (5, 4096), 2048 + 2048 + 3000 + 4088)):
        x, t = le.xent_pad_inputs(dtype, CPU, which)
        assert x.shape == shape and x.dtype == dtype and int(torch.isinf(x).sum()) == npad
        assert bool(torch.isfinite(x.gather(1, t[:, None])).all())  # targets in the finite columns
        loss, lse, d = le.xent_oracle(x, t, 2.5)
        rloss, rd = _xent_torch(x, t, 2.5)
        assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(d).all())
        _close(("loss", "d"), (loss, d), (rloss, rd), **tol)
        assert bool((d[torch.isinf(x)] == 0).all())


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_xent_oracle_out_of_range_targets(dtype):
    x, t = le.xent_oor_inputs(dtype, CPU)
    R, V = x.shape
    bad = (t < 0) | (t >= V)
    assert bad.tolist() == [False, True, False, False, True, False] and t[1] == -100 and t[4] == V
    loss, lse, d = le.xent_oracle(x, t, 2.5)
    assert torch.equal(torch.isnan(loss), bad)
    # the valid rows: F.cross_entropy over them alone, its mean rescaled to the R rows of the batch
    rloss, rd = _xent_torch(x[~bad], t[~bad], 2.5 * int((~bad).sum()) / R)
    _close(("loss", "d"), (loss[~bad], d[~bad]), (rloss, rd), rtol=1e-12, atol=1e-12)
    # the others: softmax * g / R, no one-hot
    _close(("d",), (d[bad],), (torch.softmax(x[bad].double(), -1) * 2.5 / R,), rtol=1e-12, atol=1e-15)
    _close(("lse",), (lse,), (torch.log(torch.exp(x.double()).sum(-1)),), rtol=1e-12, atol=1e-12)


def test_offset_view_and_aligned_helper():
    """offset_view builds what the alignment guard is for; ops.lm._aligned copies exactly that"""
    from cs744_pytorch_distributed_tutorial_amd.ops import lm
    for dtype in (F32, BF16):
        t = torch.randn(5, 512).to(dtype)
        v = le.offset_view(t)
        assert v.is_contiguous() and v.data_ptr() % 16 == t.element_size() and torch.equal(v, t)
        a = lm._aligned(v)
        assert a.data_ptr() % 16 == 0 and a.is_contiguous() and torch.equal(a, t)
        assert lm._aligned(t) is t
        nc = t.t()
        assert lm._aligned(nc).is_contiguous() and torch.equal(lm._aligned(nc), nc)


@pytest.mark.parametrize("i", range(len(ae.CASES)), ids=[ae._cid(c) for c in ae.CASES])
def test_attention_oracle(i):
    from cs744_pytorch_distributed_tutorial_amd.ops.attention import attention_ref
    B, S, Hq, Hkv, D, causal, qs = ae.CASES[i]
    q, k, v, do = ae.inputs(i, CPU)
    assert q.shape == (B, S, Hq, D) and k.shape == v.shape == (B, S, Hkv, D) and q.dtype == BF16
    o, lse, dq, dk, dv = ae.attention_oracle(q, k, v, do, causal)
    ref = _autograd(lambda a, b, c: attention_ref(a, b, c, causal), [q, k, v], do)
    # gradients of peaked scores cancel (dS = P (dP - delta) with P close to one-hot): fp32 keeps less
    tol = dict(rtol=1e-3, atol=1e-4) if qs != 1 else REF_TOL
    _close(("o", "dq", "dk", "dv"), (o, dq, dk, dv), ref, **tol)
    if S == 1:
        assert not bool(dq.any()) and not bool(dk.any())
    if causal:
        assert not bool(dq[:, 0].any())  # the first query sees one key: dS = 0
    # lse (base 2) as tests/test_attention_gpu.py::test_flash_attention_lse computes it, in fp32
    rep = Hq // Hkv
    s = (q.float().transpose(1, 2) @ k.float().repeat_interleave(rep, dim=2).transpose(1, 2).transpose(-1, -2)) / math.sqrt(D)
    if causal:
        s = s.masked_fill(torch.ones(S, S, dtype=torch.bool).triu(1), float("-inf"))
    torch.testing.assert_close(lse, (torch.logsumexp(s, -1) / math.log(2.0)).double(), rtol=1e-5, atol=1e-4)
