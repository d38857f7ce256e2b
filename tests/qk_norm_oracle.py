"""Float64 oracle of QK-norm fused with RoPE (ops.lm.qk_norm_rope), shared by test_qk_norm_cpu.py and
test_qk_norm_gpu.py: the forward formula and the hand-written backward formulas, evaluated on the
inputs as stored (bf16 inputs are upcast exactly), and the error measures of both files."""
import torch

# per head-row max|err| / max|oracle|: the project's fp32 tolerance (tests/test_lm_gpu.py), and for bf16
# one rounding (half an ulp = 2^-8) plus fp32 noise
ROW_TOL = {torch.float32: 1e-5, torch.bfloat16: 2.0 ** -7}
# |dw - dw64| <= DW_TOL * sum_rows |t| per column: a chain of n <= 1040 fp32 additions errs by at most
# (n - 1) * 2^-24 * sum|t| <= 6.2e-5 * sum|t|, whatever its order
DW_TOL = 1e-4
MAX_ROWS = 1040


EPS = 1e-5
# (B, S, Hq, Hkv, hd, input scale): ragged S with GQA (q has exactly MAX_ROWS rows); the hd = 64 row
# packing with MHA; Hkv = 1; one row (a wave mostly idle); eps matters / r is tiny
CASES = [(2, 130, 4, 2, 128, 1.0), (3, 33, 8, 8, 64, 1.0), (2, 65, 4, 1, 128, 1.0), (1, 1, 1, 1, 64, 1.0),
         (2, 33, 4, 2, 64, 1e-3), (2, 33, 4, 2, 64, 1e3)]


def make_inputs(case, dtype, device, seed=0):
    """q, k, wq, wk, cos, sin, gq, gk drawn on the CPU from one seed (the same values on every device)"""
    from cs744_pytorch_distributed_tutorial_amd.models.llama import rope_tables
    B, S, Hq, Hkv, hd, scale = case
    g = torch.Generator().manual_seed(seed)
    q = (torch.randn(B, S, Hq, hd, generator=g) * scale).to(dtype)
    k = (torch.randn(B, S, Hkv, hd, generator=g) * scale).to(dtype)
    wq, wk = torch.rand(hd, generator=g) + 0.5, torch.rand(hd, generator=g) + 0.5
    gq = torch.randn(B, S, Hq, hd, generator=g).to(dtype)
    gk = torch.randn(B, S, Hkv, hd, generator=g).to(dtype)
    cos, sin = rope_tables(S, hd, 500000.0, torch.device("cpu"))
    return tuple(t.to(device) for t in (q, k, wq, wk, cos, sin, gq, gk))


def check_against_oracle(inp, outs, grads, dtype, tag=""):
    """assert the bounds of the module docstring on (q', k') and (dq, dk, dwq, dwk); grads may be None"""
    q, k, wq, wk, cos, sin, gq, gk = inp
    tol = ROW_TOL[dtype]
    for name, got, want in zip(("q'", "k'"), outs, forward(q, k, wq, wk, cos, sin, EPS)):
        assert got.dtype == dtype and got.shape == want.shape
        e = row_err(got, want)
        print(f"[qk-norm] {tag} {name} row err {e:.3e} (bound {tol:.3e})")
        assert e <= tol, (tag, name, e)
    if grads is None:
        return
    dq, dk, dwq, dwk, tq, tk = backward(q, k, wq, wk, cos, sin, gq, gk, EPS)
    for name, got, want in zip(("dq", "dk"), grads[:2], (dq, dk)):
        assert got.dtype == dtype and got.shape == want.shape
        e = row_err(got, want)
        print(f"[qk-norm] {tag} {name} row err {e:.3e} (bound {tol:.3e})")
        assert e <= tol, (tag, name, e)
    if len(grads) > 2:
        for name, got, want, ts in zip(("dwq", "dwk"), grads[2:], (dwq, dwk), (tq, tk)):
            assert got.dtype == torch.float32 and got.shape == want.shape
            e = dw_err(got, want, ts)
            print(f"[qk-norm] {tag} {name} err / sum|t| {e:.3e} (bound {DW_TOL:.0e})")
            assert e <= DW_TOL, (tag, name, e)


def _d(t):
    return t.double().cpu()  # no detach: float64 autograd can run through forward()


def _rot(n, cos, sin, S, sign=1.0):
    """rotate the pairs (2j, 2j+1) of n [B, S, H, hd] by the angle (s, j); sign = -1: the transpose"""
    c, s = cos[:S][None, :, None, :], sign * sin[:S][None, :, None, :]
    p = n.reshape(*n.shape[:-1], -1, 2)
    n0, n1 = p[..., 0], p[..., 1]
    return torch.stack([n0 * c - n1 * s, n0 * s + n1 * c], -1).reshape(n.shape)


def forward(q, k, wq, wk, cos, sin, eps):
    """(q', k') in float64 on the CPU"""
    cos, sin = _d(cos), _d(sin)

    def one(x, w):
        x, w = _d(x), _d(w)
        r = torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps)
        return _rot(x * r * w, cos, sin, x.shape[1])

    return one(q, wq), one(k, wk)


def backward(q, k, wq, wk, cos, sin, gq, gk, eps):
    """(dq, dk, dwq, dwk, sum|t|_q, sum|t|_k) in float64: gn = R^T g, xh = x r, c = mean(w gn xh),
    dx = r (w gn - xh c), t = gn xh, dw = sum over the head-rows of t"""
    cos, sin = _d(cos), _d(sin)

    def one(x, w, g):
        x, w, g = _d(x), _d(w), _d(g)
        r = torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps)
        gn = _rot(g, cos, sin, x.shape[1], -1.0)
        xh = x * r
        c = (w * gn * xh).mean(-1, keepdim=True)
        t = (gn * xh).reshape(-1, x.shape[-1])
        return r * (w * gn - xh * c), t.sum(0), t.abs().sum(0)

    dq, dwq, tq = one(q, wq, gq)
    dk, dwk, tk = one(k, wk, gk)
    return dq, dk, dwq, dwk, tq, tk


def row_err(got, want):
    """the largest max|err| / max|oracle| over the head-rows; a row whose oracle is all zero must be
    reproduced exactly (it then counts 0, otherwise inf)"""
    hd = want.shape[-1]
    err = (_d(got) - want).abs().reshape(-1, hd).amax(1)
    ref = want.abs().reshape(-1, hd).amax(1)
    ratio = torch.where(ref > 0, err / ref.clamp_min(1e-300), torch.where(err > 0, float("inf"), 0.0).double())
    return float(ratio.max()) if ratio.numel() else 0.0


def dw_err(got, want, tsum):
    """the largest |dw - dw64| / sum|t| over the columns (a column with sum|t| = 0 must be exactly 0)"""
    err = (_d(got) - want).abs()
    ratio = torch.where(tsum > 0, err / tsum.clamp_min(1e-300), torch.where(err > 0, float("inf"), 0.0).double())
    return float(ratio.max())
