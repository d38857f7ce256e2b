"""Float64 oracles, input builders and derived error bounds for the NHWC fp32 BatchNorm + ReLU
(+ 2x2 max-pool) kernels (csrc/kernels/bn.hip, bn_device.h, bn_fin.h) and the BN-backward partial
sums of the data-gradient GEMM (conv_common.h dgrad_bn_partials, conv_gemm.hip splitk_reduce_body).

Everything runs on CPU tensors. The formulas are those in the header of bn.hip. Every error is
taken per channel (or per element), never against a tensor-wide maximum. The bounds are derived in
docs/bn_edge_tests.md; nothing here is tuned to what the kernels give.

Conventions
* Values the launchers round to fp32 (momentum, eps) enter the oracle as that fp32 value.
* Decisions (ReLU mask, pool argmax) follow tests/test_native_engine_gpu.py::_FixedDecisionVGG: z is
  the exact y * scale + shift rounded once to fp32 (the kernels' fma), the argmax is the first
  maximum in window order (strict ``>``), the mask is the strict ``z > 0``.
"""
import math

import torch

U = 2.0 ** -24  # fp32 unit roundoff


def f32(v):
    """the fp32 value a launcher's (float) cast gives, as a Python float"""
    return float(torch.tensor(v, dtype=torch.float32))


# ---------------------------------------------------------------------------------------------- builders
def ladder(B, H, W, seed=0):
    """Case (c): 16 channels with means in {0, +-1, +-30, +-1000} and standard deviations from 1e-3
    to 10; channel 15 is constant (M2 exactly 0). -> (y [B, H, W, 16] fp32, gamma, beta)."""
    g = torch.Generator().manual_seed(seed)
    means = torch.tensor([0, 1, -1, 30, -30, 1000, -1000, 0, 1, -30, 1000, -1000, 30, -1, 1000, 30.0],
                         dtype=torch.float64)
    stds = torch.tensor([1, 1e-3, 10, 1e-2, 1, 1e-3, 10, 1e-3, 1e-1, 10, 1, 1e-2, 1e-3, 1e-2, 1e-1, 0.0],
                        dtype=torch.float64)
    y = (torch.randn(B, H, W, 16, generator=g, dtype=torch.float64) * stds + means).float()
    gamma = torch.tensor([1, -1, 0, 1e-3, 1e3, 0.5, -2, 1e3, -1e-3, 1, 0, 1e-3, -1e3, 2, 1, 1], dtype=torch.float32)
    beta = torch.tensor([0, 0.5, -0.5, 1, -1, 0.25, 0, 2, -2, 0.1, 1, 0, 0.5, -0.1, 0, 3], dtype=torch.float32)
    return y, gamma, beta


def ordinary(B, H, W, C, seed=0):
    """Per-channel statistics that differ: mean in [-2, 2], std in [0.25, 4]; gamma of both signs."""
    g = torch.Generator().manual_seed(1000 + seed)
    mu = torch.rand(C, generator=g, dtype=torch.float64) * 4 - 2
    sd = 0.25 * 16 ** torch.rand(C, generator=g, dtype=torch.float64)
    y = (torch.randn(B, H, W, C, generator=g, dtype=torch.float64) * sd + mu).float()
    gamma = ((torch.rand(C, generator=g) + 0.5) * torch.where(torch.rand(C, generator=g) < 0.25, -1.0, 1.0)).float()
    beta = torch.randn(C, generator=g).float()
    return y, gamma, beta


def grad_like(B, H, W, C, pool, seed=0):
    g = torch.Generator().manual_seed(2000 + seed)
    Ho, Wo = (H // 2, W // 2) if pool else (H, W)
    return torch.randn(B, Ho, Wo, C, generator=g).float()


def coeffs_from(y, gamma, beta, eps=1e-5):
    """fp32 (scale, shift, mean, invstd) of y's float64 batch statistics (a consistent forward)."""
    y2 = y.double().reshape(-1, y.shape[-1])
    mean, var = y2.mean(0), y2.var(0, unbiased=False)
    inv = 1.0 / torch.sqrt(var + eps)
    return ((gamma.double() * inv).float(), (beta.double() - mean * gamma.double() * inv).float(), mean.float(),
            inv.float())


def tie_case(kind, B=2, H=4, W=4, C=16, seed=0):
    """Case (g): supplied-coefficient decision cases, pooled. -> dict(y, G, scale, shift, mean, invstd,
    gamma). Products y * scale are exact in fp32 (scale a power of two or 0), so the kernels' z
    equals the oracle's whether or not the compiler contracts the fma."""
    g = torch.Generator().manual_seed(3000 + seed)
    one = torch.ones(C)
    d = dict(G=torch.randn(B, H // 2, W // 2, C, generator=g).float(), mean=(0.25 * torch.randn(C, generator=g)).float(),
             invstd=(torch.rand(C, generator=g) + 0.5).float(), gamma=(torch.rand(C, generator=g) + 0.5).float(),
             scale=one.clone(), shift=torch.zeros(C))
    # small integers / 8: every value, and its double, exactly representable
    y = (torch.randint(-16, 8, (B, H, W, C), generator=g).float() / 8.0)
    win = y.view(B, H // 2, 2, W // 2, 2, C)  # [b, ho, i, wo, j, c]; window position p = 2 i + j
    if kind.startswith("pos"):  # equal positive maxima at the positions in kind[3:]
        for p in (int(ch) for ch in kind[3:]):
            win[:, :, p // 2, :, p % 2, :] = 3.0
    elif kind == "zero":  # z exactly 0 at the window maximum: y = +-0, every other value negative
        win.copy_(-win.abs() - 0.125)
        win[:, :, 0, :, 1, :] = 0.0
        win[:, :, 1, :, 0, :] = -0.0
    elif kind == "negscale":
        d["scale"] = -2.0 * one
        d["shift"] = 0.5 * one
    elif kind == "scale0":  # every z equals shift > 0: every window a four-way tie
        d["scale"] = torch.zeros(C)
        d["shift"] = 0.75 * one
        d["gamma"] = torch.zeros(C)
    else:
        raise ValueError(kind)
    d["y"] = y
    return d


def build(builder, shape):
    return builder(*shape[:3]) if builder is ladder else builder(*shape)


# (name, builder, (B, H, W, C), R): every forward input of tests/test_bn_edges_gpu.py (the CPU file runs
# an fp32 evaluation over the same list). Cases (a), (b) = (f) one unit, (c), (e), (d) finalize alone,
# (f), and (d)'s T = 511 / 512 / 513 at R = 2.
FWD_CASES = [("a", ordinary, (2, 4, 4, 16), 8), ("b", ordinary, (1, 1, 1, 16), 1),
             ("c16", ladder, (2, 8, 8, 16), 16), ("c7", ladder, (2, 8, 8, 16), 7), ("c512", ladder, (4, 32, 32, 16), 8),
             ("e1", ordinary, (3, 2, 8, 16), 7), ("e2", ordinary, (2, 8, 2, 16), 7), ("e3", ordinary, (1, 2, 2, 4), 3),
             ("d5", ordinary, (3, 2, 8, 5), 7), ("d6", ordinary, (3, 2, 8, 6), 7),
             ("f257", ordinary, (257, 1, 1, 16), 16), ("f65", ordinary, (65, 2, 2, 16), 16),
             ("f1024", ordinary, (33, 8, 8, 1024), 64)]
FWD_CASES += [(f"d{T}-{C}", ordinary, (T, 1, 2, C), 2) for T in (511, 512, 513) for C in (8, 12, 64)]
# ((B, H, W, C), pool): the backward shapes of cases (h) and (i)
BWD_CASES = [((2, 4, 4, C), p) for C in (4, 12, 20, 1024) for p in (True, False)]
BWD_CASES += [((5, 32, 32, 512), False), ((3, 2, 8, 16), True), ((3, 2, 8, 16), False), ((2, 8, 2, 16), True),
              ((2, 8, 2, 16), False), ((1, 2, 2, 4), True), ((1, 2, 2, 4), False)]
TIE_KINDS = ["pos01", "pos12", "pos23", "pos03", "pos0123", "zero", "negscale", "scale0"]


# ---------------------------------------------------------------------------------------------- forward
def tile_partials(y, R):
    """(mean, M2) of R-row tiles of y viewed [M, C], computed in float64 and rounded to fp32 as the
    conv epilogue stores them: [T, C, 2] fp32."""
    y2 = y.double().reshape(-1, y.shape[-1])
    M, C = y2.shape
    T = (M + R - 1) // R
    out = torch.zeros(T, C, 2, dtype=torch.float64)
    for t in range(T):
        seg = y2[t * R:min(M, t * R + R)]
        mu = seg.mean(0)
        out[t, :, 0] = mu
        out[t, :, 1] = ((seg - mu) ** 2).sum(0)
    return out.float()


def chan_depth(T):
    """Upper bound of the Chan combines on any path from a tile partial to the result: a lane's
    serial combines (every 64th tile; the wide kernel's every 128th is fewer) plus the tree
    (6 butterfly steps; 7 LDS steps in the wide kernel; 4 shuffles + 3 waves in the fused one).
    T = 1: none (the partial is copied)."""
    if T <= 1:
        return 0
    return (T + 63) // 64 - 1 + min(7, math.ceil(math.log2(T)))


def fwd_oracle(st, R, M, gamma, beta, rm=None, rv=None, momentum=0.1, eps=1e-5, depth=None):
    """From fp32 tile partials st [T, C, 2]: float64 mean / var / invstd / scale / shift and the
    running update, each with its bound `e_<name>` (per channel)."""
    st = st.double()
    T, C = st.shape[0], st.shape[1]
    n = torch.full((T,), float(R), dtype=torch.float64)
    n[-1] = M - (T - 1) * R
    mt, m2t = st[..., 0], st[..., 1]
    mean = (n[:, None] * mt).sum(0) / M
    m2b = (n[:, None] * (mt - mean) ** 2).sum(0)
    M2 = m2t.sum(0) + m2b
    var = M2 / M
    mom, eps = f32(momentum), f32(eps)
    g, b = gamma.double(), beta.double()
    inv = 1.0 / torch.sqrt(var + eps)
    o = dict(mean=mean, var=var, M2=M2, invstd=inv, scale=g * inv, shift=b - mean * g * inv)
    # ---- bounds (docs/bn_edge_tests.md "Forward statistics")
    D = chan_depth(T) if depth is None else depth
    A = mt.abs().max(0).values
    S = mt.max(0).values - mt.min(0).values
    e_m = D * U * (A + 3 * S)
    e_d = 2 * e_m + U * S
    Wn = M * D / 2.0
    e_M2 = 2 * e_d * torch.sqrt(m2b * Wn) + e_d ** 2 * Wn + (2 * D + 4) * U * M2
    e_var = e_M2 / M + U * var
    lo, hi = (var - e_var).clamp_min(0.0) + eps, var + e_var + eps
    e_inv = torch.maximum(1 / torch.sqrt(lo) - inv, inv - 1 / torch.sqrt(hi)) + 3 * U * inv
    o.update(e_mean=e_m + U * mean.abs(), e_var=e_var, e_M2=e_M2, e_invstd=e_inv,
             e_scale=g.abs() * e_inv + U * o["scale"].abs(),
             e_shift=(g * inv).abs() * e_m + (mean * g).abs() * e_inv + 3 * U * (mean * g * inv).abs()
             + U * o["shift"].abs(), e_m=e_m)
    if rm is not None:
        unb = M2 / (M - 1) if M > 1 else var
        e_unb = e_M2 / (M - 1) + U * unb if M > 1 else e_var
        a, c = (1.0 - mom) * rm.double(), (1.0 - mom) * rv.double()
        o["running_mean"] = a + mom * mean
        o["running_var"] = c + mom * unb
        o["unbiased"] = unb
        o["e_running_mean"] = mom * e_m + 4 * U * (a.abs() + (mom * mean).abs())
        o["e_running_var"] = mom * e_unb + 4 * U * (c.abs() + (mom * unb).abs())
    return o


def eval_oracle(gamma, beta, rm, rv, eps=1e-5):
    eps = f32(eps)
    g, b, rm, rv = gamma.double(), beta.double(), rm.double(), rv.double()
    inv = 1.0 / torch.sqrt(rv + eps)
    sc, sh = g * inv, b - rm * g * inv
    return dict(scale=sc, shift=sh, e_scale=4 * U * sc.abs(), e_shift=6 * U * (rm * sc).abs() + U * sh.abs(),
                mean=rm, invstd=inv, e_invstd=3 * U * inv, e_m=torch.zeros_like(inv))


def pool_max(z):
    B, H, W, C = z.shape
    return z.view(B, H // 2, 2, W // 2, 2, C).amax((2, 4))


def apply_oracle(y, o, gamma, pool):
    """relu(y * scale + shift) (+ 2x2 max) in float64 with the oracle's coefficients, and the
    per-element bound: 2 roundings of the kernel's own fma-or-not evaluation plus the propagated
    statistics error g dinv (y - mean) - scale dm (ReLU and max are 1-Lipschitz and monotone, so a
    window's bound is the largest of its elements')."""
    yd, g = y.double(), gamma.double()
    pre = yd * o["scale"] + o["shift"]
    mean = o["mean"]
    bound = (2 * U * ((yd * o["scale"]).abs() + o["shift"].abs()) + g.abs() * (yd - mean).abs() * o["e_invstd"]
             + o["scale"].abs() * o["e_m"] + 4 * U * (mean * o["scale"]).abs())
    out = pre.clamp_min(0.0)
    if pool:
        out, bound = pool_max(out), pool_max(bound)
    return out, bound


# ---------------------------------------------------------------------------------------------- backward
def _windows(t):
    """[B, H, W, C] -> [B, Ho, Wo, C, 4] with window position p = 2 * (row in window) + (column)"""
    B, H, W, C = t.shape
    return t.view(B, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 5, 2, 4).reshape(B, H // 2, W // 2, C, 4)


def _unwindows(w):
    B, Ho, Wo, C, _ = w.shape
    return w.view(B, Ho, Wo, C, 2, 2).permute(0, 1, 4, 2, 5, 3).reshape(B, 2 * Ho, 2 * Wo, C)


def decisions(y, scale, shift, pool):
    """-> (z fp32 [B, H, W, C], sel [B, H, W, C] bool: the element the incoming gradient is routed to)"""
    z = (y.double() * scale.double() + shift.double()).float().clamp_min(0.0)
    if not pool:
        return z, z > 0
    w = _windows(z)
    am = torch.zeros(w.shape[:-1], dtype=torch.long)
    for p in range(1, 4):  # first maximum in window scan order (strict >)
        am = torch.where(w[..., p] > w.gather(-1, am[..., None])[..., 0], torch.full_like(am, p), am)
    pos = w.gather(-1, am[..., None])[..., 0] > 0
    return z, _unwindows(torch.nn.functional.one_hot(am, 4).bool() & pos[..., None])


def bwd_oracle(y, G, scale, shift, mean, invstd, gamma, pool, rows=None, sel=None):
    """BN + ReLU (+ pool) backward from supplied coefficients (they need not be consistent with y).
    -> dict of float64 results and bounds. rows: also the three sums per tile of `rows` incoming-
    gradient rows (G viewed [rows of C]), as the data-gradient epilogue produces them."""
    B, H, W, C = y.shape
    M = B * H * W
    if sel is None:
        _, sel = decisions(y, scale, shift, pool)
    yd = y.double()
    Gd = G.double()
    if pool:
        Gd = Gd.repeat_interleave(2, 1).repeat_interleave(2, 2)
    g = Gd * sel
    xh = (yd - mean.double()) * invstd.double()
    terms = torch.stack([g, g * xh, xh], 0).reshape(3, M, C)  # [3][M][C], full resolution
    sums, asum = terms.sum(1), terms.abs().sum(1)
    e_sums = (M + 4) * U * asum
    k1 = gamma.double() * invstd.double()
    k2, k3 = sums[0] / M, sums[1] / M
    e_k2, e_k3 = e_sums[0] / M + U * k2.abs(), e_sums[1] / M + U * k3.abs()
    dz = k1 * (g - k2 - xh * k3)
    o = dict(sums=sums, e_sums=e_sums, dgamma=sums[1], dbeta=sums[0], dbias=-k1 * k3 * sums[2],
             coef=torch.stack([k1, k2, k3], 1), e_coef=torch.stack([U * k1.abs(), e_k2, e_k3], 1),
             dz=dz.reshape(M, C), sel=sel)
    o["e_dbias"] = k1.abs() * (e_k3 * sums[2].abs() + k3.abs() * e_sums[2] + e_k3 * e_sums[2]) + 4 * U * o["dbias"].abs()
    o["e_dz"] = (k1.abs() * (e_k2 + xh.abs() * e_k3 + 4 * U * (g.abs() + k2.abs() + (xh * k3).abs()))
                 + U * dz.abs()).reshape(M, C)
    if rows is not None:
        # a gradient row's full-resolution elements: itself, or its 2x2 window
        if pool:
            per = _windows(terms.reshape(3 * B, H, W, C)).reshape(3, B * (H // 2) * (W // 2), C, 4)
            tsum, tabs, npp = per.sum(-1), per.abs().sum(-1), 4
        else:
            tsum, tabs, npp = terms, terms.abs(), 1
        Mg = tsum.shape[1]
        T = (Mg + rows - 1) // rows
        pad = T * rows - Mg
        z0 = torch.zeros(3, pad, C, dtype=torch.float64)
        o["tile_sums"] = torch.cat([tsum, z0], 1).view(3, T, rows, C).sum(2).permute(1, 2, 0)  # [T][C][3]
        o["e_tile_sums"] = ((rows * npp + 4) * U * torch.cat([tabs, z0], 1).view(3, T, rows, C).sum(2)).permute(1, 2, 0)
    return o


def tail_oracle(part, M, gamma, invstd):
    """Parameter gradients and coef from fp32 partials part [P, C, 3]: float64 sums of the fp32
    values; bounds (P + 1) 2^-24 sum |part|."""
    p = part.double()
    P = p.shape[0]
    s, a = p.sum(0), p.abs().sum(0)  # [C][3]
    e = (P + 1) * U * a
    k1 = gamma.double() * invstd.double()
    k2, k3 = s[:, 0] / M, s[:, 1] / M
    e_k2, e_k3 = e[:, 0] / M + U * k2.abs(), e[:, 1] / M + U * k3.abs()
    db = -k1 * k3 * s[:, 2]
    return dict(dgamma=s[:, 1], dbeta=s[:, 0], dbias=db, e_dgamma=e[:, 1], e_dbeta=e[:, 0],
                e_dbias=k1.abs() * (e_k3 * s[:, 2].abs() + k3.abs() * e[:, 2] + e_k3 * e[:, 2]) + 4 * U * db.abs(),
                coef=torch.stack([k1, k2, k3], 1), e_coef=torch.stack([U * k1.abs(), e_k2, e_k3], 1))


def dz_from_coef(y, G, sel, mean, invstd, coef, e_coef, pool):
    """dZ = k1 (g - k2 - xhat k3) in float64 from given coefficients, and its bound."""
    B, H, W, C = y.shape
    Gd = G.double()
    if pool:
        Gd = Gd.repeat_interleave(2, 1).repeat_interleave(2, 2)
    g = Gd * sel
    xh = (y.double() - mean.double()) * invstd.double()
    k1, k2, k3 = coef[:, 0], coef[:, 1], coef[:, 2]
    dz = k1 * (g - k2 - xh * k3)
    e = k1.abs() * (e_coef[:, 1] + xh.abs() * e_coef[:, 2] + 4 * U * (g.abs() + k2.abs() + (xh * k3).abs())) + U * dz.abs()
    return dz.reshape(-1, C), e.reshape(-1, C)


def worst(got, ref, bound):
    """largest |got - ref| / bound over the elements (0 / 0 counts as 0); for messages and the doc"""
    err = (got.double().cpu() - ref).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300))
    return float(r.max()) if r.numel() else 0.0


def check(got, ref, bound, name):
    """per-element |got - ref| <= bound; the message carries the worst ratio and where"""
    got = got.double().cpu().reshape(ref.shape)
    err = (got - ref).abs()
    bad = err > bound
    ratio = worst(got, ref, bound)
    print(f"[bn-edge] {name}: max abs err {float(err.max()) if err.numel() else 0.0:.3e}, worst {ratio:.3f} x bound")
    assert torch.isfinite(got).all(), f"{name}: non-finite output"
    assert not bad.any(), (f"{name}: {int(bad.sum())} of {bad.numel()} outside the bound, worst {ratio:.3g} x at "
                           f"{tuple(int(i) for i in bad.nonzero()[0])}")
    return ratio
