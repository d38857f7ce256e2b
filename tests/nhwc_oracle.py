"""Float64 oracles, input builders and derived error bounds for the channels-last ResNet kernels:
BatchNorm (+residual) (+ReLU), the 3x3/2 max-pool, im2col / col2im (csrc/kernels/cnn_nhwc.hip), the
bf16 implicit-GEMM convolution and its slab sum (csrc/kernels/conv_nhwc.hip) and the BatchNorm tile
statistics of the bf16 GEMM (gemm_bf16.hip tile_stats).

Everything runs on CPU tensors. Each oracle is the kernel's own formula in float64 on the same fp32 /
bf16 values; each bound is per element (or per channel) and is derived in docs/nhwc_edge_tests.md,
never fitted to what the kernels give. Values a launcher rounds to fp32 (momentum, eps) enter as that
fp32 value.
"""
import math

import torch
import torch.nn.functional as F

U = 2.0 ** -24   # fp32 unit roundoff
UB = 2.0 ** -8   # bf16 unit roundoff: 8 significand bits, spacing 2^-7 |x| at most, half of it
U64 = 2.0 ** -53
TINY = 1e-37     # absorbs fp32 / bf16 subnormal spacing in a store bound


def f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


def rt(t, dtype):
    """a float64 tensor rounded to dtype (round to nearest even) and back"""
    return t.to(dtype).double()


def trunc_bf16(t):
    """bf16 by truncation of the fp32 bit pattern (the named wrong variant), as float64"""
    bits = t.float().contiguous().view(torch.int32) & -65536
    return bits.view(torch.float32).double()


def store_bound(ref, e, dtype):
    """|stored - ref| for a value computed within e of ref and rounded once (to nearest) to dtype: e
    plus half the spacing of the binade the value lies in, 2^(floor(log2 v) - p) with p = 8 (bf16) or
    24 (fp32) — at most UB |v| resp. U |v|, and up to twice tighter"""
    _, ex = torch.frexp(ref.abs() + e)  # v = m 2^ex, m in [0.5, 1)
    p = 8 if dtype == torch.bfloat16 else 24
    return e + torch.ldexp(torch.ones_like(ref), ex - 1 - p) * (ref.abs() + e > 0) + TINY


# ------------------------------------------------------------------------------------- launch geometry
def vec_for(C, dtype):
    v16 = 8 if dtype == torch.bfloat16 else 4
    if C % v16 == 0:
        return v16
    return 4 if C % 4 == 0 else 1


def bn_grid(M, C, dtype):
    """cnn_nhwc.hip bn_grid + row_split -> dict(V, P, CG, rpb, groups=[(c_lo, c_hi, nv, lanes)])"""
    V = vec_for(C, dtype)
    CV = C // V
    CG = (CV + 255) // 256
    lanes0 = 256 // min(CV, 256)
    want = (1024 + CG - 1) // CG
    rpb = max((M + want - 1) // want, 16 * lanes0)
    groups = []
    for g in range(CG):
        nv = min(256, CV - g * 256)
        groups.append((g * 256 * V, (g * 256 + nv) * V, nv, 256 // nv))
    return dict(V=V, P=(M + rpb - 1) // rpb, CG=CG, rpb=rpb, groups=groups)


def sum_depth(M, C, dtype):
    """per channel: the additions on the longest path of a fixed-order partial sum (rows of one row
    lane, then the row lanes of the block that hold a row: adding a lane's exact 0 rounds nothing), as a
    [C] float64 tensor"""
    g = bn_grid(M, C, dtype)
    d = torch.zeros(C, dtype=torch.float64)
    rows = min(g["rpb"], M)
    for lo, hi, nv, lanes in g["groups"]:
        d[lo:hi] = (rows + lanes - 1) // lanes + min(lanes, rows)
    return d


# --------------------------------------------------------------------------------------------- builders
def ordinary(shape, dtype, seed=0):
    """x ~ N(0.7, 2^2) per element, gamma in +-[0.5, 1.5], beta ~ N(0, 1): (x in dtype, gamma, beta)"""
    g = torch.Generator().manual_seed(100 + seed)
    C = shape[-1]
    x = (torch.randn(shape, generator=g, dtype=torch.float64) * 2 + 0.7).to(dtype)
    gamma = (torch.rand(C, generator=g) + 0.5) * torch.where(torch.rand(C, generator=g) < 0.25, -1.0, 1.0)
    return x, gamma.float(), torch.randn(C, generator=g).float()


LADDER_MEANS = [0, 1, -1, 30, -30, 1000, -1000, 0, 1, -30, 1000, -1000, 30, -1, 1000, 30.0]
LADDER_STDS = [1, 1e-3, 10, 1e-2, 1, 1e-3, 10, 1e-3, 1e-1, 10, 1, 1e-2, 1e-3, 1e-2, 1e-1, 0.0]
LADDER_GAMMA = [1, -1, 0, 1e-3, 1e3, 0.5, -2, 1e3, -1e-3, 1, 0, 1e-3, -1e3, 2, 1, 1]
LADDER_BETA = [0, 0.5, -0.5, 1, -1, 0.25, 0, 2, -2, 0.1, 1, 0, 0.5, -0.1, 0, 3]


def ladder(shape, dtype, seed=0):
    """16 channels: means 0 to +-1000, spreads 1e-3 to 10, channel 15 constant; gamma negative, 0,
    1e-3, 1e3"""
    assert shape[-1] == 16
    g = torch.Generator().manual_seed(200 + seed)
    x = torch.randn(shape, generator=g, dtype=torch.float64) * torch.tensor(LADDER_STDS, dtype=torch.float64) \
        + torch.tensor(LADDER_MEANS, dtype=torch.float64)
    return x.to(dtype), torch.tensor(LADDER_GAMMA, dtype=torch.float32), torch.tensor(LADDER_BETA, dtype=torch.float32)


def outlier(sigmas, dtype, seed=0):
    """M = 2048 rows of N(0.7, 2^2), row 0 set `sigmas` standard deviations from the channel mean"""
    x, gamma, beta = ordinary((2, 32, 32, 16), dtype, seed=7 + seed)
    x = x.clone()
    x[0, 0, 0, :] = 0.7 + 2.0 * sigmas
    return x, gamma, beta


def grad_for(shape, dtype, seed=0):
    g = torch.Generator().manual_seed(300 + seed)
    return torch.randn(shape, generator=g).to(dtype)


# (name, builder, shape, dtypes): every BatchNorm input of tests/test_nhwc_edges_gpu.py through the
# statistics pass (the CPU file evaluates each in fp32 / bf16 against the bounds)
F32, BF16 = torch.float32, torch.bfloat16
BN_CASES = [("m2", ordinary, (2, 1, 1, 8), (F32, BF16)), ("m17", ordinary, (17, 1, 1, 8), (F32, BF16))]
BN_CASES += [(f"c{C}", ordinary, (3, 5, 3, C), (F32, BF16)) for C in (5, 6, 7, 12, 20)]
BN_CASES += [("c24", ordinary, (3, 5, 3, 24), (BF16,)), ("c1028", ordinary, (2, 5, 5, 1028), (F32,)),
             ("c2056", ordinary, (2, 5, 5, 2056), (BF16,)), ("c258", ordinary, (2, 5, 5, 258), (F32, BF16)),
             ("p40", ordinary, (10, 8, 8, 1024), (F32,)), ("ladder", ladder, (4, 16, 16, 16), (F32, BF16))]
BN_CASES += [(f"out{s}", lambda shape, dt, seed=0, s=s: outlier(s, dt), (2, 32, 32, 16), (F32, BF16)) for s in (15, 150)]
PAIRS = [(0.3, 1e-3), (1.0, 1e-5), (0.0, 1e-2)]


def case_relu(name):
    """the ladder and the first-row outliers run without ReLU: their bounds are wide by construction
    (|mean| / sigma up to 1e6, |x0 - mean| up to 150 sigma), so a ReLU would leave more than 0.1 % of
    the elements undecided; every other case runs with it"""
    return not (name == "ladder" or name.startswith("out"))


def pool_shapes():
    """small-integer / 8 values (exact in bf16, many natural ties): H, W in {1, 2, 3, 7, 8}, C = 5, 12, 16"""
    g = torch.Generator().manual_seed(500)
    out = []
    for i, (H, W) in enumerate([(1, 1), (1, 2), (2, 1), (2, 2), (3, 3), (1, 7), (7, 2), (3, 8), (7, 7), (8, 8), (7, 8)]):
        C = (5, 12, 16)[i % 3]
        out.append((f"{H}x{W}x{C}", torch.randint(-3, 4, (2, H, W, C), generator=g).double() / 8))
    return out


PAIRS9 = [(p, q) for p in range(9) for q in range(p + 1, 9)]


def _centre(x, b, p, v):
    x[b, 1 + p // 3, 1 + p % 3, :] = v  # position p of the centre window (oh = ow = 1) of a 5x5 image


def pool_ties():
    """-> list of (name, x float64 [B, 5, 5, 8]): all-equal and all-zero windows, equal maxima at each
    pair of positions of the centre window, -inf inputs, one NaN, two NaNs"""
    g = torch.Generator().manual_seed(501)
    base = -1.0 - torch.randint(0, 8, (len(PAIRS9), 5, 5, 8), generator=g).double() / 8
    pairs, nan1, nan2 = base.clone(), base[:9].clone(), base.clone()
    for b, (p, q) in enumerate(PAIRS9):
        _centre(pairs, b, p, 3.0)
        _centre(pairs, b, q, 3.0)
        _centre(nan2, b, p, math.nan)
        _centre(nan2, b, q, math.nan)
    for p in range(9):
        _centre(nan1, p, p, math.nan)
        _centre(nan1, p, (p + 4) % 9, 5.0)  # a larger finite value elsewhere in the window: the NaN still wins
    ninf = base[:3].clone()
    ninf[0] = -math.inf
    ninf[1, :, :, ::2] = -math.inf
    ninf[2, 1:4, 1:4, :] = -math.inf
    return [("equal", torch.full((2, 5, 5, 8), 1.5, dtype=torch.float64)), ("zero", torch.zeros(2, 5, 5, 8, dtype=torch.float64)),
            ("negzero", -torch.zeros(1, 5, 5, 8, dtype=torch.float64)), ("pairs", pairs), ("ninf", ninf), ("nan1", nan1),
            ("nan2", nan2)]


def pool_shared():
    """an input shared by four windows (1, 1) and by two ((1, 2) and (2, 1)) that all select it"""
    x = -torch.ones(3, 5, 5, 8, dtype=torch.float64)
    x[0, 1, 1], x[1, 1, 2], x[2, 2, 1] = 4.0, 4.0, 4.0
    return x


# (B, H, W, C, R, S, stride, pad): direct im2col / col2im geometries
IM2COL_CASES = [(2, 5, 6, 3, 3, 3, 1, 1), (2, 5, 6, 5, 1, 3, 2, 1), (2, 6, 5, 4, 3, 1, 2, 0), (1, 9, 9, 12, 7, 7, 2, 3),
                (2, 7, 5, 8, 1, 1, 2, 0), (1, 7, 7, 32, 3, 3, 3, 2), (2, 2, 2, 4, 3, 3, 1, 1), (1, 1, 4, 8, 3, 3, 1, 1),
                (1, 5, 5, 3, 3, 3, 2, 3), (2, 7, 9, 12, 3, 3, 2, 1), (1, 6, 6, 5, 3, 3, 1, 0), (1, 8, 8, 4, 3, 3, 1, 2)]

# (B, H, W, C, Co, R, S, stride, pad): the bf16 implicit-GEMM convolution's geometries
CONV_CASES = [(2, 6, 5, 32, 32, 1, 3, 1, 1), (2, 5, 6, 32, 64, 3, 1, 1, 1), (2, 6, 6, 32, 32, 3, 3, 1, 0),
              (1, 5, 5, 32, 96, 3, 3, 1, 2), (2, 7, 9, 64, 128, 3, 3, 2, 1), (1, 8, 8, 32, 160, 3, 3, 3, 1),
              (3, 2, 2, 32, 32, 3, 3, 1, 1), (5, 1, 1, 32, 64, 3, 3, 1, 1), (1, 9, 7, 32, 32, 5, 5, 2, 2),
              (1, 127, 1, 32, 32, 3, 3, 1, 1), (1, 128, 1, 32, 64, 3, 3, 1, 1), (1, 129, 1, 32, 96, 3, 3, 1, 1)]
# (shape, slabs allocated, slabs launched): split-K weight gradients
SPLIT_CASES = [((2, 16, 16, 32, 32, 3, 3, 1, 1), 2, 2), ((1, 23, 23, 32, 64, 3, 3, 1, 1), 2, 2),
               ((1, 41, 100, 32, 64, 1, 1, 1, 0), 16, 15)]
# (H, W, Co, R, stride, pad): the 4-channel stem
STEM_CASES = [(6, 8, 32, 3, 1, 1), (5, 9, 64, 3, 2, 1), (5, 17, 32, 3, 1, 1), (9, 17, 64, 7, 2, 3), (8, 8, 128, 7, 2, 3), (7, 9, 32, 7, 1, 3)]


def impulse_points(H, W):
    """(b, h, w) of the impulses in a 2-image batch: the corners, an edge mid-point, the last pixel of
    image 0 and the first of image 1; duplicates (tiny images) removed, order kept"""
    pts = [(0, 0, 0), (0, 0, W - 1), (0, H - 1, 0), (0, 0, W // 2), (0, H - 1, W - 1), (1, 0, 0)]
    return list(dict.fromkeys(pts))


def impulse_case(H, W, C, Co, R, S, pts=None):
    """x: a single 1 per impulse point, each in its own channel; w: distinct small integers per (r, s)
    that also differ between three output channels. Every product and sum is an integer below 256:
    exact in bf16. -> (x, w) bf16"""
    pts = impulse_points(H, W) if pts is None else pts
    x = torch.zeros(2, H, W, C)
    for i, (b, h, w_) in enumerate(pts):
        x[b, h, w_, i % C] = 1.0
    taps = (torch.arange(R * S).view(R, S) + 1).float()
    w = taps[None, :, :, None] + (torch.arange(Co) % 3).float()[:, None, None, None] + torch.zeros(Co, R, S, C)
    assert float(w.max()) * len(pts) <= 256
    return x.bfloat16(), w.bfloat16()


# ------------------------------------------------------------------------------------------ BatchNorm
def bn_stats(x, gamma=None, beta=None, rm=None, rv=None, momentum=0.1, eps=1e-5):
    """stats_kernel + finalize_fwd_kernel in float64: shifted sums of d = x - x[row 0], mean = K + S1/M,
    var = S2/M - (S1/M)^2, and the bounds of the fp32 partial sums (fixed order: sum_depth)."""
    C = x.shape[-1]
    x2 = x.double().reshape(-1, C)
    M = x2.shape[0]
    mom, eps = f32(momentum), f32(eps)
    g = torch.ones(C, dtype=torch.float64) if gamma is None else gamma.double()
    b = torch.zeros(C, dtype=torch.float64) if beta is None else beta.double()
    d = x2 - x2[0]
    n = sum_depth(M, C, x.dtype)
    S1, S2 = d.sum(0), (d * d).sum(0)
    e_S1 = (n + 1) * U * d.abs().sum(0)          # c = 1: the rounding of d itself
    e_S2 = (n + 3) * U * S2                      # c = 3: d twice in d*d, the fma
    dm = S1 / M
    var = (S2 / M - dm * dm).clamp_min(0.0)
    mean = x2[0] + dm
    e_dm = e_S1 / M
    e_var = e_S2 / M + 2 * dm.abs() * e_dm + e_dm ** 2 + 8 * U64 * (S2 / M + dm * dm)
    inv = 1.0 / torch.sqrt(var + eps)
    lo, hi = (var - e_var).clamp_min(0.0) + eps, var + e_var + eps
    e_inv = torch.maximum(1 / torch.sqrt(lo) - inv, inv - 1 / torch.sqrt(hi)) + 2 * U * inv
    return _finish(dict(M=M, mean=mean, var=var, invstd=inv, e_m=e_dm, e_var=e_var, e_invstd=e_inv), g, b, rm, rv, mom)


def _finish(o, g, b, rm, rv, mom):
    """scale / shift / running statistics from mean, var, invstd and their bounds (both finalizes)"""
    M, mean, var, inv, e_inv = o["M"], o["mean"], o["var"], o["invstd"], o["e_invstd"]
    e_mean = o["e_m"] + U * mean.abs()           # the (float) cast
    scale = g * inv
    shift = b - mean * scale
    o.update(gamma=g, scale=scale, shift=shift, e_mean=e_mean, e_scale=g.abs() * e_inv + U * scale.abs(),
             e_shift=scale.abs() * e_mean + (mean * g).abs() * e_inv + 3 * U * (mean * scale).abs() + U * shift.abs())
    if rm is not None:
        unb = var * M / (M - 1) if M > 1 else var
        e_unb = (o["e_var"] * M / (M - 1) if M > 1 else o["e_var"]) + U * unb
        a, c = (1.0 - mom) * rm.double(), (1.0 - mom) * rv.double()
        o.update(unbiased=unb, running_mean=a + mom * mean, running_var=c + mom * unb,
                 e_running_mean=mom * e_mean + 4 * U * (a.abs() + (mom * mean).abs()),
                 e_running_var=mom * e_unb + 4 * U * (c.abs() + (mom * unb).abs()))
    return o


def tile_partials(x, R):
    """fp32 (mean, M2) of the R-row tiles of x viewed [M, C], computed in float64: [T, C, 2]"""
    x2 = x.double().reshape(-1, x.shape[-1])
    M, C = x2.shape
    T = (M + R - 1) // R
    out = torch.zeros(T, C, 2, dtype=torch.float64)
    for t in range(T):
        seg = x2[t * R:min(M, t * R + R)]
        out[t, :, 0] = seg.mean(0)
        out[t, :, 1] = ((seg - seg.mean(0)) ** 2).sum(0)
    return out.float()


def bn_tiles(tiles, R, M, gamma=None, beta=None, rm=None, rv=None, momentum=0.1, eps=1e-5):
    """finalize_tiles_kernel: the exact Chan combination of the fp32 tile partials. The kernel combines
    in float64 (D = ceil(T / 32) + 5 combines on a path), so only float64 roundoff and the fp32 casts
    of the results remain."""
    t = tiles.double()
    T, C = t.shape[0], t.shape[1]
    n = torch.full((T, 1), float(R), dtype=torch.float64)
    n[-1] = M - (T - 1) * R
    mt = t[..., 0]
    mean = (n * mt).sum(0) / M
    m2b = (n * (mt - mean) ** 2).sum(0)
    M2 = t[..., 1].sum(0) + m2b
    var = M2 / M
    mom, eps = f32(momentum), f32(eps)
    g = torch.ones(C, dtype=torch.float64) if gamma is None else gamma.double()
    b = torch.zeros(C, dtype=torch.float64) if beta is None else beta.double()
    D = (T + 31) // 32 + 5
    A = mt.abs().max(0).values
    e_m = 4 * D * U64 * A
    e_var = 8 * D * U64 * (var + A * A)
    inv = 1.0 / torch.sqrt(var + eps)
    lo, hi = (var - e_var).clamp_min(0.0) + eps, var + e_var + eps
    e_inv = torch.maximum(1 / torch.sqrt(lo) - inv, inv - 1 / torch.sqrt(hi)) + 2 * U * inv
    return _finish(dict(M=M, mean=mean, var=var, invstd=inv, e_m=e_m, e_var=e_var, e_invstd=e_inv), g, b, rm, rv, mom)


def tile_rounding(tiles, R, M):
    """how far the statistics of fp32-rounded tile partials can sit from those of x itself:
    (e_mean, e_var) per channel"""
    t = tiles.double()
    T = t.shape[0]
    n = torch.full((T, 1), float(R), dtype=torch.float64)
    n[-1] = M - (T - 1) * R
    mt = t[..., 0]
    mean = (n * mt).sum(0) / M
    e_mean = U * (n * mt.abs()).sum(0) / M
    e_var = (U * t[..., 1].sum(0) + (2 * n * (mt - mean).abs() * (U * mt.abs() + e_mean)).sum(0)) / M
    return e_mean, e_var * 1.01 + 4 * e_mean ** 2


def bn_apply(x, o, res=None, relu=True):
    """y = relu(x scale + shift + res) in float64 with the oracle's coefficients.
    -> (y, bound before the store, undecided mask, z). The kernel evaluates fl(fl(x sc + sf) + res)
    with sc = fl(gamma invstd), sf = fl(beta - fl(mean) sc)."""
    xd = x.double()
    z = xd * o["scale"] + o["shift"]
    zr = z + (res.double() if res is not None else 0.0)
    e = (o["gamma"].abs() * (xd - o["mean"]).abs() * o["e_invstd"] + o["scale"].abs() * o["e_mean"]
         + 2 * U * (((xd - o["mean"]) * o["scale"]).abs() + (o["mean"] * o["scale"]).abs() + 2 * o["shift"].abs()
                    + (xd * o["scale"]).abs() + zr.abs()))
    und = (zr.abs() <= e) & (e > 0) & bool(relu)  # e == 0: the kernel's z is the oracle's, bit for bit
    return (zr.clamp_min(0.0) if relu else zr), e, und, zr


def bn_backward(x, dy, o, z=None, und=None, relu=True):
    """g = dy [z > 0]; dbeta = sum g, dgamma = sum g xhat; dx = k (g - mean g - xhat mean(g xhat)).
    Undecided elements (|z| within its bound of 0) add |g| / |g xhat| to the channel's bounds."""
    C = x.shape[-1]
    xd, g = x.double().reshape(-1, C), dy.double().reshape(-1, C)
    M = xd.shape[0]
    if relu:
        z2, u2 = z.reshape(-1, C), und.reshape(-1, C)
        extra_g = (g.abs() * u2).sum(0)
        g = g * ((z2 > 0) & ~u2)
    else:
        u2 = torch.zeros_like(g, dtype=torch.bool)
        extra_g = torch.zeros(C, dtype=torch.float64)
    mean, inv = o["mean"], o["invstd"]
    xh = (xd - mean) * inv
    e_xh = inv * (o["e_mean"] + U * (xd - mean).abs()) + (xd - mean).abs() * o["e_invstd"] + U * xh.abs()
    extra_gx = (dy.double().reshape(-1, C).abs() * (xh.abs() + e_xh) * u2).sum(0)
    n = sum_depth(M, C, x.dtype)
    db, dg = g.sum(0), (g * xh).sum(0)
    e_db = n * U * g.abs().sum(0) + extra_g
    e_dg = (n + 1) * U * (g * xh).abs().sum(0) + (g.abs() * e_xh).sum(0) + extra_gx
    k = o["gamma"] * inv
    e_k = o["gamma"].abs() * o["e_invstd"] + U * k.abs()
    mg, mgx = db / M, dg / M
    e_mg, e_mgx = e_db / M + 2 * U * mg.abs(), e_dg / M + 2 * U * mgx.abs()
    inner = g - mg - xh * mgx
    dx = k * inner
    e_dx = (e_k * inner.abs() + (k.abs() + e_k) * (e_mg + xh.abs() * e_mgx + (mgx.abs() + e_mgx) * e_xh
                                                  + 3 * U * (g.abs() + mg.abs() + (xh * mgx).abs())) + U * dx.abs())
    return dict(g=g.reshape(x.shape), dx=dx.reshape(x.shape), e_dx=e_dx.reshape(x.shape), dbeta=db, dgamma=dg,
                e_dbeta=e_db + U * db.abs(), e_dgamma=e_dg + U * dg.abs())


# ------------------------------------------------------------------------------------------- max-pool
def _window(x, dh, dw, Ho, Wo):
    """(values [B, Ho, Wo, C], valid [Ho, Wo]) of window position (dh, dw) of the 3x3/2 pad-1 pool"""
    B, H, W, C = x.shape
    ih = 2 * torch.arange(Ho) - 1 + dh
    iw = 2 * torch.arange(Wo) - 1 + dw
    ok = ((ih >= 0) & (ih < H))[:, None] & ((iw >= 0) & (iw < W))[None, :]
    v = x[:, ih.clamp(0, H - 1)][:, :, iw.clamp(0, W - 1)]
    return v, ok


def pool_fwd(x, last=False):
    """first maximum in row-major window order, a NaN replaces whatever is held (ATen's rule).
    last=True: the wrong variant that keeps the last of equal maxima. -> (y, pos int64)"""
    B, H, W, C = x.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    best = torch.full((B, Ho, Wo, C), -math.inf, dtype=x.dtype)
    pos = torch.full((B, Ho, Wo, C), -1, dtype=torch.int64)
    for dh in range(3):
        for dw in range(3):
            v, ok = _window(x, dh, dw, Ho, Wo)
            take = ((pos < 0) | ((v >= best) if last else (v > best)) | (v != v)) & ok[None, :, :, None]
            best = torch.where(take, v, best)
            pos = torch.where(take, torch.full_like(pos, dh * 3 + dw), pos)
    return best, pos


def pool_index(pos, H, W):
    """window position -> ATen's flat input index ih * W + iw"""
    B, Ho, Wo, C = pos.shape
    ih = 2 * torch.arange(Ho)[None, :, None, None] - 1 + pos // 3
    iw = 2 * torch.arange(Wo)[None, None, :, None] - 1 + pos % 3
    return ih * W + iw


def pool_bwd(dy, pos, H, W):
    """dx[q] = sum of the dy of the windows that picked q (float64), and sum |dy| of those windows"""
    B, Ho, Wo, C = dy.shape
    idx = pool_index(pos, H, W).reshape(B, -1, C)
    d = dy.double().reshape(B, -1, C)
    dx = torch.zeros(B, H * W, C, dtype=torch.float64).scatter_add_(1, idx, d)
    ab = torch.zeros(B, H * W, C, dtype=torch.float64).scatter_add_(1, idx, d.abs())
    return dx.reshape(B, H, W, C), ab.reshape(B, H, W, C)


def pool_max_bound(e):
    """a window's bound: the largest of its elements' (max is monotone and 1-Lipschitz)"""
    return F.max_pool2d(e.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1)


# ------------------------------------------------------------------------------------ im2col / col2im
def im2col_ref(x, R, S, st, pad, Kp):
    """F.unfold's columns rearranged from (c, r, s) to (r, s, c), zero columns K .. Kp - 1; exact in
    any dtype (a gather)"""
    B, H, W, C = x.shape
    u = F.unfold(x.double().permute(0, 3, 1, 2), (R, S), padding=pad, stride=st)  # [B, C*R*S, L]
    L = u.shape[2]
    col = u.view(B, C, R, S, L).permute(0, 4, 2, 3, 1).reshape(B * L, R * S * C)
    return F.pad(col, (0, Kp - R * S * C))


def col2im_ref(dcol, B, H, W, C, R, S, st, pad):
    """the float64 adjoint (F.fold), and the same of |dcol| and the number of taps per element"""
    K = R * S * C
    d = dcol.double()[:, :K]
    L = d.shape[0] // B

    def fold(t):
        u = t.view(B, L, R, S, C).permute(0, 4, 2, 3, 1).reshape(B, C * R * S, L)
        return F.fold(u, (H, W), (R, S), padding=pad, stride=st).permute(0, 2, 3, 1)
    return fold(d), fold(d.abs()), fold(torch.ones_like(d))


# ------------------------------------------------------------------------------------------- bf16 conv
def conv_geo(H, W, R, S, st, pad):
    return (H + 2 * pad - R) // st + 1, (W + 2 * pad - S) // st + 1


def conv_splits(B, H, W, C, Co, R, S, st, pad):
    """cs_conv_nhwc_splits for the weight gradient, and the launcher's clamp -> (workspace, launched)"""
    Ho, Wo = conv_geo(H, W, R, S, st, pad)
    ksteps = (B * Ho * Wo + 31) // 32
    kc = R * 32 if C == 4 else R * S * C
    tiles = ((Co + 127) // 128) * ((kc + 127) // 128)
    s = 1
    while tiles * s * 2 <= 1024 and ksteps // (2 * s) >= 8 and 2 * s * Co * kc * 4 <= 1 << 30:
        s *= 2
    per = (ksteps + min(s, ksteps) - 1) // min(s, ksteps)
    return s, (ksteps + per - 1) // per


def conv_inputs(B, H, W, C, Co, R, S, st, pad, seed=0):
    """bf16 x [B,H,W,C], w [Co,R,S,C], dy [B,Ho,Wo,Co]"""
    g = torch.Generator().manual_seed(400 + seed)
    Ho, Wo = conv_geo(H, W, R, S, st, pad)
    x = (torch.randn(B, H, W, C, generator=g) + 0.25).bfloat16()
    w = (torch.randn(Co, R, S, C, generator=g) / (R * S * C) ** 0.5).bfloat16()
    dy = torch.randn(B, Ho, Wo, Co, generator=g).bfloat16()
    return x, w, dy


def conv_ref(x, w, dy, st, pad, splits=1):
    """float64 y / dx / dW (NHWC, dW [Co, R, S, C]) on the bf16 values, with per-element bounds:
    exact bf16 products, fp32 accumulation over n terms in any order (n u sum |a b|), then the bf16 store
    (y, dx) or the fp32 slab sum (dW)."""
    xd, wd, gd = (t.double() for t in (x, w, dy))
    Co, R, S, C = w.shape
    xn, wn, gn = xd.permute(0, 3, 1, 2), wd.permute(0, 3, 1, 2), gd.permute(0, 3, 1, 2)
    y = F.conv2d(xn, wn, None, st, pad)
    ya = F.conv2d(xn.abs(), wn.abs(), None, st, pad)
    assert y.shape[2:] == gn.shape[2:]
    dx = torch.nn.grad.conv2d_input(xn.shape, wn, gn, st, pad)
    dxa = torch.nn.grad.conv2d_input(xn.shape, wn.abs(), gn.abs(), st, pad)
    dw = torch.nn.grad.conv2d_weight(xn, wn.shape, gn, st, pad)
    dwa = torch.nn.grad.conv2d_weight(xn.abs(), wn.shape, gn.abs(), st, pad)
    pix = gn.shape[0] * gn.shape[2] * gn.shape[3]
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous()
    return dict(y=nhwc(y), e_y=store_bound(nhwc(y), R * S * C * U * nhwc(ya), torch.bfloat16),
                dx=nhwc(dx), e_dx=store_bound(nhwc(dx), R * S * Co * U * nhwc(dxa), torch.bfloat16),
                dw=nhwc(dw), e_dw=(pix + splits + 1) * U * nhwc(dwa) + TINY)


def slab_lanes(S):
    SL = 1
    while SL < 16 and SL * 32 < S:
        SL *= 2
    return SL


def slab_ref(part):
    """sum over dim 0 and its bound: lane l adds ceil(S / SL) slabs, then SL lane sums"""
    S = part.shape[0]
    SL = slab_lanes(S)
    p = part.double()
    return p.sum(0), ((S + SL - 1) // SL + SL) * U * p.abs().sum(0) + TINY


def gemm_tile_stats(y, rows=256):
    """gemm_bf16.hip tile_stats on the bf16 y [M, N] it returned: two passes in fp32 over 8 serial adds,
    4 shuffles and one LDS add (13 additions). -> (mean, e_mean, M2, e_M2) each [T, N]"""
    yd = y.double()
    M = yd.shape[0]
    out = []
    for t in range((M + rows - 1) // rows):
        seg = yd[t * rows:(t + 1) * rows]
        n = seg.shape[0]
        mean = seg.mean(0)
        e_mean = (13 * U * seg.abs().sum(0)) / n + U * mean.abs()
        d = seg - mean
        e_d = e_mean + U * (d.abs() + e_mean)
        M2 = (d * d).sum(0)
        e_M2 = (2 * d.abs() * e_d + e_d ** 2).sum(0) + n * e_mean ** 2 + 16 * U * M2
        out.append((mean, e_mean, M2, e_M2))
    return tuple(torch.stack(c) for c in zip(*out))


# ------------------------------------------------------------------------------------------- checking
def worst(got, ref, bound):
    err = (got.detach().double().cpu().reshape(ref.shape) - ref).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300))
    return float(r.max()) if r.numel() else 0.0


def check(got, ref, bound, name, skip=None):
    """per-element |got - ref| <= bound (elements under `skip` left out); prints the worst ratio"""
    got = got.detach().double().cpu().reshape(ref.shape)
    bound = bound.expand_as(ref) if bound.shape != ref.shape else bound
    if skip is not None:
        keep = ~skip.reshape(ref.shape)
        assert float(skip.sum()) <= 1e-3 * skip.numel(), f"{name}: {int(skip.sum())} of {skip.numel()} undecided"
        got, ref, bound = got[keep], ref[keep], bound[keep]
    err = (got - ref).abs()
    bad = ~(err <= bound)
    ratio = worst(got, ref, bound)
    print(f"[nhwc-edge] {name}: max abs err {float(err.max()) if err.numel() else 0.0:.3e}, worst {ratio:.3f} x bound")
    assert not bad.any(), (f"{name}: {int(bad.sum())} of {bad.numel()} outside the bound, worst {ratio:.3g} x at "
                           f"{tuple(int(i) for i in bad.nonzero()[0])}")
    return ratio


def inside(got, ref, bound, skip=None):
    """bool: the same test without asserting (the wrong-variant checks)"""
    got = got.double().reshape(ref.shape)
    err = (got - ref).abs()
    ok = err <= (bound.expand_as(ref) if bound.shape != ref.shape else bound)
    if skip is not None:
        ok = ok | skip.reshape(ref.shape)
    return bool(ok.all())
