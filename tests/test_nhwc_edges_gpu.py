"""Edge tests of the channels-last ResNet kernels, MI355X only: BatchNorm (+residual) (+ReLU), the
3x3/2 max-pool and its fusions, im2col / col2im (csrc/kernels/cnn_nhwc.hip), the bf16 implicit-GEMM
convolution with its split-K weight gradient and slab sum (csrc/kernels/conv_nhwc.hip) and the
BatchNorm tile statistics of the bf16 GEMM (gemm_bf16.hip).

Oracle: tests/nhwc_oracle.py, plain float64 on the same fp32 / bf16 values with per-element bounds
derived from the roundings (checked on the CPU by tests/test_nhwc_oracles_cpu.py). Which branch each
case enters, the derivations and the errors measured are in docs/nhwc_edge_tests.md."""
import pytest
import torch
import torch.nn as nn

import nhwc_oracle as O

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
DT = [F32, BF16]
DT_IDS = ["f32", "bf16"]
BN_PARAMS = [(n, b, s, dt) for n, b, s, dts in O.BN_CASES for dt in dts]
BN_IDS = [f"{n}-{'bf16' if dt == BF16 else 'f32'}" for n, _, _, dts in O.BN_CASES for dt in dts]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cs744_pytorch_distributed_tutorial_amd.ops import native
    native.C()
    return torch.device("cuda", 0)


def _C():
    from cs744_pytorch_distributed_tutorial_amd.ops import native
    return native.C()


def _eq(a, b):
    """bitwise-style equality that lets a NaN equal a NaN"""
    a, b = a.double().cpu(), b.double().cpu()
    return a.shape == b.shape and bool(((a == b) | ((a != a) & (b != b))).all())


# ====================================================================================== BatchNorm
def _bn_run(dev, name, x, gamma, beta, res=None, relu=True, momentum=0.1, eps=1e-5, running=True, nbt0=41,
            with_mask=False, tiles=None, tile_rows=256, o=None, backward=True):
    """bn_nhwc_fwd (+ bn_nhwc_bwd) through the raw binding against the oracle; gamma / beta None: no affine"""
    C_ = _C()
    C = x.shape[-1]
    rm0, rv0 = torch.linspace(-1, 1, C), torch.linspace(0.5, 2, C)
    if o is None:
        o = O.bn_stats(x, gamma, beta, rm0, rv0, momentum, eps)
    rm, rv = (rm0.to(dev), rv0.to(dev)) if running else (None, None)
    nbt = None if nbt0 is None else torch.full((), nbt0, dtype=torch.int64, device=dev)
    w = None if gamma is None else gamma.to(dev)
    b = None if beta is None else beta.to(dev)
    xg = x.to(dev)
    rg = None if res is None else res.to(dev)
    y, stat, mask = C_.bn_nhwc_fwd(xg, rg, w, b, rm, rv, nbt, momentum, eps, relu, with_mask, tiles, tile_rows)
    torch.cuda.synchronize()
    for i, k in enumerate(("scale", "shift", "mean", "invstd")):
        O.check(stat[i], o[k], o["e_" + k], f"{name} {k}")
    ref, e, und, z = O.bn_apply(x, o, res, relu)
    O.check(y, ref, O.store_bound(ref, e, x.dtype), f"{name} y", und)
    if running:
        O.check(rm, o["running_mean"], o["e_running_mean"], f"{name} running_mean")
        O.check(rv, o["running_var"], o["e_running_var"], f"{name} running_var")
    if nbt is not None:
        assert int(nbt) == nbt0 + 1
    if not backward:
        return o, stat
    dy = O.grad_for(x.shape, x.dtype, seed=1)
    bo = O.bn_backward(x, dy, o, z, und, relu)
    dx, dres, dw, db = C_.bn_nhwc_bwd(dy.to(dev), xg, None if with_mask else rg, w, stat, relu, res is not None,
                                      mask if with_mask else None)
    torch.cuda.synchronize()
    tag = f"{name} {'mask' if with_mask else 'recompute'}"
    O.check(dx, bo["dx"], O.store_bound(bo["dx"], bo["e_dx"], x.dtype), f"{tag} dx", und)
    O.check(dw, bo["dgamma"], bo["e_dgamma"], f"{tag} dgamma")
    O.check(db, bo["dbeta"], bo["e_dbeta"], f"{tag} dbeta")
    assert bool(torch.isfinite(dx).all())
    if res is not None:  # dres = g: the incoming gradient under the ReLU mask, no arithmetic
        keep = ~und
        assert torch.equal(dres.double().cpu()[keep], bo["g"][keep]), f"{tag} dres"
        if not relu:
            assert torch.equal(dres.cpu(), dy)
    return o, stat


@pytest.mark.parametrize("res", [False, True], ids=["plain", "res"])
@pytest.mark.parametrize("name,builder,shape,dt", BN_PARAMS, ids=BN_IDS)
def test_bn_cases(dev, name, builder, shape, dt, res):
    x, gamma, beta = builder(shape, dt)
    r = O.grad_for(shape, dt, seed=9) if res else None
    relu = O.case_relu(name)
    g = O.bn_grid(x.numel() // shape[-1], shape[-1], dt)
    if name == "p40":
        assert g["P"] == 40
    if name in ("c1028", "c2056", "c258"):
        assert g["CG"] == 2 and g["groups"][1][2] == (2 if name == "c258" else 1)
    _bn_run(dev, name, x, gamma, beta, r, relu)
    if res and relu:
        _bn_run(dev, name, x, gamma, beta, r, relu, with_mask=True)


@pytest.mark.parametrize("dt", DT, ids=DT_IDS)
@pytest.mark.parametrize("momentum,eps", O.PAIRS)
def test_bn_momentum_and_eps(dev, momentum, eps, dt):
    x, gamma, beta = O.ordinary((3, 5, 3, 12), dt)
    _bn_run(dev, f"pair {momentum} {eps}", x, gamma, beta, None, True, momentum, eps)


@pytest.mark.parametrize("dt", DT, ids=DT_IDS)
def test_bn_optional_arguments(dev, dt):
    x, gamma, beta = O.ordinary((3, 5, 3, 12), dt)
    _bn_run(dev, "no affine", x, None, None, None, True, 0.3, 1e-3)
    _bn_run(dev, "no running", x, gamma, beta, None, True, 0.3, 1e-3, running=False)
    _bn_run(dev, "no nbt", x, gamma, beta, None, True, 0.3, 1e-3, nbt0=None)
    _bn_run(dev, "neither", x, None, None, O.grad_for(x.shape, dt, seed=9), True, 0.3, 1e-3, running=False, nbt0=None)


@pytest.mark.parametrize("dt", DT, ids=DT_IDS)
def test_bn_relu_exactly_zero_without_residual(dev, dt):
    """gamma = beta = 0: every pre-activation is exactly 0, not > 0 — output 0, no gradient anywhere"""
    C_ = _C()
    x, _, _ = O.ordinary((3, 5, 3, 12), dt)
    z12 = torch.zeros(12, device=dev)
    y, stat, _ = C_.bn_nhwc_fwd(x.to(dev), None, z12, z12, None, None, None, 0.1, 1e-5, True, False, None, 256)
    dx, _, dw, db = C_.bn_nhwc_bwd(O.grad_for(x.shape, dt, seed=1).to(dev), x.to(dev), None, z12, stat, True, False, None)
    for t in (y, dx, dw, db):
        assert bool((t == 0).all())


@pytest.mark.parametrize("route", ["1", "0"], ids=["mask", "recompute"])
@pytest.mark.parametrize("zero", [0.0, -0.0], ids=["+0", "-0"])
@pytest.mark.parametrize("dt", DT, ids=DT_IDS)
def test_bn_relu_exactly_zero_with_residual(dev, dt, zero, route, monkeypatch):
    from cs744_pytorch_distributed_tutorial_amd.ops.cnn_nhwc import bn_act_nhwc
    monkeypatch.setenv("CS_BN_MASK", route)
    bn = nn.BatchNorm2d(12).to(dev)
    with torch.no_grad():
        bn.weight.zero_()
    x = O.ordinary((3, 5, 3, 12), dt)[0].to(dev).requires_grad_()
    res = torch.full((3, 5, 3, 12), zero, dtype=dt, device=dev).requires_grad_()
    y = bn_act_nhwc(bn, x, True, res)
    y.backward(O.grad_for(x.shape, dt, seed=1).to(dev))
    for t in (y, x.grad, res.grad, bn.weight.grad, bn.bias.grad):
        assert bool((t == 0).all())


TILE_CASES = [(1, 16, 16), (1, 256, 100), (33, 256, 8193), (70, 16, 1105), (3, 256, 513)]


@pytest.mark.parametrize("dt,C", [(F32, 12), (BF16, 24)], ids=DT_IDS)
@pytest.mark.parametrize("T,R,M", TILE_CASES)
def test_bn_synthetic_tiles(dev, T, R, M, dt, C):
    """finalize_tiles_kernel on float64-built tile partials: against its own oracle, and against the
    statistics pass on the same x"""
    x, gamma, beta = O.ordinary((M, 1, 1, C), dt, seed=T)
    tiles = O.tile_partials(x, R)
    assert tiles.shape[0] == T and M - (T - 1) * R >= 1
    rm0, rv0 = torch.linspace(-1, 1, C), torch.linspace(0.5, 2, C)
    ot = O.bn_tiles(tiles, R, M, gamma, beta, rm0, rv0, 0.3, 1e-3)
    _, st_t = _bn_run(dev, f"tiles T={T} R={R}", x, gamma, beta, None, True, 0.3, 1e-3, tiles=tiles.to(dev), tile_rows=R,
                      o=ot, backward=False)
    os_, st_s = _bn_run(dev, f"stats M={M}", x, gamma, beta, None, True, 0.3, 1e-3, backward=False)
    e_mean, e_var = O.tile_rounding(tiles, R, M)
    O.check(st_t[2], st_s[2].double().cpu(), ot["e_mean"] + os_["e_mean"] + e_mean, f"tiles vs pass mean T={T}")
    O.check(st_t[3], st_s[3].double().cpu(), ot["e_invstd"] + os_["e_invstd"] + 0.51 * os_["invstd"] ** 3 * e_var,
            f"tiles vs pass invstd T={T}")


@pytest.mark.parametrize("M", [1, 255, 257, 513])
def test_gemm_tile_statistics(dev, M):
    """mm_bf16_bn_stats: per-256-row-tile (mean, M2) of a ragged-N product with a column mean near 100,
    against float64 of the y it returned"""
    C_ = _C()
    g = torch.Generator().manual_seed(600 + M)
    N, K = 200, 64
    a = (torch.randn(M, K, generator=g) * 0.25 + 1.0).bfloat16().to(dev)
    b = (torch.randn(N, K, generator=g) * 0.1 + 100.0 / K).bfloat16().to(dev)
    y, tiles = C_.mm_bf16_bn_stats(a, b.t())
    torch.cuda.synchronize()
    assert tiles.shape == ((M + 255) // 256, N, 2) and torch.equal(y, C_.mm_bf16(a, b.t()))
    assert 80 < float(y.float().mean()) < 120
    mean, e_mean, M2, e_M2 = O.gemm_tile_stats(y.cpu())
    O.check(tiles[..., 0], mean, e_mean, f"gemm tile mean M={M}")
    O.check(tiles[..., 1], M2, e_M2, f"gemm tile M2 M={M}")


# ======================================================================================= max-pool
@pytest.mark.parametrize("dt", DT, ids=DT_IDS)
@pytest.mark.parametrize("name,x", O.pool_shapes() + O.pool_ties(), ids=lambda v: v if isinstance(v, str) else "")
def test_pool_forward_exact_and_backward(dev, name, x, dt):
    C_ = _C()
    B, H, W, C = x.shape
    y, pos = C_.maxpool3s2_nhwc_fwd(x.to(dt).to(dev))
    ry, rpos = O.pool_fwd(x)
    assert _eq(y, ry), f"{name}: values"
    assert torch.equal(pos.cpu().long(), rpos), f"{name}: window positions"
    dy = O.grad_for(ry.shape, dt, seed=3)
    dx = C_.maxpool3s2_nhwc_bwd(dy.to(dev), pos, H, W)
    rdx, ab = O.pool_bwd(dy, rpos, H, W)
    O.check(dx, rdx, O.store_bound(rdx, 3 * O.U * ab, dt), f"pool bwd {name}")


@pytest.mark.parametrize("dt", DT, ids=DT_IDS)
def test_pool_backward_shared_input(dev, dt):
    """an input picked by four windows, and by two: the gradients are summed in fp32 and rounded once"""
    C_ = _C()
    x = O.pool_shared()
    y, pos = C_.maxpool3s2_nhwc_fwd(x.to(dt).to(dev))
    _, rpos = O.pool_fwd(x)
    assert torch.equal(pos.cpu().long(), rpos)
    dy = O.grad_for(y.shape, dt, seed=4)
    dx = C_.maxpool3s2_nhwc_bwd(dy.to(dev), pos, 5, 5)
    rdx, ab = O.pool_bwd(dy, rpos, 5, 5)
    cnt = torch.zeros(3, 25, 8, dtype=torch.float64).scatter_add_(1, O.pool_index(rpos, 5, 5).reshape(3, -1, 8),
                                                                 torch.ones(3, 9, 8, dtype=torch.float64)).view(3, 5, 5, 8)
    assert float(cnt[0, 1, 1].min()) == 4 and float(cnt[1, 1, 2].min()) == 2 and float(cnt[2, 2, 1].min()) == 2
    O.check(dx, rdx, O.store_bound(rdx, 3 * O.U * ab, dt), "pool bwd shared")


@pytest.mark.parametrize("H,W", [(7, 7), (8, 8), (7, 8), (2, 3)])
@pytest.mark.parametrize("dt,C", [(BF16, 16), (BF16, 12), (BF16, 5), (F32, 8), (F32, 5)], ids=["bf16-V8", "bf16-V4", "bf16-V1", "f32-V4", "f32-V1"])
def test_fused_pool_backward_equals_two_pass(dev, dt, C, H, W):
    """bn_nhwc_bwd(pool_pos=, H=, W=) (bwd_reduce_kernel / apply_bwd_kernel POOL = true, pool_grad) against
    maxpool3s2_nhwc_bwd then bn_nhwc_bwd, bit for bit"""
    C_ = _C()
    x, gamma, beta = O.ordinary((3, H, W, C), dt, seed=H * W)
    xg, w = x.to(dev), gamma.to(dev)
    y, pos, stat = C_.bn_relu_maxpool_nhwc_fwd(xg, w, beta.to(dev), None, None, None, 0.1, 1e-5)
    dy = O.grad_for(y.shape, dt, seed=5).to(dev)
    g = C_.maxpool3s2_nhwc_bwd(dy, pos, H, W)
    two = C_.bn_nhwc_bwd(g, xg, None, w, stat, True, False)
    one = C_.bn_nhwc_bwd(dy, xg, None, w, stat, True, False, None, pos, H, W)
    torch.cuda.synchronize()
    for a, b, n in zip(one, two, ("dx", "dres", "dweight", "dbias")):
        if n != "dres":
            assert torch.equal(a, b), n


@pytest.mark.parametrize("dt", DT, ids=DT_IDS)
def test_bn_relu_maxpool_against_oracle(dev, dt):
    """the fused stem op against the oracle itself; channel 3's post-ReLU windows are all zero"""
    from cs744_pytorch_distributed_tutorial_amd.ops.cnn_nhwc import bn_relu_maxpool_nhwc
    x, gamma, beta = O.ordinary((2, 7, 8, 16), dt, seed=11)
    gamma, beta = gamma.abs(), beta.clone()
    beta[3] = -100.0
    bn = nn.BatchNorm2d(16).to(dev)
    with torch.no_grad():
        bn.weight.copy_(gamma)
        bn.bias.copy_(beta)
    xg = x.to(dev).requires_grad_()
    y = bn_relu_maxpool_nhwc(bn, xg)
    o = O.bn_stats(x, gamma, beta, torch.zeros(16), torch.ones(16), 0.1, 1e-5)
    full, e, _, _ = O.bn_apply(x, o, None, True)
    ref = O.pool_fwd(full)[0]
    O.check(y, ref, O.pool_max_bound(O.store_bound(full, e, dt)), "bn_relu_maxpool y")
    assert bool((y[..., 3] == 0).all())
    _, pos, _ = _C().bn_relu_maxpool_nhwc_fwd(x.to(dev), bn.weight.detach(), bn.bias.detach(), None, None, None, 0.1, 1e-5)
    assert torch.equal(pos[..., 3].cpu().long(), O.pool_fwd(torch.zeros(2, 7, 8, 1, dtype=torch.float64))[1][..., 0])
    y.backward(O.grad_for(y.shape, dt, seed=6).to(dev))
    assert bool((xg.grad[..., 3] == 0).all()) and float(bn.weight.grad[3]) == 0 and float(bn.bias.grad[3]) == 0
    assert bool(torch.isfinite(xg.grad).all())


# ================================================================================ im2col / col2im
@pytest.mark.parametrize("dt", DT, ids=DT_IDS)
@pytest.mark.parametrize("geo", O.IM2COL_CASES, ids=lambda g: "x".join(map(str, g)))
def test_im2col_exact_and_col2im(dev, geo, dt):
    C_ = _C()
    B, H, W, C, R, S, st, pad = geo
    V, K = O.vec_for(C, dt), R * S * C
    Kp = K + 3 if V == 1 else (K + V - 1) // V * V + V
    x = O.grad_for((B, H, W, C), dt, seed=7)
    col = C_.im2col_nhwc(x.to(dev), R, S, st, pad, Kp)
    ref = O.im2col_ref(x, R, S, st, pad, Kp)
    assert col.dtype == dt and torch.equal(col.double().cpu(), ref), "im2col is a gather: bit for bit"
    assert bool((col[:, K:] == 0).all())
    dcol = O.grad_for(ref.shape, dt, seed=8)
    dx = C_.col2im_nhwc(dcol.to(dev), B, H, W, C, R, S, st, pad)
    rdx, ab, taps = O.col2im_ref(dcol, B, H, W, C, R, S, st, pad)
    O.check(dx, rdx, O.store_bound(rdx, (taps + 1) * O.U * ab, dt), f"col2im {geo}")


# ============================================================================== bf16 implicit conv
def _conv_run(dev, geo, splits):
    C_ = _C()
    B, H, W, C, Co, R, S, st, pad = geo
    x, w, dy = O.conv_inputs(*geo)
    ref = O.conv_ref(x, w, dy, st, pad, splits)
    xg, wg, gg = x.to(dev), w.to(dev), dy.to(dev)
    y = C_.conv_nhwc_bf16(0, xg, wg, R, S, st, pad, 0, 0)
    dx = C_.conv_nhwc_bf16(1, gg, wg.permute(3, 1, 2, 0).contiguous(), R, S, st, pad, H, W)
    dw = C_.conv_nhwc_bf16(2, gg, xg, R, S, st, pad, 0, 0)
    dw2 = C_.conv_nhwc_bf16(2, gg, xg, R, S, st, pad, 0, 0)
    torch.cuda.synchronize()
    assert y.shape == ref["y"].shape and dx.shape == x.shape and dw.shape == (Co, R * S * C)
    O.check(y, ref["y"], ref["e_y"], f"conv y {geo}")
    O.check(dx, ref["dx"], ref["e_dx"], f"conv dx {geo}")
    O.check(dw.view(Co, R, S, C), ref["dw"], ref["e_dw"], f"conv dw {geo}")
    assert torch.equal(dw, dw2), "weight gradient not bit-equal run to run"


@pytest.mark.parametrize("geo", O.CONV_CASES, ids=lambda g: "x".join(map(str, g)))
def test_conv_geometries(dev, geo):
    B, H, W, C, Co, R, S, st, pad = geo
    assert _C().conv_nhwc_splits(2, B, H, W, C, Co, R, S, st, pad) == 1
    _conv_run(dev, geo, 1)


@pytest.mark.parametrize("geo,alloc,launched", O.SPLIT_CASES, ids=["two", "ragged-last", "fewer-than-allocated"])
def test_conv_split_k_weight_gradient(dev, geo, alloc, launched):
    B, H, W, C, Co, R, S, st, pad = geo
    assert _C().conv_nhwc_splits(2, B, H, W, C, Co, R, S, st, pad) == alloc
    assert _C().conv_nhwc_splits(0, B, H, W, C, Co, R, S, st, pad) == 1
    assert O.conv_splits(*geo) == (alloc, launched)
    _conv_run(dev, geo, launched)


IMPULSE = [(5, 6, 3, 3, 1, 1), (2, 2, 3, 3, 1, 1), (7, 9, 3, 3, 2, 1), (9, 7, 5, 5, 2, 2), (6, 5, 1, 3, 1, 1), (5, 6, 3, 1, 1, 1),
           (8, 8, 3, 3, 3, 1), (6, 6, 3, 3, 1, 0), (5, 5, 3, 3, 1, 2)]


@pytest.mark.parametrize("H,W,R,S,st,pad", IMPULSE)
def test_conv_distinct_tap_impulses_exact(dev, H, W, R, S, st, pad):
    """single ones at the corners, an edge mid-point and across the image boundary, integer weights
    distinct per tap: every value is a small integer, y and dx must equal the reference exactly"""
    C_ = _C()
    x, w = O.impulse_case(H, W, 32, 32, R, S)
    y = C_.conv_nhwc_bf16(0, x.to(dev), w.to(dev), R, S, st, pad, 0, 0)
    ref = torch.nn.functional.conv2d(x.double().permute(0, 3, 1, 2), w.double().permute(0, 3, 1, 2), None, st, pad)
    assert torch.equal(y.double().cpu(), ref.permute(0, 2, 3, 1)), "forward"
    Ho, Wo = O.conv_geo(H, W, R, S, st, pad)
    dy, wt = O.impulse_case(Ho, Wo, 32, 32, R, S)  # wt [C, R, S, Co]
    dx = C_.conv_nhwc_bf16(1, dy.to(dev), wt.to(dev), R, S, st, pad, H, W)
    rdx = torch.nn.grad.conv2d_input((2, 32, H, W), wt.double().permute(3, 0, 1, 2), dy.double().permute(0, 3, 1, 2), st, pad)
    assert torch.equal(dx.double().cpu(), rdx.permute(0, 2, 3, 1)), "dgrad"


@pytest.mark.parametrize("H,W,Co,R,st,pad", O.STEM_CASES, ids=lambda v: str(v))
def test_conv_stem_c4(dev, H, W, Co, R, st, pad):
    """C4 mode: taps s >= S of the padded weight zero, channel 3 of x non-zero under a zero weight channel"""
    C_ = _C()
    x, w, dy = O.conv_inputs(2, H, W, 4, Co, R, R, st, pad, seed=H * W)
    w = w.clone()
    w[..., 3] = 0
    assert float(x[..., 3].abs().min()) >= 0 and float(x[..., 3].abs().max()) > 0
    assert C_.conv_nhwc_splits(2, 2, H, W, 4, Co, R, R, st, pad) == 1
    ref = O.conv_ref(x, w, dy, st, pad, 1)
    wp = torch.nn.functional.pad(w, (0, 0, 0, 8 - R)).contiguous()
    y = C_.conv_nhwc_bf16(0, x.to(dev), wp.to(dev), R, R, st, pad, 0, 0)
    dw = C_.conv_nhwc_bf16(2, dy.to(dev), x.to(dev), R, R, st, pad, 0, 0)
    torch.cuda.synchronize()
    O.check(y, ref["y"], ref["e_y"], f"stem y {H}x{W} k{R}")
    assert dw.shape == (Co, R * 32)
    O.check(dw.view(Co, R, 8, 4)[:, :, :R].contiguous(), ref["dw"], ref["e_dw"], f"stem dw {H}x{W} k{R}")
    # distinct-tap impulses at columns 0 and W - 1: both halves of a pixel pair at the image's edges
    pts = [(0, 0, 0), (0, H - 1, W - 1), (1, H // 2, 0), (1, 0, W - 1)]
    xi, wi = O.impulse_case(H, W, 4, Co, R, R, pts)
    yi = C_.conv_nhwc_bf16(0, xi.to(dev), torch.nn.functional.pad(wi, (0, 0, 0, 8 - R)).contiguous().to(dev), R, R, st, pad, 0, 0)
    ri = torch.nn.functional.conv2d(xi.double().permute(0, 3, 1, 2), wi.double().permute(0, 3, 1, 2), None, st, pad)
    assert torch.equal(yi.double().cpu(), ri.permute(0, 2, 3, 1)), "stem impulses"


@pytest.mark.parametrize("S", [32, 33, 128, 129, 257])
def test_slab_sum_lane_edges(dev, S):
    part = O.grad_for((S, 5, 12), F32, seed=S)
    ref, e = O.slab_ref(part)
    a, b = _C().slab_sum(part.to(dev)), _C().slab_sum(part.to(dev))
    assert torch.equal(a, b)
    O.check(a, ref, e, f"slab_sum S={S}")


# ================================================================================== host refusals
def test_host_refusals(dev):
    """every one is raised by the binding's checks, before any launch"""
    C_ = _C()
    x = O.ordinary((2, 7, 8, 16), BF16)[0].to(dev)
    w = torch.ones(16, device=dev)
    y, pos, stat = C_.bn_relu_maxpool_nhwc_fwd(x, w, w, None, None, None, 0.1, 1e-5)
    dy = torch.zeros_like(y)
    full = torch.zeros_like(x)
    bad = [
        lambda: C_.bn_nhwc_bwd(dy, x, None, w, stat, True, False, None, pos.to(torch.int8), 7, 8),   # not uint8
        lambda: C_.bn_nhwc_bwd(dy, x, None, w, stat, True, False, None, pos.cpu(), 7, 8),            # not on the GPU
        lambda: C_.bn_nhwc_bwd(dy, x, None, w, stat, True, False, None, pos[:, :, :3], 7, 8),        # wrong size
        lambda: C_.bn_nhwc_bwd(dy, x, None, w, stat, True, False, None, pos.permute(0, 2, 1, 3), 7, 8),  # not contiguous
        lambda: C_.bn_nhwc_bwd(full, x, None, w, stat, True, False, None, pos, 7, 8),                # dy not pooled
        lambda: C_.bn_nhwc_bwd(dy, x, None, w, stat, True, False, None, pos, 8, 7),                  # H, W not x's
        lambda: C_.bn_nhwc_bwd(dy, x, None, w, stat, True, False, None, pos),                        # no H, W
        lambda: C_.bn_nhwc_bwd(dy, x, full, w, stat, True, True, None, pos, 7, 8),                   # residual
        lambda: C_.bn_nhwc_bwd(dy, x, None, w, stat, True, False, torch.zeros(2 * 7 * 8 * 2, dtype=torch.uint8, device=dev),
                               pos, 7, 8),                                                           # mask
        lambda: C_.bn_nhwc_bwd(full, x, None, w, stat, True, False, None, None, 7, 8),               # H, W without pool_pos
        lambda: C_.bn_nhwc_fwd(x, None, w, w, None, None, None, 0.1, 1e-5, True, False,
                               torch.zeros(2, 16, 2, device=dev), 256),                              # T = 2, ceil(112 / 256) = 1
        lambda: C_.bn_nhwc_fwd(x, None, w, w, None, None, None, 0.1, 1e-5, True, False,
                               torch.zeros(6, 16, 2, device=dev), 16),                               # T = 6, ceil(112 / 16) = 7
        lambda: C_.im2col_nhwc(x, 3, 3, 1, 1, 3 * 3 * 16 - 8),                                       # Kp < K
        lambda: C_.im2col_nhwc(x, 3, 3, 1, 1, 3 * 3 * 16 + 4),                                       # Kp % 8 != 0 (bf16, C = 16)
    ]
    x32 = torch.zeros(1, 1, 2, 32, dtype=BF16, device=dev)
    w32 = torch.zeros(32, 3, 3, 32, dtype=BF16, device=dev)
    bad += [lambda: C_.conv_nhwc_bf16(0, x32, w32, 3, 3, 1, 0, 0, 0),                                # Ho = -1
            lambda: C_.conv_nhwc_bf16(0, torch.zeros(1, 2, 2, 32, dtype=BF16, device=dev), w32, 3, 3, 2, 0, 0, 0),
            lambda: C_.conv_nhwc_bf16(2, torch.zeros(1, 1, 1, 32, dtype=BF16, device=dev), x32, 3, 3, 1, 0, 0, 0)]
    for i, f in enumerate(bad):
        with pytest.raises(RuntimeError):
            f()
            pytest.fail(f"refusal {i} was accepted")
    torch.cuda.synchronize()
