"""Edge tests of the NHWC fp32 BatchNorm + ReLU (+ 2x2 max-pool) kernels (bn.hip, bn_device.h,
bn_fin.h) and of the BN-backward partial sums computed in the data-gradient GEMM epilogue and the
split-K combine (conv_common.h dgrad_bn_partials, conv_gemm.hip splitk_reduce_body), MI355X only.

Oracle: tests/bn_oracle.py, plain float64 on the same fp32 values, with per-channel bounds derived
from the fp32 roundings (checked on the CPU by tests/test_bn_oracles_cpu.py). Which branch each case
enters, the derivations and the errors measured are in docs/bn_edge_tests.md; the case letters are
the ones used there."""
import pytest
import torch
import torch.nn.functional as F

import bn_oracle as O

pytestmark = pytest.mark.gpu

PAIRS = [(0.3, 1e-3), (1.0, 1e-5), (0.0, 1e-2)]
SENT = 12345.0


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cs744_pytorch_distributed_tutorial_amd.ops import native
    native.C()
    return torch.device("cuda", 0)


def _fn():
    from cs744_pytorch_distributed_tutorial_amd.ops import functional as Fn
    return Fn


def _state(dev, scale, shift, mean, invstd):
    st = _fn().BNState(scale.numel(), dev)
    st.scale, st.shift, st.mean, st.invstd = (t.float().to(dev).contiguous() for t in (scale, shift, mean, invstd))
    return st


# ====================================================================================== forward
def _check_stats(name, bs, o):
    for k in ("scale", "shift", "mean", "invstd"):
        O.check(getattr(bs, k), o[k], o["e_" + k], f"{name} {k}")


def _run_fwd(dev, name, y, gamma, beta, R, pool, fused, momentum=0.1, eps=1e-5, running=True, nbt0=41):
    """One forward through bn_finalize + bn_apply (fused: bn_fused_fwd) against the oracle."""
    Fn = _fn()
    B, H, W, C = y.shape
    M = B * H * W
    st = O.tile_partials(y, R)
    rm0, rv0 = torch.linspace(-1, 1, C), torch.linspace(0.5, 2, C)
    o = O.fwd_oracle(st, R, M, gamma, beta, rm0, rv0, momentum, eps)
    rm, rv = rm0.to(dev), rv0.to(dev)
    if not running:
        rm.fill_(SENT), rv.fill_(SENT)
    nbt = None if nbt0 is None else torch.full((), nbt0, dtype=torch.int64, device=dev)
    out, bs = Fn.bn_relu_pool_fwd(y.to(dev), st.to(dev), R, B, H, W, gamma.to(dev), beta.to(dev),
                                  rm if running else None, rv if running else None, nbt, pool=pool,
                                  momentum=momentum, eps=eps, fused=fused)
    torch.cuda.synchronize()
    tag = f"{name} {'fused' if fused else 'finalize+apply'} pool={int(pool)}"
    _check_stats(tag, bs, o)
    ref, bound = O.apply_oracle(y, o, gamma, pool)
    O.check(out, ref, bound, f"{tag} out")
    if running:
        O.check(rm, o["running_mean"], o["e_running_mean"], f"{tag} running_mean")
        O.check(rv, o["running_var"], o["e_running_var"], f"{tag} running_var")
    else:  # nothing to update: the buffers the caller did not pass keep their contents
        assert bool((rm == SENT).all()) and bool((rv == SENT).all())
    if nbt is not None:
        assert int(nbt) == nbt0 + 1
    return o, bs, out


def _paths(C, H, W):
    """(fused, pool) combinations the launchers admit: apply needs C % 4, fused C % 16, pool even H, W"""
    pools = [False, True] if H % 2 == 0 and W % 2 == 0 else [False]
    return [(f, p) for f in ([False, True] if C % 16 == 0 else [False]) for p in pools]


@pytest.mark.parametrize("momentum,eps", PAIRS)
def test_a_momentum_and_eps(dev, momentum, eps):
    y, gamma, beta = O.ordinary(2, 4, 4, 16)
    for fused, pool in _paths(16, 4, 4):
        _run_fwd(dev, "a", y, gamma, beta, 8, pool, fused, momentum, eps)


@pytest.mark.parametrize("fused", [False, True])
def test_a_running_none_and_nbt(dev, fused):
    y, gamma, beta = O.ordinary(2, 4, 4, 16)
    _run_fwd(dev, "a no-running", y, gamma, beta, 8, True, fused, 0.3, 1e-3, running=False)
    _run_fwd(dev, "a no-nbt", y, gamma, beta, 8, False, fused, 0.3, 1e-3, nbt0=None)
    _run_fwd(dev, "a neither", y, gamma, beta, 8, False, fused, 0.3, 1e-3, running=False, nbt0=None)


@pytest.mark.parametrize("momentum,eps,running", [(m, e, True) for m, e in PAIRS] + [(0.3, 1e-3, False)])
def test_a_in_launch_finalize(dev, momentum, eps, running):
    """conv_fwd(fin=): the last-arriving block's finalize (bn_fin.h finish<false>) with the same pairs,
    against the oracle applied to the statistics partials the launch itself wrote."""
    Fn = _fn()
    g = torch.Generator().manual_seed(5)
    B, H, W, cin, cout = 2, 8, 8, 64, 64
    x = (torch.randn(B, H, W, cin, generator=g) * 2 + 0.75).to(dev)
    w = (torch.randn(cout, 3, 3, cin, generator=g) / (3 * cin ** 0.5)).to(dev)
    gamma, beta = (torch.rand(cout, generator=g) + 0.5) * 3, torch.randn(cout, generator=g)
    rm0, rv0 = torch.linspace(-1, 1, cout), torch.linspace(0.5, 2, cout)
    rm, rv = (rm0.to(dev), rv0.to(dev)) if running else (torch.full((cout,), SENT, device=dev),) * 2
    fin = dict(gamma=gamma.to(dev), beta=beta.to(dev), momentum=momentum, eps=eps)
    if running:
        fin.update(running_mean=rm, running_var=rv)
    y, st, rows, bs = Fn.conv_fwd(x, w, None, bm=64, bn=64, splits=1, stats=True, bk=16, stage=0, fin=fin)
    torch.cuda.synchronize()
    assert rows == 64 and st.shape[0] == 2
    o = O.fwd_oracle(st.cpu(), rows, B * H * W, gamma, beta, rm0, rv0, momentum, eps)
    _check_stats(f"fin {momentum} {eps}", bs, o)
    if running:
        O.check(rm, o["running_mean"], o["e_running_mean"], "fin running_mean")
        O.check(rv, o["running_var"], o["e_running_var"], "fin running_var")
    else:
        assert bool((rm == SENT).all())


@pytest.mark.parametrize("eps", [1e-5, 1e-3, 1e-2])
@pytest.mark.parametrize("shape", [(2, 4, 4, 16), (3, 2, 8, 16), (2, 8, 2, 16), (1, 2, 2, 4)])
def test_a_eval(dev, eps, shape):
    Fn = _fn()
    B, H, W, C = shape
    y, gamma, beta = O.ordinary(B, H, W, C)
    rm, rv = torch.linspace(-2, 2, C), torch.linspace(1e-3, 4, C)
    o = O.eval_oracle(gamma, beta, rm, rv, eps)
    for pool in (False, True):
        out = Fn.bn_relu_pool_eval(y.to(dev), B, H, W, gamma.to(dev), beta.to(dev), rm.to(dev), rv.to(dev), pool=pool,
                                   eps=eps)
        ref, bound = O.apply_oracle(y, o, gamma, pool)
        O.check(out, ref, bound, f"eval {shape} eps={eps} pool={int(pool)}")


FWD = [c for c in O.FWD_CASES if c[0] not in ("a", "d5", "d6")]


@pytest.mark.parametrize("name,builder,shape,R", FWD, ids=[c[0] for c in FWD])
def test_bcdef_forward(dev, name, builder, shape, R):
    """(b) M = 1, (c) the per-channel ladder, (d) the finalize dispatch edge, (e) non-square,
    (f) the fused forward's chunking; momentum 0.3 / eps 1e-3 so neither default is assumed."""
    y, gamma, beta = O.build(builder, shape)
    B, H, W, C = y.shape
    for fused, pool in _paths(C, H, W):
        o, bs, _ = _run_fwd(dev, name, y, gamma, beta, R, pool, fused, 0.3, 1e-3)
    if name == "b":  # n > 1.f ? M2 / (n - 1) : var
        assert float(o["var"].abs().max()) == 0.0
    if builder is O.ladder:  # the constant channel: M2 stays exactly 0
        assert abs(float(bs.invstd[15]) - 1e-3 ** -0.5) <= 4 * O.U * 1e-3 ** -0.5


@pytest.mark.parametrize("C", [5, 6])
def test_d_finalize_alone_odd_channels(dev, C):
    """C not a multiple of 4: the last block's idle waves (c < C); bn_apply does not take such a C"""
    from cs744_pytorch_distributed_tutorial_amd.ops import native
    y, gamma, beta = O.ordinary(3, 2, 8, C)
    R, M = 7, 48
    st = O.tile_partials(y, R)
    rm0, rv0 = torch.linspace(-1, 1, C), torch.linspace(0.5, 2, C)
    o = O.fwd_oracle(st, R, M, gamma, beta, rm0, rv0, 0.3, 1e-3)
    rm, rv = rm0.to(dev), rv0.to(dev)
    nbt = torch.full((), 41, dtype=torch.int64, device=dev)
    bs = _fn().BNState(C, dev)
    # each output is the first C floats of an 8-float row: a store past c < C lands on a sentinel
    guard = torch.full((6, 8), SENT, device=dev)
    guard[4, :C], guard[5, :C] = rm0.to(dev), rv0.to(dev)
    bs.scale, bs.shift, bs.mean, bs.invstd, rm, rv = (guard[i] for i in range(6))
    native.C().bn_finalize(st.to(dev), st.shape[0], R, M, gamma.to(dev), beta.to(dev), rm, rv, nbt, 0.3, 1e-3,
                           bs.scale, bs.shift, bs.mean, bs.invstd)
    torch.cuda.synchronize()
    assert bool((guard[:, C:] == SENT).all())
    bs.scale, bs.shift, bs.mean, bs.invstd = (guard[i, :C] for i in range(4))
    _check_stats(f"d C={C}", bs, o)
    O.check(rm[:C], o["running_mean"], o["e_running_mean"], "running_mean")
    O.check(rv[:C], o["running_var"], o["e_running_var"], "running_var")
    assert int(nbt) == 42


# ====================================================================================== backward
def _tile_part(o, dev):
    return o["tile_sums"].float().contiguous().to(dev)


def _run_bwd(dev, name, y, G, scale, shift, mean, invstd, gamma, pool):
    """bn_bwd, bn_fused_bwd, bn_bwd_tail and bn_bwd_tail_fused (where the shape rules admit) against
    the oracle; the tails are fed the oracle's 16-row tile sums rounded to fp32."""
    Fn = _fn()
    B, H, W, C = y.shape
    M = B * H * W
    o = O.bwd_oracle(y, G, scale, shift, mean, invstd, gamma, pool, rows=16)
    st = _state(dev, scale, shift, mean, invstd)
    yd, Gd, gd = y.to(dev), G.to(dev), gamma.to(dev)
    got = {}
    for fused in ([False, True] if C % 16 == 0 else [False]):
        tag = f"{name} {'bn_fused_bwd' if fused else 'bn_bwd'}"
        dz, dgamma, dbeta, dbias = Fn.bn_relu_pool_bwd(yd, Gd, st, gd, B, H, W, pool=pool, fused=fused)
        torch.cuda.synchronize()
        O.check(dgamma, o["dgamma"], o["e_sums"][1], f"{tag} dgamma")
        O.check(dbeta, o["dbeta"], o["e_sums"][0], f"{tag} dbeta")
        O.check(dbias, o["dbias"], o["e_dbias"], f"{tag} dbias")
        O.check(dz, o["dz"], o["e_dz"], f"{tag} dz")
        got[tag] = dz
    part = _tile_part(o, dev)
    t = O.tail_oracle(part.cpu(), M, gamma, invstd)
    dzr, e_dz = O.dz_from_coef(y, G, o["sel"], mean, invstd, t["coef"], t["e_coef"], pool)
    for fused in ([False, True] if C % 16 == 0 else [False]):
        tag = f"{name} {'bn_bwd_tail_fused' if fused else 'bn_bwd_tail'}"
        dz, dgamma, dbeta, dbias, coef = Fn.bn_relu_pool_bwd_tail(yd, Gd, st, gd, B, H, W, part, part.shape[0],
                                                                  pool=pool, fused=fused)
        torch.cuda.synchronize()
        for k, v in (("dgamma", dgamma), ("dbeta", dbeta), ("dbias", dbias), ("coef", coef)):
            O.check(v, t[k], t["e_" + k], f"{tag} {k}")
        O.check(dz, dzr, e_dz, f"{tag} dz")
        got[tag] = dz
    return o, got


@pytest.mark.parametrize("kind", O.TIE_KINDS)
def test_g_decisions(dev, kind):
    d = O.tie_case(kind)
    o, got = _run_bwd(dev, f"g {kind}", d["y"], d["G"], d["scale"], d["shift"], d["mean"], d["invstd"], d["gamma"], True)
    if kind == "scale0":  # gamma = 0: dz = 0 exactly, while dgamma depends on which element is routed
        assert all(float(v.abs().max()) == 0.0 for v in got.values())
        assert float(o["dgamma"].abs().min()) > 0.0
    if kind == "zero":
        assert float(o["sums"][0].abs().max()) == 0.0


@pytest.mark.parametrize("shape,pool", O.BWD_CASES, ids=[f"{s}-{int(p)}" for s, p in O.BWD_CASES])
def test_hi_backward_shapes(dev, shape, pool):
    """(h) channel counts 4 / 12 / 20 / 1024 and the 256- / 2048-block caps, (i) non-square"""
    B, H, W, C = shape
    y, gamma, beta = O.ordinary(B, H, W, C)
    G = O.grad_like(B, H, W, C, pool)
    sc, sh, mu, inv = O.coeffs_from(y, gamma, beta, eps=1e-3)
    _run_bwd(dev, f"h {shape} pool={int(pool)}", y, G, sc, sh, mu, inv, gamma, pool)


@pytest.mark.parametrize("P", [1, 63, 513, 700])
@pytest.mark.parametrize("fused", [False, True])
def test_j_tails_from_synthetic_partials(dev, P, fused):
    """P > 512: bn_bwd_finalize_kernel's second trip; P > 256: bn_bwd_tail_fused_kernel's"""
    Fn = _fn()
    B, H, W, C, pool = 2, 4, 4, 16, True
    y, gamma, beta = O.ordinary(B, H, W, C)
    G = O.grad_like(B, H, W, C, pool)
    sc, sh, mu, inv = O.coeffs_from(y, gamma, beta)
    g = torch.Generator().manual_seed(P)
    part = (torch.randn(P, C, 3, generator=g) * 10 ** torch.randint(-2, 3, (P, 1, 1), generator=g).float()).contiguous()
    t = O.tail_oracle(part, B * H * W, gamma, inv)
    _, sel = O.decisions(y, sc, sh, pool)
    dzr, e_dz = O.dz_from_coef(y, G, sel, mu, inv, t["coef"], t["e_coef"], pool)
    st = _state(dev, sc, sh, mu, inv)
    runs = []
    for _ in range(2):
        res = Fn.bn_relu_pool_bwd_tail(y.to(dev), G.to(dev), st, gamma.to(dev), B, H, W, part.to(dev), P, pool=pool,
                                       fused=fused)
        torch.cuda.synchronize()
        runs.append([r.cpu() for r in res])
    dz, dgamma, dbeta, dbias, coef = runs[0]
    tag = f"j P={P} fused={int(fused)}"
    for k, v in (("dgamma", dgamma), ("dbeta", dbeta), ("dbias", dbias), ("coef", coef)):
        O.check(v, t[k], t["e_" + k], f"{tag} {k}")
    O.check(dz, dzr, e_dz, f"{tag} dz")
    assert all(torch.equal(a, b) for a, b in zip(*runs))


# ====================================================================================== ered
ERED_TILES = [(64, 64, 1, 16, 0), (128, 64, 1, 32, 0), (64, 128, 1, 32, 3), (64, 64, 1, 64, 4), (64, 64, 1, 64, 16 | 4),
              (64, 64, 1, 32, 64), (64, 64, 3, 16, 0), (64, 64, 64, 16, 0)]
ERED = [(s, n, p, t) for s in [(3, 4, 4), (5, 8, 8), (2, 4, 16)] for n in (64, 128) for p in (False, True)
        for t in ERED_TILES]


@pytest.mark.parametrize("shape,N,pool,tile", ERED, ids=[f"{s}-{n}-{int(p)}-{t}" for s, n, p, t in ERED])
def test_k_dgrad_with_ered(dev, shape, N, pool, tile):
    Fn = _fn()
    from cs744_pytorch_distributed_tutorial_amd.ops import native
    B, H, W = shape
    bm, bn, sp, bk, stage = tile
    cout, M = 64, B * H * W
    g = torch.Generator().manual_seed(N + H)
    dz = torch.randn(M, cout, generator=g).to(dev)
    w = (torch.randn(cout, 3, 3, N, generator=g) / (3 * cout ** 0.5)).to(dev)
    Hy, Wy = (2 * H, 2 * W) if pool else (H, W)
    y, gamma, beta = O.ordinary(B, Hy, Wy, N)
    sc, sh, mu, inv = O.coeffs_from(y, gamma, beta, eps=1e-3)
    st = _state(dev, sc, sh, mu, inv)
    yd, gd = y.to(dev), gamma.to(dev)
    kw = dict(bm=bm, bn=bn, splits=sp, bk=bk, stage=stage)
    dx0 = Fn.conv_dgrad(dz, w, B, H, W, **kw)
    runs = []
    for _ in range(2):
        dx, part, P = Fn.conv_dgrad(dz, w, B, H, W, ered=dict(y=yd, st=st, pool=pool), **kw)
        torch.cuda.synchronize()
        runs.append((dx.cpu(), part.cpu()))
    rows = native.C().conv_ered_rows(9 * cout, bm, bk, sp)
    nsp = native.C().conv_effective_splits(9 * cout, bk, sp)
    assert rows == (bm if nsp == 1 else 16) and P == (M + rows - 1) // rows
    if sp == 64:
        assert nsp == 36  # > 32: the fold pre-pass runs before the combine
    assert torch.equal(runs[0][0], dx0.cpu()), "ered changed dx"
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    G = runs[0][0].view(B, H, W, N)
    o = O.bwd_oracle(y, G, sc, sh, mu, inv, gamma, pool, rows=rows)
    tag = f"k {shape} N={N} pool={int(pool)} {tile}"
    O.check(runs[0][1], o["tile_sums"], o["e_tile_sums"], f"{tag} partials")
    # both tails on these partials: against the oracle's sums (tile bound + the tail's own), and
    # against bn_bwd on G = dx (which carries its own summation bound)
    t = O.tail_oracle(runs[0][1], B * Hy * Wy, gamma, inv)
    e_tot = o["e_tile_sums"].sum(0) + torch.stack([t["e_dbeta"], t["e_dgamma"], torch.zeros(N, dtype=torch.float64)], 1)
    dzr, e_dz = O.dz_from_coef(y, G, o["sel"], mu, inv, t["coef"], t["e_coef"], pool)
    ref = Fn.bn_relu_pool_bwd(yd, G.to(dev), st, gd, B, Hy, Wy, pool=pool)
    for fused in (False, True):
        dzt, dgamma, dbeta, dbias, coef = Fn.bn_relu_pool_bwd_tail(yd, G.to(dev), st, gd, B, Hy, Wy, part, P, pool=pool,
                                                                   fused=fused)
        torch.cuda.synchronize()
        O.check(dgamma, o["dgamma"], e_tot[:, 1], f"{tag} tail{int(fused)} dgamma")
        O.check(dbeta, o["dbeta"], e_tot[:, 0], f"{tag} tail{int(fused)} dbeta")
        O.check(dbias, t["dbias"], t["e_dbias"], f"{tag} tail{int(fused)} dbias")
        O.check(coef, t["coef"], t["e_coef"], f"{tag} tail{int(fused)} coef")
        O.check(dzt, dzr, e_dz, f"{tag} tail{int(fused)} dz")
        O.check(dgamma, ref[1].double().cpu(), e_tot[:, 1] + o["e_sums"][1], f"{tag} tail{int(fused)} vs bn_bwd dgamma")
        O.check(dbeta, ref[2].double().cpu(), e_tot[:, 0] + o["e_sums"][0], f"{tag} tail{int(fused)} vs bn_bwd dbeta")
        O.check(dzt, ref[0].double().cpu(), e_dz + o["e_dz"], f"{tag} tail{int(fused)} vs bn_bwd dz")


def test_test_facing_bindings_refuse_bad_arguments(dev):
    """The host checks of the ered arguments and of the two tails: refused before any launch."""
    from cs744_pytorch_distributed_tutorial_amd.ops import native
    C, Fn = native.C(), _fn()
    B, H, W, N, cout = 2, 4, 4, 64, 64
    M = B * H * W
    z = lambda *s: torch.zeros(*s, device=dev)  # noqa: E731
    vec = dict(ered_scale=z(N), ered_shift=z(N), ered_mean=z(N), ered_invstd=z(N))
    conv = lambda mode, **kw: C.conv_gemm(mode, z(B, H, W, N), z(cout, 3, 3, N), z(M, cout), None,  # noqa: E731
                                          z(M * max(N, cout)), None, None, B, H, W, N, cout, False, 64, 64, 1, 16, 0, **kw)
    good = dict(ered_y=z(M * N), ered_part=z(N * 3), **vec)
    conv(Fn.DGRAD, **good)  # the accepted form, for contrast
    with pytest.raises(RuntimeError, match="DGRAD"):
        conv(Fn.FWD, **good)
    with pytest.raises(RuntimeError, match="ered_y"):
        conv(Fn.DGRAD, **{**good, "ered_pool": True})  # pooled: y has 4 M N elements
    with pytest.raises(RuntimeError, match="ered_part"):
        conv(Fn.DGRAD, **{**good, "ered_part": z(N * 3 - 1)})
    with pytest.raises(RuntimeError, match="ered_mean"):
        conv(Fn.DGRAD, **{**good, "ered_mean": z(N - 1)})
    with pytest.raises(RuntimeError, match="ered needs"):
        conv(Fn.DGRAD, ered_part=z(N * 3), ered_y=z(M * N))
    with pytest.raises(RuntimeError, match="float32"):
        conv(Fn.DGRAD, **{**good, "ered_y": z(M * N).double()})
    tail = lambda f, Cc, P, Hh=4, pool=True, part=None: f(  # noqa: E731
        z(B * Hh * 4 * Cc), z(B * Hh * 4 * Cc), B, Hh, 4, Cc, pool, *((z(4 * Cc),) if f is C.bn_bwd_tail_fused else
                                                                      (z(Cc), z(Cc), z(Cc), z(Cc))),
        z(Cc), z(max(P, 1) * Cc * 3) if part is None else part, P, z(Cc * 3), None, None, None, z(B * Hh * 4 * Cc))
    tail(C.bn_bwd_tail, 12, 2), tail(C.bn_bwd_tail_fused, 16, 2)
    for f, Cc, P, Hh, part in [(C.bn_bwd_tail_fused, 12, 2, 4, None), (C.bn_bwd_tail, 6, 2, 4, None),
                               (C.bn_bwd_tail, 1028, 1, 4, None), (C.bn_bwd_tail, 16, 0, 4, None),
                               (C.bn_bwd_tail_fused, 16, 0, 4, None), (C.bn_bwd_tail, 16, 2, 3, None),
                               (C.bn_bwd_tail_fused, 16, 2, 3, None), (C.bn_bwd_tail, 16, 3, 4, z(2 * 16 * 3)),
                               (C.bn_bwd_tail_fused, 16, 3, 4, z(2 * 16 * 3))]:
        with pytest.raises(RuntimeError):
            tail(f, Cc, P, Hh, True, part)


# ====================================================================================== non-square conv
def _close(a, b, rel=2e-5):
    a = a.double().cpu()
    b = b.double().cpu()
    scale = b.abs().max().item() + 1e-12
    err = (a - b).abs().max().item()
    assert err <= rel * scale, f"max err {err:.3e} vs scale {scale:.3e}"


@pytest.mark.parametrize("H,W", [(4, 16), (16, 4)])
@pytest.mark.parametrize("tile", [(64, 64, 1, 16, 0), (64, 64, 1, 64, 16 | 4), (64, 64, 1, 32, 64)])
def test_l_non_square_conv(dev, H, W, tile):
    """conv fwd (+ statistics), dgrad and wgrad with H != W, at the tolerances of
    tests/test_conv_bn_gpu.py"""
    Fn = _fn()
    bm, bn, sp, bk, stage = tile
    B, cin, cout = 2, 64, 64
    g = torch.Generator().manual_seed(H)
    x = torch.randn(B, cin, H, W, generator=g, dtype=torch.float64)
    w = torch.randn(cout, cin, 3, 3, generator=g, dtype=torch.float64) / (3 * cin ** 0.5)
    b = torch.randn(cout, generator=g, dtype=torch.float64)
    gy = torch.randn(B, cout, H, W, generator=g, dtype=torch.float64)
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous().float().to(dev)  # noqa: E731
    xd, wd, gyd = nhwc(x), nhwc(w), nhwc(gy).view(-1, cout)
    kw = dict(bm=bm, bn=bn, splits=sp, bk=bk, stage=stage)
    ref = F.conv2d(x, w, b, padding=1).permute(0, 2, 3, 1).reshape(-1, cout)
    y, st, rows = Fn.conv_fwd(xd, wd, b.float().to(dev), stats=True, **kw)
    _close(y, ref)
    for t in range(st.shape[0]):
        seg = ref[t * rows:(t + 1) * rows]
        _close(st[t, :, 0], seg.mean(0), 1e-4)
        _close(st[t, :, 1], ((seg - seg.mean(0)) ** 2).sum(0), 1e-4)
    dx = Fn.conv_dgrad(gyd, wd, B, H, W, **kw)
    _close(dx, torch.nn.grad.conv2d_input(x.shape, w, gy, padding=1).permute(0, 2, 3, 1).reshape(-1, cin))
    dw = Fn.conv_wgrad(gyd, xd, cout, **kw)
    _close(dw, torch.nn.grad.conv2d_weight(x, w.shape, gy, padding=1).permute(0, 2, 3, 1))
