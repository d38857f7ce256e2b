"""CPU checks of tests/bn_oracle.py: the float64 oracles agree with float64 ATen autograd, an fp32
evaluation of the same formulas stays inside every derived bound on every input builder the GPU
tests use, and the variance bound still rejects a one-pass E[x^2] - E[x]^2 (docs/bn_edge_tests.md)."""
import pytest
import torch
import torch.nn.functional as F

import bn_oracle as O

f32 = torch.float32


# ------------------------------------------------------------------ fp32 evaluation of the same formulas
def _chan32(n, m, M2, nb, mb, M2b):
    nn = n + nb
    d = mb - m
    safe = nn.clamp_min(1.0)
    m_c = m + d * (nb / safe)
    M2_c = M2 + M2b + d * d * (n * nb / safe)
    keep, take = nb == 0, n == 0
    pick = lambda a, b, c: torch.where(keep, a, torch.where(take, b, c))  # noqa: E731
    return pick(n, nb, nn), pick(m, mb, m_c), pick(M2, M2b, M2_c)


def fwd_fp32(st, R, M, gamma, beta, rm, rv, momentum, eps):
    """bn_finalize_kernel's order in torch fp32: lane l combines tiles l, l + 64, ..., then the
    6-step butterfly; finalize_store's arithmetic."""
    T, C = st.shape[0], st.shape[1]
    n, m, M2 = (torch.zeros(64, C, dtype=f32) for _ in range(3))
    lane = torch.arange(64)
    for s in range((T + 63) // 64):
        t = s * 64 + lane
        ok = t < T
        tc = t.clamp_max(T - 1)
        cnt = torch.where(ok, (M - tc * R).clamp_max(R), torch.zeros_like(tc)).to(f32)[:, None].expand(64, C)
        n, m, M2 = _chan32(n, m, M2, cnt, st[tc, :, 0], st[tc, :, 1])
    for off in (32, 16, 8, 4, 2, 1):
        idx = lane ^ off
        n, m, M2 = _chan32(n, m, M2, n[idx], m[idx], M2[idx])
    n, m, M2 = n[0], m[0], M2[0]
    mom, eps = torch.tensor(momentum, dtype=f32), torch.tensor(eps, dtype=f32)
    var = M2 / n
    inv = 1.0 / torch.sqrt(var + eps)
    unb = torch.where(n > 1, M2 / (n - 1).clamp_min(1.0), var)
    return dict(mean=m, var=var, invstd=inv, scale=gamma * inv, shift=beta - m * gamma * inv,
                running_mean=(1 - mom) * rm + mom * m, running_var=(1 - mom) * rv + mom * unb)


FWD, _build = O.FWD_CASES, O.build


@pytest.mark.parametrize("name,builder,shape,R", FWD, ids=[c[0] for c in FWD])
@pytest.mark.parametrize("momentum,eps", [(0.1, 1e-5), (0.3, 1e-3), (1.0, 1e-5), (0.0, 1e-2)])
def test_fp32_forward_is_inside_the_bounds(name, builder, shape, R, momentum, eps):
    y, gamma, beta = _build(builder, shape)
    C = y.shape[-1]
    M = y.numel() // C
    st = O.tile_partials(y, R)
    rm, rv = torch.linspace(-1, 1, C), torch.linspace(0.5, 2, C)
    o = O.fwd_oracle(st, R, M, gamma, beta, rm, rv, momentum, eps)
    e = fwd_fp32(st, R, M, gamma, beta, rm, rv, momentum, eps)
    for k in ("mean", "var", "invstd", "scale", "shift", "running_mean", "running_var"):
        O.check(e[k], o[k], o["e_" + k], f"{name} {k}")
    for pool in (False, True):
        if pool and (shape[1] % 2 or shape[2] % 2):
            continue
        ref, bound = O.apply_oracle(y, o, gamma, pool)
        out = (y * e["scale"] + e["shift"]).clamp_min(0.0)
        O.check(O.pool_max(out) if pool else out, ref, bound, f"{name} out pool={pool}")


def test_m1_takes_the_biased_variance():
    y, gamma, beta = O.ordinary(1, 1, 1, 16)
    o = O.fwd_oracle(O.tile_partials(y, 1), 1, 1, gamma, beta, torch.zeros(16), torch.ones(16), 0.5, 1e-5)
    assert torch.equal(o["var"], torch.zeros(16, dtype=torch.float64))
    assert torch.equal(o["unbiased"], o["var"])  # n > 1 ? M2 / (n - 1) : var
    assert torch.equal(o["running_var"], torch.full((16,), 0.5, dtype=torch.float64))
    out, bound = O.apply_oracle(y, o, gamma, False)  # xhat = 0: the output is relu(beta)
    assert ((out.reshape(16) - beta.double().clamp_min(0)).abs() <= bound.reshape(16)).all()


@pytest.mark.parametrize("shape,R", [((2, 8, 8), 16), ((2, 8, 8), 7), ((4, 32, 32), 8)])
def test_variance_bound_rejects_one_pass_fp32(shape, R):
    """E[x^2] - E[x]^2 accumulated in fp32 leaves the variance bound on every ladder channel whose
    mean / std is 1e3 or more (and the constant channel's M2 = 0 is lost), while the Chan combine
    (test above) stays inside: the bound discriminates."""
    y, gamma, beta = O.ladder(*shape)
    M = y.numel() // 16
    o = O.fwd_oracle(O.tile_partials(y, R), R, M, gamma, beta)
    y2 = y.reshape(M, 16)
    s = torch.zeros(16, dtype=f32)
    q = torch.zeros(16, dtype=f32)
    for r in range(0, M, 64):  # fp32 partial sums, in row order
        s = s + y2[r:r + 64].sum(0)
        q = q + (y2[r:r + 64] * y2[r:r + 64]).sum(0)
    one = q / M - (s / M) * (s / M)
    # |mean| / std = 1e3, 3e3, 1e3, 1e5, 3e4, 1e4. Left out: channel 5 (1e6: the std is 16 ulps of the
    # mean, and with 512 tiles the rounding of the running mean alone exceeds the spread, so the bound
    # exceeds the variance) and the constant channel 15, where both methods are exact.
    hard = torch.tensor([1, 3, 10, 11, 12, 14])
    outside = (one.double() - o["var"]).abs() > o["e_var"]
    assert outside[hard].all(), (one, o["var"], o["e_var"])
    # and the bound is no blank cheque: below 5% of the variance wherever |mean| / std <= 1e4
    soft = torch.tensor([0, 1, 2, 3, 4, 6, 7, 8, 9, 10, 13, 14])
    assert (o["e_var"][soft] < 0.05 * o["var"][soft]).all(), (o["e_var"], o["var"])
    assert float(o["var"][15]) == 0.0


# ------------------------------------------------------------------ the oracle against float64 ATen
def _aten(y, gamma, beta, G, pool, eps=1e-5, momentum=0.1):
    yn = y.double().permute(0, 3, 1, 2).contiguous().requires_grad_()
    g, b = gamma.double().requires_grad_(), beta.double().requires_grad_()
    C = y.shape[-1]
    rm, rv = torch.full((C,), 0.25, dtype=torch.float64), torch.full((C,), 2.0, dtype=torch.float64)
    z = F.relu(F.batch_norm(yn, rm, rv, g, b, training=True, momentum=momentum, eps=eps))
    if pool:
        z = F.max_pool2d(z, 2, 2)
    z.backward(G.double().permute(0, 3, 1, 2))
    return z.detach().permute(0, 2, 3, 1), yn.grad.permute(0, 2, 3, 1).reshape(-1, C), g.grad, b.grad, rm, rv


def _rel_close(a, b, tol=1e-6):
    # the only fp32 roundings on the oracle's side are the tile partials' (2^-24 of values of order 1 to 10)
    a, b = a.double().reshape(b.shape), b.double()
    assert ((a - b).abs() <= tol * (b.abs() + 1.0)).all(), float(((a - b).abs() / (b.abs() + 1.0)).max())


ATEN_SHAPES = [(2, 4, 4, 16), (3, 2, 8, 16), (2, 8, 2, 16), (1, 2, 2, 4), (2, 4, 4, 12)]
ATEN = [(s, p, None) for s in ATEN_SHAPES for p in (False, True)]
ATEN += [(s, True, t) for s in ATEN_SHAPES for t in ("pos01", "pos12", "pos23", "pos03", "pos0123")]


@pytest.mark.parametrize("shape,pool,ties", ATEN)
def test_oracle_matches_float64_aten(shape, pool, ties):
    B, H, W, C = shape
    y, gamma, beta = O.ordinary(B, H, W, C)
    if ties is not None:
        y = O.tie_case(ties, B, H, W, C)["y"] * 0.5 + 0.25
        gamma = gamma.abs()  # equal y -> equal positive-side z
        beta = beta.abs() + 0.5
    G = O.grad_like(B, H, W, C, pool)
    z, dy, dg, db, rm, rv = _aten(y, gamma, beta, G, pool, eps=1e-3, momentum=0.3)
    M = B * H * W
    st = O.tile_partials(y, 3)
    o = O.fwd_oracle(st, 3, M, gamma, beta, torch.full((C,), 0.25), torch.full((C,), 2.0), 0.3, 1e-3)
    out, _ = O.apply_oracle(y, o, gamma, pool)
    _rel_close(out, z)
    _rel_close(o["running_mean"], rm)
    _rel_close(o["running_var"], rv)
    # backward from the float64 coefficients
    b = O.bwd_oracle(y, G, o["scale"], o["shift"], o["mean"], o["invstd"], gamma, pool)
    _rel_close(b["dz"], dy, 1e-5)
    _rel_close(b["dgamma"], dg, 1e-5)
    _rel_close(b["dbeta"], db, 1e-5)
    assert (b["dbias"].abs() <= 1e-5 * (db.abs() + 1)).all()  # BN removes the conv bias
    if ties is not None:  # the routing took the first of the equal maxima
        first = int(ties[3])
        w = O._windows(b["sel"])
        tied = O._windows(y)[..., first] == 1.75  # 3.0 * 0.5 + 0.25
        assert tied.all() and w[..., first][tied].all()


# ------------------------------------------------------------------ fp32 backward inside the bounds
BWD = O.BWD_CASES


def _bwd_fp32(y, G, sel, scale, shift, mean, invstd, gamma, pool, rows):
    C = y.shape[-1]
    M = y.numel() // C
    Gf = G.repeat_interleave(2, 1).repeat_interleave(2, 2) if pool else G
    g = Gf * sel
    xh = (y - mean) * invstd
    t = torch.stack([g, g * xh, xh], 0).reshape(3, M, C)
    s = t.sum(1)
    k1, k2, k3 = gamma * invstd, s[0] / M, s[1] / M
    dz = (k1 * (g - k2 - xh * k3)).reshape(M, C)
    tiles = None
    if rows is not None:
        per = O._windows(t.reshape(-1, *y.shape[1:])).sum(-1).reshape(3, -1, C) if pool else t
        Mg = per.shape[1]
        T = (Mg + rows - 1) // rows
        per = torch.cat([per, torch.zeros(3, T * rows - Mg, C)], 1)
        tiles = per.view(3, T, rows, C).sum(2).permute(1, 2, 0)
    return s, torch.stack([k1, k2, k3], 1), -k1 * k3 * s[2], dz, tiles


@pytest.mark.parametrize("shape,pool", BWD)
def test_fp32_backward_is_inside_the_bounds(shape, pool):
    B, H, W, C = shape
    y, gamma, beta = O.ordinary(B, H, W, C)
    G = O.grad_like(B, H, W, C, pool)
    sc, sh, mu, inv = O.coeffs_from(y, gamma, beta)
    o = O.bwd_oracle(y, G, sc, sh, mu, inv, gamma, pool, rows=16)
    s, coef, dbias, dz, tiles = _bwd_fp32(y, G, o["sel"], sc, sh, mu, inv, gamma, pool, 16)
    O.check(s, o["sums"], o["e_sums"], "sums")
    O.check(coef, o["coef"], o["e_coef"], "coef")
    O.check(dbias, o["dbias"], o["e_dbias"], "dbias")
    O.check(dz, o["dz"], o["e_dz"], "dz")
    O.check(tiles, o["tile_sums"], o["e_tile_sums"], "tile sums")
    # the tails' bound from the fp32 tile partials
    t = O.tail_oracle(tiles, B * H * W, gamma, inv)
    O.check(tiles.sum(0)[:, 1], t["dgamma"], t["e_dgamma"], "tail dgamma")
    O.check(tiles.sum(0)[:, 0], t["dbeta"], t["e_dbeta"], "tail dbeta")


@pytest.mark.parametrize("kind", ["pos01", "pos12", "pos23", "pos03", "pos0123", "zero", "negscale", "scale0"])
def test_decision_cases(kind):
    d = O.tie_case(kind)
    o = O.bwd_oracle(d["y"], d["G"], d["scale"], d["shift"], d["mean"], d["invstd"], d["gamma"], True, rows=16)
    w = O._windows(o["sel"])  # [B, Ho, Wo, C, 4]
    assert (w.sum(-1) <= 1).all()
    if kind.startswith("pos"):
        first = int(kind[3])
        assert w[..., first].all() and int(w.sum()) == w[..., 0].numel()
    elif kind == "zero":
        assert not w.any()  # z = 0 is not > 0: nothing routed
        assert torch.equal(o["dbeta"], torch.zeros(16, dtype=torch.float64))
    elif kind == "scale0":
        assert w[..., 0].all() and not w[..., 1:].any()
        assert float(o["dz"].abs().max()) == 0.0 and float(o["dgamma"].abs().max()) > 0.0
    else:  # negative scale: the routed element is the window's smallest y
        yw = O._windows(d["y"])
        z, _ = O.decisions(d["y"], d["scale"], d["shift"], True)
        routed = w.any(-1)
        assert routed.any()
        assert (yw[w] == yw.amin(-1)[routed]).all()
    s, coef, dbias, dz, tiles = _bwd_fp32(d["y"], d["G"], o["sel"], d["scale"], d["shift"], d["mean"], d["invstd"],
                                          d["gamma"], True, 16)
    O.check(s, o["sums"], o["e_sums"], "sums")
    O.check(dz, o["dz"], o["e_dz"], "dz")
    O.check(tiles, o["tile_sums"], o["e_tile_sums"], "tile sums")
