"""Edge tests of the bf16 matrix-core GEMM (csrc/kernels/gemm_bf16.hip) on an MI355X: odd and tiny K,
M and N below and just past a tile, operands inside NaN-filled parents, the accumulator modes behind
a canary, split-K, the BatchNorm-statistics epilogue, and the dispatch that decides whether a product
of the LM path reaches the kernel at all. Oracle, builders and bounds: tests/gemm_oracle.py (checked
on CPU by tests/test_gemm_oracles_cpu.py); which branch each case enters and the measured
error / bound ratios: docs/gemm_edge_tests.md.

Which calls reach the kernel. Groups 1-5 call the bindings `mm_bf16` / `mm_bf16_bn_stats` directly.
The bindings have no other path: they launch `gemm_kernel` or raise, and never call torch.mm. Every
operand of groups 1-5 is a view inside a parent filled with NaN (`gemm_oracle.views`), and every result
is required to be finite: a kernel that read one neighbour and let it into a stored sum would fail.
The accumulator tests also pin the in-place write (data_ptr, strides, canary bits around the view).
Groups 6 and 7 go through `lm._mm`, which may choose
torch.mm: there the `spy` fixture wraps both `mm_bf16` and `torch.mm` and every test asserts the
counts -- a group-6 pair with `gemm_operands_ok` true ran `mm_bf16` once and torch.mm never, one with
it false ran torch.mm once and `mm_bf16` never (and the binding called directly raises)."""
import pytest
import torch

import gemm_oracle as O
import nhwc_oracle as NO

pytestmark = pytest.mark.gpu

BF16, F32 = O.BF16, O.F32
DEV = "cuda"


@pytest.fixture(scope="module")
def C():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cs744_pytorch_distributed_tutorial_amd.ops import native
    yield native.C()
    print("\n[gemm-edge] worst error / bound per group: "
          + ", ".join(f"{k} {v:.4f}" for k, v in sorted(O.MEASURED.items())))


def _gen(layout, M, N, K):
    return torch.Generator().manual_seed(O.seed_of(layout, M, N, K))


def _bit_equal(x, y):
    return x.dtype == y.dtype and x.shape == y.shape and torch.equal(O.bits(x).cpu(), O.bits(y).cpu())


# ------------------------------------------------------------------------------- 1. ragged shapes
@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("layout,shape", O.RAGGED, ids=[f"{lay}-{'x'.join(map(str, s))}" for lay, s in O.RAGGED])
def test_ragged_shapes_in_poisoned_parents(C, layout, shape, dt):
    M, N, K = shape
    a, b = O.views(M, N, K, layout, _gen(layout, M, N, K), device=DEV)
    c = C.mm_bf16(a, b, dt == F32)
    assert c.dtype == dt and c.is_contiguous()
    ref, bound = O.reference(a, b, dt)
    O.check(c, ref, bound, f"ragged {layout} {shape} {dt}", group="1 ragged")


# ------------------------------------------------------------------------------------- 2. one-hot
@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("layout,M,N,K", O.ONEHOT, ids=[f"{c[0]}-K{c[3]}" for c in O.ONEHOT])
def test_one_hot_rows_and_columns_are_exact(C, layout, M, N, K, dt):
    """A row i = 2^(i % 8 - 3) at k = ks[i]: C[i] = that amplitude times B[ks[i], :], bit for bit, zeros
    +0 (B holds -0: the accumulator starts at +0 and -0 + +0 = +0). Then the mirror, B one-hot
    columns. Rows and columns run past the first wave tile (128 x 64) into a second workgroup tile."""
    ak, bk = O.LAYOUTS[layout]
    g = _gen(layout, M, N, K)
    ks = O.onehot_ks(K)
    for hot_a in (True, False):
        hot, kk, amp = O.onehot(M if hot_a else N, K, ks)
        dense = O.values(N if hot_a else M, K, g)
        av, bv = (hot, dense) if hot_a else (dense, hot)
        a, _ = O.embed(av, ak, device=DEV)
        bt, _ = O.embed(bv, bk, device=DEV)
        c = C.mm_bf16(a, bt.t(), dt == F32)
        want = O.onehot_expect(kk, amp, dense, dt)
        want = want if hot_a else want.t()
        assert bool(torch.isfinite(c).all())
        assert not bool(((c == 0) & (O.bits(c) != 0)).any()), "a zero came out as -0"
        same = O.bits(c).cpu() == O.bits(want)
        assert bool(same.all()), (f"{layout} K={K} {'A' if hot_a else 'B'} one-hot: {int((~same).sum())} wrong, first at "
                                  f"{tuple(int(i) for i in (~same).nonzero()[0])}")


# ------------------------------------------------------------------------------------- 3. split-K
@pytest.mark.parametrize("layout,M,N,K", O.SPLIT, ids=[f"{c[0]}-K{c[3]}" for c in O.SPLIT])
def test_split_k_counts(C, layout, M, N, K):
    """every listed count that leaves no split empty is within the one bound (it holds for any
    summation order, so for any slab count); a count that leaves one empty raises: at these K that is
    16 (kper = 576, 15 x 576 >= K), by the launcher's own rule kper x (splits - 1) < K"""
    a, b = O.views(M, N, K, layout, _gen(layout, M, N, K), device=DEV)
    ref, bound = O.reference(a, b, F32)
    for S in O.SPLIT_COUNTS:
        if O.split_runs(K, S):
            O.check(C.mm_bf16(a, b, True, splits=S), ref, bound, f"split {layout} K={K} S={S}", group="3 split-K")
        else:
            with pytest.raises(RuntimeError):
                C.mm_bf16(a, b, True, splits=S)
    auto = C.mm_bf16(a, b, True)
    O.check(auto, ref, bound, f"split {layout} K={K} auto", group="3 split-K")
    assert _bit_equal(auto, C.mm_bf16(a, b, True))
    assert _bit_equal(auto, C.mm_bf16(a, b, True, splits=O.default_splits(M, N, K)))


@pytest.mark.parametrize("layout,M,N,K", O.SPLIT, ids=[f"{c[0]}-K{c[3]}" for c in O.SPLIT])
def test_split_k_one_hot_at_the_split_edges(C, layout, M, N, K):
    """the last k of split 0, the first of split 1 and the last of all: exact for every split count"""
    ak, bk = O.LAYOUTS[layout]
    dense = O.values(N, K, _gen(layout, M, N, K))
    bt, _ = O.embed(dense, bk, device=DEV)
    for S in [s for s in O.SPLIT_COUNTS if O.split_runs(K, s)] + [-1]:
        kper = O.kper(K, S if S > 0 else O.default_splits(M, N, K))
        ks = sorted({k for k in (kper - 1, kper, K - 1) if k < K})
        hot, kk, amp = O.onehot(M, K, ks)
        a, _ = O.embed(hot, ak, device=DEV)
        c = C.mm_bf16(a, bt.t(), True, splits=S)
        assert _bit_equal(c, O.onehot_expect(kk, amp, dense, F32)), (S, ks)


def test_empty_split_raises(C):
    """K = 136: splits = 3 is 64 + 64 + 8 (kper = 64, 2 x 64 < 136) and runs; splits = 4 would leave
    the fourth split empty (3 x 64 >= 136), as splits = 3 does at K = 128: those must raise, not return"""
    M, N = 40, 72
    for K, S, runs in ((136, 3, True), (136, 4, False), (128, 3, False), (128, 2, True)):
        assert O.split_runs(K, S) == runs
        a, b = O.views(M, N, K, "tn", _gen("tn", M, N, K), device=DEV)
        if runs:
            O.check(C.mm_bf16(a, b, True, splits=S), *O.reference(a, b, F32), f"K={K} S={S}", group="3 split-K")
        else:
            with pytest.raises(RuntimeError):
                C.mm_bf16(a, b, True, splits=S)
            acc = torch.zeros(M, N, device=DEV)
            with pytest.raises(RuntimeError):
                C.mm_bf16(a, b, acc=acc, splits=S)
            assert not bool(acc.any())
    with pytest.raises(RuntimeError):  # the binding's own range, 1 .. 256
        C.mm_bf16(a, b, True, splits=257)


@pytest.mark.parametrize("strided", [False, True], ids=["contiguous", "strided"])
@pytest.mark.parametrize("layout,M,N,K", O.SPLIT, ids=[f"{c[0]}-K{c[3]}" for c in O.SPLIT])
def test_split_k_into_an_fp32_accumulator(C, layout, M, N, K, strided):
    """acc += a @ b over slabs: a contiguous acc is summed in place, a strided one (ldc = N + 8)
    through the binding's sum-then-copy branch; nothing outside the view changes"""
    g = _gen(layout, M, N, K)
    a, b = O.views(M, N, K, layout, g, device=DEV)
    acc0 = O.values(M, N, g).float()
    for S in (3, -1):
        if strided:
            acc, parent = O.acc_view(M, N, F32, device=DEV)
            acc.copy_(acc0)
            assert not acc.is_contiguous()
        else:
            acc, parent = acc0.to(DEV), None
        out = C.mm_bf16(a, b, acc=acc, splits=S)
        assert out.data_ptr() == acc.data_ptr() and out.stride() == acc.stride()
        ref, bound = O.reference(a, b, F32, acc0)
        O.check(acc, ref, bound, f"split acc {layout} K={K} S={S} strided={strided}", group="3 split-K")
        assert parent is None or O.canary_intact(parent)


# ----------------------------------------------------------------------- 4. accumulators, unsplit
@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("layout", list(O.LAYOUTS))
@pytest.mark.parametrize("M,N,K", O.ACC)
def test_accumulate_into_a_strided_view(C, M, N, K, layout, dt):
    assert O.default_splits(M, N, K) == 1
    g = _gen(layout, M, N, K)
    a, b = O.views(M, N, K, layout, g, device=DEV)
    acc0 = O.values(M, N, g).to(dt)
    acc, parent = O.acc_view(M, N, dt, device=DEV)
    acc.copy_(acc0)
    out = C.mm_bf16(a, b, acc=acc)
    assert out.data_ptr() == acc.data_ptr() and out.dtype == dt and out.stride() == (N + 8, 1)
    ref, bound = O.reference(a, b, dt, acc0)
    O.check(acc, ref, bound, f"acc {layout} {(M, N, K)} {dt}", group="4 accumulate")
    assert O.canary_intact(parent), "a store left the view"


@pytest.mark.parametrize("layout", list(O.LAYOUTS))
def test_bf16_accumulator_plus_zero_keeps_its_bits(C, layout):
    """a = 0: every product is 0 and old + 0 rounds back to old, bit for bit -- except an old -0,
    because the sum is formed in fp32 as (+0) + (-0) = +0"""
    M, N, K = O.ACC[0]
    g = _gen(layout, M, N, K)
    a, b = O.views(M, N, K, layout, g, device=DEV)
    a.zero_()  # the view alone: its parent stays NaN
    acc0 = O.values(M, N, g)
    assert bool(((acc0 == 0) & (O.bits(acc0) != 0)).any())
    acc, parent = O.acc_view(M, N, BF16, device=DEV)
    acc.copy_(acc0)
    C.mm_bf16(a, b, acc=acc)
    assert _bit_equal(acc.contiguous(), acc0 + 0.0)
    assert O.canary_intact(parent)


@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("layout", list(O.LAYOUTS))
def test_accumulator_exact_on_small_integers(C, layout, dt):
    """operands in {-1, 0, 1}, old values in [-3, 3], K = 72: |result| <= 75 is an integer below 256,
    exact in bf16, so the one rounding changes nothing"""
    M, N, K = O.ACC[0]
    g = _gen(layout, M, N, K)
    a, b = O.views(M, N, K, layout, g, device=DEV, make=lambda r, k, g: O.small_ints(r, k, g, 1))
    acc0 = O.small_ints(M, N, g, 3).to(dt)
    acc, parent = O.acc_view(M, N, dt, device=DEV)
    acc.copy_(acc0)
    C.mm_bf16(a, b, acc=acc)
    want = a.double().cpu() @ b.double().cpu() + acc0.double()
    assert float(want.abs().max()) <= 75
    assert bool((acc.double().cpu() == want).all())
    assert O.canary_intact(parent)


# ---------------------------------------------------------------------------- 5. mm_bf16_bn_stats
@pytest.mark.parametrize("M,N,K", O.STATS)
def test_bn_stats_epilogue_on_a_poisoned_operand(C, M, N, K):
    a, b = O.views(M, N, K, "nt", _gen("nt", M, N, K), device=DEV)
    assert a.stride(0) == K + 8
    y, tiles = C.mm_bf16_bn_stats(a, b)
    assert _bit_equal(y, C.mm_bf16(a, b))
    O.check(y, *O.reference(a, b, BF16), f"bn_stats y {(M, N, K)}", group="5 bn_stats y")
    assert tiles.shape == ((M + 255) // 256, N, 2) and bool(torch.isfinite(tiles).all())
    mean, e_mean, M2, e_M2 = NO.gemm_tile_stats(y.cpu())
    r1 = NO.check(tiles[..., 0], mean, e_mean, f"gemm tile mean {(M, N, K)}")
    r2 = NO.check(tiles[..., 1], M2, e_M2, f"gemm tile M2 {(M, N, K)}")
    O.MEASURED["5 bn_stats tiles"] = max(O.MEASURED.get("5 bn_stats tiles", 0.0), r1, r2)


# -------------------------------------------------------------------------- 6. dispatch agreement
def _padded(vals, ld):
    """[rows, cols] as a view of a contiguous [rows, ld]"""
    p = torch.zeros(vals.shape[0], ld, dtype=vals.dtype)
    p[:, :vals.shape[1]] = vals
    return p.to(DEV)[:, :vals.shape[1]]


def _off_base(vals, elems):
    """contiguous, its base `elems` elements past a 16-byte boundary"""
    flat = torch.zeros(vals.numel() + elems, dtype=vals.dtype, device=DEV)
    v = flat[elems:].view(vals.shape)
    v.copy_(vals)
    return v


def _pairs():
    """name -> (a [M, K], b [K, N], gemm_operands_ok as cs_gemm_bf16's rules give it)"""
    g = torch.Generator().manual_seed(66)
    v = O.values
    out = {}
    for lay in O.LAYOUTS:                                   # every layout, poisoned parents
        out[f"{lay} 17x12x16"] = (*O.views(17, 12, 16, lay, g, device=DEV), True)
    out["tn odd K 17x12x3"] = (*O.views(17, 12, 3, "tn", g, device=DEV), True)
    out["tn K=1"] = (*O.views(16, 8, 1, "tn", g, device=DEV), True)
    for lay in ("nt", "nn", "tt"):                          # K % 8 != 0 with aligned rows (ld = 16)
        ak, bk = O.LAYOUTS[lay]
        a = _padded(v(16, 12, g), 16) if ak else _padded(v(12, 16, g), 16).t()
        b = _padded(v(8, 12, g), 16).t() if bk else _padded(v(12, 8, g), 16)
        out[f"{lay} K=12"] = (a, b, False)
    out["tn K=12"] = (_padded(v(12, 16, g), 16).t(), _padded(v(12, 8, g), 16), True)
    out["a K-major ld=12"] = (_padded(v(16, 8, g), 12), v(8, 8, g).to(DEV), False)
    out["a M-major ld=20"] = (_padded(v(8, 17, g), 20).t(), v(8, 8, g).to(DEV), False)
    out["b N-major ld=12"] = (v(16, 8, g).to(DEV), _padded(v(8, 8, g), 12), False)
    out["a base +8 bytes"] = (_off_base(v(16, 16, g), 4), v(16, 8, g).to(DEV), False)
    out["b base +2 bytes"] = (v(16, 16, g).to(DEV), _off_base(v(16, 8, g), 1), False)
    out["N=10 ld=16"] = (v(16, 16, g).to(DEV), _padded(v(16, 10, g), 16), False)
    out["N=12 contiguous"] = (v(16, 16, g).to(DEV), v(16, 12, g).to(DEV), False)  # ldb = 12
    out["a expanded row"] = (v(1, 16, g).to(DEV).expand(16, 16), v(16, 8, g).to(DEV), False)
    out["a expanded column"] = (v(16, 1, g).to(DEV).expand(16, 16), v(16, 8, g).to(DEV), False)
    out["a expanded scalar"] = (v(1, 1, g).to(DEV).expand(16, 16), v(16, 8, g).to(DEV), False)
    out["b no unit stride"] = (v(16, 16, g).to(DEV), v(16, 16, g).to(DEV).view(16, 8, 2)[:, :, 0], False)
    out["fp32 operands"] = (v(16, 16, g).float().to(DEV), v(16, 8, g).float().to(DEV), False)
    out["fp32 b"] = (v(16, 16, g).to(DEV), v(16, 8, g).float().to(DEV), False)
    out["empty K"] = (torch.zeros(16, 0, dtype=BF16, device=DEV), torch.zeros(0, 8, dtype=BF16, device=DEV), True)
    out["empty M"] = (torch.zeros(0, 16, dtype=BF16, device=DEV), v(16, 8, g).to(DEV), True)
    return out


PAIR_NAMES = ["nt 17x12x16", "nn 17x12x16", "tt 17x12x16", "tn 17x12x16", "tn odd K 17x12x3", "tn K=1", "nt K=12",
              "nn K=12", "tt K=12", "tn K=12", "a K-major ld=12", "a M-major ld=20", "b N-major ld=12", "a base +8 bytes",
              "b base +2 bytes", "N=10 ld=16", "N=12 contiguous", "a expanded row", "a expanded column",
              "a expanded scalar", "b no unit stride", "fp32 operands", "fp32 b", "empty K", "empty M"]


@pytest.fixture(scope="module")
def pairs(C):
    p = _pairs()
    assert list(p) == PAIR_NAMES
    return p


@pytest.fixture
def spy(C, monkeypatch):
    """counts of the calls that reach the kernel binding and of those that reach torch.mm"""
    from cs744_pytorch_distributed_tutorial_amd.ops import lm
    calls = {"kernel": 0, "torch": 0}
    kernel, mm = C.mm_bf16, torch.mm

    def spy_kernel(*a, **kw):
        calls["kernel"] += 1
        return kernel(*a, **kw)

    def spy_mm(*a, **kw):
        calls["torch"] += 1
        return mm(*a, **kw)
    monkeypatch.setattr(C, "mm_bf16", spy_kernel)
    monkeypatch.setattr(torch, "mm", spy_mm)
    calls["lm"], calls["raw"] = lm, kernel
    return calls


@pytest.mark.parametrize("name", PAIR_NAMES)
def test_dispatch_agrees_with_the_binding(C, pairs, spy, name, monkeypatch):
    lm, raw = spy["lm"], spy["raw"]
    a, b, expect_ok = pairs[name]
    ok = lm.gemm_operands_ok(a, b)
    assert ok == expect_ok
    mixed = a.dtype != b.dtype
    if ok:
        for f32 in (False, True):
            c = raw(a, b, f32)
            O.check(c, *O.reference(a, b, c.dtype), f"dispatch {name} f32={f32}", group="6 dispatch")
    else:
        with pytest.raises(RuntimeError):
            raw(a, b)
        with pytest.raises(RuntimeError):
            raw(a, b, True)
    if mixed:
        return  # torch.mm refuses mixed dtypes too: nothing for _mm to fall back to
    monkeypatch.setattr(lm, "_GEMM", "native")
    for f32 in (False, True):
        if f32 and a.dtype == F32:
            continue  # torch.mm's out_dtype is for bf16 operands
        before = dict(kernel=spy["kernel"], torch=spy["torch"])
        c = lm._mm(a, b, f32)
        assert (spy["kernel"] - before["kernel"], spy["torch"] - before["torch"]) == ((1, 0) if ok else (0, 1))
        assert c.dtype == (F32 if f32 or a.dtype == F32 else BF16)
        O.check(c, *O.reference(a, b, c.dtype), f"_mm {name} f32={f32}", group="6 dispatch")


# ------------------------------------------------------------------------------ 7. ShadowLinear
# out = 136: every leading dimension and K-major K is a multiple of 8, so all three products pass
# cs_gemm_bf16's checks. out = 132: dx = dy W has a K-major K of 132 and dW = dy^T x reads dy^T with
# a row stride of 132, neither a multiple of 8: the launcher refuses both, only y = x W^T can run.
@pytest.mark.parametrize("T", [37, 1])
@pytest.mark.parametrize("out,mode,reached", [(136, "native", 3), (136, "wgrad", 1), (132, "native", 1),
                                              (132, "wgrad", 0)])
def test_shadow_linear_products(C, spy, monkeypatch, out, mode, reached, T):
    """y, dx (bf16) and dW (fp32) of a ShadowLinear under bf16 autocast against float64 on the bf16
    shadow and activations. dW's reduction is the token count: T = 37 runs the M-major K tail (rows =
    37 of a 64-deep K-tile), T = 1 a single k row."""
    lm = spy["lm"]
    monkeypatch.setattr(lm, "_GEMM", mode)
    g = torch.Generator().manual_seed(7 * T + out)
    lin = lm.ShadowLinear(72, out, bias=False).to(DEV)
    with torch.no_grad():
        lin.weight.copy_(O.values(out, 72, g).float())
    x = O.values(T, 72, g).to(DEV).requires_grad_()
    gy = O.values(T, out, g).to(DEV)
    with torch.autocast("cuda", dtype=BF16):
        y = lin(x)
    y.backward(gy)
    assert spy["kernel"] == reached and spy["kernel"] + spy["torch"] == 3
    w = lin.weight.detach().to(BF16)
    assert y.dtype == BF16 and x.grad.dtype == BF16 and lin.weight.grad.dtype == F32
    grp = "7 ShadowLinear"
    O.check(y, *O.reference(x.detach(), w.t(), BF16), f"shadow y out={out} {mode} T={T}", group=grp)
    O.check(x.grad, *O.reference(gy, w, BF16), f"shadow dx out={out} {mode} T={T}", group=grp)
    O.check(lin.weight.grad, *O.reference(gy.t(), x.detach(), F32), f"shadow dW out={out} {mode} T={T}", group=grp)
