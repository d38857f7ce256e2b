"""The GEMM oracle of tests/gemm_oracle.py checked without a GPU: plain fp32 products of the same
values (torch.mm, and a chunked-K sum in another order) stay inside the per-element bounds at every
shape of tests/test_gemm_edges_gpu.py; each named wrong result falls outside them; the one-hot
expectation is exact with +0 zeros; the builders put NaN exactly where they claim."""
import pytest
import torch

import gemm_oracle as O

BF16, F32 = O.BF16, O.F32
SHAPES = ([(lay, *s) for lay, s in O.RAGGED] + O.ONEHOT + O.SPLIT
          + [(lay, *s) for lay in O.LAYOUTS for s in O.ACC] + [("nt", *s) for s in O.STATS])


def _gen(layout, M, N, K):
    return torch.Generator().manual_seed(O.seed_of(layout, M, N, K))


def _mm32(a, b):
    return torch.mm(a.float().contiguous(), b.float().contiguous())


def _mm32_chunked(a, b, step=64):
    """the fp32 sum of 64-deep partial products, last chunk first"""
    af, bf = a.float(), b.float()
    K = af.shape[1]
    c = torch.zeros(af.shape[0], bf.shape[1])
    for k0 in reversed(range(0, K, step)):
        c = c + torch.mm(af[:, k0:k0 + step].contiguous(), bf[k0:k0 + step].contiguous())
    return c


@pytest.fixture(scope="module")
def cases():
    """every table shape once: operands, fp32 product, both references"""
    out = {}
    for lay, M, N, K in SHAPES:
        a, b = O.views(M, N, K, lay, _gen(lay, M, N, K))
        out[(lay, M, N, K)] = (a, b, _mm32(a, b), O.reference(a, b, F32), O.reference(a, b, BF16))
    return out


def test_table_covers_what_the_issue_lists():
    assert len(O.RAGGED) == 4 * 8 + 6
    assert all(s[2] % 8 == 0 for lay, s in O.RAGGED if lay != "tn")
    assert {K for lay, (_, _, K) in O.RAGGED if lay == "tn"} >= {1, 3, 63, 65, 67, 129, 8, 16, 56}
    assert max(M * N * K for _, M, N, K in SHAPES) <= 520 * 520 * 8200


def test_fp32_products_stay_inside_the_bounds(cases):
    for key, (a, b, c32, (ref, bound), (refb, boundb)) in cases.items():
        for name, c in (("mm", c32), ("chunked", _mm32_chunked(a, b))):
            assert O.inside(c, ref, bound), (key, name, O.ratio(c, ref, bound))
            assert O.inside(c.to(BF16), refb, boundb), (key, name, "bf16", O.ratio(c.to(BF16), refb, boundb))


def test_accumulators_stay_inside_the_bounds():
    for M, N, K in O.ACC:
        g = _gen("nt", M, N, K)
        a, b = O.views(M, N, K, "nt", g)
        for dt in (F32, BF16):
            acc0 = O.values(M, N, g).to(dt)
            ref, bound = O.reference(a, b, dt, acc0)
            got = (_mm32(a, b) + acc0.float()).to(dt)
            assert O.inside(got, ref, bound), (M, N, K, dt, O.ratio(got, ref, bound))


def _fails_somewhere(cases, mutate, keys=None):
    """the mutated fp32 result is outside the fp32 bound, and its bf16 rounding outside the bf16 one,
    on at least one shape"""
    hit32 = hitb = False
    for key, (a, b, c32, (ref, bound), (refb, boundb)) in cases.items():
        if keys is not None and not keys(key):
            continue
        bad = mutate(key, a, b, c32)
        if bad is None:
            continue
        hit32 |= not O.inside(bad, ref, bound)
        hitb |= not O.inside(bad.to(BF16), refb, boundb)
    return hit32 and hitb


def test_dropped_k_chunk_in_one_row_fails(cases):
    def mutate(key, a, b, c):
        M, K = a.shape
        if K < 16:
            return None
        m, k0 = M // 2, (K // 8 - 1) * 8
        c = c.clone()
        c[m] -= a[m, k0:k0 + 8].float() @ b[k0:k0 + 8].float()
        return c
    assert _fails_somewhere(cases, mutate)


def test_swapped_k_chunks_of_b_fail(cases):
    def mutate(key, a, b, c):
        K = a.shape[1]
        if K < 16:
            return None
        bb = b.float().clone()
        bb[0:8], bb[8:16] = b[8:16].float(), b[0:8].float()
        return _mm32(a, bb)
    assert _fails_somewhere(cases, mutate)


def test_dropped_last_odd_k_fails(cases):
    def mutate(key, a, b, c):
        return _mm32(a[:, :-1], b[:-1]) if a.shape[1] > 1 else torch.zeros_like(c)
    assert _fails_somewhere(cases, mutate, keys=lambda k: k[3] % 2 == 1)


def test_swapped_rows_16_apart_fail(cases):
    def mutate(key, a, b, c):
        if c.shape[0] < 17:
            return None
        c = c.clone()
        c[[0, 16]] = c[[16, 0]]
        return c
    assert _fails_somewhere(cases, mutate)


@pytest.mark.parametrize("layout,M,N,K", [("nt", 129, 68, 72), ("tn", 129, 68, 63)])
def test_neighbour_added_in_the_k_tail_fails(layout, M, N, K):
    """the first element past K of both operands (the poison, here 1.0) joins the sum: with NaN it
    would turn every output NaN; even as a finite 1.0 the per-element bound notices"""
    a, b, pa, pb = O.views(M, N, K, layout, _gen(layout, M, N, K), poison=1.0, full=True)
    ak, bk = O.LAYOUTS[layout]
    na = pa[1:-1, K] if ak else pa[K, :M]  # a(m, K) as the kernel would address it
    nb = pb[1:-1, K] if bk else pb[K, :N]
    assert bool((na == 1).all()) and bool((nb == 1).all())
    bad = _mm32(a, b) + na.float()[:, None] * nb.float()[None, :]
    for dt in (F32, BF16):
        ref, bound = O.reference(a, b, dt)
        assert O.inside(_mm32(a, b).to(dt), ref, bound)
        assert not O.inside(bad.to(dt), ref, bound)


def test_nan_poison_reaches_the_output_through_a_zero():
    a, b = O.views(17, 12, 8, "nt", _gen("nt", 17, 12, 8))
    ref, bound = O.reference(a, b, F32)
    bad = _mm32(a, b) + torch.tensor(O.NAN) * 0.0
    assert not O.inside(bad, ref, bound)
    with pytest.raises(AssertionError, match="non-finite"):
        O.check(bad, ref, bound, "nan")


def test_one_hot_expectation_is_exact_with_positive_zeros():
    g = torch.Generator().manual_seed(3)
    K, N = 131, 24
    other = O.values(N, K, g)
    ks = O.onehot_ks(K)
    assert ks == [0, 7, 8, 15, 16, 31, 32, 63, 64, 65, 122, 123, 127, 128, 130]
    assert O.onehot_ks(200)[-3:] == [191, 192, 199]
    x, kk, amp = O.onehot(40, K, ks)
    assert int((x != 0).sum()) == 40 and bool((x.double().sum(1) == amp).all())
    for dt in (F32, BF16):
        want = O.onehot_expect(kk, amp, other, dt)
        prod = (x.double() @ other.double().t())
        assert bool((want.double() == prod).all())
        zeros = want == 0
        assert bool(zeros.any()) and not bool((O.bits(want)[zeros] != 0).any())  # every zero is +0
        # the expectation keeps the bits of a plain fp32 product of the same values
        assert torch.equal(O.bits(want), O.bits((_mm32(x, other.t()) + 0.0).to(dt)))
    assert bool(((other == 0) & (O.bits(other) != 0)).any())  # the dense operand does hold -0


@pytest.mark.parametrize("layout,M,N,K", [(lay, *s) for lay, s in O.RAGGED] + O.ONEHOT[:1] + O.SPLIT)
def test_builders_place_the_poison(layout, M, N, K):
    a, b, pa, pb = O.views(M, N, K, layout, _gen(layout, M, N, K), full=True)
    assert a.shape == (M, K) and b.shape == (K, N)
    assert bool(torch.isfinite(a.float()).all()) and bool(torch.isfinite(b.float()).all())
    for v, parent, kmajor, rows in ((a, pa, O.LAYOUTS[layout][0], M), (b.t(), pb, O.LAYOUTS[layout][1], N)):
        nan = torch.isnan(parent.float())
        if kmajor:
            assert v.stride(1) == 1 and v.stride(0) == K + 8
            assert bool(nan[0].all()) and bool(nan[-1].all()) and bool(nan[:, K:].all())  # rows around, pad columns
            assert int(nan.sum()) == parent.numel() - rows * K
        else:
            assert v.stride(0) == 1 and v.stride(1) == O.p8(rows) + 8
            assert bool(nan[K:].all()) and bool(nan[:, rows:].all())                       # k rows past K, pad columns
            assert nan[K:].shape[0] == 3 and int(nan.sum()) == parent.numel() - rows * K
        ld = v.stride(0) if kmajor else v.stride(1)
        assert ld % 8 == 0 and ld >= (K if kmajor else rows)
        assert (v.data_ptr() - parent.data_ptr()) % 16 == 0 and v.data_ptr() % 16 == 0
    # the values are the mix the bounds were derived for, not uniform [-1, 1]
    if M * K >= 2048:
        av = a.double()
        assert bool((av == 0).any()) and bool(((a == 0) & (O.bits(a) != 0)).any())
        assert float(av.abs().max()) > 16 and float(av.mean()) != 0


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_acc_view_alignment_and_canary(dtype):
    for M, N in ((129, 68), (257, 260), (40, 72)):
        v, parent = O.acc_view(M, N, dtype)
        assert v.shape == (M, N) and v.stride() == (N + 8, 1) and v.stride(0) % 4 == 0
        assert v.data_ptr() % (8 if dtype == BF16 else 16) == 0
        assert O.canary_intact(parent)
        v.copy_(torch.zeros(M, N))
        assert O.canary_intact(parent)
        for idx in ((0, 5), (M + 1, 5), (3, 3), (3, N + 4), (M, N + 7)):
            p2 = parent.clone()
            p2[idx] = 0.0
            assert not O.canary_intact(p2)
    assert float(torch.tensor(O.CANARY).to(BF16)) == O.CANARY


def test_split_rule_mirrors_the_launcher():
    assert [O.kper(8200, s) for s in O.SPLIT_COUNTS] == [8200, 4160, 2752, 1664, 576, 576]
    assert [O.split_runs(8200, s) for s in O.SPLIT_COUNTS] == [True, True, True, True, True, False]
    assert [O.split_runs(8197, s) for s in O.SPLIT_COUNTS] == [True, True, True, True, True, False]
    # K = 136: three splits are 64 + 64 + 8, none empty; four would leave the last one empty
    assert O.split_runs(136, 3) and not O.split_runs(136, 4) and not O.split_runs(128, 3)
    assert O.default_splits(40, 72, 8200) == 8 and O.default_splits(40, 72, 8197) == 8
    assert O.default_splits(257, 260, 200) == 1
