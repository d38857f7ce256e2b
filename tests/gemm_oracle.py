"""Float64 oracle, hostile operand builders and derived error bounds for the bf16 matrix-core GEMM
(csrc/kernels/gemm_bf16.hip through the bindings mm_bf16 / mm_bf16_bn_stats).

Plain helpers: nothing here needs a GPU (the builders take a `device`; the CPU tests leave it at
"cpu"). The kernel never pads: rows, columns and k outside an operand get an out-of-range buffer
offset and must land as zeros. So every operand here is a VIEW inside a parent filled with NaN
(pad columns, the rows before and after the view, the k rows past K): a single neighbour that is read
and multiplied, even by a zero, turns the output NaN.

Bounds are per element and follow from the roundings alone (docs/gemm_edge_tests.md):
bf16 x bf16 products are exact in fp32, so an fp32 sum of K of them (plus an old accumulator value
acc0) in ANY order, with any number of split-K slabs, is within (K + 1) 2^-23 (|a| @ |b| + |acc0|) of
the float64 result -- twice the first-order bound; a bf16 result adds one rounding, 2^-8 |ref|.
"""
import math

import torch

NAN = math.nan
BF16, F32 = torch.bfloat16, torch.float32
LAYOUTS = {"nt": (True, True), "nn": (True, False), "tt": (False, True), "tn": (False, False)}  # (a, b) K-major
CANARY = -24832.0  # finite, exact in bf16 (bits 0xC6C2) and fp32, far from every value the tests produce

# ------------------------------------------------------------------------------------------ the tables
# (M, N, K) with K % 8 == 0: every layout. K = 8, 16, 56: one partial K-tile; 72, 136, 200: a tail of 8
RAGGED8 = [(1, 4, 8), (15, 12, 16), (17, 60, 56), (129, 68, 72), (255, 252, 136), (257, 260, 200), (513, 4, 64),
           (1, 516, 128)]
# odd K: only "tn" (both operands M-major), where K is the token count of a weight gradient
RAGGED_ODD = [(16, 8, 1), (17, 12, 3), (129, 68, 63), (255, 252, 65), (257, 260, 67), (64, 64, 129)]
RAGGED = [(lay, s) for lay in LAYOUTS for s in RAGGED8] + [("tn", s) for s in RAGGED_ODD]
ONEHOT = [(lay, 272, 264, 200) for lay in LAYOUTS] + [("tn", 272, 264, 131)]
SPLIT = [("tn", 40, 72, 8200), ("nt", 40, 72, 8200), ("tn", 40, 72, 8197)]
SPLIT_COUNTS = [1, 2, 3, 5, 15, 16]
ACC = [(129, 68, 72), (257, 260, 200)]
STATS = [(257, 200, 72), (1, 4, 8)]


def p8(n):
    return (n + 7) // 8 * 8


def seed_of(layout, M, N, K):
    return 1000003 * list(LAYOUTS).index(layout) + 10007 * M + 101 * N + K


# -------------------------------------------------------------------------- the launcher's split rule
def kper(K, splits):
    """k per split, as cs_gemm_bf16 computes it: whole K-tiles of 64"""
    return K if splits == 1 else ((K + splits - 1) // splits + 63) // 64 * 64


def split_runs(K, splits):
    """whether cs_gemm_bf16 accepts the count: no split may be empty"""
    return splits == 1 or kper(K, splits) * (splits - 1) < K


def default_splits(M, N, K):
    """cs_gemm_bf16_splits"""
    tiles = ((M + 255) // 256) * ((N + 255) // 256)
    s = 1
    while s < 256 and tiles * s * 2 <= 512 and K // (2 * s) >= 1024 and 2 * s * M * N * 4 <= 1 << 30:
        s *= 2
    while s > 1 and not split_runs(K, s):
        s -= 1
    return s


# --------------------------------------------------------------------------------------------- builders
def values(rows, K, g):
    """[rows, K] bf16: per-row magnitudes 2^-6 .. 2^6, mean 1/4 of the row's magnitude (sums do not
    cancel to nothing, so a dropped or doubled term shows), ~6 % exact zeros of both signs"""
    x = torch.randn(rows, K, generator=g, dtype=torch.float64) + 0.25
    x = x * torch.exp2(torch.randint(-6, 7, (rows, 1), generator=g).double())
    u = torch.rand(rows, K, generator=g)
    x = torch.where(u < 0.03, torch.zeros_like(x), x)
    x = torch.where((u >= 0.03) & (u < 0.06), -torch.zeros_like(x), x)
    return x.to(BF16)


def small_ints(rows, K, g, hi=3):
    """integers in [-hi, hi] as bf16: products and short sums are exact in every format involved"""
    return torch.randint(-hi, hi + 1, (rows, K), generator=g).to(BF16)


def embed(vals, kmajor, poison=NAN, device="cpu"):
    """vals [rows, K] -> (view [rows, K], parent). K-major: parent [rows + 2, K + 8], view
    parent[1:-1, :K] (row stride K + 8, base 16-byte aligned iff K % 8 == 0). M-major: parent
    [K + 3, p8(rows) + 8], view parent[:K, :rows].t() (unit stride along rows, k stride a multiple of 8)."""
    rows, K = vals.shape
    if kmajor:
        parent = torch.full((rows + 2, K + 8), poison, dtype=BF16)
        parent[1:-1, :K] = vals
        parent = parent.to(device)
        return parent[1:-1, :K], parent
    parent = torch.full((K + 3, p8(rows) + 8), poison, dtype=BF16)
    parent[:K, :rows] = vals.t()
    parent = parent.to(device)
    return parent[:K, :rows].t(), parent


def views(M, N, K, layout, g, poison=NAN, device="cpu", full=False, make=values):
    """a [M, K] and b [K, N] in the storage `layout` names, each a view of a parent filled with
    `poison`. full=True also returns the two parents."""
    ak, bk = LAYOUTS[layout]
    a, pa = embed(make(M, K, g), ak, poison, device)
    bt, pb = embed(make(N, K, g), bk, poison, device)
    return (a, bt.t(), pa, pb) if full else (a, bt.t())


def acc_view(M, N, dtype, canary=CANARY, device="cpu"):
    """(view [M, N], parent [M + 2, N + 8]): view = parent[1:-1, 4:4 + N], the parent filled with the
    canary. N % 4 == 0 keeps the view 8-byte (bf16) / 16-byte (fp32) aligned and its row stride % 4 == 0."""
    parent = torch.full((M + 2, N + 8), canary, dtype=dtype, device=device)
    return parent[1:-1, 4:4 + N], parent


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


def canary_intact(parent, canary=CANARY):
    """every element of the parent outside acc_view's view still holds the canary's bits"""
    want = bits(torch.full((1,), canary, dtype=parent.dtype))[0].item()
    outside = torch.ones(parent.shape, dtype=torch.bool)
    outside[1:-1, 4:-4] = False
    return bool((bits(parent).cpu()[outside] == want).all())


# ----------------------------------------------------------------------------------------------- oracle
def reference(a, b, out_dtype, acc0=None):
    """(ref, bound) float64 on CPU for C = a @ b (+ acc0) stored as out_dtype"""
    ad, bd = a.detach().double().cpu(), b.detach().double().cpu()
    K = ad.shape[1]
    ref, mag = ad @ bd, ad.abs() @ bd.abs()
    if acc0 is not None:
        ref, mag = ref + acc0.double().cpu(), mag + acc0.double().cpu().abs()
    bound = (K + 1) * 2.0 ** -23 * mag
    if out_dtype == BF16:
        bound = bound + 2.0 ** -8 * ref.abs()
    return ref, bound


def ratio(got, ref, bound):
    """the worst error / bound (0 where the error is 0, inf where the bound is 0 and the error is not,
    or where the result is not finite)"""
    got = got.detach().double().cpu()
    err = (got - ref).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    r = torch.where(torch.isfinite(got), r, torch.full_like(r, math.inf))
    return float(r.max()) if r.numel() else 0.0


def inside(got, ref, bound):
    return got.shape == ref.shape and ratio(got, ref, bound) <= 1.0


MEASURED = {}  # group -> worst ratio seen in this process (printed; docs/gemm_edge_tests.md records them)


def check(got, ref, bound, name, group=None):
    """finite everywhere and per-element |got - ref| <= bound; prints and returns the worst ratio"""
    assert tuple(got.shape) == tuple(ref.shape), f"{name}: shape {tuple(got.shape)}"
    g = got.detach().double().cpu()
    assert bool(torch.isfinite(g).all()), f"{name}: {int((~torch.isfinite(g)).sum())} non-finite outputs"
    r = ratio(got, ref, bound)
    if group is not None:
        MEASURED[group] = max(MEASURED.get(group, 0.0), r)
    print(f"[gemm-edge] {name}: worst error / bound {r:.4f}")
    bad = ~((g - ref).abs() <= bound)
    assert not bad.any(), (f"{name}: {int(bad.sum())} of {bad.numel()} outside the bound, worst {r:.3g} x at "
                           f"{tuple(int(i) for i in bad.nonzero()[0])}")
    return r


# ---------------------------------------------------------------------------------------------- one-hot
def onehot_ks(K):
    """k at the edges of the 8-element chunk, the swizzle period, the 32-deep k-step and the 64-deep K-tile"""
    return sorted({k for k in (0, 7, 8, 15, 16, 31, 32, 63, 64, 65, 127, 128, K - 9, K - 8, K - 1) if 0 <= k < K})


def onehot(rows, K, ks):
    """([rows, K] bf16 with row i = 2^(i % 8 - 3) at k = ks[i % len(ks)], the k per row, the amplitudes)"""
    idx = torch.arange(rows)
    kk = torch.tensor(ks)[idx % len(ks)]
    amp = torch.exp2((idx % 8).double() - 3)
    x = torch.zeros(rows, K, dtype=torch.float64)
    x[idx, kk] = amp
    return x.to(BF16), kk, amp


def onehot_expect(kk, amp, other, out_dtype):
    """row i = amp[i] * other[:, kk[i]] for other [n, K] (the dense operand, one row per output
    column) -> [len(kk), n] in out_dtype: a power of two times a bf16 value is exact, and a zero
    comes out as +0 whatever its sign (the accumulator starts at +0 and -0 + +0 = +0)."""
    e = amp[:, None] * other.detach().double().cpu()[:, kk].t()
    out = e.to(out_dtype)
    assert bool((out.double() == e).all())
    return out + 0.0
