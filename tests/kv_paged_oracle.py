"""Helpers of tests/test_kv_paged_cpu.py and tests/test_kv_paged_gpu.py: a page pool built on the host with every
unreachable datum in the kernel's way, its logical (gathered) view, the float64 oracle over an arbitrary set of
visible keys, and the expected bytes of a paged append as a host loop over (b, s)."""
import torch

from decode_oracle import decode_oracle64
from kv_fp8_oracle import FP8, dequantize_oracle, quantize_oracle

BF16 = torch.bfloat16


def bytes_of(t):
    return t.view(torch.uint8)


def nan_of(dtype):
    """a NaN of `dtype` (FP8: the code 0x7F)"""
    if dtype == FP8:
        return torch.tensor([0x7F], dtype=torch.uint8).view(FP8)[0]
    return torch.tensor(float("nan"), dtype=dtype)


def deal_pages(need, C, P, seed):
    """int32 [B, C]: `need[b]` distinct pages per row out of P, dealt column by column from a seeded permutation (so
    a row's pages are non-monotone and interleaved with the other rows'); the columns past a row's need alternate
    between -1 and P + 5."""
    B = len(need)
    perm = torch.randperm(P, generator=torch.Generator().manual_seed(seed)).tolist()
    table = torch.empty(B, C, dtype=torch.int32)
    for b in range(B):
        for c in range(C):
            table[b, c] = -1 if (b + c) % 2 == 0 else P + 5
    for c in range(C):
        for b in range(B):
            if c < need[b]:
                table[b, c] = perm.pop()
    return table


def scatter_to_pages(logical, table, lens, P, page):
    """logical [B, Smax, ...] -> pool [P, page, ...] of the same dtype, NaN everywhere except rows n < lens[b] of
    the pages the table names (so every unowned page and the tail of every last page is NaN)"""
    pool = torch.empty(P, page, *logical.shape[2:], dtype=logical.dtype)
    if logical.dtype == FP8:
        bytes_of(pool).fill_(0x7F)
    else:
        pool.fill_(float("nan"))
    src, dst = bytes_of(logical) if logical.dtype == FP8 else logical, bytes_of(pool) if logical.dtype == FP8 else pool
    for b in range(logical.shape[0]):
        n = min(max(int(lens[b]), 0), logical.shape[1])
        for c in range(-(-n // page)):
            e = int(table[b, c])
            if 0 <= e < P:
                hi = min(n, (c + 1) * page)
                dst[e, :hi - c * page] = src[b, c * page:hi]
    return pool


def visible(table, lens, P, page):
    """bool [B, C * page]: n < lens[b] (clamped) and the entry of n in [0, P)"""
    B, C = table.shape
    vis = torch.zeros(B, C * page, dtype=torch.bool)
    for b in range(B):
        n = min(max(int(lens[b]), 0), C * page)
        for i in range(n):
            vis[b, i] = 0 <= int(table[b, i // page]) < P
    return vis


def gather_nan(pool, table, lens, page):
    """the logical view [B, C * page, ...] of a pool by an explicit loop, with NaN (not zeros) wherever key n is not
    visible: at and past the length, and on invalid pages"""
    B, C = table.shape
    P = pool.shape[0]
    out = torch.empty(B, C * page, *pool.shape[2:], dtype=pool.dtype)
    fp8 = pool.dtype == FP8
    if fp8:
        bytes_of(out).fill_(0x7F)
    else:
        out.fill_(float("nan"))
    src, dst = (bytes_of(pool), bytes_of(out)) if fp8 else (pool, out)
    vis = visible(table, lens, P, page)
    for b in range(B):
        for c in range(C):
            e = int(table[b, c])
            if 0 <= e < P:
                m = vis[b, c * page:(c + 1) * page]
                dst[b, c * page:(c + 1) * page][m] = src[e][m]
    return out


def oracle_visible64(q, k64, v64, vis, scale=None):
    """decode_oracle64 over an arbitrary visible set: the visible keys of every row are moved to the front (softmax
    attention does not depend on the order of the keys) and counted. k64 / v64: [B, Smax, Hkv, D] float64, finite
    where visible. -> (o float64 [B, Hq, D], vmax float64 [B, Hkv])"""
    B, Smax = vis.shape
    kc, vc = torch.zeros_like(k64), torch.zeros_like(v64)
    lens = []
    for b in range(B):
        idx = vis[b].nonzero().flatten()
        kc[b, :len(idx)], vc[b, :len(idx)] = k64[b, idx], v64[b, idx]
        lens.append(len(idx))
    return decode_oracle64(q, kc, vc, lens, scale)


def reachable_rows(table, lens, P, page):
    """bool [P, page]: the pool rows some sequence sees"""
    vis = visible(table, lens, P, page)
    reach = torch.zeros(P, page, dtype=torch.bool)
    for b in range(table.shape[0]):
        for i in vis[b].nonzero().flatten().tolist():
            reach[int(table[b, i // page]), i % page] = True
    return reach


def expected_append(bufs, table, k, v, pos, counts, page):
    """The host's copy of `bufs` = (k_pages, v_pages[, k_scale, v_scale]) after a paged append of k, v [B, S, Hkv,
    D]: a loop over (b, s) that applies the store predicate to the oracle quantiser's bytes (FP8) or the input's own
    bytes (bf16). Everything no stored token owns keeps what `bufs` held."""
    want = [t.cpu().clone() for t in bufs]
    fp8 = len(bufs) == 4
    P = want[0].shape[0]
    B, C = table.shape
    if fp8:
        (qk, sk), (qv, sv) = quantize_oracle(k), quantize_oracle(v)
    else:
        qk, qv = k.cpu(), v.cpu()
    stored = 0
    for b in range(B):
        for s in range(k.shape[1]):
            if counts is not None and s >= int(counts[b]):
                continue
            p = (0 if pos is None else int(pos[b])) + s
            if p < 0 or p >= C * page:
                continue
            e = int(table[b, p // page])
            if e < 0 or e >= P:
                continue
            stored += 1
            bytes_of(want[0])[e, p % page], bytes_of(want[1])[e, p % page] = bytes_of(qk)[b, s], bytes_of(qv)[b, s]
            if fp8:
                want[2][e, p % page], want[3][e, p % page] = sk[b, s], sv[b, s]
    return want, stored


def dequant(codes, scale):
    return dequantize_oracle(codes, scale)
