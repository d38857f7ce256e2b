"""The sampling contract of docs/sampling.md in float64, one row at a time, with the margin of every decision, and
the builders of the test cases (used by tests/test_sample_cpu.py and tests/test_sample_gpu.py).

Only step 1, s = float(z) / T, is done in fp32, the way the kernel does it; weights, sums and comparisons are
float64. A margin says how far a decision was from going the other way:
  p_margin     top-p: the distance of top_p * W from the cumulative masses just below and at the cut, over W;
  minp_margin  min-p: the distance in s of the nearest candidate from smax + log(min_p);
  u_margin     the draw: the distance of u * W_kept from the two ends of the drawn token's CDF interval, over W_kept.
A side on which nothing can flip (no mass above the cut's first value, no kept token in front of the drawn one) is
infinite. The builders assert p_margin, u_margin >= 1e-4 and minp_margin >= 1e-3: conditions of construction, orders
of magnitude above the fp32 error of a weight (1e-7 relative) and of the kernel's integer masses (2^-27 of a
128256-token row), not tolerances measured on the code under test."""
import functools
import math
from collections import namedtuple

import numpy as np
import torch

Row = namedtuple("Row", "token kept keep probs p_margin minp_margin u_margin")
P_MARGIN = U_MARGIN = 1e-4
MINP_MARGIN = 1e-3
INF = float("inf")


def scaled(z: torch.Tensor, T: float) -> np.ndarray:
    """step 1: fp32 division, NaN -> -inf, as float64"""
    s = (z.float() / torch.tensor(T, dtype=torch.float32)).double().numpy().copy()
    s[np.isnan(s)] = -INF
    return s + 0.0


def oracle_row(z: torch.Tensor, u: float, T=1.0, k=None, p=None, mp=None) -> Row:
    """z: [V] of any float dtype; u: a Python float (the fp32 value the kernel gets, exactly)."""
    V = z.numel()
    zf = z.float().double().numpy().copy()
    bad = bool(np.isnan(zf).any())
    zf[np.isnan(zf)] = -INF
    one = np.zeros(V, bool)
    if T == 0:
        i = int(np.flatnonzero(zf == zf.max())[0])
        one[i] = True
        return Row(i, 1, one, one.astype(float), INF, INF, INF)
    s = scaled(z, T)
    smax = s.max()
    if bad or not math.isfinite(smax):  # step 8: any token in [0, V); the oracle names the arg max
        i = int(np.flatnonzero(s == smax)[0])
        one[i] = True
        return Row(i, 1, one, one.astype(float), INF, INF, INF)
    keep = s > -INF
    if k is not None and 1 <= k < V:
        keep &= s >= np.sort(s)[V - k]
    w = np.exp(s - smax)
    minp_margin = INF
    if mp is not None and mp > 0:
        minp_margin = float(np.abs(s[keep] - (smax + math.log(mp))).min())
        keep &= w >= mp
    p_margin = INF
    if p is not None and p < 1:
        vals, inv = np.unique(s[keep], return_inverse=True)  # ascending
        group = np.bincount(inv, weights=w[keep], minlength=len(vals))[::-1]  # mass per distinct value, descending
        cum = np.cumsum(group)
        W = cum[-1]
        target = float(np.float32(p)) * W
        j = int(np.flatnonzero(cum >= target)[0]) if (cum >= target).any() else len(cum) - 1
        keep &= s >= vals[::-1][j]
        below = (target - cum[j - 1]) / W if j > 0 else INF
        p_margin = float(min((cum[j] - target) / W, below))
    wk = np.where(keep, w, 0.0)
    cdf = np.cumsum(wk)
    Wk = cdf[-1]
    tgt = float(u) * Wk
    hit = np.flatnonzero(keep & (cdf >= tgt))
    idx = np.flatnonzero(keep)
    tok = int(hit[0]) if len(hit) else int(idx[-1])
    lo = cdf[tok] - wk[tok]
    below = (tgt - lo) / Wk if tok != idx[0] else INF
    above = (cdf[tok] - tgt) / Wk if tok != idx[-1] else INF
    return Row(tok, int(keep.sum()), keep, wk / Wk, p_margin, minp_margin, float(min(below, above)))


def u_mid(row: Row, tok: int) -> float:
    """the fp32 u at the midpoint of a kept token's CDF interval"""
    cdf = np.cumsum(row.probs)
    return float(np.float32(cdf[tok] - row.probs[tok] / 2))


def targets(row: Row):
    """the first kept token, the last one and a middle one, each with at least 1e-3 of the kept mass"""
    idx = np.flatnonzero(row.keep)
    big = np.flatnonzero(row.probs >= 1e-3)
    assert row.probs[idx[0]] >= 1e-3 and row.probs[idx[-1]] >= 1e-3, "construction: an end token below 1e-3"
    return [int(idx[0]), int(idx[-1]), int(big[len(big) // 2])]


def make_logits(V: int, dtype, seed: int, sigma: float = 2.0) -> torch.Tensor:
    """[V] random logits with three distinct peaks at the first, the middle and the last index: they survive every
    filter of the cases and each holds well over 1e-3 of any kept mass. Values are rounded to ``dtype``."""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(V, generator=g) * sigma
    hi = 4.5 * sigma
    z[0] = hi
    if V >= 2:
        z[V - 1] = hi + 0.5
    if V >= 3:
        z[V // 2] = hi + 1.0
    return z.to(dtype)


def nucleus_p(z: torch.Tensor, T: float, n: int) -> float:
    """a top_p whose cut falls between the n-th and the (n + 1)-th largest of tie-free top values: the fp32 value
    nearest the middle of the n-th token's slice of the cumulative mass"""
    s = scaled(z, T)
    w = np.sort(np.exp(s - s.max()))[::-1]
    cum = np.cumsum(w)
    n = min(n, len(w))
    return float(np.float32((cum[n - 1] - w[n - 1] / 2) / cum[-1]))


def margins_ok(row: Row) -> bool:
    return row.p_margin >= P_MARGIN and row.minp_margin >= MINP_MARGIN and row.u_margin >= U_MARGIN


def check_margins(row: Row, what: str = ""):
    assert row.p_margin >= P_MARGIN, f"construction {what}: top-p margin {row.p_margin:.2e}"
    assert row.minp_margin >= MINP_MARGIN, f"construction {what}: min-p margin {row.minp_margin:.2e}"
    assert row.u_margin >= U_MARGIN, f"construction {what}: draw margin {row.u_margin:.2e}"


# the filter settings of the cases: name -> (T, k, p, min_p); p "auto": nucleus_p(z, T, 4)
FILTERS = {
    "none": (1.0, None, None, None),
    "top_k": (0.7, 50, None, None),
    "top_p": (0.9, None, "auto", None),
    "min_p": (0.8, None, None, 0.02),
    "all": (0.7, 50, 0.9, 0.01),
    "off": (1.3, 1 << 30, 1.0, 0.0),  # k >= V, top_p = 1, min_p = 0: nothing filtered
}
SHAPES = [1, 2, 63, 64, 65, 1023, 1024, 1025, 4099]
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}


@functools.lru_cache(maxsize=None)
def case(V: int, dtype_name: str, B: int, filt: str):
    """One batch, built once and never changed: logits [B, V] (each row its own seed), the settings, and per target
    (first / last / middle kept token) the u [B] and the oracle's rows. Every margin is asserted here, on the CPU."""
    dtype = DTYPES[dtype_name]
    T, k, p, mp = FILTERS[filt]
    seed0 = 1000 * SHAPES.index(V) if V in SHAPES else 99000
    rows, ps, us, want = [], [], [[], [], []], [[], [], []]
    for b in range(B):
        seed = seed0 + 10 * list(DTYPES).index(dtype_name) + b
        # the oracle alone picks the inputs: the first of eight seeds whose margins hold (the last one asserts)
        for attempt in range(8):
            z = make_logits(V, dtype, seed + 100 * attempt)
            pb = nucleus_p(z, T, 4) if p == "auto" else p
            base = oracle_row(z, 0.5, T, k, pb, mp)
            toks = targets(base)
            got = [oracle_row(z, u_mid(base, tok), T, k, pb, mp) for tok in toks]
            if all(margins_ok(r) for r in got) or attempt == 7:
                break
        for j, (tok, r) in enumerate(zip(toks, got)):
            assert r.token == tok
            check_margins(r, f"V={V} {dtype_name} {filt}")
            us[j].append(u_mid(base, tok))
            want[j].append(r)
        rows.append(z)
        ps.append(pb)
    return torch.stack(rows), T, k, ps, mp, us, want


def settings_kwargs(T, k, ps, mp, dev="cpu"):
    """keyword arguments of sample_logits for a case (top_p per row where the rows differ)"""
    kw = dict(temperature=T, top_k=k, min_p=mp)
    if ps[0] is None or all(x == ps[0] for x in ps):
        kw["top_p"] = ps[0]
    else:
        kw["top_p"] = torch.tensor(ps, dtype=torch.float32, device=dev)
    return kw
