"""Float64 oracle of extend attention for tests/test_extend_cpu.py and tests/test_extend_gpu.py: an explicit loop
over (row, query, query head) on the visible keys only, so nothing stale is ever touched, the clamps of `start` and
`counts` as host arithmetic, and the builders of the operands both files share: a contiguous cache with NaN at every
stale position, and (with the helpers of tests/kv_paged_oracle.py) a page pool whose every unreachable datum is NaN
behind a non-monotone table."""
import math

import torch

from kv_paged_oracle import deal_pages, scatter_to_pages, visible


def clamp_bounds(start, counts, T, Smax):
    """-> (start clamped into [0, Smax], counts clamped into [0, min(T, Smax - start)]) as lists of int"""
    st = [min(max(int(s), 0), Smax) for s in start]
    cn = [T] * len(st) if counts is None else [int(c) for c in counts]
    return st, [min(max(c, 0), min(T, Smax - s)) for c, s in zip(cn, st)]


def extend_oracle64(q, kc, vc, start, counts=None, key_ok=None, scale=None):
    """q [B, T, Hq, D], kc / vc [B, Smax, Hkv, D] (finite wherever visible), start / counts [B] -> o float64
    [B, T, Hq, D]: query i < counts[b] of row b over the keys n <= start[b] + i (of those, the ones where `key_ok`
    bool [B, Smax] holds, when given); zeros for padded rows and for a query that sees no key."""
    B, T, Hq, D = q.shape
    Smax, Hkv = kc.shape[1], kc.shape[2]
    G = Hq // Hkv
    scale = 1.0 / math.sqrt(D) if scale is None else scale
    st, cn = clamp_bounds(start, counts, T, Smax)
    q64, k64, v64 = q.double().cpu(), kc.double().cpu(), vc.double().cpu()
    o = torch.zeros(B, T, Hq, D, dtype=torch.float64)
    for b in range(B):
        for i in range(cn[b]):
            n = st[b] + i + 1  # <= st + cn <= Smax
            idx = torch.arange(n) if key_ok is None else key_ok[b, :n].nonzero().flatten()
            if len(idx) == 0:
                continue
            for h in range(Hq):
                kv = h // G
                s = (k64[b, idx, kv] @ q64[b, i, h]) * scale
                p = torch.exp(s - s.max())
                o[b, i, h] = (p / p.sum()) @ v64[b, idx, kv]
    return o


def nan_stale_(kc, vc, start, counts, T, value=float("nan")):
    """fill every position at or past start[b] + counts[b] (both clamped) of both caches with `value`, in place"""
    st, cn = clamp_bounds(start, counts, T, kc.shape[1])
    for b in range(kc.shape[0]):
        kc[b, st[b] + cn[b]:] = value
        vc[b, st[b] + cn[b]:] = value
    return kc, vc


def rel_l2(o, o64):
    """the relative L2 error of every (row, query, head): [B, T, Hq] float64, 0 where both vectors are zero"""
    err = (o.double().cpu() - o64).norm(dim=-1)
    ref = o64.norm(dim=-1)
    return torch.where(ref > 0, err / ref.clamp_min(1e-300), err)


def paged_case(kc, vc, start, counts, T, page, seed, spare=3, hole=None):
    """The logical caches [B, Smax, ...] (Smax a multiple of `page`) as pools behind a table: row b owns
    ceil((start + counts) / page) pages dealt non-monotonically out of P = owned + `spare`; the table's other
    entries are -1 / P + 5; every unowned page and every last page's tail is NaN. `hole` = (b, column) replaces one
    owned entry by -1: an invalid page inside the visible range. -> (k_pages, v_pages, table int32 [B, C],
    key_ok bool [B, Smax])"""
    B, Smax = kc.shape[0], kc.shape[1]
    C = Smax // page
    assert C * page == Smax
    st, cn = clamp_bounds(start, counts, T, Smax)
    lens = [s + c for s, c in zip(st, cn)]
    need = [-(-n // page) for n in lens]
    P = sum(need) + spare
    table = deal_pages(need, C, P, seed)
    if hole is not None:
        assert hole[1] < need[hole[0]]
        table[hole[0], hole[1]] = -1
    kp, vp = scatter_to_pages(kc, table, lens, P, page), scatter_to_pages(vc, table, lens, P, page)
    return kp, vp, table, visible(table, lens, P, page)


# ------------------------------------------------------------------ the model driver both files share
def stale_(cache):
    """fill a fresh cache (contiguous or paged) with NaN: codes 0x7F and NaN scales for an FP8 one"""
    if cache.k_scale is not None:
        cache.k.view(torch.uint8).fill_(0x7F)
        cache.v.view(torch.uint8).fill_(0x7F)
        cache.k_scale.fill_(float("nan"))
        cache.v_scale.fill_(float("nan"))
    else:
        cache.k.fill_(float("nan"))
        cache.v.fill_(float("nan"))
    return cache


def model_scenarios(model, tokens, lens, make_cache, chunks, steps=3, pad_id=0):
    """Run `model` over `tokens` [B, S] through caches from `make_cache()` in every way that goes through
    Llama.extend. -> {name: ([(b, t, logits [V])], cache)}: the logits the cached path gives for position t of row b
    (to compare with model(tokens)[b, t]) and the cache it left.
      chunk<n>:    prefill(chunk=n) of the ragged prompts tokens[b, :lens[b]] (right-padded with pad_id)
      one_shot:    the same prompts through the one-shot prefill (no extend: the yardstick of the cache contents)
      extend_all:  one-shot prefill of the first min(lens) tokens, then ONE extend of all the rest, all_logits
      second_turn: ragged prefill, `steps` decode_steps with the true tokens, then an extend of the following
                   T2 = S - max(lens) - steps tokens with ragged counts (T2, T2 - 2), all_logits"""
    B, S = tokens.shape
    dev = tokens.device
    host = tokens.cpu()
    P = max(lens)
    prompt = tokens[:, :P].clone()
    for b, n in enumerate(lens):
        prompt[b, n:] = pad_id
    out = {}
    for n in chunks:
        cache = make_cache()
        lg = model.prefill(prompt, cache, torch.tensor(lens), chunk=n)
        out[f"chunk{n}"] = ([(b, lens[b] - 1, lg[b]) for b in range(B)], cache)
    cache = make_cache()
    lg = model.prefill(prompt, cache, torch.tensor(lens))
    out["one_shot"] = ([(b, lens[b] - 1, lg[b]) for b in range(B)], cache)

    cache, P0 = make_cache(), min(lens)
    model.prefill(tokens[:, :P0], cache)
    lg = model.extend(tokens[:, P0:], cache, all_logits=True)
    out["extend_all"] = ([(b, P0 + i, lg[b, i]) for b in range(B) for i in range(S - P0)], cache)

    cache = make_cache()
    model.prefill(prompt, cache, torch.tensor(lens))
    for j in range(steps):
        model.decode_step(torch.tensor([int(host[b, lens[b] + j]) for b in range(B)], device=dev), cache)
    T2 = S - P - steps
    counts = [T2 if b % 2 == 0 else T2 - 2 for b in range(B)]
    turn = torch.full((B, T2), pad_id, dtype=tokens.dtype)
    for b in range(B):
        turn[b, :counts[b]] = host[b, lens[b] + steps:lens[b] + steps + counts[b]]
    lg = model.extend(turn.to(dev), cache, counts=counts, all_logits=True)
    out["second_turn"] = ([(b, lens[b] + steps + i, lg[b, i]) for b in range(B) for i in range(counts[b])], cache)
    out["second_turn_state"] = ([], ([n + steps + c for n, c in zip(lens, counts)], P + steps + T2))
    return out


def worst(got, ref):
    """max |logits - ref[b, t]| over the reported positions"""
    return max((lg.double().cpu() - ref[b, t]).abs().max().item() for b, t, lg in got)
