"""Float64 oracle of decode attention for tests/test_decode_cpu.py and tests/test_decode_gpu.py: an explicit
loop over (sequence, query head) on the visible keys only, so nothing past a length is ever touched, and the
teacher-forced driver both files run a model through."""
import math

import torch


def decode_oracle64(q, kc, vc, lens, scale=None):
    """q [B, Hq, D], kc / vc [B, Smax, Hkv, D], lens [B] (clamped into [0, Smax]) -> (o float64 [B, Hq, D],
    vmax float64 [B, Hkv]: the largest |v| among each (sequence, kv head)'s visible keys, 0 where none)"""
    B, Hq, D = q.shape
    Smax, Hkv = kc.shape[1], kc.shape[2]
    G = Hq // Hkv
    scale = 1.0 / math.sqrt(D) if scale is None else scale
    q64, k64, v64 = q.double().cpu(), kc.double().cpu(), vc.double().cpu()
    o = torch.zeros(B, Hq, D, dtype=torch.float64)
    vmax = torch.zeros(B, Hkv, dtype=torch.float64)
    for b in range(B):
        n = min(max(int(lens[b]), 0), Smax)
        if n == 0:
            continue
        for h in range(Hq):
            kv = h // G
            s = (k64[b, :n, kv] @ q64[b, h]) * scale
            p = torch.exp(s - s.max())
            o[b, h] = (p / p.sum()) @ v64[b, :n, kv]
            vmax[b, kv] = v64[b, :n, kv].abs().max()
    return o, vmax


def nan_tail_(kc, vc, lens, value=float("nan")):
    """fill every position >= lens[b] of both caches with `value`, in place"""
    for b in range(kc.shape[0]):
        n = min(max(int(lens[b]), 0), kc.shape[1])
        kc[b, n:] = value
        vc[b, n:] = value
    return kc, vc


def teacher_forced(model, tokens, prompt_lens, cache, pad_id=0):
    """Prefill with ragged prompts, then decode_step with the true next tokens until the shortest row has
    reached S. -> [(b, t, logits [V])]: the cached path's logits of position t of row b, for every t from
    prompt_lens[b] - 1 to S - 1 (to compare with model(tokens)[b, t]). The prompt is right-padded with
    `pad_id`; a row that runs past S is fed `pad_id` and no longer reported."""
    B, S = tokens.shape
    P = max(prompt_lens)
    host = tokens.cpu()
    prompt = tokens[:, :P].clone()
    for b, n in enumerate(prompt_lens):
        prompt[b, n:] = pad_id
    out = []
    logits = model.prefill(prompt, cache, torch.tensor(prompt_lens))
    for b, n in enumerate(prompt_lens):
        out.append((b, n - 1, logits[b]))
    for i in range(S - min(prompt_lens)):
        pos = [n + i for n in prompt_lens]
        tok = torch.tensor([int(host[b, p]) if p < S else pad_id for b, p in enumerate(pos)], device=tokens.device)
        logits = model.decode_step(tok, cache)
        for b, p in enumerate(pos):
            if p < S:
                out.append((b, p, logits[b]))
    return out
