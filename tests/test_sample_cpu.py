"""The sampling contract off the GPU: ops.lm.sample_logits_ref against the float64 oracle of tests/sample_oracle.py
token for token and in kept, each filter against an independent sort-based formulation on tie-free inputs, the tie
rules, eos / finished, and Llama.generate with top_p / min_p / per-row settings on llama-tiny."""
import numpy as np
import pytest
import torch

import sample_oracle as so


def _lm():
    from cs744_pytorch_distributed_tutorial_amd.ops import lm
    return lm


@pytest.mark.parametrize("filt", list(so.FILTERS))
@pytest.mark.parametrize("V", so.SHAPES)
def test_ref_equals_oracle(V, filt):
    for dtype_name, B in (("fp32", 3), ("bf16", 1)):
        logits, T, k, ps, mp, us, want = so.case(V, dtype_name, B, filt)
        for u, rows in zip(us, want):
            tok, kept = _lm().sample_logits_ref(logits, torch.tensor(u), return_kept=True,
                                                **so.settings_kwargs(T, k, ps, mp))
            assert tok.dtype == torch.int64 and kept.dtype == torch.int32
            assert tok.tolist() == [r.token for r in rows]
            assert kept.tolist() == [r.kept for r in rows]


def test_big_row_case_builds():
    """the [2, 128256] batch of the GPU tests: its construction conditions hold (checked here, without a GPU)"""
    for filt in ("top_k", "all", "none"):
        logits, T, k, ps, mp, us, want = so.case(128256, "bf16", 2, filt)
        tok, kept = _lm().sample_logits_ref(logits, torch.tensor(us[2]), return_kept=True,
                                            **so.settings_kwargs(T, k, ps, mp))
        assert tok.tolist() == [r.token for r in want[2]] and kept.tolist() == [r.kept for r in want[2]]


def test_gpu_cases_build():
    """every case of tests/test_sample_gpu.py::test_against_oracle meets its construction conditions"""
    for V in so.SHAPES:
        for dtype_name in so.DTYPES:
            for B in (1, 3):
                for filt in so.FILTERS:
                    so.case(V, dtype_name, B, filt)


def _tie_free(V, seed):
    z = torch.randn(V, generator=torch.Generator().manual_seed(seed)) * 2
    assert z.unique().numel() == V
    return z


@pytest.mark.parametrize("V", [16, 1000])
def test_filters_against_sort_formulation(V):
    """each filter alone, on tie-free fp32 logits, keeps what the textbook formulation keeps: the k largest; the
    shortest sorted prefix whose mass reaches top_p; the tokens with p_i >= min_p * p_max"""
    z = _tie_free(V, 5 + V)
    prob = torch.softmax(z.double() / 0.8, -1)
    order = prob.argsort(descending=True)
    k = 7
    r = so.oracle_row(z, 0.5, 0.8, k=k)
    assert set(np.flatnonzero(r.keep)) == set(order[:k].tolist()) and r.kept == k
    p = so.nucleus_p(z, 0.8, 5)
    r = so.oracle_row(z, 0.5, 0.8, p=p)
    n = int((prob[order].cumsum(-1) < p).sum()) + 1
    assert n == 5 and set(np.flatnonzero(r.keep)) == set(order[:n].tolist())
    r = so.oracle_row(z, 0.5, 0.8, mp=0.05)
    assert r.minp_margin >= so.MINP_MARGIN
    assert set(np.flatnonzero(r.keep)) == set(torch.nonzero(prob >= 0.05 * prob.max()).flatten().tolist())
    for kw in (dict(top_k=k), dict(top_p=p), dict(min_p=0.05)):
        okw = {"top_k": "k", "top_p": "p", "min_p": "mp"}
        want = so.oracle_row(z, 0.5, 0.8, **{okw[n_]: v for n_, v in kw.items()})
        tok, kept = _lm().sample_logits_ref(z[None], torch.tensor([0.5]), 0.8, return_kept=True, **kw)
        assert (int(tok), int(kept)) == (want.token, want.kept)


def test_ties_are_kept():
    lm = _lm()
    z = torch.tensor([0.0, 3.0, 1.0, 3.0, 1.0, 1.0, -2.0, 1.0, 1.0, float("-inf")])
    # five tokens tie at the 3rd largest value: top_k = 3 keeps 2 + 5
    for k, n in ((1, 2), (2, 2), (3, 7), (6, 7), (8, 8), (9, 9), (10, 9), (50, 9)):
        tok, kept = lm.sample_logits_ref(z[None], torch.tensor([0.999]), 1.0, top_k=k, return_kept=True)
        assert int(kept) == n == so.oracle_row(z, 0.999, 1.0, k=k).kept, k
        assert z[int(tok)] >= sorted(z.tolist(), reverse=True)[min(k, 10) - 1] and z[int(tok)] > float("-inf")
    # a two-way tie at the maximum under a tiny top_p: both stay; u picks between them
    for u, want in ((0.25, 1), (0.75, 3)):
        tok, kept = lm.sample_logits_ref(z[None], torch.tensor([u]), 1.0, top_p=1e-6, return_kept=True)
        assert (int(tok), int(kept)) == (want, 2)
    # a cut that falls inside the five-way tie keeps all five
    w = torch.exp(z.double() - 3)
    p = float((2 + 2.5 * math_e(-2)) / w.sum())
    tok, kept = lm.sample_logits_ref(z[None], torch.tensor([0.5]), 1.0, top_p=p, return_kept=True)
    assert int(kept) == 7 == so.oracle_row(z, 0.5, 1.0, p=p).kept


def math_e(x):
    import math
    return math.exp(x)


def test_edges_of_the_reference():
    lm = _lm()
    z = torch.tensor([[float("-inf"), 1.0, float("-inf"), 2.0, float("-inf")]])
    assert int(lm.sample_logits_ref(z, torch.tensor([0.0]))) == 1  # u = 0: the first kept index
    assert int(lm.sample_logits_ref(z, torch.tensor([np.nextafter(np.float32(1), np.float32(0))]))) == 3
    one = torch.full((1, 7), float("-inf"))
    one[0, 4] = -3.0
    for u in (0.0, 0.3, 0.9999):
        assert int(lm.sample_logits_ref(one, torch.tensor([u]), 0.7, top_k=3, top_p=0.5, min_p=0.1)) == 4
    for bad in (torch.full((1, 5), float("nan")), torch.full((1, 5), float("-inf"))):
        assert 0 <= int(lm.sample_logits_ref(bad, torch.tensor([0.5]), 0.7, top_p=0.9)) < 5
    # greedy: the lowest index of the maximum, whatever the filters say
    tok, kept = lm.sample_logits_ref(torch.tensor([[1.0, 5.0, 5.0]]), torch.tensor([0.9]), 0.0, top_p=0.5, return_kept=True)
    assert (int(tok), int(kept)) == (1, 1)
    for kw in (dict(temperature=-1.0), dict(top_k=0), dict(top_p=0.0), dict(top_p=1.5), dict(min_p=-0.1)):
        with pytest.raises(ValueError):
            lm.sample_logits_ref(z, torch.tensor([0.5]), **kw)
    tok, kept = lm.sample_logits_ref(torch.empty(0, 5), torch.empty(0), return_kept=True)
    assert tok.shape == (0,) and kept.shape == (0,)


def test_eos_and_finished_reference():
    lm = _lm()
    z = torch.zeros(4, 6)
    z[0, 2] = z[1, 5] = z[2, 3] = z[3, 5] = 50.0
    fin = torch.tensor([0, 0, 1, 0], dtype=torch.uint8)
    tok = lm.sample_logits(z, torch.full((4,), 0.5), 1.0, eos_id=5, finished=fin)
    assert tok.tolist() == [2, 5, 5, 5] and fin.tolist() == [0, 1, 1, 1]


def test_per_row_settings_reference():
    lm = _lm()
    z = torch.stack([so.make_logits(100, torch.float32, 70 + b) for b in range(4)])
    u = torch.tensor([0.3, 0.6, 0.2, 0.7])
    T = torch.tensor([0.0, 0.7, 1.0, 1.0])
    k = torch.tensor([100, 100, 5, 100])
    p = torch.tensor([1.0, 1.0, 1.0, 0.5])
    tok, kept = lm.sample_logits(z, u, T, k, p, return_kept=True)
    single = [dict(temperature=0.0), dict(temperature=0.7), dict(top_k=5), dict(top_p=0.5)]
    for b, kw in enumerate(single):
        t1, k1 = lm.sample_logits(z[b:b + 1], u[b:b + 1], return_kept=True, **kw)
        assert (int(tok[b]), int(kept[b])) == (int(t1), int(k1))
    assert int(tok[0]) == int(z[0].argmax()) and int(kept[0]) == 1 and int(kept[2]) == 5


# ------------------------------------------------------------------ the model
@pytest.fixture(scope="module")
def tiny():
    from cs744_pytorch_distributed_tutorial_amd.models import llama
    torch.manual_seed(3)
    m = llama.build("llama-tiny").eval()
    tokens = torch.randint(1, m.cfg.vocab_size, (3, 7), generator=torch.Generator().manual_seed(5))
    return m, tokens, m.generate(tokens, 8)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def test_generate_top_p_is_reproducible(tiny):
    m, tokens, _ = tiny
    a = m.generate(tokens, 8, top_p=0.9, temperature=0.8, generator=_gen(1))
    b = m.generate(tokens, 8, top_p=0.9, temperature=0.8, generator=_gen(1))
    c = m.generate(tokens, 8, top_p=0.9, temperature=0.8, generator=_gen(2))
    assert a.dtype == torch.int64 and a.shape == (3, 8)
    assert torch.equal(a, b) and not torch.equal(a, c)
    assert int(a.min()) >= 0 and int(a.max()) < m.cfg.vocab_size
    d = m.generate(tokens, 8, min_p=0.05, temperature=0.8, generator=_gen(1), sampler="fused")
    assert d.shape == (3, 8)


def test_generate_degenerate_settings_are_greedy(tiny):
    m, tokens, greedy = tiny
    assert torch.equal(m.generate(tokens, 8, top_p=1e-6, temperature=0.8, generator=_gen(1)), greedy)
    assert torch.equal(m.generate(tokens, 8, top_k=1, temperature=0.8, sampler="fused", generator=_gen(1)), greedy)
    assert torch.equal(m.generate(tokens, 8, temperature=torch.zeros(3), generator=_gen(1)), greedy)
    assert torch.equal(m.generate(tokens, 8, temperature=0.0, sampler="fused"), greedy)


def test_generate_mixed_per_row_temperature(tiny):
    m, tokens, greedy = tiny
    out = m.generate(tokens, 8, temperature=torch.tensor([0.0, 1.0, 0.0]), generator=_gen(3))
    assert torch.equal(out[0], greedy[0]) and torch.equal(out[2], greedy[2])
    assert not torch.equal(out[1], greedy[1])


def test_generate_eos_with_fused_sampler(tiny):
    m, tokens, greedy = tiny
    eos = int(greedy[0, 2])
    out = m.generate(tokens, 8, temperature=0.0, sampler="fused", eos_id=eos)
    first = (greedy[0] == eos).nonzero()[0, 0]
    assert torch.equal(out[0, :first + 1], greedy[0, :first + 1]) and bool((out[0, first:] == eos).all())
    with pytest.raises(ValueError):
        m.generate(tokens, 2, sampler="other")
