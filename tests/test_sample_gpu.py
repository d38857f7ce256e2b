"""The fused sampler on the GPU (csrc/kernels/sample.hip through ops.lm.sample_logits, the reference patched out)
token for token and in kept against the float64 oracle of tests/sample_oracle.py, on cases whose decision margins
the builders assert on the CPU: the scalar head and tail (rows start one element into a larger buffer), every V around
the vector and tile sizes in all three dtypes, a 128256-token row, ties, degenerate filters, the distribution over
4096 evenly spaced u, the ends of u, -inf, invalid rows, per-row settings, eos / finished, determinism, the host
checks, and Llama.generate under bf16 autocast (MI355X only)."""
import numpy as np
import pytest
import torch

import sample_oracle as so

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
NEG = float("-inf")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cs744_pytorch_distributed_tutorial_amd.ops import native
    native.C()
    return torch.device("cuda", 0)


def _lm():
    from cs744_pytorch_distributed_tutorial_amd.ops import lm
    return lm


def _C():
    from cs744_pytorch_distributed_tutorial_amd import _C
    return _C


@pytest.fixture
def no_ref(monkeypatch):
    """the kernel must run: the reference raises"""
    def boom(*a, **kw):
        raise AssertionError("sample_logits fell back to the reference")
    monkeypatch.setattr(_lm(), "sample_logits_ref", boom)
    return monkeypatch


def _offset(logits, dev):
    """the same values in rows that start one element into a larger buffer: row 0 is never 16-byte aligned"""
    B, V = logits.shape
    buf = torch.empty(B * V + 1, dtype=logits.dtype, device=dev)
    view = buf[1:].view(B, V)
    view.copy_(logits)
    assert view.data_ptr() % 16 != 0 and view.stride(1) == 1
    return view


def _run(logits, u, dev, **kw):
    kw = {n: (v.to(dev) if isinstance(v, torch.Tensor) else v) for n, v in kw.items()}
    tok, kept = _lm().sample_logits(logits, torch.as_tensor(u, dtype=torch.float32).to(dev), return_kept=True, **kw)
    assert tok.dtype == torch.int64 and kept.dtype == torch.int32 and tok.shape == kept.shape == logits.shape[:1]
    return tok.tolist(), kept.tolist()


def _check_case(V, dtype_name, B, filt, dev):
    logits, T, k, ps, mp, us, want = so.case(V, dtype_name, B, filt)
    x = _offset(logits, dev)
    for u, rows in zip(us, want):
        tok, kept = _run(x, u, dev, **so.settings_kwargs(T, k, ps, mp))
        what = f"V={V} {dtype_name} B={B} {filt}"
        assert tok == [r.token for r in rows], what
        assert kept == [r.kept for r in rows], what


@pytest.mark.parametrize("dtype_name", list(so.DTYPES))
@pytest.mark.parametrize("V", so.SHAPES)
def test_against_oracle(dev, no_ref, V, dtype_name):
    """every filter setting, B in {1, 3}, u at the middle of the first, the last and a middle kept token's interval"""
    for B in (1, 3):
        for filt in so.FILTERS:
            _check_case(V, dtype_name, B, filt, dev)


@pytest.mark.parametrize("filt", ["top_k", "all", "none"])
def test_llama_vocabulary_row(dev, no_ref, filt):
    _check_case(128256, "bf16", 2, filt, dev)


@pytest.mark.parametrize("dtype_name", list(so.DTYPES))
def test_kept_counts_ties_at_kth(dev, no_ref, dtype_name):
    """top-k alone is exact, ties included: five tokens share the k-th value, so k = 3 .. 7 all keep 2 + 5"""
    for V in (9, 65, 1025, 4099):
        g = torch.Generator().manual_seed(V)
        z = (torch.rand(V, generator=g) * 4 - 8).to(so.DTYPES[dtype_name])  # all below -4
        idx = torch.randperm(V, generator=g)[:8].tolist()
        z[idx[0]], z[idx[1]] = 3.0, 2.0
        for i in idx[2:7]:
            z[i] = 1.0
        x = _offset(z[None], dev)
        for k in (1, 2, 3, 5, 7, 8, V - 1, V, V + 5):
            want = so.oracle_row(z, 0.999, 1.0, k=k)
            tok, kept = _run(x, [0.999], dev, temperature=1.0, top_k=k)
            assert kept == [want.kept], (V, k)
            assert want.keep[tok[0]], (V, k)
            if 3 <= k <= 7:
                assert kept == [7]


def test_degenerate_filters(dev, no_ref):
    z = so.make_logits(1025, torch.float32, 3)
    x = _offset(z[None], dev)
    top = int(z.argmax())
    for u in (0.0, 0.5, 0.99999):  # a top_p so small that only the maximum survives
        assert _run(x, [u], dev, temperature=0.9, top_p=1e-6) == ([top], [1])
    assert _run(x, [0.7], dev, temperature=0.9, min_p=1.0) == ([top], [1])
    assert _run(x, [0.7], dev, temperature=0.9, top_k=1) == ([top], [1])
    z2 = z.clone()
    z2[17] = z2[top]  # a two-way tie at the maximum
    x2 = _offset(z2[None], dev)
    lo, hi = sorted((17, top))
    assert _run(x2, [0.25], dev, temperature=0.9, top_p=1e-6) == ([lo], [2])
    assert _run(x2, [0.75], dev, temperature=0.9, top_p=1e-6) == ([hi], [2])
    assert _run(x2, [0.75], dev, temperature=0.0, top_p=1e-6) == ([lo], [1])  # greedy: the lowest index


def test_distribution_over_even_u(dev, no_ref):
    """one row of 16 logits over 4096 rows, u = (i + 0.5) / 4096: every token's count is within 1 of the oracle's,
    and a token outside the kept set is never drawn"""
    n = 4096
    z = (torch.randn(16, generator=torch.Generator().manual_seed(21)) * 2).to(BF16)
    u = ((torch.arange(n, dtype=torch.float64) + 0.5) / n).float()
    x = z[None].expand(n, 16).contiguous().to(dev)
    for kw, okw in ((dict(temperature=1.0), {}), (dict(temperature=0.7, top_k=9, top_p=0.9, min_p=0.01),
                                                  dict(k=9, p=0.9, mp=0.01))):
        base = so.oracle_row(z, 0.5, kw["temperature"], **okw)
        assert base.p_margin >= so.P_MARGIN and base.minp_margin >= so.MINP_MARGIN
        cdf = np.cumsum(base.probs)
        kept_idx = np.flatnonzero(base.keep)
        want = np.zeros(16, int)
        for t in u.double().numpy() * cdf[-1]:
            hit = np.flatnonzero(base.keep & (cdf >= t))
            want[hit[0] if len(hit) else kept_idx[-1]] += 1
        tok, kept = _run(x, u, dev, **kw)
        got = np.bincount(np.array(tok), minlength=16)
        print("counts", got.tolist(), "oracle", want.tolist(), "4096 p", np.round(n * base.probs, 2).tolist())
        assert np.abs(got - want).max() <= 1
        assert (got[~base.keep] == 0).all() and set(kept) == {base.kept}
        assert np.abs(want - n * base.probs).max() < 1  # the oracle's own counts: evenly spaced u


def test_ends_of_u(dev, no_ref):
    last_u = float(np.nextafter(np.float32(1), np.float32(0)))
    for V, dtype_name, filt in ((65, "fp32", "all"), (1025, "bf16", "top_p"), (4099, "fp16", "none"), (4099, "fp32", "min_p")):
        logits, T, k, ps, mp, _, want = so.case(V, dtype_name, 3, filt)
        x = _offset(logits, dev)
        kw = so.settings_kwargs(T, k, ps, mp)
        tok, _ = _run(x, [0.0] * 3, dev, **kw)
        assert tok == [int(np.flatnonzero(r.keep)[0]) for r in want[0]]
        tok, _ = _run(x, [last_u] * 3, dev, **kw)
        for t, r in zip(tok, want[0]):
            assert r.keep[t] and r.probs[t + 1:].sum() <= 1e-5


def test_neg_inf_is_never_drawn(dev, no_ref):
    V = 1025
    z = so.make_logits(V, torch.float32, 8)
    mask = torch.rand(V, generator=torch.Generator().manual_seed(9)) < 0.5
    mask[0] = mask[V - 1] = True
    z[mask] = NEG
    x = _offset(z[None].expand(64, V).contiguous(), dev)
    u = (torch.arange(64, dtype=torch.float32) + 0.5) / 64
    u[0], u[63] = 0.0, float(np.nextafter(np.float32(1), np.float32(0)))
    tok, kept = _run(x, u, dev, temperature=1.5)
    assert not mask[tok].any() and set(kept) == {int((~mask).sum())}
    one = torch.full((3, V), NEG)
    one[:, 700] = -5.0
    for kw in (dict(temperature=1.0), dict(temperature=0.7, top_k=5, top_p=0.5, min_p=0.2)):
        assert _run(_offset(one, dev), [0.0, 0.4, float(u[63])], dev, **kw) == ([700] * 3, [1] * 3)


def test_invalid_rows_stay_in_range(dev, no_ref):
    for V in (1, 7, 1025):
        z = torch.randn(4, V)
        z[0] = float("nan")
        z[1] = NEG
        z[2, V // 2] = float("nan")
        z[3] = float("inf")
        for dt in (torch.float32, BF16, torch.float16):
            for kw in (dict(temperature=0.8, top_k=3, top_p=0.9, min_p=0.1), dict(temperature=0.0), dict(temperature=1.0)):
                tok, _ = _run(_offset(z.to(dt), dev), [0.0, 0.5, 0.9, 0.99], dev, **kw)
                assert all(0 <= t < V for t in tok), (V, dt, tok)


def test_per_row_settings(dev, no_ref):
    """one launch with a greedy row, a T = 0.7 row, a top_k = 5 row and a top_p = 0.5 row: each equals its own call"""
    V = 1025
    z = torch.stack([so.make_logits(V, BF16, 70 + b) for b in range(4)])
    x = _offset(z, dev)
    u = [0.3, 0.6, 0.2, 0.7]
    tok, kept = _run(x, u, dev, temperature=torch.tensor([0.0, 0.7, 1.0, 1.0]), top_k=torch.tensor([V, V, 5, V]),
                     top_p=torch.tensor([1.0, 1.0, 1.0, 0.5]), min_p=torch.zeros(4))
    single = [dict(temperature=0.0), dict(temperature=0.7), dict(top_k=5), dict(top_p=0.5)]
    okw = [dict(T=0.0), dict(T=0.7), dict(k=5), dict(p=0.5)]
    for b in range(4):
        t1, k1 = _run(x[b:b + 1], u[b:b + 1], dev, **single[b])
        assert (tok[b], kept[b]) == (t1[0], k1[0])
        r = so.oracle_row(z[b], float(np.float32(u[b])), **okw[b])
        assert r.p_margin >= so.P_MARGIN and r.u_margin >= so.U_MARGIN
        assert (tok[b], kept[b]) == (r.token, r.kept)
    # out-of-range per-row values are clamped on the device: T < 0 -> greedy, k < 1 -> 1, p > 1 -> 1, min_p < 0 -> 0
    tok, kept = _run(x, u, dev, temperature=torch.tensor([-1.0, 1.0, 1.0, 1.0]), top_k=torch.tensor([V, 0, V, V]),
                     top_p=torch.tensor([1.0, 1.0, 7.0, 1.0]), min_p=torch.tensor([0.0, 0.0, 0.0, -3.0]))
    assert kept[0] == 1 and tok[0] == int(z[0].float().argmax()) and kept[1] == 1 and kept[2] == V and kept[3] == V


def test_eos_and_finished(dev, no_ref):
    z = torch.zeros(5, 100)
    for b, t in enumerate((2, 50, 3, 50, 99)):
        z[b, t] = 60.0
    fin = torch.tensor([0, 0, 1, 0, 0], dtype=torch.uint8, device=dev)
    tok = _lm().sample_logits(_offset(z, dev), torch.full((5,), 0.5, device=dev), 1.0, eos_id=50, finished=fin)
    assert tok.tolist() == [2, 50, 50, 50, 99] and fin.tolist() == [0, 1, 1, 1, 0]
    flag = torch.tensor([False, True, False, False, False], device=dev)  # a bool mask is updated in place as well
    tok = _lm().sample_logits(_offset(z, dev), torch.full((5,), 0.5, device=dev), 0.0, eos_id=99, finished=flag)
    assert tok.tolist() == [2, 99, 3, 50, 99] and flag.tolist() == [False, True, False, False, True]


def test_same_bits_every_run(dev, no_ref):
    logits, T, k, ps, mp, us, _ = so.case(128256, "bf16", 2, "all")
    x = _offset(logits, dev)
    runs = [_run(x, us[2], dev, **so.settings_kwargs(T, k, ps, mp)) for _ in range(3)]
    assert runs[0] == runs[1] == runs[2]
    z = torch.randn(64, 4099, generator=torch.Generator().manual_seed(2)).to(dev)
    u = torch.rand(64, generator=torch.Generator().manual_seed(3))
    a = _run(z, u, dev, temperature=0.9, top_k=100, top_p=0.95, min_p=0.001)
    assert a == _run(z, u, dev, temperature=0.9, top_k=100, top_p=0.95, min_p=0.001)


def test_host_checks(dev):
    C = _C()
    z = torch.randn(3, 64, device=dev)
    u = torch.rand(3, device=dev)
    ok_tok, ok_kept = C.sample_logits(z, u)
    assert ok_tok.shape == (3,) and ok_kept.tolist() == [64] * 3
    bad = [
        lambda: C.sample_logits(z.double(), u),
        lambda: C.sample_logits(z.long(), u),
        lambda: C.sample_logits(z, u.double()),
        lambda: C.sample_logits(z, torch.rand(4, device=dev)),
        lambda: C.sample_logits(z, u[:, None]),
        lambda: C.sample_logits(z, u.cpu()),
        lambda: C.sample_logits(z, u, top_p=0.0),
        lambda: C.sample_logits(z, u, top_p=1.5),
        lambda: C.sample_logits(z, u, top_k=-1),
        lambda: C.sample_logits(z, u, temperature=-0.5),
        lambda: C.sample_logits(z, u, min_p=2.0),
        lambda: C.sample_logits(torch.randn(64, 3, device=dev).t(), u),
        lambda: C.sample_logits(z[0], u),
        lambda: C.sample_logits(z, u, temperature_rows=torch.ones(3, device=dev, dtype=torch.float64)),
        lambda: C.sample_logits(z, u, top_k_rows=torch.ones(3, device=dev, dtype=torch.int64)),
        lambda: C.sample_logits(z, u, top_p_rows=torch.ones(2, device=dev)),
        lambda: C.sample_logits(z, u, eos_id=3),
        lambda: C.sample_logits(z, u, eos_id=3, finished=torch.zeros(3, dtype=torch.bool, device=dev)),
    ]
    for i, f in enumerate(bad):  # i: which one, in a failure's locals
        with pytest.raises(RuntimeError):
            f()
        assert i >= 0
    for kw in (dict(top_k=0), dict(top_p=0.0), dict(temperature=-1.0), dict(min_p=1.5)):  # the public op: k = 0 too
        with pytest.raises(ValueError):
            _lm().sample_logits(z, u, **kw)
    tok, kept = C.sample_logits(torch.empty(0, 64, device=dev), torch.empty(0, device=dev))
    assert tok.shape == (0,) and tok.dtype == torch.int64 and kept.shape == (0,) and kept.dtype == torch.int32
    torch.cuda.synchronize()


# ------------------------------------------------------------------ the model
def _tiny(dev):
    from cs744_pytorch_distributed_tutorial_amd.models import llama
    torch.manual_seed(11)
    return llama.build("llama-tiny").eval().to(dev)


def _gen(dev, seed):
    return torch.Generator(device=dev).manual_seed(seed)


def test_model_generate_fused(dev, no_ref):
    m = _tiny(dev)
    tokens = torch.randint(1, m.cfg.vocab_size, (3, 9), generator=torch.Generator().manual_seed(12)).to(dev)
    with torch.autocast("cuda", dtype=BF16):
        a = m.generate(tokens, 10, top_p=0.9, temperature=0.8, sampler="fused", generator=_gen(dev, 1))
        b = m.generate(tokens, 10, top_p=0.9, temperature=0.8, sampler="fused", generator=_gen(dev, 1))
        c = m.generate(tokens, 10, top_p=0.9, temperature=0.8, generator=_gen(dev, 2))
    assert a.dtype == torch.int64 and a.shape == (3, 10) and a.device.type == "cuda"
    assert torch.equal(a, b) and not torch.equal(a, c)
    assert int(a.min()) >= 0 and int(a.max()) < m.cfg.vocab_size


@pytest.mark.parametrize("cache", ["slab", "fp8", "paged"])
def test_model_top_k_1_is_greedy_first_token(dev, no_ref, cache):
    """only the first token: later ones may differ between paths (docs/decode_attention.md)"""
    m = _tiny(dev)
    tokens = torch.randint(1, m.cfg.vocab_size, (3, 9), generator=torch.Generator().manual_seed(13)).to(dev)
    kw = {"slab": {}, "fp8": dict(kv_dtype="fp8"), "paged": dict(page_size=64)}[cache]
    with torch.autocast("cuda", dtype=BF16):
        greedy = m.generate(tokens, 3, **kw)
        fused = m.generate(tokens, 3, temperature=0.8, top_k=1, sampler="fused", generator=_gen(dev, 4), **kw)
        rows = m.generate(tokens, 3, temperature=torch.zeros(3), generator=_gen(dev, 4), **kw)
    assert torch.equal(fused[:, 0], greedy[:, 0]) and torch.equal(rows[:, 0], greedy[:, 0])


def test_model_eos_and_no_host_sync(dev, no_ref):
    from cs744_pytorch_distributed_tutorial_amd.ops import attention as att
    m = _tiny(dev)
    tokens = torch.randint(1, m.cfg.vocab_size, (3, 9), generator=torch.Generator().manual_seed(14)).to(dev)
    with torch.autocast("cuda", dtype=BF16):
        free = m.generate(tokens, 12, temperature=1.0, top_p=0.95, generator=_gen(dev, 5))
        eos = int(free[0, 3])
        out = m.generate(tokens, 12, temperature=1.0, top_p=0.95, eos_id=eos, generator=_gen(dev, 5))
        # a step of the fused loop reads nothing back
        cache = att.KVCache.allocate(m.cfg, 3, 9 + 8, dev, m.cache_dtype(dev))
        logits = m.prefill(tokens, cache)
        g = _gen(dev, 6)
        m.decode_loop(logits, cache, 2, 0.8, 20, eos, g, top_p=0.9, min_p=0.01)  # warm
        torch.cuda.synchronize()
        prev = torch.cuda.get_sync_debug_mode()
        torch.cuda.set_sync_debug_mode("error")
        try:
            more = m.decode_loop(m.decode_step(out[:, 0], cache), cache, 4, 0.8, 20, eos, g, top_p=0.9, min_p=0.01)
        finally:
            torch.cuda.set_sync_debug_mode(prev)
    assert more.shape == (3, 4)
    hits = 0
    for row in out.tolist():
        if eos in row:
            hits += 1
            assert all(t == eos for t in row[row.index(eos):])
    assert hits >= 1
