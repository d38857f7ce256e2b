"""Document-masked gfx950 flash attention (csrc/kernels/attention.hip, the DOC kernels) for packed
sequences: against the fp32 reference with the same mask (oracle and tolerances of
tests/test_attention_gpu.py), bitwise against the causal kernels where the tile sequence is the
same, isolation of documents, the two-launch backward, hostile bound arrays, and the trainer."""
import functools
import math
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

O_TOL, G_TOL = 8e-3, 1.5e-2  # relative L2 error: o; dq, dk, dv (tests/test_attention_gpu.py)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cs744_pytorch_distributed_tutorial_amd.ops import native
    native.C()
    return torch.device("cuda", 0)


def _rel(a, b):
    return ((a.float() - b.float()).norm() / b.float().norm().clamp_min(1e-12)).item()


CASES = [  # B, S, Hq, Hkv, D, document lengths per row
    # boundaries inside a 64-key tile and inside a 128-query block; rows differ
    (2, 320, 4, 2, 64, [[5, 100, 130, 85], [320]]),
    # the last query block starts its key loop at tile 3 (a skipped prefix longer than one buffer
    # cycle); dK/dV of key block 0 stops before S
    (1, 384, 8, 2, 128, [[200, 184]]),
    # ragged S together with a mask
    (1, 200, 4, 1, 128, [[70, 130]]),
    # one-token documents (every query sees only itself), then a long one
    (1, 256, 4, 4, 64, [[1] * 64 + [192]]),
]


def _doc_ids(lens, device):
    return torch.tensor([[d for d, n in enumerate(row) for _ in range(n)] for row in lens], device=device)


def _inputs(i, device):
    B, S, Hq, Hkv, D, lens = CASES[i]
    assert all(sum(row) == S for row in lens) and len(lens) == B
    g = torch.Generator(device=device).manual_seed(B * 1000 + S + D)
    q = torch.randn(B, S, Hq, D, device=device, generator=g).bfloat16()
    k = torch.randn(B, S, Hkv, D, device=device, generator=g).bfloat16()
    v = torch.randn(B, S, Hkv, D, device=device, generator=g).bfloat16()
    do = torch.randn(B, S, Hq, D, device=device, generator=g).bfloat16()
    return q, k, v, do


def _run(q, k, v, do, doc):
    """native forward + backward -> o, dq, dk, dv"""
    from cs744_pytorch_distributed_tutorial_amd.ops.attention import attention, native_ok
    q, k, v = (t.detach().clone().requires_grad_() for t in (q, k, v))
    assert native_ok(q, k, v)
    o = attention(q, k, v, True, doc)
    o.backward(do)
    return o.detach(), q.grad, k.grad, v.grad


def _lse(q, k, v, doc):
    from cs744_pytorch_distributed_tutorial_amd import _C
    scale = 1.0 / math.sqrt(q.shape[-1])
    return _C.attn_fwd(q, k, v, scale, True, *doc)[1] if doc is not None else _C.attn_fwd(q, k, v, scale, True)[1]


@functools.lru_cache(maxsize=None)
def _reference(i):
    """fp32 attention_ref(..., doc=...) of case i and its gradients: computed once, never written to"""
    from cs744_pytorch_distributed_tutorial_amd.ops.attention import attention_ref, doc_bounds
    device = torch.device("cuda", 0)
    q, k, v, do = _inputs(i, device)
    doc = doc_bounds(_doc_ids(CASES[i][5], device))
    qr, kr, vr = (t.float().requires_grad_() for t in (q, k, v))
    o = attention_ref(qr, kr, vr, True, doc)
    o.backward(do.float())
    return o.detach(), qr.grad, kr.grad, vr.grad


def _check_against_reference(i, got):
    names, tols = ("o", "dq", "dk", "dv"), (O_TOL, G_TOL, G_TOL, G_TOL)
    errs = {n: _rel(a, r) for n, a, r in zip(names, got, _reference(i))}
    print(f"[docmask] case {i} {CASES[i][:5]}: " + " ".join(f"{n} {e:.3e}" for n, e in errs.items()))
    for n, a, t in zip(names, got, tols):
        assert torch.isfinite(a.float()).all(), n
        assert errs[n] < t, (n, errs[n])
    return errs


@pytest.mark.parametrize("i", range(len(CASES)))
def test_docmask_matches_reference(dev, i):
    from cs744_pytorch_distributed_tutorial_amd.ops.attention import doc_bounds
    q, k, v, do = _inputs(i, dev)
    doc = doc_bounds(_doc_ids(CASES[i][5], dev))
    _check_against_reference(i, _run(q, k, v, do, doc))


def test_one_document_is_the_causal_kernel(dev):
    """A mask of one document per row walks the same tiles with the same arithmetic: bitwise equal."""
    from cs744_pytorch_distributed_tutorial_amd.ops.attention import doc_bounds
    B, S, Hq, Hkv, D = 1, 320, 4, 2, 128
    g = torch.Generator(device=dev).manual_seed(1)
    q = torch.randn(B, S, Hq, D, device=dev, generator=g).bfloat16()
    k = torch.randn(B, S, Hkv, D, device=dev, generator=g).bfloat16()
    v = torch.randn(B, S, Hkv, D, device=dev, generator=g).bfloat16()
    do = torch.randn(B, S, Hq, D, device=dev, generator=g).bfloat16()
    doc = doc_bounds(torch.zeros(B, S, dtype=torch.long, device=dev))
    assert int(doc.kstart.max()) == 0 and int(doc.qend.min()) == S
    plain, masked = _run(q, k, v, do, None), _run(q, k, v, do, doc)
    for name, a, b in zip(("o", "dq", "dk", "dv"), masked, plain):
        assert torch.equal(a, b), name
    assert torch.equal(_lse(q, k, v, doc), _lse(q, k, v, None))


@pytest.mark.parametrize("D", [64, 128])
def test_aligned_packing_is_exact(dev, D):
    """Documents that start on 128-token boundaries see the tiles they would see alone, in the same
    order: outputs and gradients at a document's positions equal its own causal run bitwise."""
    from cs744_pytorch_distributed_tutorial_amd.ops.attention import doc_bounds
    B, S, Hq, Hkv, lens = 1, 384, 4, 2, [128, 256]
    g = torch.Generator(device=dev).manual_seed(D)
    q = torch.randn(B, S, Hq, D, device=dev, generator=g).bfloat16()
    k = torch.randn(B, S, Hkv, D, device=dev, generator=g).bfloat16()
    v = torch.randn(B, S, Hkv, D, device=dev, generator=g).bfloat16()
    do = torch.randn(B, S, Hq, D, device=dev, generator=g).bfloat16()
    doc = doc_bounds(_doc_ids([lens], dev))
    packed = _run(q, k, v, do, doc)
    lse = _lse(q, k, v, doc)
    s0 = 0
    for n in lens:
        sl = slice(s0, s0 + n)
        part = [t[:, sl].contiguous() for t in (q, k, v, do)]
        alone = _run(*part, None)
        for name, a, b in zip(("o", "dq", "dk", "dv"), packed, alone):
            assert torch.equal(a[:, sl], b), (name, s0)
        assert torch.equal(lse[:, :, sl], _lse(*part[:3], None)), s0
        s0 += n


def test_documents_are_isolated(dev):
    from cs744_pytorch_distributed_tutorial_amd.ops.attention import doc_bounds
    q, k, v, do = _inputs(0, dev)
    lens = CASES[0][5]
    doc = doc_bounds(_doc_ids(lens, dev))
    n0 = lens[0][0]  # row 0's document 0 (row 1 is a single document: left alone)
    o, lse = _run(q, k, v, do, doc)[0], _lse(q, k, v, doc)
    g = torch.Generator(device=dev).manual_seed(99)
    q2, k2, v2 = q.clone(), k.clone(), v.clone()
    for t in (q2, k2, v2):
        t[0, :n0] = torch.randn(t[0, :n0].shape, device=dev, generator=g).bfloat16() * 3
    o2, lse2 = _run(q2, k2, v2, do, doc)[0], _lse(q2, k2, v2, doc)
    assert not torch.equal(o[0, :n0], o2[0, :n0])
    assert torch.equal(o[0, n0:], o2[0, n0:]) and torch.equal(o[1], o2[1])
    assert torch.equal(lse[0, :, n0:], lse2[0, :, n0:]) and torch.equal(lse[1], lse2[1])
    # no gradient arrives at document 0's positions: its keys are seen by its own queries only
    do0 = do.clone()
    do0[0, :n0] = 0
    _, _, dk, dv = _run(q, k, v, do0, doc)
    assert bool((dk[0, :n0] == 0).all()) and bool((dv[0, :n0] == 0).all())
    assert bool((dk[0, n0:] != 0).any()) and bool((dv[0, n0:] != 0).any())


def two_launch_child():
    """Runs in a fresh process with CS_ATTN_BWD_FUSED=0 (the switch is read once per process)."""
    from cs744_pytorch_distributed_tutorial_amd.ops.attention import doc_bounds
    assert os.environ.get("CS_ATTN_BWD_FUSED") == "0"
    device = torch.device("cuda", 0)
    q, k, v, do = _inputs(1, device)
    doc = doc_bounds(_doc_ids(CASES[1][5], device))
    errs = _check_against_reference(1, _run(q, k, v, do, doc))
    print("DOCMASK_TWO_LAUNCH_OK " + " ".join(f"{n}={e:.3e}" for n, e in errs.items()))


def test_two_launch_backward(dev):
    code = f"import sys; sys.path.insert(0, {os.path.join(ROOT, 'tests')!r}); " \
           "import test_attention_docmask_gpu as t; t.two_launch_child()"
    env = dict(os.environ, CS_ATTN_BWD_FUSED="0", PYTHONPATH=ROOT)
    p = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, capture_output=True, text=True, timeout=110)
    assert p.returncode == 0, p.stdout[-1000:] + p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("DOCMASK_TWO_LAUNCH_OK")]
    assert len(lines) == 1, p.stdout[-2000:]
    print(lines[0])


def test_inconsistent_bounds_are_clamped(dev):
    """kstart beyond the row and qend before it: the kernels clamp both (kstart into [0, i], qend into
    [j + 1, S]), so every call returns and writes finite values. No meaning is checked."""
    from cs744_pytorch_distributed_tutorial_amd import _C
    B, S, Hq, Hkv, D = 2, 200, 4, 2, 64
    g = torch.Generator(device=dev).manual_seed(5)
    q = torch.randn(B, S, Hq, D, device=dev, generator=g).bfloat16()
    k = torch.randn(B, S, Hkv, D, device=dev, generator=g).bfloat16()
    v = torch.randn(B, S, Hkv, D, device=dev, generator=g).bfloat16()
    do = torch.randn(B, S, Hq, D, device=dev, generator=g).bfloat16()
    kstart = torch.full((B, S), S + 5, dtype=torch.int32, device=dev)
    qend = torch.zeros(B, S, dtype=torch.int32, device=dev)
    scale = 1.0 / math.sqrt(D)
    o, lse = _C.attn_fwd(q, k, v, scale, True, kstart, qend)
    torch.cuda.synchronize()
    assert o.shape == q.shape and lse.shape == (B, Hq, S)
    assert bool(torch.isfinite(o.float()).all())
    dq, dk, dv = _C.attn_bwd(q, k, v, o, lse, do, scale, True, kstart, qend)
    torch.cuda.synchronize()
    for t, like in ((dq, q), (dk, k), (dv, v)):
        assert t.shape == like.shape and bool(torch.isfinite(t.float()).all())


def test_binding_refuses_bad_bounds(dev):
    from cs744_pytorch_distributed_tutorial_amd import _C
    B, S, H, D = 2, 128, 2, 64
    q = torch.randn(B, S, H, D, device=dev).bfloat16()
    ok = torch.zeros(B, S, dtype=torch.int32, device=dev)
    short = ok[:, :64].contiguous()
    bad = [(ok.long(), ok, True, "int32"), (ok, ok.cpu(), True, "device"), (short, short, True, "shaped"),
           (ok.t().contiguous().t(), ok, True, "contiguous"), (ok, ok, False, "causal")]
    for ks, qe, causal, word in bad:
        with pytest.raises(RuntimeError, match=word):
            _C.attn_fwd(q, q, q, 0.125, causal, ks, qe)
    with pytest.raises(RuntimeError, match="together"):
        _C.attn_fwd(q, q, q, 0.125, True, ok, None)


def test_trainer_learns_on_packed_documents(dev, monkeypatch):
    """The AdamW training setting of tests/test_adamw_gpu.py with documents of about 32 tokens packed
    into every row: the loss falls below its first value and below ln(1024) = 6.93, uniform prediction."""
    from cs744_pytorch_distributed_tutorial_amd.ops.attention import doc_ids_from_eos
    from cs744_pytorch_distributed_tutorial_amd.runtime.torch_trainer import SyntheticBatches, TorchTrainer
    for key in ("CS744_OPTIMIZER", "CS744_LR", "CS744_WEIGHT_DECAY", "CS744_MAX_GRAD_NORM", "CS744_GRAD_COMM_DTYPE",
                "CS744_DOC_LEN"):
        monkeypatch.delenv(key, raising=False)
    seed = 5000
    tr = TorchTrainer("llama-tiny", batch_size=8, device=dev, dtype="bf16", optimizer="adamw", lr=3e-4,
                      weight_decay=0.1, max_grad_norm=1.0, doc_len=32, seed=seed)
    assert tr.doc_len == 32 and tr.eos_id == 1023
    seq = tr.data.tokens.shape[1] - 1
    tr.data = SyntheticBatches("tokens", 8, dev, seq=seq, vocab=1024, pool=8, seed=seed, doc_len=32, eos_id=tr.eos_id)
    x = tr.data.tokens[:, :-1]  # every step's inputs are rows of this pool
    n_docs = doc_ids_from_eos(x, tr.eos_id)[:, -1] + 1
    assert int(n_docs.min()) >= 2, n_docs
    losses = []
    for _ in range(50):
        tr.step()
        losses.append(tr.loss)
    losses = torch.stack(losses).float().cpu()
    print(f"[docmask] trainer: first {float(losses[0]):.3f} last {float(losses[-1]):.3f}")
    assert bool(torch.isfinite(losses).all())
    assert float(losses[-1]) < float(losses[0])
    assert float(losses[-1]) < math.log(1024)
