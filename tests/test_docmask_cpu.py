"""Document masks for packed LM sequences, the host side: ids from EOS tokens, the two bound arrays
the kernels read, the reference attention with a mask (the oracle of tests/test_attention_docmask_gpu.py),
isolation of documents in the model, and the synthetic packed token pool."""
import pytest
import torch


def _ids_from_lengths(rows):
    return torch.tensor([[d for d, n in enumerate(lens) for _ in range(n)] for lens in rows])


def test_doc_ids_from_eos_hand_written_rows():
    from cs744_pytorch_distributed_tutorial_amd.ops.attention import doc_ids_from_eos
    E = 9
    tokens = torch.tensor([
        [E, 1, 2, 3, 4, 5, 6, 7],  # EOS at position 0: a one-token document
        [1, 2, E, E, 3, 4, 5, 6],  # two adjacent EOS: the second is a document of its own
        [1, 2, 3, 4, 5, 6, 7, E],  # EOS at the last position closes the only document
        [1, 2, 3, 4, 5, 6, 7, 8],  # no EOS
    ])
    want = torch.tensor([
        [0, 1, 1, 1, 1, 1, 1, 1],
        [0, 0, 0, 1, 2, 2, 2, 2],
        [0, 0, 0, 0, 0, 0, 0, 0],
        [0, 0, 0, 0, 0, 0, 0, 0],
    ])
    got = doc_ids_from_eos(tokens, E)
    assert got.dtype == torch.int64 and torch.equal(got, want)


def test_doc_bounds_hand_written_and_errors():
    from cs744_pytorch_distributed_tutorial_amd.ops.attention import DocBounds, attention, attention_ref, doc_bounds
    ids = torch.tensor([[0, 0, 0, 1, 1, 2, 2, 2],
                        [4, 4, 4, 4, 4, 4, 4, 7]])  # ids need not start at 0 or be consecutive
    want_ks = torch.tensor([[0, 0, 0, 3, 3, 5, 5, 5], [0, 0, 0, 0, 0, 0, 0, 7]], dtype=torch.int32)
    want_qe = torch.tensor([[3, 3, 3, 5, 5, 8, 8, 8], [7, 7, 7, 7, 7, 7, 7, 8]], dtype=torch.int32)
    for dt in (torch.int64, torch.int32, torch.uint8):
        b = doc_bounds(ids.to(dt))
        assert isinstance(b, DocBounds)
        for got, want in ((b.kstart, want_ks), (b.qend, want_qe)):
            assert got.dtype == torch.int32 and got.is_contiguous() and got.device == ids.device
            assert torch.equal(got, want)
    with pytest.raises(ValueError):
        doc_bounds(torch.tensor([[0, 0, 1, 1], [0, 1, 0, 1]]))
    q = torch.randn(2, 8, 2, 16)
    with pytest.raises(ValueError):
        attention(q, q, q, causal=False, doc=b)
    with pytest.raises(ValueError):
        attention_ref(q, q, q, causal=False, doc=b)


def test_attention_ref_with_doc_equals_per_document_attention():
    from cs744_pytorch_distributed_tutorial_amd.ops.attention import attention, attention_ref, doc_bounds
    B, S, Hq, Hkv, D = 2, 96, 4, 2, 16
    lens = [[1, 40, 55], [96]]
    g = torch.Generator().manual_seed(0)
    q = torch.randn(B, S, Hq, D, generator=g)
    k = torch.randn(B, S, Hkv, D, generator=g)
    v = torch.randn(B, S, Hkv, D, generator=g)
    doc = doc_bounds(_ids_from_lengths(lens))
    o = attention_ref(q, k, v, True, doc)
    assert torch.equal(attention(q, k, v, True, doc), o)  # the op's CPU path is the reference
    for b in range(B):
        parts, s0 = [], 0
        for n in lens[b]:
            sl = slice(s0, s0 + n)
            parts.append(attention_ref(q[b:b + 1, sl], k[b:b + 1, sl], v[b:b + 1, sl], True))
            s0 += n
        torch.testing.assert_close(o[b:b + 1], torch.cat(parts, 1))
    assert torch.equal(o[1:2], attention_ref(q[1:2], k[1:2], v[1:2], True))  # one document: the causal op, bitwise


def test_model_isolates_documents():
    from cs744_pytorch_distributed_tutorial_amd.models.llama import CONFIGS, build
    from cs744_pytorch_distributed_tutorial_amd.ops.attention import doc_ids_from_eos
    torch.manual_seed(0)
    m = build("llama-tiny").eval()
    eos = CONFIGS["llama-tiny"].eos_id
    assert eos == m.vocab_size - 1 and CONFIGS["llama3-8b"].eos_id == 128001
    g = torch.Generator().manual_seed(1)
    a = torch.randint(0, eos, (1, 64), generator=g)  # no EOS among them
    a[0, 29] = eos  # documents of 30 and 34 tokens
    b = a.clone()
    b[0, :29] = (a[0, :29] + 1 + torch.randint(0, eos - 1, (29,), generator=g)) % eos  # other non-EOS tokens
    assert not (a[0, :29] == b[0, :29]).any() and not (b[0, :29] == eos).any()
    ids = doc_ids_from_eos(a, eos)
    assert torch.equal(ids, doc_ids_from_eos(b, eos)) and ids[0, 29] == 0 and ids[0, 30] == 1
    with torch.no_grad():
        la, lb = m(a, doc_ids=ids), m(b, doc_ids=ids)
        assert torch.equal(la[:, 30:], lb[:, 30:])  # bitwise: masked probabilities are exact zeros
        assert not torch.equal(la[:, :30], lb[:, :30])
        pa, pb = m(a), m(b)  # negative control: without the mask document 0 leaks into document 1
        assert not torch.equal(pa[:, 30:], pb[:, 30:])
        assert torch.equal(m(a, doc_ids=None), pa)


def test_synthetic_batches_with_documents():
    from cs744_pytorch_distributed_tutorial_amd.ops.attention import doc_ids_from_eos
    from cs744_pytorch_distributed_tutorial_amd.runtime.torch_trainer import SyntheticBatches, TorchTrainer
    cpu = torch.device("cpu")
    N, E, V, seq = 16, 99, 100, 127
    mk = lambda **kw: SyntheticBatches("tokens", 4, cpu, seq=seq, vocab=V, pool=32, seed=7, **kw)
    d1, d2 = mk(doc_len=N, eos_id=E), mk(doc_len=N, eos_id=E)
    assert torch.equal(d1.tokens, d2.tokens)  # deterministic for a seed
    x1, y1 = d1.next()
    x2, y2 = d2.next()
    assert torch.equal(x1, x2) and torch.equal(y1, y2)
    hi = 3 * N // 2
    ids = doc_ids_from_eos(d1.tokens, E)
    for row in ids:
        lens = torch.bincount(row)
        assert int(lens.min()) >= 1 and int(lens.max()) <= hi
        assert len(lens) >= (seq + 1) // hi > 1
    # without doc_len: the pool of the code before documents existed (its construction, spelled out)
    g = torch.Generator(device="cpu").manual_seed(7)
    assert torch.equal(mk().tokens, torch.randint(0, V, (32, seq + 1), generator=g))
    # where a position is not an EOS the packed pool has the undivided pool's token
    keep = d1.tokens != E
    assert torch.equal(d1.tokens[keep], mk().tokens[keep])
    with pytest.raises(ValueError):
        TorchTrainer("vgg11", 2, cpu, doc_len=16)
