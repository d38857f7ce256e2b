"""The plain causal / full gfx950 flash attention kernels (csrc/kernels/attention.hip) at the sequence
lengths tests/test_attention_gpu.py leaves out: non-causal S that is no multiple of the 64-key tile
(the only place the `key >= S` / `kj >= S` / `qq >= S` masks decide anything: under the causal mask
every key past S is already hidden from every valid query), S below one query block (128) and below
one key tile (64), S = 1, one key past a block (129, 65), and peaked scores.

Oracle: the per-head computation of tests/test_attention_gpu.py::_ref_per_head in float64, written out
from the formulas, on the same bf16 inputs. Errors are taken per row (o) and per head (gradients): a
single wrong row or head moves a whole-tensor norm by almost nothing. The bounds are the project's
O_TOL / G_TOL; per row a bf16-P, fp32-accumulate, bf16-out emulation stays at or below 3.1e-3 (o) and
2.8e-3 (gradients per head) at these shapes, so they test the kernel and not bf16. The oracle and the
input builder take a device and are checked on CPU by tests/test_lm_oracles_cpu.py.
"""
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
LSE_TOL = dict(atol=2e-3, rtol=1e-4)  # tests/test_attention_gpu.py::test_flash_attention_lse

# B, S, Hq, Hkv, D, causal, q scale. With nkt key tiles of 64 per 128-query block and `edge` the masked tiles:
CASES = [
    (1, 1, 4, 2, 64, True, 1),      # one query, one key: 1 of 128 lanes of the block live; dq = dk = 0
    (2, 1, 2, 2, 128, False, 1),    # the same, full attention, D = 128, B > 1
    (1, 63, 4, 2, 64, False, 1),    # S < one key tile: nkt = 1, edge by k0 + 64 > S alone
    (2, 65, 4, 2, 128, False, 1),   # one key into the second tile: nkt = 2, the last tile 1 key + 63 masked
    (1, 200, 4, 1, 128, False, 1),  # two query blocks, both read all nkt = 4 tiles, 8 keys live in the last
    (1, 129, 4, 2, 64, True, 1),    # second query / key block holds one row
    (1, 127, 2, 2, 128, True, 1),   # one row short of a block
    (1, 65, 8, 1, 64, True, 1),     # 8 query heads on one kv head, one row into the second key tile
    (1, 200, 4, 2, 64, True, 8),    # peaked: scores 8x, softmax close to one-hot (o, lse, finite gradients)
]
TWO_LAUNCH = 5  # the causal case run again under CS_ATTN_BWD_FUSED=0: attn_dq_kernel + attn_dkdv_kernel


def _cid(case):
    B, S, Hq, Hkv, D, causal, qs = case
    return f"{B}x{S}x{Hq}x{Hkv}x{D}-{'causal' if causal else 'full'}" + (f"-q{qs}" if qs != 1 else "")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cs744_pytorch_distributed_tutorial_amd.ops import native
    native.C()
    return torch.device("cuda", 0)


def inputs(i, device):
    """bf16 q, k, v, do of case i (the construction of tests/test_attention_gpu.py; q times the case's
    power-of-two scale, exact in bf16)"""
    B, S, Hq, Hkv, D, _, qs = CASES[i]
    g = torch.Generator(device=device).manual_seed(B * 1000 + S + D)
    q = (torch.randn(B, S, Hq, D, device=device, generator=g) * qs).bfloat16()
    k = torch.randn(B, S, Hkv, D, device=device, generator=g).bfloat16()
    v = torch.randn(B, S, Hkv, D, device=device, generator=g).bfloat16()
    do = torch.randn(B, S, Hq, D, device=device, generator=g).bfloat16()
    return q, k, v, do


def attention_oracle(q, k, v, do, causal):
    """float64, one (batch, head) at a time: o, the base-2 row log-sum-exp of the scaled scores
    [B, Hq, S], dq, dk, dv (dk / dv summed over the query heads of a kv head).
    P = softmax(Q K^T / sqrt(D) + mask); O = P V; dV = P^T dO; dP = dO V^T;
    dS = P (dP - rowsum(dO O)); dQ = dS K / sqrt(D); dK = dS^T Q / sqrt(D)."""
    B, S, Hq, D = q.shape
    Hkv = k.shape[2]
    rep = Hq // Hkv
    scale = 1.0 / math.sqrt(D)
    f = dict(dtype=torch.float64, device=q.device)
    o, dq = torch.empty(B, S, Hq, D, **f), torch.empty(B, S, Hq, D, **f)
    dk, dv = torch.zeros(B, S, Hkv, D, **f), torch.zeros(B, S, Hkv, D, **f)
    lse = torch.empty(B, Hq, S, **f)
    hidden = torch.ones(S, S, dtype=torch.bool, device=q.device).triu(1) if causal else None
    for b in range(B):
        for h in range(Hq):
            qh, kh, vh, gh = q[b, :, h].double(), k[b, :, h // rep].double(), v[b, :, h // rep].double(), do[b, :, h].double()
            s = (qh @ kh.t()) * scale
            if hidden is not None:
                s = s.masked_fill(hidden, float("-inf"))
            l = torch.logsumexp(s, -1)
            p = torch.exp(s - l[:, None])
            oh = p @ vh
            ds = p * (gh @ vh.t() - (gh * oh).sum(-1, keepdim=True))
            o[b, :, h], lse[b, h] = oh, l / math.log(2.0)
            dq[b, :, h] = ds @ kh * scale
            dk[b, :, h // rep] += ds.t() @ qh * scale
            dv[b, :, h // rep] += p.t() @ gh
    return o, lse, dq, dk, dv


@functools.lru_cache(maxsize=None)
def _reference(i):
    """the oracle of case i on the GPU: computed once, never written to"""
    return attention_oracle(*inputs(i, torch.device("cuda", 0)), CASES[i][5])


def _run(q, k, v, do, causal):
    """native forward + backward -> o, lse, dq, dk, dv"""
    from cs744_pytorch_distributed_tutorial_amd import _C
    from cs744_pytorch_distributed_tutorial_amd.ops.attention import attention, native_ok
    q, k, v = (t.detach().clone().requires_grad_() for t in (q, k, v))
    assert native_ok(q, k, v)
    o = attention(q, k, v, causal)
    o.backward(do)
    lse = _C.attn_fwd(q.detach(), k.detach(), v.detach(), 1.0 / math.sqrt(q.shape[-1]), causal)[1]
    return o.detach(), lse, q.grad, k.grad, v.grad


def _rel_over(a, r, dims):
    """worst relative L2 error over slices: norms taken over `dims`, the maximum over the rest"""
    a, r = a.double(), r.double()
    return float(((a - r).norm(dim=dims) / r.norm(dim=dims).clamp_min(1e-12)).max())


def _check(i, got, tag=""):
    B, S, Hq, Hkv, D, causal, qs = CASES[i]
    q, k, v, do = inputs(i, got[0].device)
    o, lse, dq, dk, dv = got
    ro, rlse, rdq, rdk, rdv = _reference(i)
    for name, t in zip(("o", "lse", "dq", "dk", "dv"), got):
        assert bool(torch.isfinite(t.float()).all()), name
    errs = {"o": _rel_over(o, ro, (3,)), "lse": float((lse.double() - rlse).abs().max())}
    bounds = {"o": O_TOL}
    if qs == 1:
        errs["dv"], bounds["dv"] = _rel_over(dv, rdv, (1, 3)), G_TOL
        if S > 1:
            errs["dq"], bounds["dq"] = _rel_over(dq, rdq, (1, 3)), G_TOL
            errs["dk"], bounds["dk"] = _rel_over(dk, rdk, (1, 3)), G_TOL
        else:
            # one key: P = 1, dS = dP - delta = dO.v - dO.o with o = v, exactly 0; the kernel sums the
            # two D-term products in different orders in fp32, each within D 2^-24 max|dO| max|v| of the
            # exact value; dq = dS k / sqrt(D), dk = dS q / sqrt(D); factor 4: both sums, and margin
            assert not bool(rdq.any()) and not bool(rdk.any())
            amax = lambda t: float(t.float().abs().max())  # noqa: E731
            zb = 4 * D * 2.0 ** -24 * amax(do) * amax(v) * max(amax(q), amax(k)) / math.sqrt(D)
            errs["dq"], bounds["dq"] = amax(dq), zb
            errs["dk"], bounds["dk"] = amax(dk), zb
    print(f"[attn-edges] {tag}case {i} {_cid(CASES[i])}: " +
          " ".join(f"{n} {e:.3e}" + (f" (< {bounds[n]:.1e})" if n in bounds else "") for n, e in errs.items()))
    torch.testing.assert_close(lse.double(), rlse, **LSE_TOL)
    for n, bnd in bounds.items():
        assert errs[n] <= bnd if S == 1 and n in ("dq", "dk") else errs[n] < bnd, (n, errs[n], bnd)
    return errs


@pytest.mark.parametrize("i", range(len(CASES)), ids=[_cid(c) for c in CASES])
def test_attention_edge_shapes(dev, i):
    q, k, v, do = inputs(i, dev)
    _check(i, _run(q, k, v, do, CASES[i][5]))


def two_launch_child():
    """Runs in a fresh process with CS_ATTN_BWD_FUSED=0 (the switch is read once per process)."""
    assert os.environ.get("CS_ATTN_BWD_FUSED") == "0"
    q, k, v, do = inputs(TWO_LAUNCH, torch.device("cuda", 0))
    errs = _check(TWO_LAUNCH, _run(q, k, v, do, True), tag="two-launch ")
    print("ATTN_EDGES_TWO_LAUNCH_OK " + " ".join(f"{n}={e:.3e}" for n, e in errs.items()))


def test_causal_two_launch_backward(dev):
    assert CASES[TWO_LAUNCH][:6] == (1, 129, 4, 2, 64, True)
    code = f"import sys; sys.path.insert(0, {os.path.join(ROOT, 'tests')!r}); " \
           "import test_attention_edges_gpu as t; t.two_launch_child()"
    env = dict(os.environ, CS_ATTN_BWD_FUSED="0", PYTHONPATH=ROOT)
    p = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, capture_output=True, text=True, timeout=110)
    assert p.returncode == 0, p.stdout[-1000:] + p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("ATTN_EDGES_TWO_LAUNCH_OK")]
    assert len(lines) == 1, p.stdout[-2000:]
    print(lines[0])
