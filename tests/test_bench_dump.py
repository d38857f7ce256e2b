"""bench.py's options around the timed steps, CPU only: the side measurements are off unless
--full is given, and the --dump-outputs sampler keeps small arrays whole and cuts large ones to
the same seeded positions on every call."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402


def test_plain_run_flags_default_off():
    a = bench.parse(["--gpus", "1", "--steps", "3", "--warmup", "1"])
    assert a.full is False and a.dump_outputs is None and a.steps == 3 and a.warmup == 1
    a = bench.parse(["--full", "--dump-outputs", "d"])
    assert a.full is True and a.dump_outputs == "d"


def test_sampled_whole_under_budget():
    ts = [torch.arange(6, dtype=torch.float64).view(2, 3), torch.tensor([7, 8], dtype=torch.int64)]
    out = bench._sampled(ts, 8, seed=1)
    assert out.dtype == torch.float32 and out.tolist() == [0, 1, 2, 3, 4, 5, 7, 8]


def test_sampled_over_budget_fixed_positions():
    g = torch.Generator().manual_seed(0)
    ts = [torch.randn(1000, generator=g), torch.randn(30, 100, generator=g), torch.randn(3, generator=g)]
    a = bench._sampled(ts, 400, seed=3)
    b = bench._sampled([t.clone() for t in ts], 400, seed=3)
    assert torch.equal(a, b)  # same positions from call to call
    # each tensor by its share of the budget (at least one element), never more than the budget + one per tensor
    assert a.numel() == 1000 * 400 // 4003 + 3000 * 400 // 4003 + 1 and a.numel() <= 400 + len(ts)
    # the values are elements of the tensors, taken in order of position
    first = a[:1000 * 400 // 4003]
    pos = [int((ts[0] == v).nonzero()[0]) for v in first]
    assert pos == sorted(pos)
    assert bench.DUMP_BUDGET_BYTES == 64 * 2 ** 20
