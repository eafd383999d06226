"""CPU: the comparison helpers of tests/_oracle_compare.py catch the faults they are there for, shown on synthetic
gradients - no GPU, no faulty kernel.  (What tests/test_gpu_full_batch_grads.py and the run-to-run bounds of
tests/test_gpu_determinism.py can and cannot see.)"""
import math

import pytest
import torch

from tests._oracle_compare import check_grad_rows, check_reorder, flip_cap, grad_rows, pooled_entries, reorder_bounds


def _sum_of_contributions(shape, parts, gen, scale=1.0):
    """A gradient that is the sum of `parts` independent contributions (clouds, groups): -> (the sum, one contribution)."""
    one = scale * torch.randn(shape, generator=gen, dtype=torch.float64)
    rest = scale * math.sqrt(parts - 1) * torch.randn(shape, generator=gen, dtype=torch.float64)
    return one + rest, one


def test_whole_gradient_check_resolution():
    g = torch.Generator().manual_seed(1)
    # three tensors: "big" carries most of the norm, "mid" ~10 %, "small" ~1 %
    ref = {"big": torch.randn(256, 131, generator=g, dtype=torch.float64),
           "mid": 0.1 * torch.randn(256, 131, generator=g, dtype=torch.float64),
           "small": 0.01 * torch.randn(256, 131, generator=g, dtype=torch.float64)}
    noise = {k: v * (1 + 1e-5 * torch.randn(v.shape, generator=g, dtype=torch.float64)) for k, v in ref.items()}
    rel = check_grad_rows(grad_rows((k, noise[k], ref[k]) for k in ref))           # fp32-sized noise passes
    assert rel < 2e-5
    # (1) one cloud of 64 missing from ONE tensor, ~ r / sqrt(64) = 12 % of its norm: the per-tensor bound fails, for the
    # heavy tensor and for the light one alike
    for name in ("big", "small"):
        full, one = _sum_of_contributions(ref[name].shape, 64, g, float(ref[name].std()) / 8)
        got = dict(noise)
        rows = grad_rows((k, (full - one) if k == name else got[k], full if k == name else ref[k]) for k in ref)
        e, r = [(e, r) for n_, e, r in rows if n_ == name][0]
        assert 0.08 < e / r < 0.18
        with pytest.raises(AssertionError) as info:
            check_grad_rows(rows)
        assert name in str(info.value)                                             # the failure names the tensor
    # (2) one group of 32768 missing from a weight gradient, ~ r / sqrt(32768) = 0.55 % of its norm: below the per-tensor
    # 1e-2, caught by the whole-gradient 2e-4 when the tensor carries more than 4 % of the total norm ...
    for name, caught in (("big", True), ("mid", True), ("small", False)):
        full, one = _sum_of_contributions(ref[name].shape, 32768, g, float(ref[name].std()) / math.sqrt(32768))
        rows = grad_rows((k, (full - one) if k == name else noise[k], full if k == name else ref[k]) for k in ref)
        e, r = [(e, r) for n_, e, r in rows if n_ == name][0]
        total = math.sqrt(sum(r_ * r_ for _, _, r_ in rows))
        assert 0.004 < e / r < 0.007 and (r / total > 0.04) == caught
        if caught:
            with pytest.raises(AssertionError) as info:
                check_grad_rows(rows)
            assert "whole gradient" in str(info.value) and name in str(info.value)
        else:
            check_grad_rows(rows)      # ... and NOT for a tensor that carries less: the resolution of the whole-step test
    # a missing gradient is a zero gradient
    assert grad_rows([("z", None, torch.ones(4))])[0][1:] == (2.0, 2.0)


def test_flip_allowance_scales_with_the_pooled_entries():
    assert pooled_entries(4) == 2 * (4 * 512 * 128 + 4 * 256 * 256 + 4 * 1024) + 4 * 64
    pins = {"flips": {"Encoder.sa1": (0, 0.0, 64 * 512 * 128), "Encoder.sa2": (1, 1e-7, 64 * 256 * 256),
                      "Encoder.gmax": (0, 0.0, 64 * 1024), "Encoder2.sa1": (0, 0.0, 64 * 512 * 128),
                      "Encoder2.sa2": (0, 0.0, 64 * 256 * 256), "Encoder2.gmax": (0, 0.0, 64 * 1024), "heads.gmax": (0, 0.0, 64 * 64)}}
    assert flip_cap(pins) == 256
    pins4 = {"flips": {"all": (0, 0.0, pooled_entries(4))}}
    assert flip_cap(pins4) == 16


def test_reorder_bound_passes_reordering_and_catches_a_lost_term():
    """n = 2560 rows (the small set-abstraction shape: 2 x 40 x 32) summed in fp32 in two random orders stay inside the
    8 sqrt(n) 2^-24 sum|t| bound; the same sum with ONE term missing leaves it (a term is ~ sum|t| / n, the bound
    8 sum|t| / (sqrt(n) 2^24): a lost term shows while n < 2^14 or so)."""
    n, cols = 2560, 512
    g = torch.Generator().manual_seed(2)
    t = torch.randn(n, cols, generator=g)
    sum_abs = t.double().abs().sum(0)

    def fp32_sum(order):
        acc = torch.zeros(cols)
        for i in order:                  # one fp32 addition at a time, in this order
            acc = acc + t[i]
        return acc

    a = fp32_sum(torch.randperm(n, generator=g).tolist())
    b = fp32_sum(torch.randperm(n, generator=g).tolist())
    assert not torch.equal(a, b)
    check_reorder("reordered", a, b, n, sum_abs)
    worst, walk = reorder_bounds(n, sum_abs)
    assert bool((walk < worst).all())
    order = torch.randperm(n, generator=g).tolist()
    lost = fp32_sum(order[1:])
    with pytest.raises(AssertionError):
        check_reorder("one term lost", lost, a, n, sum_abs)
    # nine entries in ten show it in the 8 sqrt(n) form (a term ~ sum|t| / n against 8 sum|t| / (sqrt(n) 2^24)); the worst-case
    # form alone sees the large terms only (a term exceeds it while n^2 < 2^23; here n^2 = 2^22.6)
    d = (lost.double() - a.double()).abs()
    assert float((d > walk).double().mean()) > 0.9
    assert float((d > worst).double().mean()) < 0.9
