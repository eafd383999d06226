"""Helpers shared by the tests that compare a whole training_step with the torch-CPU restatement (oracle/model_ref.py) and
by the run-to-run tests of tests/test_gpu_determinism.py.  An ordinary module (no fixtures, no hooks); its arithmetic is
checked without a GPU by tests/test_compare_helpers_cpu.py."""
import math

import pytest
import torch


def _device_winners(m, capture):
    """ops.WINNER_CAPTURE of one forward of the product model -> the keys oracle.model_ref.RefModel.pin_winners takes."""
    from puzzlenet_amd import _lib
    if _lib.load().pzn_gemm_get_precision() == 0:
        # (PZN_GEMM_PRECISION=f32: the encoders' global max then goes through the plain max over points, whose captures carry no
        # owner - three of them could not be told apart below; the fingerprint test covers that mode)
        pytest.skip("the winner pinning needs the split-precision paths' captures (default mode)")
    owner = {}
    for tag, enc in (("Encoder.", m.Encoder), ("Encoder2.", m.Encoder2)):
        owner[enc.mlp4.weight.data_ptr()] = tag + "sa1"
        owner[enc.mlp6.weight.data_ptr()] = tag + "sa2"
        owner[enc.out.weight.data_ptr()] = tag + "gmax"
    win = {}
    for kind, ptr, arg in capture:
        key = "heads.gmax" if kind == "maxpts" else owner[ptr]
        assert key not in win, key
        win[key] = arg.detach().cpu().to(torch.long)
    assert len(win) == 7, sorted(win)
    return win


def _check_flips(pins, max_flips=16, max_gap=1e-5):
    """The oracle's own arg-max differs from the pinned (device) winner only on near-ties: a handful of entries, each with
    the two candidates closer than fp32 rounding of the sums in front of them."""
    total = 0
    for key, (n, gap, of) in sorted(pins["flips"].items()):
        total += n
        assert gap <= max_gap, (key, n, gap)
    print("max-pool winners that differ from the oracle's own:", {k: v[0] for k, v in pins["flips"].items() if v[0]}, "of",
          sum(v[2] for v in pins["flips"].values()))
    assert total <= max_flips, pins["flips"]
    return total


def pooled_entries(B, N=None):
    """Max-pool outputs of one training_step (the `of` fields of pins["flips"] summed): per encoder the two set-abstraction
    levels (S = 512 groups x 128 channels, 256 x 256) and the global max (1024 channels), plus the heads' max (64)."""
    return 2 * (B * 512 * 128 + B * 256 * 256 + B * 1024) + B * 64


def flip_cap(pins):
    """The flip allowance of test_training_step_full_gradients_vs_oracle (16 among the pooled entries of B = 4) as the same
    share of this case's pooled entries."""
    here = sum(v[2] for v in pins["flips"].values())
    return math.ceil(16 * here / pooled_entries(4))


def grad_rows(pairs):
    """[(name, g, g_ref)] -> [(name, e = ||g - g_ref||, r = ||g_ref||)] in float64 (None = a zero gradient)."""
    rows = []
    for name, g, gr in pairs:
        g = torch.zeros(1, dtype=torch.float64) if g is None else g.detach().cpu().double()
        gr = torch.zeros(1, dtype=torch.float64) if gr is None else gr.detach().cpu().double()
        rows.append((name, float((g - gr).norm()), float(gr.norm())))
    return rows


def check_grad_rows(rows, whole=2e-4, per_tensor=1e-2, floor=1e-6):
    """The bounds of test_training_step_full_gradients_vs_oracle on rows of grad_rows(): the whole gradient within `whole`
    of its norm in L2, every tensor e <= per_tensor r + floor total.
    A failure names the tensor with e and r, worst tensors first.  -> the whole-gradient relative error."""
    total = math.sqrt(sum(r * r for _, _, r in rows))
    err = math.sqrt(sum(e * e for _, e, _ in rows))
    worst = sorted(rows, key=lambda t: -t[1] / (t[2] + floor / per_tensor * total))[:5]
    assert err <= whole * total, ("whole gradient", err / total, "worst tensors (name, e, r)", worst)
    for name, e, r in rows:
        assert e <= per_tensor * r + floor * total, (name, e, r)
    return err / max(total, 1e-300)


def reorder_bounds(n, sum_abs):
    """Two fp32 sums of the same `n` terms in different orders: each addition rounds by at most 2^-24 of the running sum,
    which never exceeds sum|t_i| -> (the worst case 2 n 2^-24 sum|t_i|, the random-walk form with a margin of 8 over its
    standard deviation, 8 sqrt(n) 2^-24 sum|t_i|).  `sum_abs`: float64 tensor of sum|t_i| per entry."""
    u = 2.0 ** -24
    return 2.0 * n * u * sum_abs, 8.0 * math.sqrt(n) * u * sum_abs


def check_reorder(name, a, b, n, sum_abs):
    """|a - b| entrywise within both bounds of reorder_bounds (a, b: two runs' fp32 results; sum_abs as there)."""
    worst, walk = reorder_bounds(n, sum_abs.double())
    d = (a.double() - b.double()).abs()
    assert bool((d <= worst).all()), (name, "worst-case bound", float((d - worst).max()))
    assert bool((d <= walk).all()), (name, "8 sqrt(n) bound", float((d / walk.clamp_min(1e-300)).max()))
