"""The benchmarked step (fp32, B = 64 pairs, N = 2048, loss_mode 1: what bench.py times) against the oracle: loss, the
FPS picks, and the whole gradient entry by entry, with the bounds of
tests/test_gpu_model.py::test_training_step_full_gradients_vs_oracle (B = 4, N = 1024).  At this size the set-abstraction
levels have 32768 / 16384 groups instead of 2048 / 1024: other grids, 8 to 16 times as many partial tiles in the
fixed-order reductions of the pooled and attention weight gradients, the full depth of the LDS-DMA ring of
csrc/poolbwd.hip, hit lists of N = 2048 points in csrc/sapool.hip, other split-K factors."""
import gc
import os
import resource
import time

import numpy as np
import pytest
import torch

from oracle import model_ref as mr
from oracle import point_ops as orc
from tests._oracle_compare import _check_flips, _device_winners, check_grad_rows, flip_cap, grad_rows, pooled_entries

pytestmark = pytest.mark.gpu


def test_benchmarked_step_full_gradients_vs_oracle():
    """cfg = Cfg(num_points=2048, loss_mode=1), synthetic.make_batch(64, 2048, seed=2048), default precision (bf16x3),
    default set-abstraction path: one training_step + backward on the device, then the torch-CPU restatement on the same
    batch with the device's max-pool winners pinned (the flip-aware scheme of the B = 4 test), its EMD spread over
    min(16, cores) threads (oracle.point_ops.set_emd_threads: the one-thread bits).  Asserted: loss within 1e-4 relative;
    x2 of both clouds (FPS of FPS) bit-equal; every gradient finite; ||g - g_ref|| <= 2e-4 ||g_ref|| over all 8,059,220
    entries; every tensor e <= 1e-2 r + 1e-6 total; every flip a near-tie (gap <= 1e-5) and at most
    ceil(16 x pooled entries here / pooled entries at B = 4) of them.

    Resolution (tests/test_compare_helpers_cpu.py shows it on synthetic gradients): one cloud's contribution missing from
    one tensor is ~ r / sqrt(64) = 12 % of its norm and fails the per-tensor bound whatever the tensor.  One GROUP's
    contribution missing from a level's weight gradient is ~ r / sqrt(32768) = 0.55 % of its norm, below the per-tensor
    1e-2; it fails the whole-gradient 2e-4 only when that tensor carries more than 2e-4 / 0.0055 = 4 % of the total norm.
    For the tensors that carry less, a single lost group passes this test: faults that fine are the business of the
    stage tests (tests/test_gpu_dense.py, tests/test_gpu_pool_wgrad_bits.py) and of the run-to-run tests
    (tests/test_gpu_determinism.py).

    Measured on an MI355X host share of 16 cores: 16.6 s for the test (device step + backward 0.4 s, oracle forward 8.3 s with
    16 EMD threads, oracle backward 6.9 s), peak RSS 15.1 GB (the device side's graph is dropped before the oracle runs);
    loss 2047.05017 / 2047.05005; whole gradient 2.9e-5 relative in L2; worst tensor 1.3e-3 of its norm
    (Encoder.bn2.weight); 97 winners of 16,912,384 differ from the oracle's own arg-max (allowed 256), all near-ties.
    No tensor needed an exception to the B = 4 bounds."""
    from puzzlenet_amd import model5_b as mb, ops, synthetic
    dev = torch.device("cuda:0")
    B, N = 64, 2048
    cfg = mr.Cfg(num_points=N, loss_mode=1)
    ops.clear_grad_sinks()
    m = mb.TouchedRegraster(cfg)
    mr.fill_params(m)
    ref = mr.RefModel(cfg)
    ref.load_state_dict(m.state_dict(), strict=True)
    m.to(dev)
    assert m.Encoder.fused_sa and m.Encoder2.fused_sa
    batch = synthetic.make_batch(B, N, dev, seed=2048)
    cpu_batch = [t.cpu() for t in batch]
    picks = {}
    dev_predict = m.predict5
    m.predict5 = lambda *a, **k: picks.setdefault("dev", dev_predict(*a, **k))
    t0 = time.perf_counter()
    torch.manual_seed(2048)
    ops.WINNER_CAPTURE = []
    try:
        loss = m.training_step(batch, 0)["loss"]
        capture, ops.WINNER_CAPTURE = ops.WINNER_CAPTURE, None
    finally:
        ops.WINNER_CAPTURE = None
    winners = _device_winners(m, capture)
    loss.backward()
    torch.cuda.synchronize()
    dev_loss = loss.item()
    # the device side is read out and dropped before the oracle runs: its graph at 64 pairs takes the host's memory
    grads = {name: (None if p.grad is None else p.grad.detach().cpu()) for name, p in m.named_parameters()}
    x2_dev = (picks["dev"][2].detach().cpu().numpy(), picks["dev"][4].detach().cpu().numpy())
    del loss, capture, picks, m, dev_predict, batch
    gc.collect()
    torch.cuda.empty_cache()
    t1 = time.perf_counter()

    pins = ref.pin_winners(winners)
    rpicks = {}
    ref_predict = ref.predict5
    ref.predict5 = lambda *a, **k: rpicks.setdefault("ref", ref_predict(*a, **k))
    threads = min(16, len(os.sched_getaffinity(0)))
    with orc.emd_threads(threads):
        torch.manual_seed(2048)
        ref_loss = ref.training_step(cpu_batch)
        ref_loss = ref_loss[0] if isinstance(ref_loss, tuple) else ref_loss
        t2 = time.perf_counter()
        x2_ref = (rpicks["ref"][2].detach().numpy(), rpicks["ref"][4].detach().numpy())
        del rpicks
        ref_loss.backward()
    assert orc.get_emd_threads() == 1
    t3 = time.perf_counter()
    print(f"seconds: device step + backward {t1 - t0:.1f}, oracle forward {t2 - t1:.1f} ({threads} EMD threads), oracle backward "
          f"{t3 - t2:.1f}; peak RSS {resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 2 ** 20:.1f} GB")
    print("loss", dev_loss, ref_loss.item())

    assert np.array_equal(x2_dev[0], x2_ref[0]) and np.array_equal(x2_dev[1], x2_ref[1])      # FPS of FPS, both clouds
    here = sum(v[2] for v in pins["flips"].values())
    assert here == pooled_entries(B), (here, pooled_entries(B))
    cap = flip_cap(pins)
    _check_flips(pins, max_flips=cap)
    assert abs(dev_loss - ref_loss.item()) <= 1e-4 * abs(ref_loss.item()), (dev_loss, ref_loss.item())
    for name, g in grads.items():
        assert g is None or bool(torch.isfinite(g).all()), name
    rows = grad_rows((name, grads[name], p.grad) for name, p in ref.named_parameters())
    assert len(rows) == len(grads)
    total = sum(r * r for _, _, r in rows) ** 0.5
    for name, e, r in sorted(rows, key=lambda t: -t[1] / (t[2] + 1e-4 * total))[:8]:
        print(f"{name:40s} e {e:.3e} r {r:.3e} e/r {e / (r + 1e-30):.3e} share of total {r / total:.3f}")
    rel = check_grad_rows(rows)
    print("whole gradient: relative L2 error", rel)
