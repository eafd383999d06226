"""The pooled level's backward keeps its bits.

* The weight-gradient pass on regenerated rows (relu(P'[idx] + Q) applied at the hit, rows staged in LDS by DMA) gives dW2
  and db2 equal to the same pass on rows that torch materialised, at both production shapes.  Both sides walk the same
  groups in the same order into the same fixed-order reduction, so nothing but the gate's place differs.
* The whole backward of the level at B = 2 equals what the build before the LDS-DMA ring recorded
  (tests/golden/make_golden_pool_bwd.py): bit for bit where the sums have a fixed order (the feature gradient, which carries
  dP, and dW2, db2), to summation-order noise where the walk by point adds with atomics (dW1[:, 0:3], db1)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _p(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else 0)


def _wgrad(lib, dout, argmax, out, G, C1, C2, h=None, P=None, Q=None, idx=None, N=0, S=0):
    dev = dout.device
    dW = torch.zeros(C2, C1, device=dev)
    db = torch.zeros(C2, device=dev)
    ws = torch.empty(lib.pzn_pool_wgrad_workspace_bytes(G, C1, C2) // 4, device=dev)
    rc = lib.pzn_pool_wgrad_f32(_p(dout), _p(argmax), _p(out), _p(h), _p(P), _p(Q), _p(idx), N, S, G, C1, C2, _p(dW), _p(db),
                                _p(ws), None)
    assert rc == 0, rc
    return dW, db


# (B, N, S, C1, C2): the first and the second level of the encoder at the benchmark's batch
@pytest.mark.parametrize("B,N,S,C1,C2", [(64, 2048, 512, 128, 128), (64, 2048, 256, 256, 256)])
def test_regenerated_rows_equal_materialised_rows(dev, B, N, S, C1, C2):
    from puzzlenet_amd import _lib
    lib = _lib.load()
    G = B * S
    g = torch.Generator(device=dev).manual_seed(C1 + S)
    P = torch.randn(B * N, C1, device=dev, generator=g)
    Q = 0.5 * torch.randn(G, C1, device=dev, generator=g)
    idx = torch.randint(0, N, (G, 32), device=dev, generator=g, dtype=torch.int64)
    dout = torch.randn(G, C2, device=dev, generator=g)
    argmax = torch.randint(0, 32, (G, C2), device=dev, generator=g, dtype=torch.int32)
    out = torch.randn(G, C2, device=dev, generator=g) + 0.12         # ~45 % of the channels dead (out <= 0), as trained
    dead = float((out <= 0).float().mean())
    assert 0.4 < dead < 0.5, dead
    dW_r, db_r = _wgrad(lib, dout, argmax, out, G, C1, C2, P=P, Q=Q, idx=idx, N=N, S=S)
    # h = relu(P'[idx] + Q) with the same fp32 add; "+ 0.0" turns a -0.0 into +0.0 (the random operands give none: an
    # exact zero sum of two nonzero floats is +0.0)
    rows = (idx + (torch.arange(G, device=dev) // S * N)[:, None]).reshape(-1)
    h = torch.relu(P[rows].view(G, 32, C1) + Q[:, None, :]).reshape(G * 32, C1) + 0.0
    dW_h, db_h = _wgrad(lib, dout, argmax, out, G, C1, C2, h=h)
    del h
    assert torch.equal(db_r, db_h)
    assert torch.equal(dW_r, dW_h), float((dW_r - dW_h).abs().max())
    assert float(dW_r.abs().max()) > 0


def test_level_backward_equals_recorded_bits(dev):
    sys.path.insert(0, GOLDEN)
    try:
        import make_golden_pool_bwd as mk
    finally:
        sys.path.remove(GOLDEN)
    rec = np.load(os.path.join(GOLDEN, "pool_bwd.npz"))
    assert [tuple(s) for s in rec["shapes"].tolist()] == [tuple(s) for s in mk.SHAPES]
    for shape in mk.SHAPES:
        got = mk.level_grads(shape, dev, int(rec["seed"]))
        for name, t in got.items():
            want = torch.from_numpy(rec[mk.key(shape, name)])
            same = torch.equal(t, want) if name in mk.EXACT else mk.close(t, want)
            assert same, (shape, name, float((t - want).abs().max()))
