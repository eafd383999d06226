"""GPU: ops.linear_cols - x @ weight[:, col0:col0 + Kin].T (+ bias), the columns of a wider weight read in place - is the
entry point pzn_linear_slice_fwd_f32 on the same operands, bit for bit, and refuses what it cannot take before any launch.
(The arithmetic of that entry point is held to float64 by tests/test_gpu_x3_exact.py.)"""
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def test_linear_cols_is_the_slice_entry_point(dev):
    from puzzlenet_amd import _lib, ops
    g = torch.Generator().manual_seed(5)
    for Kin, Nout in itertools.product((64, 1024), (64, 1024)):
        w = (torch.rand(Nout, 2 * Kin, generator=g) - 0.5).to(dev)
        b = (torch.rand(Nout, generator=g) - 0.5).to(dev)
        for M in (1, 3, 65):
            x = (torch.rand(M, Kin, generator=g) - 0.5).to(dev)
            for col0, bias in itertools.product((0, Kin), (b, None)):
                got = ops.linear_cols(x, w, col0, bias)
                want = torch.full((M, Nout), float("nan"), device=dev)
                _lib.call("pzn_linear_slice_fwd_f32", x.data_ptr(), w.data_ptr() + 4 * col0, 2 * Kin,
                          None if bias is None else bias.data_ptr(), M, Kin, Nout, 0, want.data_ptr(), ops._stream())
                tag = f"M {M} Kin {Kin} Nout {Nout} col0 {col0} bias {bias is not None}"
                assert got.shape == (M, Nout) and got.dtype == torch.float32, tag
                assert torch.equal(got, want), tag
                # the two halves are different products, and the bias is really added
                assert not torch.equal(got, ops.linear_cols(x, w, Kin - col0, bias)), tag
                if bias is not None:
                    assert not torch.equal(got, ops.linear_cols(x, w, col0)), tag
            # accumulate: the second half added to the first = the entry point called twice on one output
            acc = ops.linear_cols(x, w, 0, b)
            assert ops.linear_cols(x, w, Kin, None, True, acc) is acc
            want = torch.full((M, Nout), float("nan"), device=dev)
            for col0, flag in ((0, 0), (Kin, 1)):
                _lib.call("pzn_linear_slice_fwd_f32", x.data_ptr(), w.data_ptr() + 4 * col0, 2 * Kin, b.data_ptr(), M, Kin,
                          Nout, flag, want.data_ptr(), ops._stream())
            assert torch.equal(acc, want), f"accumulate M {M} Kin {Kin} Nout {Nout}"
    # leading axes are rows
    x3 = (torch.rand(2, 3, 64, generator=g) - 0.5).to(dev)
    w = (torch.rand(64, 128, generator=g) - 0.5).to(dev)
    assert torch.equal(ops.linear_cols(x3, w, 64), ops.linear_cols(x3.reshape(6, 64), w, 64).view(2, 3, 64))


def test_linear_cols_refuses_before_any_launch(dev, monkeypatch):
    from puzzlenet_amd import _lib, ops
    launches = []
    monkeypatch.setattr(ops, "_call", lambda name, *a, **k: launches.append(name))
    x = torch.zeros(3, 64, device=dev)
    w = torch.zeros(64, 128, device=dev)
    b = torch.zeros(64, device=dev)
    refused = {
        "x on the CPU": (x.cpu(), w, 0, b),
        "weight on the CPU": (x, w.cpu(), 0, b),
        "bias on the CPU": (x, w, 0, b.cpu()),
        "x not float32": (x.double(), w, 0, b),
        "weight not float32": (x, w.half(), 0, b),
        "bias not float32": (x, w, 0, b.double()),
        "columns past the weight": (x, w, 65, b),
        "columns in front of the weight": (x, w, -1, b),
        "x wider than the weight": (torch.zeros(3, 129, device=dev), w, 0, b),
        "rows that are not contiguous": (torch.zeros(3, 128, device=dev)[:, ::2], w, 0, b),
    }
    for tag, args in refused.items():
        with pytest.raises(_lib.PznError):
            ops.linear_cols(*args)
        assert launches == [], tag
    ops.linear_cols(x, w, 64, b)          # the spy does see a call that is taken
    assert launches == ["pzn_linear_slice_fwd_f32"]
