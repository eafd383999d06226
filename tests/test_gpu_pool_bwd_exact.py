"""The pooled level's backward against a float64 truth (tests/_pool_bwd_ref.py, proven on the CPU by
tests/test_pool_bwd_ref_cpu.py), through the C ABI: pzn_pool_wgrad_f32 on regenerated rows (pool_wgrad_regen_kernel) and on the
same rows materialised (pool_wgrad_kernel<., 16>), and pzn_sa_level_bwd_pt_f32 (the weight pass, pool_hits_kernel,
pool_point_kernel) on the lists of pzn_knn_inverse_lists.

Exact cases: dyadic inputs for which every partial sum in any order is an fp32 value, so every output must equal the truth
bit for bit - dW2 and db2 through the fixed-order reduction, dP through the walk by point, dW1[:, 0:3] and db1 through
atomics.  The case table (walk lengths, ragged batches, empty workgroups, channel pairs, planted sparse structure) and why
each shape reaches its path: ref.CASES.  Float cases: random fp32 inputs at the two largest shapes, dP, dW2 and db2 within
gamma_(n+3) * sum|term| per element; run with -s for the observed error-to-bound ratios."""
import functools

import numpy as np
import pytest
import torch

from tests import _pool_bwd_ref as ref

pytestmark = pytest.mark.gpu
D = 5                                             # feature columns of W1 beside the three coordinate columns


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _t(dev, x, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dtype).to(dev)


def _device_inputs(dev, t):
    d = {k: _t(dev, t[k]) for k in ("dout", "out", "W2", "Pp", "Q", "xyz", "new_xyz")}
    d["argmax"] = _t(dev, t["argmax"], torch.int32)
    d["idx"] = _t(dev, t["idx"], torch.int64)
    return d


@functools.lru_cache(maxsize=2)
def _exact_case(name):
    """Inputs, truth and the asserted condition of one case, shared by its tests (which follow each other)."""
    case = ref.CASES[name]
    t = ref.exact_inputs(case)
    assert ref.on_grids(t)
    truth = ref.truth_of(t)
    pre = ref.prefill(case.shape, D)
    for out, m in ref.exact_margin(truth, pre).items():
        assert m < ref.LIMIT, (name, out, m)
    return t, truth, pre


@functools.lru_cache(maxsize=1)
def _float_case(shape):
    t = ref.float_inputs(shape)
    return t, ref.truth_of(t)


def _same(got, want64, what):
    """got (device fp32) == want64 (float64 truth, an fp32 array under the condition) element by element."""
    g, w = got.detach().cpu(), want64.float()
    assert torch.equal(w.double(), want64), what
    assert g.shape == w.shape, (what, g.shape, w.shape)
    if not torch.equal(g, w):
        bad = torch.nonzero(~(g == w))
        i = tuple(int(v) for v in bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {g.numel()} entries differ; first at {i}: got {float(g[i])!r}, want {float(w[i])!r}")


def _within(got, truth, what):
    """|got - truth| <= gamma_(n+3) sum|term| for every element -> the largest error / bound."""
    err = (got.detach().cpu().double() - truth.value).abs()
    bound = ref.float_bound(truth)
    ratio = float((err[bound > 0] / bound[bound > 0]).max())
    print(f"{what}: largest |error| / bound = {ratio:.4f} (largest |error| {float(err.max()):.3e})")
    bad = ~(err <= bound)
    assert not bool(bad.any()), (what, int(bad.sum()), ratio)
    return ratio


def _rows(d, shape):
    """h[G*32, C1] = relu(Pp[point] + Q[group]) in fp32 (exact on the dyadic inputs); + 0.0 turns a -0.0 into +0.0."""
    B, N, S, C1, _ = shape
    G = B * S
    point = (d["idx"].reshape(G, 32) + (torch.arange(G, device=d["idx"].device) // S * N)[:, None]).reshape(-1)
    return torch.relu(d["Pp"][point].view(G, 32, C1) + d["Q"][:, None, :]).reshape(G * 32, C1) + 0.0


def _wgrad(d, shape, dW2, db2, materialised):
    from puzzlenet_amd import _lib
    B, N, S, C1, C2 = shape
    G = B * S
    nbytes = _lib.load().pzn_pool_wgrad_workspace_bytes(G, C1, C2)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dW2.device)
    if materialised:
        h = _rows(d, shape)
        _lib.call("pzn_pool_wgrad_f32", d["dout"].data_ptr(), d["argmax"].data_ptr(), d["out"].data_ptr(), h.data_ptr(), None, None,
                  None, 0, 0, G, C1, C2, dW2.data_ptr(), db2.data_ptr(), ws.data_ptr(), _stream())
    else:
        _lib.call("pzn_pool_wgrad_f32", d["dout"].data_ptr(), d["argmax"].data_ptr(), d["out"].data_ptr(), None, d["Pp"].data_ptr(),
                  d["Q"].data_ptr(), d["idx"].data_ptr(), N, S, G, C1, C2, dW2.data_ptr(), db2.data_ptr(), ws.data_ptr(), _stream())
    torch.cuda.synchronize()


def _lists(d, t, shape):
    """pzn_knn_inverse_lists of the case's idx, compared with NumPy's stable sort before anything walks them."""
    from puzzlenet_amd import _lib
    B, N, S, _, _ = shape
    dev = d["idx"].device
    off = torch.full((B, N + 1), -1, dtype=torch.int32, device=dev)
    rows = torch.full((B, S * 32), -1, dtype=torch.int32, device=dev)
    pts = torch.full((B, S * 32), -1, dtype=torch.int32, device=dev)
    _lib.call("pzn_knn_inverse_lists", d["idx"].data_ptr(), B, N, S, 32, off.data_ptr(), rows.data_ptr(), pts.data_ptr(), _stream())
    torch.cuda.synchronize()
    for name, got, want in zip(("off", "rows", "pts"), (off, rows, pts), ref.inverse_lists(t["idx"], N)):
        assert np.array_equal(got.cpu().numpy(), want), name
    return off, rows, pts


def _level(d, lists, shape, dP, dW2, db2, dW1, db1, accumulate):
    from puzzlenet_amd import _lib
    B, N, S, C1, C2 = shape
    nbytes = _lib.load().pzn_sa_level_bwd_pt_workspace_bytes(B, S, C2)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dP.device)
    off, rows, pts = lists
    _lib.call("pzn_sa_level_bwd_pt_f32", d["dout"].data_ptr(), d["argmax"].data_ptr(), d["out"].data_ptr(), d["W2"].data_ptr(),
              d["Pp"].data_ptr(), d["Q"].data_ptr(), d["idx"].data_ptr(), d["xyz"].data_ptr(), d["new_xyz"].data_ptr(), off.data_ptr(),
              rows.data_ptr(), pts.data_ptr(), B, N, S, D, C1, C2, dP.data_ptr(), dW2.data_ptr(), db2.data_ptr(), dW1.data_ptr(),
              None if db1 is None else db1.data_ptr(), int(accumulate), ws.data_ptr(), _stream())
    torch.cuda.synchronize()


# --------------------------------------------------------------------------- exact probes

@pytest.mark.parametrize("rows", ["regenerated", "materialised"])
@pytest.mark.parametrize("name", list(ref.CASES))
def test_pool_wgrad_exact(dev, name, rows):
    """pzn_pool_wgrad_f32: dW2 and db2, prefilled with integers (both are added to), equal prefill + truth."""
    shape = ref.CASES[name].shape
    t, truth, pre = _exact_case(name)
    d = _device_inputs(dev, t)
    dW2, db2 = _t(dev, pre["dW2"]), _t(dev, pre["db2"])
    _wgrad(d, shape, dW2, db2, rows == "materialised")
    _same(db2, truth["db2"].value + torch.from_numpy(pre["db2"]), f"{name} {rows} db2")
    _same(dW2, truth["dW2"].value + torch.from_numpy(pre["dW2"]), f"{name} {rows} dW2")


@pytest.mark.parametrize("accumulate", [0, 1], ids=["overwrite", "accumulate"])
@pytest.mark.parametrize("name", list(ref.CASES))
def test_level_backward_exact(dev, name, accumulate):
    """pzn_sa_level_bwd_pt_f32, all five outputs: dP prefilled with NaN (every row is written), dW1 [C1, 3 + D] and db1
    prefilled with integers (added to; columns 3.. of dW1 come back untouched), dW2 and db2 prefilled with NaN and
    overwritten, or with integers and added to."""
    shape = ref.CASES[name].shape
    B, N, S, C1, C2 = shape
    t, truth, pre = _exact_case(name)
    d = _device_inputs(dev, t)
    lists = _lists(d, t, shape)
    p = {k: torch.from_numpy(v) for k, v in pre.items()}
    dP = torch.full((B * N, C1), float("nan"), device=dev)
    dW2 = _t(dev, pre["dW2"]) if accumulate else torch.full((C2, C1), float("nan"), device=dev)
    db2 = _t(dev, pre["db2"]) if accumulate else torch.full((C2,), float("nan"), device=dev)
    dW1, db1 = _t(dev, pre["dW1"]), _t(dev, pre["db1"])
    _level(d, lists, shape, dP, dW2, db2, dW1, db1, accumulate)
    tag = f"{name} accumulate={accumulate}"
    _same(db2, truth["db2"].value + (p["db2"] if accumulate else 0.0), tag + " db2")
    _same(dW2, truth["dW2"].value + (p["dW2"] if accumulate else 0.0), tag + " dW2")
    _same(dP, truth["dP"].value, tag + " dP")
    _same(db1, truth["db1"].value + p["db1"], tag + " db1")
    want = p["dW1"].clone()
    want[:, 0:3] += truth["dW1"].value
    _same(dW1, want, tag + " dW1")


@pytest.mark.parametrize("name", [n for n in ref.CASES if n.startswith(("small_clouds", "two_slices"))])
def test_level_backward_without_db1(dev, name):
    """db1 == NULL: the other four outputs as before."""
    shape = ref.CASES[name].shape
    B, N, S, C1, C2 = shape
    t, truth, pre = _exact_case(name)
    d = _device_inputs(dev, t)
    lists = _lists(d, t, shape)
    dP = torch.full((B * N, C1), float("nan"), device=dev)
    dW2, db2 = torch.full((C2, C1), float("nan"), device=dev), torch.full((C2,), float("nan"), device=dev)
    dW1 = _t(dev, pre["dW1"])
    _level(d, lists, shape, dP, dW2, db2, dW1, None, 0)
    _same(db2, truth["db2"].value, name + " db2")
    _same(dW2, truth["dW2"].value, name + " dW2")
    _same(dP, truth["dP"].value, name + " dP")
    want = torch.from_numpy(pre["dW1"]).clone()
    want[:, 0:3] += truth["dW1"].value
    _same(dW1, want, name + " dW1")


# --------------------------------------------------------------------------- random fp32 inputs, derived bounds
# Observed on an MI355X, largest |error| / bound (both row sources and the level's own weight pass alike):
#   (5, 96, 500, 128, 128):  db2 0.0002   dW2 0.0005   dP 0.31
#   (5, 64, 288, 256, 256):  db2 0.0003   dW2 0.0012   dP 0.29
# The bounds are derived (module docstring of tests/_pool_bwd_ref.py), not fitted to these figures.

@pytest.mark.parametrize("rows", ["regenerated", "materialised"])
@pytest.mark.parametrize("shape", ref.FLOAT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_pool_wgrad_float_within_bound(dev, shape, rows):
    """pzn_pool_wgrad_f32 on random fp32 inputs: dW2 and db2 (onto zeros) within gamma_(n+3) sum|term| per element."""
    t, truth = _float_case(tuple(shape))
    d = _device_inputs(dev, t)
    C1, C2 = shape[3], shape[4]
    dW2, db2 = torch.zeros(C2, C1, device=dev), torch.zeros(C2, device=dev)
    _wgrad(d, shape, dW2, db2, rows == "materialised")
    _within(db2, truth["db2"], f"{shape} {rows} db2")
    _within(dW2, truth["dW2"], f"{shape} {rows} dW2")


@pytest.mark.parametrize("shape", ref.FLOAT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_level_backward_float_within_bound(dev, shape):
    """pzn_sa_level_bwd_pt_f32 on random fp32 inputs: dP, dW2 and db2 within gamma_(n+3) sum|term| per element; a dP entry no
    term lands on is exactly 0."""
    B, N, S, C1, C2 = shape
    t, truth = _float_case(tuple(shape))
    d = _device_inputs(dev, t)
    lists = _lists(d, t, shape)
    dP = torch.full((B * N, C1), float("nan"), device=dev)
    dW2, db2 = torch.full((C2, C1), float("nan"), device=dev), torch.full((C2,), float("nan"), device=dev)
    dW1, db1 = torch.zeros(C1, 3 + D, device=dev), torch.zeros(C1, device=dev)
    _level(d, lists, shape, dP, dW2, db2, dW1, db1, 0)
    _within(db2, truth["db2"], f"{shape} level db2")
    _within(dW2, truth["dW2"], f"{shape} level dW2")
    _within(dP, truth["dP"], f"{shape} level dP")
