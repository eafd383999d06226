"""The few-row chain (csrc/fewrows.hip, ops.mlp_rows): stacks of nn.Linear (+ReLU) on at most 128 rows, one launch per layer
each way, partial sums reduced by the consumer in a fixed order.

Shapes are the smallest at which the kernels can go wrong: one chunk plus a ragged K tail, an output narrower than a column
tile (6) and not a multiple of one (70, 300, 33), a single row, ragged row tiles (7, 100), the 128-row limit, and a two-part
input with (144 beside 128) and without (1024 beside 1024) a tail in the second part.  Truth is the same stack in float64 on
the CPU with the ReLU gates taken from the device output (tests/test_gpu_dense.py), bounds are that file's: 1e-5 of the
largest entry for outputs and input gradients, 1e-4 for weight and bias gradients."""
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import _x3_probe as xp
from tests.test_gpu_determinism import REPS, SINK_FILL, _Aggressor

pytestmark = pytest.mark.gpu

# (M, widths): a tuple in front is a two-part input
STACKS = [(1, (256, 6)), (7, (272, 70, 264, 6)), (64, ((128, 144), 256, 6)), (100, (520, 256, 300, 33)),
          (128, ((1024, 1024), 256, 512, 6))]
IDS = ["1x256-6", "7x272-70-264-6", "64x128+144-256-6", "100x520-256-300-33", "128x1024+1024-256-512-6"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _rel(a, b):
    a = a.detach().cpu().double()
    b = b.detach().cpu().double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _parts(widths):
    return tuple(widths[0]) if isinstance(widths[0], tuple) else (widths[0],)


@functools.lru_cache(maxsize=None)
def _case(M, widths):
    """(x parts, weights, biases, upstream gradient) on the CPU, drawn once: x, then W and b of every layer, then dy."""
    parts = _parts(widths)
    dims = (sum(parts),) + tuple(widths[1:])
    g = torch.Generator().manual_seed(M + sum(dims))
    x = torch.randn(M, dims[0], generator=g)
    ws, bs = [], []
    for k, n in zip(dims, dims[1:]):
        ws.append(torch.randn(n, k, generator=g) / math.sqrt(k))
        bs.append(0.1 * torch.randn(n, generator=g))
    go = torch.randn(M, dims[-1], generator=g)
    xs = tuple(t.contiguous() for t in torch.split(x, list(parts), dim=1))
    return xs, tuple(ws), tuple(bs), go


def _device_run(dev, M, widths, sinks=False):
    """Forward and backward on the device -> (y, every layer's gate, part gradients, dW, db)."""
    from puzzlenet_amd import ops
    xs, ws, bs, go = _case(M, widths)
    xd = [t.to(dev).requires_grad_(True) for t in xs]
    wd = [t.to(dev).requires_grad_(True) for t in ws]
    bd = [t.to(dev).requires_grad_(True) for t in bs]
    assert ops.mlp_rows_supported(xd, wd, bd)
    if sinks:
        for p in wd + bd:
            p.grad = torch.full_like(p, SINK_FILL)
        ops.register_grad_sinks(wd + bd)
    try:
        y = ops.mlp_rows(xd, wd, bd)
        (y * go.to(dev)).sum().backward()
    finally:
        ops.clear_grad_sinks()
    with torch.no_grad():       # an inner layer's output: the same launches on the first layers of the stack (ReLU behind each)
        gates = [ops.mlp_rows(xd, wd[:i + 1], bd[:i + 1], [True] * (i + 1)).cpu() > 0 for i in range(len(wd) - 1)]
    fill = SINK_FILL if sinks else 0.0
    return (y.detach().cpu(), gates, [t.grad.cpu() for t in xd], [t.grad.cpu().double() - fill for t in wd],
            [t.grad.cpu().double() - fill for t in bd])


def _truth(M, widths, gates):
    """float64 on the CPU with the device's gates -> (y, mismatching gates, part gradients, dW, db)."""
    xs, ws, bs, go = _case(M, widths)
    xr = [t.double().requires_grad_(True) for t in xs]
    wr = [t.double().requires_grad_(True) for t in ws]
    br = [t.double().requires_grad_(True) for t in bs]
    h = torch.cat(xr, dim=1)
    wrong = 0
    for i, (w, b) in enumerate(zip(wr, br)):
        h = F.linear(h, w, b)
        if i + 1 < len(wr):
            wrong += int((gates[i] != (h.detach() > 0)).sum())
            h = torch.where(gates[i], h, torch.zeros_like(h))
    (h * go.double()).sum().backward()
    return h.detach(), wrong, [t.grad for t in xr], [t.grad for t in wr], [t.grad for t in br]


@pytest.mark.parametrize("sinks", [False, True], ids=["grads", "sinks"])
@pytest.mark.parametrize("M,widths", STACKS, ids=IDS)
def test_stack_against_float64(dev, M, widths, sinks):
    y, gates, dx, dw, db = _device_run(dev, M, widths, sinks)
    yr, wrong, dxr, dwr, dbr = _truth(M, widths, gates)
    assert wrong <= 2, f"{wrong} ReLU gates differ from float64"
    figures = {"y": _rel(y, yr)}
    figures.update({f"dx{j}": _rel(a, b) for j, (a, b) in enumerate(zip(dx, dxr))})
    figures.update({f"dW{i}": _rel(a, b) for i, (a, b) in enumerate(zip(dw, dwr))})
    figures.update({f"db{i}": _rel(a, b) for i, (a, b) in enumerate(zip(db, dbr))})
    print(M, widths, "sinks" if sinks else "grads", {k: f"{v:.2e}" for k, v in figures.items()})
    for k, v in figures.items():
        assert v < (1e-4 if k.startswith(("dW", "db")) else 1e-5), (k, v, figures)


@pytest.mark.parametrize("M,widths", [STACKS[1], STACKS[2]], ids=[IDS[1], IDS[2]])
def test_bitwise_repeatable_alone_and_beside_a_gemm(dev, M, widths):
    """Every sum is fp32 in an order the shapes fix: forward and every gradient are the same bits run after run, with the
    chip to themselves and with an unrelated GEMM on a second stream."""
    from puzzlenet_amd import ops
    xs, ws, bs, go = _case(M, widths)
    xd = [t.to(dev).requires_grad_(True) for t in xs]
    wd = [t.to(dev).requires_grad_(True) for t in ws]
    bd = [t.to(dev).requires_grad_(True) for t in bs]
    god = go.to(dev)

    def run():
        y = ops.mlp_rows(xd, wd, bd)
        grads = torch.autograd.grad((y * god).sum(), xd + wd + bd)
        return [y.detach()] + list(grads)

    agg = _Aggressor(dev)
    agg.size_for(run)
    first = None
    for mode in ("alone", "beside a GEMM"):
        if mode != "alone":
            agg.start()
        for r in range(REPS):
            if mode != "alone":
                agg()
            cur = run()
            torch.cuda.synchronize()
            if first is None:
                first = [t.clone() for t in cur]
                assert all(bool(torch.isfinite(t).all()) and float(t.abs().max()) > 0 for t in first)
                continue
            for i, (a, b) in enumerate(zip(cur, first)):
                assert torch.equal(a, b), f"tensor {i} of run {r} ({mode}) differs from run 0 in {int((a != b).sum())} entries"
    torch.cuda.synchronize()


@pytest.mark.parametrize("M,widths", STACKS, ids=IDS)
def test_chain_against_the_per_layer_path(dev, M, widths, monkeypatch):
    """model5_b._ROWS_CHAIN switches run_seq_parts between the chain and cat + one ops.linear per layer: the two differ by
    the few-row summation order only, 5e-6 of the largest entry (tests/test_gpu_determinism.py)."""
    from puzzlenet_amd import model5_b
    xs, ws, bs, go = _case(M, widths)
    dims = (sum(_parts(widths)),) + tuple(widths[1:])
    seq = model5_b._seq(*dims).to(dev)
    lins = [m for m in seq if isinstance(m, torch.nn.Linear)]
    with torch.no_grad():
        for m, w, b in zip(lins, ws, bs):
            m.weight.copy_(w)
            m.bias.copy_(b)
    out = {}
    for flag in (True, False):
        monkeypatch.setattr(model5_b, "_ROWS_CHAIN", flag)
        xd = [t.to(dev).requires_grad_(True) for t in xs]
        y = model5_b.run_seq_parts(seq, xd)
        grads = torch.autograd.grad((y * go.to(dev)).sum(), xd + list(seq.parameters()))
        out[flag] = [y.detach()] + list(grads)
    for i, (a, b) in enumerate(zip(out[True], out[False])):
        assert _rel(a, b) <= 5e-6, (i, _rel(a, b))


# ------------------------------------------------------------------------------------------ exact probes

SEED = 2207
PROBES = [(7, 272, 70, 40), (64, 520, 264, 6), (100, 256, 72, 33)]       # (M, K, N1, N2)


def _t(dev, x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dev)


def _same(got, want, what):
    g = got.detach().cpu().numpy()
    assert g.shape == want.shape, (what, g.shape, want.shape)
    if not np.array_equal(g, want):
        bad = np.argwhere(g != want)
        i = tuple(int(v) for v in bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {g.size} entries differ; first at {i}: got {g[i]!r}, want {want[i]!r}")


@pytest.mark.parametrize("M,K,N1,N2", PROBES, ids=[f"{m}x{k}-{a}-{b}" for m, k, a, b in PROBES])
def test_forward_products_exact_through_the_consumer_sum(dev, M, K, N1, N2):
    """Integer operands for which each kept plane product and every partial sum is an fp32 value (tests/_x3_probe.py): layer 1
    carries the class operands (3,1), (1,3), (2,2) with an integer bias and a ReLU, layer 2 is a selection matrix, so the
    result is layer 1's output as the second launch summed it from the partial tiles - bit for bit."""
    from puzzlenet_amd import ops
    for cls in xp.CLASSES:
        _, launches = xp.probe_plan(cls, K, N1)
        for launch in range(launches):
            x, wt, room = xp.make_pair(cls, M, K, N1, "b", launch, SEED)
            rng = np.random.default_rng([SEED, launch, M, N1])
            bias = xp.addend(rng, (N1,), room)
            y1 = xp.ref_relu(xp.ref_bias(xp.check(x, wt, bias=bias, cls=cls), bias))
            sel = np.zeros((N1, N2))
            sel[rng.integers(0, N1, size=N2), np.arange(N2)] = 1.0
            y2 = xp.check(y1.astype(np.float64), sel)
            k0 = 128 if launch % 2 else K                          # every other launch: the input as two parts
            xd = _t(dev, x)
            parts = [xd] if k0 == K else [xd[:, :k0].contiguous(), xd[:, k0:].contiguous()]
            ws, bs = [_t(dev, wt.T), _t(dev, sel.T)], [_t(dev, bias), None]
            assert ops.mlp_rows_supported(parts, ws, bs)
            y = ops.mlp_rows(parts, ws, bs)
            _same(y, xp.as_f32(y2), f"y class({cls[0]},{cls[1]}) launch {launch}")


@pytest.mark.parametrize("M,K,N", [(7, 272, 70), (100, 520, 33)], ids=["7x272-70", "100x520-33"])
def test_backward_products_exact(dev, M, K, N):
    """The same for the two backward products of a one-layer chain: dx = dy W (chunks of N, reduced by the last launch) and
    dW = dy^T x, db = column sums of dy (sums over the rows)."""
    from puzzlenet_amd import ops
    for cls in xp.CLASSES:
        for launch in range(xp.probe_plan(cls, N, K)[1]):
            dy, w, _ = xp.make_pair(cls, M, N, K, "b", launch, SEED + 1)
            dx = xp.check(dy, w, cls=cls)
            xd = torch.zeros(M, K, device=dev, requires_grad=True)
            y = ops.mlp_rows([xd], [_t(dev, w)], [None])
            got, = torch.autograd.grad(y, xd, _t(dev, dy))
            _same(got, xp.as_f32(dx), f"dx class({cls[0]},{cls[1]}) launch {launch}")
        for launch in range(xp.probe_plan(cls, M, N)[1]):
            dyt, x, _ = xp.make_pair(cls, N, M, K, "a", launch, SEED + 2)
            dw = xp.check(dyt, x, cls=cls)
            assert int(np.abs(dyt).sum(axis=1).max()) < xp.LIMIT
            wd = torch.zeros(N, K, device=dev, requires_grad=True)
            bd = torch.zeros(N, device=dev, requires_grad=True)
            y = ops.mlp_rows([_t(dev, x)], [wd], [bd])
            gw, gb = torch.autograd.grad(y, [wd, bd], _t(dev, dyt.T))
            _same(gw, xp.as_f32(dw), f"dW class({cls[0]},{cls[1]}) launch {launch}")
            _same(gb, xp.as_f32(xp.ref_colsum(dyt.T)), f"db class({cls[0]},{cls[1]}) launch {launch}")


# ------------------------------------------------------------------------------------------ what the chain does not take

def _reference_ok(dev, M, dims):
    from puzzlenet_amd import ops
    g = torch.Generator().manual_seed(M + sum(dims))
    x = torch.randn(M, dims[0], generator=g)
    ws = [torch.randn(n, k, generator=g) / math.sqrt(k) for k, n in zip(dims, dims[1:])]
    bs = [0.1 * torch.randn(n, generator=g) for n in dims[1:]]
    xd, wd, bd = x.to(dev).requires_grad_(True), [w.to(dev).requires_grad_(True) for w in ws], [b.to(dev) for b in bs]
    assert not ops.mlp_rows_supported([xd], wd, bd)
    y = ops.mlp_rows([xd], wd, bd)
    y.sum().backward()
    h = x.double()
    for i, (w, b) in enumerate(zip(ws, bs)):
        h = F.linear(h, w.double(), b.double())
        if i + 1 < len(ws):
            h = F.relu(h)
    assert _rel(y, h) < 1e-5 and xd.grad is not None and all(w.grad is not None for w in wd)
    return xd, wd, bd


def test_unsupported_stacks_take_the_per_layer_path(dev):
    import ctypes
    from puzzlenet_amd import _lib, ops
    _reference_ok(dev, 129, (256, 6))                 # more than 128 rows
    _reference_ok(dev, 16, (256, 64, 6))              # a layer with K = 64
    lib = _lib.load()
    old = lib.pzn_gemm_get_precision()
    _lib.check(lib.pzn_gemm_set_precision(0), "set_precision")
    try:
        _reference_ok(dev, 16, (256, 128, 6))         # the exact-fp32 mode keeps the general engine
    finally:
        lib.pzn_gemm_set_precision(old)
    # the entry point itself says so, before any launch
    M, dims = 129, (256, 6)
    x, w, b = torch.zeros(M, 256, device=dev), torch.zeros(6, 256, device=dev), torch.zeros(6, device=dev)
    y = torch.full((M, 6), 7.0, device=dev)
    ws = torch.empty(1 << 16, device=dev)
    arr = (ctypes.c_int * 2)(*dims)
    rc = lib.pzn_fewrow_chain_fwd_f32(x.data_ptr(), 256, None, 0, M, 1, arr, ops._ptrs([w]), ops._ptrs([b]), (ctypes.c_int * 1)(0),
                                      ops._ptrs([y]), ws.data_ptr(), ws.numel() * 4, torch.cuda.current_stream().cuda_stream)
    assert rc == _lib.CONSTANTS["PZN_EUNSUPPORTED"]
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())
