"""GPU parity of the dense engine (csrc/gemm.hip, chamfer.hip) against plain fp32/fp64 torch
restatements of the same ops evaluated on CPU.  Tolerance 1e-4 relative unless noted
(the f32-input MFMA is an exact fp32 fma chain; differences are summation order only)."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests._attn_launch import fused_block as _fused_block
from tests._attn_ref import attn_block_ref as _attn_block_ref64, attn_chain_ref as _attn_chain_ref64

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(params=["auto", "f32", "x3"])
def precision(request):
    """Run the dense tests on every matrix-core path (exact fp32 MFMA, bf16x3 split precision, auto)."""
    from puzzlenet_amd import _lib
    lib = _lib.load()
    old = lib.pzn_gemm_get_precision()
    _lib.check(lib.pzn_gemm_set_precision({"f32": 0, "x3": 1, "auto": 2}[request.param]), "set_precision")
    yield request.param
    lib.pzn_gemm_set_precision(old)


def _rel(a, b):
    a = a.detach().cpu().double()
    b = b.detach().cpu().double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


@pytest.mark.parametrize("M,K,N,relu,bias", [
    (4096, 64, 128, True, True), (1000, 67, 128, True, True), (777, 131, 256, False, True),
    (64, 2048, 1024, True, True), (64, 256, 6, False, True), (5000, 3, 64, False, True),
    (300, 32, 2, False, True), (256, 1280, 1024, False, False), (129, 128, 64, True, True), (1, 64, 64, False, True),
    # shapes that take the weight-stationary forward / input-gradient kernel (wsgemm.hip) and the direct-fragment
    # weight-gradient kernel (dfgemm.hip): ragged row tiles, K tails (68, 132 -> odd double-step counts), column
    # tails, one / two / four 32-column tiles per wave, the two-sets-in-flight walk (16384 x 256 x 256)
    (4100, 68, 96, True, True), (6000, 132, 256, True, True), (4096, 128, 32, False, True),
    (8192, 256, 64, True, False), (16384, 256, 256, True, True), (4128, 96, 160, False, True),
    (4112, 67, 128, True, True), (8192, 131, 256, False, True), (4096, 64, 64, True, True),
    # few rows, long K (the pose head): K split across workgroups, atomic epilogue, bias / ReLU in a second launch
    (64, 1024, 512, True, True), (100, 300, 70, True, True), (128, 520, 256, False, False), (7, 257, 33, True, False),
    # the per-point heads: one or two tile blocks of the weight gradient (4 / 8 row replicas meeting in LDS), narrow
    # N / K (clamped column loads of the direct-fragment kernel)
    (131072, 64, 64, True, True), (131072, 128, 64, True, True), (131072, 3, 64, False, True),
    (131072, 32, 2, False, True), (8192, 5, 7, True, True), (32768, 64, 32, True, True)])
def test_linear_fwd_bwd(dev, precision, M, K, N, relu, bias):
    from puzzlenet_amd import ops
    g = torch.Generator().manual_seed(M + K + N)
    x = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g) / math.sqrt(K)
    b = torch.randn(N, generator=g) if bias else None
    go = torch.randn(M, N, generator=g)
    xr, wr = x.double().requires_grad_(True), w.double().requires_grad_(True)
    br = b.double().requires_grad_(True) if bias else None
    xd, wd = x.to(dev).requires_grad_(True), w.to(dev).requires_grad_(True)
    bd = b.to(dev).requires_grad_(True) if bias else None
    y = ops.linear(xd, wd, bd, relu)
    yr = F.linear(xr, wr, br)
    if relu:
        # the ReLU gate of the reference backward is taken from the device output: with millions of outputs a
        # pre-activation within fp32 rounding of zero turns up, and its gate is then a coin flip, not an error
        gate = (y.detach().cpu() > 0)
        assert int((gate != (yr.detach() > 0)).sum()) <= max(2, y.numel() // 500000)
        yr = torch.where(gate, yr, torch.zeros_like(yr))
    (yr * go.double()).sum().backward()
    assert _rel(y, yr) < 1e-5
    (y * go.to(dev)).sum().backward()
    assert _rel(xd.grad, xr.grad) < 1e-5
    assert _rel(wd.grad, wr.grad) < 1e-4
    if bias:
        assert _rel(bd.grad, br.grad) < 1e-4


def test_linear_nd_input_and_no_grad_paths(dev):
    from puzzlenet_amd import ops
    x = torch.randn(3, 5, 7, 16, device=dev)
    w = torch.randn(8, 16, device=dev, requires_grad=True)
    y = ops.linear(x, w, None, False)
    assert y.shape == (3, 5, 7, 8)
    assert _rel(y, F.linear(x.cpu(), w.detach().cpu())) < 1e-5
    y.sum().backward()
    assert w.grad.shape == (8, 16)


@pytest.mark.parametrize("B,S,C0,C1,C2", [(2, 64, 67, 128, 128), (2, 40, 131, 256, 256), (1, 5, 20, 32, 48),
                                            (4, 64, 68, 128, 128), (2, 80, 132, 256, 256), (3, 50, 64, 64, 128)])
def test_shared_mlp_max(dev, precision, B, S, C0, C1, C2):
    from puzzlenet_amd import ops
    g = torch.Generator().manual_seed(C0)
    x = torch.randn(B, S, 32, C0, generator=g)
    w1, b1 = torch.randn(C1, C0, generator=g) / math.sqrt(C0), 0.1 * torch.randn(C1, generator=g)
    w2, b2 = torch.randn(C2, C1, generator=g) / math.sqrt(C1), 0.1 * torch.randn(C2, generator=g)
    go = torch.randn(B, S, C2, generator=g)
    ref = [t.double().requires_grad_(True) for t in (x, w1, b1, w2, b2)]
    yr = torch.max(F.relu(F.linear(F.relu(F.linear(ref[0], ref[1], ref[2])), ref[3], ref[4])), dim=-2)[0]
    (yr * go.double()).sum().backward()
    d = [t.to(dev).requires_grad_(True) for t in (x, w1, b1, w2, b2)]
    y = ops.shared_mlp_max(*d)
    assert y.shape == (B, S, C2)
    assert _rel(y, yr) < 1e-5
    (y * go.to(dev)).sum().backward()
    for a, r, name in zip(d, ref, ("x", "w1", "b1", "w2", "b2")):
        assert _rel(a.grad, r.grad) < 1e-4, name


@pytest.mark.parametrize("B,L,dk,dv", [(3, 256, 64, 256), (2, 100, 16, 40), (1, 33, 8, 8)])
def test_attention(dev, precision, B, L, dk, dv):
    from puzzlenet_amd import ops
    g = torch.Generator().manual_seed(L)
    q, k, v = torch.randn(B, L, dk, generator=g), torch.randn(B, L, dk, generator=g), torch.randn(B, L, dv, generator=g)
    go, ga = torch.randn(B, L, dv, generator=g), torch.randn(B, L, L, generator=g)
    ref = [t.double().requires_grad_(True) for t in (q, k, v)]
    attn_r = F.softmax(ref[0] @ ref[1].transpose(-2, -1) / math.sqrt(dk), dim=-1)
    out_r = attn_r @ ref[2]
    ((out_r * go.double()).sum() + (attn_r * ga.double()).sum()).backward()
    d = [t.to(dev).requires_grad_(True) for t in (q, k, v)]
    out, attn = ops.attention(*d)
    assert _rel(out, out_r) < 1e-5 and _rel(attn, attn_r) < 1e-5
    ((out * go.to(dev)).sum() + (attn * ga.to(dev)).sum()).backward()
    for a, r, name in zip(d, ref, "qkv"):
        assert _rel(a.grad, r.grad) < 1e-4, name
    # values only (the model's case: the attention map feeds no differentiable op)
    d2 = [t.to(dev).requires_grad_(True) for t in (q, k, v)]
    (ops.attention(*d2)[0] * go.to(dev)).sum().backward()
    assert d2[0].grad is not None


@pytest.mark.parametrize("B,n,m", [(3, 200, 200), (2, 128, 128), (2, 300, 77), (4, 2048, 2048), (1, 64, 64)])
def test_chamfer_vs_oracle(dev, B, n, m):
    from oracle import point_ops as orc
    from puzzlenet_amd import ops
    rng = np.random.default_rng(n + m)
    a = rng.random((B, n, 3), dtype=np.float32)
    b = rng.random((B, m, 3), dtype=np.float32)
    moa, aoa, mob, aob = orc.chamfer(a, b)
    ta, tb = torch.from_numpy(a).to(dev).requires_grad_(True), torch.from_numpy(b).to(dev).requires_grad_(True)
    d1, d2 = ops.chamfer(ta, tb)
    # expansion form: absolute error ~ eps * |p|^2, compare absolutely
    np.testing.assert_allclose(d1.detach().cpu().numpy(), moa, rtol=1e-4, atol=3e-6)
    np.testing.assert_allclose(d2.detach().cpu().numpy(), mob, rtol=1e-4, atol=3e-6)
    w1 = torch.from_numpy(rng.standard_normal((B, m)).astype(np.float32)).to(dev)
    w2 = torch.from_numpy(rng.standard_normal((B, n)).astype(np.float32)).to(dev)
    ((d1 * w1).sum() + (d2 * w2).sum()).backward()
    # analytic gradient at the oracle's arg-mins
    ga = np.zeros_like(a, dtype=np.float64)
    gb = np.zeros_like(b, dtype=np.float64)
    w1n, w2n = w1.cpu().numpy().astype(np.float64), w2.cpu().numpy().astype(np.float64)
    for bb in range(B):
        for j in range(m):
            i = aoa[bb, j]
            dlt = 2 * w1n[bb, j] * (a[bb, i].astype(np.float64) - b[bb, j])
            ga[bb, i] += dlt
            gb[bb, j] -= dlt
        for i in range(n):
            j = aob[bb, i]
            dlt = 2 * w2n[bb, i] * (a[bb, i].astype(np.float64) - b[bb, j])
            ga[bb, i] += dlt
            gb[bb, j] -= dlt
    # a near-tie may pick another partner: compare in L2
    assert np.linalg.norm(ta.grad.cpu().numpy() - ga) / np.linalg.norm(ga) < 2e-3
    assert np.linalg.norm(tb.grad.cpu().numpy() - gb) / np.linalg.norm(gb) < 2e-3


def test_chamfer_identity_and_symmetry(dev):
    from puzzlenet_amd import ops
    a = torch.rand(2, 512, 3, device=dev)
    b = torch.rand(2, 512, 3, device=dev)
    d1, d2 = ops.chamfer(a, a)
    assert float(d1.abs().max()) < 1e-5 and float(d2.abs().max()) < 1e-5
    x1, x2 = ops.chamfer(a, b)
    y1, y2 = ops.chamfer(b, a)
    assert torch.equal(x1, y2) and torch.equal(x2, y1)         # both passes see bit-identical P


@pytest.mark.parametrize("B,N,S,D,C1,C2", [(2, 300, 40, 64, 128, 128), (2, 128, 24, 128, 256, 256), (1, 64, 5, 8, 16, 24),
                                              (4, 600, 64, 64, 128, 128), (2, 400, 96, 128, 256, 256),
                                              (3, 97, 33, 12, 64, 40)])
def test_sa_mlp_max_fused_vs_composed(dev, precision, B, N, S, D, C1, C2):
    """Set-abstraction level (ops.sa_mlp_max) == group -> shared MLP -> max composed from fp64 torch ops: the encoder's
    shapes (C1 in {128, 256}) through the per-point kernels - rows generated inside the matrix-core kernel and the backward
    by point, never in memory -, every other shape through the grouped-row composition the function falls back to."""
    from oracle import point_ops as orc
    from puzzlenet_amd import ops
    rng = np.random.default_rng(D + S)
    xyz = rng.random((B, N, 3), dtype=np.float32)
    feat = rng.standard_normal((B, N, D)).astype(np.float32)
    new_xyz = xyz[:, :S].copy()
    idx = orc.knn(xyz, new_xyz, 32)
    g = torch.Generator().manual_seed(1)
    w1, b1 = torch.randn(C1, 3 + D, generator=g) / math.sqrt(3 + D), 0.1 * torch.randn(C1, generator=g)
    w2, b2 = torch.randn(C2, C1, generator=g) / math.sqrt(C1), 0.1 * torch.randn(C2, generator=g)
    go = torch.randn(B, S, C2, generator=g)
    grouped = torch.from_numpy(orc.group(xyz, feat, new_xyz, idx)).double()
    featr = torch.from_numpy(feat).double().requires_grad_(True)
    tidx = torch.from_numpy(idx)
    gfe = torch.gather(featr, 1, tidx.reshape(B, -1, 1).expand(-1, -1, D)).reshape(B, S, 32, D)
    xin = torch.cat([grouped[..., :3], gfe], dim=-1)
    ref = [t.double().requires_grad_(True) for t in (w1, b1, w2, b2)]
    yr = torch.max(F.relu(F.linear(F.relu(F.linear(xin, ref[0], ref[1])), ref[2], ref[3])), dim=-2)[0]
    (yr * go.double()).sum().backward()
    d = [t.to(dev).requires_grad_(True) for t in (w1, b1, w2, b2)]
    fd = torch.from_numpy(feat).to(dev).requires_grad_(True)
    y = ops.sa_mlp_max(torch.from_numpy(xyz).to(dev), fd, torch.from_numpy(new_xyz).to(dev), torch.from_numpy(idx).to(dev), *d)
    assert _rel(y, yr) < 1e-5
    (y * go.to(dev)).sum().backward()
    assert _rel(fd.grad, featr.grad) < 1e-4
    for a, r, name in zip(d, ref, ("w1", "b1", "w2", "b2")):
        assert _rel(a.grad, r.grad) < 1e-4, name
    if N >= 64:
        # idx=None: the neighbour search runs inside the call — same values
        d2 = [t.to(dev).requires_grad_(True) for t in (w1, b1, w2, b2)]
        f2 = torch.from_numpy(feat).to(dev).requires_grad_(True)
        y2 = ops.sa_mlp_max(torch.from_numpy(xyz).to(dev), f2, torch.from_numpy(new_xyz).to(dev), None, *d2)
        assert torch.equal(y2, y)
        (y2 * go.to(dev)).sum().backward()
        assert _rel(f2.grad, featr.grad) < 1e-4
        if ops.sa_level_fused_supported(f2, None, d2[0], d2[2]):
            # the per-point path sums dP by owner and the pooled layer's dW2 / db2 from the workgroups' partial tiles in a fixed
            # order (csrc/poolbwd.hip: no atomics): the same bits as the first run (idx given or searched: the same indices)
            assert torch.equal(f2.grad, fd.grad)
            assert torch.equal(d2[2].grad, d[2].grad) and torch.equal(d2[3].grad, d[3].grad)


@pytest.mark.parametrize("B,N,S,D,C", [(4, 2048, 512, 64, 128), (4, 512, 256, 128, 256), (2, 300, 40, 64, 128)])
def test_sa_level_one_call_equals_the_stepwise_form(dev, B, N, S, D, C):
    """The level behind one C entry point each way (csrc/sachain.hip: the coordinate columns of the first layer in the store
    epilogue of the product on the features, pzn_ws_gemm_r3, where the skinny-layer kernel takes the shape) against the same
    level enqueued entry point by entry point from Python (product, then pzn_sa_prep_f32's pass over the table): output,
    arg-max and the order-fixed gradients bit-identical."""
    from puzzlenet_amd import ops
    g = torch.Generator().manual_seed(C + N)
    xyz = torch.rand(B, N, 3, generator=g).to(dev)
    feat0 = torch.randn(B, N, D, generator=g).to(dev)
    new_xyz = xyz[:, :S].contiguous()
    w = [(torch.randn(C, 3 + D, generator=g) / math.sqrt(3 + D)).to(dev), (0.1 * torch.randn(C, generator=g)).to(dev),
         (torch.randn(C, C, generator=g) / math.sqrt(C)).to(dev), (0.1 * torch.randn(C, generator=g)).to(dev)]
    go = torch.randn(B, S, C, generator=g).to(dev)

    def run(stepwise):
        feat = feat0.clone().requires_grad_(True)
        ps = [t.clone().requires_grad_(True) for t in w]
        ops.KernelTimer.enabled = stepwise
        try:
            y = ops.sa_mlp_max(xyz, feat, new_xyz, None, *ps)
            (y * go).sum().backward()
        finally:
            ops.KernelTimer.enabled = False
        return y.detach(), feat.grad, ps[2].grad, ps[3].grad

    one, step = run(False), run(True)
    for a, b in zip(one, step):
        assert torch.equal(a, b)


@pytest.mark.parametrize("sinks", [False, True])
def test_attention_block_fused_vs_composed(dev, sinks):
    """pzn_attn_block_* (layerAttention behind one entry point each way, residual / offset lines and the dx sums
    in GEMM epilogues) against the block composed from linear + attention + tensor ops, outputs and every
    gradient, also with the attention map receiving a gradient and with the parameter gradients going straight
    into registered sinks (accumulate epilogues)."""
    from puzzlenet_amd import ops
    B, L, E, dk = 20, 256, 256, 64            # 5120 rows: inside the weight-stationary kernel's domain
    g = torch.Generator().manual_seed(3)
    x0 = (0.5 * torch.randn(B, L, E, generator=g)).to(dev)
    shapes = [(dk, E), (dk,), (dk, E), (dk,), (E, E), (E,), (E, E), (E,)]
    params0 = [(torch.randn(*s, generator=g) / (math.sqrt(E) if len(s) == 2 else 4)).to(dev) for s in shapes]
    wr, wa = torch.randn(B, L, E, generator=g).to(dev), torch.randn(B, L, L, generator=g).to(dev)

    def run(fused):
        x = x0.clone().requires_grad_(True)
        ps = [p.clone().requires_grad_(True) for p in params0]
        ops.clear_grad_sinks()
        if sinks:
            for p in ps:
                p.grad = torch.full_like(p, 0.25)          # pre-existing content: the kernels must ADD to it
            ops.register_grad_sinks(ps)
        assert ops.attention_block_supported(x, dk)
        if fused:
            r, a = ops.attention_block(x, *ps)
        else:
            wq, bq, wk, bk, wv, bv, wo, bo = ps
            q, k, v = ops.linear(x, wq, bq), ops.linear(x, wk, bk), ops.linear(x, wv, bv)
            t, a = ops.attention(q, k, v)
            r = x + ops.linear(x - t, wo, bo, relu=True)
        ((r * wr).sum() + (a * wa).sum()).backward()
        ops.clear_grad_sinks()
        return r.detach(), a.detach(), x.grad, [p.grad for p in ps]

    rf, af, gxf, gpf = run(True)
    rc, ac, gxc, gpc = run(False)
    assert _rel(rf, rc) < 1e-5 and _rel(af, ac) < 1e-5
    assert _rel(gxf, gxc) < 1e-4
    for a_, b_ in zip(gpf, gpc):
        # (the key bias has a mathematically zero gradient — softmax is shift-invariant — so it gets an absolute floor)
        assert float((a_ - b_).abs().max()) < 2e-4 * max(float(b_.abs().max()), 5e-2)


# Stated tolerance of the opt-in bf16 attention mode (pzn_attn_set_precision(1)): operands are rounded to bf16 (8
# significant bits: relative step 2^-8, rounding error <= 2^-9 = 2e-3 per operand), products and sums are fp32.  A logit
# q.k / sqrt(dk) with |q|, |k| ~ sqrt(dk) then carries an absolute error of ~3e-3, which softmax turns into the same
# relative error of the map; values and gradients add the rounding of their own operands.  Held to 2e-2 of the
# tensor's largest magnitude forward and 4e-2 backward, and to 1e-2 in the relative L2 norm.
BF16_FWD_TOL, BF16_BWD_TOL, BF16_L2_TOL = 2e-2, 4e-2, 1e-2


@pytest.fixture
def attn_bf16():
    from puzzlenet_amd import _lib
    lib = _lib.load()
    old = lib.pzn_attn_get_precision()
    _lib.check(lib.pzn_attn_set_precision(1), "pzn_attn_set_precision")
    yield
    lib.pzn_attn_set_precision(old)


def _l2(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


@pytest.mark.parametrize("B,L,dk,dv", [(3, 256, 64, 256), (2, 100, 16, 40)])
def test_attention_bf16_mode(dev, attn_bf16, B, L, dk, dv):
    """scaled_dot_production (model5_b.py:67-75) with the contractions as single bf16 MFMAs, fp32 softmax, against the
    fp64 composition at the stated bf16 tolerance; the mode must really be a different (coarser) result than the
    default path, and the default path must be untouched once the mode is switched back."""
    from puzzlenet_amd import _lib, ops
    g = torch.Generator().manual_seed(L)
    q, k, v = torch.randn(B, L, dk, generator=g), torch.randn(B, L, dk, generator=g), torch.randn(B, L, dv, generator=g)
    go = torch.randn(B, L, dv, generator=g)
    ref = [t.double().requires_grad_(True) for t in (q, k, v)]
    attn_r = F.softmax(ref[0] @ ref[1].transpose(-2, -1) / math.sqrt(dk), dim=-1)
    out_r = attn_r @ ref[2]
    (out_r * go.double()).sum().backward()
    d = [t.to(dev).requires_grad_(True) for t in (q, k, v)]
    out, attn = ops.attention(*d)
    assert _rel(out, out_r) < BF16_FWD_TOL and _rel(attn, attn_r) < BF16_FWD_TOL
    assert _l2(out, out_r) < BF16_L2_TOL and _l2(attn, attn_r) < BF16_L2_TOL
    assert _rel(out, out_r) > 1e-4            # it IS the bf16 path (the default agrees to 1e-5)
    (out * go.to(dev)).sum().backward()
    for a, r, name in zip(d, ref, "qkv"):
        assert _rel(a.grad, r.grad) < BF16_BWD_TOL and _l2(a.grad, r.grad) < 2 * BF16_L2_TOL, name
    lib = _lib.load()
    lib.pzn_attn_set_precision(0)
    out32, _ = ops.attention(*[t.to(dev) for t in (q, k, v)])
    lib.pzn_attn_set_precision(1)
    assert _rel(out32, out_r) < 1e-5


def test_attention_block_bf16_mode(dev, attn_bf16):
    """layerAttention behind pzn_attn_block_* in the bf16 attention mode: projections stay fp32-accurate, the four
    contractions are bf16; outputs and gradients against an fp64 restatement of model5_b.py:83-101."""
    from puzzlenet_amd import ops
    B, L, E, dk = 20, 256, 256, 64
    g = torch.Generator().manual_seed(3)
    x0 = 0.5 * torch.randn(B, L, E, generator=g)
    shapes = [(dk, E), (dk,), (dk, E), (dk,), (E, E), (E,), (E, E), (E,)]
    params0 = [torch.randn(*s, generator=g) / (math.sqrt(E) if len(s) == 2 else 4) for s in shapes]
    wr = torch.randn(B, L, E, generator=g)
    xr = x0.double().requires_grad_(True)
    pr = [p.double().requires_grad_(True) for p in params0]
    wq, bq, wk, bk, wv, bv, wo, bo = pr
    qr, kr, vr = xr @ wq.t() + bq, xr @ wk.t() + bk, xr @ wv.t() + bv
    ar = F.softmax(qr @ kr.transpose(-2, -1) / math.sqrt(dk), dim=-1)
    rr = xr + torch.relu((xr - ar @ vr) @ wo.t() + bo)
    (rr * wr.double()).sum().backward()
    x = x0.to(dev).requires_grad_(True)
    ps = [p.to(dev).requires_grad_(True) for p in params0]
    ops.clear_grad_sinks()
    assert ops.attention_block_supported(x, dk)
    r, a = ops.attention_block(x, *ps)
    assert _rel(r, rr) < BF16_FWD_TOL and _rel(a, ar) < BF16_FWD_TOL and _l2(r, rr) < BF16_L2_TOL
    (r * wr.to(dev)).sum().backward()
    # dx passes through the ReLU of the output projection: a gate whose pre-activation sits within the bf16 error of
    # zero flips and moves single entries by a whole term, so dx is held in L2 and by the share of deviating entries
    dxe = (x.grad.cpu().double() - xr.grad).abs()
    assert _l2(x.grad, xr.grad) < 2 * BF16_L2_TOL
    assert float((dxe > BF16_BWD_TOL * xr.grad.abs().max()).double().mean()) < 1e-3
    for p_, q_ in zip(ps, pr):
        assert _l2(p_.grad, q_.grad) < 2 * BF16_L2_TOL or float(q_.grad.abs().max()) < 5e-2
        # (the key bias has a mathematically zero gradient — softmax is shift-invariant — and collects the bf16 rounding
        # noise of 5120 rows instead: absolute floor)
        assert float((p_.grad.cpu().double() - q_.grad).abs().max()) < 2 * BF16_BWD_TOL * max(float(q_.grad.abs().max()), 0.25)


@pytest.mark.parametrize("M,E,Nout,nsl", [(16384, 256, 1024, 5), (1000, 64, 96, 3), (4096, 128, 128, 2)])
def test_linear_slice_entry_points(dev, M, E, Nout, nsl):
    """pzn_linear_slice_{fwd,dgrad,wgrad}_f32: products on a column slice W[:, a:a+E] of a wider weight (row stride ldw),
    against float64 matmuls of the same slice; fwd also in accumulate mode, dgrad with an addend, wgrad adding into
    the slice of a pre-filled gradient buffer (the neighbouring columns must stay untouched)."""
    from puzzlenet_amd import _lib
    g = torch.Generator().manual_seed(M + E)
    ldw = nsl * E
    W = (torch.randn(Nout, ldw, generator=g) / math.sqrt(E)).to(dev)
    bias = torch.randn(Nout, generator=g).to(dev)
    xs = [torch.randn(M, E, generator=g).to(dev) for _ in range(nsl)]
    dy = torch.randn(M, Nout, generator=g).to(dev)
    add = torch.randn(M, E, generator=g).to(dev)
    st = torch.cuda.current_stream().cuda_stream
    y = torch.empty(M, Nout, device=dev)
    for i, x in enumerate(xs):
        _lib.call("pzn_linear_slice_fwd_f32", x.data_ptr(), W.data_ptr() + 4 * E * i, ldw, bias.data_ptr(), M, E, Nout,
                  int(i > 0), y.data_ptr(), st)
    ref = torch.cat(xs, 1).double() @ W.double().t() + bias.double()
    assert _rel(y, ref.float()) < 1e-5
    sl = nsl - 1
    dx = torch.empty(M, E, device=dev)
    _lib.call("pzn_linear_slice_dgrad_f32", dy.data_ptr(), W.data_ptr() + 4 * E * sl, ldw, M, E, Nout, add.data_ptr(),
              dx.data_ptr(), st)
    ref = dy.double() @ W[:, sl * E:(sl + 1) * E].double() + add.double()
    assert _rel(dx, ref.float()) < 1e-5
    dW = torch.full((Nout, ldw), 0.5, device=dev)
    db = torch.full((Nout,), -1.0, device=dev)
    _lib.call("pzn_linear_slice_wgrad_f32", dy.data_ptr(), xs[sl].data_ptr(), M, E, Nout, dW.data_ptr() + 4 * E * sl, ldw,
              db.data_ptr(), st)
    ref = torch.full((Nout, ldw), 0.5, dtype=torch.float64, device=dev)
    ref[:, sl * E:(sl + 1) * E] += dy.double().t() @ xs[sl].double()
    assert _rel(dW, ref.float()) < 1e-5
    assert torch.equal(dW[:, :sl * E], torch.full((Nout, sl * E), 0.5, device=dev))
    assert _rel(db, (-1.0 + dy.double().sum(0)).float()) < 1e-5


@pytest.mark.parametrize("B,L,seg_cols,nseg,Nout", [(64, 256, 256, 5, 1024), (7, 100, 64, 3, 70), (5, 33, 320, 1, 129)])
def test_linear_maxpts_sparse_backward(dev, B, L, seg_cols, nseg, Nout):
    """pzn_linear_maxpts_{dgrad,wgrad}_f32 (backward of linear + max over the points with one non-zero per (cloud,
    channel)) against the dense float64 products on the scattered gradient; rows hit by many channels and rows hit by
    none, dW / db pre-filled (the kernels add), x given as separate column blocks."""
    import ctypes
    from puzzlenet_amd import _lib
    g = torch.Generator().manual_seed(B * L + Nout)
    Kin = nseg * seg_cols
    W = torch.randn(Nout, Kin, generator=g).to(dev)
    xs = [torch.randn(B * L, seg_cols, generator=g).to(dev) for _ in range(nseg)]
    dg = torch.randn(B, Nout, generator=g).to(dev)
    arg = torch.randint(0, L, (B, Nout), generator=g).to(torch.int32)
    arg[:, : Nout // 2] = arg[:, : Nout // 2] % 3          # half of the channels pile onto three rows
    arg = arg.to(dev)
    st = torch.cuda.current_stream().cuda_stream
    dout = torch.zeros(B, L, Nout, dtype=torch.float64, device=dev)
    dout.scatter_(1, arg.long().unsqueeze(1), dg.double().unsqueeze(1))
    dx = torch.full((B * L, Kin), float("nan"), device=dev)
    ws = torch.empty(_lib.load().pzn_linear_maxpts_workspace_bytes(B, Nout) // 4, dtype=torch.int32, device=dev)
    _lib.call("pzn_linear_maxpts_dgrad_f32", dg.data_ptr(), arg.data_ptr(), W.data_ptr(), B, L, Kin, Nout, ws.data_ptr(),
              dx.data_ptr(), st)
    dx2 = torch.empty_like(dx)
    _lib.call("pzn_linear_maxpts_dgrad_f32", dg.data_ptr(), arg.data_ptr(), W.data_ptr(), B, L, Kin, Nout, ws.data_ptr(),
              dx2.data_ptr(), st)
    assert torch.equal(dx, dx2)                            # fixed summation order: reproducible bit for bit
    ref = dout.reshape(B * L, Nout) @ W.double()
    assert _rel(dx, ref.float()) < 1e-5
    never = (dout != 0).sum(dim=2).reshape(-1) == 0
    assert bool((dx[never] == 0).all())                    # rows no channel selected: exact zeros
    dW = torch.full((Nout, Kin), 0.25, device=dev)
    db = torch.full((Nout,), -2.0, device=dev)
    segs = (ctypes.c_void_p * nseg)(*[x.data_ptr() for x in xs])
    _lib.call("pzn_linear_maxpts_wgrad_f32", dg.data_ptr(), arg.data_ptr(), segs, nseg, seg_cols, B, L, Nout, dW.data_ptr(),
              db.data_ptr(), st)
    ref = 0.25 + dout.reshape(B * L, Nout).t() @ torch.cat(xs, 1).double()
    assert _rel(dW, ref.float()) < 1e-5
    assert _rel(db, (-2.0 + dg.double().sum(0)).float()) < 1e-5


# ---------------------------------------------------------------- chained attention kernels (csrc/attnfused.hip)

@pytest.mark.parametrize("B", [2, 64])
def test_attention_fused_block_intermediates(dev, B):
    """One layerAttention block through pzn_attn_fused_{prep_weights,proj,fwd,bwd_q,bwd_k}: the block output, x - attn v,
    the attention map, ln-sum-exp, and every backward intermediate (dz, delta, dq, u, dk, dv, dx) against float64 at
    1e-5 relative (measured 1e-7 .. 8e-7); B = 64 is the production launch (128 workgroups)."""
    L, E, dk = 256, 256, 64
    M = B * L
    g = torch.Generator().manual_seed(3)
    x = (0.5 * torch.randn(M, E, generator=g)).to(dev)
    wq, wk = [(torch.randn(dk, E, generator=g) / 16).to(dev) for _ in range(2)]
    wv, wo = [(torch.randn(E, E, generator=g) / 16).to(dev) for _ in range(2)]
    bq, bk = [(torch.randn(dk, generator=g) / 4).to(dev) for _ in range(2)]
    bv, bo = [(torch.randn(E, generator=g) / 4).to(dev) for _ in range(2)]
    dr = torch.randn(M, E, generator=g).to(dev)
    args = (x.view(B, L, E), wq, bq, wk, bk, wv, bv, wo, bo, dr.view(B, L, E))
    ref = _attn_block_ref64(*args)
    # the ReLU gate is discrete: an element whose pre-activation is within rounding of zero may be gated differently,
    # which is no kernel error; none may flip away from zero, and where one flips near zero the backward is compared with
    # the float64 backward THROUGH THE DEVICE'S GATES (a flipped element moves dz by a whole dr element)
    got = _fused_block(dev, *args)     # (also: dq holds the same values in its two layouts)
    dz = got["dz"]
    flipped = (dz != 0) != (ref["dz"].reshape(M, E) != 0)
    assert int((flipped & (ref["z"].abs() > 1e-5).reshape(M, E)).sum()) == 0
    assert int(flipped.sum()) <= 4
    if int(flipped.sum()):
        ref = _attn_block_ref64(*args, gate=(dz != 0))
    tol = 1e-5
    for name, val in got.items():
        want = ref[name].reshape(val.shape)
        assert _rel(val.double(), want) < tol, (name, _rel(val.double(), want))


def _attn_block_bf16_spec(x, wq, bq, wk, bk, wv, bv, wo, bo, dr):
    """What the chained kernels compute in the bf16 attention mode, stated in float64: EVERY matrix-product operand is
    rounded to bf16 (round to nearest even) at the point where the fp32 path would split it into three planes, products
    and sums are exact-ish (fp32 on the device), softmax / residuals / gates are fp32.  Same keys as _attn_block_ref64."""
    D = torch.float64
    bf = lambda t: t.to(torch.float32).to(torch.bfloat16).to(D)
    X = x.to(D)
    Xb = bf(X)
    q, k, v = Xb @ bf(wq).T + bq.to(D), Xb @ bf(wk).T + bk.to(D), Xb @ bf(wv).T + bv.to(D)
    qb, kb, vb = bf(q), bf(k), bf(v)
    s = qb @ kb.transpose(1, 2) / 8
    P = torch.softmax(s, dim=-1)
    t = X - bf(P) @ vb
    z = bf(t) @ bf(wo).T + bo.to(D)
    r = X + torch.relu(z)
    DR = dr.to(D)
    dz = DR * (z > 0)
    dt = bf(dz) @ bf(wo)
    dab = bf(-dt)
    dP = dab @ vb.transpose(1, 2)
    delta = (P * dP).sum(-1)
    dS = P * (dP - delta[..., None]) / 8
    dq, dk, dv = bf(dS) @ kb, bf(dS).transpose(1, 2) @ qb, bf(P).transpose(1, 2) @ dab
    u = DR + dt
    dx = u + bf(dq) @ bf(wq) + bf(dk) @ bf(wk) + bf(dv) @ bf(wv)
    return dict(r=r, t=t, map=P, lse=torch.logsumexp(s, dim=-1), dz=dz, delta=delta, dq=dq, u=u, dk=dk, dv=dv, dx=dx, z=z)


def test_attention_fused_block_bf16_mode(dev, attn_bf16):
    """The chained kernels' single-plane instantiation (pzn_attn_set_precision(1): BASELINE configs[4], "bf16 attn with
    MFMA"): one bf16 MFMA per product, every product of the block.  Two checks: (1) against the float64 statement of
    exactly that arithmetic (_attn_block_bf16_spec: operands rounded to bf16 where the default path splits them) at
    2e-3 in relative L2 - the implementation is what it says, an element whose rounding boundary is crossed by fp32
    noise moves by one bf16 step; (2) against the unrounded float64 block at the mode's stated tolerance."""
    from puzzlenet_amd import _lib, ops
    B, L, E, dk = 8, 256, 256, 64
    M = B * L
    g = torch.Generator().manual_seed(3)
    x = (0.5 * torch.randn(M, E, generator=g)).to(dev)
    wq, wk = [(torch.randn(dk, E, generator=g) / 16).to(dev) for _ in range(2)]
    wv, wo = [(torch.randn(E, E, generator=g) / 16).to(dev) for _ in range(2)]
    bq, bk = [(torch.randn(dk, generator=g) / 4).to(dev) for _ in range(2)]
    bv, bo = [(torch.randn(E, generator=g) / 4).to(dev) for _ in range(2)]
    dr = torch.randn(M, E, generator=g).to(dev)
    lib = _lib.load()
    assert lib.pzn_attn_get_precision() == 1
    P = ops._ptrs
    st = torch.cuda.current_stream().cuda_stream
    raw = lambda n: torch.zeros(n, dtype=torch.uint8, device=dev)
    mk = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)
    W = raw(lib.pzn_attn_fused_weight_bytes())
    _lib.call("pzn_attn_fused_prep_weights", wq.data_ptr(), wk.data_ptr(), wv.data_ptr(), wo.data_ptr(), W.data_ptr(), st)
    qkb, vb = lib.pzn_attn_fused_qk_image_bytes(B), lib.pzn_attn_fused_v_image_bytes(B)
    qrp, krp, vrp = raw(qkb), raw(qkb), raw(vb)
    _lib.call("pzn_attn_fused_proj", 1, P([x]), P([W]), P([bq]), P([bk]), P([bv]), B, P([qrp]), P([krp]), P([vrp]), st)
    r, t, lse, amap = mk(M, E), mk(M, E), mk(M), mk(B, L, L)
    mask = torch.zeros((M, 8), dtype=torch.int32, device=dev)
    _lib.call("pzn_attn_fused_fwd", 1, P([x]), P([qrp]), P([krp]), P([vrp]), P([W]), P([bo]), B, P([r]), P([t]), P([mask]),
              P([amap]), P([lse]), 0, 1.0, st)
    dz, u, dq, delta, dqt = mk(M, E), mk(M, E), mk(M, dk), mk(M), mk(M, dk)
    darp = raw(vb)
    _lib.call("pzn_attn_fused_bwd_q", 1, P([dr]), E, None, E, P([mask]), P([qrp]), P([krp]), P([vrp]), P([W]), B, P([dz]), P([u]),
              P([dq]), P([dqt]), P([darp]), P([delta]), st)
    dkk, dvv, dx = mk(M, dk), mk(M, E), mk(M, E)
    _lib.call("pzn_attn_fused_bwd_k", 1, P([qrp]), P([krp]), P([vrp]), P([darp]), P([W]), P([lse]),
              P([delta]), P([u]), P([dqt]), B, P([dkk]), P([dvv]), P([dx]), st)
    untile = ops.attention_tile_image_rows
    got = dict(r=r, t=t, map=amap, lse=lse, dz=dz, delta=delta, dq=dq, u=untile(u, E), dk=dkk, dv=dvv, dx=dx)
    args = (x.view(B, L, E), wq, bq, wk, bk, wv, bv, wo, bo, dr.view(B, L, E))
    spec, exact = _attn_block_bf16_spec(*args), _attn_block_ref64(*args)
    # gates are discrete: compare the backward only where the device's gates are the statement's (a pre-activation within
    # rounding of zero may fall either way; such rows are rare and excluded through dz itself)
    same_gate = ((dz != 0) == (spec["dz"].reshape(M, E) != 0)).all(dim=1)
    assert float(same_gate.float().mean()) > 0.9
    for name in ("r", "t", "map", "lse"):
        assert _l2(got[name], spec[name].reshape(got[name].shape)) < 2e-3, (name, _l2(got[name], spec[name].reshape(got[name].shape)))
    for name in ("r", "t"):
        assert _l2(got[name], exact[name].reshape(got[name].shape)) < 2 * BF16_L2_TOL, name
    assert _l2(got["r"], exact["r"].reshape(M, E)) > 1e-4          # it IS the single-plane path
    # backward against the statement, on clouds whose every gate agrees (dx / dk / dv mix the rows of a cloud)
    ok_cloud = same_gate.view(B, L).all(dim=1)
    # row-local quantities: on every row whose gates agree (always checked)
    for name in ("dz", "delta"):
        a_, b_ = got[name][same_gate], spec[name].reshape(got[name].shape)[same_gate]
        assert _l2(a_, b_) < 5e-3, (name, _l2(a_, b_))
    # the rest mixes the rows of a cloud (dq, u through the softmax's backward; dk, dv, dx sum over the queries): on clouds
    # whose every gate agrees - and there must be some, or the single-plane backward would go unchecked
    assert int(ok_cloud.sum()) >= 1, f"no cloud of {B} has all {L * E} gates equal to the statement's"
    sel = ok_cloud.repeat_interleave(L)
    for name in ("dz", "delta", "dq", "u", "dk", "dv", "dx"):
        a_, b_ = got[name][sel], spec[name].reshape(got[name].shape)[sel]
        assert _l2(a_, b_) < 5e-3, (name, _l2(a_, b_))


@pytest.mark.parametrize("nprob", [1, 2])
def test_attention_chain_fused_map_strips(dev, nprob):
    """map_strips=True (what training_step asks for: model5_b.py:937-942 takes only the row mean of the mean map): the second
    result is [B,16,256] whose mean over dim 1 equals the full [B,256,256] map's (1e-6 of its largest entry: the same 1024
    terms in another order), colmean_argmax picks the same column, the other results are bit-identical and the gradients the
    same (the map carries none)."""
    from puzzlenet_amd import ops
    B, L, E, dk, Nout = 5, 256, 256, 64, 1024
    g = torch.Generator().manual_seed(23)
    shapes = [(dk, E), (dk,), (dk, E), (dk,), (E, E), (E,), (E, E), (E,)]
    xs = [(0.5 * torch.randn(B, L, E, generator=g)).to(dev).requires_grad_(True) for _ in range(nprob)]
    blocks = [[tuple((torch.randn(*s, generator=g) / (math.sqrt(E) if len(s) == 2 else 4)).to(dev).requires_grad_(True)
                     for s in shapes) for _ in range(4)] for _ in range(nprob)]
    ws = [(torch.randn(Nout, 5 * E, generator=g) / math.sqrt(5 * E)).to(dev).requires_grad_(True) for _ in range(nprob)]
    bs = [(0.1 * torch.randn(Nout, generator=g)).to(dev).requires_grad_(True) for _ in range(nprob)]
    go = [torch.randn(B, Nout, generator=g).to(dev) for _ in range(nprob)]
    leaves = xs + [p for bl in blocks for blk in bl for p in blk] + ws + bs
    runs = []
    for strips in (False, True):
        for t in leaves:
            t.grad = None
        res = ops.attention_chain_fused(xs, blocks, ws, bs, need_out=False, map_strips=strips)
        sum((r[2] * go_).sum() for r, go_ in zip(res, go)).backward()
        runs.append((res, [t.grad.clone() for t in leaves]))
    (full, gfull), (strip, gstrip) = runs
    for p in range(nprob):
        assert full[p][1].shape == (B, L, L) and strip[p][1].shape == (B, L // 16, L)
        want, got = full[p][1].mean(dim=1), strip[p][1].mean(dim=1)
        assert float((want - got).abs().max()) <= 1e-6 * float(want.abs().max())
        assert torch.equal(ops.colmean_argmax(full[p][1])[1], ops.colmean_argmax(strip[p][1])[1])
        assert torch.equal(full[p][2], strip[p][2]) and full[p][0] is None and strip[p][0] is None
    top = max(float(b.norm()) for b in gstrip)
    for a, b in zip(gfull, gstrip):      # (the weight gradients end in atomic adds: equal to the order of a sum; the key biases'
        assert float((a - b).norm()) <= 1e-5 * float(b.norm()) + 1e-7 * top      #  gradient is mathematically zero: rounding noise)



@pytest.mark.parametrize("strips", [False, True])
@pytest.mark.parametrize("sinks", [False, True])
def test_attention_chain_one_call_equals_the_composition(dev, strips, sinks):
    """ops._AttnChainOne (csrc/attnchain.hip: the encoder's attention chain enqueued by the library behind one C call each
    way) against ops._AttnChainFused (the same kernels enqueued one by one from Python) in the case predict5 creates
    (no `out`, gradient through the maximum only): map and maximum bit-identical, the input gradient bit-identical, the 34
    parameter gradients equal to the order of their atomic sums - also when they are added into registered sinks."""
    from puzzlenet_amd import ops
    B, L, E, dk, Nout = 6, 256, 256, 64, 1024
    g = torch.Generator().manual_seed(31)
    shapes = [(dk, E), (dk,), (dk, E), (dk,), (E, E), (E,), (E, E), (E,)]
    x0 = (0.5 * torch.randn(B, L, E, generator=g)).to(dev)
    flat0 = [(torch.randn(*s, generator=g) / (math.sqrt(E) if len(s) == 2 else 4)).to(dev) for _ in range(4) for s in shapes]
    flat0 += [(torch.randn(Nout, 5 * E, generator=g) / math.sqrt(5 * E)).to(dev), (0.1 * torch.randn(Nout, generator=g)).to(dev)]
    go = torch.randn(B, Nout, generator=g).to(dev)

    def run(one):
        x = x0.clone().requires_grad_(True)
        flat = [p.clone().requires_grad_(True) for p in flat0]
        ops.clear_grad_sinks()
        if sinks:
            for p in flat:
                p.grad = torch.full_like(p, 0.125)          # pre-existing content: the kernels must ADD to it
            ops.register_grad_sinks(flat)
        if one:
            assert ops.attention_chain_one_supported(x, dk, flat[32])
            amap, fg = ops._AttnChainOne.apply(strips, x, *flat)
        else:
            _, amap, fg = ops._AttnChainFused.apply(1, 2 if strips else 0, x, *flat)
        (fg * go).sum().backward()
        ops.clear_grad_sinks()
        return amap.detach(), fg.detach(), x.grad, [p.grad for p in flat]

    m1, f1, gx1, gp1 = run(True)
    m0, f0, gx0, gp0 = run(False)
    assert torch.equal(m1, m0) and torch.equal(f1, f0) and torch.equal(gx1, gx0)
    top = max(float(b.norm()) for b in gp0)
    for a, b in zip(gp1, gp0):
        assert float((a - b).norm()) <= 1e-5 * float(b.norm()) + 1e-7 * top
    # the one-call form sums the blocks' weight gradients from partial tiles in a fixed order (csrc/attnwgrad.hip with the
    # chain's workspace): the same bits on a second run
    gp2 = run(True)[3]
    for a, b in zip(gp1[:32], gp2[:32]):
        assert torch.equal(a, b)


@pytest.mark.parametrize("M", [64, 1280, 1600, 16384])
@pytest.mark.parametrize("accumulate", [False, True])
def test_attention_weight_gradients_one_launch(dev, M, accumulate):
    """pzn_attn_fused_wgrads at the encoder's shape (E = 256, dk = 64: csrc/attnwgrad.hip, one launch of LDS-shared tiles; without
    a workspace the row ranges meet in atomics) against float64 products: dWo = dz^T t, dWq/k/v = dq/dk/dv^T x and the four
    column sums (backward of model5_b.py:83-101), overwriting and adding to what is there.  M = 64: one row range of four steps;
    1280, 1600: ragged last range; 16 384: the bench shape."""
    from puzzlenet_amd import _lib
    E, dk = 256, 64
    g = torch.Generator().manual_seed(M + int(accumulate))
    dz, t, dv, x = ((torch.randn(M, E, generator=g) * (1 + 3 * torch.rand(1, E, generator=g))).to(dev) for _ in range(4))
    dq, dkk = (torch.randn(M, dk, generator=g).to(dev) for _ in range(2))
    outs = [torch.full(s, 0.5 if accumulate else float("nan"), device=dev)
            for s in ((dk, E), (dk,), (dk, E), (dk,), (E, E), (E,), (E, E), (E,))]      # dWq dbq dWk dbk dWv dbv dWo dbo
    _lib.call("pzn_attn_fused_wgrads", dz.data_ptr(), t.data_ptr(), dq.data_ptr(), dkk.data_ptr(), dv.data_ptr(), x.data_ptr(), M,
              E, dk, *[o.data_ptr() for o in outs], int(accumulate), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    d = lambda a: a.double()
    want = [d(dq).T @ d(x), d(dq).sum(0), d(dkk).T @ d(x), d(dkk).sum(0), d(dv).T @ d(x), d(dv).sum(0), d(dz).T @ d(t), d(dz).sum(0)]
    for name, got, w in zip("dWq dbq dWk dbk dWv dbv dWo dbo".split(), outs, want):
        w = w + (0.5 if accumulate else 0.0)
        err = float((d(got) - w).abs().max())
        assert err <= 1e-5 * float(w.abs().max()), (name, err, float(w.abs().max()))


@pytest.mark.parametrize("nprob,use", [(1, "max"), (2, "max"), (2, "out")])
def test_attention_chain_fused_vs_float64(dev, nprob, use):
    """ops.attention_chain_fused (model5_b.py:462-475 for one or two encoders in the same launches) against a float64
    composition: outputs at 1e-5, every gradient (35 tensors per encoder) at 2e-4 of its maximum (the key biases,
    whose gradient is mathematically zero, against an absolute floor of 5e-5), in relative L2 at 1e-4."""
    from puzzlenet_amd import ops
    B, L, E, dk, Nout = 4, 256, 256, 64, 1024
    g = torch.Generator().manual_seed(11)
    shapes = [(dk, E), (dk,), (dk, E), (dk,), (E, E), (E,), (E, E), (E,)]
    probs = []
    for _ in range(nprob):
        x0 = (0.5 * torch.randn(B, L, E, generator=g)).to(dev)
        blocks0 = [[(torch.randn(*s, generator=g) / (math.sqrt(E) if len(s) == 2 else 4)).to(dev) for s in shapes] for _ in range(4)]
        w0 = (torch.randn(Nout, 5 * E, generator=g) / math.sqrt(5 * E)).to(dev)
        b0 = (0.1 * torch.randn(Nout, generator=g)).to(dev)
        wg = torch.randn(B, Nout, generator=g).to(dev) if use == "max" else (torch.randn(B, L, Nout, generator=g) / 16).to(dev)
        probs.append((x0, blocks0, w0, b0, wg))

    def leafs(dtype):
        out = []
        for x0, blocks0, w0, b0, wg in probs:
            out.append((x0.to(dtype).clone().requires_grad_(True),
                        [[p.to(dtype).clone().requires_grad_(True) for p in blk] for blk in blocks0],
                        w0.to(dtype).clone().requires_grad_(True), b0.to(dtype).clone().requires_grad_(True), wg.to(dtype)))
        return out

    res, grads = {}, {}
    for kind, dtype in (("fused", torch.float32), ("ref", torch.float64)):
        lf = leafs(dtype)
        if kind == "fused":
            assert ops.attention_chain_fused_supported(lf[0][0], dk, lf[0][2])
            out = ops.attention_chain_fused([l[0] for l in lf], [l[1] for l in lf], [l[2] for l in lf], [l[3] for l in lf])
        else:
            out = [_attn_chain_ref64(x, blocks, w, b) for x, blocks, w, b, _ in lf]
        loss = sum((r[2 if use == "max" else 0] * l[4]).sum() for r, l in zip(out, lf))
        loss.backward()
        res[kind] = [(r[0].detach(), r[1].detach(), r[2].detach()) for r in out]
        grads[kind] = [[x.grad] + [p.grad for blk in blocks for p in blk] + [w.grad, b.grad] for x, blocks, w, b, _ in lf]
    for p in range(nprob):
        for a_, b_ in zip(res["fused"][p], res["ref"][p]):
            assert _rel(a_.double(), b_) < 1e-5
        for i, (a_, b_) in enumerate(zip(grads["fused"][p], grads["ref"][p])):
            # (floor: the key biases' gradient is mathematically zero; what is left is the rounding noise of B*L*L terms, ~1e-5)
            assert float((a_.double() - b_).abs().max()) < 2e-4 * max(float(b_.abs().max()), 0.25), i
            if float(b_.norm()) > 1e-3:
                assert _rel(a_.double(), b_) < 1e-4, i


@pytest.mark.parametrize("B,N", [(3, 100), (8, 2048)])
def test_cat_global_linear_relu_vs_torch(dev, B, N):
    """First layer of the boundary heads (model5_b.py:745-752) without the repeat + concatenation: relu(Linear(cat([g.repeat,
    x], -1))) as a per-point product + a per-cloud bias, forward and every gradient against the float64 composition."""
    from puzzlenet_amd import ops
    C, Cg, Co = 64, 64, 64
    g_ = torch.Generator().manual_seed(11)
    x = torch.randn(B, N, C, generator=g_)
    gl = torch.randn(B, 1, Cg, generator=g_)
    w = torch.randn(Co, Cg + C, generator=g_) / (Cg + C) ** 0.5
    b = 0.1 * torch.randn(Co, generator=g_)
    go = torch.randn(B, N, Co, generator=g_)
    ts = [t.to(dev).requires_grad_(True) for t in (x, gl, w, b)]
    y = ops.cat_global_linear_relu(*ts)
    (y * go.to(dev)).sum().backward()
    td = [t.double().requires_grad_(True) for t in (x, gl, w, b)]
    ref = torch.relu(torch.nn.functional.linear(torch.cat([td[1].expand(-1, N, -1), td[0]], dim=-1), td[2], td[3]))
    (ref * go.double()).sum().backward()

    def rel(a, r):
        return float((a.detach().cpu().double() - r).norm() / (r.norm() + 1e-30))
    assert rel(y, ref.detach()) < 1e-5
    for name, t, r in zip(("dx", "dg", "dW", "db"), ts, td):
        assert rel(t.grad, r.grad) < 1e-4, name


@pytest.mark.parametrize("B,need_out", [(2, True), (5, False), (16, True)])
def test_outproj_maxpts_vs_float64(dev, B, need_out):
    """csrc/outproj.hip through the C ABI: cat(x_0..x_4) W^T + b and the max over the 256 points (model5_b.py:466-475) against
    float64; B = 5 takes the plain block order (4 B workgroups not a multiple of 8), out = NULL writes only the maximum;
    two identical points in every cloud pin the tie rule (the lower point wins, as torch.max)."""
    import os
    from puzzlenet_amd import _lib, ops
    L, E, Nout = 256, 256, 1024
    M = B * L
    g = torch.Generator().manual_seed(21 + B)
    xs = [torch.randn(B, L, E, generator=g) for _ in range(5)]
    for x in xs:
        x[:, 200] = x[:, 37]                     # points 37 and 200 of every cloud coincide in all five slices
    w = torch.randn(Nout, 5 * E, generator=g) / (5 * E) ** 0.5
    b = 0.1 * torch.randn(Nout, generator=g)
    xd = [x.reshape(M, E).contiguous().to(dev) for x in xs]
    wd, bd = w.to(dev), b.to(dev)
    lib = _lib.load()
    ws = torch.empty(lib.pzn_outproj_maxpts_workspace_bytes(L, E, 5, Nout), dtype=torch.uint8, device=dev)
    assert ws.numel() > 0
    out = torch.full((M, Nout), float("nan"), device=dev) if need_out else None
    fmax = torch.empty(B, Nout, device=dev)
    arg = torch.empty(B, Nout, dtype=torch.int32, device=dev)
    _lib.call("pzn_outproj_maxpts_fwd_f32", ops._ptrs(xd), 5, wd.data_ptr(), bd.data_ptr(), B, L, E, Nout,
              out.data_ptr() if need_out else None, fmax.data_ptr(), arg.data_ptr(), ws.data_ptr(),
              torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    ref = torch.cat([x.double() for x in xs], dim=-1) @ w.double().T + b.double()          # [B, L, Nout]
    rmax, rarg = ref.max(dim=1)
    if need_out:
        assert _rel(out.cpu().view(B, L, Nout), ref) < 2e-6
    assert float((fmax.cpu().double() - rmax).abs().max()) < 1e-5 * float(rmax.abs().max())
    a = arg.cpu().long()
    assert int(a.min()) >= 0 and int(a.max()) < L
    # the kernel's arg-max row reaches the maximum to rounding, and never names point 200 (its twin 37 is lower)
    picked = ref.gather(1, a.unsqueeze(1)).squeeze(1)
    assert float((picked - rmax).abs().max()) < 1e-5 * float(rmax.abs().max())
    assert int((a == 200).sum()) == 0
    assert float((a == rarg).float().mean()) > 0.999


@pytest.mark.parametrize("B,N,S,C", [(3, 300, 100, 128), (5, 512, 500, 256), (1, 64, 8, 256)])
def test_sa_level_streamed_vs_float64(dev, B, N, S, C):
    """csrc/salevel.hip through pzn_sa_level_fwd_ws_f32 on ragged group counts (G = 300: one round with idle wavefronts;
    2500: two rounds, the second partly empty; 8: the minimum): max and arg-max over the 32 generated rows against float64
    and against the weight-stationary kernel."""
    from puzzlenet_amd import _lib
    g = torch.Generator().manual_seed(C + S)
    P = torch.randn(B * N, C, generator=g).to(dev)
    Q = (0.3 * torch.randn(B * S, C, generator=g)).to(dev)
    idx = torch.randint(0, N, (B, S, 32), generator=g).to(dev)
    w2 = (torch.randn(C, C, generator=g) / C ** 0.5).to(dev)
    b2 = (0.1 * torch.randn(C, generator=g)).to(dev)
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    R = B * S
    ws = torch.empty(lib.pzn_sa_level_fwd_workspace_bytes(C, C), dtype=torch.uint8, device=dev)
    assert ws.numel() == C * C * 6
    res = []
    for use_ws in (True, False):
        out = torch.full((R, C), float("nan"), device=dev)
        arg = torch.full((R, C), -1, dtype=torch.int32, device=dev)
        if use_ws:
            _lib.call("pzn_sa_level_fwd_ws_f32", P.data_ptr(), Q.data_ptr(), idx.data_ptr(), w2.data_ptr(), b2.data_ptr(), B, N, S,
                      C, C, out.data_ptr(), arg.data_ptr(), ws.data_ptr(), st)
        else:
            _lib.call("pzn_sa_level_fwd_f32", P.data_ptr(), Q.data_ptr(), idx.data_ptr(), w2.data_ptr(), b2.data_ptr(), B, N, S, C,
                      C, out.data_ptr(), arg.data_ptr(), st)
        res.append((out, arg))
    torch.cuda.synchronize()
    (o1, a1), (o0, a0) = res
    rows = torch.relu(P.double().view(B, N, C)[torch.arange(B, device=dev)[:, None, None], idx] + Q.double().view(B, S, 1, C))
    ref = torch.relu(rows @ w2.double().T + b2.double())                 # [B, S, 32, C]
    rmax = ref.max(dim=2).values.view(R, C)
    assert bool(torch.isfinite(o1).all()) and int(a1.min()) >= 0 and int(a1.max()) < 32
    assert float((o1.double() - rmax).abs().max()) < 2e-6 * max(1.0, float(rmax.abs().max()))
    assert float((o1 - o0).abs().max()) < 1e-5
    assert float((a1 != a0).float().mean()) < 1e-4
    picked = ref.view(R, 32, C).gather(1, a1.long().unsqueeze(1)).squeeze(1)
    assert float((picked - rmax).abs().max()) < 1e-5
    # the two halves as their own entry points (weight split, then the level on the prepared workspace): the same bits
    import os
    if R >= 8:
        ws2 = torch.empty_like(ws)
        o2 = torch.full((R, C), float("nan"), device=dev)
        a2 = torch.full((R, C), -1, dtype=torch.int32, device=dev)
        _lib.call("pzn_sa_level_prep_weights_f32", w2.data_ptr(), C, C, ws2.data_ptr(), st)
        _lib.call("pzn_sa_level_fwd_packed_f32", P.data_ptr(), Q.data_ptr(), idx.data_ptr(), b2.data_ptr(), B, N, S, C, C,
                  o2.data_ptr(), a2.data_ptr(), ws2.data_ptr(), st)
        torch.cuda.synchronize()
        assert torch.equal(o2, o1) and torch.equal(a2, a1)


@pytest.mark.parametrize("B,N,C2,C3,per_cloud", [(2, 64, 64, 64, False), (3, 96, 32, 2, True), (3, 160, 64, 64, False),
                                                  (4, 2048, 32, 2, True), (5, 2048, 64, 64, False), (1, 32, 32, 2, True),
                                                  # three tiles per wavefront with a ragged last one / four (a divisor of the
                                                  # cloud's 64 tiles) / a cloud of 4096 points
                                                  (33, 2048, 64, 64, False), (33, 2048, 32, 2, True), (9, 4096, 32, 2, True)])
def test_point_mlp3_vs_float64(dev, B, N, C2, C3, per_cloud):
    """csrc/pointmlp.hip through ops.point_mlp3: the boundary heads' three-layer chains (model5_b.py:571-592, 738-754) in one
    launch each way against float64 autograd — output and every gradient, with the global half of the first layer
    (per_cloud: cat([g.repeat(1, N, 1), x], -1), :745-749) folded into a per-cloud bias.  Sizes cover one tile per
    wavefront, several tiles per wavefront (the walk with the next operands in flight) and a lone tile."""
    from puzzlenet_amd import ops
    if not ops.point_mlp3_available(64, 64, C2, C3):
        pytest.skip("PZN_POINT_MLP=0 turns the fused chains off")
    g = torch.Generator().manual_seed(7 + C2 + B)
    x = torch.randn(B, N, 64, generator=g)
    gl = torch.randn(B, 1, 64, generator=g) if per_cloud else None
    W1 = torch.randn(64, 128 if per_cloud else 64, generator=g) / 8
    b1 = 0.1 * torch.randn(64, generator=g)
    W2, b2 = torch.randn(C2, 64, generator=g) / 8, 0.1 * torch.randn(C2, generator=g)
    W3, b3 = torch.randn(C3, C2, generator=g) / C2 ** 0.5, 0.1 * torch.randn(C3, generator=g)
    go = torch.randn(B, N, C3, generator=g)
    leaves = [x, W1, b1, W2, b2, W3, b3] + ([gl] if per_cloud else [])
    ref = [t.double().requires_grad_(True) for t in leaves]
    xin = torch.cat([ref[7].expand(-1, N, -1), ref[0]], -1) if per_cloud else ref[0]
    yr = F.linear(F.relu(F.linear(F.relu(F.linear(xin, ref[1], ref[2])), ref[3], ref[4])), ref[5], ref[6])
    (yr * go.double()).sum().backward()
    d = [t.to(dev).requires_grad_(True) for t in leaves]
    y = ops.point_mlp3(d[0], d[1], d[2], d[3], d[4], d[5], d[6], g=d[7] if per_cloud else None)
    assert y.shape == (B, N, C3)
    assert _rel(y, yr) < 1e-5
    (y * go.to(dev)).sum().backward()
    for name, a, r in zip(("x", "W1", "b1", "W2", "b2", "W3", "b3", "g"), d, ref):
        assert _rel(a.grad, r.grad) < 2e-5, name
    # the same result on a second call (fixed summation order of the partial sums)
    first = [t.grad.clone() for t in d]
    for t in d:
        t.grad = None
    (ops.point_mlp3(d[0], d[1], d[2], d[3], d[4], d[5], d[6], g=d[7] if per_cloud else None) * go.to(dev)).sum().backward()
    for a, f in zip(d, first):
        assert torch.equal(a.grad, f)


@pytest.mark.parametrize("C2,C3,per_cloud", [(64, 64, False), (32, 2, True)])
def test_point_mlp3_full_size_c_abi(dev, C2, C3, per_cloud):
    """The heads' full shape (64 x 2048 rows: four tiles per wavefront, 256 workgroups of partial sums) through the C ABI
    (pzn_point_mlp3_fwd_f32 / _bwd_f32) against float64.  With 16.8 M hidden units a pre-activation within fp32 rounding
    of zero turns up, and its gate is then a coin flip, not an error: the float64 backward takes the gates of the device
    activations (as tests above do for single layers)."""
    from puzzlenet_amd import _lib, ops
    if not ops.point_mlp3_available(64, 64, C2, C3):
        pytest.skip("PZN_POINT_MLP=0 turns the fused chains off")
    B, N = 64, 2048
    M = B * N
    g = torch.Generator().manual_seed(C2)
    x = torch.randn(M, 64, generator=g)
    W1, W2, W3 = torch.randn(64, 64, generator=g) / 8, torch.randn(C2, 64, generator=g) / 8, torch.randn(C3, C2, generator=g) / C2 ** 0.5
    b1 = torch.randn(B, 64, generator=g) if per_cloud else 0.1 * torch.randn(64, generator=g)
    b2, b3 = 0.1 * torch.randn(C2, generator=g), 0.1 * torch.randn(C3, generator=g)
    dy = torch.randn(M, C3, generator=g)
    d = {k: v.to(dev) for k, v in dict(x=x, W1=W1, b1=b1, W2=W2, b2=b2, W3=W3, b3=b3, dy=dy).items()}
    mk = lambda *sh: torch.empty(sh, dtype=torch.float32, device=dev)
    h1, h2, y = mk(M, 64), mk(M, C2), mk(M, C3)
    p = lambda t: t.data_ptr()
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.pzn_point_mlp3_fwd_f32(p(d["x"]), M, N, p(d["W1"]), 64, p(d["b1"]), int(per_cloud), p(d["W2"]), p(d["b2"]),
                                          p(d["W3"]), p(d["b3"]), C2, C3, p(h1), p(h2), p(y), st), "fwd")
    ws = torch.empty(lib.pzn_point_mlp3_bwd_workspace_bytes(M, N, int(per_cloud), C2, C3), dtype=torch.uint8, device=dev)
    dx, dW1, dW2, dW3, db2, db3 = mk(M, 64), mk(64, 64), mk(C2, 64), mk(C3, C2), mk(C2), mk(C3)
    db1 = mk(B, 64) if per_cloud else mk(64)
    _lib.check(lib.pzn_point_mlp3_bwd_f32(p(d["dy"]), p(d["x"]), p(h1), p(h2), M, N, p(d["W1"]), 64, int(per_cloud), p(d["W2"]),
                                          p(d["W3"]), C2, C3, p(dx), p(dW1), p(db1), p(dW2), p(db2), p(dW3), p(db3), 0, p(ws), st), "bwd")
    # accumulate != 0: the parameter gradients are added to what the buffers hold (here: 1.0 everywhere -> the result + 1);
    # dx and the per-cloud db1 are overwritten either way
    acc = [torch.ones_like(t) for t in (dW1, db1, dW2, db2, dW3, db3)]
    dx2 = torch.full_like(dx, 7.0)
    _lib.check(lib.pzn_point_mlp3_bwd_f32(p(d["dy"]), p(d["x"]), p(h1), p(h2), M, N, p(d["W1"]), 64, int(per_cloud), p(d["W2"]),
                                          p(d["W3"]), C2, C3, p(dx2), p(acc[0]), p(acc[1]), p(acc[2]), p(acc[3]), p(acc[4]),
                                          p(acc[5]), 1, p(ws), st), "bwd accumulate")
    torch.cuda.synchronize()
    assert torch.equal(dx2, dx)
    for t, want, fresh in zip(acc, (dW1, db1, dW2, db2, dW3, db3), (False, bool(per_cloud), False, False, False, False)):
        assert torch.equal(t, want if fresh else want + 1.0)
    r = {k: v.double().requires_grad_(k != "dy") for k, v in dict(x=x, W1=W1, b1=b1, W2=W2, b2=b2, W3=W3, b3=b3, dy=dy).items()}
    bias1 = r["b1"].repeat_interleave(N, 0) if per_cloud else r["b1"]
    z1 = r["x"] @ r["W1"].t() + bias1
    g1, g2 = h1.cpu() > 0, h2.cpu() > 0
    assert int((g1 != (z1.detach() > 0)).sum()) <= 8
    a1 = torch.where(g1, z1, torch.zeros_like(z1))
    z2 = a1 @ r["W2"].t() + r["b2"]
    assert int((g2 != (z2.detach() > 0)).sum()) <= 8
    a2 = torch.where(g2, z2, torch.zeros_like(z2))
    yr = a2 @ r["W3"].t() + r["b3"]
    (yr * r["dy"]).sum().backward()
    assert _rel(h1, a1) < 1e-5 and _rel(h2, a2) < 1e-5 and _rel(y, yr) < 1e-5
    for name, a, ref in (("dx", dx, r["x"].grad), ("dW1", dW1, r["W1"].grad), ("dW2", dW2, r["W2"].grad), ("dW3", dW3, r["W3"].grad),
                         ("db1", db1, r["b1"].grad), ("db2", db2, r["b2"].grad), ("db3", db3, r["b3"].grad)):
        assert _rel(a, ref) < 1e-5, name
