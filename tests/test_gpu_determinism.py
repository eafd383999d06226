"""Reproducibility, forward and backward: with the same inputs (and the same FPS start indices) a stage must give the same
outputs run after run - bit-identical where no kernel sums with atomics (point ops, set abstraction, attention; backward:
see the EXACT rows of BACKWARD_TABLE below), within summation-order noise where partial sums meet in fp32 atomics (forward:
the few-row pose head, 5e-6 of the largest entry, measured 2.5e-7; backward: the ATOMIC rows of the table, each with the file
and line of its atomic add).  A larger difference means a race between wavefronts or streams, or a lost update.  The stages
are checked separately so that a failure names its kernel; the backward stages run at the benchmarked shapes (B = 64) and at
one small odd shape each, alone and beside an unrelated GEMM on a second stream, with and without registered gradient
sinks."""
import math

import numpy as np
import pytest
import torch

from oracle import model_ref as mr
from tests._oracle_compare import check_reorder

pytestmark = pytest.mark.gpu
REPS = 12


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _same(a, b):
    if isinstance(a, torch.Tensor):
        return torch.equal(a, b)
    return all(_same(x, y) for x, y in zip(a, b))


def _rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def test_knn_and_group_repeatable(golden_model, dev):
    from puzzlenet_amd import ops
    G = golden_model
    xyz = _t(G["p5_batch0"], dev)
    g = torch.Generator().manual_seed(5)
    feat = torch.randn(xyz.shape[0], xyz.shape[1], 64, generator=g).to(dev)
    new_xyz = xyz[:, ::2].contiguous()
    first = None
    for _ in range(REPS):
        idx = ops.knn(xyz, new_xyz, 32)
        out, gx, idx2 = ops.knn_group(xyz, feat, new_xyz)
        cur = tuple(t for t in (idx, out, gx, idx2) if t is not None)
        first = first or cur
        assert _same(cur, first)
        assert torch.equal(idx, idx2)


@pytest.mark.parametrize("two_streams", [False, True])
def test_predict5_forward_repeatable(golden_model, dev, two_streams):
    from puzzlenet_amd import model5_b as mb
    G = golden_model
    m = mb.TouchedRegraster(mr.Cfg())
    mr.fill_params(m)
    m.to(dev)
    m.two_streams = two_streams
    batch = [_t(G[f"p5_batch{i}"], dev) for i in range(8)]
    first = None
    names = ["pose", "x2", "attention", "mrpc_x2", "mrpc_attention", "de_fpcb", "de_mrpcb"]
    for r in range(REPS):
        torch.manual_seed(2024)
        with torch.no_grad():
            out = m.predict5(batch, 4, need=True, training=True)
        cur = [out[0], out[2], out[3], out[4], out[5], out[6], out[7]]
        torch.cuda.synchronize()
        if first is None:
            first = [t.clone() for t in cur]
            continue
        rel = {n: _rel(a, b) for n, a, b in zip(names, cur, first)}
        bad = {n: v for n, v in rel.items() if v > (5e-6 if n in ("pose", "de_fpcb", "de_mrpcb") else 0.0)}
        assert not bad, f"run {r}: {bad} differ from run 0"


def test_encoder_stages_repeatable(golden_model, dev):
    """the encoder's stages one by one on the same inputs: set abstraction (search + P'/Q + generated-row max-pool kernel),
    attention chain node"""
    from puzzlenet_amd import model5_b as mb, ops
    G = golden_model
    m = mb.TouchedRegraster(mr.Cfg())
    mr.fill_params(m)
    m.to(dev)
    enc = m.Encoder
    xyz = _t(G["p5_batch0"], dev)
    with torch.no_grad():
        xf = enc.local_features(xyz)
        xf = xf[0] if isinstance(xf, tuple) else xf      # (the fused stem returns its output under two names)
        f1 = ops.farthest_point_sample(xyz, 512, torch.zeros(xyz.shape[0], dtype=torch.long, device=dev))
        x1 = ops.index_points(xyz, f1)
        f2 = ops.farthest_point_sample(x1, 256, torch.zeros(xyz.shape[0], dtype=torch.long, device=dev))
        x2 = ops.index_points(x1, f2)
        first = None
        for r in range(REPS):
            xf_r = enc.local_features(xyz)
            xf_r = xf_r[0] if isinstance(xf_r, tuple) else xf_r
            a = ops.sa_mlp_max(xyz, xf, x1, None, enc.mlp3.weight, enc.mlp3.bias, enc.mlp4.weight, enc.mlp4.bias)
            b = ops.sa_mlp_max(x1, a, x2, None, enc.mlp5.weight, enc.mlp5.bias, enc.mlp6.weight, enc.mlp6.bias)
            cur = {"local_features": xf_r, "sa1": a, "sa2": b}
            x = b
            for i, blk in enumerate((enc.atten1, enc.atten2, enc.atten3, enc.atten4)):
                x, amap = blk(x)
                cur[f"att{i + 1}"], cur[f"map{i + 1}"] = x, amap
            cur["out"] = ops.linear(torch.cat([cur["att1"], cur["att2"], cur["att3"], cur["att4"], b], dim=-1),
                                      enc.out.weight, enc.out.bias)
            cur["max"] = ops.max_over_points(cur["out"])
            torch.cuda.synchronize()
            if first is None:
                first = {k: v.clone() for k, v in cur.items()}
                continue
            bad = {k: _rel(cur[k], first[k]) for k in cur if not torch.equal(cur[k], first[k])}
            assert not bad, f"run {r}: {bad} differ from run 0"


# ---- backward stages ------------------------------------------------------------------------------------------------------
# Every output tensor of every backward stage, in one of two classes.
#   EXACT   torch.equal with run 0: no kernel on its way adds to it atomically (partial tiles summed in a fixed order, or one
#           owner per element).
#   ATOMIC  partial sums meet in fp32 atomics, so the order of the sum differs between runs: (file:line of the atomic add).
#           At B = 64 held to the file's rule for atomic epilogues, 5e-6 of the tensor's largest entry; at the stage's small
#           odd shape to the derived bounds of tests/_oracle_compare.reorder_bounds (worst case 2 n 2^-24 sum|t_i| and
#           8 sqrt(n) 2^-24 sum|t_i|, sum|t_i| restated in float64 on the CPU), which a single lost term breaks.
EXACT, ATOMIC = "EXACT", "ATOMIC"
_BLOCK = ("wq", "bq", "wk", "bk", "wv", "bv", "wo", "bo")
BACKWARD_TABLE = {
    # csrc/sachain.hip: pzn_sa_level_chain_bwd_f32 (inverse lists, walk by point, pooled weight gradients, dP -> features)
    "sa_level": {
        "y": (EXACT,), "dfeat": (EXACT,), "dW2": (EXACT,), "db2": (EXACT,),      # dP by owner; pool_wgrad partial tiles (poolbwd.hip)
        # columns 0:3 by the walk (sapool.hip:257), columns 3: = dP^T feat through pzn_linear_slice_wgrad_f32 (dfgemm.hip:207, or
        # the general engine's split-K epilogue gemm.hip:587 where the direct-fragment kernel does not take the shape)
        "dW1": (ATOMIC, "puzzlenet_amd/csrc/sapool.hip:257, puzzlenet_amd/csrc/dfgemm.hip:207, puzzlenet_amd/csrc/gemm.hip:587"),
        "db1": (ATOMIC, "puzzlenet_amd/csrc/sapool.hip:259"),
    },
    # csrc/attnchain.hip: pzn_attn_chain_bwd_f32; block gradients from partial tiles (attnwgrad.hip, attn_wgrad_reduce_kernel),
    # the out projection's sparse backward without atomics (maxptsbwd.hip: sorted winners, one owner per element)
    "attn_chain": dict([("map", (EXACT,)), ("max", (EXACT,)), ("dx", (EXACT,)), ("out.weight", (EXACT,)), ("out.bias", (EXACT,))] +
                       [(f"block{i}.{n}", (EXACT,)) for i in range(4) for n in _BLOCK]),
    # csrc/gemm.hip: pzn_attn_block_bwd_f32 (the block on its own): dx through accumulate epilogues on one stream; the weight
    # gradients through pzn_df_wgrad3 / pzn_linear_wgrad_f32, whose row ranges meet in atomics
    "attention_block": dict([("r", (EXACT,)), ("attn", (EXACT,)), ("dx", (EXACT,))] +
                            [(n, (ATOMIC, "puzzlenet_amd/csrc/dfgemm.hip:207 (weights), :212 (biases); puzzlenet_amd/csrc/gemm.hip:587"))
                             for n in _BLOCK]),
    # csrc/stem.hip: the layers' gradients from the workgroups' parts in a fixed order (stem_reduce_kernel); the BatchNorm
    # gradients are ONE add per point and launch (stem.hip:391-392, 445-446: thread 0 of the workgroup that owns point n), so
    # there is no order to differ in
    "stem": {"y": (EXACT,), "lin1.weight": (EXACT,), "lin1.bias": (EXACT,), "lin2.weight": (EXACT,), "lin2.bias": (EXACT,),
             "bn1.weight": (EXACT,), "bn1.bias": (EXACT,), "bn2.weight": (EXACT,), "bn2.bias": (EXACT,)},
    # csrc/pointmlp.hip: partial sums in a fixed order, one owner per element.  With a global half (per-cloud bias) the [B, 64]
    # products behind it go through the general engine's few-row / weight-gradient paths, which keep the atomic epilogue
    "point_mlp3": {"y": (EXACT,), "dx": (EXACT,), "dW2": (EXACT,), "db2": (EXACT,), "dW3": (EXACT,), "db3": (EXACT,),
                   "dW1": (EXACT,), "db1": (EXACT,)},
    "point_mlp3_per_cloud": {"y": (EXACT,), "dx": (EXACT,), "dW2": (EXACT,), "db2": (EXACT,), "dW3": (EXACT,), "db3": (EXACT,),
                             "dW1.local": (EXACT,),
                             "dW1.global": (ATOMIC, "puzzlenet_amd/csrc/dfgemm.hip:207, puzzlenet_amd/csrc/gemm.hip:587"),
                             "db1": (ATOMIC, "puzzlenet_amd/csrc/dfgemm.hip:212, puzzlenet_amd/csrc/gemm.hip:587"),
                             "dg": (ATOMIC, "puzzlenet_amd/csrc/gemm.hip:587")},
}
ATOMIC_REL = 5e-6          # of the tensor's largest entry: the rule of test_predict5_forward_repeatable above
SINK_FILL = 0.25           # what registered gradient buffers hold before the kernels add to them


def test_backward_table_is_not_vacuous():
    must = [("sa_level", n) for n in ("dfeat", "dW2", "db2")] + [("attn_chain", f"block{i}.{n}") for i in range(4)
                                                                   for n in ("wq", "wk", "wv", "wo")]
    for stage, name in must:
        assert BACKWARD_TABLE[stage][name] == (EXACT,), (stage, name)
    for stage, rows in BACKWARD_TABLE.items():
        for name, row in rows.items():
            assert row[0] in (EXACT, ATOMIC) and (row[0] == EXACT or (len(row) == 2 and ".hip:" in row[1])), (stage, name)


class _Aggressor:
    """An unrelated GEMM kept busy on a second stream (the general matrix-core engine, AGPR accumulators: the aggressor of
    tests/test_gpu_concurrency.py).  A victim run here lasts from tens of microseconds to milliseconds, so the number of
    launches in front of a run is sized from event times: 1.5 times the victim's own duration, the backward included."""

    def __init__(self, dev):
        g = torch.Generator().manual_seed(3)
        self.x = torch.randn(4096, 1280, generator=g).to(dev)
        self.w = (torch.randn(1024, 1280, generator=g) / 30).to(dev)
        self.y = torch.empty(4096, 1024, device=dev)
        self.side = torch.cuda.Stream()
        self.launches = 2

    def size_for(self, run):
        run()                                                   # (first call: allocator, lazy loads)
        torch.cuda.synchronize()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        ev[0].record()
        run()
        ev[1].record()
        self.start()
        ev[2].record(self.side)
        self(8)
        ev[3].record(self.side)
        torch.cuda.synchronize()
        victim, one = ev[0].elapsed_time(ev[1]), ev[2].elapsed_time(ev[3]) / 8
        self.launches = max(2, min(512, math.ceil(1.5 * victim / max(one, 1e-3))))
        return victim, one

    def start(self):
        self.side.wait_stream(torch.cuda.current_stream())

    def __call__(self, n=None):
        from puzzlenet_amd.ops import _call, _p
        for _ in range(n or self.launches):
            _call("pzn_linear_fwd_f32", _p(self.x), _p(self.w), None, 4096, 1280, 1024, 0, _p(self.y), self.side.cuda_stream)


def _repeat(stage, run, dev, reps, bounds=None):
    """run() -> {name: tensor}, `reps` times alone and `reps` times beside the aggressor, every run against run 0 according
    to BACKWARD_TABLE[stage].  bounds: {name: (n, sum|t_i| float64 on the CPU)} for the ATOMIC rows (the small shapes) - the
    derived bounds replace the 5e-6 rule there."""
    table = BACKWARD_TABLE[stage]
    agg = _Aggressor(dev)
    victim_ms, agg_ms = agg.size_for(run)
    first = None
    seen = {}
    for mode in ("alone", "beside a GEMM"):
        if mode != "alone":
            agg.start()
        for r in range(reps):
            if mode != "alone":
                agg()
            cur = run()
            torch.cuda.synchronize()
            assert set(cur) == set(table), (stage, sorted(set(cur) ^ set(table)))
            if first is None:
                first = {k: v.detach().clone() for k, v in cur.items()}
                for k, v in first.items():
                    assert bool(torch.isfinite(v).all()) and float(v.abs().max()) > 0, (stage, k, "empty or not finite")
                continue
            for k, v in cur.items():
                if table[k][0] == EXACT:
                    if not torch.equal(v, first[k]):
                        d = (v != first[k])
                        rows = d.reshape(d.shape[0], -1).any(1).nonzero().flatten()[:8].tolist() if d.dim() > 1 else []
                        raise AssertionError(f"{stage}.{k} run {r} ({mode}) differs from run 0 in {int(d.sum())} of {d.numel()} "
                                             f"entries, max |diff| {float((v - first[k]).abs().max()):.3e}, first rows {rows}")
                    continue
                rel = _rel(v, first[k])
                seen[k] = max(seen.get(k, 0.0), rel)
                if bounds is not None:
                    n, sum_abs = bounds[k]
                    check_reorder(f"{stage}.{k} run {r} ({mode})", v.cpu(), first[k].cpu(), n, sum_abs)
                else:
                    assert rel <= ATOMIC_REL, f"{stage}.{k} run {r} ({mode}): {rel:.3e} of the largest entry (atomic add at {table[k][1]})"
    torch.cuda.synchronize()
    print(f"{stage}: victim {victim_ms:.3f} ms, aggressor launch {agg_ms:.3f} ms x {agg.launches} per run; ATOMIC outputs, largest "
          f"run-to-run difference / largest entry: {({k: float(f'{v:.2e}') for k, v in seen.items()})}")


def _with_sinks(ps, sinks):
    from puzzlenet_amd import ops
    ops.clear_grad_sinks()
    if sinks:
        for p in ps:
            p.grad = torch.full_like(p, SINK_FILL)          # pre-existing content: the kernels must ADD to it
        ops.register_grad_sinks(ps)


def _level_case(dev, shape):
    B, N, S, D, C1, C2 = shape
    g = torch.Generator().manual_seed(C1 + N + B)
    xyz = torch.rand(B, N, 3, generator=g)
    feat = torch.randn(B, N, D, generator=g)
    w = [torch.randn(C1, 3 + D, generator=g) / math.sqrt(3 + D), 0.1 * torch.randn(C1, generator=g),
         torch.randn(C2, C1, generator=g) / math.sqrt(C1), 0.1 * torch.randn(C2, generator=g)]
    go = torch.randn(B, S, C2, generator=g)
    return xyz, feat, w, go


def _level_sum_abs(xyz, feat, w, go, S, sinks):
    """sum|t_i| of the first layer's gradients of a level, float64 on the CPU, the gates as 0/1 masks: rows [B, S, 32] of
    [xyz[j] - centre | feat[j]], dH2 = go at the max-pool winner where the output is positive, |dH1| = gate1 (|dH2| |W2|),
    dW1 = dH1^T X, db1 = column sums: n = B S 32 rows (+ 1: the registered buffer's content)."""
    from oracle import point_ops as orc
    B, N, D = feat.shape
    idx = torch.from_numpy(orc.knn(xyz.numpy(), xyz[:, :S].contiguous().numpy(), 32))
    bi = torch.arange(B)[:, None, None]
    X = torch.cat([xyz[bi, idx] - xyz[:, :S, None], feat[bi, idx]], -1).double()              # [B, S, 32, 3 + D]
    w1, b1, w2, b2 = (t.double() for t in w)
    h1 = X @ w1.t() + b1
    h2 = torch.relu(h1) @ w2.t() + b2
    best, arg = h2.max(dim=2)
    dh2 = torch.zeros_like(h2).scatter_(2, arg.unsqueeze(2), (go.double().abs() * (best > 0)).unsqueeze(2))
    dh1 = (dh2 @ w2.abs()) * (h1 > 0)
    n = B * S * 32 + int(sinks)
    fill = SINK_FILL if sinks else 0.0
    return {"dW1": (n, torch.einsum("bskc,bskq->cq", dh1, X.abs()) + fill), "db1": (n, dh1.sum((0, 1, 2)) + fill)}


@pytest.mark.parametrize("sinks", [False, True])
@pytest.mark.parametrize("shape", [(64, 2048, 512, 64, 128, 128), (64, 512, 256, 128, 256, 256), (2, 300, 40, 64, 128, 128)])
def test_sa_level_backward_repeatable(dev, shape, sinks):
    """A set-abstraction level forward + backward through ops.sa_mlp_max in the one-call form the model takes
    (pzn_sa_level_chain_fwd/bwd_f32), both production shapes and a small one with partial tiles; the neighbour search runs
    inside the call.  EXACT: output, feature gradient (it carries dP), dW2, db2.  ATOMIC: dW1, db1 (seen: up to 7.4e-7 of the
    largest entry at B = 64).  0.05-0.15 s per case on an MI355X (1.7 s for the first, which loads the library)."""
    from puzzlenet_amd import ops
    B, N, S, D, C1, C2 = shape
    xyz_c, feat_c, w_c, go_c = _level_case(dev, shape)
    xyz, feat0, go = xyz_c.to(dev), feat_c.to(dev), go_c.to(dev)
    new_xyz = xyz[:, :S].contiguous()
    w = [t.to(dev) for t in w_c]
    assert not ops.KernelTimer.enabled

    def run():
        feat = feat0.detach().requires_grad_(True)
        ps = [t.clone().requires_grad_(True) for t in w]
        _with_sinks(ps, sinks)
        assert ops.sa_level_fused_supported(feat, None, ps[0], ps[2])
        y = ops.sa_mlp_max(xyz, feat, new_xyz, None, *ps)
        assert type(y.grad_fn).__name__.startswith("_SaLevelFused")      # not the composed form behind PznUnsupported
        y.backward(go)
        ops.clear_grad_sinks()
        return {"y": y.detach(), "dfeat": feat.grad, "dW1": ps[0].grad, "db1": ps[1].grad, "dW2": ps[2].grad, "db2": ps[3].grad}

    small = B < 64
    _repeat("sa_level", run, dev, REPS,
            bounds=_level_sum_abs(xyz_c, feat_c, w_c, go_c, S, sinks) if small else None)


def _chain_params(g, E, dk, Nout):
    shapes = [(dk, E), (dk,), (dk, E), (dk,), (E, E), (E,), (E, E), (E,)]
    flat = [torch.randn(*s, generator=g) / (math.sqrt(E) if len(s) == 2 else 4) for _ in range(4) for s in shapes]
    return flat + [torch.randn(Nout, 5 * E, generator=g) / math.sqrt(5 * E), 0.1 * torch.randn(Nout, generator=g)]


@pytest.mark.parametrize("strips", [False, True])
@pytest.mark.parametrize("sinks", [False, True])
@pytest.mark.parametrize("B", [64, 3])
def test_attention_chain_backward_repeatable(dev, B, sinks, strips):
    """The attention chain of one encoder (four blocks + out projection 1280 -> 1024 + max over the points) through
    ops._AttnChainOne in the case predict5 creates: map, maximum, the input gradient and all 34 parameter gradients, the
    sparse backward of the out projection included - every one EXACT.  B = 3: the chain takes L = 256, E = 256, dk = 64 only,
    so the odd case is a batch that fills no row range of the weight-gradient kernel.  0.10-0.15 s per case."""
    from puzzlenet_amd import ops
    L, E, dk, Nout = 256, 256, 64, 1024
    g = torch.Generator().manual_seed(31 + B)
    x0 = (0.5 * torch.randn(B, L, E, generator=g)).to(dev)
    flat0 = [t.to(dev) for t in _chain_params(g, E, dk, Nout)]
    go = torch.randn(B, Nout, generator=g).to(dev)
    names = [f"block{i}.{n}" for i in range(4) for n in _BLOCK] + ["out.weight", "out.bias"]

    def run():
        x = x0.detach().requires_grad_(True)
        flat = [p.clone().requires_grad_(True) for p in flat0]
        _with_sinks(flat, sinks)
        assert ops.attention_chain_one_supported(x, dk, flat[32])
        amap, fg = ops._AttnChainOne.apply(strips, x, *flat)
        fg.backward(go)
        ops.clear_grad_sinks()
        out = {"map": amap.detach(), "max": fg.detach(), "dx": x.grad}
        out.update({n: p.grad for n, p in zip(names, flat)})
        return out

    _repeat("attn_chain", run, dev, REPS)


def _block_sum_abs(x, ps, wr, wa, sinks):
    """sum|t_i| of the eight parameter gradients of one layerAttention block: the block in float64 with q, k, v and the out
    layer's pre-activation kept, each weight gradient |dY|^T |X|, each bias gradient the column sums of |dY| over the
    n = B L rows."""
    import torch.nn.functional as F
    wq, bq, wk, bk, wv, bv, wo, bo = (t.double() for t in ps)
    xd = x.double()
    M = x.shape[0] * x.shape[1]
    q, k, v = (F.linear(xd, w_, b_).requires_grad_(True) for w_, b_ in ((wq, bq), (wk, bk), (wv, bv)))
    attn = torch.softmax(q @ k.transpose(1, 2) / math.sqrt(q.shape[-1]), -1)
    r = xd - attn @ v
    z = F.linear(r, wo, bo).requires_grad_(True)
    out = xd + torch.relu(z)
    dq, dk_, dv, dz = torch.autograd.grad((out * wr.double()).sum() + (attn * wa.double()).sum(), (q, k, v, z))
    n, fill = M + int(sinks), SINK_FILL if sinks else 0.0
    res = {}
    for name, dy, xin in (("q", dq, xd), ("k", dk_, xd), ("v", dv, xd), ("o", dz, r.detach())):
        dy2, x2 = dy.reshape(M, -1).abs(), xin.reshape(M, -1).abs()
        res["w" + name] = (n, dy2.t() @ x2 + fill)
        res["b" + name] = (n, dy2.sum(0) + fill)
    return res


@pytest.mark.parametrize("sinks", [False, True])
@pytest.mark.parametrize("B,L,E,dk", [(64, 256, 256, 64), (17, 244, 256, 64)])
def test_attention_block_backward_repeatable(dev, B, L, E, dk, sinks):
    """One layerAttention block through ops.attention_block (pzn_attn_block_fwd/bwd_f32), the map receiving a gradient too:
    output, map and input gradient EXACT; the eight parameter gradients ATOMIC.  The odd shape (17 x 244 = 4148 rows: a ragged
    last 32-row tile, maps of 244 columns) is inside the fused block's domain (>= 4096 rows).  Seen: up to 4.5e-7 of the largest
    entry - except the key bias, whose gradient is mathematically zero (softmax is shift-invariant): its entries ARE rounding
    noise, 9 % apart between two runs at the small shape and far inside the derived bound (absolute, from sum|t_i|).
    0.10-0.15 s per case."""
    from puzzlenet_amd import ops
    g = torch.Generator().manual_seed(3 + B)
    x_c = 0.5 * torch.randn(B, L, E, generator=g)
    shapes = [(dk, E), (dk,), (dk, E), (dk,), (E, E), (E,), (E, E), (E,)]
    ps_c = [torch.randn(*s, generator=g) / (math.sqrt(E) if len(s) == 2 else 4) for s in shapes]
    wr_c, wa_c = torch.randn(B, L, E, generator=g), torch.randn(B, L, L, generator=g)
    x0, wr, wa = x_c.to(dev), wr_c.to(dev), wa_c.to(dev)
    ps0 = [t.to(dev) for t in ps_c]
    if not ops.attention_block_supported(x0, dk):
        pytest.skip("the fused block refuses this shape")

    def run():
        x = x0.detach().requires_grad_(True)
        ps = [p.clone().requires_grad_(True) for p in ps0]
        _with_sinks(ps, sinks)
        r, a = ops.attention_block(x, *ps)
        torch.autograd.backward((r, a), (wr, wa))
        ops.clear_grad_sinks()
        out = {"r": r.detach(), "attn": a.detach(), "dx": x.grad}
        out.update({n: p.grad for n, p in zip(_BLOCK, ps)})
        return out

    small = B < 64
    _repeat("attention_block", run, dev, REPS, bounds=_block_sum_abs(x_c, ps_c, wr_c, wa_c, sinks) if small else None)


@pytest.mark.parametrize("B,N", [(64, 2048), (5, 77)])
def test_stem_backward_repeatable(dev, B, N):
    """The stem forward + backward (ops.stem, training mode, the output under both names with a gradient through each):
    the output and all eight parameter gradients EXACT.  0.04-0.10 s per case."""
    from puzzlenet_amd import ops
    from tests.test_gpu_stem import _modules
    g = torch.Generator().manual_seed(7 * B + N)
    mods = [m.to(dev).train() for m in _modules(N, N, torch.float32)]
    xyz = (torch.rand(B, N, 3, generator=g) * 2 - 1).to(dev)
    go1, go2 = torch.randn(B, N, 64, generator=g).to(dev), torch.randn(B, N, 64, generator=g).to(dev)
    assert ops.stem_supported(xyz, *mods)
    ops.clear_grad_sinks()

    def run():
        for m in mods:
            m.weight.grad = m.bias.grad = None
        a, b = ops.stem(xyz, *mods, two=True)
        torch.autograd.backward((a, b), (go1, go2))
        out = {"y": a.detach()}
        for name, m in zip(("lin1", "bn1", "lin2", "bn2"), mods):
            out[name + ".weight"], out[name + ".bias"] = m.weight.grad, m.bias.grad
        return out

    _repeat("stem", run, dev, REPS)


def _mlp3_sum_abs(x, gl, W1, b1, W2, b2, W3, b3, go):
    """sum|t_i| of the gradients behind the per-cloud bias of the heads' chain, float64 on the CPU: dcb[b] = the column sums of
    the first layer's gated gradient over the cloud's points (order-fixed in the kernel), then dW1.global = dcb^T g and
    db1 = column sums of dcb over the n = B clouds, dg = dcb W1[:, :Cg] over the n = 64 channels."""
    import torch.nn.functional as F
    B, N, _ = x.shape
    Cg = gl.shape[-1]
    x, gl, W1, b1, W2, b2, W3, b3, go = (t.double() for t in (x, gl, W1, b1, W2, b2, W3, b3, go))
    z1 = (F.linear(torch.cat([gl.expand(-1, N, -1), x], -1), W1, b1)).requires_grad_(True)
    y = F.linear(torch.relu(F.linear(torch.relu(z1), W2, b2)), W3, b3)
    dcb = torch.autograd.grad((y * go).sum(), z1)[0].sum(1)                     # [B, 64]
    g2 = gl.reshape(B, Cg)
    return {"dW1.global": (B, dcb.abs().t() @ g2.abs()), "db1": (B, dcb.abs().sum(0)), "dg": (64, (dcb.abs() @ W1[:, :Cg].abs()).view(B, 1, Cg))}


@pytest.mark.parametrize("B,N,C2,C3,per_cloud", [(64, 2048, 64, 64, False), (64, 2048, 32, 2, True), (3, 96, 32, 2, True),
                                                  (3, 160, 64, 64, False)])
def test_point_mlp3_backward_repeatable(dev, B, N, C2, C3, per_cloud):
    """The boundary heads' chains forward + backward through ops.point_mlp3, both instantiations at the heads' full size
    (64 x 2048 rows) and at a small shape with a ragged last tile: output, input gradient and the chain's own parameter
    gradients EXACT; what hangs off the per-cloud bias (global half of W1, b1, the gradient of the global vector) ATOMIC by the code (seen: no
    difference at all - these few-row products run as two K splits, and a sum of two terms has one order).  0.04-0.09 s per
    case."""
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
    go_c = torch.randn(B, N, C3, generator=g)
    leaves = [x, W1, b1, W2, b2, W3, b3] + ([gl] if per_cloud else [])
    d0 = [t.to(dev) for t in leaves]
    go = go_c.to(dev)
    ops.clear_grad_sinks()

    def run():
        d = [t.detach().requires_grad_(True) for t in d0]
        y = ops.point_mlp3(d[0], d[1], d[2], d[3], d[4], d[5], d[6], g=d[7] if per_cloud else None)
        y.backward(go)
        out = {"y": y.detach(), "dx": d[0].grad, "db1": d[2].grad, "dW2": d[3].grad, "db2": d[4].grad, "dW3": d[5].grad, "db3": d[6].grad}
        if per_cloud:
            out["dW1.global"], out["dW1.local"], out["dg"] = d[1].grad[:, :64].contiguous(), d[1].grad[:, 64:].contiguous(), d[7].grad
        else:
            out["dW1"] = d[1].grad
        return out

    small = B < 64
    _repeat("point_mlp3_per_cloud" if per_cloud else "point_mlp3", run, dev, REPS,
            bounds=_mlp3_sum_abs(x, gl, W1, b1, W2, b2, W3, b3, go_c) if small and per_cloud else None)
