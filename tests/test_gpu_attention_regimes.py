"""The attention kernels against float64 where the softmax is NOT flat (tests/_attn_ref.py states the truth, the regimes
and the yardstick; tests/test_attn_ref_cpu.py holds the regimes to what they claim).

Every other attention test feeds logits that span ~2 with ~240 of 256 keys effective: there any row maximum is as good as
the true one, ln-sum-exp is at most 5.9, and P has one magnitude.  Here: one chained block in five regimes (softmax16's
maximum and its cross-lane exchange, lse and the backward's recomputation of P from it at |lse| of hundreds, the three-plane
split of P and dS over their whole range), the stand-alone path through all three row-softmax forms of csrc/gemm.hip with
ragged and full rows and with every logit below -150, and the four-block chain with peaks, including the arg-max the model
reads off the map.

Bound of a tensor T: max(1e-5 max|T64|, M err32(T)), err32 = max|T32 - T64| of the same statement in float32 on the CPU
(through the same ReLU gates).  The first term is the suite's tolerance; the second follows the conditioning of the input.

M = 8.  Measured on an MI355X with the assertion on M off (max|T_gpu - T64| / err32; the table per regime and tensor is in
docs/kernel_notes.md, "Attention: float64 truth where the softmax is not flat"); worst ratio per regime among the entries
where the err32 term is the binding one (elsewhere the floor holds, with the error at most 0.65 of it):
    chained block     soft -, peaked - (the floor holds everywhere), sharp 1.40 (dv), offset 2.07 (delta), mixed 2.80 (dv)
    ops.attention     peaked 0.45 (dq, L = 600; the floor elsewhere), negative 0.60 (dq, L = 33)
    attention_block   peaked 2.28 (dbk)
    chain, x 3        outputs 1.14 (fg), strips 1.49, gradients 2.74 (use = "max"), 1.76 (use = "out")
M is twice the worst of these (2.80), rounded up to a power of two.  A ratio above 16 is a finding, not a reason for a
larger M; none was measured (largest of all, floor-held: 14.8, a bias gradient of block 4 at 0.05 of its bound)."""
import pytest
import torch

from tests import _attn_ref as ar
from tests._attn_launch import fused_block

pytestmark = pytest.mark.gpu

M = 8.0
B = 2
EPS = 2.0 ** -24
RATIOS = {}          # (case, tensor) -> dict(err, err32, floor, ratio): what the last run measured


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _held(case, pairs, floors=None):
    """pairs: name -> (device tensor, T32, T64).  Records err / err32 of every tensor, then asserts all the bounds at once
    (so that a failure shows every figure)."""
    bad = []
    for name, (got, t32, t64) in pairs.items():
        t64 = t64.reshape(got.shape)
        err = float((got.detach().cpu().double() - t64).abs().max())
        e32 = float((t32.reshape(got.shape).double() - t64).abs().max())
        floor = (floors or {}).get(name, 1e-5 * float(t64.abs().max()))
        RATIOS[(case, name)] = dict(err=err, err32=e32, floor=floor, ratio=err / e32 if e32 else 0.0)
        if not err <= max(floor, M * e32):
            bad.append((name, err, floor, e32, err / e32 if e32 else float("inf")))
    assert not bad, (case, "(tensor, err, 1e-5 floor, err32, err / err32)", bad)


def _rows_sum_to_one(amap, n):
    """Every row of a softmax, summed in float64, within (n + 2) 2^-24 of 1: n summands, the reciprocal and the scaling, each
    one rounding in fp32."""
    a = amap.detach().cpu().double()
    assert bool(torch.isfinite(a).all()) and float(a.min()) >= 0.0
    assert float((a.sum(-1) - 1.0).abs().max()) <= (n + 2) * EPS


# ---------------------------------------------------------------- a, b: one chained block, every intermediate, every regime

@pytest.fixture(scope="module", params=ar.REGIMES)
def block(request, dev):
    args = ar.regime(request.param, B)
    got = fused_block(dev, *args)
    gate = (got["dz"] != 0).cpu().view(B, ar.L, ar.E)
    r32, r64 = ar.block_refs(args, gate=gate)            # through the device's gates (the same as float64's unless one flipped)
    return request.param, got, gate, r32, r64


def test_block_intermediates_vs_float64(block):
    name, got, gate, r32, r64 = block
    z64 = r64["z"]
    flipped = gate != (z64 > 0)
    zbound, _ = ar.bound("z", r32, r64, M)
    assert int((flipped & (z64.abs() > zbound)).sum()) == 0
    assert int(flipped.sum()) <= 4
    _held("block/" + name, {k: (got[k], r32[k], r64[k]) for k in ar.BLOCK_TENSORS})


def test_block_map_is_a_distribution_and_all_is_finite(block):
    name, got, _, _, _ = block
    for k in ar.BLOCK_TENSORS:
        assert bool(torch.isfinite(got[k]).all()), (name, k)
    _rows_sum_to_one(got["map"], ar.L)


# ---------------------------------------------------------------- c: the stand-alone path and its three softmax forms

@pytest.mark.parametrize("Lk", [33, 100, 256, 300, 512, 600])
@pytest.mark.parametrize("name", ar.STANDALONE_REGIMES)
def test_standalone_attention_vs_float64(dev, name, Lk):
    """ops.attention at L = 33, 100 (softmax_*_reg_kernel<4>, ragged), 256 (<4>, full), 300 (<8>, ragged), 512 (<8>, full),
    600 (the general row kernels), forward and backward with a gradient into both results."""
    from puzzlenet_amd import ops
    prob = ar.standalone_regime(name, B, Lk, 16, 40, seed=Lk)
    r32, r64 = ar.standalone_eval(prob, torch.float32), ar.standalone_eval(prob, torch.float64)
    if name == "negative":
        assert float(r64["s"].max()) < -150
    d = [t.to(dev).requires_grad_(True) for t in prob[:3]]
    out, attn = ops.attention(*d)
    ((out * prob[3].to(dev)).sum() + (attn * prob[4].to(dev)).sum()).backward()
    got = dict(out=out, attn=attn, dq=d[0].grad, dk=d[1].grad, dv=d[2].grad)
    for k, val in got.items():
        assert bool(torch.isfinite(val).all()), k
    _rows_sum_to_one(attn, Lk)
    _held(f"standalone/{name}/{Lk}", {k: (got[k], r32[k], r64[k]) for k in got})


def test_attention_block_peaked_vs_float64(dev):
    """ops.attention_block (the block composed from the same kernels; its domain starts at B L = 4096, so B = 16) in `peaked`:
    r, the map, dx and the eight parameter gradients through the device's gates (yo = relu(.) is what its backward gates by)."""
    from puzzlenet_amd import ops
    Bb = 16
    args = ar.regime("peaked", Bb)
    x = args[0].to(dev).requires_grad_(True)
    ps = [t.to(dev).requires_grad_(True) for t in args[1:9]]
    assert ops.attention_block_supported(x, ar.DK)
    r, amap = ops.attention_block(x, *ps)
    yo = r.grad_fn.saved_tensors[-1]
    assert yo.shape == (Bb * ar.L, ar.E) and float(yo.min()) >= 0.0
    gate = (yo > 0).cpu().view(Bb, ar.L, ar.E)
    (r * args[9].to(dev)).sum().backward()
    r32, r64 = ar.block_refs(args, gate=gate)
    flipped = gate != (r64["z"] > 0)
    zbound, _ = ar.bound("z", r32, r64, M)
    assert int((flipped & (r64["z"].abs() > zbound)).sum()) == 0 and int(flipped.sum()) <= 4
    _rows_sum_to_one(amap, ar.L)
    pairs = dict(r=(r, r32["r"], r64["r"]), map=(amap, r32["map"], r64["map"]), dx=(x.grad, r32["dx"], r64["dx"]))
    for k, p in zip(ar.BLOCK_PARAM_GRADS, ps):
        pairs[k] = (p.grad, r32[k], r64[k])
    # dbk is mathematically zero (the softmax does not see a shift of the keys): it is the column sum of dk, and is held to
    # the floor of one dk entry
    _held("attention_block/peaked", pairs, floors=dict(dbk=1e-5 * float(r64["dk"].abs().max())))


# ---------------------------------------------------------------- d: the chain, once, with peaks

@pytest.fixture(scope="module", params=["max", "out"])
def chain_case(request):
    use = request.param
    prob = ar.chain_regime(B, use)
    return use, prob, ar.chain_eval(prob, use, torch.float32), ar.chain_eval(prob, use, torch.float64)


def _chain_run(dev, prob, use, **kw):
    from puzzlenet_amd import ops
    x0, blocks0, w0, b0, wg = prob
    leaf = lambda a: a.to(dev).requires_grad_(True)
    x, blocks, w, b = leaf(x0), [[leaf(p) for p in blk] for blk in blocks0], leaf(w0), leaf(b0)
    assert ops.attention_chain_fused_supported(x, ar.DK, w)
    y, amap, fg = ops.attention_chain_fused([x], [blocks], [w], [b], **kw)[0]
    ((fg if use == "max" else y) * wg.to(dev)).sum().backward()
    return y, amap, fg, [x.grad] + [p.grad for blk in blocks for p in blk] + [w.grad, b.grad]


def _chain_grads_held(case, grads, g32, g64):
    """All 35 gradients to max(the bound of test_attention_chain_fused_vs_float64, M err32): 2e-4 of max(max|g|, 0.25), and
    1e-4 of max|g| where the gradient is not rounding noise (norm > 1e-3)."""
    assert len(grads) == len(g64) == 35
    pairs, floors = {}, {}
    for i, (a_, b32, b64) in enumerate(zip(grads, g32, g64)):
        mx = float(b64.abs().max())
        floors[f"g{i}"] = min(2e-4 * max(mx, 0.25), 1e-4 * mx if float(b64.norm()) > 1e-3 else float("inf"))
        pairs[f"g{i}"] = (a_, b32, b64)
    _held(case, pairs, floors)


def test_chain_peaked_vs_float64(dev, chain_case):
    """ops.attention_chain_fused with every block's wq, wk x 3 (14 / 5 / 1.8 / 1.04 effective keys block by block)."""
    use, prob, (o32, g32, _), (o64, g64, _) = chain_case
    y, amap, fg, grads = _chain_run(dev, prob, use)
    assert amap.shape == (B, ar.L, ar.L)
    _held(f"chain/{use}/out", dict(y=(y, o32["y"], o64["y"]), map=(amap, o32["map"], o64["map"]), fg=(fg, o32["fg"], o64["fg"])))
    _rows_sum_to_one(amap, ar.L + 4)               # (the mean of four maps: each within 258 roundings, four more to add them up)
    _chain_grads_held(f"chain/{use}/grads", grads, g32, g64)


def test_chain_peaked_map_strips_and_argmax(dev, chain_case):
    """map_strips=True (use = "max" without `out`: the one-call form training_step takes; use = "out": the composed one): the
    strips' column means against the float64 mean map's, and colmean_argmax of the device's map - full and in strips - is
    the float64 arg-max in BOTH clouds (test_attn_ref_cpu.py: the top-2 gap is > 100 err32, no cloud is a toss-up)."""
    from puzzlenet_amd import ops
    use, prob, (o32, g32, _), (o64, g64, _) = chain_case
    y, strips, fg, grads = _chain_run(dev, prob, use, need_out=(use == "out"), map_strips=True)
    assert strips.shape == (B, ar.L // 16, ar.L) and (y is None) == (use == "max")
    pairs = dict(strips=(strips, o32["strips"], o64["strips"]), fg=(fg, o32["fg"], o64["fg"]))
    if y is not None:
        pairs["y"] = (y, o32["y"], o64["y"])
    mean_s, arg_s = ops.colmean_argmax(strips)
    pairs["colmean"] = (mean_s, o32["colmean"], o64["colmean"])
    _held(f"chain/{use}/strips", pairs)
    want = o64["colmean"].argmax(-1)
    assert torch.equal(arg_s.cpu(), want)
    full = _chain_run(dev, prob, use)[1]
    assert torch.equal(ops.colmean_argmax(full)[1].cpu(), want)
    _chain_grads_held(f"chain/{use}/strips-grads", grads, g32, g64)
