"""The attention regimes are what they claim, on the reference alone (no GPU): each regime's defining property on the
float64 logits, the float32 statement finite and gating exactly as float64 does wherever fp32 can gate at all (so that the
GPU test's flip cap is the device's alone), every yardstick that can be non-zero non-zero, and for the peaked chain an arg-max that float32 noise cannot
move.  Thresholds: the figures measured at B = 2, seed 3, with slack (median spread / effective keys / |lse| per regime:
soft 1.5 / 238 / 5.9, peaked 12.4 / 14.8 / 11.3, sharp 87.6 / 1.1 / 73, offset 35.4 / 1.4 / 223, mixed 77.8 / 1.0 / 559)."""
import pytest
import torch

from tests import _attn_ref as ar

B = 2


@pytest.fixture(scope="module", params=ar.REGIMES)
def block(request):
    args = ar.regime(request.param, B)
    r32, r64 = ar.block_refs(args)           # (both through float64's gates; z itself does not depend on them)
    return request.param, args, r32, r64


def test_regime_draws_are_the_block_tests_draws():
    """`soft` is test_attention_fused_block_intermediates' input, bit for bit; the others differ from it only where stated."""
    g = torch.Generator().manual_seed(3)
    x = 0.5 * torch.randn(B * ar.L, ar.E, generator=g)
    wq = torch.randn(ar.DK, ar.E, generator=g) / 16
    soft, sharp, mixed, offset = (ar.regime(n, B) for n in ("soft", "sharp", "mixed", "offset"))
    assert torch.equal(soft[0].reshape(-1, ar.E), x) and torch.equal(soft[1], wq)
    assert torch.equal(sharp[1], 8 * wq) and torch.equal(sharp[0], soft[0]) and torch.equal(sharp[9], soft[9])
    assert torch.equal(mixed[0].reshape(-1, ar.E)[6], 4.0 * x[6]) and torch.equal(mixed[0].reshape(-1, ar.E)[259], 12.0 * x[259])
    assert torch.equal((offset[2] - soft[2]).abs().round(), torch.full((ar.DK,), 12.0)) and torch.equal(offset[1], wq)


def test_float32_statement_is_finite_and_gates_as_float64(block):
    """0 flips among the 131 072 pre-activations that fp32 can gate at all.  `offset` holds one |z64| of 8.2e-9, below ONE
    rounding of its own sum, 2^-24 (|bo| + sum |t| |wo|) ~ 3e-7: no fp32 evaluation decides that gate, and which way it falls
    depends on the summation order of the CPU's GEMM (0 flips with one BLAS code path, 1 with another, same inputs).  Such
    elements are counted on float64 alone - one in `offset`, none elsewhere - and the flips may not exceed that count."""
    name, args, r32, r64 = block
    for key, val in r32.items():
        assert bool(torch.isfinite(val).all()), (name, key)
    z64 = r64["z"]
    assert z64.numel() == 131072
    one_rounding = 2.0 ** -24 * (r64["t"].abs() @ args[7].double().abs().T + args[8].double().abs())
    undecidable = z64.abs() <= one_rounding
    assert int(undecidable.sum()) == (1 if name == "offset" else 0), name
    flipped = (r32["z"] > 0) != (z64 > 0)
    assert int((flipped & ~undecidable).sum()) == 0, name
    assert int(flipped.sum()) <= int(undecidable.sum()), name


def test_regime_property(block):
    name, _, _, r64 = block
    st = ar.logit_stats(r64["s"])
    med = {k: float(v.median()) for k, v in st.items()}
    if name == "soft":
        assert float(st["spread"].max()) < 4
    elif name == "peaked":
        assert 4 < med["eff"] < 64
    elif name == "sharp":
        assert med["spread"] > 60 and med["pmax"] > 0.9
    elif name == "offset":
        assert float(st["lse"].abs().median()) > 100 and float(st["spread"].max()) < 60
    else:
        assert ar.tile_max_range(r64["s"]) > 88 * 8
        # (and already among four adjacent queries, scaled 0.05 / 1 / 4 / 12)
        m = (8 * r64["s"]).max(-1)[0].reshape(-1, 4)
        assert float((m.max(-1)[0] - m.min(-1)[0]).median()) > 88


def test_yardsticks_are_nonzero(block):
    """err32 > 0 for every compared tensor but dz (a gate times an input: exact in both types)."""
    name, _, r32, r64 = block
    for key in ar.BLOCK_TENSORS + ar.BLOCK_PARAM_GRADS:
        e = ar.yardstick(key, r32, r64)
        assert (e == 0.0) if key == "dz" else (e > 0.0), (name, key, e)


def test_bound_is_the_suites_own_where_the_softmax_is_flat():
    """In `soft` fp32 itself is within 1e-5 of float64 in every tensor: with the margin at 1 the floor binds, the regime test
    there is the existing test's statement."""
    r32, r64 = ar.block_refs(ar.regime("soft", B))
    for key in ar.BLOCK_TENSORS:
        bnd, binding = ar.bound(key, r32, r64, 1.0)
        assert not binding and bnd == 1e-5 * float(r64[key].abs().max()), key


@pytest.mark.parametrize("Lk", [33, 100, 256, 300, 512, 600])
@pytest.mark.parametrize("name", ar.STANDALONE_REGIMES)
def test_standalone_regimes(name, Lk):
    prob = ar.standalone_regime(name, B, Lk, 16, 40, seed=Lk)
    r32, r64 = ar.standalone_eval(prob, torch.float32), ar.standalone_eval(prob, torch.float64)
    for key, val in r32.items():
        assert bool(torch.isfinite(val).all()), key
    for key in ("out", "attn", "dq", "dk", "dv"):
        assert ar.yardstick(key, r32, r64) > 0.0, key
    s = r64["s"]
    if name == "peaked":
        assert 2.5 < float(s.std()) < 3.5
    else:
        assert float(s.max()) < -150
        assert float((prob[1] * torch.full((16,), 0.25)).sum(-1).max()) < 0        # k's component along the shift: strictly negative


@pytest.fixture(scope="module")
def chain():
    prob = ar.chain_regime(B, "max")
    return ar.chain_eval(prob, "max", torch.float32), ar.chain_eval(prob, "max", torch.float64)


def test_chain_regime_sharpens_block_by_block(chain):
    (o32, g32, _), (_, _, maps) = chain
    eff = [float((1.0 / (m * m).sum(-1)).median()) for m in maps]
    assert eff[0] > 8 and eff[3] < 2 and eff[0] > eff[1] > eff[2] > eff[3], eff
    for t in list(o32.values()) + g32:
        assert bool(torch.isfinite(t).all())


def test_chain_yardsticks_are_nonzero(chain):
    (o32, g32, _), (o64, g64, _) = chain
    for key in o64:
        assert ar.yardstick(key, o32, o64) > 0.0, key
    assert len(g64) == 35
    for i, (a, b) in enumerate(zip(g32, g64)):
        assert float((a.double() - b).abs().max()) > 0.0, i


def test_chain_argmax_is_out_of_float32_noise(chain):
    """The float64 top-2 gap of the mean map's column means exceeds 100 x their err32 in both clouds: the GPU test may demand
    the float64 arg-max of every cloud, none skipped."""
    (o32, _, _), (o64, _, _) = chain
    err32 = ar.yardstick("colmean", o32, o64)
    top2 = o64["colmean"].topk(2, dim=-1)[0]
    assert err32 > 0 and float((top2[:, 0] - top2[:, 1]).min()) > 100 * err32
    assert torch.equal(o32["colmean"].argmax(-1), o64["colmean"].argmax(-1))
