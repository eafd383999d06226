"""GPU: ops.chamfer / ops._Chamfer (csrc/chamfer.hip: chamfer_pack_kernel, chamfer_rowmin_kernel, chamfer_bwd_kernel) against
the float64 restatement tests/_chamfer_ref.py, which tests/test_chamfer_ref_cpu.py tests on its own (the C oracle passes (a),
(b) and (d) below on every input kind).

What is compared with what, and where the bounds come from (nothing below is tuned to the kernel):

(a) minima.  Truth is the float64 DIFFERENCE form D of the float32 inputs.  Bd = gamma_5 (|a|^2 + |b|^2 + 2 sum |a_c b_c|)
    bounds |P32 - D| (_chamfer_ref.distance_bound: 5 roundings on the longest path of the expansion form), so a returned
    minimum lies in [min (D - Bd), min (D + Bd)] of its row or column.
(b) arg-mins.  In range, and for a returned index c of a row whose float64 arg-min is c*:
    D(c) - Bd(c) <= P32(c) <= P32(c*) <= D(c*) + Bd(c*), hence D(c) - D(c*) <= Bd(c) + Bd(c*).
(c) the returned minimum IS the kernel's formula at the returned pair, bit for bit.  Python's math.fma (3.13) is not
    assumed: _chamfer_ref.fma32 is an exact single-rounding float32 fma in NumPy (tested against rational arithmetic on the
    CPU), so the bit-equal form is always the one asserted.  Up to 2^20 pairs the whole float32 matrix is formed that way
    and the four outputs must equal its minima and FIRST arg-mins bit for bit.
(d) ties.  Bit copies of a point have bit-equal P whatever the rounding: the returned index is the lowest of the copies
    for copies inside one wavefront's quarter of a tile, in different quarters, in different tiles, for the loader's
    padding (copies of row 0) - in both directions, and it equals the oracle's index.
(e) chamfer(b, a) is chamfer(a, b) with the roles swapped, bit for bit; a permuted view gives the bits of its contiguous copy.
(f) backward.  At the device's own arg-mins every entry is within gamma_(K+2) sum |term| of the float64 gradient
    (_chamfer_ref.grad: a term rounds twice, K terms are added onto zero in any order), under three weightings: both
    outputs, the first only, the second only (a null pointer each).  No output weighted: no gradient, no launch.
(g) run to run.  The four forward outputs are bit-identical.  Two backward calls differ per entry by at most twice (f)'s
    bound and are bit-identical where K <= 2 (one addition, or two commuting ones, onto zero).
(h) the entry point's limits: 65535 problems in one call, more through ops.chamfer in chunks; what ops.py rejects.

NaN and inf inputs are out of scope.  Run with -s for the figures of DESIGN section 4.
"""
import functools

import numpy as np
import pytest
import torch

from tests import _chamfer_ref as ref

pytestmark = pytest.mark.gpu

SCALES = {"scale1e-3": 1e-3, "scale100": 100.0}
CASES = ([("uniform", s) for s in ref.SHAPES] + [("ties", s) for s in ref.TIE_SHAPES]
         + [("offset10", s) for s in ((2, 65, 513), (2, 300, 77), (1, 257, 1025))]
         + [("scale1e-3", s) for s in ((2, 65, 513), (2, 300, 77))] + [("scale100", s) for s in ((2, 65, 513), (1, 257, 1025))]
         + [("funnel", (2, 65, 513)), ("funnel", ref.FUNNEL_SHAPE)])
# the backward: every grid edge of chamfer_bwd_kernel (256 threads, sized by max(n, m)) in uniform data, ties, and the
# many-to-one scatters: (1, 2049, 1) lands 2050 atomics on b's only point, the funnel 2050 on one a-point
BWD_CASES = ([("uniform", s) for s in ((1, 1, 1), (3, 1, 7), (2, 3, 513), (2, 65, 513), (1, 257, 1025), (2, 300, 77), (1, 1, 2049),
                                       (1, 2049, 1), (2, 1536, 1537))]
             + [("ties", (2, 65, 513)), ("offset10", (2, 300, 77)), ("funnel", ref.FUNNEL_SHAPE)])
WEIGHTS = ["both", "first", "second"]
FULL_MATRIX_PAIRS = 1 << 20


def _id(case):
    return case[0] + "-" + "x".join(map(str, case[1]))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _inputs(case):
    kind, shape = case
    seed = ref.seed_of(kind, shape)
    if kind == "uniform":
        return ref.uniform(seed, *shape)
    if kind == "ties":
        return ref.with_ties(seed, *shape)
    if kind == "offset10":
        return ref.offset(seed, *shape)
    if kind == "funnel":
        return ref.funnel(seed, *shape)
    return ref.scaled(seed, *shape, SCALES[kind])


@functools.lru_cache(maxsize=2)
def _truth(case):
    c = _inputs(case)
    return ref.truth(c.a, c.b), ref.distance_bound(c.a, c.b)


@pytest.fixture(scope="module")
def forward(dev):
    """case -> two forward calls' (min_over_a, min_over_b, arg_over_a, arg_over_b) as NumPy; each case runs once."""
    from puzzlenet_amd import ops
    done = {}

    def run(case):
        if case not in done:
            c = _inputs(case)
            a, b = torch.from_numpy(c.a).to(dev), torch.from_numpy(c.b).to(dev)
            done[case] = [tuple(t.cpu().numpy() for t in ops._Chamfer.apply(a, b)) for _ in range(2)]
        return done[case]
    return run


def _weights(case, which):
    kind, (B, n, m) = case
    rng = np.random.default_rng(ref.seed_of(kind, case[1]) + 1)
    g1, g2 = rng.standard_normal((B, m)).astype(np.float32), rng.standard_normal((B, n)).astype(np.float32)
    if kind == "funnel":      # one sign: the terms on the funnel's entry do not cancel
        g1, g2 = np.abs(g1) + np.float32(0.5), np.abs(g2) + np.float32(0.5)
    return (g1 if which != "second" else None), (g2 if which != "first" else None)


@pytest.fixture(scope="module")
def backward(dev):
    """(case, weighting) -> (arg_over_a, arg_over_b, [grad_a, grad_b] of two backward calls through one forward)."""
    from puzzlenet_amd import ops
    done = {}

    def run(case, which):
        if (case, which) not in done:
            c = _inputs(case)
            a = torch.from_numpy(c.a).to(dev).requires_grad_(True)
            b = torch.from_numpy(c.b).to(dev).requires_grad_(True)
            moa, mob, aoa, aob = ops._Chamfer.apply(a, b)
            g1, g2 = _weights(case, which)
            loss = 0.0
            if g1 is not None:
                loss = loss + (moa * torch.from_numpy(g1).to(dev)).sum()
            if g2 is not None:
                loss = loss + (mob * torch.from_numpy(g2).to(dev)).sum()
            grads = [tuple(t.cpu().numpy() for t in torch.autograd.grad(loss, (a, b), retain_graph=True)) for _ in range(2)]
            done[case, which] = (aoa.cpu().numpy(), aob.cpu().numpy(), grads)
        return done[case, which]
    return run


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_minima_lie_in_the_float64_interval(forward, case):
    """(a)"""
    moa, mob, aoa, aob = forward(case)[0]
    assert moa.dtype == np.float32 and mob.dtype == np.float32
    D, Bd = _truth(case)
    worst = ref.check_minima(D, Bd, moa, mob)
    print(f"(a) {_id(case)}: worst (minimum - float64 minimum) / bound {worst:+.3f}")


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_argmins_are_float64_nearest_within_the_bound(forward, case):
    """(b)"""
    moa, mob, aoa, aob = forward(case)[0]
    assert aoa.dtype == np.int32 and aob.dtype == np.int32
    D, Bd = _truth(case)
    worst, flips = ref.check_argmins(D, Bd, aoa, aob)
    print(f"(b) {_id(case)}: worst (D(c) - D(c*)) / (Bd(c) + Bd(c*)) {worst:.3f}; {flips} of {aoa.size + aob.size} indices "
          "differ from the float64 arg-min")


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_minimum_is_the_formula_at_the_returned_index(forward, case):
    """(c), bit for bit (exact float32 fma in NumPy; math.fma is not needed)."""
    c = _inputs(case)
    moa, mob, aoa, aob = forward(case)[0]
    bi = np.arange(c.a.shape[0])[:, None]
    want_a = ref.kernel_p32(c.a[bi, aoa], c.b)      # [B,m]: a's partner of every b-point
    want_b = ref.kernel_p32(c.a, c.b[bi, aob])      # [B,n]
    assert np.array_equal(moa.view(np.uint32), want_a.view(np.uint32))
    assert np.array_equal(mob.view(np.uint32), want_b.view(np.uint32))
    if c.a.shape[0] * c.a.shape[1] * c.b.shape[1] <= FULL_MATRIX_PAIRS:
        P = ref.kernel_matrix(c.a, c.b)
        assert np.array_equal(moa, P.min(axis=1)) and np.array_equal(mob, P.min(axis=2))
        assert np.array_equal(aoa, P.argmin(axis=1)) and np.array_equal(aob, P.argmin(axis=2))      # np.argmin: the first


@pytest.mark.parametrize("case", [c for c in CASES if c[0] in ("ties", "funnel")], ids=_id)
def test_ties_go_to_the_lowest_index(forward, case):
    """(d)"""
    from oracle import point_ops as orc
    c = _inputs(case)
    moa, mob, aoa, aob = forward(case)[0]
    assert c.planted
    ref.planted_are_float64_ties(c, *_truth(case))
    ref.check_first_copy(c.a, c.b, aoa, aob)
    ref.check_planted(c, aoa, aob)
    _, o_aoa, _, o_aob = orc.chamfer(c.a, c.b)
    for direction, bb, row, want in c.planted:
        assert int((o_aoa if direction == "over_a" else o_aob)[bb, row]) == want
    print(f"(d) {_id(case)}: {len(c.planted)} planted queries return the lowest copy, as the oracle does")


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_forward_is_bit_identical_run_to_run(forward, case):
    """(g), forward: all four outputs."""
    first, second = forward(case)
    for x, y in zip(first, second):
        assert np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y)


@pytest.mark.parametrize("case", [("ties", (2, 300, 77)), ("ties", (2, 65, 513)), ("uniform", (1, 2049, 1))], ids=_id)
def test_swapped_roles_give_swapped_bits(dev, forward, case):
    """(e) n != m: both passes see bit-identical P, and the arg-mins follow."""
    from puzzlenet_amd import ops
    c = _inputs(case)
    moa, mob, aoa, aob = forward(case)[0]
    s_moa, s_mob, s_aoa, s_aob = (t.cpu().numpy() for t in ops._Chamfer.apply(torch.from_numpy(c.b).to(dev),
                                                                               torch.from_numpy(c.a).to(dev)))
    assert np.array_equal(s_moa.view(np.uint32), mob.view(np.uint32)) and np.array_equal(s_mob.view(np.uint32), moa.view(np.uint32))
    assert np.array_equal(s_aoa, aob) and np.array_equal(s_aob, aoa)


def test_permuted_view_gives_the_bits_of_its_contiguous_copy(dev):
    """(e) [B,3,n].permute(0, 2, 1), as the model passes its clouds: forward bit for bit; the backward bit for bit on every
    entry with K <= 2 terms and within twice (f)'s bound elsewhere (the atomics' order is free, see (g)), and it reaches the
    [B,3,n] tensor through the view."""
    from puzzlenet_amd import ops
    case = ("uniform", (2, 65, 513))
    c = _inputs(case)
    g1, g2 = (torch.from_numpy(g).to(dev) for g in _weights(case, "both"))
    out = []
    for contiguous in (False, True):
        xa = torch.from_numpy(c.a).to(dev).permute(0, 2, 1).contiguous().requires_grad_(True)      # [B,3,n]
        xb = torch.from_numpy(c.b).to(dev).permute(0, 2, 1).contiguous().requires_grad_(True)
        a, b = xa.permute(0, 2, 1), xb.permute(0, 2, 1)
        assert not a.is_contiguous()
        if contiguous:
            a, b = a.contiguous(), b.contiguous()
        res = ops._Chamfer.apply(a, b)
        ((res[0] * g1).sum() + (res[1] * g2).sum()).backward()
        out.append([t.detach().cpu().numpy() for t in res] + [xa.grad.permute(0, 2, 1).cpu().numpy(), xb.grad.permute(0, 2, 1).cpu().numpy()])
    for x, y in zip(out[0][:4], out[1][:4]):
        assert np.array_equal(x, y)
    want = ref.grad(c.a, c.b, out[0][2], out[0][3], g1.cpu().numpy(), g2.cpu().numpy())
    for got in out:
        ref.check_grad(want, got[4], got[5])
    for x, y, absum, k in ((out[0][4], out[1][4], want[2], want[4]), (out[0][5], out[1][5], want[3], want[5])):
        assert (np.abs(x.astype(np.float64) - y) <= 2 * ref.entry_bound(absum, k)).all()
        assert np.array_equal(x[k <= 2], y[k <= 2])


@pytest.mark.parametrize("which", WEIGHTS)
@pytest.mark.parametrize("case", BWD_CASES, ids=_id)
def test_backward_within_the_rounding_of_its_sums(backward, case, which):
    """(f)"""
    c = _inputs(case)
    aoa, aob, grads = backward(case, which)
    want = ref.grad(c.a, c.b, aoa, aob, *_weights(case, which))
    worst = max(ref.check_grad(want, *g) for g in grads)
    kmax = int(max(want[4].max(), want[5].max()))
    print(f"(f) {_id(case)} {which}: worst |entry32 - entry| / (gamma_(K+2) sum |term|) {worst:.3f}; largest K {kmax}")
    if case[0] == "funnel":
        # the entry all of b lands on: no cancellation (sum |term| = |sum|), so the bound is relative to the entry itself -
        # float32 resolution of the float64 sum, gamma_(K+2) at most
        n = c.a.shape[1]
        ga, ga_abs, ka = want[0][:, n // 2], want[2][:, n // 2], want[4][:, n // 2]
        assert (ka >= (c.b.shape[1] if which != "second" else 1)).all()
        assert np.allclose(ga_abs, np.abs(ga), rtol=1e-12, atol=0)
        rel = np.abs(grads[0][0][:, n // 2].astype(np.float64) - ga) / np.abs(ga)
        assert (rel <= ref.gamma(ka + ref.TERM_ROUNDINGS)[:, None]).all()
        print(f"    funnel entry, K = {int(ka.max())}: relative error {rel.max():.2e} = {rel.max() / ref.U32:.1f} u "
              f"(bound {float(ref.gamma(ka.max() + 2)) / ref.U32:.0f} u)")


@pytest.mark.parametrize("which", WEIGHTS)
@pytest.mark.parametrize("case", BWD_CASES, ids=_id)
def test_backward_run_to_run(backward, case, which):
    """(g), backward."""
    c = _inputs(case)
    aoa, aob, (first, second) = backward(case, which)
    want = ref.grad(c.a, c.b, aoa, aob, *_weights(case, which))
    differ = total = 0
    for x, y, absum, k in ((first[0], second[0], want[2], want[4]), (first[1], second[1], want[3], want[5])):
        assert (np.abs(x.astype(np.float64) - y) <= 2 * ref.entry_bound(absum, k)).all()
        assert np.array_equal(x[k <= 2], y[k <= 2])
        differ += int((x != y).sum())
        total += int((k > 2).sum()) * 3
    print(f"(g) {_id(case)} {which}: {differ} of {total} entries with K > 2 differ between two backward calls")


def test_unused_outputs_launch_nothing(dev, monkeypatch):
    """(f) neither minimum reaches the loss: backward returns no gradient and calls no entry point."""
    from puzzlenet_amd import ops

    class Drop(torch.autograd.Function):      # passes its input on and sends no gradient back
        @staticmethod
        def forward(ctx, x):
            return x.clone()

        @staticmethod
        def backward(ctx, g):
            return None

    c = _inputs(("uniform", (2, 65, 513)))
    a = torch.from_numpy(c.a).to(dev).requires_grad_(True)
    b = torch.from_numpy(c.b).to(dev).requires_grad_(True)
    moa, mob, aoa, aob = ops._Chamfer.apply(a, b)
    assert not aoa.requires_grad and not aob.requires_grad
    calls = []
    monkeypatch.setattr(ops, "_call", lambda *x, **k: calls.append(x[0]))
    (Drop.apply(moa).sum() + Drop.apply(mob).sum()).backward(retain_graph=True)
    assert calls == [] and a.grad is None and b.grad is None
    (Drop.apply(moa).sum() + mob.sum()).backward()      # one of them does: one launch
    assert calls == ["pzn_chamfer_bwd_f32"]


def test_batch_limit_and_chunks(dev, monkeypatch):
    """(h) 65535 problems are one call (the grid's y edge); one more is a PznError of _Chamfer that launches nothing, and
    ops.chamfer answers it in two calls, each chunk with the bits of a call of its own, gradients included."""
    from puzzlenet_amd import _lib, ops
    assert ops.CHAMFER_MAX_BATCH == 65535
    c = ref.uniform(77, 65535, 1, 1)
    moa, mob, aoa, aob = (t.cpu().numpy() for t in ops._Chamfer.apply(torch.from_numpy(c.a).to(dev), torch.from_numpy(c.b).to(dev)))
    D, Bd = ref.truth(c.a, c.b), ref.distance_bound(c.a, c.b)
    ref.check_minima(D, Bd, moa, mob)
    ref.check_argmins(D, Bd, aoa, aob)
    assert np.array_equal(moa, ref.kernel_p32(c.a, c.b)) and np.array_equal(moa, mob)

    c = ref.uniform(78, 65536, 2, 3)
    a, b = torch.from_numpy(c.a).to(dev).requires_grad_(True), torch.from_numpy(c.b).to(dev).requires_grad_(True)
    calls = []
    real = ops._call
    monkeypatch.setattr(ops, "_call", lambda *x, **k: calls.append(x[0]))
    with pytest.raises(_lib.PznError, match="65535"):
        ops._Chamfer.apply(a, b)
    assert calls == []
    monkeypatch.setattr(ops, "_call", lambda *x, **k: (calls.append(x[0]), real(*x, **k))[1])
    d1, d2 = ops.chamfer(a, b)
    assert calls == ["pzn_chamfer_fwd_f32"] * 2 and d1.shape == (65536, 3) and d2.shape == (65536, 2)
    parts = [ops._Chamfer.apply(a[s:e], b[s:e]) for s, e in ((0, 65535), (65535, 65536))]
    assert torch.equal(d1, torch.cat([p[0] for p in parts])) and torch.equal(d2, torch.cat([p[1] for p in parts]))
    D, Bd = ref.truth(c.a, c.b), ref.distance_bound(c.a, c.b)
    ref.check_minima(D, Bd, d1.detach().cpu().numpy(), d2.detach().cpu().numpy())
    rng = np.random.default_rng(79)
    g1, g2 = rng.standard_normal((65536, 3)).astype(np.float32), rng.standard_normal((65536, 2)).astype(np.float32)
    ((d1 * torch.from_numpy(g1).to(dev)).sum() + (d2 * torch.from_numpy(g2).to(dev)).sum()).backward()
    aoa = torch.cat([p[2] for p in parts]).cpu().numpy()
    aob = torch.cat([p[3] for p in parts]).cpu().numpy()
    ref.check_grad(ref.grad(c.a, c.b, aoa, aob, g1, g2), a.grad.cpu().numpy(), b.grad.cpu().numpy())


def test_what_the_wrapper_rejects(dev, monkeypatch):
    """(h) as ops.py says today.  Checked in Python, before any entry point is called: a tensor that is not on the GPU, shapes
    other than a[B,n,3], b[B,m,3] with one B.  Checked by the entry point itself before it launches (PZN_CHECK_ARG): an empty
    cloud or an empty batch - a PznError, NOT empty minima (icp_refine answers an empty batch; chamfer does not).  And one
    that is not rejected: a float64 input is rounded to float32 without a word (_f32) and gives the bits of its float32 copy."""
    from puzzlenet_amd import _lib, ops
    pts = torch.rand(2, 8, 3, device=dev)
    calls = []
    real = ops._call
    monkeypatch.setattr(ops, "_call", lambda *x, **k: calls.append(x[0]))
    for bad in (lambda: ops.chamfer(pts.cpu(), pts),
                lambda: ops.chamfer(pts, pts.cpu()),
                lambda: ops.chamfer(pts.cpu().numpy(), pts),
                lambda: ops.chamfer(pts, torch.rand(2, 8, 2, device=dev)),
                lambda: ops.chamfer(torch.rand(2, 8, 4, device=dev), pts),
                lambda: ops.chamfer(pts, torch.rand(8, 3, device=dev)),
                lambda: ops.chamfer(pts, torch.rand(3, 8, 3, device=dev))):
        with pytest.raises(_lib.PznError) as info:
            bad()
        assert not isinstance(info.value, _lib.PznUnsupported)
    assert calls == []
    monkeypatch.setattr(ops, "_call", real)
    for bad in (lambda: ops.chamfer(pts[:, :0], pts), lambda: ops.chamfer(pts, pts[:, :0]), lambda: ops.chamfer(pts[:0], pts[:0])):
        with pytest.raises(_lib.PznError):
            bad()
    want = ops._Chamfer.apply(pts, pts.flip(1))
    got = ops._Chamfer.apply(pts.double(), pts.flip(1).double())
    for x, y in zip(got, want):
        assert x.dtype == y.dtype and torch.equal(x, y)
