"""GPU: refine= of puzzlenet_amd.assembly - every pair pose refined on its picked boundary rows (refine_pairs, one launch of
ops.icp_refine) - in match_pairs and in ProgressiveAssembler, with the closed-form model of tests/test_gpu_assembly.py.
refine = 0 has to be today's table; the kernel itself is held to float64 in tests/test_gpu_icp_refine.py.

Two calls of match_pairs are not equal bit for bit in every field, with or without this feature: the few-row layers of the
encoders' global vectors and of the pose head sum their K-splits in fp32 atomics (csrc/gemm.hip, few_rows), so `twist` - and
with it T and score - carries summation-order noise from call to call (tests/test_gpu_determinism.py holds that noise to 5e-6
of the largest entry).  "The same as the call without the argument" is therefore checked as far as two calls WITHOUT the
argument agree with each other: a field that is torch.equal between two plain calls must be torch.equal to the refine = 0
call, a field that is not is held to that file's rule; on top, refine = 0 issues the same library launches with the same
integer arguments as the plain call (no launch more), T is se3.exp(twist) bit for bit and score is today's formula bit for
bit on that T.  Everything the refinement itself adds is compared on ONE table's own twist, where nothing is noisy."""
import numpy as np
import pytest
import torch

from oracle import model_ref as mr
from tests import _icp_ref as ref

pytestmark = pytest.mark.gpu

K, N, TOP = 5, 1024, 128
REFINE = 20
ATOMIC_REL = 5e-6      # tests/test_gpu_determinism.py: forward outputs behind an atomic epilogue, of the largest entry


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def model(dev):
    from puzzlenet_amd import model5_b as mb
    m = mb.TouchedRegraster(mr.Cfg())
    mr.fill_params(m)
    m.to(dev)
    return m


@pytest.fixture(scope="module")
def inputs():
    g = torch.Generator().manual_seed(2718)
    pieces = torch.rand(K, N, 3, generator=g)
    s1 = torch.randint(0, N, (K,), generator=g)
    s2 = torch.randint(0, 512, (K,), generator=g)
    return pieces, (s1, s2)


@pytest.fixture(scope="module")
def tables(dev, model, inputs):
    from puzzlenet_amd import assembly
    pieces, start = inputs
    p = pieces.to(dev)
    from puzzlenet_amd import ops
    trace = {}

    def traced(key, **kw):
        real, calls = ops._call, []

        def spy(name, *a, **k):
            calls.append((name,) + tuple(x for x in a if isinstance(x, int) and 0 <= x < (1 << 20)))
            return real(name, *a, **k)
        ops._call = spy
        try:
            out = assembly.match_pairs(model, p, k=TOP, start=start, **kw)
        finally:
            ops._call = real
        trace[key] = calls
        return out
    return dict(pieces=p, plain=traced("plain"), plain2=traced("plain2"), zero=traced("zero", refine=0),
                fine=traced("fine", refine=REFINE), trace=trace)


def _rel(a, b):
    a, b = a.double(), b.double()
    fin = torch.isfinite(b)
    assert torch.equal(fin, torch.isfinite(a))
    return float((a[fin] - b[fin]).abs().max() / b[fin].abs().max().clamp_min(1e-30))


def _same_as_far_as_reproducible(tables, other, skip=()):
    """Every field of tables[other] against the plain call: torch.equal where two plain calls are torch.equal, the atomic rule
    of tests/test_gpu_determinism.py where they are not (see the module docstring)."""
    for name in tables["plain"]._fields:
        if name in skip:
            continue
        a, a2, b = getattr(tables["plain"], name), getattr(tables["plain2"], name), getattr(tables[other], name)
        if torch.equal(a, a2):
            assert torch.equal(a, b), name
        else:
            assert a.dtype == torch.float32, f"{name}: two plain calls differ in an index field"
            print(f"{name}: two plain calls differ by {_rel(a2, a):.2e} of the largest entry; {other} by {_rel(b, a):.2e}")
            assert _rel(b, a) <= ATOMIC_REL, name


def test_refine_zero_is_todays_table(tables, inputs):
    from puzzlenet_amd import ops, se3
    _same_as_far_as_reproducible(tables, "zero")
    assert tables["trace"]["zero"] == tables["trace"]["plain"]           # the same launches: today's path, not one more
    assert not any("icp" in c[0] for c in tables["trace"]["zero"])
    assert sum("icp" in c[0] for c in tables["trace"]["fine"]) == 1      # and refine > 0 adds exactly one
    t = tables["zero"]
    assert torch.equal(t.T, se3.exp(t.twist))
    p = tables["pieces"]
    Bf = ops.index_points(p, t.top_f.reshape(K, K * TOP)).view(K * K, TOP, 3)
    Bm = ops.index_points(p, t.top_m).unsqueeze(0).expand(K, -1, -1, -1).reshape(K * K, TOP, 3)
    d1, d2 = ops.chamfer(Bf, se3.transform_points(t.T.reshape(K * K, 4, 4), Bm))
    want = (d1.mean(dim=1) + d2.mean(dim=1)).view(K, K).masked_fill(torch.eye(K, dtype=torch.bool, device=p.device), float("inf"))
    assert torch.equal(t.score, want)


def test_refined_table(tables, inputs):
    from puzzlenet_amd import assembly, se3
    t0, t = tables["plain"], tables["fine"]
    off = ~torch.eye(K, dtype=torch.bool, device=t.score.device)
    assert bool((t.score[off] <= t0.score[off]).all())
    assert bool((t.score[off] < t0.score[off]).any())                   # a pose moved somewhere
    assert bool(torch.isinf(t.score.diagonal()).all()) and bool((t.score.diagonal() > 0).all())
    _same_as_far_as_reproducible(tables, "fine", skip=("T", "score"))
    assert torch.equal(t0.T, se3.exp(t0.twist)) and not torch.equal(t.T, se3.exp(t.twist))
    # score = the chamfer of the picked rows under the returned pose, in float64 (bound: _icp_ref.objective_interval)
    pieces = inputs[0].numpy()
    top_f, top_m, T, score = t.top_f.cpu().numpy(), t.top_m.cpu().numpy(), t.T.cpu().numpy(), t.score.cpu().numpy()
    for i in range(K):
        for j in range(K):
            if i != j:
                lo, hi = ref.objective_interval(pieces[i][top_f[i, j]], pieces[j][top_m[j]], T[i, j])
                assert lo <= float(score[i, j]) <= hi, (i, j, lo, float(score[i, j]), hi)
                R = T[i, j, :3, :3].astype(np.float64)
                assert np.abs(R.T @ R - np.eye(3)).max() <= 2.0 ** -21 and np.linalg.det(R) > 0
    # refine_pairs from the network's poses - the table's own twist, see the module docstring - reproduces the table
    r = assembly.refine_pairs(tables["pieces"], t.top_f, tables["pieces"], t.top_m, se3.exp(t.twist), REFINE)
    assert torch.equal(r.T, t.T)
    assert torch.equal(r.score[off], t.score[off])
    assert r.iters_used.shape == (K, K) and r.iters_used.dtype == torch.int32 and int(r.iters_used.max()) <= REFINE
    assert bool((r.score <= r.score0).all())
    # score0 is the unrefined table's quantity by this kernel's own evaluation (bounds of
    # test_gpu_assembly.py::test_score_is_the_oracles_chamfer, which hold the chamfer kernel to the oracle)
    np.testing.assert_allclose(r.score0[off].cpu().numpy(), t0.score[off].cpu().numpy(), rtol=1e-4, atol=2e-6)
    print(f"refine = {REFINE}: mean iters_used {float(r.iters_used.float().mean()):.2f}, "
          f"mean score ratio {float((t.score[off] / t0.score[off]).mean()):.3f}")


def test_refine_pairs_rectangular_block_and_rejections(tables):
    from puzzlenet_amd import _lib, assembly
    t0, p = tables["plain"], tables["pieces"]
    full = assembly.refine_pairs(p, t0.top_f, p, t0.top_m, t0.T, 5)
    blk = assembly.refine_pairs(p[1:3], t0.top_f[1:3, 2:], p[2:], t0.top_m[2:], t0.T[1:3, 2:], 5)
    assert blk.T.shape == (2, K - 2, 4, 4)
    for a, b in zip(blk, full):
        assert torch.equal(a, b[1:3, 2:])
    with pytest.raises(_lib.PznError):
        assembly.refine_pairs(p.cpu(), t0.top_f, p, t0.top_m, t0.T, 5)
    with pytest.raises(_lib.PznError):
        assembly.refine_pairs(p, t0.top_f, p, t0.top_m, t0.T[:, :2], 5)
    with pytest.raises(_lib.PznUnsupported):
        assembly.refine_pairs(p, t0.top_f, p, t0.top_m, t0.T, -1)


def test_negative_refine_is_rejected_everywhere(dev, model, inputs):
    """One behaviour for refine < 0: PznError from match_pairs, pair_block and ProgressiveAssembler alike, before any work."""
    from puzzlenet_amd import _lib, assembly, ops
    pieces, start = inputs
    p = pieces.to(dev)
    real, calls = ops._call, []
    ops._call = lambda name, *a, **k: (calls.append(name), real(name, *a, **k))[1]
    try:
        with pytest.raises(_lib.PznError):
            assembly.match_pairs(model, p, k=TOP, start=start, refine=-1)
        with pytest.raises(_lib.PznError):
            assembly.pair_block(model, p, None, p, None, TOP, refine=-1)
        with pytest.raises(_lib.PznError):
            assembly.ProgressiveAssembler(model, p, k=TOP, start=start, refine=-1)
    finally:
        ops._call = real
    assert calls == []


def _snapshot(asm):
    t = asm.table
    return dict(parts=asm.parts.clone(), twist=t.twist.clone(), T=t.T.clone(), de_fpcb=t.de_fpcb.clone(), top_f=t.top_f.clone(),
                top_m=t.top_m.clone(), score=t.score.clone(), members=[list(m) for m in asm.members])


def _part_of(members, piece):
    return next(q for q, mem in enumerate(members) if piece in mem)


def test_progressive_merges_by_the_refined_pose(dev, model, inputs, tables):
    from puzzlenet_amd import assembly, ops, se3
    pieces, start = inputs
    asm = assembly.ProgressiveAssembler(model, pieces.to(dev), k=TOP, start=start, generator=torch.Generator().manual_seed(7),
                                        refine=REFINE)
    t = asm.table                                                        # the table it starts from: refined as match_pairs'
    r = assembly.refine_pairs(asm.parts, t.top_f, asm.parts, t.top_m, se3.exp(t.twist), REFINE)
    off = ~torch.eye(K, dtype=torch.bool, device=dev)
    assert torch.equal(r.T, t.T) and torch.equal(r.score[off], t.score[off]) and not torch.equal(t.T, se3.exp(t.twist))
    rounds = 0
    while True:
        before = _snapshot(asm)
        edge = asm.step()
        if edge is None:
            break
        i, j = _part_of(before["members"], edge[0]), _part_of(before["members"], edge[1])
        n = i if i < j else i - 1
        Kp = before["parts"].shape[0]
        # the pose of the chosen pair is the refined one ...
        r = assembly.refine_pairs(before["parts"][i:i + 1], before["top_f"][i:i + 1, j:j + 1], before["parts"][j:j + 1],
                                  before["top_m"][j:j + 1], se3.exp(before["twist"][i:i + 1, j:j + 1]), REFINE)
        assert torch.equal(r.T[0, 0], before["T"][i, j]) and torch.equal(r.score[0, 0], before["score"][i, j])
        assert not torch.equal(before["T"][i, j], se3.exp(before["twist"][i, j].reshape(1, 6))[0])
        assert edge[2] == float(before["score"][i, j])
        # ... the merge moved part j by it ...
        u = torch.tensor([asm.merge_starts[rounds]], dtype=torch.long, device=dev)
        merged, _ = ops.merge_resample(before["parts"][i:i + 1], before["parts"][j:j + 1], before["T"][i, j].reshape(1, 4, 4), u,
                                       N, before["top_f"][i, j].reshape(1, TOP), before["top_m"][j].reshape(1, TOP))
        assert torch.equal(merged[0], asm.parts[n])
        # ... and the ledger recorded it (first round: G of the moved piece IS the pose)
        if rounds == 0:
            assert np.array_equal(asm.G[edge[1]], before["T"][i, j].double().cpu().numpy())
        # entries outside the new row and column: bit for bit the table before the step
        keep = [q for q in range(Kp) if q != j]
        others = [q for q in range(Kp - 1) if q != n]
        for name in ("twist", "T", "de_fpcb", "top_f", "score"):
            was, now = before[name][keep][:, keep], getattr(asm.table, name)
            for a in others:
                for b in others:
                    assert torch.equal(now[a, b], was[a, b]), (name, a, b)
        assert bool(torch.isinf(asm.table.score.diagonal()).all())
        rounds += 1
    assert rounds == K - 1
    res = asm.result()
    pid, rid = res.piece_id.cpu(), res.row_id.cpu()
    G = res.G[pid.numpy()]
    want = np.einsum("nab,nb->na", G[:, :3, :3], pieces[pid, rid].double().numpy()) + G[:, :3, 3]
    assert float(np.abs(want - res.cloud.cpu().double().numpy()).max()) <= 1e-5      # (bound of test_gpu_progressive.py)


def test_progressive_refine_zero_is_todays_walk(dev, model, inputs):
    """refine = 0: the constructor and a round issue the launches of today's path, not one more; refine > 0 adds one per
    pair_block call (the table, then the new row and the new column)."""
    from puzzlenet_amd import assembly, ops
    pieces, start = inputs

    def launches(**kw):
        real, calls = ops._call, []

        def spy(name, *a, **k):
            calls.append(name)
            return real(name, *a, **k)
        ops._call = spy
        try:
            asm = assembly.ProgressiveAssembler(model, pieces.to(dev), k=TOP, start=start,
                                                generator=torch.Generator().manual_seed(7), **kw)
            assert asm.step() is not None
        finally:
            ops._call = real
        return calls
    plain, zero, fine = launches(), launches(refine=0), launches(refine=REFINE)
    assert zero == plain and "pzn_icp_refine_f32" not in plain
    assert fine.count("pzn_icp_refine_f32") == 3
