"""GPU: ops.assemble_forest (csrc/assemblewalk.hip, assemble_forest_kernel) against assembly.forest_rule - the numpy statement of the
rule in include/pzn.h, itself held to single linkage and to walk_rule in tests/test_assembly_forest_cpu.py - with np.array_equal on all
eleven outputs, the float64 poses included: both sides compose them in IEEE double in the same order, so there is no tolerance.  Then
the chain a pile goes through - datapipe.fracture, datapipe.pile, truth_table, assemble_forest_batch, refine_assembly_batch,
evaluate_pile_batch - end to end on a small batch.  The table kinds are those of tests/_walk_cases.py."""
import numpy as np
import pytest
import torch

from tests import _fracture as fr
from tests import _walk_cases as wc

pytestmark = pytest.mark.gpu

Z = 5                 # a second workgroup (four piles a workgroup)
IN_FLIGHT = 1024      # piles one launch holds at a time (256 workgroups of four wavefronts): more take turns


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _same(got, want):
    """Every output of ops.assemble_forest (device tensors) against forest_rule's fields (numpy): type, shape, np.array_equal."""
    assert len(got) == len(want) == 11
    for name, g, w in zip(want._fields, got, want):
        g = g.cpu().numpy()
        assert g.dtype == w.dtype and g.shape == w.shape, (name, g.dtype, g.shape)
        assert np.array_equal(g, w), name


def _run(dev, S, T, count=None, max_score=None, joint_score=None):
    from puzzlenet_amd import ops
    c = None if count is None else torch.from_numpy(count).to(dev)
    return ops.assemble_forest(torch.from_numpy(S).to(dev), torch.from_numpy(T).to(dev), c, max_score, joint_score)


@pytest.mark.parametrize("kind", wc.KINDS)
@pytest.mark.parametrize("K", (2, 3, 33, 64))
def test_kernel_is_the_rule(dev, K, kind):
    from puzzlenet_amd import assembly
    S, T, max_score = wc.make(kind, Z, K, 1300)
    want = assembly.forest_rule(S, T, max_score=max_score)
    _same(_run(dev, S, T, max_score=max_score), want)
    if kind == "random":                                # a threshold that leaves several components, explicit joint sets
        for ms, js in ((0.3 / K, None), (0.3 / K, 0.25), (None, float("inf")), (0.3 / K, float("nan"))):
            _same(_run(dev, S, T, max_score=ms, joint_score=js), assembly.forest_rule(S, T, max_score=ms, joint_score=js))
    if kind == "nan30":                                 # +inf and NaN inside a component under joint_score = +inf
        S[:, 0, 1] = np.inf
        _same(_run(dev, S, T, joint_score=float("inf")), assembly.forest_rule(S, T, joint_score=float("inf")))


def test_many_restarts(dev):
    """K = 64 with no entry at all (64 singletons: 63 roots by the fold over the table and one by the last piece left) and with a
    threshold that keeps one entry in 2 K, at most about K / 2 edges: many small components."""
    from puzzlenet_amd import assembly
    K = 64
    S, T, _ = wc.make("random", Z, K, 1400)
    S[0], S[1] = np.nan, np.inf
    want = assembly.forest_rule(S, T, max_score=0.5 / K)
    assert want.n_components[:2].tolist() == [K, K] and (want.n_components[2:] > K // 4).all() and (want.n_edges[2:] > 0).all()
    _same(_run(dev, S, T, max_score=0.5 / K), want)


@pytest.mark.parametrize("fill", (float("nan"), -1.0))
def test_mixed_counts(dev, fill):
    """Piles of 2 .. K pieces in one launch, four counts out of range; the padding holds NaN or -1 and is never read."""
    from puzzlenet_amd import assembly
    K = 33
    counts = np.array([33, 2, 17, 1, 34, 5, 0, -3, 32], dtype=np.int32)
    for kind in ("blocks", "nan30"):
        S, T, _ = wc.make(kind, len(counts), K, 1500)
        for z, c in enumerate(counts):
            c = max(int(c), 0)
            S[z, c:, :], S[z, :, c:] = fill, fill
            T[z, c:, :], T[z, :, c:] = fill, fill
        for ms in (None, 0.05):
            want = assembly.forest_rule(S, T, count=counts, max_score=ms)
            assert want.root[[3, 4, 6, 7]].tolist() == [-1] * 4 and (want.root[[0, 1, 2, 5, 8]] >= 0).all()
            _same(_run(dev, S, T, count=counts, max_score=ms), want)


def test_more_piles_than_one_launch_holds(dev):
    from puzzlenet_amd import assembly
    n = IN_FLIGHT + 6
    S, T, _ = wc.make("lattice", n, 3, 1600)
    S2, T2, _ = wc.make("nan30", n, 3, 1601)
    S[::2], T[::2] = S2[::2], T2[::2]
    want = assembly.forest_rule(S, T)
    assert len(set(want.n_components.tolist())) > 1
    _same(_run(dev, S, T), want)


def test_two_runs_give_the_same_bits(dev):
    S, T, m = wc.make("max_score", 64, 33, 1700)
    a, b = _run(dev, S, T, max_score=m), _run(dev, S, T, max_score=m)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert int(a[10].max()) > 1


@pytest.mark.parametrize("K", (5, 64))
def test_a_complete_walk_is_the_walk(dev, K):
    """Where every pile's walk completes, the forest's eight shared outputs are ops.assemble_walk's."""
    from puzzlenet_amd import ops
    for kind in ("lattice", "random"):
        S, T, _ = wc.make(kind, Z, K, 1800)
        s, t = torch.from_numpy(S).to(dev), torch.from_numpy(T).to(dev)
        walk, forest = ops.assemble_walk(s, t), ops.assemble_forest(s, t)
        assert bool(walk[5].all()) and forest[10].tolist() == [1] * Z
        assert all(torch.equal(x, y) for x, y in zip(walk, forest[:8]))


def test_interface_edges(dev):
    from puzzlenet_amd import _lib, ops
    S, T, _ = wc.make("random", 2, 4, 1900)
    s, t = torch.from_numpy(S).to(dev), torch.from_numpy(T).to(dev)
    with pytest.raises(_lib.PznError):
        ops.assemble_forest(s.cpu(), t)
    with pytest.raises(_lib.PznError):
        ops.assemble_forest(s, t[:, :3])
    with pytest.raises(_lib.PznError):
        ops.assemble_forest(s, t, count=torch.zeros(2, dtype=torch.int64, device=dev))
    with pytest.raises(_lib.PznError):
        ops.assemble_forest(s, t, max_score=float("nan"))
    for K in (1, 65):
        with pytest.raises(_lib.PznUnsupported):
            ops.assemble_forest(torch.zeros(1, K, K, device=dev), torch.zeros(1, K, K, 4, 4, device=dev))
    assert ops.assemble_forest_supported(2) and ops.assemble_forest_supported(64) and not ops.assemble_forest_supported(65)
    # the library itself: K = 65 is refused before any launch (nothing is read: the pointers are null), Z = 0 is a success, a NaN
    # max_score is an invalid argument
    lib, o = _lib.load(), None
    raw = lambda max_score, Z, K: lib.pzn_assemble_forest_f32(o, o, o, max_score, 1.0, Z, K, o, o, o, o, o, o, o, o, o, o, o, o)
    assert raw(1.0, 1, 65) == _lib.CONSTANTS["PZN_EUNSUPPORTED"] and raw(1.0, 0, 4) == _lib.CONSTANTS["PZN_OK"]
    assert raw(float("nan"), 1, 4) == _lib.CONSTANTS["PZN_EINVAL"]
    empty = ops.assemble_forest(s[:0], t[:0])
    assert [tuple(x.shape) for x in empty] == [(0,), (0, 3, 3), (0, 3), (0,), (0, 4, 4, 4), (0, 4), (0, 12, 2), (0,), (0, 4), (0, 4),
                                              (0,)]


# --------------------------------------------------------------------------- a small pile end to end

FB, FM, FP, FK, Fn, Fk, FQ = 4, 4096, 3, 8, 256, 32, 2      # clouds, points, pieces, candidates, n, k; objects per pile
TOL = 0.01


@pytest.fixture(scope="module")
def piles(dev):
    """Two piles of two fractured clouds each under a fixed shuffle, the table a perfect matcher returns for them, the forest over
    it and its refinement; computed once.

    The table is one a matcher can return: top_f[a,c] is the fracture's - piece a's k rows nearest to piece c - and top_m[c], of
    which a PairTable has one per moved piece, is piece c's k rows nearest to its partner, the piece of its object it touches
    best (the smallest fracture cd).  T is truth_table's, mates complete inside an object, and the score is PairTable.score's
    definition on these picks under T - the chamfer of the two picked sets where they belong -, +inf across objects.  Towards its
    partner a piece scores the fracture's cd; any other entry compares two different faces of the moved piece and scores their
    distance.  So the walk connects every object through entries whose two sets are the two sides of one break, whichever faces
    pass the 0.015 contact threshold, and the joints - no worse than the worst edge - are such entries too: the refinement is
    asked about breaks that close where the truth puts them."""
    from puzzlenet_amd import assembly, datapipe, ops
    raw = fr.clouds(FB, FM, 50)
    normals, u_anchor, u_start, twist = fr.draws(FB, FP, FK, 51)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    frac = datapipe.fracture(to(raw), to(normals), to(u_anchor), to(u_start), to(twist), n=Fn, k=Fk)
    perm = torch.tensor([[4, 0, 3, 2, 5, 1], [1, 5, 0, 4, 2, 3]], device=dev)
    pile = datapipe.pile(frac, objects=FQ, perm=perm)
    ZP, K = FB // FQ, FQ * FP
    same = pile.object_of[:, :, None] == pile.object_of[:, None, :]
    off = ~torch.eye(K, dtype=torch.bool, device=dev)
    partner = pile.cd.masked_fill(~off, float("inf")).argmin(dim=2)                              # [ZP,K], of the same object
    src = pile.source.long()
    b, p = torch.arange(ZP, device=dev)[:, None] * FQ + src // FP, src % FP
    near = frac.top[b[:, :, None], p[:, :, None], torch.where(same, p[:, None, :], p[:, :, None])]      # [ZP,K,K,k]; across: any rows
    top_f = near
    top_m = near[torch.arange(ZP, device=dev)[:, None], torch.arange(K, device=dev)[None, :], partner]
    rest = pile.rest.reshape(ZP * K, Fn, 3)
    A = ops.index_points(rest, top_f.reshape(ZP * K, K * Fk)).view(ZP, K, K, Fk, 3)
    Bm = ops.index_points(rest, top_m.reshape(ZP * K, Fk)).view(ZP, 1, K, Fk, 3).expand(ZP, K, K, Fk, 3)
    d1, d2 = ops.chamfer(A.reshape(-1, Fk, 3).contiguous(), Bm.reshape(-1, Fk, 3).contiguous())
    picked = (d1.mean(dim=1) + d2.mean(dim=1)).view(ZP, K, K)
    tables = [assembly.truth_table(pile.pose[z], same[z], picked[z]) for z in range(ZP)]
    T = torch.from_numpy(np.stack([t for t, _ in tables]).astype(np.float32)).to(dev)
    S = torch.from_numpy(np.stack([s for _, s in tables]).astype(np.float32)).to(dev)
    forest = assembly.assemble_forest_batch(S, T)
    table = assembly.PairTable(None, T, None, None, top_f, top_m, S, None)
    refined = assembly.refine_assembly_batch(pile.pieces, table, forest, sweeps=2)
    return dict(frac=frac, pile=pile, perm=perm, S=S, T=T, forest=forest, refined=refined, ZP=ZP, K=K, partner=partner, picked=picked)


def test_pile_regroups_the_fracture(piles):
    frac, pile, perm = piles["frac"], piles["pile"], piles["perm"]
    ZP, K = piles["ZP"], piles["K"]
    assert bool(frac.ok.all()) and pile.ok.tolist() == [True] * ZP
    assert torch.equal(pile.source.long(), perm) and torch.equal(pile.object_of.long(), perm // FP)
    for z in range(ZP):
        for a in range(K):
            q, pa = divmod(int(perm[z, a]), FP)
            assert torch.equal(pile.pieces[z, a], frac.pieces[z * FQ + q, pa]) and torch.equal(pile.pose[z, a], frac.pose[z * FQ + q, pa])
            assert torch.equal(pile.rest[z, a], frac.rest[z * FQ + q, pa])
    same = pile.object_of[:, :, None] == pile.object_of[:, None, :]
    assert not bool((pile.mates & ~same).any()) and bool(torch.isinf(pile.cd[~same]).all()) and bool(torch.isfinite(pile.cd[same]).all())


def test_forest_batch_sorts_and_assembles_the_piles(dev, piles):
    from puzzlenet_amd import assembly, ops
    pile, forest, ZP, K = piles["pile"], piles["forest"], piles["ZP"], piles["K"]
    want = assembly.forest_rule(piles["S"], piles["T"])
    _same((forest.root, forest.edges, forest.edge_score, forest.n_edges, forest.G, forest.placed.to(torch.uint8), forest.joints,
           forest.n_joints, forest.component, forest.roots, forest.n_components), want)
    is_root = np.zeros((ZP, K), dtype=bool)
    for z in range(ZP):
        is_root[z, want.roots[z, :want.n_components[z]]] = True
    assert np.array_equal(forest.movable.cpu().numpy(), ~is_root) and forest.movable.dtype == torch.bool
    real, calls = ops._call, []

    def spy(name, *a, **k):
        calls.append(name)
        return real(name, *a, **k)
    ops._call = spy
    try:
        assembly.assemble_forest_batch(piles["S"], piles["T"])
    finally:
        ops._call = real
    assert calls == ["pzn_assemble_forest_f32"]
    ev = assembly.evaluate_pile_batch(forest.G, forest.component, pile.pose, pile.rest, pile.object_of)
    print("forest: n_components", ev.n_components.tolist(), "max msd together",
          float(ev.msd[forest.component[:, :, None] == forest.component[:, None, :]].max()))
    assert ev.exact.tolist() == [True] * ZP and ev.n_components.tolist() == [FQ] * ZP
    assert ev.pair_precision.tolist() == ev.pair_recall.tolist() == ev.pair_pose_recall.tolist() == [1.0] * ZP
    # the one-tree walk on the same tables places one object of each pile
    walk = assembly.assemble_batch(piles["S"], piles["T"])
    assert walk.placed.sum(dim=1).tolist() == [FP] * ZP


def test_refinement_takes_the_forest_as_it_is(dev, piles):
    """Two sweeps over both piles' components in the one launch: the summed score falls (0.051 -> 0.033 and 0.071 -> 0.050 when
    this was written), no root moves, and the largest msd between two pieces of one object stays at 0.0041, under tol = 0.01 - the
    picked sets of a break's two sides are different samples of it, so its chamfer minimum lies a sample spacing off the truth."""
    from puzzlenet_amd import assembly
    pile, forest, out, ZP, K = piles["pile"], piles["forest"], piles["refined"], piles["ZP"], piles["K"]
    assert out.G.shape == (ZP, K, 4, 4) and out.joints is forest.joints
    # every joint asks a piece about its partner: the two sets are the two sides of one break (the fixture's docstring)
    for z in range(ZP):
        js = forest.joints[z, :int(forest.n_joints[z])].tolist()
        print(f"pile {z}: partner {piles['partner'][z].tolist()}, joints {js}, edge scores {forest.edge_score[z].tolist()}")
        assert len(js) >= K - FQ and all(int(piles["partner"][z, j]) == i for i, j in js)
        at = (piles["partner"][z], torch.arange(K, device=dev))                # towards its partner: the fracture's cd
        assert torch.allclose(piles["picked"][z][at], pile.cd[z][at], rtol=1e-5, atol=0)
    print("refinement: score0", out.score0.tolist(), "score", out.score.tolist(), "accepted", out.accepted.tolist())
    assert bool((out.score <= out.score0).all())
    g0 = forest.G.to(torch.float32)
    for z in range(ZP):                                  # the roots' poses are unchanged, bit for bit
        for r in forest.roots[z, :int(forest.n_components[z])].tolist():
            assert torch.equal(out.G[z, r], g0[z, r]) and int(out.accepted[z, r]) == 0
    ev = assembly.evaluate_pile_batch(out.G, forest.component, pile.pose, pile.rest, pile.object_of, tol=TOL)
    together = (forest.component[:, :, None] == forest.component[:, None, :]) & ~torch.eye(K, dtype=torch.bool, device=dev)
    print("refined: max msd together", float(ev.msd[together].max()), "ratios", ev.pair_precision.tolist(), ev.pair_recall.tolist(),
          ev.pair_pose_recall.tolist())
    assert ev.exact.tolist() == [True] * ZP
    assert ev.pair_precision.tolist() == ev.pair_recall.tolist() == ev.pair_pose_recall.tolist() == [1.0] * ZP
    # the batched score against the host's, pile by pile, to the tolerance of tests/test_gpu_assembly_batch.py
    for z in range(ZP):
        one = assembly.evaluate_pile(out.G[z], forest.component[z], pile.pose[z], pile.rest[z], pile.object_of[z], tol=TOL)
        msd = ev.msd[z].cpu().numpy()
        print(f"pile {z}: msd abs diff {np.abs(msd - one.msd).max():.2e}, rel "
              f"{np.abs(msd / np.where(one.msd > 0, one.msd, 1.0) - 1)[one.msd > 0].max():.2e}")
        assert np.abs(msd - one.msd).max() <= 1e-12 and (np.abs(msd - one.msd) <= 1e-12 * one.msd).all()
        assert (float(ev.pair_precision[z]), float(ev.pair_recall[z]), float(ev.pair_pose_recall[z]), int(ev.n_components[z]),
                bool(ev.exact[z])) == one[:5]


def test_evaluate_pile_batch_counts(dev, piles):
    """Merged objects, a split object and counts below K, against the host on the same inputs (NaN ratios included)."""
    from puzzlenet_amd import assembly
    pile, forest, ZP, K = piles["pile"], piles["forest"], piles["ZP"], piles["K"]
    comp = forest.component.clone()
    comp[0] = 0                                          # pile 0: both objects in one component
    comp[1, int(forest.roots[1, 1])] = 7                 # pile 1: a root split off its component
    count = torch.tensor([K, 1], dtype=torch.int32, device=dev)
    for cnt in (None, count):
        ev = assembly.evaluate_pile_batch(forest.G, comp, pile.pose, pile.rest, pile.object_of, cnt)
        for z in range(ZP):
            one = assembly.evaluate_pile(forest.G[z], comp[z], pile.pose[z], pile.rest[z], pile.object_of[z],
                                         None if cnt is None else int(cnt[z]))
            got = (float(ev.pair_precision[z]), float(ev.pair_recall[z]), float(ev.pair_pose_recall[z]))
            assert all((a != a and b != b) or a == b for a, b in zip(got, one[:3])), (got, one[:3])
            assert int(ev.n_components[z]) == one.n_components and bool(ev.exact[z]) == one.exact
    assert float(ev.pair_precision[1]) != float(ev.pair_precision[1])      # one piece counted: no pair
    with pytest.raises(assembly._lib.PznError):
        assembly.evaluate_pile_batch(forest.G.cpu(), comp, pile.pose, pile.rest, pile.object_of)
    with pytest.raises(assembly._lib.PznError):
        assembly.evaluate_pile_batch(forest.G[:, :3], comp, pile.pose, pile.rest, pile.object_of)
