"""GPU: ops.assemble_forest_beam (csrc/assemblebeam.hip, assemble_forest_beam_kernel) against assembly.forest_beam_rule -
the numpy statement of the rule in include/pzn.h, itself held to forest_rule, to beam_rule and to a scalar replay in
tests/test_assembly_forest_beam_cpu.py - bit for bit in all thirteen outputs, the float64 poses and costs included: both sides do
the same IEEE double operations in the same order, so there is no tolerance.  Then against the two kernels it joins,
ops.assemble_forest at beam = branch = 1 and ops.assemble_beam on tables without a restart, and on piles of planted objects.  The
table kinds are those of tests/_beam_cases.py, the piles those of tests/_forest_beam_cases.py."""
import numpy as np
import pytest
import torch

from tests import _beam_cases as bc
from tests import _forest_beam_cases as fb

pytestmark = pytest.mark.gpu

Z = 5
SIZES = (2, 3, 5, 8, 17)
BEAMS = ((1, 1), (1, 4), (4, 4), (3, 5), (8, 8))
KINDS = bc.KINDS + ("pile",)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _same(got, want):
    """Every output of ops.assemble_forest_beam (device tensors) against forest_beam_rule's fields (numpy), torch.equal."""
    assert len(got) == len(want) == 13
    for name, g, w in zip(want._fields, got, want):
        w = torch.from_numpy(w)
        assert g.dtype == w.dtype and g.shape == w.shape, (name, g.dtype, tuple(g.shape))
        assert torch.equal(g.cpu(), w), name


def _run(dev, S, T, M, count=None, **kw):
    from puzzlenet_amd import ops
    c = None if count is None else torch.from_numpy(count).to(dev)
    return ops.assemble_forest_beam(torch.from_numpy(S).to(dev), torch.from_numpy(T).to(dev), torch.from_numpy(M).to(dev), c, **kw)


def _make(kind, K, seed):
    """-> (score [Z,K',K'], T, moment, max_score): a kind of tests/_beam_cases.py, or Z piles of two objects of max(2, K // 2)
    pieces (K' = 2, 2, 4, 8, 16 -> 4, 4, 4, 8, 16)."""
    if kind == "pile":
        return fb.piles(range(seed, seed + Z), 2, max(2, K // 2))[:3] + (fb.MAX_SCORE,)
    return bc.make(kind, Z, K, seed)


@pytest.mark.parametrize("kind", KINDS)
def test_kernel_is_the_rule(dev, kind):
    """Every size with two (beam, branch) pairs, one under weight 1 and one under weight 0, turning with the kind and the size so
    that every pair meets every size; ragged counts with 0 and 1 among them."""
    from puzzlenet_amd import assembly
    several = differs = False
    for n, K in enumerate(SIZES):
        S, T, M, max_score = _make(kind, K, 600)
        count = bc.ragged(Z, S.shape[1])
        greedy = assembly.forest_rule(S, T, count=count, max_score=max_score)
        at = KINDS.index(kind) + n
        for (B, C), weight in ((BEAMS[at % 5], 1.0), (BEAMS[(at + 2) % 5], 0.0)):
            kw = dict(beam=B, branch=C, weight=weight, max_score=max_score)
            want = assembly.forest_beam_rule(S, T, M, count=count, **kw)
            _same(_run(dev, S, T, M, count, **kw), want)
            several |= bool((want.n_components > 1).any())
            differs |= not np.array_equal(want.edges, greedy.edges)
    if kind in ("max_score", "blocks", "pile"):
        assert several                                   # a restart child won somewhere
    if kind == "pile":
        assert differs                                   # and so did a child of rank > 0: not the forest walk's edges


@pytest.mark.parametrize("BC", BEAMS)
def test_lattice_ties_under_weight_zero(dev, BC):
    """Integer scores and weight 0: most selections are cost ties, decided by (slot, rank); with a threshold, restarts among them."""
    from puzzlenet_amd import assembly
    S, T, M, _ = bc.make("lattice", Z, 8, 610)
    for max_score in (None, 0.0):
        kw = dict(beam=BC[0], branch=BC[1], weight=0.0, max_score=max_score)
        _same(_run(dev, S, T, M, None, **kw), assembly.forest_beam_rule(S, T, M, **kw))


def test_limits_and_restart_cost(dev):
    from puzzlenet_amd import assembly
    S, T, M, _ = bc.make("random", Z, 8, 620)
    several = False
    for kw in (dict(max_score=0.5, vote_score=0.25), dict(max_score=0.1), dict(vote_score=0.1, joint_score=0.3),
               dict(max_score=0.1, restart_cost=0.0, joint_score=0.05), dict(max_score=0.1, restart_cost=5.0, weight=2.5),
               dict(max_score=0.1, restart_cost=float("nan"), vote_score=float("inf"), joint_score=float("inf")),
               dict(max_score=0.05, restart_cost=-1.0, beam=8, branch=8)):
        want = assembly.forest_beam_rule(S, T, M, **kw)
        _same(_run(dev, S, T, M, None, **kw), want)
        several |= bool((want.n_components > 1).any())
    assert several


def test_sixty_four_pieces(dev):
    """K = 64, B = 8: the largest LDS footprint (above 64 KB: the attribute is set), on a table with many restarts; and B = C = 2."""
    from puzzlenet_amd import assembly
    S, T, M, max_score = bc.make("max_score", 1, 64, 630)
    kw = dict(beam=8, branch=2, max_score=max_score)
    want = assembly.forest_beam_rule(S, T, M, **kw)
    assert int(want.n_components[0]) > 1
    _same(_run(dev, S, T, M, None, **kw), want)
    S, T, M, _ = bc.make("random", 2, 64, 631)
    kw = dict(beam=2, branch=2)
    _same(_run(dev, S, T, M, None, **kw), assembly.forest_beam_rule(S, T, M, **kw))


def test_beam_one_branch_one_is_the_forest_kernel(dev):
    from puzzlenet_amd import ops
    for kind, K in (("lattice", 8), ("nan30", 17), ("max_score", 33), ("blocks", 8)):
        S, T, M, max_score = bc.make(kind, Z, K, 640)
        count = bc.ragged(Z, K)
        c = torch.from_numpy(count).to(dev)
        forest = ops.assemble_forest(torch.from_numpy(S).to(dev), torch.from_numpy(T).to(dev), c, max_score)
        for weight in (0.0, 1.0):
            got = _run(dev, S, T, M, count, beam=1, branch=1, weight=weight, max_score=max_score)
            assert all(torch.equal(a, b) for a, b in zip(forest, got[:11]))
            assert got[12].tolist() == [int(2 <= x <= K) for x in count]


def test_without_a_restart_it_is_the_beam_kernel(dev):
    from puzzlenet_amd import ops
    for kind, K in (("random", 17), ("planted", 8)):
        S, T, M, _ = bc.make(kind, Z, K, 650)
        count = bc.ragged(Z, K)
        s, t, m, c = (torch.from_numpy(x).to(dev) for x in (S, T, M, count))
        for B, C in ((4, 4), (8, 8)):
            beam = ops.assemble_beam(s, t, m, c, beam=B, branch=C)
            got = ops.assemble_forest_beam(s, t, m, c, beam=B, branch=C)
            assert all(torch.equal(a, b) for a, b in zip(beam, got[:8] + got[11:]))
            assert got[10].tolist() == [int(2 <= x <= K) for x in count]


def test_two_runs_give_the_same_bits(dev):
    S, T, M, max_score = bc.make("max_score", 16, 17, 660)
    a = _run(dev, S, T, M, None, beam=8, branch=8, max_score=max_score)
    b = _run(dev, S, T, M, None, beam=8, branch=8, max_score=max_score)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert int(a[10].max()) > 1


def test_planted_piles_end_to_end(dev):
    """assemble_forest_beam_batch on four planted piles of two objects of six pieces: one library call, movable excludes every
    root, every pile right; assemble_forest_batch on the same tables is right on none."""
    from puzzlenet_amd import assembly, ops
    Zp = 4
    S, T, M, pose, object_of, max_score = fb.piles(range(Zp), 2, 6)
    K = S.shape[1]
    s, t, m = (torch.from_numpy(x).to(dev) for x in (S, T, M))
    real, calls = ops._call, []

    def spy(name, *a, **k):
        calls.append(name)
        return real(name, *a, **k)
    ops._call = spy
    try:
        asm = assembly.assemble_forest_beam_batch(s, t, m, max_score=max_score)
    finally:
        ops._call = real
    assert calls == ["pzn_assemble_forest_beam_f32"]
    assert asm._fields == assembly.ForestBatch._fields + ("cost", "n_hyp")
    want = assembly.forest_beam_rule(S, T, M, max_score=max_score)      # the defaults: beam = branch = 4, weight = 1
    _same((asm.root, asm.edges, asm.edge_score, asm.n_edges, asm.G, asm.placed.to(torch.uint8), asm.joints, asm.n_joints,
           asm.component, asm.roots, asm.n_components, asm.cost, asm.n_hyp), want)
    assert asm.placed.dtype == torch.bool and asm.movable.dtype == torch.bool and asm.cost.shape == (Zp, 4)
    is_root = np.zeros((Zp, K), dtype=bool)
    for z in range(Zp):
        is_root[z, want.roots[z, :want.n_components[z]]] = True
    assert np.array_equal(asm.movable.cpu().numpy(), ~is_root) and is_root.sum() == 2 * Zp
    forest = assembly.assemble_forest_batch(s, t, max_score=max_score)
    G, comp, roots, nc = (x.cpu().numpy() for x in (asm.G, asm.component, asm.roots, asm.n_components))
    fG, fcomp, froots, fnc = (x.cpu().numpy() for x in (forest.G, forest.component, forest.roots, forest.n_components))
    beam_right = [fb.right(G[z], comp[z], roots[z], nc[z], pose[z], object_of[z]) for z in range(Zp)]
    forest_right = [fb.right(fG[z], fcomp[z], froots[z], fnc[z], pose[z], object_of[z]) for z in range(Zp)]
    print("planted piles: forest beam right", beam_right, "forest walk right", forest_right)
    assert all(beam_right) and not any(forest_right)


def test_argument_errors_and_empty_batch(dev):
    from puzzlenet_amd import _lib, ops
    S, T, M, _ = bc.make("random", 2, 4, 670)
    s, t, m = (torch.from_numpy(x).to(dev) for x in (S, T, M))
    for bad in (lambda: ops.assemble_forest_beam(s.cpu(), t, m), lambda: ops.assemble_forest_beam(s, t, m.cpu()),
                lambda: ops.assemble_forest_beam(s, t, m.float()), lambda: ops.assemble_forest_beam(s, t[:, :3], m),
                lambda: ops.assemble_forest_beam(s, t, m[:, :3]),
                lambda: ops.assemble_forest_beam(s, t, m, count=torch.zeros(2, dtype=torch.int64, device=dev)),
                lambda: ops.assemble_forest_beam(s, t, m, max_score=float("nan")),
                lambda: ops.assemble_forest_beam(s, t, m, weight=float("nan"))):
        with pytest.raises(_lib.PznError):
            bad()
    for K, B, C in ((1, 4, 4), (65, 4, 4), (4, 0, 4), (4, 9, 4), (4, 4, 9)):
        with pytest.raises(_lib.PznUnsupported):
            ops.assemble_forest_beam(torch.zeros(1, K, K, device=dev), torch.zeros(1, K, K, 4, 4, device=dev),
                                     torch.zeros(1, K, 4, 4, dtype=torch.float64, device=dev), beam=B, branch=C)
    assert ops.assemble_forest_beam_supported(2, 1, 1) and ops.assemble_forest_beam_supported(64, 8, 8)
    assert not ops.assemble_forest_beam_supported(65, 1, 1) and not ops.assemble_forest_beam_supported(8, 9, 1)
    # the library itself: refused before any launch (nothing is read: the pointers are null), Z = 0 is a success
    lib, o = _lib.load(), None
    raw = lambda B, weight, max_score, n, K: lib.pzn_assemble_forest_beam_f32(o, o, o, o, B, 4, weight, max_score, 1.0, 1.0, 1.0, n, K,
                                                                               o, o, o, o, o, o, o, o, o, o, o, o, o, o)
    assert raw(4, 1.0, 1.0, 1, 65) == raw(9, 1.0, 1.0, 1, 8) == _lib.CONSTANTS["PZN_EUNSUPPORTED"]
    assert raw(4, float("nan"), 1.0, 1, 4) == raw(4, 1.0, float("nan"), 1, 4) == _lib.CONSTANTS["PZN_EINVAL"]
    assert raw(4, 1.0, 1.0, 0, 4) == _lib.CONSTANTS["PZN_OK"]
    empty = ops.assemble_forest_beam(s[:0], t[:0], m[:0], beam=3)
    assert [tuple(x.shape) for x in empty] == [(0,), (0, 3, 3), (0, 3), (0,), (0, 4, 4, 4), (0, 4), (0, 12, 2), (0,), (0, 4), (0, 4),
                                              (0,), (0, 3), (0,)]
