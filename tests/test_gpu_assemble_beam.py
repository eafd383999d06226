"""GPU: ops.assemble_beam (csrc/assemblebeam.hip, assemble_beam_kernel) against assembly.beam_rule - the numpy statement of the
rule in include/pzn.h, itself held to walk_rule and to a scalar replay in tests/test_assembly_beam_cpu.py - bit for bit in every
output, the float64 poses and costs included: both sides do the same IEEE double operations in the same order, so there is no
tolerance.  The table kinds are those of tests/_beam_cases.py."""
import numpy as np
import pytest
import torch

from tests import _beam_cases as bc

pytestmark = pytest.mark.gpu

Z = 5
SIZES = (2, 3, 5, 8, 17)
BEAMS = ((1, 1), (1, 4), (4, 4), (3, 5), (8, 8))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _same(got, want):
    """Every output of ops.assemble_beam (device tensors) against beam_rule's fields (numpy), torch.equal."""
    assert len(got) == len(want) == 10
    for name, g, w in zip(want._fields, got, want):
        w = torch.from_numpy(w)
        assert g.dtype == w.dtype and g.shape == w.shape, (name, g.dtype, tuple(g.shape))
        assert torch.equal(g.cpu(), w), name


def _run(dev, S, T, M, count=None, **kw):
    from puzzlenet_amd import ops
    c = None if count is None else torch.from_numpy(count).to(dev)
    return ops.assemble_beam(torch.from_numpy(S).to(dev), torch.from_numpy(T).to(dev), torch.from_numpy(M).to(dev), c, **kw)


@pytest.mark.parametrize("kind", bc.KINDS)
def test_kernel_is_the_rule(dev, kind):
    """Every size with two (beam, branch) pairs, one under weight 1 and one under weight 0, turning with the kind and the size so
    that every pair meets every size; ragged counts with 0 and 1 among them.  lattice under weight 0 is decided by (slot, rank)."""
    from puzzlenet_amd import assembly
    beam_mattered = False
    for n, K in enumerate(SIZES):
        S, T, M, max_score = bc.make(kind, Z, K, 500)
        count = bc.ragged(Z, K)
        greedy = assembly.walk_rule(S, T, count=count, max_score=max_score)
        at = bc.KINDS.index(kind) + n
        for (B, C), weight in ((BEAMS[at % 5], 1.0), (BEAMS[(at + 2) % 5], 0.0)):
            kw = dict(beam=B, branch=C, weight=weight, max_score=max_score)
            want = assembly.beam_rule(S, T, M, count=count, **kw)
            _same(_run(dev, S, T, M, count, **kw), want)
            beam_mattered |= not np.array_equal(want.edges, greedy.edges)
    if kind in ("random", "planted"):
        assert beam_mattered                             # some result is not the greedy tree: a child of rank > 0 won


@pytest.mark.parametrize("BC", BEAMS)
def test_lattice_ties_under_weight_zero(dev, BC):
    """Integer scores and weight 0: most selections are cost ties, decided by (slot, rank)."""
    from puzzlenet_amd import assembly
    S, T, M, _ = bc.make("lattice", Z, 8, 510)
    kw = dict(beam=BC[0], branch=BC[1], weight=0.0)
    _same(_run(dev, S, T, M, None, **kw), assembly.beam_rule(S, T, M, **kw))


def test_max_score_and_vote_score(dev):
    from puzzlenet_amd import assembly
    S, T, M, _ = bc.make("random", Z, 8, 520)
    for kw in (dict(max_score=0.5, vote_score=0.25), dict(max_score=0.5), dict(vote_score=0.1, joint_score=0.3),
               dict(max_score=0.2, vote_score=float("inf"), joint_score=float("inf"), weight=2.5)):
        want = assembly.beam_rule(S, T, M, **kw)
        _same(_run(dev, S, T, M, None, **kw), want)
    assert (want.n_edges < 7).any()


def test_sixty_four_pieces(dev):
    from puzzlenet_amd import assembly
    S, T, M, _ = bc.make("random", 2, 64, 530)
    kw = dict(beam=2, branch=2)
    _same(_run(dev, S, T, M, None, **kw), assembly.beam_rule(S, T, M, **kw))


def test_beam_one_branch_one_is_the_walk_kernel(dev):
    from puzzlenet_amd import ops
    for kind, K in (("lattice", 8), ("nan30", 17), ("max_score", 33), ("planted", 8)):
        S, T, M, max_score = bc.make(kind, Z, K, 540)
        count = bc.ragged(Z, K)
        c = torch.from_numpy(count).to(dev)
        walk = ops.assemble_walk(torch.from_numpy(S).to(dev), torch.from_numpy(T).to(dev), c, max_score)
        for weight in (0.0, 1.0):
            beam = _run(dev, S, T, M, count, beam=1, branch=1, weight=weight, max_score=max_score)
            assert all(torch.equal(a, b) for a, b in zip(walk, beam[:8]))
            assert beam[9].tolist() == [int(2 <= x <= K) for x in count]


def test_two_runs_give_the_same_bits(dev):
    S, T, M, _ = bc.make("lattice", 16, 17, 550)
    a, b = _run(dev, S, T, M, None, beam=8, branch=8), _run(dev, S, T, M, None, beam=8, branch=8)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_assemble_beam_batch_is_one_launch(dev):
    from puzzlenet_amd import assembly, ops
    K = 5
    S, T, M, _ = bc.make("planted", Z, K, 560)
    s, t, m = (torch.from_numpy(x).to(dev) for x in (S, T, M))
    real, calls = ops._call, []

    def spy(name, *a, **k):
        calls.append(name)
        return real(name, *a, **k)
    ops._call = spy
    try:
        asm = assembly.assemble_beam_batch(s, t, m)
    finally:
        ops._call = real
    assert calls == ["pzn_assemble_beam_f32"]
    assert asm._fields == assembly.AssemblyBatch._fields + ("cost", "n_hyp")
    want = assembly.beam_rule(S, T, M)                   # the defaults: beam = branch = 4, weight = 1
    _same((asm.root, asm.edges, asm.edge_score, asm.n_edges, asm.G, asm.placed.to(torch.uint8), asm.joints, asm.n_joints, asm.cost,
           asm.n_hyp), want)
    assert asm.placed.dtype == torch.bool and asm.movable.dtype == torch.bool and asm.cost.shape == (Z, 4)
    movable = want.placed.astype(bool) & (np.arange(K)[None, :] != want.root[:, None])
    assert np.array_equal(asm.movable.cpu().numpy(), movable)


def test_argument_errors_and_empty_batch(dev):
    from puzzlenet_amd import _lib, ops
    S, T, M, _ = bc.make("random", 2, 4, 570)
    s, t, m = (torch.from_numpy(x).to(dev) for x in (S, T, M))
    for bad in (lambda: ops.assemble_beam(s.cpu(), t, m), lambda: ops.assemble_beam(s, t, m.cpu()),
                lambda: ops.assemble_beam(s.double(), t, m), lambda: ops.assemble_beam(s, t, m.float()),
                lambda: ops.assemble_beam(s, t[:, :3], m), lambda: ops.assemble_beam(s, t, m[:, :3]),
                lambda: ops.assemble_beam(s, t, m[0]), lambda: ops.assemble_beam(s[0], t[0], m[0]),
                lambda: ops.assemble_beam(s, t, m, count=torch.zeros(2, dtype=torch.int64, device=dev)),
                lambda: ops.assemble_beam(s, t, m, count=torch.zeros(3, dtype=torch.int32, device=dev)),
                lambda: ops.assemble_beam(s, t, m, max_score=float("nan")),
                lambda: ops.assemble_beam(s, t, m, weight=float("nan"))):
        with pytest.raises(_lib.PznError):
            bad()
    for K, B, C in ((1, 4, 4), (65, 4, 4), (4, 0, 4), (4, 9, 4), (4, 4, 0), (4, 4, 9)):
        with pytest.raises(_lib.PznUnsupported):
            ops.assemble_beam(torch.zeros(1, K, K, device=dev), torch.zeros(1, K, K, 4, 4, device=dev),
                              torch.zeros(1, K, 4, 4, dtype=torch.float64, device=dev), beam=B, branch=C)
    assert ops.assemble_beam_supported(2, 1, 1) and ops.assemble_beam_supported(64, 8, 8) and not ops.assemble_beam_supported(65, 8, 8)
    assert not ops.assemble_beam_supported(64, 9, 1) and not ops.assemble_beam_supported(64, 1, 9)
    empty = ops.assemble_beam(s[:0], t[:0], m[:0], beam=3)
    assert [tuple(x.shape) for x in empty] == [(0,), (0, 3, 3), (0, 3), (0,), (0, 4, 4, 4), (0, 4), (0, 12, 2), (0,), (0, 3), (0,)]


def test_end_to_end_on_a_matched_batch(dev):
    """match_puzzles -> boundary_moments -> assemble_beam_batch -> refine_assembly_batch -> evaluate_batch at the smallest setup
    of tests/test_gpu_assembly_batch.py; the beam result is beam_rule on the downloaded table."""
    from oracle import model_ref as mr
    from puzzlenet_amd import assembly, model5_b as mb, ops
    Zp, P, N, TOP = 3, 3, 1024, 128
    model = mb.TouchedRegraster(mr.Cfg())
    mr.fill_params(model)
    model.to(dev)
    g = torch.Generator().manual_seed(3141)
    pieces = torch.rand(Zp, P, N, 3, generator=g).to(dev)
    s1, s2 = torch.randint(0, N, (Zp, P), generator=g), torch.randint(0, 512, (Zp, P), generator=g)
    table = assembly.match_puzzles(model, pieces, k=TOP, start=(s1, s2))
    moment = assembly.boundary_moments(pieces, table.top_m)
    assert moment.shape == (Zp, P, 4, 4) and moment.dtype == torch.float64 and moment.is_cuda
    x = ops.index_points(pieces.view(Zp * P, N, 3), table.top_m.view(Zp * P, TOP)).double().cpu().numpy()
    xh = np.concatenate((x, np.ones((Zp * P, TOP, 1))), axis=-1)
    want_m = np.einsum("pna,pnb->pab", xh, xh) / TOP
    # TOP products of magnitude <= 1, summed in some order in float64 and divided
    assert np.abs(moment.cpu().numpy().reshape(Zp * P, 4, 4) - want_m).max() <= 2 * TOP * 2.0 ** -53
    assert bool((moment[..., 3, 3] == 1.0).all())
    asm = assembly.assemble_beam_batch(table.score, table.T, moment)
    want = assembly.beam_rule(table.score, table.T, moment)
    _same((asm.root, asm.edges, asm.edge_score, asm.n_edges, asm.G, asm.placed.to(torch.uint8), asm.joints, asm.n_joints, asm.cost,
           asm.n_hyp), want)
    assert bool(asm.placed.all())
    out = assembly.refine_assembly_batch(pieces, table, asm, sweeps=5)
    assert out.G.shape == (Zp, P, 4, 4) and bool((out.score <= out.score0).all()) and out.joints is asm.joints
    pose = torch.eye(4, dtype=torch.float32, device=dev).expand(Zp, P, 4, 4).contiguous()
    ev = assembly.evaluate_batch(out.G, asm.placed, pose, pieces[:, :, :256].contiguous(), asm.root, asm.edges, asm.n_edges)
    assert ev.msd.shape == (Zp, P) and bool(torch.isfinite(ev.msd).all()) and ev.part_accuracy.shape == (Zp,)
