"""GPU: ops.assemble_walk (csrc/assemblewalk.hip, assemble_walk_kernel) against assembly.walk_rule - the numpy statement of the
rule in include/pzn.h, itself held to assembly.assemble in tests/test_assembly_walk_cpu.py - bit for bit in every output, the
float64 poses included: both sides compose them in IEEE double in the same order, so there is no tolerance.  The table kinds are
those of tests/_walk_cases.py."""
import numpy as np
import pytest
import torch

from tests import _walk_cases as wc

pytestmark = pytest.mark.gpu

Z = 5
IN_FLIGHT = 1024      # puzzles one launch holds at a time (256 workgroups of four wavefronts): more take turns


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _same(got, want):
    """Every output of ops.assemble_walk (device tensors) against walk_rule's fields (numpy), torch.equal."""
    assert len(got) == len(want) == 8
    for name, g, w in zip(want._fields, got, want):
        w = torch.from_numpy(w)
        assert g.dtype == w.dtype and g.shape == w.shape, (name, g.dtype, tuple(g.shape))
        assert torch.equal(g.cpu(), w), name


def _run(dev, S, T, count=None, max_score=None, joint_score=None):
    from puzzlenet_amd import ops
    c = None if count is None else torch.from_numpy(count).to(dev)
    return ops.assemble_walk(torch.from_numpy(S).to(dev), torch.from_numpy(T).to(dev), c, max_score, joint_score)


@pytest.mark.parametrize("kind", wc.KINDS)
@pytest.mark.parametrize("K", (2, 5, 33, 64))
def test_kernel_is_the_rule(dev, K, kind):
    from puzzlenet_amd import assembly
    S, T, max_score = wc.make(kind, Z, K, 500)
    want = assembly.walk_rule(S, T, max_score=max_score)
    _same(_run(dev, S, T, max_score=max_score), want)
    if kind == "random":                                # explicit and unbounded joint sets on the same walk
        for js in (0.25, float("inf")):
            _same(_run(dev, S, T, joint_score=js), assembly.walk_rule(S, T, joint_score=js))
    if kind == "nan30":                                 # +inf and NaN between placed pieces under joint_score = +inf
        S[:, 0, 1] = np.inf
        _same(_run(dev, S, T, joint_score=float("inf")), assembly.walk_rule(S, T, joint_score=float("inf")))


@pytest.mark.parametrize("fill", (float("nan"), -1.0))
def test_mixed_counts(dev, fill):
    """Puzzles of 2 .. K pieces in one launch, two counts out of range; the padding holds NaN or -1 and is never read."""
    from puzzlenet_amd import assembly
    K = 33
    counts = np.array([33, 2, 17, 1, 34, 5, 0, -3, 32], dtype=np.int32)
    for kind in ("lattice", "nan30"):
        S, T, _ = wc.make(kind, len(counts), K, 600)
        for z, c in enumerate(counts):
            c = max(int(c), 0)
            S[z, c:, :], S[z, :, c:] = fill, fill
            T[z, c:, :], T[z, :, c:] = fill, fill
        want = assembly.walk_rule(S, T, count=counts)
        assert want.root[[3, 4, 6, 7]].tolist() == [-1] * 4 and (want.root[[0, 1, 2, 5, 8]] >= 0).all()
        _same(_run(dev, S, T, count=counts), want)


def test_more_puzzles_than_one_launch_holds(dev):
    from puzzlenet_amd import assembly
    n = IN_FLIGHT + 7
    S, T, _ = wc.make("lattice", n, 3, 700)
    S2, T2, _ = wc.make("random", n, 3, 701)
    S[::2], T[::2] = S2[::2], T2[::2]
    _same(_run(dev, S, T), assembly.walk_rule(S, T))


def test_two_runs_give_the_same_bits(dev):
    S, T, _ = wc.make("lattice", 64, 33, 800)
    a, b = _run(dev, S, T), _run(dev, S, T)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_assemble_batch_is_one_launch(dev):
    from puzzlenet_amd import assembly, ops
    K = 5
    S, T, _ = wc.make("random", Z, K, 900)
    s, t = torch.from_numpy(S).to(dev), torch.from_numpy(T).to(dev)
    real, calls = ops._call, []

    def spy(name, *a, **k):
        calls.append(name)
        return real(name, *a, **k)
    ops._call = spy
    try:
        asm = assembly.assemble_batch(s, t)
    finally:
        ops._call = real
    assert calls == ["pzn_assemble_walk_f32"]
    want = assembly.walk_rule(S, T)
    _same((asm.root, asm.edges, asm.edge_score, asm.n_edges, asm.G, asm.placed.to(torch.uint8), asm.joints, asm.n_joints), want)
    assert asm.placed.dtype == torch.bool and asm.movable.dtype == torch.bool
    movable = want.placed.astype(bool) & (np.arange(K)[None, :] != want.root[:, None])
    assert np.array_equal(asm.movable.cpu().numpy(), movable) and int(asm.movable.sum()) == Z * (K - 1)
    # a puzzle without a root has nothing movable
    none = assembly.assemble_batch(s, t, count=torch.tensor([1, K, K + 1, K, K], dtype=torch.int32, device=dev))
    assert none.root[[0, 2]].tolist() == [-1, -1] and not bool(none.movable[[0, 2]].any()) and not bool(none.placed[[0, 2]].any())


def test_argument_errors(dev):
    from puzzlenet_amd import _lib, ops
    S, T, _ = wc.make("random", 2, 4, 1000)
    s, t = torch.from_numpy(S).to(dev), torch.from_numpy(T).to(dev)
    with pytest.raises(_lib.PznError):
        ops.assemble_walk(s.cpu(), t)
    with pytest.raises(_lib.PznError):
        ops.assemble_walk(s.double(), t)
    with pytest.raises(_lib.PznError):
        ops.assemble_walk(s, t[:, :3])
    with pytest.raises(_lib.PznError):
        ops.assemble_walk(s[0], t[0])
    with pytest.raises(_lib.PznError):
        ops.assemble_walk(s, t, count=torch.zeros(2, dtype=torch.int64, device=dev))
    with pytest.raises(_lib.PznError):
        ops.assemble_walk(s, t, count=torch.zeros(3, dtype=torch.int32, device=dev))
    with pytest.raises(_lib.PznError):
        ops.assemble_walk(s, t, max_score=float("nan"))
    for K in (1, 65):
        with pytest.raises(_lib.PznUnsupported):
            ops.assemble_walk(torch.zeros(1, K, K, device=dev), torch.zeros(1, K, K, 4, 4, device=dev))
    assert ops.assemble_walk_supported(2) and ops.assemble_walk_supported(64) and not ops.assemble_walk_supported(65)
    empty = ops.assemble_walk(s[:0], t[:0])
    assert [tuple(x.shape) for x in empty] == [(0,), (0, 3, 3), (0, 3), (0,), (0, 4, 4, 4), (0, 4), (0, 12, 2), (0,)]
