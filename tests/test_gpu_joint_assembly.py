"""GPU: assembly.refine_assembly - the placed poses of a greedy assembly refined jointly over every joint (one gather, one
launch of ops.joint_refine) - on the closed-form model of tests/test_gpu_assembly.py and on a hand-made ring whose loop the
greedy walk cannot close.  The kernel itself is held to float64 in tests/test_gpu_joint_refine.py.

match_pairs is not repeatable bit for bit from call to call (tests/test_gpu_assembly_refine.py says why), so "the same bits
as without the call" is checked on ONE table: its tensors, the walk over it and refine_pairs on it before and after."""
import numpy as np
import pytest
import torch

from oracle import model_ref as mr
from tests import _icp_ref as ref
from tests import _joint_ref as jr

pytestmark = pytest.mark.gpu

K, N, TOP = 5, 1024, 128
STEP_FACTOR = 4.0
MARGIN_FACTOR = 16.0
RING_K, RING_N, RING_TOP, RING_CASES = 4, 64, 32, 12
RING = [(0, 1), (1, 2), (2, 3), (3, 0)]


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
def table(dev, model):
    from puzzlenet_amd import assembly
    g = torch.Generator().manual_seed(2719)
    assert model.num_points == N
    pieces = torch.rand(K, N, 3, generator=g).to(dev)
    start = (torch.randint(0, N, (K,), generator=g), torch.randint(0, 512, (K,), generator=g))
    return pieces, assembly.match_pairs(model, pieces, k=TOP, start=start)


def _f32(G):
    return np.asarray(G, dtype=np.float64).astype(np.float32)


def test_refine_assembly_on_a_random_table(dev, table):
    from puzzlenet_amd import assembly, ops
    pieces, t = table
    asm = assembly.assemble(t.score, t.T)
    assert asm.placed.all()
    before = [x.clone() for x in (pieces,) + tuple(t)]
    pairs_before = assembly.refine_pairs(pieces, t.top_f, pieces, t.top_m, t.T, 5)
    real, calls = ops._call, []

    def spy(name, *a, **k):
        calls.append(name)
        return real(name, *a, **k)
    ops._call = spy
    try:
        out = assembly.refine_assembly(pieces, t, asm)
    finally:
        ops._call = real
    assert calls == ["pzn_gather_fwd_f32", "pzn_joint_refine_f32"]                    # one gather and one launch
    G = out.G.cpu().numpy()
    assert np.array_equal(G[asm.root], _f32(asm.G[asm.root])) and int(out.accepted[asm.root]) == 0
    assert float(out.score) <= float(out.score0) and out.G.dtype == torch.float32 and out.G.shape == (K, 4, 4)
    assert all((i, j) in out.joints for i, j, _, _ in asm.edges)                      # every tree edge is a joint
    S = t.score.cpu().numpy()
    worst = max(e[2] for e in asm.edges)
    assert out.joints == [(i, j) for i in range(K) for j in range(K) if i != j and S[i, j] <= worst]
    print(f"{len(out.joints)} joints of {K * (K - 1)}; score {float(out.score):.6f} from {float(out.score0):.6f}, "
          f"{int(out.sweeps_used)} sweeps, accepted {out.accepted.tolist()}")
    # sweeps = 0 gives asm.G
    zero = assembly.refine_assembly(pieces, t, asm, sweeps=0)
    assert np.array_equal(zero.G.cpu().numpy(), _f32(asm.G)) and float(zero.score) == float(zero.score0) == float(out.score0)
    assert int(zero.sweeps_used) == 0 and int(zero.accepted.abs().max()) == 0
    # the first edge alone: its joint energy under asm.G is the table's score of that pair (the same sets, a composed pose)
    i0, j0, s0, _ = asm.edges[0]
    first = assembly.refine_assembly(pieces, t, asm, sweeps=0, joint_score=s0)
    assert first.joints == [(i0, j0)]
    np.testing.assert_allclose(float(first.score0), s0, rtol=1e-4)
    # every ordered pair
    full = assembly.refine_assembly(pieces, t, asm, joint_score=float("inf"))
    assert len(full.joints) == K * (K - 1) and float(full.score) <= float(full.score0)
    # nothing it was given has changed, and the functions beside it answer as before
    assert all(torch.equal(x, y) for x, y in zip(before, (pieces,) + tuple(t)))
    again = assembly.assemble(t.score, t.T)
    assert again.root == asm.root and again.edges == asm.edges and np.array_equal(again.G, asm.G)
    assert all(torch.equal(x, y) for x, y in zip(pairs_before, assembly.refine_pairs(pieces, t.top_f, pieces, t.top_m, t.T, 5)))


def test_unplaced_pieces_keep_the_identity(dev, table):
    from puzzlenet_amd import assembly
    pieces, t = table
    whole = assembly.assemble(t.score, t.T)
    asm = assembly.assemble(t.score, t.T, max_score=whole.edges[0][2])                # the walk stops after its first edge
    assert (~asm.placed).sum() == K - 2
    out = assembly.refine_assembly(pieces, t, asm)
    G = out.G.cpu().numpy()
    for p in range(K):
        if not asm.placed[p]:
            assert np.array_equal(G[p], np.eye(4, dtype=np.float32)) and int(out.accepted[p]) == 0
            assert all(p not in e for e in out.joints)
    assert np.array_equal(G[asm.root], _f32(asm.G[asm.root])) and float(out.score) <= float(out.score0)
    assert all((i, j) in out.joints for i, j, _, _ in asm.edges)
    # an assembly without an edge has no joint: asm.G comes back and nothing is launched for it
    none = assembly.refine_assembly(pieces, t, assembly.assemble(t.score, t.T, max_score=-1.0))
    assert none.joints == [] and np.array_equal(none.G.cpu().numpy(), np.tile(np.eye(4, dtype=np.float32), (K, 1, 1)))
    assert float(none.score) == 0 and float(none.score0) == 0


def test_refine_assembly_argument_errors(dev, table):
    from puzzlenet_amd import _lib, assembly
    pieces, t = table
    asm = assembly.assemble(t.score, t.T)
    with pytest.raises(_lib.PznError):
        assembly.refine_assembly(pieces.cpu(), t, asm)
    with pytest.raises(_lib.PznError):
        assembly.refine_assembly(pieces[:4], t, asm)
    with pytest.raises(_lib.PznUnsupported):
        assembly.refine_assembly(pieces, t, asm, sweeps=-1)


# --------------------------------------------------------------------------- loop closure on a hand-made table

def _ring_case(seed, dev):
    """Four pieces in a ring, each the moved piece of exactly one joint (0->1->2->3->0).  Joint (i, j) is RING_TOP points of a
    closed curve that both pieces hold: piece i in its rows 0..31 (top_f[i,j]), piece j in its rows 32..63 in another order
    (top_m[j]).  T[i,j] is the true relative pose perturbed by up to 2 degrees and 0.005 per axis; the score is the table's
    formula in float64 -> (pieces, PairTable with the fields refine_assembly reads, truth [4,4,4])."""
    from puzzlenet_amd import assembly
    rng = np.random.default_rng(seed)
    truth = np.stack([ref.rigid(ref.rot(rng.normal(size=3), rng.uniform(0.3, 2.5)), rng.uniform(-0.3, 0.3, 3)) for _ in range(RING_K)])
    pieces = np.zeros((RING_K, RING_N, 3))
    for e, (i, j) in enumerate(RING):
        world = ref.curve(rng.uniform(0, 1, RING_TOP), bool(e & 1)) @ ref.rot(rng.normal(size=3), rng.uniform(0, np.pi)).T \
            + rng.uniform(-0.5, 0.5, 3)
        pieces[i, :RING_TOP] = ref.transform(jr._inverse(truth[i]), world)
        pieces[j, RING_TOP:] = ref.transform(jr._inverse(truth[j]), world[rng.permutation(RING_TOP)])
    pieces = pieces.astype(np.float32)
    top_f = np.tile(np.arange(RING_TOP), (RING_K, RING_K, 1))
    top_m = np.tile(RING_TOP + np.arange(RING_TOP), (RING_K, 1))
    T = np.tile(np.eye(4), (RING_K, RING_K, 1, 1))
    S = np.full((RING_K, RING_K), np.inf)
    for i, j in RING:
        c = ref.transform(truth[i], pieces[i, :RING_TOP]).mean(axis=0)              # the joint's centre, in the world
        Rp = ref.rot(rng.normal(size=3), rng.uniform(-1, 1) * np.deg2rad(2.0))
        Pm = ref.rigid(Rp, c - Rp @ c + rng.uniform(-0.005, 0.005, 3))
        T[i, j] = (jr._inverse(truth[i]) @ Pm @ truth[j]).astype(np.float32)
        S[i, j] = ref.objective(pieces[i, :RING_TOP], pieces[j, RING_TOP:], T[i, j])[0]
    t = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x)).to(dev, dt)
    table = assembly.PairTable(None, t(T, torch.float32), None, None, t(top_f, torch.long), t(top_m, torch.long),
                               t(S, torch.float32), None)
    return t(pieces, torch.float32), table, truth


def test_ring_of_four_closes_its_loop(dev):
    from puzzlenet_amd import assembly
    cases = []
    for n in range(RING_CASES):
        pieces, table, truth = _ring_case(7300 + n, dev)
        asm = assembly.assemble(table.score, table.T)
        assert asm.placed.all() and len(asm.edges) == 3
        worst = float(table.score[torch.isfinite(table.score)].max())
        two = assembly.refine_assembly(pieces, table, asm, sweeps=2, joint_score=worst)
        full = assembly.refine_assembly(pieces, table, asm, sweeps=30, joint_score=worst)
        assert two.joints == sorted(RING) and full.joints == two.joints                # the tree's three edges and the loop's
        assert float(two.score) <= float(two.score0) and float(full.score) <= float(full.score0)      # exactly
        assert float(full.score0) == float(two.score0)
        # the same problem for the float64 loop: poses and truth in the root's frame
        p = pieces.cpu().numpy()
        movable = np.arange(RING_K) != asm.root
        P = jr.Puzzle(RING_K, two.joints, [p[i, :RING_TOP] for i, _ in two.joints], [p[j, RING_TOP:] for _, j in two.joints],
                      _f32(asm.G), np.stack([jr._inverse(truth[asm.root]) @ truth[q] for q in range(RING_K)]), movable)
        cases.append((P, two, full, jr.refine(P, 2), jr.refine(P, 30)))
    yard = max(ref.pose_err(jr.visit_f32(P, P.G0, q, jr.piece_energy(P, jr.f32(P.G0), q)[1]), jr.visit(P, jr.f32(P.G0), q, round32=False))
               for P, *_ in cases for q in range(RING_K) if P.movable[q])
    tol = STEP_FACTOR * yard
    left_out = 0
    for n, (P, two, full, want2, want30) in enumerate(cases):
        e0 = jr.pose_error(P.G0, P.truth)
        e2, e30 = jr.pose_error(two.G.cpu().numpy(), P.truth), jr.pose_error(full.G.cpu().numpy(), P.truth)
        w2, w30 = jr.pose_error(want2.G, P.truth), jr.pose_error(want30.G, P.truth)
        fmt = lambda v: " ".join(f"{x:.2e}" for x in v)
        print(f"case {n}: pose error per piece, walk {fmt(e0)} | 2 sweeps {fmt(e2)} (float64 loop {fmt(w2)}) | 30 sweeps {fmt(e30)} "
              f"(float64 loop {fmt(w30)}); score {float(full.score0):.3e} -> {float(two.score):.3e} -> {float(full.score):.3e} "
              f"(float64 loop {want30.score0:.3e} -> {want2.score:.3e} -> {want30.score:.3e}), sweeps used {int(full.sweeps_used)} "
              f"({want30.sweeps_used})")
        if want2.margin_ratio < MARGIN_FACTOR:
            left_out += 1
            continue
        assert two.accepted.tolist() == want2.accepted.tolist() and int(two.sweeps_used) == want2.sweeps_used, n
        assert max(ref.pose_err(two.G[q].cpu().numpy(), want2.G[q]) for q in range(RING_K)) <= tol, n
        if w2.max() < e0.max():                      # where the float64 loop ends nearer the truth, so does the device
            assert e2.max() < e0.max(), n
    print(f"left out {left_out} of {len(cases)}; tolerance {tol:.3e}")
    # with 32 points a side most float64 loops meet a margin below 16 bounds in one of their 256 rows; the seeds above leave
    # three loops that do not (the CPU side alone decides this)
    assert len(cases) - left_out == 3
