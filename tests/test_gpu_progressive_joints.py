"""GPU: ops.progressive_joints (csrc/progjoints.hip, pzn_progressive_joints_f32) against its numpy statement
assembly.progressive_joints_rule, all seven outputs bit for bit; assembly.refine_progressive_batch on the planted puzzles of
tests/test_progressive_joints_cpu.py against the float64 loop of tests/_joint_ref.py; and the two launches behind the real
progressive walks (plumbing only: the closed-form weights' poses mean nothing).  The inputs are tests/_progressive_joints.py's."""
import numpy as np
import pytest
import torch

from oracle import model_ref as mr
from tests import _icp_ref as ref
from tests import _joint_counts as jc
from tests import _joint_ref as jr
from tests import _progressive_joints as pj

pytestmark = pytest.mark.gpu

SWEEPS = 30
# (Z, P, N, k): one entry a thread and less; k no multiple of 64; more than one entry a thread
SHAPES = [(3, 4, 64, 16), (2, 5, 96, 20), (2, 3, 400, 320)]
FILLS = (-1, 0, 0, 0, 0, -1, -1)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _device(dev, pieces, G, dropped):
    return (torch.from_numpy(np.ascontiguousarray(pieces)).to(dev), torch.from_numpy(np.ascontiguousarray(G)).to(dev),
            torch.from_numpy(np.ascontiguousarray(dropped)).to(dev))


def _check(dev, pieces, G, dropped, least):
    """The kernel's seven outputs equal the rule's -> the rule's."""
    from puzzlenet_amd import assembly, ops
    want = assembly.progressive_joints_rule(pieces, G, dropped, least)
    got = ops.progressive_joints(*_device(dev, pieces, G, dropped), least=least)
    assert len(got) == len(want) == 7
    for n, (x, y) in enumerate(zip(got, want)):
        y = torch.from_numpy(y)
        assert x.dtype == y.dtype and x.shape == y.shape, n
        assert torch.equal(x.cpu(), y), (n, int((x.cpu() != y).sum()))
    return want


@pytest.mark.parametrize("n", range(len(SHAPES)))
def test_kernel_is_the_rule_on_simulated_ledgers(dev, n):
    from puzzlenet_amd import ops
    Z, P, N, k = SHAPES[n]
    sim = pj.simulate(np.random.default_rng(6200 + n), Z, P, N, k)
    dropped = sim.dropped.copy()
    dropped[:, Z - 1] = -1                               # a puzzle that made no merge at all
    if Z > 2:
        dropped[-1, 0] = -1                              # a puzzle with no merge in its last round
    pad = dropped[:, :Z - 1, :, :, 0] == -1
    assert pad.any() and not pad.all() and (dropped[0, 0, :, :, 0] >= 0).any()      # -1 padding inside live lists
    for least in (1, 3):
        want = _check(dev, sim.pieces, sim.G, dropped, least)
        assert (want[0][:Z - 1, :, 0] >= 0).any() and (want[0][Z - 1] == -1).all()
    # the same bits on a second run
    args = _device(dev, sim.pieces, sim.G, dropped)
    one, two = ops.progressive_joints(*args, least=2), ops.progressive_joints(*args, least=2)
    assert all(torch.equal(x, y) for x, y in zip(one, two))
    # least above every count: no joint, every output at its fill value
    for x, fill in zip(ops.progressive_joints(*args, least=k + 1), FILLS):
        assert bool((x == fill).all())
    for x, fill in zip(_check(dev, sim.pieces, sim.G, dropped, k + 1), FILLS):
        assert (x == fill).all()


def test_kernel_is_the_rule_on_the_smallest_shape_and_on_exact_ties(dev):
    rng = np.random.default_rng(6300)
    pieces = rng.uniform(-1, 1, size=(1, 2, 8, 3)).astype(np.float32)
    G = np.stack([[ref.rigid(ref.rot(rng.normal(size=3), 0.3), rng.uniform(-0.1, 0.1, 3)) for _ in range(2)]])
    dropped = np.array([[[[[0, 5]], [[1, 2]]]]], dtype=np.int64)                   # [1,1,2,1,2]
    joints, a, b, na, nb, rows_a, rows_b = _check(dev, pieces, G, dropped, 1)
    assert joints.tolist() == [[[0, 1]]] and na.tolist() == nb.tolist() == [[1]] and rows_a.tolist() == [[[5]]]
    assert (_check(dev, pieces, G, dropped, 2)[0] == -1).all()
    pieces, G, dropped, want = pj.lattice()
    joints, a, b, na, nb, rows_a, rows_b = _check(dev, pieces, G, dropped, 3)
    n = len(want)
    assert rows_b[0, 1, :nb[0, 1]].tolist() == [y for y in range(n) if want[y] == 0]
    assert rows_b[0, 2, :nb[0, 2]].tolist() == [y for y in range(n) if want[y] == 1]
    # an all -1 ledger
    for x, fill in zip(_check(dev, pieces, G, np.full_like(dropped, -1), 1), FILLS):
        assert (x == fill).all()


def test_refused_before_any_launch(dev, monkeypatch):
    from puzzlenet_amd import _lib, assembly, ops
    calls = []
    monkeypatch.setattr(ops, "_call", lambda *a, **k: calls.append(a[0]))
    mk = lambda P, k, gt=torch.float64, dt=torch.int64: (torch.zeros(1, P, 8, 3, device=dev), torch.zeros(1, P, 4, 4, dtype=gt, device=dev),
                                                          torch.zeros(1, 1, 2, k, 2, dtype=dt, device=dev))
    for args in (mk(65, 4), mk(4, 1025), mk(1, 4)):
        with pytest.raises(_lib.PznUnsupported):
            ops.progressive_joints(*args)
    pieces, G, dropped = mk(4, 4)
    for bad in (lambda: ops.progressive_joints(*mk(4, 4, gt=torch.float32)),       # no silent conversion
                lambda: ops.progressive_joints(*mk(4, 4, dt=torch.int32)),
                lambda: ops.progressive_joints(pieces.double(), G, dropped),
                lambda: ops.progressive_joints(pieces, G, dropped, least=0),
                lambda: ops.progressive_joints(pieces, G[:, :3], dropped),
                lambda: ops.progressive_joints(pieces, G, dropped[:, :, :1])):
        with pytest.raises(_lib.PznError) as info:
            bad()
        assert not isinstance(info.value, _lib.PznUnsupported)
    # the refinement: a walk without dropped rows says why; limits before any tensor is touched
    res = assembly.ProgressiveBatchResult(G, None, None, None, None, None, torch.zeros(1, 4, dtype=torch.int32, device=dev), None,
                                          None, None, None, None)
    with pytest.raises(_lib.PznError, match="drop_matched"):
        assembly.refine_progressive_batch(pieces, res)
    p65, g65, d65 = mk(65, 4)
    with pytest.raises(_lib.PznUnsupported):
        assembly.refine_progressive_batch(p65, res._replace(G=g65, part=torch.zeros(1, 65, dtype=torch.int32, device=dev), dropped=d65))
    with pytest.raises(_lib.PznUnsupported):
        assembly.refine_progressive_batch(pieces, res._replace(dropped=mk(4, 1025)[2]))
    assert calls == []
    assert len(ops.progressive_joints(*mk(4, 4))) == 7 and calls == ["pzn_progressive_joints_f32"]
    # no puzzles: a success that launches nothing
    out = ops.progressive_joints(pieces[:0], G[:0], dropped[:, :0])
    assert out[0].shape == (0, 6, 2) and len(calls) == 1


# --------------------------------------------------------------------------- refine_progressive_batch on the planted puzzles

def _stacked(K, m=pj.M):
    """The eight planted puzzles of K pieces as one batch: the pieces padded to one N with the far point no list names."""
    cases = [pj.planted(K, seed, m=m) for k_, seed in pj.CASES if k_ == K]
    N = max(pl.N for pl in cases)
    pieces = np.full((len(cases), K, N, 3), 50.0, dtype=np.float32)
    for z, pl in enumerate(cases):
        pieces[z, :, :pl.N] = pl.pieces
    G = np.stack([pl.G0 for pl in cases])
    dropped = np.stack([pl.dropped for pl in cases], axis=1)
    part = np.stack([pl.part for pl in cases])
    return cases, pieces, G, dropped, part


@pytest.fixture(scope="module")
def trajectory_tolerance():
    """tests/test_gpu_joint_counts.py's bound for trajectories: STEP_FACTOR x the largest error of the float32 restatement of a
    visit over the cases of tests/_joint_counts.visit_cases whose optimum is unique."""
    rows = [jc.visit_row(P) for graph in jc.VISIT_GRAPHS for P in jc.visit_cases(graph)]
    return jc.STEP_FACTOR * max(yard for _, yard, _, gap in rows if gap >= jc.GAP_MIN)


@pytest.mark.parametrize("K", [4, 6, 8])
def test_refine_progressive_batch_on_planted_puzzles(dev, K, trajectory_tolerance):
    from puzzlenet_amd import assembly, ops
    cases, pieces, G, dropped, part = _stacked(K)
    Z = len(cases)
    pd, Gd, dd = _device(dev, pieces, G, dropped)
    res = assembly.ProgressiveBatchResult(Gd, None, None, None, torch.zeros(Z, dtype=torch.int32, device=dev),
                                          torch.ones(Z, K, dtype=torch.bool, device=dev), torch.from_numpy(part).to(dev), None, None,
                                          None, None, dd)
    out = assembly.refine_progressive_batch(pd, res, sweeps=SWEEPS, least=3)
    assert isinstance(out, assembly.ProgressiveJointRefined)
    J = K * (K - 1) // 2
    assert out.G.shape == (Z, K, 4, 4) and out.G.dtype == torch.float32 and out.joints.shape == (Z, J, 2)
    assert out.joint_score.shape == out.count_f.shape == out.count_m.shape == (Z, J) and out.rows_f.shape == (Z, J, 4 * pj.M)
    assert bool((out.score <= out.score0).all())
    G0 = Gd.float()
    assert torch.equal(out.G[:, 0], G0[:, 0]) and int(out.accepted[:, 0].abs().max()) == 0        # the frame piece keeps G0's bits
    got = out.G.cpu().numpy()
    for z, pl in enumerate(cases):
        assert sorted((min(i, j), max(i, j)) for i, j in out.joints[z].cpu().tolist() if i >= 0) == sorted(pl.contacts)
        before = jr.pose_error(jr.f32(pl.G0.astype(np.float32)), pl.truth)
        after = jr.pose_error(got[z], pl.truth)
        print(f"K = {K} seed {z}: score {float(out.score0[z]):.3e} -> {float(out.score[z]):.3e}, pose error per piece "
              f"{np.round(before[1:], 4).tolist()} -> {np.round(after[1:], 4).tolist()}")
        assert (after[1:] < before[1:]).all(), (K, z, before, after)
    # the float64 loop: tests/test_gpu_joint_counts.py's trajectory check, with its margin rule and its tolerance, on these
    # puzzles (the rule leaves all of them out) and on the ones of SHORT_M points a contact (tests/_progressive_joints.py)
    entered = {}
    for m in (pj.M, pj.SHORT_M):
        cases, pieces, G, dropped, part = _stacked(K, m)
        pd, Gd, dd = _device(dev, pieces, G, dropped)
        short = assembly.refine_progressive_batch(pd, res._replace(G=Gd, dropped=dd), sweeps=jc.TRAJECTORY_SWEEPS, least=3)
        outputs = [x.cpu().numpy() for x in (short.joints, ) + ops.progressive_joints(pd, Gd, dd, 3)[1:]]
        short_G, short_acc, short_used = short.G.cpu().numpy(), short.accepted.cpu().numpy(), short.sweeps_used.cpu().numpy()
        entered[m] = 0
        for z, pl in enumerate(cases):
            mine = [x[z:z + 1] for x in outputs]
            want, enters = pj.short_trajectory(pl, mine, jc.TRAJECTORY_SWEEPS, jc.MARGIN_FACTOR)
            if not enters:
                continue
            entered[m] += 1
            assert short_acc[z].tolist() == want.accepted.tolist() and int(short_used[z]) == want.sweeps_used, (K, m, z)
            err = max(ref.pose_err(short_G[z, p], want.G[p]) for p in range(K))
            assert err <= trajectory_tolerance, (K, m, z, err, trajectory_tolerance)
    print(f"K = {K}: {entered} of {Z} puzzles entered the trajectory check (tolerance {trajectory_tolerance:.3e})")
    assert entered[pj.SHORT_M] >= Z // 2


def test_unplaced_pieces_and_frame_pieces_keep_their_bits(dev):
    """Two parts and a single piece in one puzzle: the planted puzzle of 4 pieces in slots 0..3 and again in slots 4..7, its frame
    piece in slot 4, and slot 8 a piece nothing names."""
    from puzzlenet_amd import assembly
    pl = pj.planted(4, 0)
    K, P = pl.K, 2 * pl.K + 1
    pieces = np.full((1, P, pl.N, 3), 50.0, dtype=np.float32)
    pieces[0, :K], pieces[0, K:2 * K] = pl.pieces, pl.pieces
    G = np.tile(np.eye(4), (1, P, 1, 1))
    G[0, :K], G[0, K:2 * K] = pl.G0, pl.G0
    dropped = np.full((2 * (K - 1), 1, 2, pl.k, 2), -1, dtype=np.int64)
    dropped[:K - 1, 0] = pl.dropped
    second = pl.dropped.copy()
    second[..., 0] = np.where(second[..., 0] >= 0, second[..., 0] + K, -1)
    dropped[K - 1:, 0] = second
    part = np.array([[0] * K + [K] * K + [P - 1]], dtype=np.int32)
    pd, Gd, dd = _device(dev, pieces, G, dropped)
    res = assembly.ProgressiveBatchResult(Gd, None, None, None, None, None, torch.from_numpy(part).to(dev), None, None, None, None, dd)
    out = assembly.refine_progressive_batch(pd, res, sweeps=SWEEPS)
    one = assembly.refine_progressive_batch(pd[:, :K].contiguous(), res._replace(G=Gd[:, :K].contiguous(), part=res.part[:, :K].contiguous(),
                                                                                  dropped=dd[:K - 1].contiguous()), sweeps=SWEEPS)
    G0 = Gd.float()
    for p in (0, K, P - 1):
        assert torch.equal(out.G[0, p], G0[0, p]) and int(out.accepted[0, p]) == 0
    assert int(out.accepted[0, 1:K].min()) > 0 and int(out.accepted[0, K + 1:2 * K].min()) > 0
    # no joint between the parts, and each part moves as it does alone
    joints = out.joints[0].cpu().tolist()
    assert all((i < K) == (j < K) and P - 1 not in (i, j) for i, j in joints if i >= 0)
    assert torch.equal(out.G[0, :K], one.G[0]) and torch.equal(out.G[0, K:2 * K, :, :], one.G[0])


# --------------------------------------------------------------------------- through the real walks

K_W, N_W, TOP_W = 4, 1024, 128                  # tests/test_gpu_progressive.py's shape, its smallest


@pytest.fixture(scope="module")
def walks(dev):
    from puzzlenet_amd import assembly
    from puzzlenet_amd import model5_b as mb
    model = mb.TouchedRegraster(mr.Cfg())
    mr.fill_params(model)
    model.to(dev)
    g = torch.Generator().manual_seed(1618)
    pieces = torch.rand(2, K_W, N_W, 3, generator=g).to(dev)
    start = (torch.randint(0, N_W, (2, K_W), generator=g), torch.randint(0, 512, (2, K_W), generator=g))
    asm = assembly.ProgressiveAssembler(model, pieces[0], k=TOP_W, start=(start[0][0], start[1][0]), generator=torch.Generator().manual_seed(7))
    prog = asm.run()
    merge_starts = torch.tensor([asm.merge_starts, asm.merge_starts], dtype=torch.long)
    batch = assembly.assemble_progressive_batch(model, pieces, k=TOP_W, start=start, merge_starts=merge_starts)
    return pieces, prog, batch


def test_through_the_real_walks(dev, walks):
    from puzzlenet_amd import assembly, ops
    pieces, prog, batch = walks
    Z, P = 2, K_W
    J = P * (P - 1) // 2
    out = assembly.refine_progressive_batch(pieces, batch, sweeps=SWEEPS)
    # joints only between pieces that some edge put on opposite sides
    part = np.tile(np.arange(P), (Z, 1))
    opposite = [set() for _ in range(Z)]
    edges, n_edges = batch.edges.cpu().numpy(), batch.n_edges.cpu().numpy()
    for z in range(Z):
        for _, _, i, j in edges[z, :n_edges[z]]:
            opposite[z] |= {(p, q) for p in np.flatnonzero(part[z] == i) for q in np.flatnonzero(part[z] == j)}
            part[z][part[z] == j] = i
        assert np.array_equal(part[z], batch.part[z].cpu().numpy())
        listed = [(i, j) for i, j in out.joints[z].cpu().tolist() if i >= 0]
        assert listed and all((i, j) in opposite[z] for i, j in listed), (z, listed, opposite[z])
    # the two launches, reproduced exactly
    joints, a, b, na, nb, rows_a, rows_b = ops.progressive_joints(pieces, batch.G, batch.dropped, 3)
    k = batch.dropped.shape[3]
    G, score, score0, joint_score, used, accepted = ops.joint_refine(
        a.view(Z * J, k, 3), b.view(Z * J, k, 3), joints, batch.G.float(), batch.part != torch.arange(P, device=dev)[None], SWEEPS,
        na=na.view(-1), nb=nb.view(-1))
    for x, y in zip(out, (G, score, score0, used, accepted, joints, joint_score, na, nb, rows_a, rows_b)):
        assert torch.equal(x, y)
    assert bool((out.score <= out.score0).all())
    movable = batch.part != torch.arange(P, device=dev)[None]
    assert torch.equal(out.G[~movable], batch.G.float()[~movable])
    # the kernel is the rule on a real ledger, too
    want = assembly.progressive_joints_rule(pieces, batch.G, batch.dropped, 3)
    for x, y in zip((joints, a, b, na, nb, rows_a, rows_b), want):
        assert torch.equal(x.cpu(), torch.from_numpy(y))
    # it goes through evaluate_batch as it is
    pose = torch.eye(4, dtype=torch.float64, device=dev).repeat(Z, P, 1, 1)
    assembly.evaluate_batch(out.G, batch.placed, pose, pieces, batch.root, batch.edges, batch.n_edges)


def test_refine_progressive_is_the_batched_call_at_z_1(dev, walks):
    from puzzlenet_amd import assembly
    pieces, prog, batch = walks
    # the two walks of puzzle 0 made the same merges (their poses and, after the first round, their merged parts and so the rows
    # they left out differ in the last bits of the few-row layers, as tests/test_gpu_progressive_batch.py says)
    n = int(batch.n_edges[0])
    assert n == len(prog.edges) == K_W - 1
    assert [tuple(e[:2]) for e in prog.edges] == [tuple(r[:2]) for r in batch.edges[0, :n].cpu().tolist()]
    own = torch.stack([torch.stack((e[3], e[4]), dim=0) for e in prog.edges], dim=0)
    assert own.shape == batch.dropped[:, 0].shape
    single = assembly.refine_progressive(pieces[0], prog, sweeps=SWEEPS)
    # the batched call at Z = 1 on the per-puzzle walk's own poses and rows, with the batched walk's part (the frame pieces the
    # device booked, which the per-puzzle form rebuilds on the host from the edge labels)
    res = assembly.ProgressiveBatchResult(torch.from_numpy(prog.G)[None].to(dev), None, None, None, None, None, batch.part[:1].contiguous(),
                                          None, None, None, None, own[:, None].contiguous())
    both = assembly.refine_progressive_batch(pieces[:1].contiguous(), res, sweeps=SWEEPS)
    assert isinstance(single, assembly.ProgressiveJointRefined)
    for name, x, y in zip(single._fields, single, both):
        assert x.shape == y.shape[1:] and torch.equal(x, y[0]), name
    with pytest.raises(assembly._lib.PznError, match="drop_matched"):
        assembly.refine_progressive(pieces[0], prog._replace(edges=[e[:3] + (None, None) for e in prog.edges]))
