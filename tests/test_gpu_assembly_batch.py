"""GPU: the batched assembly chain - assembly.match_puzzles, assemble_batch, refine_assembly_batch, evaluate_batch - against the
per-puzzle functions it stands beside (match_pairs, walk_rule / assemble, refine_assembly, evaluate), with the closed-form model
of tests/test_gpu_assembly.py.  The walk kernel itself is held to its rule in tests/test_gpu_assemble_walk.py.

match_puzzles against match_pairs: two calls of match_pairs are not equal bit for bit either (the few-row layers sum their
K-splits in fp32 atomics, tests/test_gpu_assembly_refine.py), so the whole table cannot be asserted bit-equal across batch
compositions.  x2 (coordinates only) is; twist and the two logit fields are held to the tolerances tests/test_gpu_assembly.py
holds match_pairs itself to; the picks and the score are checked against the table's OWN logits, picks and poses, where nothing
is noisy."""
import numpy as np
import pytest
import torch

from oracle import model_ref as mr
from tests import _fracture as fr

pytestmark = pytest.mark.gpu

Z, P, N, TOP = 3, 3, 1024, 128
FB, FM, FP, FK, Fn, Fk = 3, 4096, 4, 8, 256, 32      # the fracture batch: clouds, points, pieces, candidates, n, k
TOL = 0.01


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
def batch(dev, model):
    """Z puzzles of P seeded pieces, their batched table, the per-puzzle tables with the same starts, the batched walk and its
    rule; computed once."""
    from puzzlenet_amd import assembly
    g = torch.Generator().manual_seed(3141)
    assert model.num_points == N
    pieces = torch.rand(Z, P, N, 3, generator=g).to(dev)
    s1, s2 = torch.randint(0, N, (Z, P), generator=g), torch.randint(0, 512, (Z, P), generator=g)
    table = assembly.match_puzzles(model, pieces, k=TOP, start=(s1, s2))
    singles = [assembly.match_pairs(model, pieces[z], k=TOP, start=(s1[z], s2[z])) for z in range(Z)]
    asm = assembly.assemble_batch(table.score, table.T)
    rule = assembly.walk_rule(table.score, table.T)
    return dict(pieces=pieces, table=table, singles=singles, asm=asm, rule=rule)


def _close(got, want, rtol, atol, msg):
    np.testing.assert_allclose(got.detach().cpu().numpy(), want.detach().cpu().numpy(), rtol=rtol, atol=atol, err_msg=msg)


def test_match_puzzles_against_match_pairs(batch):
    from puzzlenet_amd import ops, se3
    t, pieces = batch["table"], batch["pieces"]
    assert t.twist.shape == (Z, P, P, 6) and t.T.shape == (Z, P, P, 4, 4) and t.de_fpcb.shape == (Z, P, P, 2, N)
    assert t.de_mrpcb.shape == (Z, P, 2, N) and t.top_f.shape == (Z, P, P, TOP) and t.top_m.shape == (Z, P, TOP)
    assert t.score.shape == (Z, P, P) and t.x2.shape == (Z, P, 256, 3) and t.top_f.dtype == torch.int64
    eye = torch.eye(P, dtype=torch.bool, device=pieces.device)
    for z, one in enumerate(batch["singles"]):
        assert torch.equal(t.x2[z], one.x2)                                      # the same 256 points, bit for bit
        _close(t.twist[z], one.twist, 1e-4, 1e-5, "twist")
        _close(t.de_fpcb[z], one.de_fpcb, 1e-4, 1e-4, "de_fpcb")
        _close(t.de_mrpcb[z], one.de_mrpcb, 1e-4, 1e-4, "de_mrpcb")
        # the picks are the top k of its own logits, by the same calls
        y_f = t.de_fpcb[z].permute(0, 1, 3, 2).contiguous()                      # [P,P,N,2], the kernel's layout
        assert torch.equal(t.top_f[z], ops.topk_rows(torch.softmax(y_f, dim=-1)[..., 1].reshape(P * P, N), TOP).view(P, P, TOP))
        y_m = t.de_mrpcb[z].permute(0, 2, 1).contiguous()
        assert torch.equal(t.top_m[z], ops.topk_rows(torch.softmax(y_m, dim=-1)[..., 1], TOP))
        # T is se3.exp of its own twist and the score the chamfer of its own picks under its own T, bit for bit
        assert torch.equal(t.T[z], se3.exp(t.twist[z]))
        Bf = ops.index_points(pieces[z], t.top_f[z].reshape(P, P * TOP)).view(P * P, TOP, 3)
        Bm = ops.index_points(pieces[z], t.top_m[z]).unsqueeze(0).expand(P, -1, -1, -1).reshape(P * P, TOP, 3)
        d1, d2 = ops.chamfer(Bf, se3.transform_points(t.T[z].reshape(P * P, 4, 4), Bm))
        want = (d1.mean(dim=1) + d2.mean(dim=1)).view(P, P).masked_fill(eye, float("inf"))
        assert torch.equal(t.score[z], want)


def test_match_puzzles_encodes_full_batches(dev, model, batch):
    """One encode_pieces for all Z P pieces: fewer library launches than Z calls of match_pairs."""
    from puzzlenet_amd import assembly, ops
    real, calls = ops._call, []

    def spy(name, *a, **k):
        calls.append(name)
        return real(name, *a, **k)
    ops._call = spy
    try:
        assembly.match_puzzles(model, batch["pieces"], k=TOP)
        n_batch = len(calls)
        del calls[:]
        assembly.match_pairs(model, batch["pieces"][0], k=TOP)
        n_one = len(calls)
    finally:
        ops._call = real
    print(f"library launches: match_puzzles of {Z} puzzles {n_batch}, match_pairs of one {n_one}")
    assert n_batch < Z * n_one                                                    # the encoders' launches are shared
    with pytest.raises(assembly._lib.PznError):
        assembly.match_puzzles(model, batch["pieces"][0], k=TOP)
    with pytest.raises(assembly._lib.PznError):
        assembly.match_puzzles(model, batch["pieces"].cpu(), k=TOP)
    with pytest.raises(assembly._lib.PznError):
        assembly.match_puzzles(model, batch["pieces"], k=TOP, start=(torch.zeros(Z * P, dtype=torch.long),) * 2)


def _assembly_of(rule, z):
    """assemble's Assembly from walk_rule's fields of puzzle z."""
    from puzzlenet_amd import assembly
    n = int(rule.n_edges[z])
    edges = [(int(i), int(j), float(s), int(new)) for (i, j, new), s in zip(rule.edges[z, :n], rule.edge_score[z, :n])]
    return assembly.Assembly(int(rule.root[z]), edges, rule.G[z], rule.placed[z].astype(bool))


def _sub(table, z):
    from puzzlenet_amd import assembly
    return assembly.PairTable(*(f[z] for f in table))


@pytest.mark.parametrize("joint_score", (None, float("inf")))
def test_refine_assembly_batch_against_refine_assembly(dev, batch, joint_score):
    from puzzlenet_amd import assembly, ops
    pieces, t = batch["pieces"], batch["table"]
    if joint_score is None:
        asm, rule = batch["asm"], batch["rule"]
    else:
        asm, rule = assembly.assemble_batch(t.score, t.T, joint_score=joint_score), assembly.walk_rule(t.score, t.T, joint_score=joint_score)
    assert torch.equal(asm.joints.cpu(), torch.from_numpy(rule.joints)) and torch.equal(asm.G.cpu(), torch.from_numpy(rule.G))
    real, calls = ops._call, []

    def spy(name, *a, **k):
        calls.append(name)
        return real(name, *a, **k)
    ops._call = spy
    try:
        out = assembly.refine_assembly_batch(pieces, t, asm, sweeps=30)
    finally:
        ops._call = real
    assert calls == ["pzn_gather_fwd_f32", "pzn_joint_refine_f32"]                # one gather and one launch, Z puzzles
    assert out.G.shape == (Z, P, 4, 4) and out.G.dtype == torch.float32 and out.joints is asm.joints
    zero = assembly.refine_assembly_batch(pieces, t, asm, sweeps=0)
    assert torch.equal(zero.G, asm.G.to(torch.float32)) and torch.equal(zero.score, zero.score0)
    assert torch.equal(zero.score0, out.score0) and int(zero.accepted.abs().max()) == 0
    assert bool((out.score <= out.score0).all())
    moved = 0
    for z in range(Z):
        one = assembly.refine_assembly(pieces[z], _sub(t, z), _assembly_of(rule, z), sweeps=30, joint_score=joint_score)
        n = int(rule.n_joints[z])
        assert one.joints == [tuple(int(v) for v in r) for r in rule.joints[z, :n]] and n > 0
        assert torch.equal(out.G[z], one.G) and torch.equal(out.score[z], one.score) and torch.equal(out.score0[z], one.score0)
        assert torch.equal(out.accepted[z], one.accepted) and torch.equal(out.sweeps_used[z], one.sweeps_used)
        moved += int(one.accepted.sum())
    assert moved > 0                                                              # some pose did move


def test_refine_assembly_batch_argument_errors(dev, batch):
    from puzzlenet_amd import _lib, assembly
    pieces, t, asm = batch["pieces"], batch["table"], batch["asm"]
    with pytest.raises(_lib.PznError):
        assembly.refine_assembly_batch(pieces.cpu(), t, asm)
    with pytest.raises(_lib.PznError):
        assembly.refine_assembly_batch(pieces[:2], t, asm)
    with pytest.raises(_lib.PznUnsupported):
        assembly.refine_assembly_batch(pieces, t, asm, sweeps=-1)


# --------------------------------------------------------------------------- evaluation on a fracture batch

@pytest.fixture(scope="module")
def fracture(dev):
    from puzzlenet_amd import datapipe
    raw = fr.clouds(FB, FM, 40)
    normals, u_anchor, u_start, twist = fr.draws(FB, FP, FK, 41)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return datapipe.fracture(to(raw), to(normals), to(u_anchor), to(u_start), to(twist), n=Fn, k=Fk)


def _inv(X):
    out = np.eye(4)
    out[:3, :3] = X[:3, :3].T
    out[:3, 3] = -X[:3, :3].T @ X[:3, 3]
    return out


def _nudge(rng, deg, shift):
    """A rigid motion of `deg` degrees about a random axis and a translation of length `shift`."""
    w = rng.normal(size=3)
    w /= np.linalg.norm(w)
    th = np.deg2rad(deg)
    Kx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    out = np.eye(4)
    out[:3, :3] = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)
    v = rng.normal(size=3)
    out[:3, 3] = shift * v / np.linalg.norm(v)
    return out


def test_evaluate_batch_against_evaluate(dev, fracture):
    """Every pose is the truth times a nudge - 1 degree and 0.02 (msd about 4e-4, far below tol) or 25 degrees and 0.3 (far
    above) -, the root's included: no error is a difference of nearly equal numbers, so float64 on both sides agrees to about
    n 2^-53 relative (sums of n = 256 terms) and the atan2 argument has norm 2."""
    from puzzlenet_amd import assembly
    f = fracture
    rng = np.random.default_rng(5)
    X = f.pose.double().cpu().numpy()
    root = np.array([0, 3, 1], dtype=np.int32)
    G = np.stack([[X[z, root[z]] @ _inv(X[z, p]) @ (_nudge(rng, 1.0, 0.02) if (z + p) % 3 else _nudge(rng, 25.0, 0.3))
                   for p in range(FP)] for z in range(FB)])
    placed = np.ones((FB, FP), dtype=bool)
    placed[1, 0] = placed[2, 2] = placed[2, 3] = False
    edges = np.full((FB, FP - 1, 3), -1, dtype=np.int32)
    edges[0] = [(0, 1, 1), (2, 1, 2), (3, 0, 3)]
    edges[1, :2] = [(3, 1, 1), (1, 2, 2)]
    n_edges = np.array([3, 2, 0], dtype=np.int32)
    to = lambda a: torch.from_numpy(a).to(dev)
    ev = assembly.evaluate_batch(to(G), to(placed), f.pose, f.rest, to(root), to(edges), to(n_edges), f.mates, tol=TOL)
    assert ev.rot_deg.dtype == torch.float64 and ev.msd.shape == (FB, FP) and ev.part_ok.dtype == torch.bool
    some_ok = some_not = False
    for z in range(FB):
        e = [tuple(int(v) for v in r) for r in edges[z, :n_edges[z]]]
        one = assembly.evaluate(G[z], placed[z], f.pose[z], f.rest[z], int(root[z]), e, f.mates[z], tol=TOL)
        assert np.abs(one.msd - TOL).min() > 1e-6                                 # no verdict hangs on the last places
        rot, trans, msd = (x[z].cpu().numpy() for x in (ev.rot_deg, ev.trans, ev.msd))
        print(f"puzzle {z}: max |rot| diff {np.abs(rot - one.rot_deg).max():.2e}, |trans| {np.abs(trans - one.trans).max():.2e}, "
              f"msd rel {np.abs(msd / one.msd - 1).max():.2e}")
        assert np.abs(rot - one.rot_deg).max() <= 1e-12 and np.abs(trans - one.trans).max() <= 1e-12
        assert np.abs(msd - one.msd).max() <= 1e-12 and (np.abs(msd - one.msd) <= 1e-12 * one.msd).all()
        assert np.array_equal(ev.part_ok[z].cpu().numpy(), one.part_ok)
        assert float(ev.part_accuracy[z]) == one.part_accuracy
        if one.edge_precision is None:
            assert bool(torch.isnan(ev.edge_precision[z]))
        else:
            assert float(ev.edge_precision[z]) == one.edge_precision
        some_ok |= bool(one.part_ok.any())
        some_not |= bool((placed[z] & ~one.part_ok).any())
    assert some_ok and some_not
    assert assembly.evaluate_batch(to(G), to(placed), f.pose, f.rest, to(root)).edge_precision is None
    with pytest.raises(assembly._lib.PznError):
        assembly.evaluate_batch(to(G), to(placed), f.pose.cpu(), f.rest, to(root))
    with pytest.raises(assembly._lib.PznError):
        assembly.evaluate_batch(to(G)[:, :3], to(placed), f.pose, f.rest, to(root))


def _connected(adj):
    seen, todo = {0}, [0]
    while todo:
        i = todo.pop()
        for j in np.flatnonzero(adj[i]):
            if int(j) not in seen:
                seen.add(int(j))
                todo.append(int(j))
    return len(seen) == len(adj)


def test_the_truth_assembles_itself_in_a_batch(dev, fracture):
    """truth_table's scores and poses for every puzzle of the batch -> assemble_batch -> evaluate_batch: every edge joins two
    mates and every piece lands where it belongs."""
    from puzzlenet_amd import assembly
    f = fracture
    tables = [assembly.truth_table(f.pose[z], f.mates[z], f.cd[z]) for z in range(FB)]
    assert all(_connected(f.mates[z].cpu().numpy()) for z in range(FB))          # (seeds whose pieces all touch some other)
    T = torch.from_numpy(np.stack([t for t, _ in tables]).astype(np.float32)).to(dev)
    S = torch.from_numpy(np.stack([s for _, s in tables]).astype(np.float32)).to(dev)
    asm = assembly.assemble_batch(S, T)
    ev = assembly.evaluate_batch(asm.G, asm.placed, f.pose, f.rest, asm.root, asm.edges, asm.n_edges, f.mates)
    print("msd", ev.msd.tolist(), "rot_deg", ev.rot_deg.tolist())
    assert bool(asm.placed.all()) and asm.n_edges.tolist() == [FP - 1] * FB
    assert ev.part_accuracy.tolist() == [1.0] * FB and ev.edge_precision.tolist() == [1.0] * FB
    # the same answer as the per-puzzle walk on the same tables
    for z in range(FB):
        a = assembly.assemble(S[z], T[z])
        assert a.root == int(asm.root[z]) and [(i, j, n) for i, j, _s, n in a.edges] == [tuple(r) for r in asm.edges[z].tolist()]
