"""GPU: the batched progressive chain - assembly.pair_block_batch, match_puzzles' launch count, ProgressiveBatch round by round and
its result through evaluate_batch - against the per-puzzle functions it stands beside (pair_block, ops.merge_resample,
progressive_round_rule, evaluate), with the closed-form model of tests/test_gpu_assembly.py.  The round kernel itself is held to its
rule in tests/test_gpu_progressive_round.py, the blocked head to ops.pair_head in tests/test_gpu_pair_head_blocks.py.

As in tests/test_gpu_assembly_batch.py, the fields behind the few-row layers (twist, and with it T and score) are not equal bit for
bit between two calls, so they are held to that file's tolerances across calls, and bit for bit against the table's OWN logits, picks
and poses, where nothing is noisy."""
import numpy as np
import pytest
import torch

from oracle import model_ref as mr
from tests import _fracture as fr
from tests import _walk_cases as wc

pytestmark = pytest.mark.gpu

Z, P, N, TOP = 3, 4, 1024, 128
FB, FM, FP, FK, Fn, Fk = 3, 4096, 4, 8, 256, 32      # the fracture batch: clouds, points, pieces, candidates, n, k


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
def inputs(dev, model):
    g = torch.Generator().manual_seed(2718)
    assert model.num_points == N
    pieces = torch.rand(Z, P, N, 3, generator=g).to(dev)
    start = (torch.randint(0, N, (Z, P), generator=g), torch.randint(0, 512, (Z, P), generator=g))
    merge_starts = torch.randint(0, N, (Z, P - 1), generator=g)
    return pieces, start, merge_starts


def _snapshot(pb):
    """Every tensor of a ProgressiveBatch's state, cloned."""
    t = pb.table
    out = dict(twist=t.twist.clone(), T=t.T.clone(), y_f=t.de_fpcb.permute(0, 1, 2, 4, 3).clone(), top_f=t.top_f.clone(),
               score=t.score.clone())                                             # (y_f: the kernel's [Z,P,P,N,2] layout)
    out.update({name: getattr(pb, name).clone() for name in ("parts", "piece_id", "row_id")})
    out.update({"codes." + n: f.clone() for n, f in zip(pb.codes._fields, pb.codes)})
    out.update({"ledger." + n: f.clone() for n, f in zip(pb.ledger._fields, pb.ledger)})
    return out


@pytest.fixture(scope="module")
def walk(dev, model, inputs):
    """One ProgressiveBatch walked to its end, with a snapshot of the state before the first round and after every round."""
    from puzzlenet_amd import assembly
    pieces, start, merge_starts = inputs
    pb = assembly.ProgressiveBatch(model, pieces, k=TOP, start=start, merge_starts=merge_starts)
    shots, picks = [_snapshot(pb)], []
    for _ in range(P - 1):
        took, pick = pb.step()
        shots.append(_snapshot(pb))
        picks.append((took.cpu().numpy(), pick.cpu().numpy()))
    with pytest.raises(assembly._lib.PznError):
        pb.step()                                                                 # the P - 1 rounds are made
    return dict(pb=pb, shots=shots, picks=picks, result=pb.result())


def _close(got, want, rtol, atol, msg):
    np.testing.assert_allclose(got.detach().cpu().numpy(), want.detach().cpu().numpy(), rtol=rtol, atol=atol, err_msg=msg)


def _own_score(pf, top_f, pm, top_m, T):
    """The score of one pair from its own picks and pose, by pair_block's calls: pf, pm [N,3], top_f, top_m [k], T [4,4]."""
    from puzzlenet_amd import ops, se3
    Bf = ops.index_points(pf[None], top_f[None])
    Bm = ops.index_points(pm[None], top_m[None])
    d1, d2 = ops.chamfer(Bf, se3.transform_points(T[None], Bm))
    return (d1.mean(dim=1) + d2.mean(dim=1))[0]


# --------------------------------------------------------------------------- pair_block_batch

def test_pair_block_batch_against_pair_block(dev, model, inputs):
    from puzzlenet_amd import assembly, ops, se3
    pieces, start, _ = inputs
    flat = assembly.encode_pieces(model, pieces.view(Z * P, N, 3), TOP, tuple(s.reshape(-1) for s in start))
    codes = assembly.PieceCodes(*(f.view(Z, P, *f.shape[1:]) for f in flat))
    blk = assembly.pair_block_batch(model, pieces, codes, pieces, codes, TOP)
    ref = assembly.pair_block_batch(model, pieces, codes, pieces, codes, TOP, refine=5)
    assert blk.twist.shape == (Z, P, P, 6) and blk.T.shape == (Z, P, P, 4, 4) and blk.de_fpcb.shape == (Z, P, P, 2, N)
    assert blk.top_f.shape == (Z, P, P, TOP) and blk.top_f.dtype == torch.int64 and blk.score.shape == (Z, P, P)
    assert torch.equal(blk.T, se3.exp(blk.twist))
    assert torch.equal(ref.de_fpcb, blk.de_fpcb) and torch.equal(ref.top_f, blk.top_f)
    lower = 0
    for z in range(Z):
        cz = assembly.PieceCodes(*(f[z] for f in codes))
        one = assembly.pair_block(model, pieces[z], cz, pieces[z], cz, TOP)
        assert torch.equal(blk.de_fpcb[z], one.de_fpcb)                          # the blocked head has the same bits
        assert torch.equal(blk.top_f[z], one.top_f)
        _close(blk.twist[z], one.twist, 1e-4, 1e-5, "twist")
        # picks and score against the block's own logits, picks and poses, by the same calls
        y_f = blk.de_fpcb[z].permute(0, 1, 3, 2).contiguous()
        assert torch.equal(blk.top_f[z], ops.topk_rows(torch.softmax(y_f, dim=-1)[..., 1].reshape(P * P, N), TOP).view(P, P, TOP))
        Bf = ops.index_points(pieces[z], blk.top_f[z].reshape(P, P * TOP)).view(P * P, TOP, 3)
        Bm = ops.index_points(pieces[z], codes.top_m[z])
        d1, d2 = ops.chamfer(Bf, se3.transform_points(blk.T[z].reshape(P * P, 4, 4),
                                                      Bm.unsqueeze(0).expand(P, -1, -1, -1).reshape(P * P, TOP, 3)))
        assert torch.equal(blk.score[z], (d1.mean(dim=1) + d2.mean(dim=1)).view(P, P))
        # refine = 5: T and score are _refine_gathered's on its own gathers, from se3.exp of its own twist
        r = assembly._refine_gathered(Bf, Bm, se3.exp(ref.twist[z]), 5)
        assert torch.equal(ref.T[z], r.T) and torch.equal(ref.score[z], r.score)
        lower += int((r.score < r.score0).sum())
    assert lower > 0                                                              # some pose did move
    with pytest.raises(assembly._lib.PznError):
        assembly.pair_block_batch(model, pieces[0], codes, pieces, codes, TOP)
    with pytest.raises(assembly._lib.PznError):
        assembly.pair_block_batch(model, pieces, codes, pieces[:2], codes, TOP)
    with pytest.raises(assembly._lib.PznError):
        assembly.pair_block_batch(model, pieces.cpu(), codes, pieces, codes, TOP)


# --------------------------------------------------------------------------- ProgressiveBatch, round by round

def test_rounds_follow_the_rule(walk):
    """The ledger after a round is progressive_round_rule on the table and the ledger held before it."""
    from puzzlenet_amd import assembly
    merges = 0
    for r in range(P - 1):
        before, after = walk["shots"][r], walk["shots"][r + 1]
        state = assembly.ProgressiveState(*(before["ledger." + n] for n in assembly.ProgressiveState._fields))
        want, took, pick = assembly.progressive_round_rule(before["score"], before["T"], state)
        for name, w in zip(want._fields, want):
            g = after["ledger." + name].cpu()
            assert g.dtype == torch.from_numpy(w).dtype and torch.equal(g, torch.from_numpy(w)), (r, name)
        assert np.array_equal(walk["picks"][r][0], took) and np.array_equal(walk["picks"][r][1], pick)
        merges += int(took.sum())
    assert merges == Z * (P - 1)                                                  # finite scores: every puzzle walks to one part


def test_merged_parts_are_merge_resample_on_the_state_before(walk, inputs):
    from puzzlenet_amd import ops
    merge_starts = inputs[2]
    for r in range(P - 1):
        before, after = walk["shots"][r], walk["shots"][r + 1]
        took, pick = walk["picks"][r]
        for z in range(Z):
            assert took[z]
            i, j = (int(v) for v in pick[z])
            merged, src = ops.merge_resample(before["parts"][z, i][None], before["parts"][z, j][None], before["T"][z, i, j][None],
                                             merge_starts[z, r:r + 1].to(before["parts"].device), N, before["top_f"][z, i, j][None],
                                             before["codes.top_m"][z, j][None])
            assert torch.equal(after["parts"][z, i], merged[0])
            assert torch.equal(after["piece_id"][z, i], torch.cat((before["piece_id"][z, i], before["piece_id"][z, j]))[src[0]])
            assert torch.equal(after["row_id"][z, i], torch.cat((before["row_id"][z, i], before["row_id"][z, j]))[src[0]])
            # the rows left out are the matched ones, and no kept point is one of them
            gone = walk["pb"].dropped[r][z].reshape(-1, 2)
            want = torch.cat((torch.stack((before["piece_id"][z, i], before["row_id"][z, i]), dim=1)[before["top_f"][z, i, j]],
                              torch.stack((before["piece_id"][z, j], before["row_id"][z, j]), dim=1)[before["codes.top_m"][z, j]]))
            assert torch.equal(gone, want)
            kept = set(zip(after["piece_id"][z, i].tolist(), after["row_id"][z, i].tolist()))
            assert not kept & set(map(tuple, gone.tolist()))
            # every other slot's part and provenance stay as they were
            others = [s for s in range(P) if s != i]
            for name in ("parts", "piece_id", "row_id"):
                assert torch.equal(after[name][z, others], before[name][z, others]), name


def test_provenance(walk, inputs):
    """Every point of every live part is pieces[z, piece_id, row_id] under G (the tolerance of _check_provenance in
    tests/test_gpu_progressive.py: fp32 points moved by fp32 poses against the float64 ledger)."""
    pieces = inputs[0].cpu()
    worst = 0.0
    for shot in walk["shots"]:
        G, alive = shot["ledger.G"].cpu().numpy(), shot["ledger.alive"].cpu().numpy()
        for z in range(Z):
            for s in np.flatnonzero(alive[z]):
                pid, rid = shot["piece_id"][z, s].cpu(), shot["row_id"][z, s].cpu()
                src = pieces[z][pid, rid].double().numpy()
                g = G[z][pid.numpy()]
                want = np.einsum("nab,nb->na", g[:, :3, :3], src) + g[:, :3, 3]
                worst = max(worst, float(np.abs(want - shot["parts"][z, s].cpu().double().numpy()).max()))
    print(f"provenance: largest deviation {worst:.3g}")
    assert worst <= 1e-5
    last = walk["shots"][-1]
    for z in range(Z):                                                            # one part is left and it holds all P pieces
        s = int(np.flatnonzero(last["ledger.alive"][z].cpu().numpy())[0])
        assert sorted(set(last["piece_id"][z, s].tolist())) == list(range(P))


def test_tables_stay_consistent_and_kept_entries_keep_their_bits(walk):
    """After every round: the new row and column are consistent with their own logits, picks and poses (and so is every other live
    entry, whose two parts did not change); everything outside row i, column i and the dead slots has its bits from before; dead
    slots and the diagonal have score +inf."""
    from puzzlenet_amd import ops, se3
    for r in range(P - 1):
        before, after = walk["shots"][r], walk["shots"][r + 1]
        pick = walk["picks"][r][1]
        alive = after["ledger.alive"].cpu().numpy().astype(bool)
        y_f, top_f, top_m = after["y_f"], after["top_f"], after["codes.top_m"]
        assert torch.equal(top_f.view(Z * P * P, TOP), ops.topk_rows(torch.softmax(y_f, dim=-1)[..., 1].reshape(Z * P * P, N), TOP))
        y_m = after["codes.de_mrpcb"].permute(0, 1, 3, 2).contiguous()
        assert torch.equal(top_m.view(Z * P, TOP), ops.topk_rows(torch.softmax(y_m, dim=-1)[..., 1].reshape(Z * P, N), TOP))
        assert torch.equal(after["T"], se3.exp(after["twist"]))
        score = after["score"].cpu()
        for z in range(Z):
            i, j = (int(v) for v in pick[z])
            assert alive[z, i] and not alive[z, j]
            for a in range(P):
                for b in range(P):
                    if a == b or not (alive[z, a] and alive[z, b]):
                        assert score[z, a, b] == float("inf")
                        continue
                    own = _own_score(after["parts"][z, a], top_f[z, a, b], after["parts"][z, b], top_m[z, b], after["T"][z, a, b])
                    assert torch.equal(after["score"][z, a, b], own), (r, z, a, b)
                    if a != i and b != i:
                        assert torch.equal(after["score"][z, a, b], before["score"][z, a, b])
            keep = [s for s in range(P) if s != i]
            for name in ("twist", "T", "y_f", "top_f"):
                assert torch.equal(after[name][z][keep][:, keep], before[name][z][keep][:, keep]), (r, z, name)
            for name in ("U", "V", "local_f", "g_max", "de_mrpcb", "top_m", "x2"):
                assert torch.equal(after["codes." + name][z, keep], before["codes." + name][z, keep]), (r, z, name)


def test_a_puzzle_stopped_by_max_score_keeps_every_bit(dev, model, inputs, walk):
    """max_score between two first-round minima of the table: the puzzles above it stop in the first round and keep every state
    tensor bit for bit while the others walk on."""
    from puzzlenet_amd import assembly
    pieces, start, merge_starts = inputs
    first = walk["shots"][0]["score"].view(Z, -1).min(dim=1).values.cpu().double().numpy()
    order = np.sort(first)
    limit = float((order[0] + order[1]) / 2)
    assert (order[1] - order[0]) > 1e-3 * order[1]                                # (the few-row layers' noise is far below the gap)
    pb = assembly.ProgressiveBatch(model, pieces, k=TOP, start=start, merge_starts=merge_starts, max_score=limit)
    shot0 = _snapshot(pb)
    took, _ = pb.step()
    assert took.tolist().count(1) == 1 and int(took.cpu().numpy().argmax()) == int(first.argmin())
    for _ in range(P - 2):
        pb.step()
    shot = _snapshot(pb)
    stopped = [z for z in range(Z) if not took[z]]
    for name in shot:
        if name == "ledger.done":
            assert shot[name][stopped].tolist() == [1] * len(stopped)
        else:
            assert torch.equal(shot[name][stopped], shot0[name][stopped]), name
    go = int(took.cpu().numpy().argmax())
    assert int(shot["ledger.n_edges"][go]) >= 1 and not torch.equal(shot["parts"][go], shot0["parts"][go])
    res = pb.result()
    assert res.root[stopped].tolist() == [-1] * len(stopped) and not bool(res.placed[stopped].any()) and int(res.root[go]) >= 0
    assert bool((res.dropped[0][stopped] == -1).all()) and bool((res.dropped[0][go] >= 0).all())


def test_puzzles_of_fewer_pieces_than_slots(dev, model, inputs):
    """count below P: the slots at or beyond it start dead, never take part and keep their pieces; a puzzle of c pieces makes c - 1
    merges and then idles."""
    from puzzlenet_amd import assembly
    pieces, start, merge_starts = inputs
    counts = [4, 2, 3]
    pb = assembly.ProgressiveBatch(model, pieces, k=TOP, start=start, merge_starts=merge_starts,
                                   count=torch.tensor(counts, dtype=torch.int32, device=dev))
    score0 = pb.table.score.cpu()
    for z, c in enumerate(counts):
        assert bool(torch.isinf(score0[z, c:]).all()) and bool(torch.isinf(score0[z, :, c:]).all())
        assert bool(torch.isfinite(score0[z, :c, :c][~torch.eye(c, dtype=torch.bool)]).all())
    r = pb.run()
    assert r.n_edges.tolist() == [c - 1 for c in counts] and r.alive.sum(dim=1).tolist() == [1] * Z
    assert pb.ledger.done.tolist() == [0, 1, 1]                                   # the short puzzles met a round with one part left
    for z, c in enumerate(counts):
        assert r.placed[z].tolist() == [True] * c + [False] * (P - c)
        assert torch.equal(r.parts[z, c:], pieces[z, c:]) and r.part[z, c:].tolist() == list(range(c, P))
        assert int(r.edges[z, :c - 1].max()) < c and bool((r.edges[z, c - 1:] == -1).all())
        live = int(r.alive[z].int().argmax())
        assert sorted(set(r.piece_id[z, live].tolist())) == list(range(c))


def test_result_goes_through_evaluate_batch(dev, walk):
    """result() feeds evaluate_batch as it is; per puzzle it agrees with evaluate on the downloaded G, placed and root (random rigid
    'truth' poses: no error is a difference of nearly equal numbers, the tolerances of test_evaluate_batch_against_evaluate)."""
    from puzzlenet_amd import assembly
    r = walk["result"]
    assert r.G.dtype == torch.float64 and r.G.shape == (Z, P, 4, 4) and r.edges.shape == (Z, P - 1, 4) and r.root.shape == (Z,)
    assert r.placed.dtype == torch.bool and bool(r.placed.all()) and r.n_edges.tolist() == [P - 1] * Z
    assert r.parts.shape == (Z, P, N, 3) and r.dropped.shape == (P - 1, Z, 2, TOP, 2) and r.alive.sum(dim=1).tolist() == [1] * Z
    rng = np.random.default_rng(11)
    pose = torch.from_numpy(wc.rigid(rng, (Z, P))).to(dev)
    rest = torch.from_numpy(rng.normal(size=(Z, P, 64, 3)).astype(np.float32)).to(dev)
    mates = torch.from_numpy(rng.random((Z, P, P)) < 0.5).to(dev)
    ev = assembly.evaluate_batch(r.G, r.placed, pose, rest, r.root, r.edges, r.n_edges, mates)
    for z in range(Z):
        assert int(r.root[z]) == int(r.part[z, int(r.edges[z, 0, 0])]) and bool(r.alive[z, int(r.root[z])])
        e = [tuple(int(v) for v in row[:2]) for row in r.edges[z].cpu().numpy()]
        one = assembly.evaluate(r.G[z], r.placed[z], pose[z], rest[z], int(r.root[z]), e, mates[z])
        rot, trans, msd = (x[z].cpu().numpy() for x in (ev.rot_deg, ev.trans, ev.msd))
        print(f"puzzle {z}: max |rot| diff {np.abs(rot - one.rot_deg).max():.2e}, |trans| {np.abs(trans - one.trans).max():.2e}, "
              f"msd rel {np.abs(msd / np.maximum(one.msd, 1e-300) - 1).max():.2e}")
        assert np.abs(rot - one.rot_deg).max() <= 1e-12 and np.abs(trans - one.trans).max() <= 1e-12
        # (the root's own msd is the rounding of pose[root] inv(pose[root]) - I, about 1e-32: no relative bound holds there)
        others = np.arange(P) != int(r.root[z])
        assert np.abs(msd - one.msd).max() <= 1e-12 and (np.abs(msd - one.msd) <= 1e-12 * one.msd)[others].all()
        assert np.array_equal(ev.part_ok[z].cpu().numpy(), one.part_ok) and float(ev.part_accuracy[z]) == one.part_accuracy
        assert float(ev.edge_precision[z]) == one.edge_precision


# --------------------------------------------------------------------------- on the truth

def test_the_truth_assembles_itself_round_by_round(dev):
    """truth_table's scores and poses of a small fracture, ops.progressive_round driven for P - 1 rounds: every merge joins two
    parts that touch, one part is left, and every piece lands where it belongs (test_the_truth_assembles_itself_in_a_batch's bound:
    part_ok, msd < 0.01).

    The table of the first round is truth_table's as it is.  Slots are not compacted and slot j dies with its row, so on a table
    that never changes the part in slot i would only ever meet the mates of piece i itself - a walk can strand there with parts that
    do touch (seen on this fracture: two of three puzzles stop after one merge).  A progressive walk computes the merged part's row
    and column again; what a perfect matcher returns for them is known in closed form and is filled in between the rounds: the
    merged part touches whatever either of the two touched, at the smaller distance (the element-wise minimum of rows i, j and of
    columns i, j), and T[i,c] = pose[i] inv(pose[c]) already is the truth between the frames of slot i and slot c, mates or not."""
    from puzzlenet_amd import assembly, datapipe, ops
    raw = fr.clouds(FB, FM, 40)
    normals, u_anchor, u_start, twist = fr.draws(FB, FP, FK, 41)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    f = datapipe.fracture(to(raw), to(normals), to(u_anchor), to(u_start), to(twist), n=Fn, k=Fk)
    tables = [assembly.truth_table(f.pose[z], f.mates[z], f.cd[z]) for z in range(FB)]
    T = torch.from_numpy(np.stack([t for t, _ in tables]).astype(np.float32)).to(dev)
    S = torch.from_numpy(np.stack([s for _, s in tables]).astype(np.float32)).to(dev)
    mates = f.mates.cpu().numpy() != 0
    state = ops.progressive_state(FB, FP, dev)
    z = torch.arange(FB, device=dev)
    for _ in range(FP - 1):
        part = state.part.cpu().numpy()
        took, pick = ops.progressive_round(S, T, state)
        assert took.tolist() == [1] * FB
        for q, (i, j) in enumerate(pick.tolist()):      # some piece of part i and some piece of part j are mates
            assert mates[q][np.ix_(part[q] == i, part[q] == j)].any()
        i, j = pick[:, 0], pick[:, 1]
        S[z, i] = torch.minimum(S[z, i], S[z, j])
        S[z, :, i] = torch.minimum(S[z, :, i], S[z, :, j])
    assert state.alive.sum(dim=1).tolist() == [1] * FB and state.n_edges.tolist() == [FP - 1] * FB and state.done.tolist() == [0] * FB
    root = state.alive.argmax(dim=1).to(torch.int32)
    assert bool((state.part == root[:, None]).all())
    ev = assembly.evaluate_batch(state.G, state.part == root[:, None], f.pose, f.rest, root)
    print("msd", ev.msd.tolist(), "rot_deg", ev.rot_deg.tolist())
    assert ev.part_accuracy.tolist() == [1.0] * FB and bool(ev.part_ok.all())


# --------------------------------------------------------------------------- launch counts

def _launches(fn):
    from puzzlenet_amd import ops
    real, calls = ops._call, []

    def spy(name, *a, **k):
        calls.append(name)
        return real(name, *a, **k)
    ops._call = spy
    try:
        fn()
    finally:
        ops._call = real
    return calls


def test_launch_counts_do_not_grow_with_z(dev, model):
    """match_puzzles and one ProgressiveBatch.step() make the same library launches for two puzzles as for four."""
    from puzzlenet_amd import assembly
    g = torch.Generator().manual_seed(99)
    pieces = torch.rand(4, P, N, 3, generator=g).to(dev)
    n2 = _launches(lambda: assembly.match_puzzles(model, pieces[:2], k=TOP))
    n4 = _launches(lambda: assembly.match_puzzles(model, pieces, k=TOP))
    print(f"library launches: match_puzzles of 2 puzzles {len(n2)}, of 4 puzzles {len(n4)}")
    assert n2 == n4 and n4.count("pzn_pair_head_blocks_fwd_f32") == 1
    steps = []
    for z in (2, 4):
        pb = assembly.ProgressiveBatch(model, pieces[:z], k=TOP)
        steps.append(_launches(pb.step))
    print(f"library launches: one ProgressiveBatch.step() of 2 puzzles {len(steps[0])}, of 4 puzzles {len(steps[1])}")
    assert steps[0] == steps[1]
    assert steps[1].count("pzn_progressive_round_f32") == 1 and steps[1].count("pzn_merge_resample_f32") == 1
    assert steps[1].count("pzn_pair_head_blocks_fwd_f32") == 2                    # the new row and the new column
