"""GPU: training pairs cut out of fractures - ops.fracture_pair (pzn_fracture_pair_f32, csrc/fracture.hip) against its numpy
statement datapipe.fracture_pair_rule bit for bit in every output; datapipe.cut_pairs_fracture against the single cut at two
pieces, against the ops it is made of, and its acceptance test against float64; PairFeeder(pieces=...) on top."""
import numpy as np
import pytest
import torch

from tests import _double_cut as dc
from tests import _fracture_pair as fp

pytestmark = pytest.mark.gpu

GUARD = 4096      # floats behind the pieces buffer that no launch may touch
SENTINEL = -7.5
# |cd (float32, device) - cd (float64, numpy)|, derived as CD_MARGIN of tests/test_gpu_double_feeder.py is: the device takes
# squared distances in the expansion form |a|^2 + |b|^2 - 2 a.b in float32; the clouds of tests/_fracture.py fill [-0.5, 0.5)^3,
# so |p|^2 <= 0.75 and |a|^2 + |b|^2 <= 1.5; each of the three roundings (the sum, the product sum, the final fma) is at most
# 2^-24 * 1.5 = 8.95e-8, so a distance is off by <= 2.7e-7, a mean of distances by no more, and cd (two means) by <= 5.4e-7.
CD_MARGIN = 5.4e-7


def _dev():
    return torch.device("cuda:0")


def _to(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(_dev())


def _launch_guarded(raw, normals, u_anchor, u, pieces, n_min, neighbours, cap):
    """pzn_fracture_pair_f32 through the C ABI on buffers of the test's own, the pieces buffer followed by a guard band.
    -> the outputs in ops.fracture_pair's order (numpy), the guard band"""
    from puzzlenet_amd import ops
    B, M, _ = raw.shape
    P, K = normals.shape[1] + 1, normals.shape[2]
    dev = _dev()
    d_raw, d_normals, d_anchor, d_u = (_to(t) for t in (raw, normals, u_anchor, u))
    d_pieces = _to(np.asarray(pieces, dtype=np.int32))
    flat = torch.full((4 * B * cap * 3 + GUARD,), SENTINEL, dtype=torch.float32, device=dev)
    counts = torch.empty((4 * B,), dtype=torch.int64, device=dev)
    start = torch.empty((4 * B,), dtype=torch.int64, device=dev)
    kind = torch.empty((B,), dtype=torch.int32, device=dev)
    pair = torch.empty((B, 4), dtype=torch.int32, device=dev)
    label = torch.empty((B, M), dtype=torch.uint8, device=dev)
    planes = torch.empty((B, P - 1, 4), dtype=torch.float64, device=dev)
    target = torch.empty((B, P - 1), dtype=torch.int32, device=dev)
    cand = torch.empty((B, P - 1), dtype=torch.int32, device=dev)
    ok = torch.empty((B,), dtype=torch.uint8, device=dev)
    ops._call("pzn_fracture_pair_f32", d_raw.data_ptr(), d_normals.data_ptr(), d_anchor.data_ptr(), d_pieces.data_ptr(),
              d_u.data_ptr(), float(neighbours), B, M, P, K, n_min, cap, flat.data_ptr(), counts.data_ptr(), start.data_ptr(),
              kind.data_ptr(), pair.data_ptr(), label.data_ptr(), planes.data_ptr(), target.data_ptr(), cand.data_ptr(),
              ok.data_ptr(), ops._stream())
    torch.cuda.synchronize()
    body = flat[:4 * B * cap * 3].view(4 * B, cap, 3)
    out = [t.cpu().numpy() for t in (body, counts, start, kind, pair, label, planes, target, cand, ok.to(torch.bool))]
    return out, flat[4 * B * cap * 3:].cpu().numpy()


def _compare(got, want, tag):
    for name, g, w in zip(fp.NAMES, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (tag, name, g.dtype, w.dtype, g.shape, w.shape)
        if g.tobytes() != w.tobytes():
            bad = np.flatnonzero((g != w).reshape(len(g), -1).any(1))
            raise AssertionError(f"{tag}: {name} differs in rows {bad[:8].tolist()} ({len(bad)} of {len(g)})")


def _run_and_compare(raw, normals, u_anchor, u, pieces, n_min, neighbours, cap, tag):
    """The kernel through ops.fracture_pair and through the guarded buffers, both against the statement -> its records."""
    from puzzlenet_amd import ops
    recs, want = fp.batch_statement(raw, normals, u_anchor, u, pieces, n_min, neighbours, cap)
    got = ops.fracture_pair(_to(raw), _to(normals), _to(u_anchor), _to(np.asarray(pieces, dtype=np.int32)), _to(u), n_min,
                            neighbours, cap)
    torch.cuda.synchronize()
    _compare([t.cpu().numpy() for t in got], want, tag)
    guarded, band = _launch_guarded(raw, normals, u_anchor, u, pieces, n_min, neighbours, cap)
    _compare(guarded, want, (tag, "guarded"))
    assert (band == SENTINEL).all(), tag                       # nothing behind the last piece's `cap` rows was written
    return recs


def _aim(u_row, Pb, a, c):
    """Set u_a, u_c of one sample so that the drawn ordered pair is (a, c)."""
    u_row[1] = (a + 0.5) / Pb
    u_row[2] = (c - (c > a) + 0.5) / (Pb - 1)


def _sibling(raw, normals, u_anchor, u, Pb, P, n_min):
    from puzzlenet_amd import datapipe
    r = datapipe.fracture_pair_rule(raw, normals, u_anchor, u, Pb, P, n_min, 0.0, raw.shape[0])
    return int(r["pair"][0]), int(r["pair"][1])


def _inputs(B, M, P, K, seed):
    raw = fp.clouds(B, M, seed)
    normals, u_anchor, u, twist = fp.draws(B, P, K, seed + 1)
    return raw, normals, u_anchor, u, twist


def test_kernel_against_the_rule_with_every_kind():
    """B = 5, per-sample pieces (2, 3, 4, 5, 5): u_kind, u_a and u_c are set so that the batch holds a SIBLING by u_kind, a
    NEIGHBOUR, and a neighbour draw that IS the sibling pair (in the reversed order), whatever the seeds give elsewhere."""
    from puzzlenet_amd import datapipe as dp
    B, M, P, K, n_min = 5, 1000, 5, 4, 64
    pieces = [2, 3, 4, 5, 5]
    raw, normals, u_anchor, u, _ = _inputs(B, M, P, K, 300)
    u[:, 0] = [0.1, 0.9, 0.1, 0.1, 0.1]
    s2 = _sibling(raw[2], normals[2], u_anchor[2], u[2], 4, P, n_min)
    _aim(u[2], 4, *[(a, c) for a in range(4) for c in range(4) if a != c and {a, c} != set(s2)][3])      # a pair that is not
    s3 = _sibling(raw[3], normals[3], u_anchor[3], u[3], 5, P, n_min)
    _aim(u[3], 5, s3[1], s3[0])                                                                           # D, U: the sibling pair
    recs = _run_and_compare(raw, normals, u_anchor, u, pieces, n_min, 0.5, M, "five")
    kinds = [r["kind"] for r in recs]
    print("kinds", kinds, "pairs", [r["pair"].tolist() for r in recs], "ok", [r["ok"] for r in recs])
    assert kinds[:4] == [dp.SIBLING, dp.SIBLING, dp.NEIGHBOUR, dp.SIBLING]
    assert u[3, 0] < 0.5 and tuple(recs[3]["pair"]) == s3 + (-1, -1)      # the fold: drawn as a neighbour, the sibling pair
    assert tuple(recs[2]["pair"][2:]) == s2 and all(r["ok"] for r in recs)
    for b, r in enumerate(recs):
        fp.check_invariants(raw[b], normals[b], u_anchor[b], u[b], pieces[b], n_min, 0.5, M, r)


# (B, M, P, K, n_min, cap, pieces, neighbours)
CASES = [
    (3, 1025, 4, 4, 64, 1025, (4, 3, 2), 1.0),          # an odd run length: runs of 2 points, the last thread short
    (1, 65536, 16, 16, 1024, 32768, (16,), 1.0),        # the limit shape: runs of 64 points, more than 64 KiB of LDS
    (2, 333, 16, 2, 4, 333, (16, 9), 0.5),              # steps without a valid candidate
    (4, 2048, 5, 1, 64, 2048, (5, 5, 3, 2), 0.5),       # K = 1: the most-balanced path; an empty piece is possible
    (3, 4096, 3, 8, 128, 1200, (3, 2, 3), 1.0),         # a cap below a piece's size: rows beyond cap are never written, ok = 0
]
SALT = {333: 4}      # (tests/test_gpu_fracture.py's: seeds whose two samples include a step without a valid candidate)


@pytest.mark.parametrize("case", CASES, ids=str)
def test_kernel_against_the_rule(case):
    B, M, P, K, n_min, cap, pieces, neighbours = case
    salt = M + P + SALT.get(M, 0)
    raw = fp.clouds(B, M, 1000 + salt)
    normals, u_anchor, u, _ = fp.draws(B, P, K, 2000 + salt)
    recs = _run_and_compare(raw, normals, u_anchor, u, pieces, n_min, neighbours, cap, case)
    oks = [r["ok"] for r in recs]
    print(case, "ok", oks, "kinds", [r["kind"] for r in recs], "counts", [r["counts"].tolist() for r in recs])
    for b, r in enumerate(recs):
        fp.check_invariants(raw[b], normals[b], u_anchor[b], u[b], pieces[b], n_min, neighbours, cap, r)
    if M in (333, 2048):
        assert not all(oks)                                    # the most-balanced path was compared
    if cap == 1200:
        assert not any(oks) and all(r["counts"].max() > cap for r in recs)
    if M == 65536:
        assert all(oks)


def test_p2_is_the_single_cut():
    """Two pieces: the sibling pair is (up, down) of the one plane, so the 8-tuple is cut_pairs' on the recorded plane."""
    from puzzlenet_amd import datapipe as dp
    B, M, K, n, k = 4, 5000, 16, 512, 64
    raw, normals, u_anchor, u, twist = _inputs(B, M, 2, K, 410)
    got, ok, rec = dp.cut_pairs_fracture(_to(raw), _to(normals), _to(u_anchor), 2, _to(u), _to(twist), n=n, k=k, neighbours=0.5)
    assert bool(ok.all()) and not bool(rec.kind.any()) and not bool(rec.rejected.any())
    assert rec.pair.cpu().tolist() == [[0, 1, -1, -1]] * B
    plane = rec.planes[:, 0]                                   # [B,4]: the plane taken, its only candidate now
    want, wok, wplane = dp.cut_pairs(_to(raw), plane[:, None, :3].contiguous(), plane[:, 3:4].contiguous(),
                                     _to(np.ascontiguousarray(u[:, 3:5])), _to(twist), n=n, k=k)
    torch.cuda.synchronize()
    assert bool(wok.all()) and torch.equal(wplane, plane)
    for name, g, w in zip("down moved igt up downb upb down_mask up_mask".split(), got, want):
        assert g.dtype == w.dtype and torch.equal(g, w), name
    assert torch.equal(rec.U, got[3]) and torch.equal(rec.D, got[0])


def _stated_pairs(raw, recs, which, twist, n, k):
    """The statement's pieces (which[b] = True: the fallback pair) sampled by ops.farthest_point_sample from the stated start
    indices and passed through datapipe.pairs_from_pieces."""
    from puzzlenet_amd import datapipe as dp, ops
    B = len(recs)
    rows = {False: (0, 1), True: (2, 3)}
    U = np.stack([recs[b]["pieces"][rows[bool(which[b])][0]] for b in range(B)])
    D = np.stack([recs[b]["pieces"][rows[bool(which[b])][1]] for b in range(B)])
    s_u = np.array([recs[b]["start"][rows[bool(which[b])][0]] for b in range(B)], dtype=np.int64)
    s_d = np.array([recs[b]["start"][rows[bool(which[b])][1]] for b in range(B)], dtype=np.int64)
    U, D = _to(U), _to(D)
    Us = ops.index_points(U, ops.farthest_point_sample(U, n, _to(s_u)))
    Ds = ops.index_points(D, ops.farthest_point_sample(D, n, _to(s_d)))
    return dp.pairs_from_pieces(Us, Ds, _to(twist), k)


def test_cut_pairs_fracture_against_the_ops_it_is_made_of():
    from puzzlenet_amd import datapipe as dp
    B, M, P, K, n, k = 4, 4096, 4, 8, 256, 32
    raw, normals, u_anchor, u, twist = _inputs(B, M, P, K, 520)
    u[:, 0] = [0.1, 0.1, 0.9, 0.1]
    pieces = [4, 4, 4, 3]
    recs, _ = fp.batch_statement(raw, normals, u_anchor, u, pieces, n, 0.5, M)
    assert all(r["ok"] for r in recs) and {r["kind"] for r in recs} == {dp.SIBLING, dp.NEIGHBOUR}
    got, ok, rec = dp.cut_pairs_fracture(_to(raw), _to(normals), _to(u_anchor), pieces, _to(u), _to(twist), n=n, k=k, neighbours=0.5)
    torch.cuda.synchronize()
    assert bool(ok.all())
    assert rec.kind.cpu().tolist() == [r["kind"] for r in recs] and rec.pair.cpu().tolist() == [r["pair"].tolist() for r in recs]
    assert rec.label.cpu().numpy().tobytes() == np.stack([r["label"] for r in recs]).tobytes()
    assert rec.planes.cpu().numpy().tobytes() == np.stack([r["planes"] for r in recs]).tobytes()
    rejected = rec.rejected.cpu().numpy()
    print("kinds", rec.kind.cpu().tolist(), "rejected", rejected.tolist(), "cd", rec.cd.cpu().tolist())
    assert not (rejected & (rec.kind.cpu().numpy() != dp.NEIGHBOUR)).any()
    primary = _stated_pairs(raw, recs, [False] * B, twist, n, k)
    assert torch.equal(rec.U, primary[3]) and torch.equal(rec.D, primary[0])
    assert torch.equal(rec.Ub, primary[5]) and torch.equal(rec.Db, primary[4])
    has_fallback = [r["kind"] == dp.NEIGHBOUR for r in recs]
    # (rows without a fallback keep the primary here; they are never compared as a fallback)
    fallback = _stated_pairs(raw, [dict(pieces=r["pieces"] if f else r["pieces"][:2] * 2, start=r["start"] if f else list(r["start"][:2]) * 2)
                                   for r, f in zip(recs, has_fallback)], [True] * B, twist, n, k)
    names = "down moved igt up downb upb down_mask up_mask".split()
    for b in range(B):
        want = fallback if rejected[b] else primary
        for name, g, w in zip(names, got, want):
            assert torch.equal(g[b], w[b]), (b, name, bool(rejected[b]))


def test_acceptance_rule_against_float64():
    """fr.clouds seed 5, draws seed 6, every sample a 4-piece fracture with neighbours = 1.  Chosen on the CPU with the statement,
    the oracle's FPS and a float64 boundary: sample 1 draws the sibling pair; the others are NEIGHBOUR with cd = 0.2771, 0.0045,
    0.1370, 0.0057, 0.0156, 0.0046, 0.0180 - four above 0.015 (rejected), three below (kept), the nearest 6e-4 away."""
    from puzzlenet_amd import datapipe as dp
    B, M, P, K, n, k = 8, 10000, 4, 16, 1024, 128
    raw = fp.clouds(B, M, 5)
    normals, u_anchor, u, twist = fp.draws(B, P, K, 6)
    recs, _ = fp.batch_statement(raw, normals, u_anchor, u, [P] * B, n, 1.0, M)
    assert all(r["ok"] for r in recs) and [r["kind"] for r in recs].count(dp.NEIGHBOUR) == 7
    got, ok, rec = dp.cut_pairs_fracture(_to(raw), _to(normals), _to(u_anchor), P, _to(u), _to(twist), n=n, k=k, neighbours=1.0)
    torch.cuda.synchronize()
    assert bool(ok.all())
    kind, rejected, cd32 = rec.kind.cpu().numpy(), rec.rejected.cpu().numpy(), rec.cd.cpu().numpy()
    assert kind.tolist() == [r["kind"] for r in recs]
    Ub, Db = rec.Ub.cpu().numpy(), rec.Db.cpu().numpy()
    assert Ub.shape == Db.shape == (B, k, 3)
    cd64 = np.array([fp.cd64(Ub[b], Db[b]) for b in range(B)])
    print("cd float64", cd64.tolist(), "max |cd32 - cd64|", float(np.abs(cd32.astype(np.float64) - cd64).max()), "rejected", rejected.tolist())
    assert float(np.abs(cd32.astype(np.float64) - cd64).max()) <= CD_MARGIN
    nb = kind == dp.NEIGHBOUR
    left_out = nb & (np.abs(cd64 - 0.015) < CD_MARGIN)
    assert int(left_out.sum()) * 10 <= int(nb.sum())
    want = nb & (cd64 > 0.015)
    assert np.array_equal(rejected[~left_out], want[~left_out])
    assert rejected.any() and (nb & ~rejected).any()                                  # both outcomes
    # the final pair: the primary where it was kept, the sibling pair where not
    primary = _stated_pairs(raw, recs, [False] * B, twist, n, k)
    assert torch.equal(rec.U, primary[3]) and torch.equal(rec.D, primary[0])
    label = rec.label.cpu().numpy()
    rows = [{r.tobytes(): i for i, r in enumerate(raw[b])} for b in range(B)]
    pair = rec.pair.cpu().numpy()
    for b in range(B):
        lu, ld = (pair[b, 2], pair[b, 3]) if rejected[b] else (pair[b, 0], pair[b, 1])
        assert all(label[b][rows[b][r.tobytes()]] == lu for r in got[3][b].cpu().numpy())
        assert all(label[b][rows[b][r.tobytes()]] == ld for r in got[0][b].cpu().numpy())


def test_fracture_feeder_builds_fresh_batches_and_feeds_the_training_step():
    """Seeds 11 and 5: on the CPU statement every sample of their first five batches has a valid cut at every step."""
    from oracle import model_ref as mr
    from puzzlenet_amd import datapipe as dp, engine
    from puzzlenet_amd import model5_b as mb
    dev = _dev()
    B, M, N = 6, 12000, 1024
    raw = dc.shells(B, M, 21)

    def take(seed, count):
        f = dp.PairFeeder(raw, dev, n=N, seed=seed, pieces=(2, 5))
        assert f._width == 4 * 16 * 4 + 1 + 7 + 6 and f.pieces == (2, 5) and f.neighbours == 0.5
        out = [f.next_batch() for _ in range(count)]
        f.close()
        return out

    a, b = take(11, 3), take(11, 3)
    for x, y in zip(a, b):
        assert all(torch.equal(s, t) for s, t in zip(x, y))                      # same seed, same batches
        assert all(torch.equal(s, t) for s, t in zip(x.fracture, y.fracture))
    assert not torch.equal(a[0][0], a[1][0]) and not torch.equal(a[1][0], a[2][0])      # fresh every time
    rows = [{r.tobytes(): i for i, r in enumerate(raw[s])} for s in range(B)]
    kinds, counts = set(), set()
    for batch in a:
        assert bool(batch.ok.all()) and batch.cut is None and batch.plane is None and batch.double is None
        down, moved, igt, up, downb, upb, down_mask, up_mask = batch
        rec = batch.fracture
        kind, pair, rejected, label = (t.cpu().numpy() for t in (rec.kind, rec.pair, rec.rejected, rec.label))
        planes = rec.planes.cpu().numpy()
        kinds.update(kind.tolist())
        assert planes.shape == (B, 4, 4) and planes.dtype == np.float64 and label.shape == (B, M)
        assert down.shape == up.shape == (B, N, 3)
        assert not (rejected & (kind != dp.NEIGHBOUR)).any()
        for s in range(B):
            n_pieces = int(label[s].max()) + 1
            counts.add(n_pieces)
            assert not planes[s, n_pieces - 1:].any() and planes[s, :n_pieces - 1].any(1).all()
            lu, ld = (pair[s, 2], pair[s, 3]) if rejected[s] else (pair[s, 0], pair[s, 1])
            assert 0 <= lu < n_pieces and 0 <= ld < n_pieces and lu != ld
            # every row is a row of its cloud whose label is the piece `pair` and `rejected` say
            assert all(label[s][rows[s][r.tobytes()]] == lu for r in up[s].cpu().numpy())
            assert all(label[s][rows[s][r.tobytes()]] == ld for r in down[s].cpu().numpy())
        assert float((igt[:, 3] - torch.tensor([0., 0., 0., 1.], device=dev)).abs().max()) == 0
        R = igt[:, :3, :3]
        assert float((R.transpose(1, 2) @ R - torch.eye(3, device=dev)).abs().max()) < 1e-5
        assert float((torch.linalg.det(R.double().cpu()) - 1).abs().max()) < 1e-5
        want = (R @ up.transpose(1, 2) + igt[:, :3, 3:]).transpose(1, 2)
        assert float((moved - want).abs().max()) < 1e-5
        assert bool((down_mask.sum(1) == 128).all()) and bool((up_mask.sum(1) == 128).all())
        assert downb.shape == upb.shape == (B, 128, 3)
    assert len(kinds) > 1 and len(counts) > 1      # (18 samples: both kinds and several piece counts among them)
    feeder = dp.PairFeeder(raw, dev, n=N, seed=5, pieces=(2, 5))
    torch.manual_seed(0)
    model = mb.TouchedRegraster(mr.Cfg(loss_mode=1, num_points=N)).to(dev)
    runner = engine.TrainStep(model, feeder.next_batch(), 1e-3, world=1)
    losses = []
    for _ in range(4):
        losses.append(runner.step(next_batch=feeder.next_batch()))
    torch.cuda.synchronize()
    assert all(np.isfinite(float(l)) for l in losses) and len({round(float(l), 3) for l in losses}) > 1
    assert bool(torch.isfinite(runner.grads.flat).all())
    runner.close()
    feeder.close()


def test_feeder_without_the_argument_is_the_single_cut_feeder():
    """PairFeeder(...) and PairFeeder(..., pieces=None) draw the same numbers in the same order and run the same code."""
    from puzzlenet_amd import datapipe as dp
    dev = _dev()
    raw = dc.shells(6, 5000, 3)
    for seed in (0, 7):
        f, g = dp.PairFeeder(raw, dev, n=1024, seed=seed), dp.PairFeeder(raw, dev, n=1024, seed=seed, pieces=None, neighbours=0.25)
        assert f._width == g._width == f.K * 4 + 8 and g.pieces is None and f._mode is g._mode is dp._PLANE_MODE
        for _ in range(3):
            x, y = f.next_batch(), g.next_batch()
            x.ready.synchronize()      # the tensors are produced on each feeder's own stream: wait for them before
            y.ready.synchronize()      # reading them on this one
            assert all(torch.equal(s, t) for s, t in zip(x, y))
            assert torch.equal(x.ok, y.ok) and all(torch.equal(s, t) for s, t in zip(x.plane, y.plane))
            assert x.fracture is None and y.fracture is None and bool(x.ok.all())
        f.close()
        g.close()


def test_rejections_launch_nothing(monkeypatch):
    from puzzlenet_amd import _lib, datapipe as dp, ops
    calls = []
    monkeypatch.setattr(ops, "_call", lambda *a, **k: calls.append(a[0]))
    B, M, P, K = 2, 64, 3, 3
    raw, normals, u_anchor, u, twist = (_to(t) for t in _inputs(B, M, P, K, 1))
    n17 = torch.zeros((B, 16, K, 3), dtype=torch.float64, device=_dev())
    big = torch.zeros((1, 65537, 3), dtype=torch.float32, device=_dev())
    assert ops.fracture_pair_supported(65536, 16, 1) and not ops.fracture_pair_supported(65537, 2, 1)
    assert not ops.fracture_pair_supported(64, 1, 1) and not ops.fracture_pair_supported(64, 17, 1)
    for bad in (lambda: ops.fracture_pair(raw, n17, n17[..., 0].contiguous(), 2, u, 4, 0.5, M),                    # P = 17
                lambda: ops.fracture_pair(raw, normals[:, :0], u_anchor[:, :0], 2, u, 4, 0.5, M),                  # P = 1
                lambda: ops.fracture_pair(big, normals[:1], u_anchor[:1], 2, u[:1], 4, 0.5, 32768),                # M above the limit
                lambda: dp.cut_pairs_fracture(raw, normals, u_anchor, 2, u, twist, n=16, cap=40000)):              # beyond the FPS limit
        with pytest.raises(_lib.PznUnsupported):
            bad()
    for bad in (lambda: ops.fracture_pair(raw.cpu(), normals, u_anchor, 2, u, 4, 0.5, M),                          # a CPU tensor
                lambda: ops.fracture_pair(raw, normals, u_anchor, 2, u.cpu(), 4, 0.5, M),
                lambda: ops.fracture_pair(raw.double(), normals, u_anchor, 2, u, 4, 0.5, M),                       # wrong dtypes
                lambda: ops.fracture_pair(raw, normals.float(), u_anchor, 2, u, 4, 0.5, M),
                lambda: ops.fracture_pair(raw, normals, u_anchor.float(), 2, u, 4, 0.5, M),
                lambda: ops.fracture_pair(raw, normals, u_anchor, 2, u.float(), 4, 0.5, M),
                lambda: ops.fracture_pair(raw, normals, u_anchor[:, :, :2], 2, u, 4, 0.5, M),                      # K differs
                lambda: ops.fracture_pair(raw, normals, u_anchor, 2, u[:, :6], 4, 0.5, M),                         # six uniforms
                lambda: ops.fracture_pair(raw, normals, u_anchor, 2, u, 4, 0.5, 0),                                # cap = 0
                lambda: ops.fracture_pair(raw, normals, u_anchor, 2, u, 4, 1.5, M),                                # neighbours
                lambda: ops.fracture_pair(raw, normals, u_anchor, 2, u, 4, -0.1, M),
                lambda: ops.fracture_pair(raw, normals, u_anchor, 1, u, 4, 0.5, M),                                # pieces outside 2 .. P
                lambda: ops.fracture_pair(raw, normals, u_anchor, [2, 4], u, 4, 0.5, M),
                lambda: ops.fracture_pair(raw, normals, u_anchor, [2, 3, 3], u, 4, 0.5, M),                        # one count too many
                lambda: ops.fracture_pair(raw, normals, u_anchor, torch.tensor([2.0, 3.0]), u, 4, 0.5, M),         # not integers
                lambda: ops.fracture_pair(raw, normals, u_anchor, torch.zeros(B, dtype=torch.int64, device=_dev()), u, 4, 0.5, M)):
        with pytest.raises(_lib.PznError):
            bad()
    assert calls == []
    ops.fracture_pair(raw, normals, u_anchor, [2, 3], u, 4, 0.5, M)
    assert calls == ["pzn_fracture_pair_f32"]


def test_the_entry_point_refuses_what_the_host_cannot_see():
    """The C entry point refuses the shapes itself; a count outside 2 .. P in DEVICE memory is refused by the launch, per sample:
    kind -1, no piece, ok = 0 - and the sample beside it is cut as if alone."""
    from puzzlenet_amd import _lib, ops
    B, M, P, K = 3, 500, 4, 3
    raw, normals, u_anchor, u, _ = _inputs(B, M, P, K, 7)
    d = [_to(t) for t in (raw, normals, u_anchor, u)]
    p = d[0].data_ptr()
    assert _lib.load().pzn_fracture_pair_f32(p, p, p, p, p, 0.5, B, M, 17, K, 4, M, p, p, p, p, p, p, p, p, p, p, ops._stream()) == -3
    assert _lib.load().pzn_fracture_pair_f32(p, p, p, p, p, 1.5, B, M, P, K, 4, M, p, p, p, p, p, p, p, p, p, p, ops._stream()) == -1
    pieces = np.array([5, 3, 1], dtype=np.int32)
    got = [t.cpu().numpy() for t in ops.fracture_pair(d[0], d[1], d[2], _to(pieces), d[3], 16, 0.5, M)]
    torch.cuda.synchronize()
    _, want = fp.batch_statement(raw[1:2], normals[1:2], u_anchor[1:2], u[1:2], [3], 16, 0.5, M)
    named = dict(zip(fp.NAMES, got))
    for name, w in zip(fp.NAMES, want):
        g = named[name][1::B] if name in ("pieces", "counts", "start") else named[name][1:2]
        assert g.tobytes() == w.tobytes(), name
    for b in (0, 2):
        assert named["kind"][b] == -1 and not named["ok"][b] and named["pair"][b].tolist() == [-1] * 4
        assert (named["counts"][b::B] == -1).all() and not named["start"][b::B].any() and not named["label"][b].any()
        assert not named["planes"][b].any() and not named["target"][b].any() and not named["cand"][b].any()
        assert all(row.tobytes() == raw[b, 0].tobytes() for q in range(4) for row in named["pieces"][q * B + b])
