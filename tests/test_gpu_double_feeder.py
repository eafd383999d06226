"""GPU: the double-cut loader (PairFeeder(split_twice=True); the reference's `train.py --random_slice`, dataset.py:1203-1355).
ops.cut_compact_double (pzn_cut_compact_double_f32: steps 1-7 of datapipe.double_cut_rule in one launch) against that numpy
statement bit for bit; the skipped rows of the background FPS; datapipe.cut_pairs_double against make_pairs_regions (pinned to
the reference by data2.npz) on the statement's recipes; the acceptance test recomputed in float64; the feeder on top."""
import numpy as np
import pytest
import torch

from tests import _double_cut as dc

pytestmark = pytest.mark.gpu

MARGIN = 1e-12      # a point this near a plane may be left out of the comparison (at most 1 per 10 000; these inputs have none)
# |cd (float32, device) - cd (float64, numpy)|: a sample whose float64 cd is this near 0.015 is left out of the acceptance test.
# The device takes squared distances in the reference's expansion form |a|^2 + |b|^2 - 2 a.b in float32: with |p| <= 0.45 on
# these clouds, |a|^2 + |b|^2 <= 0.41 and each of its three roundings (the sum, the product sum, the final fma) is at most
# 2^-24 * 0.41 = 2.4e-8, so a distance is off by <= 7.3e-8, a mean of distances by no more, and cd (two means) by <= 1.5e-7.
# The test prints the difference it finds on its inputs; it has to stay below this bound.
CD_MARGIN = 1.5e-7


def _dev():
    return torch.device("cuda:0")


def _to(x, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(x)).to(_dev())


def _assert_no_point_near_a_plane(raw, planes1, planes2):
    near = 0
    for b in range(raw.shape[0]):
        near += int((dc.margins(raw[b], planes1[b]) < MARGIN).sum()) + int((dc.margins(raw[b], planes2[b]) < MARGIN).sum())
    assert near * 10000 <= raw.shape[0] * raw.shape[1]
    assert near == 0      # (nothing has to be left out)


def _run_and_compare(raw, planes1, planes2, u, n, n_rich, cap):
    from puzzlenet_amd import ops
    got = ops.cut_compact_double(_to(raw), _to(planes1[..., :3]), _to(planes1[..., 3]), _to(planes2[..., :3]), _to(planes2[..., 3]),
                                 _to(u), n, n_rich, cap)
    torch.cuda.synchronize()
    pieces, counts, start, kind, planes, tabs, ok = (t.cpu().numpy() for t in got)
    recs, want = dc.batch_statement(raw, planes1, planes2, u, n, n_rich, cap)
    tag = (n, n_rich, cap)
    assert np.array_equal(kind, want[3]), (tag, kind.tolist(), want[3].tolist())
    assert planes.tobytes() == want[4].tobytes(), tag
    assert np.array_equal(tabs, want[5]), (tag, tabs.tolist(), want[5].tolist())
    assert np.array_equal(counts, want[1]), (tag, counts.tolist(), want[1].tolist())
    assert np.array_equal(start, want[2]), (tag, start.tolist(), want[2].tolist())
    assert np.array_equal(ok, want[6]), (tag, ok.tolist(), want[6].tolist())
    assert pieces.dtype == np.float32 and pieces.tobytes() == want[0].tobytes(), tag
    return recs, want


def _base_inputs():
    """B, M, K = 8, 10000, 8 on origin-centred shells; the seed / se / choice draws set so that every kind occurs."""
    B, M, K = 8, 10000, 8
    raw = dc.shells(B, M, 3)
    planes1, planes2, u = dc.draws(B, K, 31)
    u[:, 0] = [0.1, 0.5, 0.5, 0.5, 0.9, 0.9, 0.5, 0.9]      # seed 0, 1, 1, 1, 2, 2, 1, 2
    u[:, 1] = [0.5, 0.1, 0.5, 0.9, 0.1, 0.5, 0.5, 0.9]      # se   -, 0, 1, 2, 0, 1, 1, 2
    u[:, 2] = [0.2, 0.2, 0.7, 0.2, 0.7, 0.2, 0.2, 0.7]      # choice
    planes1[4:, 0, 3] = 0.0      # (a first plane through the centre: `down` is rich too, so that seed 2 cuts it)
    return raw, planes1, planes2, u


def test_double_cut_kernel_against_the_statement():
    from puzzlenet_amd import datapipe as dp
    raw, planes1, planes2, u = _base_inputs()
    B, M, _ = raw.shape
    _assert_no_point_near_a_plane(raw, planes1, planes2)
    for cap in (M, 7000):
        recs, want = _run_and_compare(raw, planes1, planes2, u, 1024, 3000, cap)
    kinds = [r["kind"] for r in recs]
    print("kinds", kinds, "counts", want[1].reshape(4, B).T.tolist())
    assert set(kinds) == {dp.SINGLE, dp.HALF_VS_REST, dp.HALF_VS_OTHER, dp.HALVES}       # every kind occurs
    assert any(r["d_tab"][1] != 0 for r in recs)                                          # a two-region piece among them
    # the first three plane-2 candidates pushed off the cloud: the re-draw
    off3 = planes2.copy()
    off3[:, :3, 3] = 5.0
    _assert_no_point_near_a_plane(raw, planes1, off3)
    for cap in (M, 7000):
        recs3, _ = _run_and_compare(raw, planes1, off3, u, 1024, 3000, cap)
    twice = [b for b, r in enumerate(recs3) if r["kind"] != dp.SINGLE]
    assert twice and all(any(np.array_equal(recs3[b]["planes"][1], off3[b, t]) for t in range(3, 7)) for b in twice)
    # all seven pushed off: the single cut everywhere
    off7 = planes2.copy()
    off7[:, :, 3] = 5.0
    for cap in (M, 7000):
        recs7, _ = _run_and_compare(raw, planes1, off7, u, 1024, 3000, cap)
    assert all(r["kind"] == dp.SINGLE and not r["planes"][1].any() for r in recs7)


def test_double_cut_kernel_odd_shape():
    B, M, K = 3, 777, 4
    raw = dc.shells(B, M, 9)
    planes1, planes2, u = dc.draws(B, K, 77)
    u[:, 0], u[:, 1] = [0.5, 0.9, 0.5], [0.1, 0.5, 0.9]
    _assert_no_point_near_a_plane(raw, planes1, planes2)
    recs, _ = _run_and_compare(raw, planes1, planes2, u, 50, 150, M)
    print("kinds", [r["kind"] for r in recs])
    _run_and_compare(raw, planes1, planes2, u, 50, 150, 400)
    # no plane-1 candidate valid: ok = 0 and the most balanced one
    far, u0 = planes1.copy(), u.copy()
    far[:, :, 3] = 0.2 - 0.02 * np.arange(K)      # a sliver of `down` at most
    u0[:, 0] = 0.1
    _assert_no_point_near_a_plane(raw, far, planes2)
    recs, want = _run_and_compare(raw, far, planes2, u0, 300, 150, M)
    assert not want[6].any() and all(r["kind"] == 0 for r in recs)


@pytest.mark.parametrize("P, cap, npoint", [(8, 5000, 1024), (5, 1500, 256), (3, 9000, 64)])
def test_background_fps_skips_pieces_that_do_not_exist(P, cap, npoint):
    """counts = -1: index 0 everywhere, no rounds; the other rows as the same call without the skipped samples gives them.
    P even: pieces p and p + P / 2 (the two pieces of a sample) share a workgroup - samples 1 and 3 are skipped whole, and sample 0
    has one piece skipped beside a real one (it then counts as one row)."""
    from puzzlenet_amd import ops
    rng = np.random.RandomState(P)
    pieces = rng.rand(P, cap, 3).astype(np.float32)
    counts = rng.randint(npoint + 50, cap + 1, size=P).astype(np.int64)
    start = np.array([rng.randint(0, c) for c in counts], dtype=np.int64)
    if P % 2 == 0:
        skipped = [1, 1 + P // 2, 3, 3 + P // 2]
        half_skipped = [P // 2]
    else:
        skipped, half_skipped = [p for p in (1, 3) if p < P], []
    for p in skipped + half_skipped:
        counts[p], start[p] = -1, 0
    for p in range(P):
        pieces[p, max(int(counts[p]), 1):] = pieces[p, 0]      # padding: copies of the first row
    got = ops.farthest_point_sample(_to(pieces), npoint, _to(start), background=True, counts=_to(counts), max_count=cap)
    keep = [p for p in range(P) if p not in skipped]
    kept_counts = counts[keep].copy()
    kept_counts[kept_counts < 0] = 1
    want = ops.farthest_point_sample(_to(pieces[keep]), npoint, _to(start[keep]), background=True, counts=_to(kept_counts), max_count=cap)
    torch.cuda.synchronize()
    got, want = got.cpu().numpy(), want.cpu().numpy()
    assert np.array_equal(got[keep], want)
    assert not got[skipped + half_skipped].any()
    real = [p for p in keep if p not in half_skipped]
    assert all(len(set(got[p].tolist())) == npoint and got[p].max() < counts[p] for p in real)      # (real rows: real picks)


def _recipes(recs, which):
    """The statement's pieces as make_pairs_regions arguments; which[b] = True: the fallback pair of plane 1 alone."""
    from puzzlenet_amd import datapipe as dp
    B = len(recs)
    planes = np.stack([r["planes"] for r in recs])
    u_tab = np.array([(dp.UP, 0) if which[b] else recs[b]["u_tab"] for b in range(B)], dtype=np.int64)
    d_tab = np.array([(dp.DOWN, 0) if which[b] else recs[b]["d_tab"] for b in range(B)], dtype=np.int64)
    s_u = np.array([recs[b]["start"][2 if which[b] else 0] for b in range(B)], dtype=np.int64)
    s_d = np.array([recs[b]["start"][3 if which[b] else 1] for b in range(B)], dtype=np.int64)
    return planes, u_tab, d_tab, s_u, s_d


def _regions(raw, recs, which, twist, n):
    from puzzlenet_amd import datapipe as dp
    planes, u_tab, d_tab, s_u, s_d = _recipes(recs, which)
    out, ok = dp.make_pairs_regions(_to(raw), _to(planes[:, 0, :3]), _to(planes[:, 0, 3]), _to(planes[:, 1, :3]), _to(planes[:, 1, 3]),
                                    _to(u_tab), _to(d_tab), _to(s_u), _to(s_d), _to(twist), n=n)
    assert bool(ok.all())
    return out


def _twists(B, seed):
    x = np.random.RandomState(seed).randn(B, 6)
    return (x / np.linalg.norm(x, axis=1, keepdims=True) * 0.8).astype(np.float32)


def _cut_pairs_double(raw, planes1, planes2, u, twist, n):
    from puzzlenet_amd import datapipe as dp
    out = dp.cut_pairs_double(_to(raw), _to(planes1[..., :3]), _to(planes1[..., 3]), _to(planes2[..., :3]), _to(planes2[..., 3]),
                              _to(u), _to(twist), n=n)
    torch.cuda.synchronize()
    return out


def _compare_tuples(got, want, rows):
    """The project's bounds for this path: pieces bit for bit, igt and moved to 1e-6, masks within 2
    labels per cloud."""
    D, moved, igt, U, Db, Ub, Dm, Um = (t[rows] for t in got)
    wD, wmoved, wigt, wU, wDb, wUb, wDm, wUm = (t[rows] for t in want)
    assert torch.equal(U, wU) and torch.equal(D, wD)
    assert float((igt - wigt).abs().max()) <= 1e-6 and float((moved - wmoved).abs().max()) <= 1e-6
    assert int((Dm != wDm).sum(1).max()) <= 2 and int((Um != wUm).sum(1).max()) <= 2
    assert bool((Dm.sum(1) == 128).all()) and bool((Um.sum(1) == 128).all())


def test_cut_pairs_double_against_make_pairs_regions():
    """The same draws through cut_pairs_double and through make_pairs_regions on the statement's recipes."""
    raw, planes1, planes2, u = _base_inputs()
    B, n = raw.shape[0], 1024
    twist = _twists(B, 5)
    recs, _ = dc.batch_statement(raw, planes1, planes2, u, n, 3000, raw.shape[1])
    got, ok, rec = _cut_pairs_double(raw, planes1, planes2, u, twist, n)
    assert bool(ok.all())
    assert np.array_equal(rec.kind.cpu().numpy(), [r["kind"] for r in recs])
    primary = _regions(raw, recs, [False] * B, twist, n)
    assert torch.equal(rec.U, primary[3]) and torch.equal(rec.D, primary[0])      # the primary pair, bit for bit
    rejected = rec.rejected.cpu().numpy()
    print("rejected", rejected.tolist(), "cd", rec.cd.cpu().numpy().tolist())
    final = primary if not rejected.any() else _regions(raw, recs, rejected.tolist(), twist, n)
    _compare_tuples(got, final, torch.arange(B, device=_dev()))


def _acceptance_inputs():
    """All samples HALF_VS_OTHER (seed 1, se 1).  Even samples: plane 2 parallel to plane 1 at signed distance 0.12 / |normal|
    = 0.137 inside `up`, so the far half (choice 0: U = uppc) lies >= 0.137 from `down`: cd >= 2 * 0.137^2 = 0.037 > 0.015, while
    the near half (choice 1) touches it.  Odd samples: a plane 2 across plane 1, so that either half touches `down`.
    Chosen on the CPU with the statement, the oracle's FPS and a numpy chamfer: cd = 0.0649 for samples 0 and 4 (rejected),
    0.0007 .. 0.0052 for the other six (kept); none is near 0.015."""
    B, M, K = 8, 10000, 4
    raw = dc.shells(B, M, 3)
    planes1, planes2, u = dc.draws(B, K, 41)
    planes1[:, 0] = (0.5, 0.6, 0.4, 0.02)
    planes2[0::2, 0] = (0.5, 0.6, 0.4, -0.12)
    planes2[1::2, 0] = (1.0, 0.0, 0.05, 0.0)
    u[:, 0], u[:, 1] = 0.5, 0.5
    u[:, 2] = [0.2, 0.2, 0.7, 0.7, 0.2, 0.7, 0.7, 0.2]
    return raw, planes1, planes2, u


def test_acceptance_rule_against_float64():
    from puzzlenet_amd import datapipe as dp
    raw, planes1, planes2, u = _acceptance_inputs()
    B, n = raw.shape[0], 1024
    twist = _twists(B, 6)
    recs, _ = dc.batch_statement(raw, planes1, planes2, u, n, 3000, raw.shape[1])
    assert all(r["kind"] == dp.HALF_VS_OTHER for r in recs)
    got, ok, rec = _cut_pairs_double(raw, planes1, planes2, u, twist, n)
    assert bool(ok.all())
    kind, rejected, cd32 = rec.kind.cpu().numpy(), rec.rejected.cpu().numpy(), rec.cd.cpu().numpy()
    Ub, Db = rec.Ub.cpu().numpy(), rec.Db.cpu().numpy()
    assert Ub.shape == Db.shape == (B, 128, 3)
    cd64 = np.array([dc.chamfer_cd(Db[b], Ub[b]) for b in range(B)])
    print("cd float64", cd64.tolist(), "max |cd32 - cd64|", float(np.abs(cd32.astype(np.float64) - cd64).max()), "rejected", rejected.tolist())
    assert float(np.abs(cd32.astype(np.float64) - cd64).max()) <= CD_MARGIN
    hvo = kind == dp.HALF_VS_OTHER
    left_out = hvo & (np.abs(cd64 - 0.015) < CD_MARGIN)
    assert int(left_out.sum()) * 10 <= int(hvo.sum())
    want = hvo & (cd64 > 0.015)
    assert np.array_equal(rejected[~left_out], want[~left_out])
    assert rejected.any() and (hvo & ~rejected).any()                                 # both outcomes
    # the final pair: the primary where it was kept, the fallback pieces sampled from their own start indices where not
    primary, fallback = _regions(raw, recs, [False] * B, twist, n), _regions(raw, recs, [True] * B, twist, n)
    rej = torch.from_numpy(rejected).to(_dev())
    assert torch.equal(rec.U, primary[3]) and torch.equal(rec.D, primary[0])
    _compare_tuples(got, fallback, rej.nonzero().flatten())
    _compare_tuples(got, primary, (~rej).nonzero().flatten())


def _feeder_clouds(B=6, M=12000):
    return dc.shells(B, M, 21)


def test_double_feeder_builds_fresh_batches_and_feeds_the_training_step():
    from oracle import model_ref as mr
    from puzzlenet_amd import datapipe as dp, engine
    from puzzlenet_amd import model5_b as mb
    dev = _dev()
    B, M, N = 6, 12000, 1024
    raw = _feeder_clouds(B, M)

    def take(seed, count):
        f = dp.PairFeeder(raw, dev, n=N, seed=seed, candidates=16, split_twice=True)
        assert f._width == (16 + 7) * 4 + 7 + 6
        out = [f.next_batch() for _ in range(count)]
        f.close()
        return out

    a, b = take(11, 3), take(11, 3)
    for x, y in zip(a, b):
        assert all(torch.equal(s, t) for s, t in zip(x, y))                      # same seed, same batches
        assert all(torch.equal(s, t) for s, t in zip(x.double, y.double))
    assert not torch.equal(a[0][0], a[1][0]) and not torch.equal(a[1][0], a[2][0])      # fresh every time
    rows = [{r.tobytes() for r in raw[s]} for s in range(B)]
    seen = set()
    for batch in a:
        assert bool(batch.ok.all()) and batch.cut is None
        down, moved, igt, up, downb, upb, down_mask, up_mask = batch
        d = batch.double
        kind, planes, tabs, rejected = d.kind.cpu().numpy(), d.planes.cpu().numpy(), d.tabs.cpu().numpy(), d.rejected.cpu().numpy()
        seen.update(kind.tolist())
        assert planes.shape == (B, 2, 4) and planes.dtype == np.float64 and tabs.shape == (B, 4)
        assert torch.equal(batch.plane[0], d.planes[:, 0, :3]) and torch.equal(batch.plane[1], d.planes[:, 0, 3])
        assert down.shape == up.shape == (B, N, 3)
        for s in range(B):
            u_np, d_np = up[s].cpu().numpy(), down[s].cpu().numpy()
            assert all(r.tobytes() in rows[s] for r in u_np) and all(r.tobytes() in rows[s] for r in d_np)
            # every row lies in the cells its piece's tables name (the pair of plane 1 alone where the pair was rejected)
            u_tab, d_tab = ((dp.UP, 0), (dp.DOWN, 0)) if rejected[s] else (tabs[s, :2], tabs[s, 2:])
            for pts, tab in ((u_np, u_tab), (d_np, d_tab)):
                code = 2 * dp._side64(pts, planes[s, 0]).astype(np.int64) + dp._side64(pts, planes[s, 1]).astype(np.int64)
                assert ((((int(tab[0]) | int(tab[1])) >> code) & 1) == 1).all()
            if kind[s] == dp.SINGLE:
                assert not planes[s, 1].any() and tuple(tabs[s]) == (dp.UP, 0, dp.DOWN, 0)
        assert not (rejected & (kind != dp.HALF_VS_OTHER)).any()
        assert float((igt[:, 3] - torch.tensor([0., 0., 0., 1.], device=dev)).abs().max()) == 0
        R = igt[:, :3, :3]
        assert float((R.transpose(1, 2) @ R - torch.eye(3, device=dev)).abs().max()) < 1e-5
        assert float((torch.linalg.det(R.double().cpu()) - 1).abs().max()) < 1e-5
        want = (R @ up.transpose(1, 2) + igt[:, :3, 3:]).transpose(1, 2)
        assert float((moved - want).abs().max()) < 1e-5
        assert bool((down_mask.sum(1) == 128).all()) and bool((up_mask.sum(1) == 128).all())
        assert downb.shape == upb.shape == (B, 128, 3)
    assert len(seen) > 1      # (18 samples: more than one kind of cut among them)
    feeder = dp.PairFeeder(raw, dev, n=N, seed=5, candidates=16, split_twice=True)
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
    """PairFeeder(...) and PairFeeder(..., split_twice=False) draw the same numbers in the same order and run the same code."""
    from puzzlenet_amd import datapipe as dp
    dev = _dev()
    raw = dc.shells(6, 5000, 3)
    for seed in (0, 7):
        f, g = dp.PairFeeder(raw, dev, n=1024, seed=seed), dp.PairFeeder(raw, dev, n=1024, seed=seed, split_twice=False)
        assert f._width == g._width == f.K * 4 + 8 and f.split_twice is False
        for _ in range(3):
            x, y = f.next_batch(), g.next_batch()
            x.ready.synchronize()      # the tensors are produced on each feeder's own stream: wait for them before
            y.ready.synchronize()      # reading them on this one
            assert all(torch.equal(s, t) for s, t in zip(x, y))
            assert torch.equal(x.ok, y.ok) and all(torch.equal(s, t) for s, t in zip(x.plane, y.plane))
            assert x.double is None and y.double is None and bool(x.ok.all())
        f.close()
        g.close()
