"""GPU: the solid-cut loader.  ops.cut_compact_solid (pzn_cut_compact_solid_f32: sphere / cylinder / cone cut with re-draw,
stable partition, padding, start indices in one launch) against the numpy statement of the same thing on the ORACLE's masks
(oracle/solids.py: open3d 0.15.2's resolution-50 meshes restated, brute-force face-plane membership), bit for bit; then
datapipe.PairFeeder(cut=kind) on top of it, and the default plane path left as it was."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

KINDS = ["sphere", "cylinder", "cone"]
SEEDS = {"sphere": 101, "cylinder": 102, "cone": 103}
MARGIN = 1e-9      # a point whose decisive margin is below this may be left out of the mask comparison (at most 1 per 10 000)


def _face_planes(kind, rot, shift):
    """Outward unit normals n_f and offsets d_f of the moved mesh's triangles (inside: n_f . p < d_f for every f)."""
    from oracle import solids
    V, T = solids.solid_mesh(kind, rot, shift)
    a, b, c = V[T[:, 0]], V[T[:, 1]], V[T[:, 2]]
    n = np.cross(b - a, c - a)
    keep = np.linalg.norm(n, axis=1) > 0
    a, n = a[keep], n[keep]
    n = n * np.sign(np.einsum("fi,fi->f", n, a - V.mean(axis=0)))[:, None]
    n = n / np.linalg.norm(n, axis=1, keepdims=True)
    return n, np.einsum("fi,fi->f", n, a)


def _oracle(points, kind, rot, shift):
    """-> (the oracle's up-mask [M], each point's decisive margin |min_f (d_f - n_f . p)| [M]); numpy float64 on the CPU."""
    from oracle import solids
    P = points.astype(np.float64)
    n, d = _face_planes(kind, rot, shift)
    slack = np.full(len(P), np.inf)
    for s in range(0, len(n), 512):
        slack = np.minimum(slack, (d[s:s + 512] - P @ n[s:s + 512].T).min(axis=1))
    mask = solids.solid_cut_mask(P, kind, rot, shift)
    assert np.array_equal(mask, slack > 0)
    return mask, np.abs(slack)


def _inputs(kind, B, M, K, seed):
    rng = np.random.default_rng(seed)
    raw = rng.random((B, M, 3))
    if kind == "cone":
        raw = raw * 1.6 - 0.8
    raw = raw.astype(np.float32)
    params = np.zeros((B, K, 6))
    for b in range(B):
        for k in range(K):
            params[b, k, :3] = rng.random(3)
            params[b, k, 3:] = rng.random(3) / 3
    u = rng.random((B, 2))
    return raw, params, u


_MASKS = {}


def _masks(tag, raw, kind, params):
    """The oracle's masks [B,K,M] and margins for every candidate (cached per cloud and candidate: the brute force over the
    sphere's 9800 triangles is the slow part)."""
    B, K = params.shape[:2]
    for b in range(B):
        for k in range(K):
            key = (kind, tag, b, params[b, k].tobytes())
            if key not in _MASKS:
                _MASKS[key] = _oracle(raw[b], kind, params[b, k, :3], params[b, k, 3:])
    got = [[_MASKS[(kind, tag, b, params[b, k].tobytes())] for k in range(K)] for b in range(B)]
    return np.array([[g[0] for g in row] for row in got]), np.array([[g[1] for g in row] for row in got])


def _statement(raw, masks, params, u, n_min, cap):
    """numpy: first valid candidate by the oracle's masks, else the most balanced (first among equals); stable partition;
    padding with the piece's first row (the cloud's first row for an empty piece); start = clamp(floor(u count), 0, count - 1)."""
    B, M, _ = raw.shape
    K = params.shape[1]
    pieces = np.zeros((2 * B, cap, 3), dtype=np.float32)
    counts, start = np.zeros(2 * B, dtype=np.int64), np.zeros(2 * B, dtype=np.int64)
    chosen, chosen_k, ok = np.zeros((B, 6)), np.zeros(B, dtype=np.int32), np.zeros(B, dtype=bool)
    for b in range(B):
        pick, best = None, (-1, 0)
        for k in range(K):
            up = int(masks[b, k].sum())
            if min(up, M - up) > best[0]:
                best = (min(up, M - up), k)
            if up >= n_min and M - up >= n_min:
                pick = k
                break
        valid = pick is not None
        pick = pick if valid else best[1]
        m = masks[b, pick]
        chosen[b], chosen_k[b] = params[b, pick], pick
        for half, rows in ((0, raw[b][m]), (1, raw[b][~m])):
            cnt = len(rows)
            counts[half * B + b] = cnt
            first = rows[0] if cnt else raw[b][0]
            pieces[half * B + b] = first
            pieces[half * B + b, :min(cnt, cap)] = rows[:cap]
            start[half * B + b] = max(0, min(cnt - 1, int(np.floor(u[b, half] * cnt))))
        ok[b] = valid and counts[b] <= cap and counts[B + b] <= cap
    return pieces, counts, start, chosen, chosen_k, ok


def _run_and_compare(kind, raw, params, u, masks, n_min, cap):
    from puzzlenet_amd import ops
    dev = torch.device("cuda:0")
    got = ops.cut_compact_solid(torch.from_numpy(raw).to(dev), kind, torch.from_numpy(params).to(dev),
                                torch.from_numpy(u).to(dev), n_min, cap)
    torch.cuda.synchronize()
    pieces, counts, start, chosen, chosen_k, ok = (t.cpu().numpy() for t in got)
    want = _statement(raw, masks, params, u, n_min, cap)
    tag = (kind, n_min, cap)
    assert np.array_equal(chosen_k, want[4]), (tag, chosen_k.tolist(), want[4].tolist(), counts.tolist(), want[1].tolist())
    assert chosen.tobytes() == want[3].tobytes(), tag
    assert np.array_equal(counts, want[1]), (tag, counts.tolist(), want[1].tolist())
    assert np.array_equal(ok, want[5]), (tag, ok.tolist(), want[5].tolist())
    assert np.array_equal(start, want[2]), (tag, start.tolist(), want[2].tolist())
    assert pieces.tobytes() == want[0].tobytes(), tag
    return want


def _kernel_masks(kind, raw, params, u):
    """The kernel's own membership of every candidate, read off its output: with ONE candidate and n_min = 0 the candidate is
    taken whatever it is, and the up piece is the inside rows in order."""
    from puzzlenet_amd import ops
    dev = torch.device("cuda:0")
    B, M, _ = raw.shape
    K = params.shape[1]
    out = np.zeros((B, K, M), dtype=bool)
    raw_d, u_d = torch.from_numpy(raw).to(dev), torch.from_numpy(u).to(dev)
    for k in range(K):
        pieces, counts, *_ = ops.cut_compact_solid(raw_d, kind, torch.from_numpy(params[:, k:k + 1].copy()).to(dev), u_d, 0, M)
        pieces, counts = pieces.cpu().numpy(), counts.cpu().numpy()
        for b in range(B):
            # stable partition: walk the cloud and the up piece together
            up_rows, at = pieces[b, :counts[b]], 0
            for j in range(M):
                if at < len(up_rows) and raw[b, j].tobytes() == up_rows[at].tobytes():
                    out[b, k, j], at = True, at + 1
            assert at == len(up_rows)
    return out


@pytest.mark.parametrize("kind", KINDS)
def test_solid_cut_kernel_against_the_oracle(kind):
    """B, M, K = 4, 10000, 8, the stated draws.  Masks: equal to the oracle's point for point, but for points whose decisive
    margin is below 1e-9 (at most one per 10 000: for these inputs the smallest margins are 7.7e-8 / 1.5e-6 / 2.2e-7, so
    none).  Then chosen candidate, parameters, counts, ok, start and both pieces with their padding, bit for bit, for
    n_min = 1024 / 2048 and cap = M / 7000; with the first three candidates made empty (the re-draw), and with all of them
    made empty (ok = 0, the most balanced one taken)."""
    B, M, K = 4, 10000, 8
    raw, params, u = _inputs(kind, B, M, K, SEEDS[kind])
    masks, margin = _masks("base", raw, kind, params)
    print(f"{kind}: smallest decisive margin {margin.min():.3g}, n_up of sample 0 {masks[0].sum(1).tolist()}")
    got = _kernel_masks(kind, raw, params, u)
    differ = got != masks
    left_out = margin < MARGIN
    print(f"{kind}: {int(differ.sum())} of {differ.size} memberships differ, {int(left_out.sum())} left out")
    assert int(left_out.sum()) * 10000 <= differ.size
    assert not (differ & ~left_out).any()
    assert not left_out.any() and not differ.any()      # (these inputs: nothing is near a face)
    for n_min in (1024, 2048):
        for cap in (M, 7000):
            _run_and_compare(kind, raw, params, u, masks, n_min, cap)
    if kind == "cone":      # (the cone ignores shift: no way to empty it by a translation)
        return
    for first in (3, K):
        far = params.copy()
        far[:, :first, 3:] = 5.0
        far_masks, _ = _masks("base", raw, kind, far)
        assert not far_masks[:, :first].any()
        for n_min in (1024, 2048):
            for cap in (M, 7000):
                want = _run_and_compare(kind, raw, far, u, far_masks, n_min, cap)
                if first == K:
                    assert not want[5].any() and (want[4] == 0).all() and (want[1][:B] == 0).all()
                else:
                    assert (want[4] >= 3).all()


@pytest.mark.parametrize("kind", KINDS)
def test_solid_cut_kernel_odd_shape(kind):
    B, M, K = 3, 777, 4
    raw, params, u = _inputs(kind, B, M, K, SEEDS[kind] + 1000)
    masks, margin = _masks("odd", raw, kind, params)
    assert margin.min() >= MARGIN
    _run_and_compare(kind, raw, params, u, masks, 50, M)


@pytest.mark.parametrize("kind", ["cylinder", "cone"])
def test_solid_cut_kernel_runs_longer_than_the_register_mask(kind):
    """M > 65536: a thread's run no longer fits the 64-bit mask and the chosen candidate is evaluated again."""
    B, M, K = 1, 70001, 2
    raw, params, u = _inputs(kind, B, M, K, SEEDS[kind] + 2000)
    masks, margin = _masks("long", raw, kind, params)
    assert int((margin < MARGIN).sum()) * 10000 <= margin.size and margin.min() >= MARGIN
    _run_and_compare(kind, raw, params, u, masks, 20000, M)
    _run_and_compare(kind, raw, params, u, masks, 1024, 40000)


def _raw_clouds(kind, B=6, M=12000):
    rng = np.random.default_rng({"sphere": 1, "cylinder": 2, "cone": 3}[kind])
    return (rng.random((B, M, 3)) * (1.6 if kind == "cone" else 1.0) - (0.8 if kind == "cone" else 0.0)).astype(np.float32)


@pytest.mark.parametrize("kind", KINDS)
def test_solid_feeder_builds_fresh_batches_and_feeds_the_training_step(kind):
    """PairFeeder(cut=kind): reproducible from the seed, a fresh cut per batch, every `up` point inside and every `down` point
    outside the solid of batch.cut by the oracle, every sampled row a row of the raw cloud, 128-point masks, a rigid motion;
    and TrainStep.step(next_batch=...) trains on the batches."""
    from oracle import model_ref as mr
    from oracle import solids
    from puzzlenet_amd import datapipe, engine
    from puzzlenet_amd import model5_b as mb
    dev = torch.device("cuda:0")
    B, M, N = 6, 12000, 1024
    raw = _raw_clouds(kind, B, M)

    def take(seed, count):
        f = datapipe.PairFeeder(raw, dev, n=N, seed=seed, candidates=16, cut=kind)
        out = [f.next_batch() for _ in range(count)]
        f.close()
        return out

    a, b = take(11, 3), take(11, 3)
    for x, y in zip(a, b):
        assert all(torch.equal(s, t) for s, t in zip(x, y))                      # same seed, same batches
        assert all(torch.equal(s, t) for s, t in zip(x.cut[1:], y.cut[1:]))
    assert not torch.equal(a[0][0], a[1][0]) and not torch.equal(a[1][0], a[2][0])      # a fresh cut every time
    rows = [{r.tobytes() for r in raw[s]} for s in range(B)]
    for batch in a:
        assert bool(batch.ok.all())
        assert batch.plane is None and batch.cut[0] == kind
        down, moved, igt, up, downb, upb, down_mask, up_mask = batch
        rot, shift = batch.cut[1].cpu().numpy(), batch.cut[2].cpu().numpy()
        assert rot.shape == shift.shape == (B, 3) and rot.dtype == np.float64
        assert down.shape == up.shape == (B, N, 3)
        for s in range(B):
            u_np, d_np = up[s].cpu().numpy(), down[s].cpu().numpy()
            assert solids.solid_cut_mask(u_np, kind, rot[s], shift[s]).all()
            assert not solids.solid_cut_mask(d_np, kind, rot[s], shift[s]).any()
            assert all(r.tobytes() in rows[s] for r in u_np) and all(r.tobytes() in rows[s] for r in d_np)
        assert float((igt[:, 3] - torch.tensor([0., 0., 0., 1.], device=dev)).abs().max()) == 0
        R = igt[:, :3, :3]
        assert float((R.transpose(1, 2) @ R - torch.eye(3, device=dev)).abs().max()) < 1e-5
        assert float((torch.linalg.det(R.double().cpu()) - 1).abs().max()) < 1e-5
        want = (R @ up.transpose(1, 2) + igt[:, :3, 3:]).transpose(1, 2)
        assert float((moved - want).abs().max()) < 1e-5
        assert bool((down_mask.sum(1) == 128).all()) and bool((up_mask.sum(1) == 128).all())
        assert downb.shape == upb.shape == (B, 128, 3)
    feeder = datapipe.PairFeeder(raw, dev, n=N, seed=5, candidates=16, cut=kind)
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


def test_default_feeder_is_the_plane_feeder():
    """PairFeeder(...) and PairFeeder(..., cut="plane") draw the same numbers in the same order and run the same code."""
    from puzzlenet_amd import datapipe
    dev = torch.device("cuda:0")
    B, M, N = 6, 5000, 1024
    rng = np.random.RandomState(3)
    v = rng.randn(B, M, 3).astype(np.float32)
    v /= np.linalg.norm(v, axis=2, keepdims=True)
    raw = v * (0.25 + 0.2 * rng.rand(B, 1, 3).astype(np.float32))
    for seed in (0, 7):
        f, g = datapipe.PairFeeder(raw, dev, n=N, seed=seed), datapipe.PairFeeder(raw, dev, n=N, seed=seed, cut="plane")
        assert f._width == g._width == f.K * 4 + 8
        for _ in range(3):
            x, y = f.next_batch(), g.next_batch()
            x.ready.synchronize()      # the tensors are produced on each feeder's own stream: wait for them before
            y.ready.synchronize()      # reading them on this one
            assert all(torch.equal(s, t) for s, t in zip(x, y))
            assert torch.equal(x.ok, y.ok) and all(torch.equal(s, t) for s, t in zip(x.plane, y.plane))
            assert x.cut is None and y.cut is None and bool(x.ok.all())
        f.close()
        g.close()
