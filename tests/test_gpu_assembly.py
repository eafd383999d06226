"""GPU: puzzlenet_amd.assembly - the all-pairs table with every piece encoded once (match_pairs) against the oracle's
literal predict5 on the materialised pair batch, its fallback path, and the walk from pieces to an assembled cloud."""
import numpy as np
import pytest
import torch

from oracle import model_ref as mr

pytestmark = pytest.mark.gpu

K, N, TOP = 5, 1024, 128


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _rel(a, b):
    a = a.detach().cpu().double()
    b = b.detach().cpu().double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _close(got, want, rtol, atol, msg=""):
    np.testing.assert_allclose(got.detach().cpu().numpy(), want.detach().cpu().numpy(), rtol=rtol, atol=atol, err_msg=msg)


def _fps_from(queue):
    """oracle.model_ref.farthest_point_sample with the start vector taken from `queue` instead of drawn."""
    def fps(xyz, npoint):
        B, n, _ = xyz.shape
        centroids = torch.zeros(B, npoint, dtype=torch.long)
        distance = torch.ones(B, n) * 1e10
        farthest = queue.pop(0).clone()
        assert farthest.shape == (B,) and int(farthest.max()) < n
        batch_indices = torch.arange(B, dtype=torch.long)
        for i in range(npoint):
            centroids[:, i] = farthest
            centroid = xyz[batch_indices, farthest, :].view(B, 1, 3)
            dist = torch.sum((xyz - centroid) ** 2, -1)
            distance = torch.min(distance, dist)
            farthest = torch.max(distance, -1)[1]
        return centroids
    return fps


@pytest.fixture(scope="module")
def case(dev):
    """Seeded pieces in the unit cube, the device's table for them and the oracle's predict5 (eval) on the 25-row pair
    batch fpc = pieces[I], mrpc = pieces[J]; computed once, read by every test below."""
    from puzzlenet_amd import assembly, model5_b as mb
    g = torch.Generator().manual_seed(2718)
    pieces = torch.rand(K, N, 3, generator=g)
    s1 = torch.randint(0, N, (K,), generator=g)
    s2 = torch.randint(0, 512, (K,), generator=g)
    I = torch.arange(K).repeat_interleave(K)
    J = torch.arange(K).repeat(K)

    m = mb.TouchedRegraster(mr.Cfg())
    mr.fill_params(m)
    m.to(dev)
    table = assembly.match_pairs(m, pieces.to(dev), k=TOP, start=(s1, s2))

    ref = mr.RefModel(mr.Cfg())
    mr.fill_params(ref)
    queue = [s1[I], s2[I], s1[J], s2[J]]      # Encoder sg1, sg2, then Encoder2 sg1, sg2
    mp = pytest.MonkeyPatch()
    mp.setattr(mr, "farthest_point_sample", _fps_from(queue))
    try:
        with torch.no_grad():
            out, _, x2_f, _, x2_m, _, de_fpcb, de_mrpcb = ref.predict5([pieces[I], pieces[J]], training=False)
    finally:
        mp.undo()
    assert not queue
    oracle = dict(out=out, x2_f=x2_f, x2_m=x2_m, de_fpcb=de_fpcb, de_mrpcb=de_mrpcb)
    return dict(model=m, pieces=pieces, start=(s1, s2), I=I, J=J, table=table, oracle=oracle)


def test_match_pairs_vs_oracle_predict5(case):
    t, o, I, J = case["table"], case["oracle"], case["I"], case["J"]
    assert t.twist.shape == (K, K, 6) and t.T.shape == (K, K, 4, 4)
    assert t.de_fpcb.shape == (K, K, 2, N) and t.de_mrpcb.shape == (K, 2, N)
    assert t.top_f.shape == (K, K, TOP) and t.top_m.shape == (K, TOP) and t.top_f.dtype == torch.int64
    # bounds of tests/test_gpu_model.py::test_predict5, all 25 pairs (i = j included)
    _close(t.twist.reshape(K * K, 6), o["out"], rtol=1e-4, atol=1e-5, msg="twist")
    from puzzlenet_amd import se3
    assert torch.equal(t.T, se3.exp(t.twist))
    _close(t.de_fpcb.reshape(K * K, 2, N), o["de_fpcb"], rtol=1e-4, atol=1e-4, msg="de_fpcb")
    _close(t.de_mrpcb[J.to(t.de_mrpcb.device)], o["de_mrpcb"], rtol=1e-4, atol=1e-4, msg="de_mrpcb")
    x2 = t.x2.cpu()
    assert torch.equal(x2[I], o["x2_f"]) and torch.equal(x2[J], o["x2_m"])      # the same 256 points, bit for bit


def test_top_k_is_the_oracles_selection(case):
    """Every index the device returns has an oracle class-1 probability of at least the oracle's k-th largest minus 1e-5
    (a near-tie may resolve either way, nothing else may), and no index comes twice."""
    t, o, J = case["table"], case["oracle"], case["J"]
    p_f = torch.softmax(o["de_fpcb"], dim=1)[:, 1, :]                    # [25, N]
    p_m = torch.softmax(o["de_mrpcb"], dim=1)[:, 1, :][:K]               # rows (i = 0, j): [K, N]
    assert torch.equal(J[:K], torch.arange(K))
    for name, p, idx in (("top_f", p_f, t.top_f.reshape(K * K, TOP).cpu()), ("top_m", p_m, t.top_m.cpu())):
        assert int(idx.min()) >= 0 and int(idx.max()) < N, name
        assert all(len(set(r.tolist())) == TOP for r in idx), name
        kth = torch.topk(p, TOP, dim=1)[0][:, -1:]
        assert bool((torch.gather(p, 1, idx) >= kth - 1e-5).all()), name


def test_score_is_the_oracles_chamfer(case):
    """score[i, j] = the oracle's chamfer_loss between the fixed piece's picked points and the moved piece's picked points
    under the oracle's pose, evaluated at the device's own indices (bounds of test_se3_chamfer_comp); +inf on the diagonal."""
    t, o, pieces, I, J = case["table"], case["oracle"], case["pieces"], case["I"], case["J"]
    top_f, top_m = t.top_f.reshape(K * K, TOP).cpu(), t.top_m.cpu()
    Bf = torch.gather(pieces[I], 1, top_f.unsqueeze(-1).expand(-1, -1, 3))
    Bm = torch.gather(pieces[J], 1, top_m[J].unsqueeze(-1).expand(-1, -1, 3))
    Bm = mr.se3_transform(mr.se3_exp(o["out"]), Bm.permute(0, 2, 1)).permute(0, 2, 1)
    d1, d2 = mr.chamfer_loss(Bf, Bm)
    want = (d1.mean(dim=1) + d2.mean(dim=1)).view(K, K)
    got = t.score.cpu()
    off = ~torch.eye(K, dtype=torch.bool)
    assert bool(torch.isinf(got.diagonal()).all()) and bool((got.diagonal() > 0).all())
    np.testing.assert_allclose(got[off].numpy(), want[off].numpy(), rtol=1e-4, atol=2e-6)


def test_fallback_equals_fast_path(case, dev, monkeypatch):
    """Where the pair-head kernel does not take the shape, match_pairs runs the boundary head once per moved piece: the same
    logits to rounding."""
    from puzzlenet_amd import assembly, ops
    calls = []
    real = ops.pair_head_blocks
    monkeypatch.setattr(ops, "pair_head_blocks", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    fast = assembly.match_pairs(case["model"], case["pieces"].to(dev), k=TOP, start=case["start"])
    assert calls == [1]                                   # the fast path is what ran above
    monkeypatch.setattr(ops, "pair_head_blocks_supported", lambda *a: False)
    slow = assembly.match_pairs(case["model"], case["pieces"].to(dev), k=TOP, start=case["start"])
    assert calls == [1]
    assert slow.de_fpcb.shape == fast.de_fpcb.shape
    assert _rel(slow.de_fpcb, fast.de_fpcb) < 1e-5


def test_end_to_end(case, dev):
    from puzzlenet_amd import assembly
    t = case["table"]
    a = assembly.assemble(t.score, t.T)
    assert bool(a.placed.all()) and len(a.edges) == K - 1
    assert np.array_equal(a.G[a.root], np.eye(4))
    pieces = case["pieces"].to(dev)
    cloud = assembly.apply(pieces, a.G)
    assert cloud.shape == (K, N, 3) and bool(torch.isfinite(cloud).all())
    assert torch.equal(cloud[a.root], pieces[a.root])
    # a placed piece is where its chain of pair poses puts it
    i, j, _s, new = a.edges[0]
    g = t.T[i, j].double().cpu().numpy()
    if new == i:
        g = np.linalg.inv(g)
    np.testing.assert_allclose(a.G[new], g, rtol=0, atol=1e-5)      # (rigid inverse of a float32 pose)


def test_match_pairs_rejects_cpu_pieces(case):
    from puzzlenet_amd import _lib, assembly
    with pytest.raises(_lib.PznError):
        assembly.match_pairs(case["model"], case["pieces"], k=TOP, start=case["start"])
