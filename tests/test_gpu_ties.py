"""GPU: farthest point sampling, merge_resample, kNN, the fused kNN + group launch and the ball query on LATTICE clouds
(tests/_lattice.py), where most rounds and most queries are decided by an exact tie between different points: lowest
index wins the arg-max, kNN order is (distance, index), the ball keeps d <= r^2.  Coordinates are multiples of 1 / 8
(queries of 1 / 16), so every distance is exact in float32 and only the selection logic is under test; every comparison
is np.array_equal against the C oracle (or tests/_merge_ref.py).  tests/test_lattice_cpu.py checks, without a GPU, that
the oracle equals an independent integer reference on these very inputs and that they are decided by ties."""
import numpy as np
import pytest
import torch

from oracle import point_ops as orc
from tests import _lattice as L
from tests import _merge_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from puzzlenet_amd import _lib
    assert _lib.load().pzn_device_check() == 0
    return torch.device("cuda:0")


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# ---------------------------------------------------------------------------------------------- FPS, main entry

def _fps_main(dev, case):
    from puzzlenet_amd import ops
    want = orc.farthest_point_sample(case["xyz"], case["S"], case["start"])
    got = ops.farthest_point_sample(_t(case["xyz"], dev), case["S"], _t(case["start"], dev)).cpu().numpy()
    assert np.array_equal(got, want)
    return want


@pytest.mark.parametrize("N", L.FPS_MAIN_N)
def test_fps_main(dev, N):
    """Either side of every dispatch edge of pzn_fps_f32; two clouds, different starts, one the last index."""
    _fps_main(dev, L.fps_case(N, side=L.FPS_MAIN_SIDE.get(N)))


@pytest.mark.parametrize("name", sorted(L.FPS_SPECIAL))
def test_fps_special(dev, name):
    """S = N, an all-identical cloud, negative coordinates, and a lattice exhausted before the last pick (the last rounds
    tie at distance 0 on every lane of every wavefront) for each of the three rounds."""
    from puzzlenet_amd import ops
    case = L.fps_case(**L.FPS_SPECIAL[name])
    want = _fps_main(dev, case)
    if name == "identical":
        assert (want[:, 1:] == 0).all()
    if name.startswith("zero_"):      # ... and from the background entry
        got = ops.farthest_point_sample(_t(case["xyz"], dev), case["S"], _t(case["start"], dev), background=True)
        assert np.array_equal(got.cpu().numpy(), want)


# ------------------------------------------------------------------------------------------- FPS, background=True

@pytest.mark.parametrize("N", L.FPS_BG_N)
def test_fps_background(dev, N):
    """The five launch_published shapes; two clouds share a workgroup where the form has four wavefronts (B = 2), three
    take one workgroup each."""
    from puzzlenet_amd import ops
    case = L.fps_bg_case(N)
    want = orc.farthest_point_sample(case["xyz"], case["S"], case["start"])
    for B in (2, 3):
        got = ops.farthest_point_sample(_t(case["xyz"][:B], dev), case["S"], _t(case["start"][:B], dev), background=True)
        assert np.array_equal(got.cpu().numpy(), want[:B]), B


@pytest.mark.parametrize("N,counts", L.FPS_BG_COUNTS)
def test_fps_background_counts(dev, N, counts):
    """Padded buffers (rows >= counts[b] are copies of row 0, which tie with it in every round): the picks of the real
    rows alone, and the main entry's on the whole buffer; an odd and an even number of live register slots."""
    from puzzlenet_amd import ops
    case = L.fps_counts_case(N, counts)
    S = case["S"]
    want = np.stack([orc.farthest_point_sample(case["xyz"][b:b + 1, :c], S, case["start"][b:b + 1])[0]
                     for b, c in enumerate(counts)])
    xyz, start = _t(case["xyz"], dev), _t(case["start"], dev)
    cnt = torch.tensor(counts, dtype=torch.int64, device=dev)
    main = ops.farthest_point_sample(xyz, S, start).cpu().numpy()
    assert np.array_equal(main, want)
    for B in (2, 3):
        for bound in (0, max(counts[:B]), max(counts[:B]) + 100):
            got = ops.farthest_point_sample(xyz[:B], S, start[:B], background=True, counts=cnt[:B], max_count=bound)
            assert np.array_equal(got.cpu().numpy(), want[:B]), (B, bound)


# ------------------------------------------------------------------------------------------------ merge_resample

@pytest.mark.parametrize("Na,Nb,n_out,with_drops", L.MERGE_CASES)
def test_merge_resample(dev, Na, Nb, n_out, with_drops):
    """Two overlapping parts of one lattice under poses that keep it exact (identity; a 90-degree rotation with a
    translation in multiples of 1 / 8): placed rows of b coincide with rows of a, as matched boundaries do."""
    from puzzlenet_amd import ops
    case = L.merge_case(Na, Nb, n_out, with_drops)
    c = lambda k: None if case[k] is None else torch.from_numpy(case[k])
    a, b, T, start, drop_a, drop_b = (c(k) for k in ("a", "b", "T", "start", "drop_a", "drop_b"))
    d = lambda t: None if t is None else t.to(dev)
    out, src = ops.merge_resample(d(a), d(b), d(T), d(start), n_out, d(drop_a), d(drop_b))
    want_out, want_src = _merge_ref.merge_resample(a, b, T, start, n_out, drop_a, drop_b)
    assert torch.equal(src.cpu(), want_src)
    assert torch.equal(out.cpu(), want_out)
    if with_drops:
        for m in range(2):
            dropped = set(drop_a[m].tolist()) | set((drop_b[m] + Na).tolist())
            assert not dropped & set(src[m].tolist()), m
    else:
        # the identity pose (merge 0) is the FPS kernel on the concatenation
        union = torch.cat((a[:1], b[:1]), dim=1)
        fps = ops.farthest_point_sample(union.to(dev), n_out, start[:1].to(dev)).cpu()
        assert torch.equal(src[:1].cpu(), fps)


# ----------------------------------------------------------------------------------------------------------- kNN

@pytest.mark.parametrize("name", sorted(L.KNN_CASES))
def test_knn(dev, name):
    """K = 32 at every R of knn_select_kernel, K in {1, 7, 31}, repeated sites (the overflow path of select32),
    knn32_kernel (N < 64, N > 8192, K = N = 40) and knn_any_kernel (K > 32); queries on and off the lattice."""
    from puzzlenet_amd import ops
    case = L.knn_case(name)
    got = ops.knn(_t(case["xyz"], dev), _t(case["q"], dev), case["K"]).cpu().numpy()
    assert np.array_equal(got, orc.knn(case["xyz"], case["q"], case["K"]))


def test_knn_needs_k_at_most_n(dev):
    from puzzlenet_amd import _lib, ops
    case = L.knn_case("knn32_n40_k40")
    with pytest.raises(_lib.PznError):
        ops.knn(_t(case["xyz"], dev), _t(case["q"], dev), 41)


def test_knn_many_queries_per_workgroup(dev):
    from puzzlenet_amd import ops
    case = L.knn_many_queries_case()
    got = ops.knn(_t(case["xyz"], dev), _t(case["q"], dev), 32).cpu().numpy()
    assert np.array_equal(got, orc.knn(case["xyz"], case["q"], 32))


@pytest.mark.parametrize("N", sorted(L.KNN_GROUP))
@pytest.mark.parametrize("D", [64, 128, 8])
def test_knn_group(dev, N, D):
    """The fused search + group launch on the same clouds: compile-time pieces of 16 rows (D = 64) and 8 rows (D = 128),
    and the generic piece (D = 8)."""
    from puzzlenet_amd import ops
    case = L.knn_case(L.KNN_GROUP[N])
    xyz, q = case["xyz"], case["q"]
    B, S = q.shape[:2]
    feat = np.random.default_rng(N + D).standard_normal((B, N, D)).astype(np.float32)
    new_points, gx, idx = ops.knn_group(_t(xyz, dev), _t(feat, dev), _t(q, dev), want_grouped_xyz=True)
    want_idx = orc.knn(xyz, q, 32)
    assert np.array_equal(idx.cpu().numpy(), want_idx)
    want_points, want_gx = orc.group(xyz, feat, q, want_idx, want_grouped_xyz=True)
    assert np.array_equal(new_points.cpu().numpy().view(np.uint32), want_points.view(np.uint32))
    assert np.array_equal(gx.cpu().numpy(), want_gx)


# ---------------------------------------------------------------------------------------------------- ball query

@pytest.fixture(scope="module")
def ball_cases():
    return {N: L.ball_case(N) for N in L.BALL_N}


@pytest.mark.parametrize("N", L.BALL_N)
@pytest.mark.parametrize("nsample", L.BALL_NSAMPLE)
def test_ball_query(dev, ball_cases, N, nsample):
    """Radii as Python floats: lattice neighbours exactly ON the sphere are kept (r^2 = 1 / 64 and 2 / 64 in float32), a
    radius whose float32 square is just below 2 / 64 drops them, and an empty ball returns N."""
    import puzzlenet_amd.pointnet_util as pu
    from puzzlenet_amd import ops
    case = ball_cases[N]
    xyz = _t(case["xyz"], dev)
    for r in L.BALL_RADII:
        got = pu.query_ball_point(r, nsample, xyz, _t(case["fq_on"], dev)).cpu().numpy()
        assert np.array_equal(got, orc.query_ball_point(r, nsample, case["xyz"], case["fq_on"])), r
    got = ops.ball_query(L.BALL_EMPTY_RADIUS, nsample, xyz, _t(case["fq_off"], dev)).cpu().numpy()
    assert (got == N).all()
    assert np.array_equal(got, orc.query_ball_point(L.BALL_EMPTY_RADIUS, nsample, case["xyz"], case["fq_off"]))
