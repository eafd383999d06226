"""CPU: for every shape tests/test_gpu_ties.py runs, the integer references of tests/_lattice.py equal the C oracle
(oracle/point_ops.py), and the inputs really are decided by exact ties between different points - so the GPU test cannot
quietly stop testing the tie rules.  No GPU."""
import numpy as np
import pytest
import torch

from oracle import point_ops as orc
from tests import _lattice as L
from tests import _merge_ref


# ------------------------------------------------------------------------------------------------ the helper itself

def test_lattice_sites_and_exact_floats():
    rng = np.random.default_rng(1)
    few = L.lattice(200, 6, rng)
    assert few.shape == (200, 3) and few.min() >= 0 and few.max() <= 5
    assert len(np.unique(few, axis=0)) == 200                          # a subset without repetition
    many = L.lattice(700, 6, rng)
    assert len(np.unique(many, axis=0)) == 216                         # every site, plus repeats
    assert not np.array_equal(many[:216], np.unique(many, axis=0))      # shuffled
    f = L.cloud(few, shift=-40)
    assert f.dtype == np.float32 and f.min() >= -5.0 and f.max() <= -2.0
    assert np.array_equal(f.astype(np.float64) * 8, few - 40)
    # squared distances of such floats are exact in float32, whatever the order of the operations
    a, b = f[:50, None, :], f[None, 50:100, :]
    d32 = ((a - b) * (a - b)).sum(-1, dtype=np.float32)
    assert np.array_equal(d32.astype(np.float64) * 256, L._sq(L.to_units(few[:50], -40), L.to_units(few[50:100], -40)))
    rots = L.signed_permutations()
    assert len(rots) == 24 and np.array_equal(rots[0], np.eye(3, dtype=np.int64))


def test_radii_in_float32():
    """What the four radii are once squared and rounded to float32 (the kernels and the oracle compare in float32)."""
    r_axis, r_diag, r_diag32, r_wide = L.BALL_RADII
    assert L.r2_units(r_axis) == 4.0                                   # 1 / 64: axis neighbours on the sphere
    assert L.r2_units(r_diag) == 8.0                                   # exactly 2 / 64: diagonal neighbours on the sphere
    assert 7.999 < L.r2_units(r_diag32) < 8.0                          # 0.031249998: just below, they are outside
    assert L.r2_units(r_wide) == 16.0
    assert L.r2_units(L.BALL_EMPTY_RADIUS) < 3.0                       # an off-lattice query's nearest point is at 3 / 256


# ---------------------------------------------------------------------------------------------------------- FPS

def _fps_check(case, T, want_ties=True):
    """int reference == oracle on every cloud of the case -> the statistics of each cloud."""
    want = orc.farthest_point_sample(case["xyz"], case["S"], case["start"])
    stats = []
    for b in range(len(case["units"])):
        picks, st = L.fps_int(case["units"][b], case["S"], case["start"][b], stats_T=T)
        assert np.array_equal(picks, want[b]), b
        stats.append(st)
        if want_ties and case["N"] >= 63:
            assert st["tied"] >= 0.7 * st["rounds"], st
            if case["N"] > 64:
                assert st["cross"] >= 0.5 * st["rounds"], st
    return stats


@pytest.mark.parametrize("N", L.FPS_MAIN_N)
def test_fps_main_cases(N):
    case = L.fps_case(N, side=L.FPS_MAIN_SIDE.get(N))
    assert case["start"][-1] == N - 1 and (N == 1 or case["start"][0] != case["start"][1])
    _fps_check(case, L.fps_threads(N))


@pytest.mark.parametrize("name", sorted(L.FPS_SPECIAL))
def test_fps_special_cases(name):
    case = L.fps_case(**L.FPS_SPECIAL[name])
    stats = _fps_check(case, L.fps_threads(case["N"]))
    if name == "s_equals_n":
        assert case["S"] == case["N"]
        for b in range(2):
            assert len(np.unique(case["units"][b], axis=0)) == case["N"]      # distinct sites: every row is picked once
            assert sorted(L.fps_int(case["units"][b], case["S"], case["start"][b])) == list(range(case["N"]))
    if name == "identical":
        picks = L.fps_int_batch(case["units"], case["S"], case["start"])
        assert (picks[:, 1:] == 0).all()
    if name == "shifted":
        assert case["xyz"].max() < 0
    if name.startswith("zero_"):
        # S < N and the lattice is exhausted before the last pick: the last rounds tie at 0 on every lane of every wavefront
        assert case["S"] < case["N"] and L.fps_form(case["N"]) == name[5:]
        for st in stats:
            assert st["zero"] >= case["S"] - case["side"] ** 3 - 1 > 0, st


def test_fps_zero_ties_cover_every_form():
    assert {L.fps_form(L.FPS_SPECIAL[n]["N"]) for n in L.FPS_SPECIAL if n.startswith("zero_")} == {"key32", "key64", "published"}


@pytest.mark.parametrize("N", L.FPS_BG_N)
def test_fps_background_cases(N):
    case = L.fps_bg_case(N)
    T = L.fps_threads(N, background_cap=N)
    _fps_check(case, T)
    if N in (600, 2300):
        assert ((N + T - 1) // T) % 2 == 1                               # an odd number of live register slots


def test_fps_background_shapes_are_the_five_launches():
    caps = (2048, 4096, 8192, 16384, 32768)
    assert [min(c for c in caps if N <= c) for N in L.FPS_BG_N] == list(caps)


@pytest.mark.parametrize("N,counts", L.FPS_BG_COUNTS)
def test_fps_counts_cases(N, counts):
    case = L.fps_counts_case(N, counts)
    parities = set()
    for b, c in enumerate(counts):
        assert case["S"] <= c < N and case["start"][b] < c
        assert (case["units"][b, c:] == case["units"][b, 0]).all()      # padding: copies of row 0
        want = orc.farthest_point_sample(case["xyz"][b:b + 1, :c], case["S"], case["start"][b:b + 1])[0]
        picks = L.fps_int(case["units"][b, :c], case["S"], case["start"][b])
        assert np.array_equal(picks, want)
        # padding never changes a pick: it ties with row 0 in every round and row 0 has the lower index
        assert np.array_equal(L.fps_int(case["units"][b], case["S"], case["start"][b]), picks)
        parities.add(((c + 255) // 256) % 2)
    assert max(counts) + 100 < N and max(counts) <= 4096                # both bounds stay below N: 256 threads per cloud
    assert parities == {0, 1}


# --------------------------------------------------------------------------------------------------------- merge

@pytest.mark.parametrize("Na,Nb,n_out,with_drops", L.MERGE_CASES)
def test_merge_cases(Na, Nb, n_out, with_drops):
    case = L.merge_case(Na, Nb, n_out, with_drops)
    U = Na + Nb
    a, b, T = (torch.from_numpy(case[k]) for k in ("a", "b", "T"))
    assert np.array_equal(case["T"][0], np.eye(4, dtype=np.float32)) and not np.array_equal(case["T"][1], case["T"][0])
    for m in range(2):
        # the pose keeps the lattice exact: the placed rows of b are the integer sites they were drawn as
        placed = _merge_ref.transform_rows(T[m], b[m]).numpy()
        assert np.array_equal(placed.astype(np.float64) * L.UNIT, case["union"][m][Na:])
        # overlapping parts: some placed rows of b coincide with rows of a
        both = len(np.unique(case["union"][m], axis=0))
        assert both <= U - Nb // 4 and both < U
        if with_drops:
            assert n_out <= L.merge_kept_distinct(case, m)
    if not with_drops:
        _, src = _merge_ref.merge_resample(a, b, T, torch.from_numpy(case["start"]), n_out)
        want = L.fps_int_batch(case["union"], n_out, case["start"])
        assert np.array_equal(src.numpy(), want)


def test_merge_shapes_cover_the_unions():
    assert sorted(na + nb for na, nb, _ in L.MERGE_SHAPES) == [200, 256, 330, 700, 1024, 2048, 4096]


# ----------------------------------------------------------------------------------------------------------- kNN

def _knn_check(case, tie_share):
    want = orc.knn(case["xyz"], case["q"], case["K"])
    stats = []
    for b in range(len(case["units"])):
        assert np.array_equal(L.knn_int(case["units"][b], case["q_units"][b], case["K"]), want[b]), b
        st = L.knn_stats(case["units"][b], case["q_units"][b], case["K"])
        if case["K"] < case["N"]:
            assert st["tie"].mean() >= tie_share, (b, st["tie"].mean())
        stats.append(st)
    return stats


@pytest.mark.parametrize("name", sorted(L.KNN_CASES))
def test_knn_cases(name):
    case = L.knn_case(name)
    assert (case["q_units"][:, -8:] % 2 == 1).all() and (case["q_units"][:, :-8] % 2 == 0).all()
    stats = _knn_check(case, 0.5)
    if name in L.KNN_OVERFLOW:
        # repeated sites: some query passes more than 128 candidates, or more than 7 on one lane, through select32's first bound
        assert len(np.unique(case["units"][0], axis=0)) < case["N"]
        assert any(((st["cand"] > 128) | (st["lane_max"] > 7)).any() for st in stats)
        assert any(((st["cand"] > 64) & (st["cand"] <= 128)).any() for st in stats)      # and cand_reduce after the collection


def test_knn_many_queries_case():
    case = L.knn_many_queries_case()
    assert case["xyz"].shape == (64, 64, 3) and case["q"].shape == (64, 512, 3)
    want = orc.knn(case["xyz"], case["q"], 32)
    for b in range(0, 64, 7):
        assert np.array_equal(L.knn_int(case["units"][b], case["q_units"][b], 32), want[b])
    st = L.knn_stats(case["units"][0], case["q_units"][0], 32)
    assert st["tie"].mean() >= 0.5


def test_knn_cases_cover_the_kernels():
    ns = lambda prefix: sorted({v[1] for k, v in L.KNN_CASES.items() if k.startswith(prefix) and v[3] == 32})
    assert ns("select_") == [64, 128, 129, 256, 257, 512, 513, 1024, 1025, 2048, 2049, 4096, 4097, 8192]
    assert ns("knn32_") == [33, 63, 8193, 13000]
    assert {(v[1], v[3]) for k, v in L.KNN_CASES.items() if k.startswith("any_")} == {(n, k) for n in (64, 300, 2048)
                                                                                       for k in (33, 48, 64)}
    assert all(L.KNN_GROUP[n] in L.KNN_CASES for n in (129, 2048, 8192))


# ---------------------------------------------------------------------------------------------------- ball query

@pytest.mark.parametrize("N", L.BALL_N)
def test_ball_cases(N):
    case = L.ball_case(N)
    for ns in L.BALL_NSAMPLE:
        for r in L.BALL_RADII:
            want = orc.query_ball_point(r, ns, case["xyz"], case["fq_on"])[0]
            assert np.array_equal(L.ball_int(L.r2_units(r), ns, case["units"][0], case["q_on"][0]), want), (ns, r)
        want = orc.query_ball_point(L.BALL_EMPTY_RADIUS, ns, case["xyz"], case["fq_off"])[0]
        assert np.array_equal(L.ball_int(L.r2_units(L.BALL_EMPTY_RADIUS), ns, case["units"][0], case["q_off"][0]), want)
        assert (want == N).all()                                        # nothing in the ball: the reference's rule gives N
    # points exactly ON the two spheres exist, so `<=` against `<` decides hits; the radius just below 2 / 64 drops them
    d = L._sq(case["q_on"][0], case["units"][0])
    assert (d == 4).any() and (d == 8).any()
    r_axis, r_diag, r_diag32, _ = L.BALL_RADII
    full = lambda r: L.ball_int(L.r2_units(r), N, case["units"][0], case["q_on"][0])
    assert not np.array_equal(full(r_diag), full(r_diag32))
