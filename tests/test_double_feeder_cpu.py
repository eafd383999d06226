"""CPU: datapipe.double_cut_rule, the numpy statement of the double-cut loader (PairFeeder(split_twice=True); the reference's
`train.py --random_slice`, dataset.py:1203-1355), on constructed clouds whose side counts are known exactly: every kind, every
threshold at its edge, the seed flips, the re-draws, the fallbacks; its region tables against plan_double_cut_like_reference's;
its pieces against the _segments / _compact_segments semantics of make_pairs_regions; and the plumbing (header, binding table,
the feeder's refusals).  The kernel is held to the statement in tests/test_gpu_double_feeder.py."""
import os

import numpy as np
import pytest

from tests import _double_cut as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, N_RICH = 1024, 3000
X0, Y0 = (1.0, 0.0, 0.0, 0.0), (0.0, 1.0, 0.0, 0.0)        # side = (x >= 0), side = (y >= 0)
OFF = (1.0, 0.0, 0.0, 5.0)                                  # every point on side 1: never a valid cut
U_SEED = {0: 0.1, 1: 0.5, 2: 0.9}
U_SE = {0: 0.1, 1: 0.5, 2: 0.9}


def cloud(n11, n10, n01, n00, seed=0):
    """n_{s1 s2} points in the quadrant (x >= 0) = s1, (y >= 0) = s2, |x|, |y| in [0.1, 0.4], shuffled."""
    rng = np.random.RandomState(seed)
    parts = []
    for cnt, sx, sy in ((n11, 1, 1), (n10, 1, -1), (n01, -1, 1), (n00, -1, -1)):
        p = rng.uniform(0.1, 0.4, size=(cnt, 3))
        p[:, 0] *= sx
        p[:, 1] *= sy
        p[:, 2] -= 0.25
        parts.append(p)
    pts = np.concatenate(parts).astype(np.float32)
    return pts[rng.permutation(len(pts))]


def rule(raw, seed=1, se=0, choice=0, planes1=None, planes2=None, n=N, n_rich=N_RICH, cap=None, starts=(0.0, 0.75, 0.5, 0.25)):
    from puzzlenet_amd import datapipe
    planes1 = [X0] * 4 if planes1 is None else planes1
    planes2 = [Y0] * 7 if planes2 is None else planes2
    u = [U_SEED[seed], U_SE[se], 0.25 + 0.5 * choice] + list(starts)
    return datapipe.double_cut_rule(raw, np.array(planes1, dtype=np.float64), np.array(planes2, dtype=np.float64), u, n=n, n_rich=n_rich, cap=cap)


def quadrant(raw, s1, s2):
    return raw[((raw[:, 0] >= 0) == bool(s1)) & ((raw[:, 1] >= 0) == bool(s2))]


def test_every_kind_is_reachable_and_its_pieces_are_the_stated_rows():
    from puzzlenet_amd import datapipe as dp
    raw = cloud(3500, 2500, 2000, 2000)                     # a = 6000, b = 4000
    up, down = raw[raw[:, 0] >= 0], raw[raw[:, 0] < 0]
    r = rule(raw, seed=0)
    assert r["kind"] == dp.SINGLE and r["ok"] and tuple(r["u_tab"]) == (dp.UP, 0) and tuple(r["d_tab"]) == (dp.DOWN, 0)
    assert np.array_equal(r["planes"], [X0, (0, 0, 0, 0)])
    assert np.array_equal(r["pieces"][0], up) and np.array_equal(r["pieces"][1], down)
    assert r["pieces"][2] is None and r["pieces"][3] is None and r["counts"].tolist() == [6000, 4000, -1, -1]
    assert r["start"].tolist() == [0, 3000, 0, 0]           # clamp(floor(u count), 0, count - 1); 0 where there is no piece
    r = rule(raw, seed=1, se=0, choice=0)                   # U = uppc of up, D = downpc of up, then down
    assert r["kind"] == dp.HALF_VS_REST and tuple(r["u_tab"]) == (dp.UP_UPPC, 0) and tuple(r["d_tab"]) == (dp.UP_DOWNPC, dp.DOWN)
    assert np.array_equal(r["pieces"][0], quadrant(raw, 1, 1))
    assert np.array_equal(r["pieces"][1], np.vstack([quadrant(raw, 1, 0), down])) and r["counts"].tolist() == [3500, 6500, -1, -1]
    assert np.array_equal(r["planes"], [X0, Y0])
    r = rule(raw, seed=1, se=0, choice=1)
    assert tuple(r["u_tab"]) == (dp.UP_DOWNPC, 0) and tuple(r["d_tab"]) == (dp.UP_UPPC, dp.DOWN)
    assert np.array_equal(r["pieces"][1], np.vstack([quadrant(raw, 1, 1), down]))
    r = rule(raw, seed=2, se=1, choice=1)                   # U = downpc of down, D = up; fallback (up, down)
    assert r["kind"] == dp.HALF_VS_OTHER and tuple(r["u_tab"]) == (dp.DOWN_DOWNPC, 0) and tuple(r["d_tab"]) == (dp.UP, 0)
    assert np.array_equal(r["pieces"][0], quadrant(raw, 0, 0)) and np.array_equal(r["pieces"][1], up)
    assert np.array_equal(r["pieces"][2], up) and np.array_equal(r["pieces"][3], down)
    assert r["counts"].tolist() == [2000, 6000, 6000, 4000] and r["start"].tolist() == [0, 4500, 3000, 1000]
    r = rule(raw, seed=1, se=2, choice=1)                   # the halves: `choice` plays no part
    assert r["kind"] == dp.HALVES and tuple(r["u_tab"]) == (dp.UP_UPPC, 0) and tuple(r["d_tab"]) == (dp.UP_DOWNPC, 0)
    assert np.array_equal(r["pieces"][0], quadrant(raw, 1, 1)) and np.array_equal(r["pieces"][1], quadrant(raw, 1, 0))
    assert r["counts"].tolist() == [3500, 2500, -1, -1]
    # the largest draws still name the last branch / the last row
    r = rule(raw, seed=1, se=1, choice=0, starts=(1.0 - 2.0 ** -53,) * 4)
    assert r["start"].tolist() == [3499, 3999, 5999, 3999]


@pytest.mark.parametrize("a, inner_is_up", [(N_RICH - 1, False), (N_RICH, True)])
def test_seed_1_needs_a_rich_up_piece(a, inner_is_up):
    from puzzlenet_amd import datapipe as dp
    raw = cloud(a - 1400, 1400, 2000, 2000)                 # b = 4000 >= n_rich
    r = rule(raw, seed=1, se=2)
    assert r["kind"] == dp.HALVES
    assert tuple(r["u_tab"]) == ((dp.UP_UPPC, 0) if inner_is_up else (dp.DOWN_UPPC, 0))


@pytest.mark.parametrize("b, inner_is_up", [(N_RICH - 1, True), (N_RICH, False)])
def test_seed_2_needs_a_rich_down_piece(b, inner_is_up):
    from puzzlenet_amd import datapipe as dp
    raw = cloud(2000, 2000, b - 1400, 1400)                 # a = 4000 >= n_rich
    r = rule(raw, seed=2, se=2)
    assert r["kind"] == dp.HALVES
    assert tuple(r["u_tab"]) == ((dp.UP_UPPC, 0) if inner_is_up else (dp.DOWN_UPPC, 0))


def test_both_seed_flips_in_sequence():
    """seed 1 with a < n_rich becomes 2, which with b < n_rich becomes 1 again (dataset.py:1214-1217): `up` is cut."""
    from puzzlenet_amd import datapipe as dp
    raw = cloud(1500, 1400, 1300, 1200)                     # a = 2900, b = 2500, both below n_rich, both halves of up >= n
    r = rule(raw, seed=1, se=2)
    assert r["kind"] == dp.HALVES and tuple(r["u_tab"]) == (dp.UP_UPPC, 0) and r["counts"].tolist() == [1500, 1400, -1, -1]
    r = rule(raw, seed=2, se=2)                             # seed 2 takes the second flip only: `up` as well
    assert r["kind"] == dp.HALVES and tuple(r["u_tab"]) == (dp.UP_UPPC, 0)


@pytest.mark.parametrize("c, kind_name", [(N - 1, "half_vs_rest"), (N, "half_vs_other")])
def test_half_vs_other_needs_n_points_in_the_other_piece(c, kind_name):
    from puzzlenet_amd import datapipe as dp, ops
    raw = cloud(3000, 2000, c - 500, 500)                   # a = 5000; seed 1 stays (the second flip is for seed 2 only)
    r = rule(raw, seed=1, se=1, choice=0)
    assert ops.DOUBLE_CUT_KINDS[r["kind"]] == kind_name
    if kind_name == "half_vs_rest":
        assert tuple(r["d_tab"]) == (dp.UP_DOWNPC, dp.DOWN) and r["counts"].tolist() == [3000, 2000 + c, -1, -1]
    else:
        assert tuple(r["d_tab"]) == (dp.DOWN, 0) and r["counts"].tolist() == [3000, c, 5000, c]


@pytest.mark.parametrize("half, kind_name", [(N - 1, "single"), (N, "halves")])
def test_a_half_needs_n_points(half, kind_name):
    from puzzlenet_amd import datapipe as dp, ops
    for raw in (cloud(half, 3000, 2000, 2000), cloud(3000, half, 2000, 2000)):      # uppc short, downpc short
        r = rule(raw, seed=1, se=2)
        assert ops.DOUBLE_CUT_KINDS[r["kind"]] == kind_name
        if kind_name == "single":
            assert np.array_equal(r["planes"][1], np.zeros(4)) and tuple(r["u_tab"]) == (dp.UP, 0) and r["ok"]


def test_plane_2_is_redrawn_up_to_six_times():
    from puzzlenet_amd import datapipe as dp
    raw = cloud(3500, 2500, 2000, 2000)
    y1 = (0.0, 1.0, 0.0, 1e-3)
    r = rule(raw, seed=1, se=2, planes2=[OFF] * 3 + [y1] + [Y0] * 3)
    assert r["kind"] == dp.HALVES and np.array_equal(r["planes"][1], y1)
    r = rule(raw, seed=1, se=2, planes2=[OFF] * 6 + [y1])                            # the sixth re-draw still counts
    assert r["kind"] == dp.HALVES and np.array_equal(r["planes"][1], y1)
    r = rule(raw, seed=1, se=2, planes2=[OFF] * 7)                                   # none valid: the single cut
    assert r["kind"] == dp.SINGLE and r["ok"] and np.array_equal(r["planes"], [X0, (0, 0, 0, 0)])
    assert r["counts"].tolist() == [6000, 4000, -1, -1]


def test_single_takes_the_first_valid_plane_1_candidate_or_the_most_balanced():
    from puzzlenet_amd import datapipe as dp
    rng = np.random.RandomState(3)
    x = np.repeat([-0.3, -0.1, 0.1, 0.3], [500, 400, 1000, 600])
    raw = np.stack([x, rng.uniform(-0.4, 0.4, len(x)), rng.uniform(-0.4, 0.4, len(x))], axis=1).astype(np.float32)
    raw = raw[rng.permutation(len(raw))]

    def px(z):
        return (1.0, 0.0, 0.0, z)
    # up = 1600 / 2000 / 600 for z = 0 / 0.2 / -0.2 of M = 2500: no candidate leaves 1024 on both sides
    r = rule(raw, seed=0, planes1=[px(0.2), px(0.0), px(-0.2), px(0.0)])
    assert r["kind"] == dp.SINGLE and not r["ok"]
    assert np.array_equal(r["planes"][0], px(0.0)) and r["counts"].tolist() == [1600, 900, -1, -1]      # the first of the two equals
    # a lower bar: candidate 0 fails it (500 down), candidate 1 passes
    r = rule(raw, seed=0, n=600, planes1=[px(0.2), px(-0.2), px(0.0), px(0.0)])
    assert r["ok"] and np.array_equal(r["planes"][0], px(-0.2)) and r["counts"].tolist() == [600, 1900, -1, -1]
    # seed 1 on a cloud too small to cut twice falls through to the same search
    r2 = rule(raw, seed=1, se=1, n=600, n_rich=0, planes1=[px(0.2), px(-0.2), px(0.0), px(0.0)], planes2=[OFF] * 7)
    assert r2["kind"] == dp.SINGLE and np.array_equal(r2["planes"], r["planes"])
    # ok = False also when a piece exceeds cap
    assert not rule(raw, seed=0, n=600, cap=1500, planes1=[px(-0.2)] * 4)["ok"]
    assert rule(raw, seed=0, n=600, cap=1900, planes1=[px(-0.2)] * 4)["ok"]


def test_region_tables_are_those_of_the_plan():
    """The (kind, u_tab, d_tab) combinations the rule emits over many draws are exactly those plan_double_cut_like_reference
    (pinned to the reference by data2.npz) emits: 1 for single, 4 for half_vs_rest, 4 for half_vs_other, 2 for halves."""
    import torch
    from puzzlenet_amd import datapipe as dp, ops
    raw = dc.shells(1, 8000, 5)[0] - np.float32(0.06)       # (shifted against the planes' offsets: either piece is rich about as often)
    planes1, planes2, u = dc.draws(600, 4, 17)
    mine = set()
    for i in range(600):
        r = dp.double_cut_rule(raw, planes1[i], planes2[i], u[i], n=N, n_rich=N_RICH)
        mine.add((ops.DOUBLE_CUT_KINDS[r["kind"]], tuple(r["u_tab"]), tuple(r["d_tab"])))
    np_state, torch_state = np.random.get_state(), torch.get_rng_state()
    try:
        np.random.seed(23)
        torch.manual_seed(23)
        plan = set()
        for _ in range(600):
            rec = dp.plan_double_cut_like_reference(raw, lambda cand: 0.0, n=N)
            plan.add((rec["kind"], tuple(rec["u_tab"]), tuple(rec["d_tab"])))
    finally:
        np.random.set_state(np_state)
        torch.set_rng_state(torch_state)
    assert mine == plan
    assert sorted(k for k, _, _ in mine) == ["half_vs_other"] * 4 + ["half_vs_rest"] * 4 + ["halves"] * 2 + ["single"]


def _compact_segments_numpy(raw, code, tab, cap):
    """datapipe._segments + _compact_segments on one cloud, restated in numpy (those run on device tensors)."""
    in0, in1 = (int(tab[0]) >> code) & 1, (int(tab[1]) >> code) & 1
    seg = np.where(in0 == 1, 0, np.where(in1 == 1, 1, 2))
    count = int((seg < 2).sum())
    packed = raw[np.argsort(seg, kind="stable")[:cap]]
    return np.where((np.arange(cap) < count)[:, None], packed, packed[:1]), count


@pytest.mark.parametrize("seed, se, choice", [(0, 0, 0), (1, 0, 0), (2, 0, 1), (1, 1, 1), (2, 1, 0), (1, 2, 0), (2, 2, 0)])
def test_pieces_are_what_make_pairs_regions_would_compact(seed, se, choice):
    from puzzlenet_amd import datapipe as dp
    raw = dc.shells(1, 9000, 8)[0]
    planes1, planes2, _ = dc.draws(1, 4, 4)
    planes1[0, 0] = (0.3, 0.5, 0.2, 0.02)                   # a near-even first split, so that either piece can be cut again
    planes2[0, 0] = (0.5, 0.1, 0.6, 0.01)
    u = [U_SEED[seed], U_SE[se], 0.25 + 0.5 * choice, 0.3, 0.6, 0.2, 0.9]
    r = dp.double_cut_rule(raw, planes1[0], planes2[0], u, n=N, n_rich=N_RICH)
    assert r["kind"] == (dp.SINGLE if seed == 0 else (dp.HALF_VS_REST, dp.HALF_VS_OTHER, dp.HALVES)[se])
    code = 2 * dp._side64(raw, r["planes"][0]).astype(np.int64) + dp._side64(raw, r["planes"][1]).astype(np.int64)
    tabs = [r["u_tab"], r["d_tab"]] + ([(dp.UP, 0), (dp.DOWN, 0)] if r["kind"] == dp.HALF_VS_OTHER else [])
    for cap in (len(raw), 3000):
        for p, tab in enumerate(tabs):
            want, count = _compact_segments_numpy(raw, code, tab, cap)
            assert count == r["counts"][p]
            assert dc.padded(r["pieces"][p], raw[0], cap).tobytes() == want.astype(np.float32).tobytes()


def test_rejection_is_half_vs_other_above_the_reference_bound():
    from puzzlenet_amd import datapipe as dp
    kind = np.array([dp.SINGLE, dp.HALF_VS_REST, dp.HALF_VS_OTHER, dp.HALF_VS_OTHER, dp.HALVES])
    cd = np.array([1.0, 1.0, 0.015, np.nextafter(0.015, 1.0), 1.0])
    assert dp.double_cut_rejects(kind, cd).tolist() == [False, False, False, True, False]


def test_header_and_binding_table_agree_on_the_double_cut():
    from puzzlenet_amd import _lib
    args = _lib.PARAMS["pzn_cut_compact_double_f32"]        # the parameters as include/pzn.h writes them
    res, bound = _lib.SIGNATURES["pzn_cut_compact_double_f32"]
    assert res is _lib._c_i and len(bound) == len(args) == 20
    for decl, ctype in zip(args, bound):      # pointers travel as addresses, the scalars as ints: position by position
        assert (ctype is _lib._c_i) == decl.startswith("int "), (decl, ctype)
    assert args[6:12] == ["int B", "int M", "int K", "int n_min", "int n_rich", "int cap"] and args[-1] == "pzn_stream_t stream"


def test_double_cut_is_listed_for_integrators():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    row = [l for l in doc.splitlines() if l.startswith("| `pzn_cut_compact_double_f32`")]
    assert len(row) == 1 and "ops.cut_compact_double" in row[0] and "dataset.py:1203-1355" in row[0]


def test_feeder_refuses_double_cuts_with_solids_before_the_device_is_looked_at():
    from puzzlenet_amd import _lib, datapipe
    raw = np.zeros((2, 64, 3), dtype=np.float32)
    for cut in ("sphere", "cylinder", "cone"):
        with pytest.raises(_lib.PznUnsupported, match="split_twice"):
            datapipe.PairFeeder(raw, "cuda:0", cut=cut, split_twice=True)
    with pytest.raises(_lib.PznError):                      # the plane form on the CPU: there is no CPU fallback
        datapipe.PairFeeder(raw, "cpu", split_twice=True)


def test_ops_cut_compact_double_rejects_cpu_tensors():
    import torch
    from puzzlenet_amd import _lib, ops
    z = lambda *s: torch.zeros(*s, dtype=torch.float64)
    with pytest.raises(_lib.PznError):
        ops.cut_compact_double(torch.zeros(1, 8, 3), z(1, 2, 3), z(1, 2), z(1, 7, 3), z(1, 7), z(1, 7), 1, 3, 8)
