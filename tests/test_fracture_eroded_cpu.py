"""CPU: the numpy statement of the eroded fracture - datapipe.fracture_eroded_rule / fracture_pair_eroded_rule - against the rules
without erosion where nothing is lost, against its own invariants by replay, and at its edges: a candidate that erosion makes
invalid, a cloud that is lost whole, a NaN, and points exactly on the rims of the band (the comparisons are strict)."""
import functools

import numpy as np
import pytest

from tests import _fracture_curved as fc
from tests import _fracture_eroded as fe

FORMS = (False, True)      # curved


@functools.lru_cache(maxsize=None)
def _stated(i, curved, eroded=True):
    """The rule on SHAPES[i], without a cap -> (inputs, the rule's records)"""
    shape = fe.SHAPES[i]
    raw, form, u_anchor, u_start, erode = fe.inputs(shape, curved)
    if not eroded:
        erode = np.zeros_like(erode)
    recs, _ = fe.batch_statement(raw, form, u_anchor, u_start, erode, shape[4], shape[1])
    return (raw, form, u_anchor, u_start, erode), recs


@pytest.mark.parametrize("curved", FORMS)
@pytest.mark.parametrize("i", (1, 2, 5, 6))
def test_zero_erosion_is_the_rule_without(i, curved):
    from puzzlenet_amd import datapipe as dp
    B, M, P, K, n_min, cap = fe.SHAPES[i]
    raw, form, u_anchor, u_start, erode = fe.inputs(fe.SHAPES[i], curved)
    zero = np.zeros_like(erode)
    u, _ = fc.pair_draws(B, 50 + M)
    pieces = [max(2, P - 3 * b) for b in range(B)]
    for b in range(B):
        normals, frames, half_curv = fe.of_sample(form, b)
        got = dp.fracture_eroded_rule(raw[b], normals, u_anchor[b], u_start[b], zero[b], P, n_min, cap, frames=frames, half_curv=half_curv)
        pair = dp.fracture_pair_eroded_rule(raw[b], normals, u_anchor[b], u[b], zero[b], pieces[b], P, n_min, 0.75, cap, frames=frames,
                                            half_curv=half_curv)
        if curved:
            want = dp.fracture_curved_rule(raw[b], frames, half_curv, u_anchor[b], u_start[b], P, n_min, cap)
            want_pair = dp.fracture_pair_curved_rule(raw[b], frames, half_curv, u_anchor[b], u[b], pieces[b], P, n_min, 0.75, cap)
        else:
            want = dp.fracture_rule(raw[b], normals, u_anchor[b], u_start[b], P, n_min, cap)
            want_pair = dp.fracture_pair_rule(raw[b], normals, u_anchor[b], u[b], pieces[b], P, n_min, 0.75, cap)
        for g, w in ((got, want), (pair, want_pair)):
            assert not g["lost"].any() and g["anchor"].dtype == np.int32
            assert set(w) <= set(g) and set(g) - set(w) <= {"anchor", "lost"}
            for key, x in w.items():
                if key == "pieces":
                    assert all((p is None and q is None) or p.tobytes() == q.tobytes() for p, q in zip(g[key], x)), key
                else:
                    assert np.asarray(g[key]).tobytes() == np.asarray(x).tobytes() and type(g[key]) is type(x), key


@pytest.mark.parametrize("curved", FORMS)
@pytest.mark.parametrize("i", range(len(fe.SHAPES)))
def test_invariants(i, curved):
    B, M, P, K, n_min, cap = fe.SHAPES[i]
    raw, form, u_anchor, u_start, erode = fe.inputs(fe.SHAPES[i], curved)
    recs, _ = fe.batch_statement(raw, form, u_anchor, u_start, erode, n_min, cap)
    share = [float(r["lost"].sum()) / M for r in recs]
    print(fe.SHAPES[i], "curved" if curved else "plane", "ok", [r["ok"] for r in recs], "lost share", np.round(share, 3).tolist())
    for b, r in enumerate(recs[:2]):
        fe.check_invariants(raw[b], fe.of_sample(form, b), u_anchor[b], u_start[b], erode[b], n_min, cap, r)
    assert all(s > 0 for s in share)


@pytest.mark.parametrize("curved", FORMS)
def test_erosion_changes_the_candidate_taken_and_every_step_stays_valid(curved):
    """The four shapes with several candidates and no cap in the way: a candidate that leaves >= n_min points on both sides of the
    surface no longer does after the loss, and a later one is taken - with every step of every sample still valid."""
    for i in (1, 2, 3, 4):
        _, recs = _stated(i, curved)
        _, plain = _stated(i, curved, eroded=False)
        changed = sum(int((r["cand"] != q["cand"]).sum()) for r, q in zip(recs, plain))
        M = fe.SHAPES[i][1]
        print(fe.SHAPES[i], "curved" if curved else "plane", "steps with another candidate", changed, "lost share",
              [round(float(r["lost"].sum()) / M, 3) for r in recs])
        assert all(r["ok"] for r in recs) and all(q["ok"] for q in plain)
        assert changed >= 1
        assert all(0 < r["lost"].sum() and r["counts"].sum() + r["lost"].sum() == M for r in recs)


@pytest.mark.parametrize("curved", FORMS)
def test_a_cloud_that_is_lost_whole(curved):
    """M = 64 in the unit cube, every width 10: step 1 loses the whole cloud, steps 2 and 3 are not made."""
    from puzzlenet_amd import datapipe as dp
    M, P, K = 64, 4, 2
    raw = fc.clouds(1, M, 3)[0]
    frames, half_curv, u_anchor, u_start, _ = fc.draws(1, P, K, 4)
    form = (None, frames[0], half_curv[0]) if curved else (np.ascontiguousarray(frames[0, :, :, 2]), None, None)
    erode = np.full((P - 1, 4), 10.0)
    r = dp.fracture_eroded_rule(raw, form[0], u_anchor[0], u_start[0], erode, P, 4, M, frames=form[1], half_curv=form[2])
    assert r["ok"] is False and (r["label"] == fe.LOST).all() and r["lost"].tolist() == [M, 0, 0] and not r["counts"].any()
    assert r["target"].tolist() == [0, 0, 0] and not r["planes"][1:].any() and not r["cand"][1:].any() and not r["anchor"][1:].any()
    assert r["planes"][0].any() and np.array_equal(r["order"], np.arange(M)) and not r["start"].any()
    assert all(p.tobytes() == np.broadcast_to(raw[0], (M, 3)).tobytes() for p in r["pieces"])
    fe.check_invariants(raw, form, u_anchor[0], u_start[0], erode, 4, M, r)
    pair = dp.fracture_pair_eroded_rule(raw, form[0], u_anchor[0], np.full(7, 0.5), erode, 4, P, 4, 0.0, M, frames=form[1],
                                        half_curv=form[2])
    assert pair["ok"] is False and pair["pair"].tolist() == [0, 3, -1, -1] and pair["counts"].tolist() == [0, 0, -1, -1]
    assert pair["lost"].tolist() == [M, 0, 0] and (pair["label"] == fe.LOST).all()


@pytest.mark.parametrize("curved", FORMS)
def test_a_nan_row_loses_nothing(curved):
    from puzzlenet_amd import datapipe as dp
    B, M, P, K, n_min, cap = fe.SHAPES[3]
    raw, form, u_anchor, u_start, erode = fe.inputs(fe.SHAPES[3], curved)
    normals, frames, half_curv = fe.of_sample(form, 0)
    e = erode[0].copy()
    e[1] = np.nan
    e[2] = [np.nan, 0.02, 0.0, 0.0]                 # a band with one NaN rim: no comparison with it holds
    r = dp.fracture_eroded_rule(raw[0], normals, u_anchor[0], u_start[0], e, P, n_min, cap, frames=frames, half_curv=half_curv)
    assert r["lost"][1] == 0 and r["lost"][2] == 0 and r["lost"][0] > 0 and r["lost"][3] > 0
    fe.check_invariants(raw[0], (normals, frames, half_curv), u_anchor[0], u_start[0], e, n_min, cap, r)


def test_draw_erosion():
    from puzzlenet_amd import datapipe as dp
    e = dp.draw_erosion(np.random.RandomState(1), 64, 9, 0.02, (0.05, 0.1))
    assert e.shape == (64, 8, 4) and e.dtype == np.float64 and (e >= 0).all()
    assert e[..., :2].max() < 0.02 and e[..., 2].max() < 0.05 and e[..., 3].max() < 0.1
    assert e[..., :2].max() > 0.019 and e[..., 2].max() > 0.045 and e[..., 3].max() > 0.09      # the ranges are used
    assert e.tobytes() == (np.random.RandomState(1).rand(64, 8, 4) * np.array([0.02, 0.02, 0.05, 0.1])).tobytes()
    bands = dp.draw_erosion(np.random.RandomState(1), 3, 2, 0.5)
    assert bands.shape == (3, 1, 4) and not bands[..., 2:].any()                                  # no chip by default
    assert not dp.draw_erosion(np.random.RandomState(1), 3, 5, 0.0).any()


def test_points_exactly_on_the_rims_of_the_band_are_kept():
    raw, forms, u_anchor, u_start, erode, n_min = fe.lattice_case()
    both = []
    for form in forms:
        recs, _ = fe.batch_statement(raw, form, u_anchor, u_start, erode, n_min, raw.shape[1])
        print("on the rims", fe.check_lattice_rims(raw, form, erode, recs))
        for b, r in enumerate(recs[:2]):
            fe.check_invariants(raw[b], fe.of_sample(form, b), u_anchor[b], u_start[b], erode[b], n_min, raw.shape[1], r)
        both.append(recs)
    for p, c in zip(*both):                                    # exact arithmetic: the two forms cut alike
        assert np.array_equal(p["label"], c["label"]) and np.array_equal(p["cand"], c["cand"])


def test_the_feeder_refuses_erosion_it_cannot_use_before_it_touches_the_device():
    from puzzlenet_amd import _lib, datapipe as dp
    raw = fc.clouds(2, 64, 1)
    for kwargs in (dict(erosion=0.02), dict(chip=(0.05, 0.1)), dict(erosion=0.02, cut="sphere")):
        with pytest.raises(_lib.PznUnsupported):
            dp.PairFeeder(raw, "cuda:0", **kwargs)
    for kwargs in (dict(erosion=-0.01), dict(erosion=float("nan")), dict(erosion=float("inf")), dict(erosion="0.02"),
                   dict(chip=(0.05,)), dict(chip=(0.05, -0.1)), dict(erosion=0.01, chip=(float("inf"), 0.1))):
        with pytest.raises(_lib.PznError):
            dp.PairFeeder(raw, "cuda:0", pieces=3, **kwargs)
