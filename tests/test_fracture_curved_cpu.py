"""CPU: datapipe.fracture_curved_rule and fracture_pair_curved_rule, the numpy statements of the curved fracture kernels: the
invariants by replay, the side test against exact rational arithmetic, zero curvature against fracture_rule where both are exact,
the host draws restated, and the feeder's arguments.  The kernels are held to the statements in tests/test_gpu_fracture_curved.py."""
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import _fracture as fr
from tests import _fracture_curved as fc


@pytest.mark.parametrize("shape", fr.OK_SHAPES[:3], ids=str)
def test_invariants_where_every_step_has_a_valid_candidate(shape):
    from puzzlenet_amd import datapipe
    M, P, K, n_min = shape
    B = 3
    raw = fc.clouds(B, M, 100 + M)
    frames, half_curv, u_anchor, u_start, _ = fc.draws(B, P, K, 200 + M)
    for case in ("random", "saddle"):
        hc = fc.shaped(half_curv, case)
        for b in range(B):
            r = datapipe.fracture_curved_rule(raw[b], frames[b], hc[b], u_anchor[b], u_start[b], P, n_min, M)
            fc.check_invariants(raw[b], frames[b], hc[b], u_anchor[b], u_start[b], n_min, M, r)
            assert r["ok"] and r["counts"].min() >= n_min, (case, b)


@pytest.mark.parametrize("shape", fr.NOT_OK_SHAPES, ids=str)
def test_invariants_where_some_step_has_none(shape):
    from puzzlenet_amd import datapipe
    M, P, K, n_min = shape
    B = 6
    raw = fc.clouds(B, M, 300 + M)
    frames, half_curv, u_anchor, u_start, _ = fc.draws(B, P, K, 400 + M)
    oks = []
    for cap in (M, M // 3):                                    # and a cap below the largest piece
        for b in range(B):
            r = datapipe.fracture_curved_rule(raw[b], frames[b], half_curv[b], u_anchor[b], u_start[b], P, n_min, cap)
            fc.check_invariants(raw[b], frames[b], half_curv[b], u_anchor[b], u_start[b], n_min, cap, r)
            oks.append(r["ok"])
    print(shape, "ok", oks)
    assert not all(oks[:B])                                    # the most-balanced path was replayed


def _exact(x, a, frame, hc):
    """f in exact rational arithmetic from the float64 inputs (the float32 coordinates widened)"""
    F = Fraction
    d = [F(float(x[i])) - F(float(a[i])) for i in range(3)]
    s1, s2, h = (sum(d[i] * F(float(e[i])) for i in range(3)) for e in frame)
    return h + F(float(hc[0])) * s1 * s1 + F(float(hc[1])) * s2 * s2


def test_the_side_test_against_exact_arithmetic():
    """A seeded uniform cloud of 300 points, one drawn surface with curvatures up to 2 through one of them: every point with
    |f| >= 2^-40 is on the side of the exact sign; the points nearer than that are the anchor and at most 0.5 % of the cloud."""
    from puzzlenet_amd import datapipe
    M = 300
    raw = fc.clouds(1, M, 17)[0]
    frames, half_curv, u_anchor, _, _ = fc.draws(1, 2, 1, 18, curvature=2.0)
    frame, hc = frames[0, 0, 0], half_curv[0, 0, 0]
    row = datapipe._start_index(u_anchor[0, 0, 0], M)
    a = raw[row].astype(np.float64)
    f = datapipe.quadric_value(raw, a, frame, hc)
    assert f.tobytes() == fc.value(raw, raw[row], frame, hc).tobytes() and f[row] == 0.0
    exact = [_exact(raw[j], a, frame, hc) for j in range(M)]
    assert exact[row] == 0
    near = [j for j in range(M) if abs(exact[j]) < Fraction(1, 2 ** 40)]
    print("nearer than 2^-40:", near, "anchor", row, "up", int((f >= 0).sum()), "of", M)
    assert row in near and len(near) - 1 <= M * 5 // 1000
    wrong = [j for j in range(M) if j not in near and (f[j] >= 0) != (exact[j] >= 0)]
    assert not wrong, wrong
    assert 0 < int((f >= 0).sum()) < M                         # the surface has points on both sides
    # and the rule's first step is this side test
    r = datapipe.fracture_curved_rule(raw, frames[0], half_curv[0], u_anchor[0], np.zeros(2), 2, 1, M)
    assert r["anchor"][0] == row and np.array_equal(r["label"] == 0, f >= 0)


def test_zero_curvature_is_the_plane_rule_where_both_are_exact():
    """Lattice clouds (multiples of 1/16) and signed coordinate axes as frames: d . n and x . n - a . n are both exact, so the
    curved rule with half_curv = 0 labels as fracture_rule does with the frames' normals; many points lie exactly on a surface."""
    from puzzlenet_amd import datapipe
    B, M, P, K, n_min = 20, 600, 5, 4, 40
    raw = fc.lattice_clouds(B, M, 5)
    frames, normals = fc.axis_frames(B, P, K, 6)
    _, _, u_anchor, u_start, _ = fc.draws(B, P, K, 7)
    on_surface = 0
    for b in range(B):
        c = datapipe.fracture_curved_rule(raw[b], frames[b], np.zeros((P - 1, K, 2)), u_anchor[b], u_start[b], P, n_min, M)
        p = datapipe.fracture_rule(raw[b], normals[b], u_anchor[b], u_start[b], P, n_min, M)
        for key in ("label", "target", "cand", "counts", "order", "start", "planes"):
            assert np.array_equal(c[key], p[key]), (b, key)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(c["pieces"], p["pieces"])) and c["ok"] == p["ok"]
        fc.check_invariants(raw[b], frames[b], np.zeros((P - 1, K, 2)), u_anchor[b], u_start[b], n_min, M, c)
        a, k = int(c["anchor"][0]), int(c["cand"][0])
        on_surface += int((fc.value(raw[b], raw[b, a], frames[b, 0, k], np.zeros(2)) == 0).sum()) - 1
    print("points exactly on the first surface, the anchor apart:", on_surface)
    assert on_surface > B                                      # the f = 0, up case was compared


@pytest.mark.parametrize("Pb", [2, 3, 5])
def test_the_pair_rule_is_the_curved_fracture_with_the_plane_rules_pair(Pb):
    from puzzlenet_amd import datapipe
    B, M, P, K, n_min = 4, 1000, 5, 4, 64
    raw = fc.clouds(B, M, 31)
    frames, half_curv, u_anchor, _, _ = fc.draws(B, P, K, 32)
    u, _ = fc.pair_draws(B, 33)
    for b in range(B):
        r = datapipe.fracture_pair_curved_rule(raw[b], frames[b], half_curv[b], u_anchor[b], u[b], Pb, P, n_min, 0.5, M)
        f = datapipe.fracture_curved_rule(raw[b], frames[b, :Pb - 1], half_curv[b, :Pb - 1], u_anchor[b, :Pb - 1], np.zeros(Pb), Pb,
                                          n_min, M)
        assert np.array_equal(r["label"], f["label"])
        for key in ("planes", "target", "cand", "anchor"):
            assert r[key].shape[0] == P - 1 and r[key][:Pb - 1].tobytes() == f[key].tobytes() and not r[key][Pb - 1:].any()
        assert tuple(r["pair"][:2] if r["kind"] == datapipe.SIBLING else r["pair"][2:]) == (int(f["target"][Pb - 2]), Pb - 1)
        for q in range(4):
            if r["pair"][q] >= 0:
                assert r["counts"][q] == f["counts"][r["pair"][q]] and r["pieces"][q].tobytes() == f["pieces"][r["pair"][q]].tobytes()
            else:
                assert r["counts"][q] == -1 and r["pieces"][q] is None


def _restated_cuts(rng, B, P, K, curvature):
    """The calls _draw_fracture_curved_cuts makes on rng, restated -> (frames [B,R,3,3], half_curv [B,R,2], u_anchor [B,R])"""
    R = (P - 1) * K
    v = rng.randn(B, R, 3)
    n = v / np.linalg.norm(v, axis=2, keepdims=True)
    u_anchor = rng.rand(B, R)
    t = rng.randn(B, R, 3)
    e1 = t - (t * n).sum(2, keepdims=True) * n
    assert (np.linalg.norm(e1, axis=2) >= 1e-12).all()
    e1 = e1 / np.linalg.norm(e1, axis=2, keepdims=True)
    kappa = (2.0 * rng.rand(B, R, 2) - 1.0) * curvature
    return np.stack([e1, np.cross(n, e1), n], axis=2), kappa / 2.0, u_anchor


def _orthonormal(frames):
    g = np.einsum("...ij,...kj->...ik", frames, frames)
    assert np.abs(g - np.eye(3)).max() <= 1e-12
    assert np.abs(np.linalg.det(frames) - 1.0).max() <= 1e-12                 # right-handed: e2 = n x e1


def test_draw_order_of_the_fracture_form():
    from puzzlenet_amd import datapipe
    B, P, K, mag, curvature = 5, 6, 3, 0.8, 2.0
    R = (P - 1) * K
    cols = datapipe._fracture_curved_cols(P, K)
    assert [c.stop - c.start for c in cols] == [9 * R, 2 * R, R, P, 6 * P]
    assert cols[0].start == 0 and all(a.stop == b.start for a, b in zip(cols[:-1], cols[1:]))
    out = np.full((B, cols[-1].stop), np.nan)
    datapipe.draw_fracture_curved_batch(np.random.RandomState(9), torch.Generator().manual_seed(9), B, P, K, mag, curvature, out)
    rng, gen = np.random.RandomState(9), torch.Generator().manual_seed(9)
    frames, half, u_anchor = _restated_cuts(rng, B, P, K, curvature)
    u_start = rng.rand(B, P)
    x = torch.randn(B * P, 6, generator=gen, dtype=torch.float64)
    tw = (x / x.norm(p=2, dim=1, keepdim=True) * mag).numpy().reshape(B, 6 * P)
    for got, want in zip((out[:, c] for c in cols), (frames.reshape(B, -1), half.reshape(B, -1), u_anchor, u_start, tw)):
        assert got.tobytes() == np.ascontiguousarray(want).tobytes()
    _orthonormal(frames)
    assert np.abs(half).max() <= curvature / 2 and half.min() < 0 < half.max()
    # the normals and the anchors are the plane form's for the same seed; the split form returns the same numbers
    normals, anchors, _, _ = datapipe.fracture_draws(np.random.RandomState(9), torch.Generator().manual_seed(9), B, P, K, mag)
    assert frames[:, :, 2].tobytes() == normals.tobytes() and u_anchor.tobytes() == anchors.tobytes()
    split = datapipe.fracture_curved_draws(np.random.RandomState(9), torch.Generator().manual_seed(9), B, P, K, mag, curvature)
    assert [t.shape for t in split] == [(B, P - 1, K, 3, 3), (B, P - 1, K, 2), (B, P - 1, K), (B, P), (B, P, 6)]
    for got, c in zip(split, cols):
        assert got.tobytes() == out[:, c].tobytes()


def test_draw_order_of_the_pair_form():
    from puzzlenet_amd import datapipe
    B, lo, hi, K, mag, curvature = 5, 2, 6, 3, 0.8, 4.0
    R = (hi - 1) * K
    cols = datapipe._fracture_pair_curved_cols(hi, K)
    assert [c.stop - c.start for c in cols] == [9 * R, 2 * R, R, 1, 7, 6]
    assert cols[0].start == 0 and all(a.stop == b.start for a, b in zip(cols[:-1], cols[1:]))
    out = np.full((B, cols[-1].stop), np.nan)
    datapipe.draw_fracture_pair_curved_batch(np.random.RandomState(9), torch.Generator().manual_seed(9), B, lo, hi, K, mag, curvature, out)
    rng, gen = np.random.RandomState(9), torch.Generator().manual_seed(9)
    frames, half, u_anchor = _restated_cuts(rng, B, hi, K, curvature)
    pieces = lo + np.floor(rng.rand(B, 1) * (hi - lo + 1))
    u = rng.rand(B, 7)
    x = torch.randn(B, 6, generator=gen, dtype=torch.float64)
    tw = (x / x.norm(p=2, dim=1, keepdim=True) * mag).numpy()
    for got, want in zip((out[:, c] for c in cols), (frames.reshape(B, -1), half.reshape(B, -1), u_anchor, pieces, u, tw)):
        assert got.tobytes() == np.ascontiguousarray(want).tobytes()
    _orthonormal(frames)
    assert set(out[:, cols[3]].ravel()) <= set(range(lo, hi + 1)) and np.abs(half).max() <= curvature / 2
    mode = datapipe._fracture_pair_curved_mode(lo, hi, curvature)
    assert mode.cols(K)[-1].stop == cols[-1].stop and mode.build is datapipe._build_fracture_pair_curved
    again = np.full_like(out, np.nan)
    mode.draw(np.random.RandomState(9), torch.Generator().manual_seed(9), B, K, mag, again)
    assert again.tobytes() == out.tobytes()


def test_fracture_arguments_are_the_draws_of_either_mode():
    """What the tools' --curvature passes to datapipe.fracture: the plane draws at 0, the curved draws and normals=None above."""
    from puzzlenet_amd import _lib, datapipe
    B, P, K, mag = 3, 4, 2, 0.8
    seeded = lambda: (np.random.RandomState(4), torch.Generator().manual_seed(4))
    plane = datapipe.fracture_arguments(*seeded(), B, P, K, mag, 0.0)
    assert list(plane) == ["normals", "u_anchor", "u_start", "twist"]
    for got, want in zip(plane.values(), datapipe.fracture_draws(*seeded(), B, P, K, mag)):
        assert got.tobytes() == want.tobytes()
    curved = datapipe.fracture_arguments(*seeded(), B, P, K, mag, 2.0)
    assert curved.pop("normals") is None and list(curved) == ["frames", "half_curv", "u_anchor", "u_start", "twist"]
    for got, want in zip(curved.values(), datapipe.fracture_curved_draws(*seeded(), B, P, K, mag, 2.0)):
        assert got.tobytes() == want.tobytes()
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(_lib.PznError, match="curvature"):
            datapipe.fracture_arguments(*seeded(), B, P, K, mag, bad)


def test_a_tangent_along_the_normal_falls_back_to_an_axis():
    """A generator whose tangent draw is the normal itself: nothing of it is left after the projection, and the coordinate axis
    least aligned with the normal takes its place."""
    from puzzlenet_amd import datapipe

    class Rng:
        def __init__(self):
            self.real, self.normal_draw = np.random.RandomState(3), None

        def randn(self, *shape):
            if self.normal_draw is None:
                self.normal_draw = self.real.randn(*shape)
                return self.normal_draw.copy()
            return self.normal_draw / np.linalg.norm(self.normal_draw, axis=2, keepdims=True)

        def rand(self, *shape):
            return self.real.rand(*shape)

    B, P, K = 2, 3, 2
    frames, _, _, _, _ = datapipe.fracture_curved_draws(Rng(), torch.Generator().manual_seed(0), B, P, K, 0.8, 2.0)
    _orthonormal(frames)
    n, e1 = frames[..., 2, :], frames[..., 0, :]
    least = np.argmin(np.abs(n), axis=-1)
    assert (np.argmax(np.abs(e1), axis=-1) == least).all() and (np.take_along_axis(e1, least[..., None], -1) > 0.5).all()


def test_feeder_arguments():
    from puzzlenet_amd import _lib, datapipe
    raw = np.zeros((2, 64, 3), dtype=np.float32)
    for c in (2.0, 0.0):
        with pytest.raises(_lib.PznUnsupported, match="curvature"):
            datapipe.PairFeeder(raw, "cuda:0", curvature=c)                   # without pieces
    with pytest.raises(_lib.PznUnsupported, match="curvature"):
        datapipe.PairFeeder(raw, "cuda:0", cut="sphere", curvature=2.0)
    for c in (-0.5, float("nan"), float("inf"), -float("inf")):
        with pytest.raises(_lib.PznError, match="curvature"):
            datapipe.PairFeeder(raw, "cuda:0", pieces=4, curvature=c)
    with pytest.raises(_lib.PznError):                         # accepted arguments on the CPU: there is no CPU fallback
        datapipe.PairFeeder(raw, "cpu", pieces=(2, 5), curvature=2.0)


def test_the_host_forms_refuse_half_a_surface_and_cpu_tensors():
    from puzzlenet_amd import _lib, datapipe, ops
    z = lambda *s: torch.zeros(*s, dtype=torch.float64)
    with pytest.raises(_lib.PznError):
        ops.fracture_curved(torch.zeros(1, 8, 3), z(1, 1, 2, 3, 3), z(1, 1, 2, 2), z(1, 1, 2), z(1, 2), 1, 8)
    with pytest.raises(_lib.PznError):
        ops.fracture_pair_curved(torch.zeros(1, 8, 3), z(1, 1, 2, 3, 3), z(1, 1, 2, 2), z(1, 1, 2), 2, z(1, 7), 1, 0.5, 8)
    with pytest.raises(_lib.PznError):                         # (refused before the device is looked at)
        datapipe._curved("fracture", None, z(1, 1, 2, 3, 3), None)
    with pytest.raises(_lib.PznError):
        datapipe._curved("fracture", z(1, 1, 2, 3), z(1, 1, 2, 3, 3), z(1, 1, 2, 2))
    assert datapipe._curved("fracture", None, z(1, 1, 2, 3, 3), z(1, 1, 2, 2)) and not datapipe._curved("fracture", z(1), None, None)
    assert datapipe.CurvedFracture._fields == datapipe.Fracture._fields + ("anchor", "frames", "half_curv")
    assert datapipe.CurvedFracturePair._fields == datapipe.FracturePair._fields + ("anchor",)


def test_entry_points_are_declared_and_documented():
    import os
    from puzzlenet_amd import _lib
    assert len(_lib.SIGNATURES["pzn_fracture_curved_f32"][1]) == len(_lib.SIGNATURES["pzn_fracture_f32"][1]) + 2
    assert len(_lib.SIGNATURES["pzn_fracture_pair_curved_f32"][1]) == len(_lib.SIGNATURES["pzn_fracture_pair_f32"][1]) + 2
    assert _lib.PARAMS["pzn_fracture_curved_f32"][1:3] == ["const double* frames", "const double* half_curv"]
    assert "int32_t* anchor" in _lib.PARAMS["pzn_fracture_curved_f32"] and "int32_t* anchor" in _lib.PARAMS["pzn_fracture_pair_curved_f32"]
    assert len(_lib.SIGNATURES["pzn_fracture_curved_supported"][1]) == len(_lib.SIGNATURES["pzn_fracture_pair_curved_supported"][1]) == 3
    doc = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "INTEGRATION.md")).read()
    for name, op in (("pzn_fracture_curved_f32", "ops.fracture_curved"), ("pzn_fracture_pair_curved_f32", "ops.fracture_pair_curved")):
        row = [l for l in doc.splitlines() if l.startswith(f"| `{name}`")]
        assert len(row) == 1 and op in row[0]
