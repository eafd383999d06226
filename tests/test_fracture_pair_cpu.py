"""CPU: datapipe.fracture_pair_rule, the numpy statement of the fracture loader (PairFeeder(pieces=...)): its fracture against
fracture_rule on the same draws, the sibling pair against the fracture one cut earlier, the pair draw over a grid, the edges of
`neighbours`, cap and the shapes without a valid cut; and the plumbing (staging columns, draw order, the feeder's refusals).
The kernel is held to the statement in tests/test_gpu_fracture_pair.py."""
import numpy as np
import pytest
import torch

from tests import _fracture as fr
from tests import _fracture_pair as fp

M, K, N_MIN = 1000, 4, 64


def _inputs(P, seed, B=1):
    raw = fp.clouds(B, M, seed)
    normals, u_anchor, u, _ = fp.draws(B, P, K, seed + 1)
    return raw, normals, u_anchor, u


def _rule(raw, normals, u_anchor, u, Pb, P, neighbours=0.5, n_min=N_MIN, cap=None):
    from puzzlenet_amd import datapipe
    return datapipe.fracture_pair_rule(raw, normals, u_anchor, u, Pb, P, n_min, neighbours, cap)


@pytest.mark.parametrize("P", [2, 3, 5, 8])
def test_with_every_piece_the_fracture_is_fracture_rules(P):
    from puzzlenet_amd import datapipe
    raw, normals, u_anchor, u = _inputs(P, 10 + P, B=3)
    for b in range(3):
        r = _rule(raw[b], normals[b], u_anchor[b], u[b], P, P)
        f = datapipe.fracture_rule(raw[b], normals[b], u_anchor[b], np.zeros(P), P, N_MIN, M)
        for key in ("label", "planes", "target", "cand"):
            assert r[key].dtype == f[key].dtype and r[key].tobytes() == f[key].tobytes(), (P, b, key)
        fp.check_invariants(raw[b], normals[b], u_anchor[b], u[b], P, N_MIN, 0.5, M, r)


@pytest.mark.parametrize("Pb", [2, 3, 4, 6])
def test_with_fewer_pieces_it_is_the_smaller_fracture_and_the_rows_beyond_are_zero(Pb):
    from puzzlenet_amd import datapipe
    P = 7
    raw, normals, u_anchor, u = _inputs(P, 20 + Pb, B=3)
    for b in range(3):
        r = _rule(raw[b], normals[b], u_anchor[b], u[b], Pb, P)
        f = datapipe.fracture_rule(raw[b], normals[b, :Pb - 1], u_anchor[b, :Pb - 1], np.zeros(Pb), Pb, N_MIN, M)
        assert r["label"].tobytes() == f["label"].tobytes()
        for key in ("planes", "target", "cand"):
            assert r[key].shape[0] == P - 1 and r[key][:Pb - 1].tobytes() == f[key].tobytes(), (Pb, b, key)
            assert not r[key][Pb - 1:].any()
        fp.check_invariants(raw[b], normals[b], u_anchor[b], u[b], Pb, N_MIN, 0.5, M, r)
        # later draw rows are not read
        other = normals[b].copy()
        other[Pb - 1:] = np.nan
        r2 = _rule(raw[b], other, u_anchor[b], u[b], Pb, P)
        assert r2["label"].tobytes() == r["label"].tobytes() and r2["planes"].tobytes() == r["planes"].tobytes()


@pytest.mark.parametrize("Pb", [2, 3, 5])
def test_the_sibling_pair_is_the_last_cut_of_the_fracture_one_piece_earlier(Pb):
    from puzzlenet_amd import datapipe
    P = 5
    raw, normals, u_anchor, u = _inputs(P, 30 + Pb, B=4)
    seen_ok = 0
    for b in range(4):
        r = _rule(raw[b], normals[b], u_anchor[b], u[b], Pb, P, neighbours=0.0)
        assert r["kind"] == datapipe.SIBLING
        t = int(r["target"][Pb - 2])
        assert tuple(r["pair"]) == (t, Pb - 1, -1, -1)
        if Pb == 2:
            before = np.zeros(M, dtype=np.uint8)
        else:
            before = datapipe.fracture_rule(raw[b], normals[b, :Pb - 2], u_anchor[b, :Pb - 2], np.zeros(Pb - 1), Pb - 1, N_MIN, M)["label"]
        U, D = r["label"] == t, r["label"] == Pb - 1
        assert np.array_equal(U | D, before == t) and not (U & D).any()               # exactly that label, split in two
        assert np.array_equal(r["label"][~(U | D)], before[~(U | D)])                 # and nothing else moved
        plane = r["planes"][Pb - 2]
        assert (fr.side(raw[b][U], plane) >= 0).all() and (fr.side(raw[b][D], plane) < 0).all()
        assert r["pieces"][0][:U.sum()].tobytes() == raw[b][U].tobytes() and r["pieces"][1][:D.sum()].tobytes() == raw[b][D].tobytes()
        if r["ok"]:
            seen_ok += 1
            assert U.sum() >= N_MIN and D.sum() >= N_MIN and r["counts"][:2].tolist() == [U.sum(), D.sum()]
            assert np.bincount(r["label"], minlength=Pb).min() >= N_MIN               # every final piece, not only the pair
    assert seen_ok >= 2


def test_the_pair_draw_reaches_every_ordered_pair_and_folds_the_sibling_orders():
    from puzzlenet_amd import datapipe
    P = Pb = 5
    raw, normals, u_anchor, u = _inputs(P, 41)
    base = _rule(raw[0], normals[0], u_anchor[0], u[0], Pb, P, neighbours=0.0)
    sib = (int(base["target"][Pb - 2]), Pb - 1)
    seen = {}
    for u_a in (np.arange(40) + 0.5) / 40:
        for u_c in (np.arange(40) + 0.5) / 40:
            uu = u[0].copy()
            uu[:3] = (0.3, u_a, u_c)
            r = _rule(raw[0], normals[0], u_anchor[0], uu, Pb, P, neighbours=1.0)
            a = min(Pb - 1, int(np.floor(u_a * Pb)))
            c = min(Pb - 2, int(np.floor(u_c * (Pb - 1))))
            c += c >= a
            assert a != c
            seen.setdefault((a, c), r)
            if {a, c} == set(sib):
                assert r["kind"] == datapipe.SIBLING and tuple(r["pair"]) == sib + (-1, -1)
                assert r["counts"][2:].tolist() == [-1, -1] and r["start"][2:].tolist() == [0, 0]
                assert r["pieces"][2] is None and r["pieces"][3] is None
            else:
                assert r["kind"] == datapipe.NEIGHBOUR and tuple(r["pair"]) == (a, c) + sib
                assert (r["counts"] >= 0).all()
                assert r["counts"].tolist() == [int((r["label"] == p).sum()) for p in r["pair"]]
    assert sorted(seen) == [(a, c) for a in range(5) for c in range(5) if a != c]     # all 20
    assert sum(r["kind"] == datapipe.SIBLING for r in seen.values()) == 2
    # the draws at the ends of [0, 1)
    top = 1.0 - 2.0 ** -53
    uu = u[0].copy()
    uu[:3] = (0.0, top, top)
    r = _rule(raw[0], normals[0], u_anchor[0], uu, Pb, P, neighbours=1.0)
    assert tuple(r["pair"][:2]) in ((4, 3), sib)
    uu[:3] = (0.0, 0.0, 0.0)
    r = _rule(raw[0], normals[0], u_anchor[0], uu, Pb, P, neighbours=1.0)
    assert tuple(r["pair"][:2]) in ((0, 1), sib)


def test_two_pieces_are_always_the_sibling_pair_and_neighbours_has_hard_edges():
    from puzzlenet_amd import _lib, datapipe
    P = 4
    raw, normals, u_anchor, u = _inputs(P, 51)
    for u_kind in (0.0, 0.25, 0.5, 1.0 - 2.0 ** -53):
        uu = u[0].copy()
        uu[0] = u_kind
        for q in (0.0, 0.5, 1.0):
            r = _rule(raw[0], normals[0], u_anchor[0], uu, 2, P, neighbours=q)
            assert r["kind"] == datapipe.SIBLING and tuple(r["pair"]) == (0, 1, -1, -1)
        for Pb in (3, 4):
            r0 = _rule(raw[0], normals[0], u_anchor[0], uu, Pb, P, neighbours=0.0)
            assert r0["kind"] == datapipe.SIBLING                                     # u_kind < 0 never holds
            r1 = _rule(raw[0], normals[0], u_anchor[0], uu, Pb, P, neighbours=1.0)
            sib = (int(r1["target"][Pb - 2]), Pb - 1)
            a = min(Pb - 1, int(np.floor(uu[1] * Pb)))
            c = min(Pb - 2, int(np.floor(uu[2] * (Pb - 1))))
            c += c >= a
            assert (r1["kind"] == datapipe.NEIGHBOUR) == ({a, c} != set(sib))         # u_kind < 1 always holds
            fp.check_invariants(raw[0], normals[0], u_anchor[0], uu, Pb, N_MIN, 1.0, M, r1)
    # the threshold itself: u_kind < neighbours, strictly
    uu = u[0].copy()
    uu[:3] = (0.5, 0.1, 0.9)                                                          # (a, c) = (0, 3) at P_b = 4
    at = _rule(raw[0], normals[0], u_anchor[0], uu, 4, P, neighbours=0.5)
    above = _rule(raw[0], normals[0], u_anchor[0], uu, 4, P, neighbours=np.nextafter(0.5, 1.0))
    assert at["kind"] == datapipe.SIBLING
    assert above["kind"] == (datapipe.NEIGHBOUR if {0, 3} != {int(above["target"][2]), 3} else datapipe.SIBLING)
    for bad in (dict(Pb=1), dict(Pb=5), dict(neighbours=-0.1), dict(neighbours=1.5)):
        with pytest.raises(_lib.PznError):
            _rule(raw[0], normals[0], u_anchor[0], u[0], bad.get("Pb", 3), P, neighbours=bad.get("neighbours", 0.5))


def test_rejection_is_neighbour_above_the_reference_bound():
    from puzzlenet_amd import datapipe as dp
    kind = np.array([dp.SIBLING, dp.NEIGHBOUR, dp.NEIGHBOUR, dp.SIBLING])
    cd = np.array([1.0, 0.015, np.nextafter(0.015, 1.0), 0.0])
    assert dp.fracture_pair_rejects(kind, cd).tolist() == [False, False, True, False]
    assert dp.fracture_pair_rejects(torch.from_numpy(kind), torch.from_numpy(cd)).tolist() == [False, False, True, False]


def test_cap_truncates_the_written_pieces_and_clears_ok():
    P = Pb = 3
    raw, normals, u_anchor, u = _inputs(P, 61)
    uu = u[0].copy()
    uu[0] = 0.9
    full = _rule(raw[0], normals[0], u_anchor[0], uu, Pb, P, neighbours=0.5, cap=M)
    assert full["ok"] and full["kind"] == 0
    small = int(full["counts"][:2].max()) - 1
    cut = _rule(raw[0], normals[0], u_anchor[0], uu, Pb, P, neighbours=0.5, cap=small)
    assert not cut["ok"] and cut["label"].tobytes() == full["label"].tobytes() and np.array_equal(cut["counts"], full["counts"])
    fp.check_invariants(raw[0], normals[0], u_anchor[0], uu, Pb, N_MIN, 0.5, small, cut)
    # only WRITTEN pieces count: a third piece above cap does not clear ok
    third = ({0, 1, 2} - {int(p) for p in full["pair"][:2]}).pop()
    n_third = int((full["label"] == third).sum())
    fits = int(full["counts"][:2].max())
    if n_third > fits:
        assert _rule(raw[0], normals[0], u_anchor[0], uu, Pb, P, neighbours=0.5, cap=fits)["ok"]


@pytest.mark.parametrize("shape", fr.NOT_OK_SHAPES, ids=str)
def test_shapes_where_some_cuts_are_not_valid(shape):
    from puzzlenet_amd import datapipe
    Ms, P, Ks, n_min = shape
    B = {333: 32, 2048: 16}[Ms]                                                       # (the fracture tests' sample counts and seeds)
    raw = fp.clouds(B, Ms, 200 + Ms % 97)
    normals, u_anchor, u, _ = fp.draws(B, P, Ks, 201 + Ms % 97)
    oks = []
    for b in range(B):
        r = datapipe.fracture_pair_rule(raw[b], normals[b], u_anchor[b], u[b], P, P, n_min, 0.5, Ms)
        f = datapipe.fracture_rule(raw[b], normals[b], u_anchor[b], np.zeros(P), P, n_min, Ms)
        assert r["label"].tobytes() == f["label"].tobytes() and r["cand"].tobytes() == f["cand"].tobytes()
        assert r["ok"] == f["ok"]                                                     # cap = M: the steps alone decide
        fp.check_invariants(raw[b], normals[b], u_anchor[b], u[b], P, n_min, 0.5, Ms, r)
        oks.append(r["ok"])
    print(shape, "ok", oks)
    assert not all(oks)                                                               # the most-balanced path is in the comparison


def test_staging_columns_and_draw_order():
    from puzzlenet_amd import datapipe, ops
    B, lo, hi, Kc, mag = 5, 2, 6, 3, 0.8
    cols = datapipe._fracture_pair_cols(hi, Kc)
    widths = [c.stop - c.start for c in cols]
    assert widths == [3 * (hi - 1) * Kc, (hi - 1) * Kc, 1, 7, 6] and ops.FRACTURE_PAIR_UNIFORMS == 7
    assert cols[0].start == 0 and all(a.stop == b.start for a, b in zip(cols[:-1], cols[1:]))
    out = np.full((B, cols[-1].stop), np.nan)
    datapipe.draw_fracture_pair_batch(np.random.RandomState(9), torch.Generator().manual_seed(9), B, lo, hi, Kc, mag, out)
    # the calls made on the generators, restated: what a seed means
    rng, gen = np.random.RandomState(9), torch.Generator().manual_seed(9)
    v = rng.randn(B, (hi - 1) * Kc, 3)
    want_normals = (v / np.linalg.norm(v, axis=2, keepdims=True)).reshape(B, -1)
    want_anchor = rng.rand(B, (hi - 1) * Kc)
    want_pieces = lo + np.floor(rng.rand(B, 1) * (hi - lo + 1))
    want_u = rng.rand(B, 7)
    x = torch.randn(B, 6, generator=gen, dtype=torch.float64)
    want_tw = (x / x.norm(p=2, dim=1, keepdim=True) * mag).numpy()
    for got, want in zip((out[:, c] for c in cols), (want_normals, want_anchor, want_pieces, want_u, want_tw)):
        assert got.tobytes() == np.ascontiguousarray(want).tobytes()
    assert set(out[:, cols[2]].ravel()) <= set(range(lo, hi + 1))
    # the cut draws are draw_fracture_batch's for P = hi
    f_normals, f_anchor, _, _ = datapipe.fracture_draws(np.random.RandomState(9), torch.Generator().manual_seed(9), B, hi, Kc, mag)
    assert f_normals.reshape(B, -1).tobytes() == out[:, cols[0]].tobytes() and f_anchor.reshape(B, -1).tobytes() == out[:, cols[1]].tobytes()
    # a fixed count: lo = hi; over many draws every count of a range occurs
    cols4 = datapipe._fracture_pair_cols(4, Kc)
    out4 = np.empty((B, cols4[-1].stop))
    datapipe.draw_fracture_pair_batch(np.random.RandomState(1), torch.Generator().manual_seed(1), B, 4, 4, Kc, mag, out4)
    assert (out4[:, cols4[2]] == 4).all()
    big = np.empty((400, cols[-1].stop))
    datapipe.draw_fracture_pair_batch(np.random.RandomState(2), torch.Generator().manual_seed(2), 400, lo, hi, Kc, mag, big)
    assert set(big[:, cols[2]].ravel()) == set(range(lo, hi + 1))
    mode = datapipe._fracture_pair_mode(lo, hi)
    assert mode.cols(Kc)[-1].stop == cols[-1].stop and mode.build is datapipe._build_fracture_pair


def test_feeder_refuses_before_the_device_is_looked_at():
    from puzzlenet_amd import _lib, datapipe
    raw = np.zeros((2, 64, 3), dtype=np.float32)
    for cut in ("sphere", "cylinder", "cone"):
        with pytest.raises(_lib.PznUnsupported, match="pieces"):
            datapipe.PairFeeder(raw, "cuda:0", cut=cut, pieces=4)
    with pytest.raises(_lib.PznUnsupported, match="pieces"):
        datapipe.PairFeeder(raw, "cuda:0", split_twice=True, pieces=4)
    for bad in (1, 17, (1, 4), (3, 2), (2, 17), 0):
        with pytest.raises(_lib.PznUnsupported, match="pieces"):
            datapipe.PairFeeder(raw, "cuda:0", pieces=bad)
    for q in (-0.01, 1.01, float("nan")):
        with pytest.raises(_lib.PznError, match="neighbours"):
            datapipe.PairFeeder(raw, "cuda:0", pieces=4, neighbours=q)
    with pytest.raises(_lib.PznError):                      # accepted arguments on the CPU: there is no CPU fallback
        datapipe.PairFeeder(raw, "cpu", pieces=(2, 5), neighbours=1.0)


def test_ops_fracture_pair_rejects_cpu_tensors():
    from puzzlenet_amd import _lib, ops
    z = lambda *s: torch.zeros(*s, dtype=torch.float64)
    with pytest.raises(_lib.PznError):
        ops.fracture_pair(torch.zeros(1, 8, 3), z(1, 1, 2, 3), z(1, 1, 2), 2, z(1, 7), 1, 0.5, 8)


def test_header_binding_table_and_integration_index_name_the_entry_points():
    import os
    from puzzlenet_amd import _lib
    args = _lib.PARAMS["pzn_fracture_pair_f32"]
    res, bound = _lib.SIGNATURES["pzn_fracture_pair_f32"]
    assert res is _lib._c_i and len(bound) == len(args) == 23
    assert args[3:6] == ["const int32_t* n_pieces", "const double* u", "double neighbours"] and bound[5] is __import__("ctypes").c_double
    assert args[6:12] == ["int B", "int M", "int P", "int K", "int n_min", "int cap"] and args[-1] == "pzn_stream_t stream"
    assert len(_lib.SIGNATURES["pzn_fracture_pair_supported"][1]) == 3
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    doc = open(os.path.join(root, "INTEGRATION.md")).read()
    row = [l for l in doc.splitlines() if l.startswith("| `pzn_fracture_pair_f32`")]
    assert len(row) == 1 and "ops.fracture_pair" in row[0] and "pzn_fracture_pair_supported" in row[0]
