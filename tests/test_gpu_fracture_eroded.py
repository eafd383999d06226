"""GPU: the fracture with material lost along every break - ops.fracture_eroded / ops.fracture_pair_eroded (pzn_fracture_eroded_f32,
pzn_fracture_pair_eroded_f32, csrc/fracture.hip), planes and surfaces, against their numpy statements
datapipe.fracture_eroded_rule / fracture_pair_eroded_rule bit for bit in every output; erosion zero against the four launches
without erosion; a cloud that is lost whole and points exactly on the band's rims; datapipe.fracture and cut_pairs_fracture with
erode= against the ops they are made of; PairFeeder(pieces=..., erosion=..., chip=...)."""
import functools

import numpy as np
import pytest
import torch

from tests import _double_cut as dc
from tests import _fracture_curved as fc
from tests import _fracture_eroded as fe

pytestmark = pytest.mark.gpu

GUARD = 4096      # floats behind the pieces buffer that no launch may touch
SENTINEL = -7.5
FORMS = (False, True)      # curved
GUARDED = (2, 5)           # the shapes whose cap is below their pieces


def _dev():
    return torch.device("cuda:0")


def _to(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(_dev())


def _compare(names, got, want, tag):
    assert len(got) == len(want) == len(names)
    for name, g, w in zip(names, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (tag, name, g.dtype, w.dtype, g.shape, w.shape)
        if g.tobytes() != w.tobytes():
            bad = np.flatnonzero((g != w).reshape(len(g), -1).any(1))
            raise AssertionError(f"{tag}: {name} differs in rows {bad[:8].tolist()} ({len(bad)} of {len(g)})")


def _eroded(raw, form, u_anchor, u_start, erode, n_min, cap):
    from puzzlenet_amd import ops
    got = ops.fracture_eroded(_to(raw), _to(form[0]), _to(u_anchor), _to(u_start), _to(erode), n_min, cap, frames=_to(form[1]),
                              half_curv=_to(form[2]))
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in got]


def _pair_eroded(raw, form, u_anchor, pieces, u, erode, n_min, neighbours, cap):
    from puzzlenet_amd import ops
    got = ops.fracture_pair_eroded(_to(raw), _to(form[0]), _to(u_anchor), _to(np.asarray(pieces, dtype=np.int32)), _to(u), _to(erode),
                                   n_min, neighbours, cap, frames=_to(form[1]), half_curv=_to(form[2]))
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in got]


def _launch_guarded(raw, form, u_anchor, u_start, erode, n_min, cap):
    """pzn_fracture_eroded_f32 through the C ABI on buffers of the test's own, the pieces buffer followed by a guard band.
    -> the outputs in ops.fracture_eroded's order (numpy), the guard band"""
    from puzzlenet_amd import ops
    B, M, _ = raw.shape
    P, K = u_start.shape[1], u_anchor.shape[2]
    dev = _dev()
    d_raw, d_ua, d_us, d_er = (_to(t) for t in (raw, u_anchor, u_start, erode))
    d_form = [_to(t) for t in form]
    ptr = [None if t is None else t.data_ptr() for t in d_form]
    flat = torch.full((P * B * cap * 3 + GUARD,), SENTINEL, dtype=torch.float32, device=dev)
    counts = torch.empty((P * B,), dtype=torch.int64, device=dev)
    start = torch.empty((P * B,), dtype=torch.int64, device=dev)
    ok = torch.empty((B,), dtype=torch.uint8, device=dev)
    label = torch.empty((B, M), dtype=torch.uint8, device=dev)
    order = torch.empty((B, M), dtype=torch.int32, device=dev)
    planes = torch.empty((B, P - 1, 4), dtype=torch.float64, device=dev)
    target, cand, anchor, lost = (torch.empty((B, P - 1), dtype=torch.int32, device=dev) for _ in range(4))
    ops._call("pzn_fracture_eroded_f32", d_raw.data_ptr(), ptr[0], ptr[1], ptr[2], d_ua.data_ptr(), d_us.data_ptr(), d_er.data_ptr(),
              B, M, P, K, n_min, cap, flat.data_ptr(), counts.data_ptr(), start.data_ptr(), label.data_ptr(), order.data_ptr(),
              planes.data_ptr(), target.data_ptr(), cand.data_ptr(), anchor.data_ptr(), lost.data_ptr(), ok.data_ptr(), ops._stream())
    torch.cuda.synchronize()
    body = flat[:P * B * cap * 3].view(P * B, cap, 3)
    out = [t.cpu().numpy() for t in (body, counts, start, label, order, planes, target, cand, anchor, lost, ok.to(torch.bool))]
    return out, flat[P * B * cap * 3:].cpu().numpy()


def _spread(B, P):
    """P_b from 2 to P across the batch, the largest first"""
    return [max(2, P - b * max(1, (P - 2) // max(B - 1, 1))) for b in range(B)]


@functools.lru_cache(maxsize=None)
def _stated(i, curved):
    """The rule on SHAPES[i], computed once -> (inputs, records, the entry point's outputs)"""
    B, M, P, K, n_min, cap = fe.SHAPES[i]
    inputs = fe.inputs(fe.SHAPES[i], curved)
    recs, want = fe.batch_statement(*inputs, n_min, cap)
    return inputs, recs, want


@pytest.mark.parametrize("curved", FORMS, ids=("plane", "curved"))
@pytest.mark.parametrize("i", range(len(fe.SHAPES)), ids=[str(s) for s in fe.SHAPES])
def test_kernel_against_the_rule(i, curved):
    B, M, P, K, n_min, cap = fe.SHAPES[i]
    (raw, form, u_anchor, u_start, erode), recs, want = _stated(i, curved)
    _compare(fe.NAMES, _eroded(raw, form, u_anchor, u_start, erode, n_min, cap), want, (fe.SHAPES[i], curved))
    if i in GUARDED:
        out, band = _launch_guarded(raw, form, u_anchor, u_start, erode, n_min, cap)
        _compare(fe.NAMES, out, want, (fe.SHAPES[i], curved, "guarded"))
        assert (band == SENTINEL).all()                        # nothing behind the last piece's `cap` rows was written
    print(fe.SHAPES[i], "curved" if curved else "plane", "ok", [r["ok"] for r in recs], "lost share",
          [round(float(r["lost"].sum()) / M, 3) for r in recs], "cand", [r["cand"].tolist() for r in recs][:2])
    for b, r in enumerate(recs[:2]):
        fe.check_invariants(raw[b], fe.of_sample(form, b), u_anchor[b], u_start[b], erode[b], n_min, cap, r)
    assert all(r["lost"].sum() > 0 and r["counts"].sum() + r["lost"].sum() == M for r in recs)
    if K > 1 and M != 333:
        # the four shapes with several candidates: every step of every sample is valid, and erosion changed a candidate somewhere
        # (one that leaves n_min points on both sides of its surface no longer does after the loss)
        plain, _ = fe.batch_statement(raw, form, u_anchor, u_start, np.zeros_like(erode), n_min, cap)
        assert all(r["ok"] for r in recs)
        assert sum(int((r["cand"] != q["cand"]).sum()) for r, q in zip(recs, plain)) >= 1


@pytest.mark.parametrize("curved", FORMS, ids=("plane", "curved"))
@pytest.mark.parametrize("i", range(len(fe.SHAPES)), ids=[str(s) for s in fe.SHAPES])
def test_pair_kernel_against_the_rule(i, curved):
    B, M, P, K, n_min, cap = fe.SHAPES[i]
    (raw, form, u_anchor, _, erode), frac, _ = _stated(i, curved)
    u, _ = fc.pair_draws(B, 3000 + M)
    pieces = _spread(B, P)
    recs, want = fe.pair_batch_statement(raw, form, u_anchor, u, erode, pieces, n_min, 0.75, cap)
    _compare(fe.PAIR_NAMES, _pair_eroded(raw, form, u_anchor, pieces, u, erode, n_min, 0.75, cap), want, (fe.SHAPES[i], curved))
    print(fe.SHAPES[i], "pieces", pieces, "kinds", [r["kind"] for r in recs], "ok", [r["ok"] for r in recs])
    for b, r in enumerate(recs):
        assert not r["anchor"][pieces[b] - 1:].any() and not r["lost"][pieces[b] - 1:].any() and not r["planes"][pieces[b] - 1:].any()
        if pieces[b] == P:                                     # the fracture under the pair is the eroded rule's
            assert np.array_equal(r["label"], frac[b]["label"]) and np.array_equal(r["lost"], frac[b]["lost"])


@pytest.mark.parametrize("curved", FORMS, ids=("plane", "curved"))
@pytest.mark.parametrize("i", (2, 3))
def test_erosion_zero_is_the_launch_without(i, curved):
    """erode = 0 through the new kernels against ops.fracture / fracture_curved / fracture_pair / fracture_pair_curved, bit for
    bit on the outputs they share; nothing is lost."""
    from puzzlenet_amd import ops
    B, M, P, K, n_min, cap = fe.SHAPES[i]
    raw, form, u_anchor, u_start, erode = fe.inputs(fe.SHAPES[i], curved)
    zero = np.zeros_like(erode)
    u, _ = fc.pair_draws(B, 3000 + M)
    pieces = _spread(B, P)
    got = dict(zip(fe.NAMES, _eroded(raw, form, u_anchor, u_start, zero, n_min, cap)))
    pair = dict(zip(fe.PAIR_NAMES, _pair_eroded(raw, form, u_anchor, pieces, u, zero, n_min, 0.75, cap)))
    d_raw, d_ua, d_us, d_u, d_pc = _to(raw), _to(u_anchor), _to(u_start), _to(u), _to(np.asarray(pieces, dtype=np.int32))
    if curved:
        old = dict(zip(fc.NAMES, ops.fracture_curved(d_raw, _to(form[1]), _to(form[2]), d_ua, d_us, n_min, cap)))
        old_pair = dict(zip(fc.PAIR_NAMES, ops.fracture_pair_curved(d_raw, _to(form[1]), _to(form[2]), d_ua, d_pc, d_u, n_min, 0.75, cap)))
    else:
        old = dict(zip([n for n in fc.NAMES if n != "anchor"], ops.fracture(d_raw, _to(form[0]), d_ua, d_us, n_min, cap)))
        old_pair = dict(zip([n for n in fc.PAIR_NAMES if n != "anchor"],
                            ops.fracture_pair(d_raw, _to(form[0]), d_ua, d_pc, d_u, n_min, 0.75, cap)))
    torch.cuda.synchronize()
    for new, was in ((got, old), (pair, old_pair)):
        assert not new["lost"].any() and set(new) - set(was) <= {"anchor", "lost"}
        for name, t in was.items():
            w = t.cpu().numpy()
            assert new[name].dtype == w.dtype and new[name].tobytes() == w.tobytes(), (name, curved)


@pytest.mark.parametrize("curved", FORMS, ids=("plane", "curved"))
def test_a_cloud_that_is_lost_whole(curved):
    """M = 64, every width 10: step 1 loses the whole cloud, steps 2 and 3 are not made - beside a sample that is cut as if alone."""
    M, P, K, n_min = 64, 4, 2, 4
    raw = fc.clouds(2, M, 3)
    frames, half_curv, u_anchor, u_start, _ = fc.draws(2, P, K, 4)
    form = (None, frames, half_curv) if curved else (np.ascontiguousarray(frames[:, :, :, 2]), None, None)
    erode = np.full((2, P - 1, 4), 10.0)
    erode[1] = [0.01, 0.01, 0.0, 0.0]
    recs, want = fe.batch_statement(raw, form, u_anchor, u_start, erode, n_min, M)
    assert not recs[0]["ok"] and (recs[0]["label"] == fe.LOST).all() and recs[0]["lost"].tolist() == [M, 0, 0]
    assert recs[1]["counts"].min() > 0
    _compare(fe.NAMES, _eroded(raw, form, u_anchor, u_start, erode, n_min, M), want, "lost whole")
    u = np.full((2, 7), 0.5)
    precs, pwant = fe.pair_batch_statement(raw, form, u_anchor, u, erode, [4, 4], n_min, 0.0, M)
    assert precs[0]["pair"].tolist() == [0, 3, -1, -1] and precs[0]["counts"].tolist() == [0, 0, -1, -1] and not precs[0]["ok"]
    _compare(fe.PAIR_NAMES, _pair_eroded(raw, form, u_anchor, [4, 4], u, erode, n_min, 0.0, M), pwant, "lost whole, pair")


def test_points_exactly_on_the_rims_of_the_band_are_kept():
    raw, forms, u_anchor, u_start, erode, n_min = fe.lattice_case()
    for form in forms:
        recs, want = fe.batch_statement(raw, form, u_anchor, u_start, erode, n_min, raw.shape[1])
        fe.check_lattice_rims(raw, form, erode, recs)
        _compare(fe.NAMES, _eroded(raw, form, u_anchor, u_start, erode, n_min, raw.shape[1]), want, "lattice")


def test_a_nan_row_loses_nothing():
    i = 3
    B, M, P, K, n_min, cap = fe.SHAPES[i]
    raw, form, u_anchor, u_start, erode = fe.inputs(fe.SHAPES[i], True)
    erode = erode.copy()
    erode[:, 1] = np.nan
    erode[:, 2] = [np.nan, 0.02, 0.0, 0.0]
    recs, want = fe.batch_statement(raw, form, u_anchor, u_start, erode, n_min, cap)
    assert all(r["lost"][1] == 0 and r["lost"][2] == 0 and r["lost"][0] > 0 for r in recs)
    _compare(fe.NAMES, _eroded(raw, form, u_anchor, u_start, erode, n_min, cap), want, "nan")


def test_limits_raise_before_any_launch(monkeypatch):
    from puzzlenet_amd import _lib, datapipe as dp, ops
    calls = []
    monkeypatch.setattr(ops, "_call", lambda *a, **k: calls.append(a[0]))
    B, M, K = 2, 64, 3
    dev = _dev()
    raw = _to(fc.clouds(B, M, 1))
    z = lambda *s: torch.zeros(s, dtype=torch.float64, device=dev)
    big = torch.zeros((1, 65537, 3), dtype=torch.float32, device=dev)
    for fn in (ops.fracture_eroded_supported, ops.fracture_pair_eroded_supported):
        assert fn(65536, 16, 1) and not fn(65537, 2, 1) and not fn(64, 1, 1) and not fn(64, 17, 1) and not fn(64, 2, 0)
    n3, fr3, hc3, ua3, us3, u7, er3 = z(B, 2, K, 3), z(B, 2, K, 3, 3), z(B, 2, K, 2), z(B, 2, K), z(B, 3), z(B, 7), z(B, 2, 4)
    for bad in (lambda: ops.fracture_eroded(raw, z(B, 16, K, 3), z(B, 16, K), z(B, 17), z(B, 16, 4), 4, M),                 # P = 17
                lambda: ops.fracture_eroded(big, n3[:1], ua3[:1], us3[:1], er3[:1], 4, 32768),                               # M above the limit
                lambda: ops.fracture_eroded(big, None, ua3[:1], us3[:1], er3[:1], 4, 32768, frames=fr3[:1], half_curv=hc3[:1]),
                lambda: ops.fracture_pair_eroded(raw, z(B, 16, K, 3), z(B, 16, K), 2, u7, z(B, 16, 4), 4, 0.5, M)):
        with pytest.raises(_lib.PznUnsupported):
            bad()
    for bad in (lambda: ops.fracture_eroded(raw.cpu(), n3, ua3, us3, er3, 4, M),                                             # a CPU tensor
                lambda: ops.fracture_eroded(raw, n3, ua3, us3, er3.cpu(), 4, M),
                lambda: ops.fracture_eroded(raw, n3.float(), ua3, us3, er3, 4, M),                                           # wrong dtypes
                lambda: ops.fracture_eroded(raw, n3, ua3, us3, er3.float(), 4, M),
                lambda: ops.fracture_eroded(raw, n3, ua3, us3, er3[:, :1], 4, M),                                            # a row per step
                lambda: ops.fracture_eroded(raw, n3, ua3, us3, z(B, 2, 3), 4, M),                                            # four widths
                lambda: ops.fracture_eroded(raw, n3, ua3, us3, None, 4, M),
                lambda: ops.fracture_eroded(raw, n3, ua3, us3, er3, 4, M, frames=fr3, half_curv=hc3),                        # both forms
                lambda: ops.fracture_eroded(raw, None, ua3, us3, er3, 4, M),                                                 # neither
                lambda: ops.fracture_eroded(raw, None, ua3, us3, er3, 4, M, frames=fr3),                                     # half a surface
                lambda: ops.fracture_eroded(raw, n3, ua3, us3, er3, 4, 0),                                                   # cap = 0
                lambda: ops.fracture_pair_eroded(raw, n3, ua3, 2, u7[:, :6], er3, 4, 0.5, M),                                # six uniforms
                lambda: ops.fracture_pair_eroded(raw, n3, ua3, 2, u7, er3, 4, 1.5, M),                                       # neighbours
                lambda: ops.fracture_pair_eroded(raw, n3, ua3, 1, u7, er3, 4, 0.5, M)):                                      # pieces outside 2 .. P
        with pytest.raises(_lib.PznError):
            bad()
    assert calls == []
    ops.fracture_eroded(raw, n3, ua3, us3, er3, 4, M)
    ops.fracture_pair_eroded(raw, None, ua3, [2, 3], u7, er3, 4, 0.5, M, frames=fr3, half_curv=hc3)
    assert calls == ["pzn_fracture_eroded_f32", "pzn_fracture_pair_eroded_f32"]
    assert dp.FRACTURE_LOST == ops.FRACTURE_LOST == fe.LOST


def test_the_entry_points_refuse_the_shapes_and_the_forms_themselves():
    from puzzlenet_amd import _lib, ops
    raw = _to(fc.clouds(2, 64, 1))
    p, s = raw.data_ptr(), ops._stream()
    lib = _lib.load()
    assert lib.pzn_fracture_eroded_f32(p, p, None, None, p, p, p, 2, 64, 17, 3, 4, 64, p, p, p, p, p, p, p, p, p, p, p, s) == -3
    assert lib.pzn_fracture_eroded_f32(p, None, p, p, p, p, p, 2, 65537, 3, 3, 4, 64, p, p, p, p, p, p, p, p, p, p, p, s) == -3
    assert lib.pzn_fracture_eroded_f32(p, p, p, p, p, p, p, 2, 64, 3, 3, 4, 64, p, p, p, p, p, p, p, p, p, p, p, s) == -1      # both forms
    assert lib.pzn_fracture_eroded_f32(p, None, p, None, p, p, p, 2, 64, 3, 3, 4, 64, p, p, p, p, p, p, p, p, p, p, p, s) == -1  # half of one
    assert lib.pzn_fracture_eroded_f32(p, None, None, None, p, p, p, 2, 64, 3, 3, 4, 64, p, p, p, p, p, p, p, p, p, p, p, s) == -1
    assert lib.pzn_fracture_eroded_f32(p, p, None, None, p, p, None, 2, 64, 3, 3, 4, 64, p, p, p, p, p, p, p, p, p, p, p, s) == -1
    assert lib.pzn_fracture_pair_eroded_f32(p, p, None, None, p, p, p, p, 0.5, 2, 64, 17, 3, 4, 64, p, p, p, p, p, p, p, p, p, p, p,
                                            p, s) == -3
    assert lib.pzn_fracture_pair_eroded_f32(p, p, p, None, p, p, p, p, 0.5, 2, 64, 3, 3, 4, 64, p, p, p, p, p, p, p, p, p, p, p, p,
                                            s) == -1
    assert lib.pzn_fracture_pair_eroded_f32(p, p, None, None, p, p, p, p, 1.5, 2, 64, 3, 3, 4, 64, p, p, p, p, p, p, p, p, p, p, p,
                                            p, s) == -1
    torch.cuda.synchronize()


# --------------------------------------------------------------------------- the host forms

@pytest.mark.parametrize("curved", FORMS, ids=("plane", "curved"))
def test_fracture_sample_with_erosion_against_the_ops_it_is_made_of(curved):
    from puzzlenet_amd import datapipe as dp, ops
    B, M, P, K, n, k = 2, 4096, 4, 8, 256, 32
    raw = fc.clouds(B, M, 40)
    frames, half_curv, u_anchor, u_start, twist = fc.draws(B, P, K, 41)
    form = (None, frames, half_curv) if curved else (np.ascontiguousarray(frames[:, :, :, 2]), None, None)
    erode = fe.widths(B, P, 42)
    d = [_to(t) for t in (raw, form[0], u_anchor, u_start, twist, form[1], form[2], erode)]
    f = dp.fracture(d[0], d[1], d[2], d[3], d[4], n=n, k=k, frames=d[5], half_curv=d[6], erode=d[7])
    packed, counts, start, label, order, planes, target, cand, anchor, lost, ok = ops.fracture_eroded(
        d[0], d[1], d[2], d[3], d[7], n, M, frames=d[5], half_curv=d[6])
    torch.cuda.synchronize()
    base = dp.CurvedFracture if curved else dp.Fracture
    assert type(f) is (dp.ErodedCurvedFracture if curved else dp.ErodedFracture)
    assert f._fields[:len(base._fields)] == base._fields and f._fields[-2:] == ("erode", "lost") and "anchor" in f._fields
    for name, t in (("label", label), ("planes", planes), ("target", target), ("cand", cand), ("anchor", anchor), ("lost", lost),
                    ("counts", counts.view(P, B).t()), ("erode", d[7])):
        assert torch.equal(getattr(f, name), t), name
    recs, _ = fe.batch_statement(raw, form, u_anchor, u_start, erode, n, M)
    assert all(r["ok"] for r in recs) and bool(f.ok.all()) and bool(ok.all())
    assert (f.counts.sum(1) + f.lost.sum(1) == M).all() and bool((f.lost.sum(1) > 0).all())
    idx = ops.farthest_point_sample(packed, n, start, background=True, counts=counts, max_count=0)
    rest = ops.index_points(packed, idx).view(P, B, n, 3).transpose(0, 1)
    assert torch.equal(f.rest, rest)
    src, lab = f.src.cpu().numpy(), f.label.cpu().numpy()
    rest = f.rest.cpu().numpy()
    for b in range(B):
        assert lab[b].tobytes() == recs[b]["label"].tobytes() and (lab[b] == fe.LOST).sum() == recs[b]["lost"].sum()
        for p in range(P):
            assert raw[b][src[b, p]].tobytes() == rest[b, p].tobytes(), (b, p)                   # src: the cloud's own rows,
            assert (lab[b][src[b, p]] == p).all()                                                # none of them a lost one
    cd, mates = f.cd.cpu().numpy(), f.mates.cpu().numpy()
    assert np.array_equal(mates, (cd <= np.float32(dp.CD_ACCEPT)) & ~np.eye(P, dtype=bool))
    plain = dp.fracture(d[0], d[1], d[2], d[3], d[4], n=n, k=k, frames=d[5], half_curv=d[6])
    assert type(plain) is base                                  # erode=None: today's call and today's result type
    pile = dp.pile(f, 2)
    assert pile.pieces.shape == (1, 2 * P, n, 3) and torch.equal(pile.pieces[0, :P], f.pieces[0])
    print("mates per sample", mates.sum((1, 2)).tolist(), "without erosion", plain.mates.sum((1, 2)).tolist(), "lost",
          f.lost.sum(1).tolist())


def _stated_pairs(recs, which, twist, n, k):
    """The statement's pieces (which[b] = True: the fallback pair) sampled by ops.farthest_point_sample from the stated start
    indices and passed through datapipe.pairs_from_pieces."""
    from puzzlenet_amd import datapipe as dp, ops
    B = len(recs)
    rows = {False: (0, 1), True: (2, 3)}
    U = _to(np.stack([recs[b]["pieces"][rows[bool(which[b])][0]] for b in range(B)]))
    D = _to(np.stack([recs[b]["pieces"][rows[bool(which[b])][1]] for b in range(B)]))
    s_u = np.array([recs[b]["start"][rows[bool(which[b])][0]] for b in range(B)], dtype=np.int64)
    s_d = np.array([recs[b]["start"][rows[bool(which[b])][1]] for b in range(B)], dtype=np.int64)
    Us = ops.index_points(U, ops.farthest_point_sample(U, n, _to(s_u)))
    Ds = ops.index_points(D, ops.farthest_point_sample(D, n, _to(s_d)))
    return dp.pairs_from_pieces(Us, Ds, _to(twist), k)


@pytest.mark.parametrize("curved", FORMS, ids=("plane", "curved"))
def test_cut_pairs_fracture_with_erosion_against_the_ops_it_is_made_of(curved):
    from puzzlenet_amd import datapipe as dp
    B, M, P, K, n, k = 4, 4096, 5, 8, 256, 32
    raw = fc.clouds(B, M, 520)
    frames, half_curv, u_anchor, _, _ = fc.draws(B, P, K, 521)
    form = (None, frames, half_curv) if curved else (np.ascontiguousarray(frames[:, :, :, 2]), None, None)
    u, twist = fc.pair_draws(B, 522)
    u[:, 0] = [0.1, 0.1, 0.9, 0.1]
    pieces = [5, 4, 5, 3]
    erode = fe.widths(B, P, 523)
    recs, _ = fe.pair_batch_statement(raw, form, u_anchor, u, erode, pieces, n, 0.5, M)
    assert {r["kind"] for r in recs} == {dp.SIBLING, dp.NEIGHBOUR}
    got, ok, rec = dp.cut_pairs_fracture(_to(raw), _to(form[0]), _to(u_anchor), pieces, _to(u), _to(twist), n=n, k=k, neighbours=0.5,
                                         frames=_to(form[1]), half_curv=_to(form[2]), erode=_to(erode))
    torch.cuda.synchronize()
    base = dp.CurvedFracturePair if curved else dp.FracturePair
    assert type(rec) is (dp.ErodedCurvedFracturePair if curved else dp.ErodedFracturePair)
    assert rec._fields[:len(base._fields)] == base._fields and rec._fields[-2:] == ("erode", "lost") and "anchor" in rec._fields
    assert ok.cpu().tolist() == [bool(r["ok"] and min(r["counts"][:2]) >= n) for r in recs]
    assert rec.kind.cpu().tolist() == [r["kind"] for r in recs] and rec.pair.cpu().tolist() == [r["pair"].tolist() for r in recs]
    for name in ("label", "planes", "target", "cand", "anchor", "lost"):
        assert getattr(rec, name).cpu().numpy().tobytes() == np.stack([r[name] for r in recs]).tobytes(), name
    assert rec.erode.cpu().numpy().tobytes() == erode.tobytes()
    rejected = rec.rejected.cpu().numpy()
    assert not (rejected & (rec.kind.cpu().numpy() != 1)).any()
    primary = _stated_pairs(recs, [False] * B, twist, n, k)
    assert torch.equal(rec.U, primary[3]) and torch.equal(rec.D, primary[0])
    assert torch.equal(rec.Ub, primary[5]) and torch.equal(rec.Db, primary[4])
    has_fallback = [r["kind"] == 1 for r in recs]
    fallback = _stated_pairs([dict(pieces=r["pieces"] if f else r["pieces"][:2] * 2, start=r["start"] if f else list(r["start"][:2]) * 2)
                              for r, f in zip(recs, has_fallback)], [True] * B, twist, n, k)
    for b in range(B):
        want = fallback if rejected[b] else primary
        for g, w in zip(got, want):
            assert torch.equal(g[b], w[b]), (b, bool(rejected[b]))
    print("kinds", rec.kind.cpu().tolist(), "rejected", rejected.tolist(), "cd", rec.cd.cpu().tolist(), "ok", ok.cpu().tolist())


# --------------------------------------------------------------------------- the feeder

def test_eroded_feeder_against_cut_pairs_fracture_on_its_own_draws():
    """Two batches of PairFeeder(pieces=(2, 5), erosion=0.02, chip=(0.05, 0.1)): the staged draws restated from the seed - the
    mode's own, then draw_erosion from the same rng - and cut_pairs_fracture on them, tensor by tensor."""
    from puzzlenet_amd import datapipe as dp
    dev = _dev()
    B, M, N, K, seed, lo, hi = 8, 2048, 256, 8, 11, 2, 5
    raw = dc.shells(B, M, 21)
    f = dp.PairFeeder(raw, dev, n=N, k=64, candidates=K, seed=seed, pieces=(lo, hi), erosion=0.02, chip=(0.05, 0.1))
    cols = dp._fracture_pair_cols(hi, K)
    assert f._width == cols[-1].stop + 4 * (hi - 1) and f.erosion == 0.02 and f.chip == (0.05, 0.1)
    rng, gen = np.random.RandomState(seed), torch.Generator().manual_seed(seed)
    lost = 0
    for _ in range(2):
        batch = f.next_batch()
        batch.ready.synchronize()
        st = np.empty((B, cols[-1].stop))
        dp.draw_fracture_pair_batch(rng, gen, B, lo, hi, K, 0.8, st)
        erode = dp.draw_erosion(rng, B, hi, 0.02, (0.05, 0.1))
        normals, u_anchor, pc, u, tw = (np.ascontiguousarray(st[:, c]) for c in cols)
        want, ok, rec = dp.cut_pairs_fracture(_to(raw), _to(normals.reshape(B, hi - 1, K, 3)), _to(u_anchor.reshape(B, hi - 1, K)),
                                              _to(pc.reshape(B).astype(np.int32)), _to(u), _to(tw), n=N, k=64, neighbours=0.5,
                                              erode=_to(erode))
        torch.cuda.synchronize()
        assert type(batch.fracture) is dp.ErodedFracturePair and batch.plane is None
        assert all(torch.equal(g, w) for g, w in zip(batch, want)) and torch.equal(batch.ok, ok)
        assert all(torch.equal(g, w) for g, w in zip(batch.fracture, rec))
        lost += int(rec.lost.sum())
    f.close()
    assert lost > 0


def test_erosion_none_is_the_feeder_without():
    """PairFeeder(pieces=...) with erosion=None, and with erosion=0.0 and an empty chip: today's mode, draws and bits."""
    from puzzlenet_amd import datapipe as dp
    dev = _dev()
    raw = dc.shells(8, 2048, 3)
    f = dp.PairFeeder(raw, dev, n=256, k=64, candidates=8, seed=7, pieces=(2, 5))
    g = dp.PairFeeder(raw, dev, n=256, k=64, candidates=8, seed=7, pieces=(2, 5), erosion=None)
    h = dp.PairFeeder(raw, dev, n=256, k=64, candidates=8, seed=7, pieces=(2, 5), erosion=0.0, chip=(0.0, 0.0))
    assert f._width == g._width == h._width == dp._fracture_pair_cols(5, 8)[-1].stop
    assert f._mode.build is g._mode.build is h._mode.build is dp._build_fracture_pair
    x, y, z = f.next_batch(), g.next_batch(), h.next_batch()
    for b in (x, y, z):
        b.ready.synchronize()
    for other in (y, z):
        assert all(torch.equal(s, t) for s, t in zip(x, other)) and torch.equal(x.ok, other.ok)
        assert type(other.fracture) is dp.FracturePair and all(torch.equal(s, t) for s, t in zip(x.fracture, other.fracture))
    for feeder in (f, g, h):
        feeder.close()
