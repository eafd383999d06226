"""GPU: the fracture along curved surfaces - ops.fracture_curved / ops.fracture_pair_curved (pzn_fracture_curved_f32,
pzn_fracture_pair_curved_f32, csrc/fracture.hip) against their numpy statements datapipe.fracture_curved_rule /
fracture_pair_curved_rule bit for bit in every output; zero curvature against the plane kernels where both are exact;
datapipe.fracture and cut_pairs_fracture with surfaces against the ops they are made of; PairFeeder(pieces=..., curvature=...)."""
import numpy as np
import pytest
import torch

from tests import _double_cut as dc
from tests import _fracture as fr
from tests import _fracture_curved as fc

pytestmark = pytest.mark.gpu

GUARD = 4096      # floats behind the pieces buffer that no launch may touch
SENTINEL = -7.5
CASES_OF_CURVATURE = ("random", "cylinder", "saddle", "eight", "zero")


def _dev():
    return torch.device("cuda:0")


def _to(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(_dev())


def _compare(names, got, want, tag):
    assert len(got) == len(want) == len(names)
    for name, g, w in zip(names, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (tag, name, g.dtype, w.dtype, g.shape, w.shape)
        if g.tobytes() != w.tobytes():
            bad = np.flatnonzero((g != w).reshape(len(g), -1).any(1))
            raise AssertionError(f"{tag}: {name} differs in rows {bad[:8].tolist()} ({len(bad)} of {len(g)})")


def _launch_guarded(raw, frames, half_curv, u_anchor, u_start, n_min, cap):
    """pzn_fracture_curved_f32 through the C ABI on buffers of the test's own, the pieces buffer followed by a guard band.
    -> the outputs in ops.fracture_curved's order (numpy), the guard band"""
    from puzzlenet_amd import ops
    B, M, _ = raw.shape
    P, K = u_start.shape[1], frames.shape[2]
    dev = _dev()
    d_raw, d_frames, d_hc, d_ua, d_us = (_to(t) for t in (raw, frames, half_curv, u_anchor, u_start))
    flat = torch.full((P * B * cap * 3 + GUARD,), SENTINEL, dtype=torch.float32, device=dev)
    counts = torch.empty((P * B,), dtype=torch.int64, device=dev)
    start = torch.empty((P * B,), dtype=torch.int64, device=dev)
    ok = torch.empty((B,), dtype=torch.uint8, device=dev)
    label = torch.empty((B, M), dtype=torch.uint8, device=dev)
    order = torch.empty((B, M), dtype=torch.int32, device=dev)
    planes = torch.empty((B, P - 1, 4), dtype=torch.float64, device=dev)
    target, cand, anchor = (torch.empty((B, P - 1), dtype=torch.int32, device=dev) for _ in range(3))
    ops._call("pzn_fracture_curved_f32", d_raw.data_ptr(), d_frames.data_ptr(), d_hc.data_ptr(), d_ua.data_ptr(), d_us.data_ptr(), B,
              M, P, K, n_min, cap, flat.data_ptr(), counts.data_ptr(), start.data_ptr(), label.data_ptr(), order.data_ptr(),
              planes.data_ptr(), target.data_ptr(), cand.data_ptr(), anchor.data_ptr(), ok.data_ptr(), ops._stream())
    torch.cuda.synchronize()
    body = flat[:P * B * cap * 3].view(P * B, cap, 3)
    out = [t.cpu().numpy() for t in (body, counts, start, label, order, planes, target, cand, anchor, ok.to(torch.bool))]
    return out, flat[P * B * cap * 3:].cpu().numpy()


def _run_and_compare(raw, frames, half_curv, u_anchor, u_start, n_min, cap, tag, guarded=False):
    """ops.fracture_curved (and the launch on guarded buffers) against the statement -> the statement's records"""
    from puzzlenet_amd import ops
    recs, want = fc.batch_statement(raw, frames, half_curv, u_anchor, u_start, n_min, cap)
    got = ops.fracture_curved(_to(raw), _to(frames), _to(half_curv), _to(u_anchor), _to(u_start), n_min, cap)
    torch.cuda.synchronize()
    _compare(fc.NAMES, [t.cpu().numpy() for t in got], want, tag)
    if guarded:
        out, band = _launch_guarded(raw, frames, half_curv, u_anchor, u_start, n_min, cap)
        _compare(fc.NAMES, out, want, (tag, "guarded"))
        assert (band == SENTINEL).all(), tag                   # nothing behind the last piece's `cap` rows was written
    return recs


def _run_pair_and_compare(raw, frames, half_curv, u_anchor, u, pieces, n_min, neighbours, cap, tag):
    from puzzlenet_amd import ops
    recs, want = fc.pair_batch_statement(raw, frames, half_curv, u_anchor, u, pieces, n_min, neighbours, cap)
    got = ops.fracture_pair_curved(_to(raw), _to(frames), _to(half_curv), _to(u_anchor), _to(np.asarray(pieces, dtype=np.int32)),
                                   _to(u), n_min, neighbours, cap)
    torch.cuda.synchronize()
    _compare(fc.PAIR_NAMES, [t.cpu().numpy() for t in got], want, tag)
    return recs


def _spread(B, P):
    """P_b from 2 to P across the batch, the largest first"""
    return [max(2, P - b * max(1, (P - 2) // max(B - 1, 1))) for b in range(B)]


# (B, M, P, K, n_min, cap)
SHAPES = [
    (3, 257, 2, 1, 8, 257),                 # one cut, one candidate, M below the thread count
    (2, 1000, 5, 17, 64, 1000),             # K > 16: the second chunk of the anchor table
    (2, 1025, 16, 4, 16, 400),              # runs of 2 points, the largest P, a cap below the first pieces
    (2, 4096, 8, 8, 128, 4096),
    (1, 65536, 16, 16, 1024, 32768),        # the M limit: runs of 64 points, more than 64 KiB of LDS
    (2, 333, 16, 2, 4, 30),                # steps without a valid candidate, a cap below the largest piece
    (4, 2048, 5, 1, 64, 500),               # K = 1: the most-balanced path, a cap below the largest piece
]
SALT = {333: 1}
# every shape with the curvatures as drawn; the other curvature cases on the two shapes with several candidates and steps
CASES = [(s, "random") for s in SHAPES] + [(s, c) for s in (SHAPES[1], SHAPES[3]) for c in CASES_OF_CURVATURE[1:]]


def _inputs(shape, case):
    B, M, P, K, n_min, cap = shape
    salt = M + P + SALT.get(M, 0)
    raw = fc.clouds(B, M, 1000 + salt)
    frames, half_curv, u_anchor, u_start, _ = fc.draws(B, P, K, 2000 + salt)
    half_curv = fc.shaped(half_curv, case, salt)
    if K > 16 and case == "random":
        # sixteen bowls so tight (kappa = 80: below one lies a needle of about 1 % of the cube) that none leaves n_min points on
        # its down side: the seventeenth candidate, in the second chunk of the anchor table, is the first that can be valid
        half_curv[:, :, :16] = 40.0
    return raw, frames, half_curv, u_anchor, u_start


@pytest.mark.parametrize("shape,case", CASES, ids=str)
def test_kernel_against_the_rule(shape, case):
    B, M, P, K, n_min, cap = shape
    raw, frames, half_curv, u_anchor, u_start = _inputs(shape, case)
    recs = _run_and_compare(raw, frames, half_curv, u_anchor, u_start, n_min, cap, (shape, case), guarded=True)
    oks = [r["ok"] for r in recs]
    print(shape, case, "ok", oks, "cand", [r["cand"].tolist() for r in recs][:2], "counts", [r["counts"].tolist() for r in recs][:2])
    for b, r in enumerate(recs[:2]):
        fc.check_invariants(raw[b], frames[b], half_curv[b], u_anchor[b], u_start[b], n_min, cap, r)
    if K > 16 and case == "random":
        assert all((r["cand"] == 16).all() for r in recs)      # every step went through the second chunk
    if M in (333, 2048):
        from puzzlenet_amd import datapipe as dp
        uncapped = [dp.fracture_curved_rule(raw[b], frames[b], half_curv[b], u_anchor[b], u_start[b], P, n_min, M)["ok"] for b in range(B)]
        assert not all(uncapped)                               # a step without a valid candidate was compared
        assert not any(oks) and all(r["counts"].max() > cap for r in recs)
    if M in (4096, 65536):
        assert all(oks)


@pytest.mark.parametrize("shape,case", CASES, ids=str)
def test_pair_kernel_against_the_rule(shape, case):
    from puzzlenet_amd import datapipe as dp
    B, M, P, K, n_min, cap = shape
    raw, frames, half_curv, u_anchor, _ = _inputs(shape, case)
    u, _ = fc.pair_draws(B, 3000 + M)
    pieces = _spread(B, P)
    recs = _run_pair_and_compare(raw, frames, half_curv, u_anchor, u, pieces, n_min, 0.75, cap, (shape, case))
    print(shape, case, "pieces", pieces, "kinds", [r["kind"] for r in recs], "ok", [r["ok"] for r in recs])
    for b, r in enumerate(recs):
        assert not r["anchor"][pieces[b] - 1:].any() and not r["planes"][pieces[b] - 1:].any()
        if case == "random":                                   # the fracture under the pair: the curved rule's, cut short
            f = dp.fracture_curved_rule(raw[b], frames[b, :pieces[b] - 1], half_curv[b, :pieces[b] - 1], u_anchor[b, :pieces[b] - 1],
                                        np.zeros(pieces[b]), pieces[b], n_min, cap)
            assert np.array_equal(r["label"], f["label"]) and np.array_equal(r["anchor"][:pieces[b] - 1], f["anchor"])


def test_pair_kernel_reaches_both_kinds_and_refuses_a_count_out_of_range():
    """P_b = 5, 4, 3, 2 and the counts 1 and 6 in DEVICE memory: those two samples get kind -1, no piece, zero rows and ok = 0, and
    the samples beside them are cut as if alone."""
    from puzzlenet_amd import datapipe as dp, ops
    B, M, P, K, n_min = 6, 1000, 5, 4, 64
    raw = fc.clouds(B, M, 300)
    frames, half_curv, u_anchor, _, _ = fc.draws(B, P, K, 301)
    u, _ = fc.pair_draws(B, 302)
    u[:, 0] = [0.1, 0.9, 0.1, 0.1, 0.1, 0.1]
    good = [5, 4, 3, 2]
    recs = _run_pair_and_compare(raw[:4], frames[:4], half_curv[:4], u_anchor[:4], u[:4], good, n_min, 0.5, M, "four")
    kinds = [r["kind"] for r in recs]
    print("kinds", kinds, "pairs", [r["pair"].tolist() for r in recs])
    assert dp.SIBLING in kinds and dp.NEIGHBOUR in kinds and kinds[1] == dp.SIBLING and kinds[3] == dp.SIBLING
    pieces = np.array(good + [1, 6], dtype=np.int32)
    got = [t.cpu().numpy() for t in ops.fracture_pair_curved(_to(raw), _to(frames), _to(half_curv), _to(u_anchor), _to(pieces), _to(u),
                                                             n_min, 0.5, M)]
    torch.cuda.synchronize()
    _, want = fc.pair_batch_statement(raw[:4], frames[:4], half_curv[:4], u_anchor[:4], u[:4], good, n_min, 0.5, M)
    named = dict(zip(fc.PAIR_NAMES, got))
    for name, w in zip(fc.PAIR_NAMES, want):
        g = named[name].reshape(4, B, -1)[:, :4].reshape(w.shape) if name in ("pieces", "counts", "start") else named[name][:4]
        assert g.tobytes() == w.tobytes(), name
    for b in (4, 5):
        assert named["kind"][b] == -1 and not named["ok"][b] and named["pair"][b].tolist() == [-1] * 4
        assert (named["counts"][b::B] == -1).all() and not named["start"][b::B].any() and not named["label"][b].any()
        assert not named["planes"][b].any() and not named["target"][b].any() and not named["cand"][b].any()
        assert not named["anchor"][b].any()
        assert all(row.tobytes() == raw[b, 0].tobytes() for q in range(4) for row in named["pieces"][q * B + b])


def test_zero_curvature_on_a_lattice_is_the_plane_kernel():
    """Coordinates in multiples of 1/16 and signed coordinate axes as frames: both side tests are exact, so the curved kernel with
    half_curv = 0 cuts as the plane kernel does with the frames' normals - with many points exactly on a surface (f = 0, up)."""
    from puzzlenet_amd import ops
    B, M, P, K, n_min = 20, 600, 5, 4, 40
    raw = fc.lattice_clouds(B, M, 5)
    frames, normals = fc.axis_frames(B, P, K, 6)
    _, _, u_anchor, u_start, _ = fc.draws(B, P, K, 7)
    zero = np.zeros((B, P - 1, K, 2))
    recs = _run_and_compare(raw, frames, zero, u_anchor, u_start, n_min, M, "lattice")
    curved = ops.fracture_curved(_to(raw), _to(frames), _to(zero), _to(u_anchor), _to(u_start), n_min, M)
    plane = ops.fracture(_to(raw), _to(normals), _to(u_anchor), _to(u_start), n_min, M)
    torch.cuda.synchronize()
    for name, i, j in (("pieces", 0, 0), ("counts", 1, 1), ("label", 3, 3), ("order", 4, 4), ("target", 6, 6), ("cand", 7, 7), ("ok", 9, 8)):
        assert torch.equal(curved[i], plane[j]), name
    on = sum(int((fc.value(raw[b], raw[b, r["anchor"][0]], frames[b, 0, r["cand"][0]], np.zeros(2)) == 0).sum()) - 1
             for b, r in enumerate(recs))
    assert on > B                                              # points exactly on the first surface, the anchors apart


def test_kernel_duplicated_points():
    B, M, P, K = 2, 3000, 6, 4
    raw = fc.clouds(B, M, 77)
    raw[:, 1::2] = raw[:, 0::2]                                # every point twice, side by side
    raw[1, 1500:] = raw[1, :1500]                              # and the second sample's first half again, far apart
    frames, half_curv, u_anchor, u_start, _ = fc.draws(B, P, K, 78)
    recs = _run_and_compare(raw, frames, half_curv, u_anchor, u_start, 32, M, "duplicates")
    for r in recs:
        assert np.array_equal(r["label"][0::2], r["label"][1::2])      # coincident points stay together
    assert np.array_equal(recs[1]["label"][1500:], recs[1]["label"][:1500])


def test_kernel_point_repeated_as_its_own_anchor():
    """The anchor occurs many times in the cloud: every copy evaluates to exactly 0 and stays on the up side; a cloud that is one
    point throughout cannot be cut at all."""
    B, M, P, K = 2, 1024, 4, 3
    raw = fc.clouds(B, M, 91)
    raw[0, ::5] = raw[0, 0]
    raw[1, :] = raw[1, 0]
    frames, half_curv, u_anchor, u_start, _ = fc.draws(B, P, K, 92)
    u_anchor[0, 0, 0] = 0.0                                    # step 1, candidate 0: the surface through row 0
    recs = _run_and_compare(raw, frames, half_curv, u_anchor, u_start, 16, M, "anchor")
    assert (recs[0]["label"][::5] == recs[0]["label"][0]).all()
    assert not recs[1]["ok"] and recs[1]["counts"].tolist() == [M, 0, 0, 0]
    _run_and_compare(raw, frames, half_curv, u_anchor, u_start, 16, 300, "anchor, cap 300", guarded=True)


def test_limits_raise_before_any_launch(monkeypatch):
    from puzzlenet_amd import _lib, datapipe as dp, ops
    calls = []
    monkeypatch.setattr(ops, "_call", lambda *a, **k: calls.append(a[0]))
    B, M, K = 2, 64, 3
    dev = _dev()
    raw = _to(fc.clouds(B, M, 1))
    z = lambda *s: torch.zeros(s, dtype=torch.float64, device=dev)
    big = torch.zeros((1, 65537, 3), dtype=torch.float32, device=dev)
    for fn in (ops.fracture_curved_supported, ops.fracture_pair_curved_supported):
        assert fn(65536, 16, 1) and not fn(65537, 2, 1) and not fn(64, 1, 1) and not fn(64, 17, 1) and not fn(64, 2, 0)
    fr3, hc3, ua3, us3, u7, tw = z(B, 2, K, 3, 3), z(B, 2, K, 2), z(B, 2, K), z(B, 3), z(B, 7), z(B, 3, 6)
    for bad in (lambda: ops.fracture_curved(raw, z(B, 16, K, 3, 3), z(B, 16, K, 2), z(B, 16, K), z(B, 17), 4, M),       # P = 17
                lambda: ops.fracture_curved(raw, z(B, 0, K, 3, 3), z(B, 0, K, 2), z(B, 0, K), z(B, 1), 4, M),          # P = 1
                lambda: ops.fracture_curved(big, fr3[:1], hc3[:1], ua3[:1], us3[:1], 4, 32768),                        # M above the limit
                lambda: ops.fracture_pair_curved(raw, z(B, 16, K, 3, 3), z(B, 16, K, 2), z(B, 16, K), 2, u7, 4, 0.5, M),
                lambda: ops.fracture_pair_curved(big, fr3[:1], hc3[:1], ua3[:1], 2, u7[:1], 4, 0.5, 32768),
                lambda: dp.fracture(raw, None, ua3, us3, tw, n=16, cap=40000, frames=fr3, half_curv=hc3),                # beyond the FPS limit
                lambda: dp.cut_pairs_fracture(raw, None, ua3, 2, u7, tw[:, 0], n=16, cap=40000, frames=fr3, half_curv=hc3)):
        with pytest.raises(_lib.PznUnsupported):
            bad()
    for bad in (lambda: ops.fracture_curved(raw.cpu(), fr3, hc3, ua3, us3, 4, M),                                      # a CPU tensor
                lambda: ops.fracture_curved(raw, fr3.cpu(), hc3, ua3, us3, 4, M),
                lambda: ops.fracture_curved(raw.double(), fr3, hc3, ua3, us3, 4, M),                                   # wrong dtypes
                lambda: ops.fracture_curved(raw, fr3.float(), hc3, ua3, us3, 4, M),
                lambda: ops.fracture_curved(raw, fr3, hc3.float(), ua3, us3, 4, M),
                lambda: ops.fracture_curved(raw, fr3, hc3, ua3.float(), us3, 4, M),
                lambda: ops.fracture_curved(raw, fr3, hc3, ua3, us3.float(), 4, M),
                lambda: ops.fracture_curved(raw, fr3[:, :, :, :2], hc3, ua3, us3, 4, M),                               # frames of two rows
                lambda: ops.fracture_curved(raw, fr3, hc3[:, :, :2], ua3, us3, 4, M),                                  # K differs
                lambda: ops.fracture_curved(raw, fr3, hc3, ua3, z(B, 4), 4, M),                                        # P of u_start differs
                lambda: ops.fracture_curved(raw, fr3, hc3, ua3, us3, 4, 0),                                            # cap = 0
                lambda: ops.fracture_pair_curved(raw, fr3, hc3, ua3, 2, u7[:, :6], 4, 0.5, M),                         # six uniforms
                lambda: ops.fracture_pair_curved(raw, fr3, hc3, ua3, 2, u7, 4, 1.5, M),                                # neighbours
                lambda: ops.fracture_pair_curved(raw, fr3, hc3, ua3, 1, u7, 4, 0.5, M),                                # pieces outside 2 .. P
                lambda: ops.fracture_pair_curved(raw, fr3, hc3, ua3, [2, 4], u7, 4, 0.5, M),
                lambda: dp.fracture(raw, None, ua3, us3, tw, n=16, frames=fr3),                                          # half a surface
                lambda: dp.fracture(raw, z(B, 2, K, 3), ua3, us3, tw, n=16, frames=fr3, half_curv=hc3),                  # normals as well
                lambda: dp.fracture(raw, None, ua3, us3, tw[:, :2], n=16, frames=fr3, half_curv=hc3)):                   # a twist per piece
        with pytest.raises(_lib.PznError):
            bad()
    assert calls == []
    ops.fracture_curved(raw, fr3, hc3, ua3, us3, 4, M)
    ops.fracture_pair_curved(raw, fr3, hc3, ua3, [2, 3], u7, 4, 0.5, M)
    assert calls == ["pzn_fracture_curved_f32", "pzn_fracture_pair_curved_f32"]


def test_the_entry_points_refuse_the_shapes_themselves():
    from puzzlenet_amd import _lib, ops
    raw = _to(fc.clouds(2, 64, 1))
    p, s = raw.data_ptr(), ops._stream()
    lib = _lib.load()
    assert lib.pzn_fracture_curved_f32(p, p, p, p, p, 2, 64, 17, 3, 4, 64, p, p, p, p, p, p, p, p, p, p, s) == -3
    assert lib.pzn_fracture_curved_f32(p, p, p, p, p, 2, 65537, 3, 3, 4, 64, p, p, p, p, p, p, p, p, p, p, s) == -3
    assert lib.pzn_fracture_curved_f32(p, p, None, p, p, 2, 64, 3, 3, 4, 64, p, p, p, p, p, p, p, p, p, p, s) == -1
    assert lib.pzn_fracture_pair_curved_f32(p, p, p, p, p, p, 0.5, 2, 64, 17, 3, 4, 64, p, p, p, p, p, p, p, p, p, p, p, s) == -3
    assert lib.pzn_fracture_pair_curved_f32(p, p, p, p, p, p, 1.5, 2, 64, 3, 3, 4, 64, p, p, p, p, p, p, p, p, p, p, p, s) == -1
    torch.cuda.synchronize()


# --------------------------------------------------------------------------- the host forms

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


def _against_the_statement(got, rec, recs, twist, n, k):
    """The 8-tuple and the record of cut_pairs_fracture with surfaces against the statement's records and the ops of the tail"""
    B = len(recs)
    assert type(rec).__name__ == "CurvedFracturePair"
    assert rec.kind.cpu().tolist() == [r["kind"] for r in recs] and rec.pair.cpu().tolist() == [r["pair"].tolist() for r in recs]
    for name in ("label", "planes", "target", "cand", "anchor"):
        assert getattr(rec, name).cpu().numpy().tobytes() == np.stack([r[name] for r in recs]).tobytes(), name
    rejected = rec.rejected.cpu().numpy()
    assert not (rejected & (rec.kind.cpu().numpy() != 1)).any()
    primary = _stated_pairs(recs, [False] * B, twist, n, k)
    assert torch.equal(rec.U, primary[3]) and torch.equal(rec.D, primary[0])
    assert torch.equal(rec.Ub, primary[5]) and torch.equal(rec.Db, primary[4])
    cd = np.array([dc.chamfer_cd(rec.Db[b].cpu().numpy(), rec.Ub[b].cpu().numpy()) for b in range(B)])
    assert np.abs(rec.cd.cpu().numpy() - cd).max() <= 5.4e-7          # CD_MARGIN of tests/test_gpu_fracture_pair.py, derived there
    has_fallback = [r["kind"] == 1 for r in recs]
    # (rows without a fallback keep the primary here; they are never compared as a fallback)
    fallback = _stated_pairs([dict(pieces=r["pieces"] if f else r["pieces"][:2] * 2, start=r["start"] if f else list(r["start"][:2]) * 2)
                              for r, f in zip(recs, has_fallback)], [True] * B, twist, n, k)
    for b in range(B):
        want = fallback if rejected[b] else primary
        for name, g, w in zip("down moved igt up downb upb down_mask up_mask".split(), got, want):
            assert torch.equal(g[b], w[b]), (b, name, bool(rejected[b]))
    return rejected


def test_cut_pairs_fracture_with_surfaces_against_the_ops_it_is_made_of():
    from puzzlenet_amd import datapipe as dp
    B, M, P, K, n, k = 4, 4096, 5, 8, 256, 32
    raw = fc.clouds(B, M, 520)
    frames, half_curv, u_anchor, _, _ = fc.draws(B, P, K, 521)
    u, twist = fc.pair_draws(B, 522)
    u[:, 0] = [0.1, 0.1, 0.9, 0.1]
    pieces = [5, 4, 5, 3]
    recs, _ = fc.pair_batch_statement(raw, frames, half_curv, u_anchor, u, pieces, n, 0.5, M)
    assert all(r["ok"] for r in recs) and {r["kind"] for r in recs} == {dp.SIBLING, dp.NEIGHBOUR}
    got, ok, rec = dp.cut_pairs_fracture(_to(raw), None, _to(u_anchor), pieces, _to(u), _to(twist), n=n, k=k, neighbours=0.5,
                                         frames=_to(frames), half_curv=_to(half_curv))
    torch.cuda.synchronize()
    assert bool(ok.all())
    rejected = _against_the_statement(got, rec, recs, twist, n, k)
    print("kinds", rec.kind.cpu().tolist(), "rejected", rejected.tolist(), "cd", rec.cd.cpu().tolist())


def _sample(B, M, P, K, n, k, seed):
    from puzzlenet_amd import datapipe
    raw = fc.clouds(B, M, seed)
    frames, half_curv, u_anchor, u_start, twist = fc.draws(B, P, K, seed + 1)
    f = datapipe.fracture(_to(raw), None, _to(u_anchor), _to(u_start), _to(twist), n=n, k=k, frames=_to(frames), half_curv=_to(half_curv))
    torch.cuda.synchronize()
    recs, _ = fc.batch_statement(raw, frames, half_curv, u_anchor, u_start, n, M)
    return raw, (frames, half_curv), recs, f


def test_fracture_sample_with_surfaces():
    from oracle import point_ops as orc
    from puzzlenet_amd import datapipe
    B, M, P, K, n, k = 2, 4096, 4, 8, 256, 32
    raw, (frames, half_curv), recs, f = _sample(B, M, P, K, n, k, 40)
    assert type(f).__name__ == "CurvedFracture" and f._fields[:len(datapipe.Fracture._fields)] == datapipe.Fracture._fields
    assert all(r["ok"] for r in recs) and bool(f.ok.all())
    assert f.rest.shape == (B, P, n, 3) and f.src.shape == (B, P, n) and f.anchor.shape == (B, P - 1) and f.anchor.dtype == torch.int32
    assert f.frames.cpu().numpy().tobytes() == frames.tobytes() and f.half_curv.cpu().numpy().tobytes() == half_curv.tobytes()
    rest, src, label = f.rest.cpu().numpy(), f.src.cpu().numpy(), f.label.cpu().numpy()
    for b, r in enumerate(recs):
        for name in ("label", "planes", "target", "cand", "anchor", "counts"):
            assert getattr(f, name)[b].cpu().numpy().tobytes() == r[name].tobytes(), (b, name)
        for p in range(P):
            idx = orc.farthest_point_sample(r["pieces"][p][None], n, r["start"][p:p + 1])[0]      # the numpy FPS, from start
            assert rest[b, p].tobytes() == r["pieces"][p][idx].tobytes(), (b, p)
            assert raw[b][src[b, p]].tobytes() == rest[b, p].tobytes(), (b, p)                   # src: the cloud's own rows
            assert (label[b][src[b, p]] == p).all()
    cd, mates = f.cd.cpu().numpy(), f.mates.cpu().numpy()
    assert np.array_equal(mates, (cd <= np.float32(datapipe.CD_ACCEPT)) & ~np.eye(P, dtype=bool))
    sym = cd == cd.transpose(0, 2, 1)
    assert np.array_equal(mates[sym], mates.transpose(0, 2, 1)[sym])          # symmetric where cd is
    print("cd symmetric in", int(sym.sum()), "of", sym.size, "mates per sample", mates.sum((1, 2)).tolist())
    assert mates.any()


def test_two_sides_of_one_curved_cut_of_a_cube_are_mates():
    _, _, recs, f = _sample(1, 4096, 2, 8, 1024, 128, 40)
    assert recs[0]["ok"] and bool(f.ok[0])
    print("cd", f.cd[0].tolist())
    assert bool(f.mates[0, 0, 1]) and bool(f.mates[0, 1, 0]) and not bool(f.mates[0, 0, 0])


# --------------------------------------------------------------------------- the feeder

def test_curved_feeder_against_a_restatement_from_the_seed():
    """Two batches of PairFeeder(pieces=(2, 5), curvature=2.0): the draws restated from the seed, the rule per sample, the pieces
    sampled from the stated start indices and the pair tail - tensor by tensor."""
    from puzzlenet_amd import datapipe as dp
    dev = _dev()
    B, M, N, K, seed, lo, hi, curvature = 4, 6000, 512, 8, 11, 2, 5, 2.0
    raw = dc.shells(B, M, 21)
    f = dp.PairFeeder(raw, dev, n=N, k=64, candidates=K, seed=seed, pieces=(lo, hi), curvature=curvature)
    cols = dp._fracture_pair_curved_cols(hi, K)
    assert f._width == cols[-1].stop == 12 * K * (hi - 1) + 1 + 7 + 6 and f.curvature == curvature
    rng, gen = np.random.RandomState(seed), torch.Generator().manual_seed(seed)
    kinds = set()
    for _ in range(2):
        batch = f.next_batch()
        batch.ready.synchronize()
        st = np.empty((B, cols[-1].stop))
        dp.draw_fracture_pair_curved_batch(rng, gen, B, lo, hi, K, 0.8, curvature, st)
        frames, half_curv, u_anchor, pc, u, tw = (st[:, c] for c in cols)
        frames, half_curv, u_anchor = frames.reshape(B, hi - 1, K, 3, 3), half_curv.reshape(B, hi - 1, K, 2), u_anchor.reshape(B, hi - 1, K)
        pieces = pc.reshape(B).astype(np.int32)
        recs, _ = fc.pair_batch_statement(raw, frames, half_curv, u_anchor, np.ascontiguousarray(u), pieces, N, 0.5, M)
        want_ok = [bool(r["ok"] and min(r["counts"][:2]) >= N) for r in recs]
        assert batch.ok.cpu().tolist() == want_ok and all(want_ok)
        assert batch.plane is None and batch.cut is None and batch.double is None
        _against_the_statement(list(batch), batch.fracture, recs, np.ascontiguousarray(tw), N, 64)
        kinds.update(r["kind"] for r in recs)
    f.close()
    assert kinds == {dp.SIBLING, dp.NEIGHBOUR}


def test_curvature_zero_is_the_plane_feeder():
    """PairFeeder(pieces=...) and PairFeeder(pieces=..., curvature=0.0): the same mode, the same draws, the same bits."""
    from puzzlenet_amd import datapipe as dp
    dev = _dev()
    raw = dc.shells(4, 6000, 3)
    f = dp.PairFeeder(raw, dev, n=512, k=64, candidates=8, seed=7, pieces=(2, 5))
    g = dp.PairFeeder(raw, dev, n=512, k=64, candidates=8, seed=7, pieces=(2, 5), curvature=0.0)
    assert f._width == g._width == dp._fracture_pair_cols(5, 8)[-1].stop and g.curvature == 0.0 == f.curvature
    assert f._mode.build is g._mode.build is dp._build_fracture_pair
    for _ in range(3):
        x, y = f.next_batch(), g.next_batch()
        x.ready.synchronize()      # the tensors are produced on each feeder's own stream: wait for them before
        y.ready.synchronize()      # reading them on this one
        assert all(torch.equal(s, t) for s, t in zip(x, y)) and torch.equal(x.ok, y.ok)
        assert type(x.fracture) is type(y.fracture) is dp.FracturePair
        assert all(torch.equal(s, t) for s, t in zip(x.fracture, y.fracture))
    f.close()
    g.close()
