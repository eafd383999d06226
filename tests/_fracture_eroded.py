"""Shared by the eroded-fracture tests (CPU and GPU): seeded draws for both forms (planes, surfaces), datapipe.fracture_eroded_rule /
fracture_pair_eroded_rule applied to a batch and laid out as the entry points lay their outputs out, and the rule's invariants
checked on one sample by replay.  A form is (normals, frames, half_curv) with the unused part None, as the rules take it."""
import numpy as np

from tests import _double_cut as dc
from tests import _fracture_curved as fc

LOST = 255
NAMES = ("pieces", "counts", "start", "label", "order", "planes", "target", "cand", "anchor", "lost", "ok")
PAIR_NAMES = ("pieces", "counts", "start", "kind", "pair", "label", "planes", "target", "cand", "anchor", "lost", "ok")

# (B, M, P, K, n_min, cap): tests/test_gpu_fracture_curved.py's
SHAPES = [
    (3, 257, 2, 1, 8, 257),                 # one cut, one candidate, M below the thread count
    (2, 1000, 5, 17, 64, 1000),             # K > 16: the second chunk of the anchor table
    (2, 1025, 16, 4, 16, 400),              # runs of 2 points, the largest P, a cap below the first pieces
    (2, 4096, 8, 8, 128, 4096),
    (1, 65536, 16, 16, 1024, 32768),        # the M limit: runs of 64 points, more than 64 KiB of LDS
    (2, 333, 16, 2, 4, 30),                 # steps without a valid candidate, a cap below the largest piece
    (4, 2048, 5, 1, 64, 500),               # K = 1: the most-balanced path, a cap below the largest piece
]
SALT = {333: 1}


def widths(B, P, seed):
    """erode [B,P-1,4] = (U[0,.03), U[0,.03), .03 + U[0,.05), U[0,.2)): bands of up to 3 % of the cube's edge on either side and
    a chip deeper than either band"""
    rng = np.random.RandomState(seed)
    u = rng.rand(B, P - 1, 4)
    return u * np.array([0.03, 0.03, 0.05, 0.2]) + np.array([0.0, 0.0, 0.03, 0.0])


def inputs(shape, curved):
    """The curved suite's clouds and draws for a shape -> raw, form, u_anchor, u_start, erode; the plane form cuts along the
    tangent planes of the curved one (normals = the frames' third rows)"""
    B, M, P, K, n_min, cap = shape
    salt = M + P + SALT.get(M, 0)
    raw = fc.clouds(B, M, 1000 + salt)
    frames, half_curv, u_anchor, u_start, _ = fc.draws(B, P, K, 2000 + salt)
    form = (None, frames, half_curv) if curved else (np.ascontiguousarray(frames[:, :, :, 2]), None, None)
    return raw, form, u_anchor, u_start, widths(B, P, 3000 + salt)


def of_sample(form, b):
    return tuple(None if t is None else t[b] for t in form)


def batch_statement(raw, form, u_anchor, u_start, erode, n_min, cap):
    """fracture_eroded_rule per sample -> (list of its dicts, pzn_fracture_eroded_f32's outputs as numpy arrays, in NAMES' order)"""
    from puzzlenet_amd import datapipe
    B, P = raw.shape[0], u_start.shape[1]
    recs = []
    for b in range(B):
        normals, frames, half_curv = of_sample(form, b)
        recs.append(datapipe.fracture_eroded_rule(raw[b], normals, u_anchor[b], u_start[b], erode[b], P, n_min, cap, frames=frames,
                                                  half_curv=half_curv))
    pieces = np.empty((P * B, cap, 3), dtype=np.float32)
    counts, start = np.empty(P * B, dtype=np.int64), np.empty(P * B, dtype=np.int64)
    for b, r in enumerate(recs):
        for p in range(P):
            pieces[p * B + b] = r["pieces"][p]
            counts[p * B + b], start[p * B + b] = r["counts"][p], r["start"][p]
    stack = lambda key: np.stack([r[key] for r in recs])
    return recs, (pieces, counts, start, stack("label"), stack("order"), stack("planes"), stack("target"), stack("cand"),
                  stack("anchor"), stack("lost"), np.array([r["ok"] for r in recs], dtype=bool))


def pair_batch_statement(raw, form, u_anchor, u, erode, pieces, n_min, neighbours, cap):
    """fracture_pair_eroded_rule per sample -> (list of its dicts, pzn_fracture_pair_eroded_f32's outputs, in PAIR_NAMES' order)"""
    from puzzlenet_amd import datapipe
    B, P = raw.shape[0], u_anchor.shape[1] + 1
    recs = []
    for b in range(B):
        normals, frames, half_curv = of_sample(form, b)
        recs.append(datapipe.fracture_pair_eroded_rule(raw[b], normals, u_anchor[b], u[b], erode[b], int(pieces[b]), P, n_min,
                                                       neighbours, cap, frames=frames, half_curv=half_curv))
    out = np.empty((4 * B, cap, 3), dtype=np.float32)
    counts, start = np.empty(4 * B, dtype=np.int64), np.empty(4 * B, dtype=np.int64)
    for b, r in enumerate(recs):
        for q in range(4):
            out[q * B + b] = dc.padded(None, raw[b, 0], cap) if r["pieces"][q] is None else r["pieces"][q]
            counts[q * B + b], start[q * B + b] = r["counts"][q], r["start"][q]
    stack = lambda key: np.stack([r[key] for r in recs])
    return recs, (out, counts, start, np.array([r["kind"] for r in recs], dtype=np.int32), stack("pair"), stack("label"),
                  stack("planes"), stack("target"), stack("cand"), stack("anchor"), stack("lost"),
                  np.array([r["ok"] for r in recs], dtype=bool))


def value(pts, a, form, s, k):
    """f of the issue's statement for candidate k of step s + 1 through the point a, written out once more: float64, every
    operation rounded on its own -> (f [m], the plane recorded: (n, -((ax n0 + ay n1) + az n2)))"""
    normals, frames, half_curv = form
    p = pts.astype(np.float64)
    a = a.astype(np.float64)
    n = normals[s, k] if frames is None else frames[s, k, 2]
    plane = np.array([n[0], n[1], n[2], -((a[0] * n[0] + a[1] * n[1]) + a[2] * n[2])])
    if frames is None:
        return ((p[:, 0] * plane[0] + p[:, 1] * plane[1]) + p[:, 2] * plane[2]) + plane[3], plane
    frame, hc = frames[s, k], half_curv[s, k]
    d0, d1, d2 = p[:, 0] - a[0], p[:, 1] - a[1], p[:, 2] - a[2]
    s1 = (d0 * frame[0, 0] + d1 * frame[0, 1]) + d2 * frame[0, 2]
    s2 = (d0 * frame[1, 0] + d1 * frame[1, 1]) + d2 * frame[1, 2]
    h = (d0 * frame[2, 0] + d1 * frame[2, 1]) + d2 * frame[2, 2]
    return (h + (hc[0] * s1) * s1) + (hc[1] * s2) * s2, plane


def lost_under(pts, a, f, row):
    """The band or the chip of erode row (w_up, w_dn, depth, rho) holds: all comparisons strict -> bool [m]"""
    w_up, w_dn, depth, rho = row
    d = pts.astype(np.float64) - a.astype(np.float64)
    r2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    return ((f > -w_dn) & (f < w_up)) | ((f > -depth) & (f < depth) & (r2 < rho * rho))


def check_invariants(raw, form, u_anchor, u_start, erode, n_min, cap, r):
    """Everything fracture_eroded_rule promises about one sample's result r, from the inputs alone: the steps are replayed from r's
    own target / cand / anchor, never from the rule's code."""
    M, P, K = raw.shape[0], u_start.shape[0], u_anchor.shape[1]
    label, counts, order, lost = r["label"], r["counts"], r["order"], r["lost"]
    assert label.dtype == np.uint8 and label.shape == (M,) and ((label < P) | (label == LOST)).all()
    assert np.array_equal(counts, np.bincount(label[label < P], minlength=P))
    assert lost.dtype == np.int32 and lost.shape == (P - 1,) and lost.sum() == (label == LOST).sum()
    assert counts.sum() + lost.sum() == M
    assert order.dtype == np.int32 and np.array_equal(order, np.argsort(label, kind="stable"))
    assert (label[order[counts.sum():]] == LOST).all() and (np.diff(order[counts.sum():]) > 0).all()    # behind the last piece
    assert r["anchor"].dtype == np.int32 and r["anchor"].shape == (P - 1,)
    for p in range(P):
        rows = raw[label == p]
        piece = r["pieces"][p]
        assert piece.shape == (cap, 3) and piece.dtype == np.float32
        kept = min(len(rows), cap)
        assert piece[:kept].tobytes() == rows[:kept].tobytes()
        fill = rows[0] if len(rows) else raw[0]
        assert all(row.tobytes() == fill.tobytes() for row in piece[kept:])
        assert r["start"][p] == max(0, min(int(counts[p]) - 1, int(np.floor(u_start[p] * counts[p]))))
    lab = np.zeros(M, dtype=np.int64)
    all_valid = True
    for s in range(1, P):
        cnt = np.bincount(lab[lab < P], minlength=P)
        t = int(r["target"][s - 1])
        assert t < s and cnt[t] == cnt[:s].max() and (cnt[:t] < cnt[t]).all()                   # the first largest label
        members = np.flatnonzero(lab == t)
        if len(members) == 0:                                                                   # everything is lost: not made
            all_valid = False
            assert not r["planes"][s - 1].any() and r["cand"][s - 1] == 0 and r["anchor"][s - 1] == 0 and lost[s - 1] == 0
            continue
        row = erode[s - 1]
        rows = [members[max(0, min(len(members) - 1, int(np.floor(u_anchor[s - 1, k] * len(members)))))] for k in range(K)]
        kept = []
        for k in range(K):
            f, _ = value(raw[members], raw[rows[k]], form, s - 1, k)
            gone = lost_under(raw[members], raw[rows[k]], f, row)
            kept.append((int(((f >= 0) & ~gone).sum()), int(((f < 0) & ~gone).sum())))
        valid = [k for k in range(K) if min(kept[k]) >= n_min]                                  # BOTH sides, after the loss
        k = int(r["cand"][s - 1])
        if valid:
            assert k == valid[0]                                                                # the first valid candidate
        else:
            all_valid = False
            assert k == int(np.argmax([min(c) for c in kept]))                                  # the first most balanced one
        a = int(r["anchor"][s - 1])
        assert a == rows[k] and lab[a] == t                                                     # the anchor: a point of the target
        f, plane = value(raw[members], raw[a], form, s - 1, k)
        assert value(raw[a:a + 1], raw[a], form, s - 1, k)[0][0] == 0.0                         # exactly on the surface
        assert r["planes"][s - 1].tobytes() == plane.tobytes()
        gone = lost_under(raw[members], raw[a], f, row)
        assert lost[s - 1] == gone.sum()
        lab[members[f < 0]] = s
        lab[members[gone]] = LOST
        # what this step lost has label 255 in the result, and no kept member of its target meets either condition
        assert (label[members[gone]] == LOST).all()
        up, dn = members[(f >= 0) & ~gone], members[(f < 0) & ~gone]
        f_up, f_dn = f[(f >= 0) & ~gone], f[(f < 0) & ~gone]
        assert not lost_under(raw[up], raw[a], f_up, row).any() and not lost_under(raw[dn], raw[a], f_dn, row).any()
        # the kept sides stand off the surface by the band's rims where the band is live for them (f >= 0 > -w_dn needs
        # w_dn > 0, f < 0 <= w_up needs w_up >= 0; a NaN rim makes no comparison hold): else f >= 0 and f < 0
        assert (f_up >= (row[0] if row[0] > 0 and row[1] > 0 else 0.0)).all()
        assert (f_dn <= -row[1]).all() if row[1] > 0 and row[0] >= 0 else (f_dn < 0).all()
        if row[0] > 0 and row[1] > 0:
            assert lab[a] == LOST                                                               # the anchor itself is lost
        assert (lab == s).sum() == len(dn) and (lab == t).sum() == len(up)
    assert np.array_equal(lab, label.astype(np.int64))                 # every lost point: lost by exactly the step of the replay
    assert r["ok"] == (all_valid and counts.max() <= cap)


def lattice_case():
    """Lattice clouds, axis frames, widths in multiples of 1/16: f is exact, and points lie exactly on both rims of the band
    -> raw, (plane form, curved form), u_anchor, u_start, erode, n_min"""
    B, M, P, K = 8, 600, 2, 4
    raw = fc.lattice_clouds(B, M, 5)
    frames, normals = fc.axis_frames(B, P, K, 6)
    _, _, u_anchor, u_start, _ = fc.draws(B, P, K, 7)
    erode = np.tile(np.array([2.0 / 16, 1.0 / 16, 0.0, 0.0]), (B, P - 1, 1))
    return raw, ((normals, None, None), (None, frames, np.zeros((B, P - 1, K, 2)))), u_anchor, u_start, erode, 40


def check_lattice_rims(raw, form, erode, recs):
    """Points at f == w_up and at f == -w_dn exist and are KEPT (up and down); the points with -w_dn < f < w_up are lost"""
    on_up = on_dn = 0
    for b, r in enumerate(recs):
        a = int(r["anchor"][0])
        f, _ = value(raw[b], raw[b, a], of_sample(form, b), 0, int(r["cand"][0]))
        w_up, w_dn = erode[b, 0, 0], erode[b, 0, 1]
        assert (r["label"][f == w_up] == 0).all() and (r["label"][f == -w_dn] == 1).all()
        assert (r["label"][(f > -w_dn) & (f < w_up)] == LOST).all() and r["label"][a] == LOST
        assert r["lost"][0] == ((f > -w_dn) & (f < w_up)).sum()
        on_up, on_dn = on_up + int((f == w_up).sum()), on_dn + int((f == -w_dn).sum())
    assert on_up > len(recs) and on_dn > len(recs)
    return on_up, on_dn
