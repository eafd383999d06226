"""Shared by the curved-fracture tests (CPU and GPU): seeded draws, clouds on a lattice with signed coordinate axes as frames (where
the side test is exact), datapipe.fracture_curved_rule / fracture_pair_curved_rule applied to a batch and laid out as the entry
points lay their outputs out, and the rule's invariants checked on one sample by replay."""
import numpy as np
import torch

from tests import _double_cut as dc
from tests import _fracture as fr

clouds = fr.clouds
NAMES = ("pieces", "counts", "start", "label", "order", "planes", "target", "cand", "anchor", "ok")
PAIR_NAMES = ("pieces", "counts", "start", "kind", "pair", "label", "planes", "target", "cand", "anchor", "ok")


def draws(B, P, K, seed, curvature=2.0, mag=0.8):
    """-> frames [B,P-1,K,3,3], half_curv [B,P-1,K,2], u_anchor [B,P-1,K], u_start [B,P], twist [B,P,6] (float64), as
    draw_fracture_curved_batch draws them"""
    from puzzlenet_amd import datapipe
    return datapipe.fracture_curved_draws(np.random.RandomState(seed), torch.Generator().manual_seed(seed), B, P, K, mag, curvature)


def pair_draws(B, seed, mag=0.8):
    """-> u [B,7] float64 uniforms, twist [B,6] float32 of length mag: tests/_fracture_pair.draws' own part"""
    rng = np.random.RandomState(seed + 7919)
    u = rng.rand(B, 7)
    x = rng.randn(B, 6)
    return u, (x / np.linalg.norm(x, axis=1, keepdims=True) * mag).astype(np.float32)


def shaped(half_curv, case, seed=0):
    """The curvature cases: half_curv as drawn ("random"), every candidate a cylinder (kappa2 = 0), a saddle (kappa1 = -kappa2),
    kappa = +-8 with drawn signs, and kappa = 0"""
    h = half_curv.copy()
    if case == "cylinder":
        h[..., 1] = 0.0
    elif case == "saddle":
        h[..., 1] = -h[..., 0]
    elif case == "eight":
        h = np.where(np.random.RandomState(seed).rand(*h.shape) < 0.5, -4.0, 4.0)
    elif case == "zero":
        h[:] = 0.0
    else:
        assert case == "random"
    return h


def lattice_clouds(B, M, seed):
    """Coordinates in multiples of 1/16 in [-0.5, 0.5): products with a signed coordinate axis and their sums are exact, and many
    points lie exactly on a plane through one of them."""
    rng = np.random.RandomState(seed)
    return ((rng.randint(0, 16, size=(B, M, 3)) - 8) / 16.0).astype(np.float32)


def axis_frames(B, P, K, seed):
    """Frames whose rows are signed coordinate axes, right-handed (e2 = n x e1).  -> frames [B,P-1,K,3,3], normals [B,P-1,K,3]"""
    rng = np.random.RandomState(seed)
    R = B * (P - 1) * K
    ni, step = rng.randint(0, 3, R), rng.randint(1, 3, R)
    n = np.eye(3)[ni] * rng.choice([-1.0, 1.0], R)[:, None]
    e1 = np.eye(3)[(ni + step) % 3] * rng.choice([-1.0, 1.0], R)[:, None]
    frames = np.stack([e1, np.cross(n, e1), n], axis=1).reshape(B, P - 1, K, 3, 3)
    return frames, np.ascontiguousarray(frames[:, :, :, 2])


def batch_statement(raw, frames, half_curv, u_anchor, u_start, n_min, cap):
    """fracture_curved_rule per sample -> (list of its dicts, pzn_fracture_curved_f32's outputs as numpy arrays, in NAMES' order)"""
    from puzzlenet_amd import datapipe
    B, P = raw.shape[0], u_start.shape[1]
    recs = [datapipe.fracture_curved_rule(raw[b], frames[b], half_curv[b], u_anchor[b], u_start[b], P, n_min, cap) for b in range(B)]
    pieces = np.empty((P * B, cap, 3), dtype=np.float32)
    counts, start = np.empty(P * B, dtype=np.int64), np.empty(P * B, dtype=np.int64)
    for b, r in enumerate(recs):
        for p in range(P):
            pieces[p * B + b] = r["pieces"][p]
            counts[p * B + b], start[p * B + b] = r["counts"][p], r["start"][p]
    stack = lambda key: np.stack([r[key] for r in recs])
    return recs, (pieces, counts, start, stack("label"), stack("order"), stack("planes"), stack("target"), stack("cand"),
                  stack("anchor"), np.array([r["ok"] for r in recs], dtype=bool))


def pair_batch_statement(raw, frames, half_curv, u_anchor, u, pieces, n_min, neighbours, cap):
    """fracture_pair_curved_rule per sample -> (list of its dicts, pzn_fracture_pair_curved_f32's outputs, in PAIR_NAMES' order)"""
    from puzzlenet_amd import datapipe
    B, P = raw.shape[0], frames.shape[1] + 1
    recs = [datapipe.fracture_pair_curved_rule(raw[b], frames[b], half_curv[b], u_anchor[b], u[b], int(pieces[b]), P, n_min,
                                               neighbours, cap) for b in range(B)]
    out = np.empty((4 * B, cap, 3), dtype=np.float32)
    counts, start = np.empty(4 * B, dtype=np.int64), np.empty(4 * B, dtype=np.int64)
    for b, r in enumerate(recs):
        for q in range(4):
            out[q * B + b] = dc.padded(None, raw[b, 0], cap) if r["pieces"][q] is None else r["pieces"][q]
            counts[q * B + b], start[q * B + b] = r["counts"][q], r["start"][q]
    stack = lambda key: np.stack([r[key] for r in recs])
    return recs, (out, counts, start, np.array([r["kind"] for r in recs], dtype=np.int32), stack("pair"), stack("label"),
                  stack("planes"), stack("target"), stack("cand"), stack("anchor"), np.array([r["ok"] for r in recs], dtype=bool))


def value(pts, a, frame, hc):
    """f of the issue's statement, written out once more: float64, every operation rounded on its own -> [m]"""
    p = pts.astype(np.float64)
    a = a.astype(np.float64)
    d0, d1, d2 = p[:, 0] - a[0], p[:, 1] - a[1], p[:, 2] - a[2]
    s1 = (d0 * frame[0, 0] + d1 * frame[0, 1]) + d2 * frame[0, 2]
    s2 = (d0 * frame[1, 0] + d1 * frame[1, 1]) + d2 * frame[1, 2]
    h = (d0 * frame[2, 0] + d1 * frame[2, 1]) + d2 * frame[2, 2]
    return (h + (hc[0] * s1) * s1) + (hc[1] * s2) * s2


def check_invariants(raw, frames, half_curv, u_anchor, u_start, n_min, cap, r):
    """Everything fracture_curved_rule promises about one sample's result r, from the inputs alone: the steps are replayed from
    r's own target / cand / anchor, never from the rule's code."""
    M, P, K = raw.shape[0], u_start.shape[0], frames.shape[1]
    label, counts, order = r["label"], r["counts"], r["order"]
    assert label.dtype == np.uint8 and label.shape == (M,) and label.max() < P                  # the labels partition the cloud
    assert np.array_equal(counts, np.bincount(label, minlength=P)) and counts.sum() == M
    assert order.dtype == np.int32 and np.array_equal(order, np.argsort(label, kind="stable"))
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
        cnt = np.bincount(lab, minlength=P)
        t = int(r["target"][s - 1])
        assert t < s and cnt[t] == cnt[:s].max() and (cnt[:t] < cnt[t]).all()                   # the first largest label
        members = np.flatnonzero(lab == t)
        rows = [members[max(0, min(len(members) - 1, int(np.floor(u_anchor[s - 1, k] * len(members)))))] for k in range(K)]
        ups = [int((value(raw[members], raw[rows[k]], frames[s - 1, k], half_curv[s - 1, k]) >= 0).sum()) for k in range(K)]
        valid = [k for k in range(K) if ups[k] >= n_min and len(members) - ups[k] >= n_min]
        bal = [min(u, len(members) - u) for u in ups]
        k = int(r["cand"][s - 1])
        if valid:
            assert k == valid[0]                                                                # the first valid candidate
        else:
            all_valid = False
            assert k == int(np.argmax(bal))                                                     # the first most balanced one
        a = int(r["anchor"][s - 1])
        assert a == rows[k] and lab[a] == t                                                     # the anchor: a point of the target
        f = value(raw[members], raw[a], frames[s - 1, k], half_curv[s - 1, k])
        at = value(raw[a:a + 1], raw[a], frames[s - 1, k], half_curv[s - 1, k])[0]
        assert at == 0.0 and at >= 0                                                            # exactly 0 (of either sign): up
        n, pa = frames[s - 1, k, 2], raw[a].astype(np.float64)
        tangent = np.array([n[0], n[1], n[2], -((pa[0] * n[0] + pa[1] * n[1]) + pa[2] * n[2])])
        assert r["planes"][s - 1].tobytes() == tangent.tobytes()                                # the tangent plane's bits
        lab[members[f < 0]] = s
        assert lab[a] == t and (lab == s).sum() + (lab == t).sum() == len(members)
        assert (value(raw[label == s], raw[a], frames[s - 1, k], half_curv[s - 1, k]) < 0).all()      # label s: the down side
    assert np.array_equal(lab, label)
    assert r["ok"] == (all_valid and counts.max() <= cap)
