"""Shared by the fracture tests (CPU and GPU): seeded clouds and draws, datapipe.fracture_rule applied to a batch and laid out as
pzn_fracture_f32 lays its outputs out, and the rule's invariants checked on one sample."""
import numpy as np
import torch

# (M, P, K, n_min): the shapes the rule was tried on; the last two leave some samples without a valid cut
OK_SHAPES = [(1000, 3, 4, 64), (1025, 4, 4, 64), (4096, 8, 8, 128), (10000, 8, 16, 256), (10000, 4, 16, 1024),
             (32768, 8, 16, 1024), (65536, 16, 16, 1024)]
NOT_OK_SHAPES = [(333, 16, 2, 4), (2048, 5, 1, 64)]


def clouds(B, M, seed):
    """Uniform in [-0.5, 0.5)^3, float32."""
    rng = np.random.RandomState(seed)
    return (rng.rand(B, M, 3) - 0.5).astype(np.float32)


def draws(B, P, K, seed, mag=0.8):
    """-> normals [B,P-1,K,3], u_anchor [B,P-1,K], u_start [B,P], twist [B,P,6] (float64), as draw_fracture_batch draws them"""
    from puzzlenet_amd import datapipe
    return datapipe.fracture_draws(np.random.RandomState(seed), torch.Generator().manual_seed(seed), B, P, K, mag)


def batch_statement(raw, normals, u_anchor, u_start, n_min, cap):
    """fracture_rule per sample -> (list of its dicts, the kernel's outputs as numpy arrays: pieces [P B,cap,3], counts [P B],
    start [P B], label [B,M], order [B,M], planes [B,P-1,4], target [B,P-1], cand [B,P-1], ok [B])"""
    from puzzlenet_amd import datapipe
    B, P = raw.shape[0], u_start.shape[1]
    recs = [datapipe.fracture_rule(raw[b], normals[b], u_anchor[b], u_start[b], P, n_min, cap) for b in range(B)]
    pieces = np.empty((P * B, cap, 3), dtype=np.float32)
    counts, start = np.empty(P * B, dtype=np.int64), np.empty(P * B, dtype=np.int64)
    for b, r in enumerate(recs):
        for p in range(P):
            pieces[p * B + b] = r["pieces"][p]
            counts[p * B + b], start[p * B + b] = r["counts"][p], r["start"][p]
    stack = lambda key: np.stack([r[key] for r in recs])
    return recs, (pieces, counts, start, stack("label"), stack("order"), stack("planes"), stack("target"), stack("cand"),
                  np.array([r["ok"] for r in recs], dtype=bool))


def side(pts, plane):
    """((x n0 + y n1) + z n2) + offset in float64, every operation rounded on its own -> the signed values [M]"""
    p = pts.astype(np.float64)
    return ((p[:, 0] * plane[0] + p[:, 1] * plane[1]) + p[:, 2] * plane[2]) + plane[3]


def check_invariants(raw, normals, u_anchor, u_start, n_min, cap, r):
    """Everything the rule promises about one sample's result r, from the inputs alone (the steps are replayed from r's own
    target / cand / planes, never from the rule's code)."""
    M, P, K = raw.shape[0], u_start.shape[0], normals.shape[1]
    label, counts, order = r["label"], r["counts"], r["order"]
    assert label.dtype == np.uint8 and label.shape == (M,) and label.max() < P                  # the labels partition the cloud
    assert np.array_equal(counts, np.bincount(label, minlength=P)) and counts.sum() == M
    assert order.dtype == np.int32 and np.array_equal(order, np.argsort(label, kind="stable"))
    for p in range(P):
        rows = raw[label == p]                                                                  # (boolean mask: cloud order)
        piece = r["pieces"][p]
        assert piece.shape == (cap, 3) and piece.dtype == np.float32
        kept = min(len(rows), cap)
        assert piece[:kept].tobytes() == rows[:kept].tobytes()
        fill = rows[0] if len(rows) else raw[0]
        assert all(row.tobytes() == fill.tobytes() for row in piece[kept:])
        want = max(0, min(int(counts[p]) - 1, int(np.floor(u_start[p] * counts[p]))))
        assert r["start"][p] == want
    # replay: the label of every point after each step, from the recorded planes
    lab = np.zeros(M, dtype=np.int64)
    all_valid = True
    for s in range(1, P):
        cnt = np.bincount(lab, minlength=P)
        t = int(r["target"][s - 1])
        assert t < s and cnt[t] == cnt[:s].max() and (cnt[:t] < cnt[t]).all()                   # the first largest label
        members = np.flatnonzero(lab == t)
        ups, anchors = [], []
        for k in range(K):
            a = members[max(0, min(len(members) - 1, int(np.floor(u_anchor[s - 1, k] * len(members)))))]
            n = normals[s - 1, k]
            pa = raw[a].astype(np.float64)
            plane = np.array([n[0], n[1], n[2], -((pa[0] * n[0] + pa[1] * n[1]) + pa[2] * n[2])])
            ups.append(int((side(raw[members], plane) >= 0).sum()))
            anchors.append((a, plane))
        valid = [k for k in range(K) if ups[k] >= n_min and len(members) - ups[k] >= n_min]
        bal = [min(u, len(members) - u) for u in ups]
        k = int(r["cand"][s - 1])
        if valid:
            assert k == valid[0]                                                                # the first valid candidate
        else:
            all_valid = False
            assert k == int(np.argmax(bal))                                                     # the first most balanced one
        a, plane = anchors[k]
        assert r["planes"][s - 1].tobytes() == plane.tobytes()
        assert side(raw[a:a + 1], plane)[0] == 0.0                                              # the anchor: exactly 0, up
        d = side(raw[members], plane)
        lab[members[d < 0]] = s
        assert (side(raw[label == s], plane) < 0).all()                # label s (now and at the end): the down side of its plane
        assert (side(raw[lab == t], plane) >= 0).all()                 # what the target keeps: the up side
        assert (lab == s).sum() + (lab == t).sum() == len(members)
    assert np.array_equal(lab, label)
    assert r["ok"] == (all_valid and counts.max() <= cap)
