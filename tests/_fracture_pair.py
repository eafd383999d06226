"""Shared by the fracture-pair tests (CPU and GPU): the clouds and cut draws of tests/_fracture.py with the pair's own draws,
datapipe.fracture_pair_rule applied to a batch and laid out as pzn_fracture_pair_f32 lays its outputs out, and the rule's
invariants checked on one sample."""
import numpy as np

from tests import _double_cut as dc
from tests import _fracture as fr

clouds = fr.clouds
NAMES = ("pieces", "counts", "start", "kind", "pair", "label", "planes", "target", "cand", "ok")


def draws(B, P, K, seed, mag=0.8):
    """-> normals [B,P-1,K,3], u_anchor [B,P-1,K] (those of tests/_fracture.draws for the same seed), u [B,7] float64 uniforms
    (u_kind, u_a, u_c, u_sU, u_sD, u_sFU, u_sFD), twist [B,6] float32 of length mag"""
    normals, u_anchor, _, _ = fr.draws(B, P, K, seed, mag)
    rng = np.random.RandomState(seed + 7919)
    u = rng.rand(B, 7)
    x = rng.randn(B, 6)
    return normals, u_anchor, u, (x / np.linalg.norm(x, axis=1, keepdims=True) * mag).astype(np.float32)


def batch_statement(raw, normals, u_anchor, u, pieces, n_min, neighbours, cap):
    """fracture_pair_rule per sample -> (list of its dicts, the kernel's outputs as numpy arrays: pieces [4B,cap,3], counts
    [4B], start [4B], kind [B], pair [B,4], label [B,M], planes [B,P-1,4], target [B,P-1], cand [B,P-1], ok [B])"""
    from puzzlenet_amd import datapipe
    B, P = raw.shape[0], normals.shape[1] + 1
    recs = [datapipe.fracture_pair_rule(raw[b], normals[b], u_anchor[b], u[b], int(pieces[b]), P, n_min, neighbours, cap)
            for b in range(B)]
    out = np.empty((4 * B, cap, 3), dtype=np.float32)
    counts, start = np.empty(4 * B, dtype=np.int64), np.empty(4 * B, dtype=np.int64)
    for b, r in enumerate(recs):
        for q in range(4):
            out[q * B + b] = dc.padded(None, raw[b, 0], cap) if r["pieces"][q] is None else r["pieces"][q]
            counts[q * B + b], start[q * B + b] = r["counts"][q], r["start"][q]
    stack = lambda key: np.stack([r[key] for r in recs])
    return recs, (out, counts, start, np.array([r["kind"] for r in recs], dtype=np.int32), stack("pair"), stack("label"),
                  stack("planes"), stack("target"), stack("cand"), np.array([r["ok"] for r in recs], dtype=bool))


def check_invariants(raw, normals, u_anchor, u, Pb, n_min, neighbours, cap, r):
    """Everything the rule promises about one sample's result r beyond the fracture itself (which the callers compare with
    fracture_rule): the kind and the pair from the draws, the pieces from the labels."""
    from puzzlenet_amd import datapipe as dp
    P = normals.shape[0] + 1
    label, pair, counts = r["label"], r["pair"], r["counts"]
    assert label.dtype == np.uint8 and label.max() <= Pb - 1
    assert not r["planes"][Pb - 1:].any() and not r["target"][Pb - 1:].any() and not r["cand"][Pb - 1:].any()
    assert r["planes"].shape == (P - 1, 4) and pair.dtype == np.int32 and pair.shape == (4,)
    sib = (int(r["target"][Pb - 2]), Pb - 1)
    a = min(Pb - 1, int(np.floor(u[1] * Pb)))
    c = min(Pb - 2, int(np.floor(u[2] * (Pb - 1))))
    c += c >= a
    assert a != c and 0 <= a < Pb and 0 <= c < Pb
    neighbour = Pb >= 3 and u[0] < neighbours and {a, c} != set(sib)
    if neighbour:
        assert r["kind"] == dp.NEIGHBOUR and tuple(pair) == (a, c) + sib
    else:
        assert r["kind"] == dp.SIBLING and tuple(pair) == sib + (-1, -1)
        assert counts[2] == counts[3] == -1 and r["pieces"][2] is None and r["pieces"][3] is None
        assert r["start"][2] == r["start"][3] == 0
    for q in range(4):
        if pair[q] < 0:
            continue
        rows = raw[label == pair[q]]
        piece = r["pieces"][q]
        assert counts[q] == len(rows) and piece.shape == (cap, 3) and piece.dtype == np.float32
        assert piece.tobytes() == dc.padded(rows, raw[0], cap).tobytes()
        assert r["start"][q] == max(0, min(len(rows) - 1, int(np.floor(u[3 + q] * len(rows)))))
    # the sibling pair: the two sides of the last plane
    plane = r["planes"][Pb - 2]
    assert (fr.side(raw[label == sib[0]], plane) >= 0).all() and (fr.side(raw[label == sib[1]], plane) < 0).all()
    assert not r["ok"] or counts.max() <= cap


def cd64(Ub, Db):
    """The acceptance test's cd in float64 from the two boundaries."""
    return dc.chamfer_cd(Db, Ub)
