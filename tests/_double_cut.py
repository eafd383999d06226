"""Shared by the double-cut tests (CPU and GPU): the statement datapipe.double_cut_rule applied to a batch and laid out as
pzn_cut_compact_double_f32 lays its outputs out, the draws of a batch, float64 margins, and a float64 chamfer."""
import numpy as np


def shells(B, M, seed):
    """Origin-centred ellipsoid shells (the planes normal = rand(3), z = rand() / 3 never cut a cloud in the positive octant)."""
    rng = np.random.RandomState(seed)
    v = rng.randn(B, M, 3).astype(np.float32)
    v /= np.linalg.norm(v, axis=2, keepdims=True)
    return (v * (0.25 + 0.2 * rng.rand(B, 1, 3).astype(np.float32))).astype(np.float32)


def draws(B, K, seed):
    """-> planes1 [B,K,4], planes2 [B,7,4], u [B,7] float64, in the ranges the feeder draws them in."""
    rng = np.random.RandomState(seed)
    planes1 = np.concatenate([rng.rand(B, K, 3), rng.rand(B, K, 1) / 3], axis=2)
    planes2 = np.concatenate([rng.rand(B, 7, 3), rng.rand(B, 7, 1) / 3], axis=2)
    return planes1, planes2, rng.rand(B, 7)


def margins(raw, planes):
    """|p . normal + z| in float64 for every point of raw [M,3] and every plane [..., 4] -> [..., M]"""
    p = raw.astype(np.float64)
    planes = np.asarray(planes, dtype=np.float64)
    return np.abs(np.einsum("...c,mc->...m", planes[..., :3], p) + planes[..., 3:4])


def padded(rows, first_of_cloud, cap):
    """A piece as the kernels store it: `cap` rows, the rows that fit, then copies of the piece's first row (of the cloud's
    first row when the piece is empty or absent)."""
    out = np.empty((cap, 3), dtype=np.float32)
    out[:] = rows[0] if rows is not None and len(rows) else first_of_cloud
    if rows is not None:
        out[:min(len(rows), cap)] = rows[:cap]
    return out


def batch_statement(raw, planes1, planes2, u, n, n_rich, cap):
    """double_cut_rule per sample -> (list of its dicts, the kernel's outputs as numpy arrays: pieces [4B,cap,3], counts [4B],
    start [4B], kind [B], planes [B,2,4], tabs [B,4], ok [B])"""
    from puzzlenet_amd import datapipe
    B = raw.shape[0]
    recs = [datapipe.double_cut_rule(raw[b], planes1[b], planes2[b], u[b], n=n, n_rich=n_rich, cap=cap) for b in range(B)]
    pieces = np.empty((4 * B, cap, 3), dtype=np.float32)
    counts, start = np.empty(4 * B, dtype=np.int64), np.empty(4 * B, dtype=np.int64)
    for b, r in enumerate(recs):
        for p in range(4):
            pieces[p * B + b] = padded(r["pieces"][p], raw[b, 0], cap)
            counts[p * B + b], start[p * B + b] = r["counts"][p], r["start"][p]
    kind = np.array([r["kind"] for r in recs], dtype=np.int32)
    planes = np.stack([r["planes"] for r in recs])
    tabs = np.array([list(r["u_tab"]) + list(r["d_tab"]) for r in recs], dtype=np.int32)
    ok = np.array([r["ok"] for r in recs], dtype=bool)
    return recs, (pieces, counts, start, kind, planes, tabs, ok)


def chamfer_cd(a, b):
    """mean over b of the squared distance to the nearest a + mean over a of that to the nearest b, float64 (the reference's
    `torch.mean(cd1) + torch.mean(cd2)`, dataset.py:1253-1254).  a [n,3], b [m,3]"""
    a, b = a.astype(np.float64), b.astype(np.float64)
    P = ((a[:, None, :] - b[None, :, :]) ** 2).sum(-1)
    return P.min(0).mean() + P.min(1).mean()
