"""Pair tables for the beam tests (tests/test_assembly_beam_cpu.py, tests/test_gpu_assemble_beam.py): the kinds of
tests/_walk_cases.py with a random symmetric positive moment per piece, and `planted`: a table that is right up to noise, with a
few false entries whose score is lower than every true one's.  numpy only."""
import numpy as np

from tests import _walk_cases as wc

KINDS = wc.KINDS + ("planted",)


def _rigid_inv(T):
    out = np.zeros_like(T)
    R, t = T[..., :3, :3], T[..., :3, 3]
    out[..., :3, :3] = np.swapaxes(R, -1, -2)
    out[..., :3, 3] = -np.einsum("...ji,...j->...i", R, t)
    out[..., 3, 3] = 1.0
    return out


def moments(rng, shape, n=128):
    """Second moments [*shape,4,4] float64 of n points uniform in [-0.5, 0.5]^3, homogeneous: symmetric and positive."""
    x = np.concatenate((rng.uniform(-0.5, 0.5, size=shape + (n, 3)), np.ones(shape + (n, 1))), axis=-1)
    return np.einsum("...na,...nb->...ab", x, x) / n


def planted(Z, P, seed, nfalse=2, share=1.0):
    """-> (score [Z,P,P] float32, T [Z,P,P,4,4] float32, moment [Z,P,4,4] float64, pose [Z,P,4,4] float64, mates [Z,P,P] bool).
    T[i,j] = pose_i inv(pose_j) with N(0, 0.005) on the translations; true scores uniform in [0.01, 0.02] where mates (symmetric,
    drawn with probability `share`, the chain i, i + 1 always set), +inf elsewhere; nfalse off-diagonal entries with a score
    uniform in [0.001, 0.005] and a fresh rigid pose."""
    rng = np.random.default_rng([seed, P, nfalse, 77])
    pose = wc.rigid(rng, (Z, P)).astype(np.float64)
    T = np.einsum("ziab,zjbc->zijac", pose, _rigid_inv(pose))
    T[..., :3, 3] += rng.normal(0.0, 0.005, size=(Z, P, P, 3))
    up = np.triu(rng.random((Z, P, P)) < share, 1)
    mates = up | np.swapaxes(up, 1, 2)
    idx = np.arange(P - 1)
    mates[:, idx, idx + 1] = mates[:, idx + 1, idx] = True
    S = np.where(mates, rng.uniform(0.01, 0.02, size=(Z, P, P)), np.inf)
    S[:, np.arange(P), np.arange(P)] = np.inf
    for z in range(Z):
        off = np.flatnonzero(~np.eye(P, dtype=bool).reshape(-1))
        for f in rng.choice(off, size=nfalse, replace=False):
            i, j = divmod(int(f), P)
            S[z, i, j] = rng.uniform(0.001, 0.005)
            T[z, i, j] = wc.rigid(rng, ())
    return S.astype(np.float32), T.astype(np.float32), moments(rng, (Z, P)), pose, mates


def make(kind, Z, K, seed):
    """-> (score [Z,K,K] float32, T [Z,K,K,4,4] float32, moment [Z,K,4,4] float64, max_score or None)."""
    if kind == "planted":
        S, T, M, _, _ = planted(Z, K, seed, nfalse=min(2, K * (K - 1) // 2), share=0.5)
        return S, T, M, None
    S, T, max_score = wc.make(kind, Z, K, seed)
    return S, T, moments(np.random.default_rng([seed, K, 99]), (Z, K)), max_score


def ragged(Z, K):
    """Counts [Z] int32 for Z >= 5 puzzles: 0, 1, K and values between."""
    c = np.array([K, 1, max(2, K - 1), 0, max(2, (K + 1) // 2)] + [K] * (Z - 5), dtype=np.int32)
    return c[:Z]
