"""Pair tables for the walk tests (tests/test_assembly_walk_cpu.py, tests/test_gpu_assemble_walk.py): the kinds of score table
at which a greedy walk can go wrong, with random rigid float32 poses.  numpy only."""
import numpy as np

KINDS = ("lattice", "random", "nan30", "blocks", "max_score")


def rigid(rng, shape):
    """Random rigid motions [*shape,4,4] float32: Rodrigues' rotation by an angle in [0, pi) about a random axis, |t_i| <= 1."""
    w = rng.normal(size=shape + (3,))
    w /= np.linalg.norm(w, axis=-1, keepdims=True)
    th = rng.uniform(0, np.pi, size=shape)[..., None, None]
    Kx = np.zeros(shape + (3, 3))
    Kx[..., 0, 1], Kx[..., 0, 2], Kx[..., 1, 0] = -w[..., 2], w[..., 1], w[..., 2]
    Kx[..., 1, 2], Kx[..., 2, 0], Kx[..., 2, 1] = -w[..., 0], -w[..., 1], w[..., 0]
    T = np.zeros(shape + (4, 4))
    T[..., :3, :3] = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)
    T[..., :3, 3] = rng.uniform(-1, 1, size=shape + (3,))
    T[..., 3, 3] = 1.0
    return T.astype(np.float32)


def make(kind, Z, K, seed):
    """-> (score [Z,K,K] float32, T [Z,K,K,4,4] float32, max_score or None).
      lattice    integers 0..3: most rounds are decided by a tie (and the diagonal holds finite values the rule must ignore)
      random     uniform [0, 1)
      nan30      uniform with 30 % NaN
      blocks     two blocks of pieces with +inf between them: the walk cannot leave the root's block
      max_score  uniform, with max_score = 1 / (2 K), about the smallest of the last round's 2 (K - 1) candidates: the walk stops
                 somewhere in mid-range"""
    rng = np.random.default_rng([seed, K, KINDS.index(kind)])
    S = rng.random((Z, K, K))
    if kind == "lattice":
        S = rng.integers(0, 4, size=(Z, K, K)).astype(np.float64)
        S[(S == 0) & (rng.random((Z, K, K)) < 0.5)] = -0.0      # half of the zeros are -0: equal keys all the same
    elif kind == "nan30":
        S[rng.random((Z, K, K)) < 0.3] = np.nan
    elif kind == "blocks":
        h = (K + 1) // 2
        S[:, :h, h:] = np.inf
        S[:, h:, :h] = np.inf
    return S.astype(np.float32), rigid(rng, (Z, K, K)), (0.5 / K if kind == "max_score" else None)
