"""Piles for the forest beam tests (tests/test_assembly_forest_beam_cpu.py, tests/test_gpu_assemble_forest_beam.py): Q planted
objects of tests/_beam_cases.py - right up to noise, with a few false entries that score below every true one - in one shuffled
table, with scores across objects above the threshold.  numpy only."""
import numpy as np

from tests import _beam_cases as bc
from tests import _walk_cases as wc

MAX_SCORE = 0.03      # above every true score (<= 0.02), below every score across objects (>= 0.05)


def pile(seed, Q, P, nfalse=2):
    """-> (score [K,K] float32, T [K,K,4,4] float32, moment [K,4,4] float64, pose [K,4,4] float64, object_of [K], max_score),
    K = Q P: scores uniform in [0.05, 0.1] with random rigid poses, the diagonal block of object q replaced by
    planted(1, P, 1000 seed + q, nfalse, share=1.0), rows and columns under one permutation."""
    rng = np.random.default_rng([seed, 5])
    K = Q * P
    S = rng.uniform(0.05, 0.1, size=(K, K)).astype(np.float32)
    T = wc.rigid(rng, (K, K))
    M = np.zeros((K, 4, 4))
    pose = np.zeros((K, 4, 4))
    for q in range(Q):
        s, t, m, x, _ = bc.planted(1, P, 1000 * seed + q, nfalse, share=1.0)
        at = slice(q * P, (q + 1) * P)
        S[at, at], T[at, at], M[at], pose[at] = s[0], t[0], m[0], x[0]
    perm = rng.permutation(K)
    S, T = S[perm][:, perm], T[perm][:, perm]
    return np.ascontiguousarray(S), np.ascontiguousarray(T), M[perm], pose[perm], perm // P, MAX_SCORE


def piles(seeds, Q, P, nfalse=2):
    """pile() for every seed, stacked -> (score [Z,K,K], T, moment, pose, object_of [Z,K], max_score)."""
    each = [pile(s, Q, P, nfalse) for s in seeds]
    return tuple(np.stack([e[n] for e in each]) for n in range(5)) + (MAX_SCORE,)


def right(G, component, roots, n_components, pose, object_of, tol=0.05):
    """A pile's answer is right when its components are the objects and every G[p] is within tol, entry by entry, of
    pose[root of p's component] inv(pose[p])."""
    K = len(object_of)
    comp = np.asarray(component)[:K]
    together = comp[:, None] == comp[None, :]
    if (comp < 0).any() or not np.array_equal(together, object_of[:, None] == object_of[None, :]):
        return False
    rts = np.asarray(roots)[:int(n_components)]
    truth = np.einsum("pab,pbc->pac", pose[rts[comp]], bc._rigid_inv(pose))
    return bool((np.abs(np.asarray(G)[:K] - truth) <= tol).all())
