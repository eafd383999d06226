"""Float64 NumPy restatement of ops.icp_refine (csrc/icprefine.hip; the contract is in include/pzn.h), and the inputs the
ICP tests share.  Nothing here is tuned to the kernel: the rotation comes from an SVD (Kabsch with the reflection fix), the
kernel's from Horn's quaternion; both minimise the same sum.

  objective(a, b, T)            E(T), the two arg-min vectors (lowest index on ties) and the smallest margin
  step(a, b, c1, c2, T)         the candidate pose from given correspondences (degenerate pairs keep T's rotation)
  step_f32(a, b, c1, c2, T)     the same step in plain float32 with sequential sums: the yardstick of the device's step
  refine(a, b, T0, iters)       the full loop: candidate rounded to float32, taken iff E(T') < E(T)
  distance_bound(a, b, T)       the fp32 rounding bound of every squared distance the kernel forms
  curve_case(...)               two samplings of one noisy closed curve, a known motion and a perturbed start pose
"""
import collections

import numpy as np

DEGENERATE = 1e-10      # ICP_DEGENERATE of csrc/icprefine.hip: degenerate iff m2 <= DEGENERATE * trace^2 (see step)

U32 = 2.0 ** -24        # unit roundoff of float32
TRANSFORM_ROUNDINGS = 4      # x' = ((r00 x + r01 y) + r02 z) + t0: a product and three sums on the longest path
SUM_ROUNDINGS = 3            # (dx^2 + dy^2) + dz^2: the square and two sums on the longest path

Refined = collections.namedtuple("Refined", "T score score0 iters_used margin scores")


def _gamma(n):
    return n * U32 / (1.0 - n * U32)


def transform(T, b):
    T = np.asarray(T, dtype=np.float64)
    return np.asarray(b, dtype=np.float64) @ T[:3, :3].T + T[:3, 3]


def sqdist(a, tb):
    d = np.asarray(a, dtype=np.float64)[:, None, :] - tb[None, :, :]
    return (d * d).sum(-1)      # [ka, kb]


def _margin(D, axis):
    if D.shape[axis] < 2:
        return np.inf
    two = np.partition(D, 1, axis=axis)
    two = np.take(two, [0, 1], axis=axis)
    return float((np.take(two, 1, axis=axis) - np.take(two, 0, axis=axis)).min())


def objective(a, b, T):
    """-> (E, c1 [ka], c2 [kb], margin): E = mean_i min_j |a_i - T b_j|^2 + mean_j min_i |a_i - T b_j|^2; np.argmin returns
    the first (lowest) index of the minimum; margin = the smallest (second-smallest - smallest) squared distance over the
    rows of both directions (inf where a direction has one candidate only)."""
    D = sqdist(a, transform(T, b))
    c1, c2 = D.argmin(axis=1), D.argmin(axis=0)
    E = D.min(axis=1).mean() + D.min(axis=0).mean()
    return float(E), c1, c2, min(_margin(D, 1), _margin(D, 0))


def _pairs(a, b, c1, c2, dtype):
    a, b = np.asarray(a, dtype=dtype), np.asarray(b, dtype=dtype)
    return np.concatenate((a, a[c2])), np.concatenate((b[c1], b))      # fixed-side p, moved-side q: ka + kb pairs


def _kabsch(S):
    """R maximising sum p . R q for S = sum q p^T: V diag(1, 1, det) U^T of S = U s V^T."""
    Uu, _, Vt = np.linalg.svd(S)
    V = Vt.T
    d = np.sign(np.linalg.det(V @ Uu.T))
    d = 1.0 if d == 0 else d
    return V @ np.diag(np.array([1.0, 1.0, d], dtype=S.dtype)) @ Uu.T


def is_degenerate(C):
    """The one degenerate rule: C = the scatter of the centred moved-side points of the pairs; with its trace tr and the sum m2
    of its three principal 2x2 minors (l1 l2 + l1 l3 + l2 l3 for eigenvalues l), degenerate iff m2 <= DEGENERATE tr^2: a
    single point, coincident points (tr = 0) and collinear points."""
    tr = C[0, 0] + C[1, 1] + C[2, 2]
    m2 = (C[0, 0] * C[1, 1] - C[0, 1] ** 2) + (C[0, 0] * C[2, 2] - C[0, 2] ** 2) + (C[1, 1] * C[2, 2] - C[1, 2] ** 2)
    return bool(m2 <= DEGENERATE * tr * tr)


def step(a, b, c1, c2, T, round32=False):
    """The rigid motion minimising sum_i |a_i - T' b_c1(i)|^2 + sum_j |a_c2(j) - T' b_j|^2, float64 -> [4,4] (float32 values
    with round32).  Degenerate pairs keep T's rotation and update the translation only."""
    p, q = _pairs(a, b, c1, c2, np.float64)
    pc, qc = p.mean(axis=0), q.mean(axis=0)
    pd, qd = p - pc, q - qc
    if is_degenerate(qd.T @ qd):
        R = np.asarray(T, dtype=np.float64)[:3, :3].copy()
    else:
        R = _kabsch(qd.T @ pd)
    out = np.eye(4)
    out[:3, :3] = R
    out[:3, 3] = pc - R @ qc
    if round32:
        out = out.astype(np.float32).astype(np.float64)
    return out


def _seq_sum32(x):
    """Column sums of a float32 array, one addition after the other in float32."""
    return np.cumsum(x, axis=0, dtype=np.float32)[-1]


def step_f32(a, b, c1, c2, T):
    """The same step written the plain way in float32: sequential float32 sums for the centroids and the cross-covariance,
    a float32 SVD -> [4,4] float32.  Its distance from step() is the yardstick the device's step is held to."""
    p, q = _pairs(a, b, c1, c2, np.float32)
    n = np.float32(p.shape[0])
    pc, qc = _seq_sum32(p) / n, _seq_sum32(q) / n
    pd, qd = p - pc, q - qc
    if is_degenerate((qd.astype(np.float64).T @ qd.astype(np.float64))):
        R = np.asarray(T, dtype=np.float32)[:3, :3].copy()
    else:
        S = _seq_sum32((qd[:, :, None] * pd[:, None, :]).reshape(-1, 9)).reshape(3, 3)
        R = _kabsch(S).astype(np.float32)
    out = np.eye(4, dtype=np.float32)
    out[:3, :3] = R
    out[:3, 3] = pc - R @ qc
    return out


def pose_err(T, want):
    """Largest absolute difference over the 12 entries of [R | t]."""
    return float(np.abs(np.asarray(T, dtype=np.float64)[:3] - np.asarray(want, dtype=np.float64)[:3]).max())


def refine(a, b, T0, iters):
    """The loop of pzn_icp_refine_f32 in float64: the pose is a set of float32 VALUES (T0 as given, every candidate rounded),
    evaluated in float64 on the original b -> Refined(T, score, score0, iters_used, margin, scores); margin = the smallest
    nearest-neighbour margin met at any pose that was evaluated, scores = E after every accepted step."""
    T = np.asarray(T0, dtype=np.float32).astype(np.float64)
    E, c1, c2, margin = objective(a, b, T)
    E0, used, scores = E, 0, [E]
    for _ in range(int(iters)):
        cand = step(a, b, c1, c2, T, round32=True)
        En, n1, n2, m = objective(a, b, cand)
        margin = min(margin, m)
        if not En < E:
            break
        T, E, c1, c2, used = cand, En, n1, n2, used + 1
        scores.append(E)
    return Refined(T, E, E0, used, margin, scores)


def distance_bound(a, b, T):
    """[ka, kb] float64: a bound on |d32 - d| for every pair, d32 = the kernel's float32 squared distance between a_i and T
    b_j, d = the float64 one.  Derivation (u = 2^-24, gamma_n = n u / (1 - n u)):
      * transform: x' = ((r00 x + r01 y) + r02 z) + t0 in float32 has |x32' - x'| <= gamma_4 M, M = |r00 x| + |r01 y| +
        |r02 z| + |t0| (a product and three sums round on the longest path: TRANSFORM_ROUNDINGS);
      * difference: fl(a - x32') is off the exact a - x' = delta by eta <= gamma_4 M (1 + u) + u |delta|;
      * squares and their sum: (dx^2 + dy^2) + dz^2 rounds three times on the longest path (SUM_ROUNDINGS), so
        |d32 - d| <= sum_c (2 |delta_c| eta_c + eta_c^2) + gamma_3 sum_c (|delta_c| + eta_c)^2."""
    T = np.asarray(T, dtype=np.float64)
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    M = np.abs(b) @ np.abs(T[:3, :3]).T + np.abs(T[:3, 3])                     # [kb, 3]
    delta = np.abs(a[:, None, :] - transform(T, b)[None, :, :])                # [ka, kb, 3]
    eta = _gamma(TRANSFORM_ROUNDINGS) * M[None] * (1.0 + U32) + U32 * delta
    return (2.0 * delta * eta + eta * eta).sum(-1) + _gamma(SUM_ROUNDINGS) * ((delta + eta) ** 2).sum(-1)


def objective_interval(a, b, T):
    """[lo, hi] that must hold the kernel's float32 E(T): every row minimum lies in [min_j (d - bound), min_j (d + bound)]
    (distance_bound); a float32 sum of n non-negative terms in ANY order, its division by n and the final addition are
    off by a factor within 1 -+ gamma_(n+2)."""
    D = sqdist(a, transform(T, b))
    Bd = distance_bound(a, b, T)
    lo = np.maximum((D - Bd).min(axis=1), 0.0).mean() + np.maximum((D - Bd).min(axis=0), 0.0).mean()
    hi = (D + Bd).min(axis=1).mean() + (D + Bd).min(axis=0).mean()
    g = _gamma(max(D.shape) + 2)
    return lo * (1.0 - g), hi * (1.0 + g)


def nearest_bound(a, b, T):
    """The largest distance_bound over the nearest-neighbour pairs of both directions under T: the scale a margin is
    compared with."""
    D = sqdist(a, transform(T, b))
    Bd = distance_bound(a, b, T)
    r = np.arange(D.shape[0])
    c = np.arange(D.shape[1])
    return float(max(Bd[r, D.argmin(axis=1)].max(), Bd[D.argmin(axis=0), c].max()))


# --------------------------------------------------------------------------- inputs

def rot(axis, angle):
    axis = np.asarray(axis, dtype=np.float64)
    axis = axis / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def rigid(R, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T


def curve(s, planar):
    """A closed curve without symmetry, coordinates of size about 0.5; s in [0, 1)."""
    w = 2 * np.pi * np.asarray(s, dtype=np.float64)
    r = 0.40 + 0.08 * np.cos(3 * w + 0.4) + 0.05 * np.sin(5 * w) + 0.06 * np.cos(w + 1.0)
    z = np.zeros_like(w) if planar else 0.15 * np.sin(2 * w) + 0.10 * np.cos(3 * w + 0.7)
    return np.stack((r * np.cos(w), 0.7 * r * np.sin(w), z), axis=-1)


Case = collections.namedtuple("Case", "a b T0 G")


def curve_case(rng, ka, kb, planar, noise=0.003, angle=np.deg2rad(8.0), shift=0.03):
    """Two samplings (ka and kb random parameters) of one closed curve with `noise` added to every point, in a random
    orientation; the moved set is taken out of place by a known motion G (G maps it back onto the fixed set) and the start
    pose is G perturbed by a rotation of up to `angle` about a random axis and a shift of up to `shift` per axis
    -> Case(a [ka,3] f32, b [kb,3] f32, T0 [4,4] f32, G [4,4] f64)."""
    W = rot(rng.normal(size=3), rng.uniform(0, np.pi))
    a = curve(rng.uniform(0, 1, ka), planar) @ W.T + rng.normal(scale=noise, size=(ka, 3))
    bt = curve(rng.uniform(0, 1, kb), planar) @ W.T + rng.normal(scale=noise, size=(kb, 3))
    G = rigid(rot(rng.normal(size=3), rng.uniform(0.3, 2.5)), rng.uniform(-0.3, 0.3, 3))
    b = (bt - G[:3, 3]) @ G[:3, :3]                                     # G^-1 applied: G b = bt
    c = a.mean(axis=0)
    Rp = rot(rng.normal(size=3), rng.uniform(-angle, angle))
    Pm = rigid(Rp, c - Rp @ c + rng.uniform(-shift, shift, 3))         # the perturbation turns about the set's centre
    return Case(a.astype(np.float32), b.astype(np.float32), (Pm @ G).astype(np.float32), G)
