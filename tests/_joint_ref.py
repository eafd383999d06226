"""Float64 NumPy restatement of ops.joint_refine (csrc/jointrefine.hip; the contract is in include/pzn.h), built on
tests/_icp_ref.py, and the inputs the joint-refinement tests share.  Nothing here is tuned to the kernel: the rotation comes
from an SVD (Kabsch with the reflection fix), the kernel's from Horn's quaternion; the sums here are centred in two passes,
the kernel's are uncentred float64 sums about a reference point.

  joint_energy(P, G, e)            E_e(G), the two arg-min vectors (lowest index on ties) and the smallest margin
  piece_energy(P, G, p)            E_p(G): the sum of E_e over p's joints, their correspondences, the smallest margin
  total(P, G)                      E(G) and every E_e
  visit(P, G, p)                   the candidate pose of a visit (rounded to float32 values) from given or found correspondences
  visit_f32(P, G, p, corr)         the same visit in plain float32 with sequential sums: the yardstick of the device's visit
  refine(P, sweeps)                the full loop
  distance_bound2(a, b, Gi, Gj)    _icp_ref.distance_bound where BOTH points are moved
  objective_interval2(...)         the interval that must hold the kernel's float32 E_e
  puzzle(rng, K, joints, k, same)  K pieces, one noisy closed curve per joint, true poses and perturbed start poses
"""
import collections

import numpy as np

from tests import _icp_ref as ref

Puzzle = collections.namedtuple("Puzzle", "K joints A B G0 truth movable")
JointRefined = collections.namedtuple("JointRefined", "G score score0 sweeps_used accepted margin_ratio scores")

GRAPHS = {
    "pair": (2, [(0, 1)]),
    "chain3": (3, [(0, 1), (1, 2)]),
    "ring4": (4, [(0, 1), (1, 2), (2, 3), (3, 0)]),
    "both3": (3, [(0, 1), (1, 0), (1, 2), (2, 1), (0, 2)]),       # both directions of two joints plus a chord
    "complete5": (5, [(i, j) for i in range(5) for j in range(5) if i != j]),
}


def f32(G):
    """Float32 VALUES held in float64."""
    return np.asarray(G, dtype=np.float32).astype(np.float64)


def incident(P, p):
    return [e for e, (i, j) in enumerate(P.joints) if i == p or j == p]


def has_joint(P, p):
    return bool(P.movable[p]) and len(incident(P, p)) > 0


def _D(P, G, e):
    i, j = P.joints[e]
    return ref.sqdist(ref.transform(G[i], P.A[e]), ref.transform(G[j], P.B[e]))      # [ka, kb]


def joint_energy(P, G, e):
    """-> (E_e, c1 [ka], c2 [kb], margin), as _icp_ref.objective with both sides in the root frame."""
    D = _D(P, G, e)
    E = D.min(axis=1).mean() + D.min(axis=0).mean()
    return float(E), D.argmin(axis=1), D.argmin(axis=0), min(ref._margin(D, 1), ref._margin(D, 0))


def piece_energy(P, G, p):
    """-> (E_p, {e: (c1, c2)}, {e: margin}) over the joints incident to p, in list order."""
    E, corr, margins = 0.0, {}, {}
    for e in incident(P, p):
        Ee, c1, c2, m = joint_energy(P, G, e)
        E += Ee
        corr[e], margins[e] = (c1, c2), m
    return E, corr, margins


def total(P, G):
    each = [joint_energy(P, G, e)[0] for e in range(len(P.joints))]
    return float(sum(each)), each


def _pairs(P, G, p, corr, dtype):
    """The pairs of a visit -> x [n,3] in p's frame, y [n,3] in the root frame, w [n]: per joint the ka rows of A (weight
    1 / ka) then the kb rows of B (weight 1 / kb), joints in list order."""
    xs, ys, ws = [], [], []
    for e in incident(P, p):
        i, j = P.joints[e]
        a, b = np.asarray(P.A[e], dtype=dtype), np.asarray(P.B[e], dtype=dtype)
        c1, c2 = corr[e]
        pa, pb = np.concatenate((a, a[c2])), np.concatenate((b[c1], b))          # the pairs (a_ia, b_ib)
        w = np.concatenate((np.full(len(a), 1.0 / len(a)), np.full(len(b), 1.0 / len(b)))).astype(dtype)
        if i == p:
            far = np.asarray(G[j], dtype=dtype)
            xs.append(pa), ys.append(pb @ far[:3, :3].T + far[:3, 3])
        else:
            far = np.asarray(G[i], dtype=dtype)
            xs.append(pb), ys.append(pa @ far[:3, :3].T + far[:3, 3])
        ws.append(w)
    return np.concatenate(xs), np.concatenate(ys), np.concatenate(ws)


def visit(P, G, p, corr=None, round32=True):
    """The candidate G_p': the weighted rigid motion minimising sum w |G_p' x - y|^2 over the pairs of p's joints under G
    (corr: {e: (c1, c2)}, found under G when None), float64 -> [4,4] (float32 values with round32).  A degenerate scatter
    of x keeps G_p's rotation."""
    if corr is None:
        corr = piece_energy(P, G, p)[1]
    x, y, w = _pairs(P, G, p, corr, np.float64)
    W = w.sum()
    xc, yc = (w[:, None] * x).sum(axis=0) / W, (w[:, None] * y).sum(axis=0) / W
    xd, yd = x - xc, y - yc
    if ref.is_degenerate((w[:, None] * xd).T @ xd):
        R = np.asarray(G[p], dtype=np.float64)[:3, :3].copy()
    else:
        R = ref._kabsch((w[:, None] * xd).T @ yd)
    out = ref.rigid(R, yc - R @ xc)
    return f32(out) if round32 else out


def visit_f32(P, G, p, corr):
    """The same visit written the plain way in float32: float32 images of the far points, sequential float32 sums for the
    weighted centroids and the cross-covariance, a float32 SVD -> [4,4] float32."""
    x, y, w = _pairs(P, G, p, corr, np.float32)
    W = ref._seq_sum32(w[:, None])[0]
    xc, yc = ref._seq_sum32(w[:, None] * x) / W, ref._seq_sum32(w[:, None] * y) / W
    xd, yd = x - xc, y - yc
    x64 = xd.astype(np.float64)
    if ref.is_degenerate((w[:, None].astype(np.float64) * x64).T @ x64):
        R = np.asarray(G[p], dtype=np.float32)[:3, :3].copy()
    else:
        S = ref._seq_sum32(((w[:, None] * xd)[:, :, None] * yd[:, None, :]).reshape(-1, 9)).reshape(3, 3)
        R = ref._kabsch(S).astype(np.float32)
    out = np.eye(4, dtype=np.float32)
    out[:3, :3] = R
    out[:3, 3] = yc - R @ xc
    return out


def _bound(delta, Ma, Mb):
    """The bound below from |delta| [..., 3] and the two sides' M [..., 3] (broadcast against each other)."""
    eta = ref._gamma(ref.TRANSFORM_ROUNDINGS) * (Ma + Mb) * (1.0 + ref.U32) + ref.U32 * delta
    return (2.0 * delta * eta + eta * eta).sum(-1) + ref._gamma(ref.SUM_ROUNDINGS) * ((delta + eta) ** 2).sum(-1)


def _moved(G, x):
    """-> (G x in float64, M = |r00 x| + |r01 y| + |r02 z| + |t0| per coordinate)."""
    G, x = np.asarray(G, dtype=np.float64), np.asarray(x, dtype=np.float64)
    return ref.transform(G, x), np.abs(x) @ np.abs(G[:3, :3]).T + np.abs(G[:3, 3])


def distance_bound2(a, b, Gi, Gj):
    """[ka, kb] float64: a bound on |d32 - d|, d32 = the kernel's float32 squared distance between Gi a_r and Gj b_c, d the
    float64 one.  _icp_ref.distance_bound with both points moved (u = 2^-24, gamma_n = n u / (1 - n u)):
      * each side: x' = ((r00 x + r01 y) + r02 z) + t0 in float32 has |x32' - x'| <= gamma_4 M, M = |r00 x| + |r01 y| +
        |r02 z| + |t0|, for ITS pose and point: Ma [ka,3] and Mb [kb,3];
      * difference: fl(xa32' - xb32') is off the exact xa' - xb' = delta by eta <= gamma_4 (Ma + Mb)(1 + u) + u |delta|;
      * squares and their sum: as there, |d32 - d| <= sum_c (2 |delta_c| eta_c + eta_c^2) + gamma_3 sum_c (|delta_c| + eta_c)^2."""
    ta, Ma = _moved(Gi, a)
    tb, Mb = _moved(Gj, b)
    return _bound(np.abs(ta[:, None, :] - tb[None, :, :]), Ma[:, None, :], Mb[None, :, :])


def objective_interval2(a, b, Gi, Gj):
    """[lo, hi] that must hold the kernel's float32 E_e: _icp_ref.objective_interval on distance_bound2."""
    D = ref.sqdist(ref.transform(Gi, a), ref.transform(Gj, b))
    Bd = distance_bound2(a, b, Gi, Gj)
    lo = np.maximum((D - Bd).min(axis=1), 0.0).mean() + np.maximum((D - Bd).min(axis=0), 0.0).mean()
    hi = (D + Bd).min(axis=1).mean() + (D + Bd).min(axis=0).mean()
    g = ref._gamma(max(D.shape) + 2)
    return lo * (1.0 - g), hi * (1.0 + g)


def joint_intervals(P, G):
    """-> [J, 2]: objective_interval2 of every joint under G."""
    return np.array([objective_interval2(P.A[e], P.B[e], G[i], G[j]) for e, (i, j) in enumerate(P.joints)]).reshape(-1, 2)


def sum_interval(iv, joints=None):
    """The interval of a float32 sum, in any order, of values inside the rows of iv [n, 2] (all of them, or the listed ones):
    n - 1 additions of non-negative terms are off by a factor within 1 -+ gamma_n."""
    iv = iv if joints is None else iv[list(joints)]
    g = ref._gamma(max(len(iv), 1))
    return float(iv[:, 0].sum() * (1.0 - g)), float(iv[:, 1].sum() * (1.0 + g))


def nearest_bound2(a, b, Gi, Gj):
    """The largest distance_bound2 over the nearest-neighbour pairs of both directions: the scale a margin is compared with."""
    ta, Ma = _moved(Gi, a)
    tb, Mb = _moved(Gj, b)
    D = ref.sqdist(ta, tb)
    c1, c2 = D.argmin(axis=1), D.argmin(axis=0)
    return float(max(_bound(np.abs(ta - tb[c1]), Ma, Mb[c1]).max(), _bound(np.abs(ta[c2] - tb), Ma[c2], Mb).max()))


def nearest_bounds(P, G):
    return [nearest_bound2(P.A[e], P.B[e], G[i], G[j]) for e, (i, j) in enumerate(P.joints)]


def margin_ratio(P, G, p, scale):
    """The smallest (nearest-neighbour margin of joint e under G) / scale[e] over p's joints."""
    margins = piece_energy(P, G, p)[2]
    return min((m / scale[e] for e, m in margins.items()), default=np.inf)


def refine(P, sweeps):
    """The loop of pzn_joint_refine_f32 in float64: poses are float32 VALUES (G0 as given, every candidate rounded), evaluated
    in float64 -> JointRefined; sweeps_used = the sweeps that took at least one candidate, accepted [K] = candidates taken
    per piece, margin_ratio = the smallest nearest-neighbour margin met at any pose that was evaluated, in units of the
    joint's nearest_bound2 under G0 (where the distances, and so the bound, are largest), scores = E after every sweep."""
    G = f32(P.G0).copy()
    scale = nearest_bounds(P, G)
    E0 = total(P, G)[0]
    accepted = np.zeros(P.K, dtype=np.int64)
    used, ratio, scores = 0, np.inf, [E0]
    for _ in range(int(sweeps)):
        any_taken = False
        for p in range(P.K):
            if not has_joint(P, p):
                continue
            Ep, corr, margins = piece_energy(P, G, p)
            ratio = min([ratio] + [m / scale[e] for e, m in margins.items()])
            cand = visit(P, G, p, corr)
            Gn = G.copy()
            Gn[p] = cand
            En, _, margins = piece_energy(P, Gn, p)
            ratio = min([ratio] + [m / scale[e] for e, m in margins.items()])
            if En < Ep:
                G, any_taken = Gn, True
                accepted[p] += 1
        if not any_taken:
            break
        used += 1
        scores.append(total(P, G)[0])
    return JointRefined(G, total(P, G)[0], E0, used, accepted, ratio, scores)


# --------------------------------------------------------------------------- inputs

def _inverse(T):
    R, t = T[:3, :3], T[:3, 3]
    return ref.rigid(R.T, -R.T @ t)


def puzzle(rng, K, joints, k, same=False, noise=0.003, angle=np.deg2rad(4.0), shift=0.01, movable=None):
    """K pieces with random true poses; each joint (i, j) is one noisy closed curve (_icp_ref.curve) in a random orientation at
    a random place of the root frame, sampled ka times for piece i and kb times for piece j (k = ka = kb, or (ka, kb)), each
    sample with its own noise; same=True (ka = kb): B's points are A's in another order, so E = 0 at the truth up to
    the rounding of the points.  The points are taken into their pieces' frames (float32).  Start poses: piece 0 at the
    truth, every other piece's truth perturbed by a rotation of up to `angle` about a random axis through the centre of its
    joints' points and a shift of up to `shift` per axis.  movable: default every piece but 0."""
    ka, kb = (k, k) if np.isscalar(k) else k
    truth = np.stack([ref.rigid(ref.rot(rng.normal(size=3), rng.uniform(0.3, 2.5)), rng.uniform(-0.3, 0.3, 3)) for _ in range(K)])
    A, B, centre, count = [], [], np.zeros((K, 3)), np.zeros(K)
    for e, (i, j) in enumerate(joints):
        W = ref.rot(rng.normal(size=3), rng.uniform(0, np.pi))
        place = rng.uniform(-0.5, 0.5, 3)
        planar = bool(e & 1)
        ra = ref.curve(rng.uniform(0, 1, ka), planar) @ W.T + place + rng.normal(scale=noise, size=(ka, 3))
        if same:
            assert ka == kb
            rb = ra[rng.permutation(ka)]
        else:
            rb = ref.curve(rng.uniform(0, 1, kb), planar) @ W.T + place + rng.normal(scale=noise, size=(kb, 3))
        A.append(ref.transform(_inverse(truth[i]), ra).astype(np.float32))
        B.append(ref.transform(_inverse(truth[j]), rb).astype(np.float32))
        for p, pts in ((i, ra), (j, rb)):
            centre[p] += pts.mean(axis=0)
            count[p] += 1
    G0 = truth.copy()
    for p in range(1, K):
        c = centre[p] / max(count[p], 1)
        Rp = ref.rot(rng.normal(size=3), rng.uniform(-angle, angle))
        G0[p] = ref.rigid(Rp, c - Rp @ c + rng.uniform(-shift, shift, 3)) @ truth[p]
    if movable is None:
        movable = np.arange(K) > 0
    return Puzzle(K, [tuple(x) for x in joints], A, B, G0.astype(np.float32), truth, np.asarray(movable, dtype=bool))


def pose_error(G, truth):
    """Largest absolute difference over the 12 entries of [R | t], per piece -> [K]."""
    d = np.abs(np.asarray(G, dtype=np.float64)[:, :3] - np.asarray(truth, dtype=np.float64)[:, :3])
    return d.reshape(len(d), -1).max(axis=1)
