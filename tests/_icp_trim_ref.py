"""Float64 NumPy statement of the trimmed pose refinement (ops.icp_refine(..., keep=(m_a, m_b)); csrc/icprefine.hip,
icp_trim_kernel; the contract is in include/pzn.h), on top of tests/_icp_ref.py, and the partial-contact inputs its tests
share.  Nothing here is tuned to the kernel.

The rule, for counts 1 <= m_a <= ka and 1 <= m_b <= kb that are fixed for a refinement:
  * kept set: of one direction's rows under a pose, the m rows with the smallest (row minimum, row index) in lexicographic
    order - among equal minima the lowest row index is kept;
  * objective: E(T) = (sum of the kept a-row minima) / m_a + (sum of the kept b-row minima) / m_b;
  * step: the least-squares rigid motion of the m_a + m_b pairs of the kept rows alone, each weighted the same (_icp_ref's
    centroids, degenerate rule and Kabsch solve over those pairs);
  * loop: the candidate is taken iff E(T') < E(T), each with its own pose's kept sets; at most `iters` accepted steps.
m_a = ka, m_b = kb is _icp_ref.refine, value for value.

  kept_rows(minima, m)                 the kept rows, ascending
  objective(a, b, T, m_a, m_b)         -> Objective(E, c1, c2, kept_a, kept_b, margin, keep_margin)
  step(a, b, c1, c2, kept_a, kept_b, T)  the candidate pose from the kept pairs
  refine(a, b, T0, iters, m_a, m_b)    the loop -> Trimmed
  kept_slack(...) / objective_interval(...)   what float32 arithmetic may do to a kept set and to E
  partial_case(...)                    a moved set of which only a share mates with the fixed set
  non_mate(...)                        the same moved set with its mating share replaced
"""
import collections

import numpy as np

from tests import _icp_ref as ref

Objective = collections.namedtuple("Objective", "E c1 c2 kept_a kept_b margin keep_margin")
Trimmed = collections.namedtuple("Trimmed", "T score score0 iters_used margin scores kept_a kept_b keep_margin c1 c2")


def kept_rows(minima, m):
    """The m rows of smallest (minimum, index), ascending: a stable sort by value keeps equal values in index order."""
    minima = np.asarray(minima)
    return np.sort(np.argsort(minima, kind="stable")[:int(m)])


def _keep_margin(minima, m):
    """(m+1)-th smallest minus m-th smallest minimum of a direction; inf where every row is kept."""
    if m >= minima.shape[0]:
        return np.inf
    s = np.sort(minima)
    return float(s[m] - s[m - 1])


def objective(a, b, T, m_a, m_b):
    """-> Objective: E of the rule above; c1 [ka], c2 [kb] the arg-mins of every row (lowest index on ties), kept_a [m_a],
    kept_b [m_b] ascending; margin = _icp_ref.objective's nearest-neighbour margin (over all rows); keep_margin = the smaller
    of the two directions' (m+1)-th minus m-th smallest row minimum."""
    D = ref.sqdist(a, ref.transform(T, b))
    c1, c2 = D.argmin(axis=1), D.argmin(axis=0)
    r1, r2 = D.min(axis=1), D.min(axis=0)
    ka_, kb_ = kept_rows(r1, m_a), kept_rows(r2, m_b)
    E = r1[ka_].mean() + r2[kb_].mean()
    return Objective(float(E), c1, c2, ka_, kb_, min(ref._margin(D, 1), ref._margin(D, 0)),
                     min(_keep_margin(r1, m_a), _keep_margin(r2, m_b)))


def step(a, b, c1, c2, kept_a, kept_b, T, round32=False):
    """_icp_ref.step over the pairs of the kept rows: (a_i, b_c1(i)) for i in kept_a and (a_c2(j), b_j) for j in kept_b,
    m_a + m_b pairs of one weight; degenerate pairs keep T's rotation."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    p = np.concatenate((a[kept_a], a[c2[kept_b]]))
    q = np.concatenate((b[c1[kept_a]], b[kept_b]))
    pc, qc = p.mean(axis=0), q.mean(axis=0)
    pd, qd = p - pc, q - qc
    if ref.is_degenerate(qd.T @ qd):
        R = np.asarray(T, dtype=np.float64)[:3, :3].copy()
    else:
        R = ref._kabsch(qd.T @ pd)
    out = np.eye(4)
    out[:3, :3] = R
    out[:3, 3] = pc - R @ qc
    if round32:
        out = out.astype(np.float32).astype(np.float64)
    return out


def step_f32(a, b, c1, c2, kept_a, kept_b, T):
    """_icp_ref.step_f32 over the kept pairs: the step written the plain way in float32 with sequential sums -> [4,4] float32.
    Its distance from step() is the yardstick the device's step is held to."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    p = np.concatenate((a[kept_a], a[c2[kept_b]]))
    q = np.concatenate((b[c1[kept_a]], b[kept_b]))
    n = np.float32(p.shape[0])
    pc, qc = ref._seq_sum32(p) / n, ref._seq_sum32(q) / n
    pd, qd = p - pc, q - qc
    if ref.is_degenerate(qd.astype(np.float64).T @ qd.astype(np.float64)):
        R = np.asarray(T, dtype=np.float32)[:3, :3].copy()
    else:
        S = ref._seq_sum32((qd[:, :, None] * pd[:, None, :]).reshape(-1, 9)).reshape(3, 3)
        R = ref._kabsch(S).astype(np.float32)
    out = np.eye(4, dtype=np.float32)
    out[:3, :3] = R
    out[:3, 3] = pc - R @ qc
    return out


def refine(a, b, T0, iters, m_a, m_b):
    """The loop of pzn_icp_refine_trim_f32 in float64 (poses are float32 VALUES, as in _icp_ref.refine) -> Trimmed: kept_a /
    kept_b are the rows kept under the RETURNED pose, c1 / c2 the arg-mins under it, margin / keep_margin the smallest met at
    any pose that was evaluated, scores = E after every accepted step."""
    T = np.asarray(T0, dtype=np.float32).astype(np.float64)
    o = objective(a, b, T, m_a, m_b)
    E0, used, scores = o.E, 0, [o.E]
    margin, keep_margin = o.margin, o.keep_margin
    for _ in range(int(iters)):
        cand = step(a, b, o.c1, o.c2, o.kept_a, o.kept_b, T, round32=True)
        n = objective(a, b, cand, m_a, m_b)
        margin, keep_margin = min(margin, n.margin), min(keep_margin, n.keep_margin)
        if not n.E < o.E:
            break
        T, o, used = cand, n, used + 1
        scores.append(o.E)
    return Trimmed(T, o.E, E0, used, margin, scores, o.kept_a, o.kept_b, keep_margin, o.c1, o.c2)


def kept_slack(a, b, T):
    """The scale a float32 kept set is held to: twice the largest _icp_ref.distance_bound.  A float32 row minimum is within
    one bound of the float64 one (the minimum of values each within B of the truth), so two rows whose float32 minima come
    in the other order than their float64 ones differ by at most two bounds."""
    return 2.0 * float(ref.distance_bound(a, b, T).max())


def objective_interval(a, b, T, m_a, m_b):
    """_icp_ref.objective_interval in trimmed form: every float32 row minimum lies in [min (d - B), min (d + B)]; the sum of
    the m smallest of n values is monotone in every one of them, so the m smallest lower ends bound it from below and the m
    smallest upper ends from above, whichever rows the kernel kept; sum, division and addition as there."""
    D = ref.sqdist(a, ref.transform(T, b))
    Bd = ref.distance_bound(a, b, T)

    def part(lo, hi, m):
        return np.sort(np.maximum(lo, 0.0))[:m].mean(), np.sort(hi)[:m].mean()
    lo1, hi1 = part((D - Bd).min(axis=1), (D + Bd).min(axis=1), m_a)
    lo2, hi2 = part((D - Bd).min(axis=0), (D + Bd).min(axis=0), m_b)
    g = ref._gamma(max(D.shape) + 2)
    return (lo1 + lo2) * (1.0 - g), (hi1 + hi2) * (1.0 + g)


# --------------------------------------------------------------------------- inputs

Partial = collections.namedtuple("Partial", "a b T0 G mating")

OTHER_GAP = (0.25, 0.5)      # the closest approach of the other faces' curve to the shared curve


def _other_curve(rng, n, W, centre, noise, planar, dense):
    """n noisy points of an unrelated closed curve (another orientation, 0.6 of the size) whose closest approach to the
    densely sampled shared curve `dense` is a draw from OTHER_GAP: pushed out along a random direction until it is."""
    W2 = ref.rot(rng.normal(size=3), rng.uniform(0, np.pi)) @ W
    shape = 0.6 * ref.curve(np.linspace(0, 1, 200, endpoint=False), planar) @ W2.T
    d = rng.normal(size=3)
    d /= np.linalg.norm(d)
    gap = rng.uniform(*OTHER_GAP)

    def closest(t):
        return np.sqrt(ref.sqdist(dense, shape + centre + t * d).min())
    lo, hi = 0.0, 4.0      # at 4.0 the two curves (each within 0.6 of its centre) are at least 2.8 apart
    while closest(lo) > gap:      # (the draw already clears the gap at the centre: start inside it)
        lo -= 0.5
    for _ in range(40):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if closest(mid) < gap else (lo, mid)
    pts = 0.6 * ref.curve(rng.uniform(0, 1, n), planar) @ W2.T + centre + hi * d
    return pts + rng.normal(scale=noise, size=(n, 3))


def partial_case(rng, ka, kb, share, planar=False, noise=0.003, angle=np.deg2rad(8.0), shift=0.03):
    """_icp_ref.curve_case with a moved set of several faces: round(share kb) of its kb rows (`mating`, bool [kb]) are a
    second sampling of the fixed set's curve, the rest lies on an unrelated curve OTHER_GAP away from it - the faces towards
    other neighbours -, all rows in one random order -> Partial(a [ka,3] f32, b [kb,3] f32, T0 [4,4] f32, G [4,4] f64,
    mating).  The fixed set is all contact, so the keep counts of the true contact are (ka, round(share kb))."""
    n_mate = int(round(share * kb))
    W = ref.rot(rng.normal(size=3), rng.uniform(0, np.pi))
    a = ref.curve(rng.uniform(0, 1, ka), planar) @ W.T + rng.normal(scale=noise, size=(ka, 3))
    mate = ref.curve(rng.uniform(0, 1, n_mate), planar) @ W.T + rng.normal(scale=noise, size=(n_mate, 3))
    dense = ref.curve(np.linspace(0, 1, 400, endpoint=False), planar) @ W.T
    other = _other_curve(rng, kb - n_mate, W, a.mean(axis=0), noise, planar, dense)
    order = rng.permutation(kb)
    bt = np.concatenate((mate, other))[order]
    mating = (np.arange(kb) < n_mate)[order]
    G = ref.rigid(ref.rot(rng.normal(size=3), rng.uniform(0.3, 2.5)), rng.uniform(-0.3, 0.3, 3))
    b = (bt - G[:3, 3]) @ G[:3, :3]
    c = a.mean(axis=0)
    Rp = ref.rot(rng.normal(size=3), rng.uniform(-angle, angle))
    Pm = ref.rigid(Rp, c - Rp @ c + rng.uniform(-shift, shift, 3))
    return Partial(a.astype(np.float32), b.astype(np.float32), (Pm @ G).astype(np.float32), G, mating)


def non_mate(rng, case, noise=0.003):
    """The moved set of `case` with its mating rows replaced by a sampling of ANOTHER closed curve about the fixed set's centre
    (the planar curve at 0.6 of the size, in a random orientation: no rigid motion lays it on the shared curve): a piece
    whose other faces are the mate's and whose face towards the fixed piece does not fit it -> b [kb,3] f32, to be started
    at the mate's pose case.T0."""
    G = case.G
    n = int(case.mating.sum())
    c = case.a.astype(np.float64).mean(axis=0)
    W3 = ref.rot(rng.normal(size=3), rng.uniform(0, np.pi))
    fake = 0.6 * ref.curve(rng.uniform(0, 1, n), True) @ W3.T + c + rng.normal(scale=noise, size=(n, 3))
    b = case.b.astype(np.float64).copy()
    b[case.mating] = (fake - G[:3, 3]) @ G[:3, :3]
    return b.astype(np.float32)
