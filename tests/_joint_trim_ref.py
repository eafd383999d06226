"""Float64 NumPy statement of the joint refinement with kept rows chosen again under the joint poses
(ops.joint_refine(..., ma=, mb=); csrc/jointtrim.hip, joint_trim_kernel; the contract is in include/pzn.h), built on
tests/_joint_ref.py and tests/_icp_trim_ref.kept_rows, and the partial-contact puzzles its tests share.  Nothing here is tuned
to the kernel: the rotation comes from an SVD, the sums are centred in two passes, the kept rows come from a stable sort.

A TrimPuzzle is a _joint_ref.Puzzle with two more fields, ma [J] and mb [J]: of joint e's len(A[e]) rows of A only the ma[e]
with the smallest (row minimum, row index) under the poses at hand count, of its rows of B the mb[e].
  * E_e = (sum of the kept A-row minima) / ma + (sum of the kept B-row minima) / mb;
  * a visit of piece p: the pairs of the kept rows of p's joints alone, weights 1 / ma and 1 / mb;
  * the candidate is taken iff E_p' < E_p, each with its own pose's kept sets.
With every count full this is _joint_ref, value for value.

  with_counts(P, ma, mb)           a Puzzle with counts
  joint_energy(P, G, e)            -> JointEnergy(E, c1, c2, kept_a, kept_b, margin, keep_margin)
  piece_energy(P, G, p)            E_p, {e: JointEnergy}
  total(P, G)                      E(G) and every E_e
  visit(P, G, p) / visit_f32(...)  the candidate of a visit in float64 / the float32 yardstick of the device's visit
  refine(P, sweeps)                the loop -> TrimRefined
  objective_interval2(...)         the interval that must hold the kernel's float32 E_e (trimmed form)
  partial_puzzle(...)              K pieces whose joints' sets mate along a share of their rows only
  mating_only(P, mating)           the same puzzle cut to its true mating rows: the oracle's input
"""
import collections

import numpy as np

from tests import _icp_ref as ref
from tests import _icp_trim_ref as tr
from tests import _joint_ref as jr

TrimPuzzle = collections.namedtuple("TrimPuzzle", jr.Puzzle._fields + ("ma", "mb"))
JointEnergy = collections.namedtuple("JointEnergy", "E c1 c2 kept_a kept_b margin keep_margin")
TrimRefined = collections.namedtuple(
    "TrimRefined", "G score score0 sweeps_used accepted margin_ratio keep_ratio scores kept_a kept_b joint_score")


def with_counts(P, ma=None, mb=None):
    """P with the counts ma [J], mb [J] (None: every row of that side)."""
    ma = [len(A) for A in P.A] if ma is None else [int(m) for m in ma]
    mb = [len(B) for B in P.B] if mb is None else [int(m) for m in mb]
    assert all(1 <= m <= len(A) for m, A in zip(ma, P.A)) and all(1 <= m <= len(B) for m, B in zip(mb, P.B))
    return TrimPuzzle(*P[:len(jr.Puzzle._fields)], ma, mb)


def joint_energy(P, G, e):
    D = jr._D(P, G, e)
    c1, c2 = D.argmin(axis=1), D.argmin(axis=0)
    r1, r2 = D.min(axis=1), D.min(axis=0)
    ka_, kb_ = tr.kept_rows(r1, P.ma[e]), tr.kept_rows(r2, P.mb[e])
    E = r1[ka_].mean() + r2[kb_].mean()
    return JointEnergy(float(E), c1, c2, ka_, kb_, min(ref._margin(D, 1), ref._margin(D, 0)),
                       min(tr._keep_margin(r1, P.ma[e]), tr._keep_margin(r2, P.mb[e])))


def piece_energy(P, G, p):
    """-> (E_p, {e: JointEnergy}) over the joints incident to p, in list order."""
    E, each = 0.0, {}
    for e in jr.incident(P, p):
        each[e] = joint_energy(P, G, e)
        E += each[e].E
    return E, each


def total(P, G):
    each = [joint_energy(P, G, e).E for e in range(len(P.joints))]
    return float(sum(each)), each


def _pairs(P, G, p, each, dtype):
    """The pairs of a visit -> x [n,3] in p's frame, y [n,3] in the root frame, w [n]: per joint the kept rows of A (weight
    1 / ma) then the kept rows of B (weight 1 / mb), each ascending, joints in list order."""
    xs, ys, ws = [], [], []
    for e in jr.incident(P, p):
        i, j = P.joints[e]
        a, b = np.asarray(P.A[e], dtype=dtype), np.asarray(P.B[e], dtype=dtype)
        o = each[e]
        pa, pb = np.concatenate((a[o.kept_a], a[o.c2[o.kept_b]])), np.concatenate((b[o.c1[o.kept_a]], b[o.kept_b]))
        w = np.concatenate((np.full(len(o.kept_a), 1.0 / len(o.kept_a)), np.full(len(o.kept_b), 1.0 / len(o.kept_b)))).astype(dtype)
        if i == p:
            far = np.asarray(G[j], dtype=dtype)
            xs.append(pa), ys.append(pb @ far[:3, :3].T + far[:3, 3])
        else:
            far = np.asarray(G[i], dtype=dtype)
            xs.append(pb), ys.append(pa @ far[:3, :3].T + far[:3, 3])
        ws.append(w)
    return np.concatenate(xs), np.concatenate(ys), np.concatenate(ws)


def visit(P, G, p, each=None, round32=True):
    """_joint_ref.visit over the kept pairs (each: piece_energy's, found under G when None)."""
    if each is None:
        each = piece_energy(P, G, p)[1]
    x, y, w = _pairs(P, G, p, each, np.float64)
    W = w.sum()
    xc, yc = (w[:, None] * x).sum(axis=0) / W, (w[:, None] * y).sum(axis=0) / W
    xd, yd = x - xc, y - yc
    if ref.is_degenerate((w[:, None] * xd).T @ xd):
        R = np.asarray(G[p], dtype=np.float64)[:3, :3].copy()
    else:
        R = ref._kabsch((w[:, None] * xd).T @ yd)
    out = ref.rigid(R, yc - R @ xc)
    return jr.f32(out) if round32 else out


def visit_f32(P, G, p, each):
    """_joint_ref.visit_f32 over the kept pairs: plain float32 with sequential sums -> [4,4] float32."""
    x, y, w = _pairs(P, G, p, each, np.float32)
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


def objective_interval2(a, b, Gi, Gj, ma, mb):
    """[lo, hi] that must hold the kernel's float32 E_e: _icp_trim_ref.objective_interval's part() over
    _joint_ref.distance_bound2 - the m smallest lower ends bound the sum of the kept minima from below and the m smallest
    upper ends from above, whichever rows the kernel kept."""
    D = ref.sqdist(ref.transform(Gi, a), ref.transform(Gj, b))
    Bd = jr.distance_bound2(a, b, Gi, Gj)

    def part(lo, hi, m):
        return np.sort(np.maximum(lo, 0.0))[:m].mean(), np.sort(hi)[:m].mean()
    lo1, hi1 = part((D - Bd).min(axis=1), (D + Bd).min(axis=1), ma)
    lo2, hi2 = part((D - Bd).min(axis=0), (D + Bd).min(axis=0), mb)
    g = ref._gamma(max(D.shape) + 2)
    return (lo1 + lo2) * (1.0 - g), (hi1 + hi2) * (1.0 + g)


def joint_intervals(P, G, joints=None):
    """-> [J, 2]: objective_interval2 of every joint (or the listed ones, NaN elsewhere) under G."""
    out = np.full((len(P.joints), 2), np.nan)
    for e in (range(len(P.joints)) if joints is None else joints):
        i, j = P.joints[e]
        out[e] = objective_interval2(P.A[e], P.B[e], G[i], G[j], P.ma[e], P.mb[e])
    return out


def refine(P, sweeps):
    """The loop of pzn_joint_refine_trim_f32 in float64 (poses are float32 VALUES, evaluated in float64) -> TrimRefined:
    _joint_ref.refine's fields; keep_ratio = the smallest keep margin met at any pose that was evaluated, in units of the
    joint's nearest_bound2 under G0, as margin_ratio is for the nearest-neighbour margins (over ALL rows, kept or not);
    kept_a / kept_b [J] = the rows kept under the returned poses, joint_score [J] = E_e under them."""
    G = jr.f32(P.G0).copy()
    scale = jr.nearest_bounds(P, G)
    J = len(P.joints)
    ratio = keep_ratio = np.inf

    def note(each):
        nonlocal ratio, keep_ratio
        ratio = min([ratio] + [o.margin / scale[e] for e, o in each.items()])
        keep_ratio = min([keep_ratio] + [o.keep_margin / scale[e] for e, o in each.items()])

    start = {e: joint_energy(P, G, e) for e in range(J)}
    note(start)
    E0 = float(sum(start[e].E for e in range(J)))
    accepted = np.zeros(P.K, dtype=np.int64)
    used, scores = 0, [E0]
    for _ in range(int(sweeps)):
        any_taken = False
        for p in range(P.K):
            if not jr.has_joint(P, p):
                continue
            Ep, each = piece_energy(P, G, p)
            note(each)
            Gn = G.copy()
            Gn[p] = visit(P, G, p, each)
            En, each_n = piece_energy(P, Gn, p)
            note(each_n)
            if En < Ep:
                G, any_taken = Gn, True
                accepted[p] += 1
        if not any_taken:
            break
        used += 1
        scores.append(total(P, G)[0])
    end = [joint_energy(P, G, e) for e in range(J)]
    note(dict(enumerate(end)))
    return TrimRefined(G, float(sum(o.E for o in end)), E0, used, accepted, ratio, keep_ratio, scores,
                       [o.kept_a for o in end], [o.kept_b for o in end], [o.E for o in end])


# --------------------------------------------------------------------------- inputs

def partial_puzzle(rng, K, joints, k, share, same=False, noise=0.003, angle=np.deg2rad(4.0), shift=0.01, movable=None, n_mate=None,
                   quick=False):
    """_joint_ref.puzzle for pieces with several faces: of the k rows of BOTH sets of joint e only n = round(share k) (or
    n_mate[e]) lie on the joint's shared curve - piece i's sampling of it and piece j's, each with its own noise; same=True:
    B's mating rows are A's in another order -, the other k - n lie on an unrelated curve placed by
    _icp_trim_ref._other_curve, OTHER_GAP away from the shared curve (the faces towards other neighbours); B's other curve
    is held that far from A's other rows as well, as two solid pieces do not run through each other next to their contact.
    quick=True (the small sets of the kernel tests' families, where no search is needed): the mating rows are one draw per
    n-th of the curve (a row's neighbours stay a fraction of 1 / n of the curve away, so no two candidates tie), and the
    other rows lie on curves of 0.6 of the size centred 1.2 + OTHER_GAP from the shared curve's centre on opposite sides of
    it: the shared curve stays within 0.55 of its centre and such a curve within 0.35 of its own, so they are at least
    OTHER_GAP apart without _other_curve's bisection.
    All rows of a set in one random order.  True poses, start poses and movable as _joint_ref.puzzle (the centre of a piece's
    perturbation is the mean of all its rows) -> (Puzzle, mating_a [J] bool [k], mating_b [J] bool [k])."""
    truth = np.stack([ref.rigid(ref.rot(rng.normal(size=3), rng.uniform(0.3, 2.5)), rng.uniform(-0.3, 0.3, 3)) for _ in range(K)])
    A, B, mates_a, mates_b, centre, count = [], [], [], [], np.zeros((K, 3)), np.zeros(K)
    for e, (i, j) in enumerate(joints):
        n = int(round(share * k)) if n_mate is None else int(n_mate[e])
        W = ref.rot(rng.normal(size=3), rng.uniform(0, np.pi))
        place = rng.uniform(-0.5, 0.5, 3)
        planar = bool(e & 1)
        dense = ref.curve(np.linspace(0, 1, 400, endpoint=False), planar) @ W.T + place
        draw = (lambda: (np.arange(n) + rng.uniform(0.2, 0.8, n)) / n) if quick else (lambda: rng.uniform(0, 1, n))
        ma_ = ref.curve(draw(), planar) @ W.T + place + rng.normal(scale=noise, size=(n, 3))
        if same:
            mb_ = ma_[rng.permutation(n)]
        else:
            mb_ = ref.curve(draw(), planar) @ W.T + place + rng.normal(scale=noise, size=(n, 3))
        if n == k:
            oa = ob = np.zeros((0, 3))
        elif quick:
            d = rng.normal(size=3)
            d /= np.linalg.norm(d)
            oa, ob = (0.6 * ref.curve(rng.uniform(0, 1, k - n), planar) @ ref.rot(rng.normal(size=3), rng.uniform(0, np.pi)).T
                      + dense.mean(axis=0) + s * (1.2 + rng.uniform(*tr.OTHER_GAP)) * d + rng.normal(scale=noise, size=(k - n, 3))
                      for s in (1.0, -1.0))
        else:
            oa = tr._other_curve(rng, k - n, W, dense.mean(axis=0), noise, planar, dense)
            ob = tr._other_curve(rng, k - n, W, dense.mean(axis=0), noise, planar, np.concatenate((dense, oa)))
        sets = []
        for mate, other in ((ma_, oa), (mb_, ob)):
            order = rng.permutation(k)
            sets.append((np.concatenate((mate, other))[order], (np.arange(k) < n)[order]))
        (ra, mating_a), (rb, mating_b) = sets
        A.append(ref.transform(jr._inverse(truth[i]), ra).astype(np.float32))
        B.append(ref.transform(jr._inverse(truth[j]), rb).astype(np.float32))
        mates_a.append(mating_a), mates_b.append(mating_b)
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
    P = jr.Puzzle(K, [tuple(x) for x in joints], A, B, G0.astype(np.float32), truth, np.asarray(movable, dtype=bool))
    return P, mates_a, mates_b


def mating_only(P, mating_a, mating_b):
    """P with every set cut to its true mating rows: what an oracle that knew the contact would refine over."""
    return jr.Puzzle(P.K, P.joints, [A[m] for A, m in zip(P.A, mating_a)], [B[m] for B, m in zip(P.B, mating_b)], P.G0, P.truth,
                     P.movable)
