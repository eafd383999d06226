"""Float64 NumPy statement of the joint refinement that finds the kept counts of every joint under the joint poses
(ops.joint_refine(..., auto=(lo_a, lo_b, power)); csrc/jointauto.hip, joint_auto_kernel; the contract is in include/pzn.h),
built on tests/_joint_trim_ref.py (the energies at given counts, the puzzles) and tests/_icp_auto_ref.py (counts, phi, the
exact-integer count), and the case families its CPU and GPU tests share.  Nothing here is tuned to the kernel.

An AutoPuzzle is a _joint_ref.Puzzle with three more fields, lo_a, lo_b and power.  Every evaluation of joint e under poses G:
  * the row minima of both directions, then per direction _icp_auto_ref.counts: the m in [lo, k] of smallest
    phi(m) = (sum of the m smallest minima) / m^(power + 1), the largest m among equal phi;
  * kept rows, E_e = e_a + e_b: _joint_trim_ref.joint_energy at those counts;
  * F_e = e_a (ka / m_a)^power + e_b (kb / m_b)^power;
  * a visit of piece p: the kept pairs of p's joints, weights (ka / m_a)^power / m_a and (kb / m_b)^power / m_b;
  * the candidate is taken iff F_p' < F_p, each with its own pose's counts and kept sets.
With lo = (ka, kb) this is _joint_trim_ref at full counts, value for value.

  with_auto(P, lo_a, lo_b, power)   a Puzzle with the rule's three numbers
  joint_energy(P, G, e)             -> AutoEnergy
  piece_energy(P, G, p), total(P, G)
  visit(P, G, p) / visit_f32(...)   the candidate of a visit in float64 / the float32 yardstick of the device's visit
  refine(P, sweeps)                 the loop -> AutoJointRefined
  lattice_joint(P, e)               counts and kept rows of a lattice puzzle's joint under G0 from integers alone
  objective_interval2(...)          the interval that must hold the kernel's float32 F_e where its counts are decided
  share_puzzle(...), share_variants(P, ...)   "does the rule help": the four refinements of a puzzle with a share per joint
  visit_cases / trajectory_cases, visit_row / trajectory_row   the families of the float64 comparisons
"""
import collections

import numpy as np

from tests import _icp_auto_ref as au
from tests import _icp_ref as ref
from tests import _joint_ref as jr
from tests import _joint_trim as jm
from tests import _joint_trim_ref as jt

AutoPuzzle = collections.namedtuple("AutoPuzzle", jr.Puzzle._fields + ("lo_a", "lo_b", "power"))
AutoEnergy = collections.namedtuple("AutoEnergy", "F E c1 c2 kept_a kept_b m_a m_b w_a w_b margin keep_margin count_margin")
AutoJointRefined = collections.namedtuple(
    "AutoJointRefined", "G score score0 objective objective0 sweeps_used accepted margin_ratio keep_ratio count_room objectives "
                        "kept_a kept_b count_a count_b joint_score")

N_BASE = len(jr.Puzzle._fields)


def with_auto(P, lo_a, lo_b, power):
    assert 1 <= lo_a <= min(len(A) for A in P.A) and 1 <= lo_b <= min(len(B) for B in P.B) and 1 <= power <= 4
    return AutoPuzzle(*P[:N_BASE], int(lo_a), int(lo_b), int(power))


def with_least(P, least=au.LEAST, power=au.POWER):
    """The least counts of a share by assembly._keep_counts' ceil rule (all sets of a side have one size)."""
    return with_auto(P, au.least_count(len(P.A[0]), least), au.least_count(len(P.B[0]), least), power)


def _at(P, e, m_a, m_b):
    """P as a TrimPuzzle whose joint e has the counts (m_a, m_b) (the other joints' counts are not read)."""
    ma, mb = [len(A) for A in P.A], [len(B) for B in P.B]
    ma[e], mb[e] = m_a, m_b
    return jt.TrimPuzzle(*P[:N_BASE], ma, mb)


def joint_energy(P, G, e):
    D = jr._D(P, G, e)
    r1, r2 = D.min(axis=1), D.min(axis=0)
    m_a, m_b = au.counts(r1, P.lo_a, P.power), au.counts(r2, P.lo_b, P.power)
    o = jt.joint_energy(_at(P, e, m_a, m_b), G, e)
    ra, rb = (r1.shape[0] / m_a) ** P.power, (r2.shape[0] / m_b) ** P.power
    F = r1[o.kept_a].mean() * ra + r2[o.kept_b].mean() * rb
    return AutoEnergy(float(F), o.E, o.c1, o.c2, o.kept_a, o.kept_b, m_a, m_b, ra / m_a, rb / m_b, o.margin, o.keep_margin,
                      min(au.count_margin(r1, P.lo_a, P.power), au.count_margin(r2, P.lo_b, P.power)))


def piece_energy(P, G, p):
    """-> (F_p, {e: AutoEnergy}) over the joints incident to p, in list order."""
    F, each = 0.0, {}
    for e in jr.incident(P, p):
        each[e] = joint_energy(P, G, e)
        F += each[e].F
    return F, each


def total(P, G):
    """-> (F, E, every AutoEnergy)."""
    each = [joint_energy(P, G, e) for e in range(len(P.joints))]
    return float(sum(o.F for o in each)), float(sum(o.E for o in each)), each


def _pairs(P, G, p, each, dtype):
    """_joint_trim_ref._pairs with the rule's weights: per joint the kept rows of A (weight w_a) then the kept rows of B
    (weight w_b), each ascending, joints in list order."""
    xs, ys, ws = [], [], []
    for e in jr.incident(P, p):
        i, j = P.joints[e]
        a, b = np.asarray(P.A[e], dtype=dtype), np.asarray(P.B[e], dtype=dtype)
        o = each[e]
        pa, pb = np.concatenate((a[o.kept_a], a[o.c2[o.kept_b]])), np.concatenate((b[o.c1[o.kept_a]], b[o.kept_b]))
        w = np.concatenate((np.full(len(o.kept_a), o.w_a), np.full(len(o.kept_b), o.w_b))).astype(dtype)
        if i == p:
            far = np.asarray(G[j], dtype=dtype)
            xs.append(pa), ys.append(pb @ far[:3, :3].T + far[:3, 3])
        else:
            far = np.asarray(G[i], dtype=dtype)
            xs.append(pb), ys.append(pa @ far[:3, :3].T + far[:3, 3])
        ws.append(w)
    return np.concatenate(xs), np.concatenate(ys), np.concatenate(ws)


def visit(P, G, p, each=None, round32=True):
    """_joint_trim_ref.visit over the kept pairs with the rule's weights."""
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
    """_joint_trim_ref.visit_f32 with the rule's weights: plain float32 with sequential sums -> [4,4] float32."""
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


def phi_slack2(a, b, Gi, Gj, lo_a, lo_b, power, factor=1.0):
    """_icp_auto_ref.phi_slack with both sides moved (_joint_ref.distance_bound2), every distance bound taken `factor` times:
    the relative gap of phi below which float32 arithmetic off by that many bounds may decide a count otherwise."""
    D = ref.sqdist(ref.transform(Gi, a), ref.transform(Gj, b))
    Bd = factor * jr.distance_bound2(a, b, Gi, Gj)
    worst = 0.0
    for axis, lo in ((1, lo_a), (0, lo_b)):
        mid = np.cumsum(np.sort(D.min(axis=axis)))
        low = np.cumsum(np.sort(np.maximum((D - Bd).min(axis=axis), 0.0)))
        high = np.cumsum(np.sort((D + Bd).min(axis=axis)))
        g = ref._gamma(np.arange(1, mid.shape[0] + 1) + 1)
        with np.errstate(divide="ignore", invalid="ignore"):
            rho = np.maximum(high * (1.0 + g) - mid, mid - low * (1.0 - g)) / mid
        rho = np.where(mid > 0.0, rho, np.inf)[lo - 1:]
        if rho.size > 1:      # (a single candidate cannot be overtaken)
            worst = max(worst, float(rho.max()))
    return 2.0 * worst / (1.0 + worst) if np.isfinite(worst) else 1.0


def count_room(P, G, e, o, factor=jm.MARGIN_FACTOR):
    """The count margin of joint e under G minus what float32 off by `factor` distance bounds may do to it: the counts are
    decided with a margin where this is positive."""
    i, j = P.joints[e]
    return o.count_margin - phi_slack2(P.A[e], P.B[e], G[i], G[j], P.lo_a, P.lo_b, P.power, factor)


def refine(P, sweeps):
    """The loop of pzn_joint_refine_auto_f32 in float64 (poses are float32 VALUES, evaluated in float64) -> AutoJointRefined:
    margin_ratio / keep_ratio as _joint_trim_ref.refine's, count_room the smallest count_room met at any pose that was
    evaluated, objectives = F after every sweep that took something; kept_*, count_*, joint_score (E_e) under the returned
    poses."""
    G = jr.f32(P.G0).copy()
    scale = jr.nearest_bounds(P, G)
    J = len(P.joints)
    ratio = keep_ratio = room = np.inf

    def note(each, at):
        nonlocal ratio, keep_ratio, room
        ratio = min([ratio] + [o.margin / scale[e] for e, o in each.items()])
        keep_ratio = min([keep_ratio] + [o.keep_margin / scale[e] for e, o in each.items()])
        room = min([room] + [count_room(P, at, e, o) for e, o in each.items()])

    start = {e: joint_energy(P, G, e) for e in range(J)}
    note(start, G)
    F0, E0 = float(sum(o.F for o in start.values())), float(sum(o.E for o in start.values()))
    accepted = np.zeros(P.K, dtype=np.int64)
    used, Fs = 0, [F0]
    for _ in range(int(sweeps)):
        any_taken = False
        for p in range(P.K):
            if not jr.has_joint(P, p):
                continue
            Fp, each = piece_energy(P, G, p)
            note(each, G)
            Gn = G.copy()
            Gn[p] = visit(P, G, p, each)
            Fn, each_n = piece_energy(P, Gn, p)
            note(each_n, Gn)
            if Fn < Fp:
                G, any_taken = Gn, True
                accepted[p] += 1
        if not any_taken:
            break
        used += 1
        Fs.append(total(P, G)[0])
    end = [joint_energy(P, G, e) for e in range(J)]
    note(dict(enumerate(end)), G)
    return AutoJointRefined(G, float(sum(o.E for o in end)), E0, float(sum(o.F for o in end)), F0, used, accepted, ratio, keep_ratio,
                            room, Fs, [o.kept_a for o in end], [o.kept_b for o in end], [o.m_a for o in end], [o.m_b for o in end],
                            [o.E for o in end])


# --------------------------------------------------------------------------- the exact-integer form

def lattice_joint(P, e, lo_a, lo_b, power):
    """Joint e of a _joint_trim.lattice_puzzle under G0: every squared distance is a small integer, so the counts follow from
    _icp_auto_ref.lattice_count (cross-multiplied Python ints) and the kept rows from a stable sort of integers ->
    dict(count_a, count_b, kept_a, kept_b, how_a, how_b, tied): tied = row minima of a direction that repeat."""
    D = jr._D(P, np.asarray(P.G0, dtype=np.float64), e)
    Di = np.rint(D).astype(np.int64)
    assert np.array_equal(Di.astype(np.float64), D)
    out = {"tied": 0}
    for name, minima, lo in (("a", Di.min(axis=1), lo_a), ("b", Di.min(axis=0), lo_b)):
        assert int(minima.sum()) < 2 ** 24      # every float32 sum of the kernel is exact
        m, how = au.lattice_count(minima, lo, power)
        out["count_" + name], out["how_" + name] = m, how
        out["kept_" + name] = np.sort(np.argsort(minima, kind="stable")[:m])
        out["tied"] += len(minima) - len(set(minima.tolist()))
    return out


# --------------------------------------------------------------------------- the float32 interval of F_e

def objective_interval2(a, b, Gi, Gj, m_a, m_b, power):
    """[lo, hi] that must hold the kernel's float32 F_e where its counts are (m_a, m_b): _joint_trim_ref.objective_interval2's
    two halves, each times r = (k / m)^power; the cast of r, the two products and the sum are four more roundings."""
    D = ref.sqdist(ref.transform(Gi, a), ref.transform(Gj, b))
    Bd = jr.distance_bound2(a, b, Gi, Gj)

    def part(lo, hi, m):
        return np.sort(np.maximum(lo, 0.0))[:m].mean(), np.sort(hi)[:m].mean()
    lo1, hi1 = part((D - Bd).min(axis=1), (D + Bd).min(axis=1), m_a)
    lo2, hi2 = part((D - Bd).min(axis=0), (D + Bd).min(axis=0), m_b)
    ra, rb = (D.shape[0] / m_a) ** power, (D.shape[1] / m_b) ** power
    g = ref._gamma(max(D.shape) + 6)
    return (lo1 * ra + lo2 * rb) * (1.0 - g), (hi1 * ra + hi2 * rb) * (1.0 + g)


def joint_intervals(P, G, each):
    """-> {e: [lo, hi]} for the joints of `each` ({e: AutoEnergy} under G)."""
    return {e: objective_interval2(P.A[e], P.B[e], G[P.joints[e][0]], G[P.joints[e][1]], o.m_a, o.m_b, P.power) for e, o in each.items()}


# --------------------------------------------------------------------------- does the rule help?

SHARE_GRAPHS = ["ring4", "complete5"]
SHARE_CASES, SHARE_K, SHARE_SWEEPS, SHARE_SEED = 6, 24, 30, 9100


def share_puzzle(rng, graph, k=SHARE_K):
    """A _joint_trim_ref.partial_puzzle whose joints each draw their true share from _icp_auto_ref.SHARES; the first joint's is
    drawn from the shares <= 0.5, so at least one joint mates along half of its rows or fewer -> (Puzzle, mating_a, mating_b,
    shares [J])."""
    K, joints = jr.GRAPHS[graph]
    shares = rng.choice(au.SHARES, size=len(joints))
    shares[0] = rng.choice([s for s in au.SHARES if s <= 0.5])
    P, ma, mb = jt.partial_puzzle(rng, K, joints, k, None, n_mate=[int(round(s * k)) for s in shares], quick=True)
    return P, ma, mb, shares


def share_cases(graph):
    rng = np.random.default_rng(SHARE_SEED + SHARE_GRAPHS.index(graph))
    return [share_puzzle(rng, graph) for _ in range(SHARE_CASES)]


def _error(G, P):
    return float(jr.pose_error(G, P.truth)[1:].mean())


def share_variants(case, sweeps=SHARE_SWEEPS):
    """The mean pose error against the truth (over the pieces that may move) of four refinements of one case ->
    (a) untrimmed, (b) one share for all joints - the mean true share -, (c) the auto rule with AutoKeep()'s defaults,
    (d) the oracle: the untrimmed refinement over the true mating rows alone."""
    P, mating_a, mating_b, shares = case
    k = len(P.A[0])
    m = au.least_count(k, float(np.mean(shares)))
    J = len(P.joints)
    a = jt.refine(jt.with_counts(P), sweeps).G
    b = jt.refine(jt.with_counts(P, [m] * J, [m] * J), sweeps).G
    c = refine(with_least(P), sweeps).G
    d = jt.refine(jt.with_counts(jt.mating_only(P, mating_a, mating_b)), sweeps).G
    return tuple(_error(G, P) for G in (a, b, c, d))


# --------------------------------------------------------------------------- the families of the float64 comparisons

VISIT_CASES, VISIT_K = 16, 9
TRAJECTORY_CASES, TRAJECTORY_SWEEPS, TRAJECTORY_K = 16, 3, 8
# chosen on the CPU among eight candidates each, by the float64 statement alone: the seeds under which every graph leaves out
# at most one case in eight
VISIT_SEED, TRAJECTORY_SEED = 9328, 9428
# graph -> cases of visit_cases(graph) that do not enter: at most 2 of 16 each (one in eight); asserted from the statement
# alone on the CPU (tests/test_joint_auto_cpu.py), and the GPU test leaves out no more
VISIT = {"chain3": 0, "ring4": 0, "both3": 0, "complete5": 0}
# graph -> cases of trajectory_cases(graph) that the float64 loop leaves out: at most 2 of 16 each (the same two test files)
TRAJECTORY = {"pair": 0, "chain3": 1, "ring4": 0, "both3": 1, "complete5": 2}


def _family(graph, seed, n_cases, k, same, movable):
    """tests/_joint_trim._family's puzzles - per joint n mating rows drawn from (k + 1) // 2 .. k and k - n rows on other faces
    - with the rule's defaults in place of given counts."""
    K, joints = jr.GRAPHS[graph]
    rng = np.random.default_rng(seed + jm.GRAPHS.index(graph))
    out = []
    for _ in range(n_cases):
        n = rng.integers((k + 1) // 2, k + 1, size=len(joints))
        P, _, _ = jt.partial_puzzle(rng, K, joints, k, None, same=same, n_mate=n, movable=movable(K), quick=True)
        out.append(with_least(P))
    return out


def trajectory_cases(graph):
    """k = 8, every piece but the root movable; the two sides of a joint are two samplings of the shared curve with their own
    noise (with B's mating rows copies of A's the minima fall to zero along a run and no relative margin of phi survives)."""
    return _family(graph, TRAJECTORY_SEED, TRAJECTORY_CASES, TRAJECTORY_K, False, lambda K: None)


def visit_cases(graph):
    """k = 9 (the scan's tail loop, rows no multiple of four), only piece 1 movable."""
    return _family(graph, VISIT_SEED, VISIT_CASES, VISIT_K, False, lambda K: np.arange(K) == 1)


def trajectory_row(P):
    """-> (the float64 loop's AutoJointRefined, entered): a case enters where every nearest-neighbour margin and every keep
    margin met at a pose the loop evaluated exceeds MARGIN_FACTOR nearest_bound2, and every count met was decided with room."""
    want = refine(P, TRAJECTORY_SWEEPS)
    return want, bool(want.margin_ratio >= jm.MARGIN_FACTOR and want.keep_ratio >= jm.MARGIN_FACTOR and want.count_room > 0.0)


def visit_row(P):
    """The float64 side of one visit of piece 1 under G0 -> (want [4,4] float64 not rounded, yardstick error = visit_f32 against
    it, entered, gap, {e: AutoEnergy} under the candidate).  tests/_joint_trim.visit_row's rule with the count margins beside
    the keep and nearest-neighbour margins, under G0 and under the candidate, and the intervals of F: float64 says the
    candidate lowers F_p beyond the rounding intervals of both sums."""
    g0 = jr.f32(P.G0)
    _, each = piece_energy(P, g0, 1)
    want = visit(P, g0, 1, each, round32=False)
    yard = ref.pose_err(visit_f32(P, P.G0, 1, each), want)
    x, y, w = _pairs(P, g0, 1, each, np.float64)
    xd, yd = x - (w[:, None] * x).sum(axis=0) / w.sum(), y - (w[:, None] * y).sum(axis=0) / w.sum()
    S = (w[:, None] * xd).T @ yd
    sv = np.linalg.svd(S, compute_uv=False)
    gap = float((sv[1] + np.sign(np.linalg.det(S)) * sv[2]) / sv[0])
    gn = g0.copy()
    gn[1] = jr.f32(want)
    _, each_n = piece_energy(P, gn, 1)
    scale = {e: jr.nearest_bound2(P.A[e], P.B[e], g0[P.joints[e][0]], g0[P.joints[e][1]]) for e in each}
    entered = gap >= jm.GAP_MIN
    for g, ea in ((g0, each), (gn, each_n)):
        entered = entered and all(min(o.margin, o.keep_margin) > jm.MARGIN_FACTOR * scale[e] and count_room(P, g, e, o) > 0.0
                                  for e, o in ea.items())
    if entered:
        iv0 = np.array(list(joint_intervals(P, g0, each).values()))
        iv1 = np.array(list(joint_intervals(P, gn, each_n).values()))
        entered = jr.sum_interval(iv1)[1] < jr.sum_interval(iv0)[0]
    return want, yard, bool(entered), gap, each_n
