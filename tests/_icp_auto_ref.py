"""Float64 NumPy statement of the pose refinement with the overlap share found per pair (ops.icp_refine(..., auto=(lo_a,
lo_b, power)); csrc/icprefine.hip, icp_auto_kernel; the contract is in include/pzn.h), on top of tests/_icp_trim_ref.py.
Nothing here is tuned to the kernel.

The rule, for least counts 1 <= lo_a <= ka, 1 <= lo_b <= kb and an integer power p in [1, 4], per EVALUATION of a pose:
  * one direction with n row minima: sorted, w_1 <= ... <= w_n, prefix sums S_m, phi(m) = S_m / m^(p+1);
  * count: the m in [lo, n] with the smallest phi, among equal phi the largest m (all minima zero: every row);
  * kept set, e_a, e_b, score = e_a + e_b: _icp_trim_ref's at those counts;
  * objective F = e_a (ka / m_a)^p + e_b (kb / m_b)^p (= n^p phi(m) per direction);
  * step: _icp_trim_ref.step over the kept pairs of the current pose; the candidate is taken iff F' < F.
lo = (ka, kb) is _icp_trim_ref.refine with every row kept, value for value.

  phi(minima, power)                   phi(m) for m = 1 .. n as an array ([m - 1])
  counts(minima, lo, power)            m*
  count_margin(minima, lo, power)      the relative gap between the best phi and the best phi of any OTHER m
  objective(a, b, T, lo_a, lo_b, power)  -> Objective
  refine(a, b, T0, iters, lo_a, lo_b, power)  the loop -> Auto
  phi_slack(a, b, T, lo_a, lo_b, power)  what float32 arithmetic may do to a count (compare count_margin with it)
"""
import collections

import numpy as np

from tests import _icp_ref as ref
from tests import _icp_trim_ref as trim

Objective = collections.namedtuple("Objective", "F E c1 c2 kept_a kept_b m_a m_b margin keep_margin count_margin")
Auto = collections.namedtuple("Auto", "T score score0 objective objective0 iters_used m_a m_b kept_a kept_b c1 c2 margin keep_margin "
                                      "count_room objectives")


def phi(minima, power):
    """phi(m) = (sum of the m smallest minima) / m^(power + 1), m = 1 .. n -> [n] float64."""
    w = np.sort(np.asarray(minima, dtype=np.float64))
    m = np.arange(1, w.shape[0] + 1, dtype=np.float64)
    return np.cumsum(w) / m ** (int(power) + 1)


def _best(f, lo):
    """The m in [lo, n] of smallest f[m - 1], the largest among equal ones."""
    n = f.shape[0]
    tail = f[lo - 1:]
    return int(lo + (n - lo) - np.argmin(tail[::-1]))      # argmin of the reversed tail: the LAST smallest


def counts(minima, lo, power):
    return _best(phi(minima, power), int(lo))


def count_margin(minima, lo, power):
    """1 - phi(m*) / (the smallest phi of any other m in [lo, n]): 0 on a tie, inf where m* is the only candidate or every
    other phi is +inf."""
    f = phi(minima, power)
    m = _best(f, int(lo))
    others = np.delete(f[lo - 1:], m - lo)
    if others.size == 0 or not np.isfinite(others.min()):
        return np.inf
    second = float(others.min())
    return 0.0 if second == 0.0 else 1.0 - float(f[m - 1]) / second


def objective(a, b, T, lo_a, lo_b, power):
    """-> Objective: the counts m_a, m_b of the pose, then everything _icp_trim_ref.objective gives at them (E, arg-mins,
    kept sets, margins), F, and count_margin = the smaller of the two directions'."""
    D = ref.sqdist(a, ref.transform(T, b))
    r1, r2 = D.min(axis=1), D.min(axis=0)
    m_a, m_b = counts(r1, lo_a, power), counts(r2, lo_b, power)
    o = trim.objective(a, b, T, m_a, m_b)
    e_a, e_b = r1[o.kept_a].mean(), r2[o.kept_b].mean()
    F = e_a * (r1.shape[0] / m_a) ** power + e_b * (r2.shape[0] / m_b) ** power
    return Objective(float(F), o.E, o.c1, o.c2, o.kept_a, o.kept_b, m_a, m_b, o.margin, o.keep_margin,
                     min(count_margin(r1, lo_a, power), count_margin(r2, lo_b, power)))


def phi_slack(a, b, T, lo_a, lo_b, power):
    """What float32 may do to a count, as _icp_trim_ref.kept_slack / objective_interval are built: every float32 row minimum
    lies in [min (d - B), min (d + B)] (B = _icp_ref.distance_bound); the sum of the m smallest of n values is monotone in
    every one of them, so the prefix sums of the sorted lower ends bound the float32 S_m from below and those of the sorted
    upper ends from above, whichever order the float32 values stand in; a float32 sum of m non-negative terms in ANY order
    is off by a factor within 1 -+ gamma_m; the float64 power is exact and the float64 division is off by 2^-53 (taken as
    one more unit of gamma).  With rho = the largest relative half-width of phi32(m) about phi(m) over the candidates m of a
    direction, another m can overtake m* only if 1 - phi(m*) / phi(m) <= 2 rho / (1 + rho): that number, the larger of the
    two directions', is returned; a count is decided where count_margin exceeds it."""
    D = ref.sqdist(a, ref.transform(T, b))
    Bd = ref.distance_bound(a, b, T)
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


def refine(a, b, T0, iters, lo_a, lo_b, power):
    """The loop of pzn_icp_refine_auto_f32 in float64 (poses are float32 VALUES, as in _icp_ref.refine) -> Auto: m_*, kept_*,
    c1 / c2 are the RETURNED pose's; margin / keep_margin the smallest met at any evaluated pose; count_room the smallest
    (count_margin - phi_slack) met at any evaluated pose; objectives = F after every accepted step."""
    T = np.asarray(T0, dtype=np.float32).astype(np.float64)
    o = objective(a, b, T, lo_a, lo_b, power)
    first, used, Fs = o, 0, [o.F]
    margin, keep_margin = o.margin, o.keep_margin
    room = o.count_margin - phi_slack(a, b, T, lo_a, lo_b, power)
    for _ in range(int(iters)):
        cand = trim.step(a, b, o.c1, o.c2, o.kept_a, o.kept_b, T, round32=True)
        n = objective(a, b, cand, lo_a, lo_b, power)
        margin, keep_margin = min(margin, n.margin), min(keep_margin, n.keep_margin)
        room = min(room, n.count_margin - phi_slack(a, b, cand, lo_a, lo_b, power))
        if not n.F < o.F:
            break
        T, o, used = cand, n, used + 1
        Fs.append(o.F)
    return Auto(T, o.E, first.E, o.F, first.F, used, o.m_a, o.m_b, o.kept_a, o.kept_b, o.c1, o.c2, margin, keep_margin, room, Fs)


# --------------------------------------------------------------------------- the cases the CPU and the GPU tests share

LEAST, POWER = 0.25, 3      # the defaults of assembly.AutoKeep
SHARES = (0.3, 0.5, 0.75, 1.0)
# (ka, kb, P) of the float64 comparison of tests/test_gpu_icp_auto.py: odd sizes with ka != kb, one row per thread on one
# side, several rows per thread, the LDS limit
FLOAT64_SHAPES = [(37, 29, 8), (64, 64, 8), (300, 70, 4), (1024, 1024, 2)]
TRAJECTORY_K, TRAJECTORY_P, TRAJECTORY_SEED = 24, 32, 7300
MARGIN_FACTOR = 16.0        # tests/test_gpu_icp_trim.py's: margins are held to this many nearest-neighbour distance bounds


def least_count(k, least=LEAST):
    """assembly._keep_counts' ceil rule, restated."""
    return min(k, max(1, int(np.ceil(least * k - 1e-9))))


def float64_cases(shape):
    ka, kb, P = shape
    rng = np.random.default_rng(61000 + 7 * ka + 3 * kb + P)
    return [trim.partial_case(rng, ka, kb, SHARES[p % 4], planar=bool(p & 2)) for p in range(P)]


def count_decided(case, T, lo_a, lo_b, power):
    """Whether float32 arithmetic cannot change the counts and kept sets of `case` under T: the count margin exceeds
    phi_slack and the keep margin at the counts exceeds _icp_trim_ref.kept_slack."""
    o = objective(case.a, case.b, T, lo_a, lo_b, power)
    return o.count_margin > phi_slack(case.a, case.b, T, lo_a, lo_b, power) and o.keep_margin > trim.kept_slack(case.a, case.b, T)


def trajectory_cases():
    rng = np.random.default_rng(TRAJECTORY_SEED)
    k = TRAJECTORY_K
    return [trim.partial_case(rng, k, k, SHARES[p % 4], planar=bool(p & 2)) for p in range(TRAJECTORY_P)]


def trajectory_left_out(case, want):
    """The float64 loop `want` of `case` met a nearest-neighbour or keep margin under MARGIN_FACTOR distance bounds, or a
    count that float32 may decide otherwise: the device's loop is not held to it."""
    nb = ref.nearest_bound(case.a, case.b, case.T0)
    return want.margin < MARGIN_FACTOR * nb or want.keep_margin < MARGIN_FACTOR * nb or not want.count_room > 0.0


# Lattice clouds (tests/_lattice.py's idea): coordinates are multiples of 1 / 8 in [0, 1), the start pose translates by a
# lattice vector, so every moved coordinate, difference, square and sum below 2^24 units of 1 / 64 is exact in float32 and
# the kernel's counts follow from integers alone.
LATTICE_SHAPES = [(1, 1, 3), (37, 29, 6), (64, 64, 6), (300, 70, 4), (1024, 1024, 2), (8, 8, 513)]


def lattice_case(shape, seed=0):
    """-> (A [P,ka,3] f32, B [P,kb,3] f32, T0 [P,4,4] f32, ia, ib, it int64 in units of 1 / 8).  About half of b's rows are
    copies of rows of a moved back by the translation (minima 0 under T0), the rest random sites of a cube with about two
    sites per row, so the other minima are a few units."""
    ka, kb, P = shape
    rng = np.random.default_rng(8800 + 5 * ka + 3 * kb + P + seed)
    side = int(min(8, max(2, round((2.0 * max(ka, kb)) ** (1.0 / 3.0)))))
    ia = rng.integers(0, side, (P, ka, 3))
    it = rng.integers(-1, 2, (P, 3))
    it[0] = 0
    ib = rng.integers(0, side, (P, kb, 3))
    for p in range(P):
        n = int(rng.integers(0, kb + 1)) if p % 3 else kb // 2
        rows = rng.permutation(kb)[:n]
        ib[p, rows] = ia[p, rng.integers(0, ka, n)] - it[p]
    T0 = np.tile(np.eye(4, dtype=np.float32), (P, 1, 1))
    T0[:, :3, 3] = it / 8.0
    return (ia / 8.0).astype(np.float32), (ib / 8.0).astype(np.float32), T0, ia, ib, it


def _phi_less(S1, m1, S2, m2, power):
    """phi(m1) < phi(m2) by cross-multiplication in Python ints."""
    return int(S1) * int(m2) ** (power + 1) < int(S2) * int(m1) ** (power + 1)


def lattice_count(minima, lo, power):
    """One direction's count from integer minima -> (m*, how it was decided: "only" one candidate, a "tie" with another m,
    a "unit" gap - one unit less in a single minimum would let another m tie or win -, or "clear")."""
    w = np.sort(np.asarray(minima, dtype=np.int64), kind="stable")
    S = [int(v) for v in np.cumsum(w)]
    n = len(S)
    best = lo
    for m in range(lo + 1, n + 1):
        if not _phi_less(S[best - 1], best, S[m - 1], m, power):      # smaller or equal: the larger m
            best = m
    how = "only" if lo == n else "clear"
    for m in range(lo, n + 1):
        if m == best:
            continue
        if not _phi_less(S[best - 1], best, S[m - 1], m, power):
            return best, "tie"
        if not _phi_less(S[best - 1], best, S[m - 1] - 1, m, power):
            how = "unit"
    return best, how


def lattice_expected(ia, ib, it, lo_a, lo_b, power):
    """One problem under T0 from integers -> dict(count_a, count_b, kept_a, kept_b, score, objective, how_a, how_b): sums of
    integer minima (units of 1 / 64), then the rule's float32 roundings: e = S / m, r = (float)((double)(n / m)^p),
    F = e_a r_a + e_b r_b, every operation rounded once (NumPy's float32 scalars do that)."""
    d = ia[:, None, :] - (ib + it)[None, :, :]
    D = (d * d).sum(-1)
    out = {}
    e, r = [], []
    for name, minima, lo in (("a", D.min(axis=1), lo_a), ("b", D.min(axis=0), lo_b)):
        m, how = lattice_count(minima, lo, power)
        kept = np.sort(np.argsort(minima, kind="stable")[:m])
        total = int(minima[kept].sum())
        assert int(minima.sum()) < 2 ** 24      # every float32 sum of the kernel is exact
        e.append(np.float32(total / 64.0) / np.float32(m))
        q = np.float64(len(minima)) / np.float64(m)
        rp = q
        for _ in range(power - 1):
            rp = rp * q
        r.append(np.float32(rp))
        out["count_" + name], out["kept_" + name], out["how_" + name] = m, kept, how
    out["score"] = np.float32(e[0] + e[1])
    out["objective"] = np.float32(np.float32(e[0] * r[0]) + np.float32(e[1] * r[1]))
    return out
