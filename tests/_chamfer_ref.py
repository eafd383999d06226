"""Float64 NumPy restatement of ops.chamfer (csrc/chamfer.hip: chamfer_pack_kernel, chamfer_rowmin_kernel,
chamfer_bwd_kernel), the rounding bounds its float32 results are held to, and the inputs the chamfer tests share.  Nothing
here is tuned to the kernel: the truth is the DIFFERENCE form sum_c (a_ic - b_jc)^2 in float64, the exact quantity that the
expansion form |a|^2 + |b|^2 - 2 a.b (kept on purpose, model5_b.py:1495-1505) approximates; every bound is a count of
roundings.

Names follow ops._Chamfer: for a[B,n,3], b[B,m,3] and D[B,n,m],
  min_over_a / arg_over_a [B,m]   min and first arg-min over i (axis 1): the partner in a of every b-point
  min_over_b / arg_over_b [B,n]   min and first arg-min over j (axis 2): the partner in b of every a-point

  truth(a, b)                      D, float64
  distance_bound(a, b)             Bd with |P32 - D| <= Bd for the kernel's and the C oracle's float32 P
  min_interval(D, Bd, axis)        the interval a float32 row / column minimum must lie in
  grad(a, b, aoa, aob, g1, g2)     float64 gradient at given arg-mins, the sums of |term| and the term counts
  fma32, kernel_p32, plain_p32     the kernel's formula (exact float32 fma) and the oracle's (no fma) in NumPy
  check_minima / check_argmins / check_grad / check_first_copy / check_planted    the assertions, shared by the CPU test of
                                   the oracle and the GPU test of the kernel
  uniform / offset / scaled / with_ties / funnel    seeded inputs
"""
import collections

import numpy as np

U32 = 2.0 ** -24        # unit roundoff of float32
ROUNDINGS = 5           # the longest path of one P entry (distance_bound)
TERM_ROUNDINGS = 2      # one gradient term 2 g (x - y): the difference and the product; 2 g is exact
TILE = 512              # chamfer_rowmin_kernel walks the other cloud in 512-point tiles, four quarters of (cnt + 3) >> 2

Case = collections.namedtuple("Case", "a b planted")      # planted: [(direction "over_a" | "over_b", batch, row, index)]

# (B, n, m) of the device test.  The kernel runs every pair in both roles, so both directions meet every edge: walked clouds of
# 1, 3, 7, 77, 511, 512, 513, 1024, 1025, 1536, 1537, 2049 points (a tile is 512; a last tile of 1 - 3 points leaves wavefronts
# an empty quarter), 1, 3, 63, 64, 65, 255, 257, ... rows (a workgroup owns 64; the pack and backward launches have 256 threads
# and grids sized by max(n, m))
SHAPES = [(1, 1, 1), (3, 1, 7), (2, 3, 513), (2, 63, 511), (2, 64, 512), (2, 65, 513), (1, 255, 1024), (1, 257, 1025),
          (2, 300, 77), (1, 1, 2049), (1, 2049, 1), (2, 1536, 1537)]
TIE_SHAPES = [s for s in SHAPES if min(s[1:]) >= 3]      # with_ties needs rows to plant in
FUNNEL_SHAPE = (1, 300, 2049)


def seed_of(kind, shape):
    return 1000 * sum(map(ord, kind)) + 131 * shape[0] + 17 * shape[1] + shape[2]


def gamma(k):
    k = np.asarray(k, dtype=np.float64)
    return k * U32 / (1.0 - k * U32)


def truth(a, b):
    """D[B,n,m] = sum_c (a_ic - b_jc)^2 in float64 of the float32 input VALUES."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    D = np.zeros((a.shape[0], a.shape[1], b.shape[1]))
    for c in range(3):      # by coordinate: no [B,n,m,3] temporary
        d = a[:, :, None, c] - b[:, None, :, c]
        D += d * d
    return D


def distance_bound(a, b):
    """Bd[B,n,m] float64 with |P32(i,j) - D(i,j)| <= Bd(i,j) for every pair.  Derivation (u = 2^-24, gamma_k = k u / (1 - k u);
    a computed value that went through k roundings on its longest path is exact * (1 + theta), |theta| <= gamma_k, term by term):
      * the kernel packs |p|^2 = fma(z, z, fma(y, y, x * x)): x*x rounds once, each fma once -> 3 roundings on the longest
        path, and every term is non-negative: |w32 - |p|^2| <= gamma_3 |p|^2;
      * zz = fma(az, bz, fma(ay, by, ax * bx)): 3 roundings: |zz32 - a.b| <= gamma_3 sum_c |a_c b_c|;
      * s = fl(wa + wb): one more on the norms -> 4;
      * P = fma(-2, zz, s): -2 zz is exact inside the fma, one final rounding -> the norms carry 5, the products 4.
    The longest path is ROUNDINGS = 5, hence Bd = gamma_5 (|a_i|^2 + |b_j|^2 + 2 sum_c |a_ic b_jc|); the exact expansion
    |a|^2 + |b|^2 - 2 a.b IS D, so nothing else enters.  The C oracle (oracle/pzn_oracle.c, orc_chamfer_fwd_f32: no fma, same
    association) rounds x*x, y*y, their sum, z*z, that sum (3 on the longest path of a norm), rx + ry (4), 2 zz exact, the
    subtraction (5): the same bound serves both."""
    a, b = np.abs(np.asarray(a, dtype=np.float64)), np.abs(np.asarray(b, dtype=np.float64))
    na, nb = (a * a).sum(-1), (b * b).sum(-1)
    return gamma(ROUNDINGS) * (na[:, :, None] + nb[:, None, :] + 2.0 * np.einsum("bic,bjc->bij", a, b))


def min_interval(D, Bd, axis):
    """[min(D - Bd), min(D + Bd)] along `axis`: the interval that holds the minimum of any values within Bd of D.  Not clamped
    at 0: the expansion form may come out slightly negative and neither the reference nor the kernel clamps."""
    return (D - Bd).min(axis=axis), (D + Bd).min(axis=axis)


def grad(a, b, aoa, aob, g_moa, g_mob):
    """Float64 gradient of sum(g_moa * min_over_a) + sum(g_mob * min_over_b) at the GIVEN arg-mins (aoa [B,m] into a, aob
    [B,n] into b); either weight may be None -> (ga, gb, ga_abs, gb_abs, ka, kb): the gradients, the per-entry sums of |term|
    and the per-entry numbers of terms.  A term is 2 g (x - y): the pair (i, j) adds it to grad_a[i] and its negative to
    grad_b[j] (dP/da_i = 2 (a_i - b_j) = -dP/db_j).
    Bound of the device's float32 entry: chamfer_bwd_kernel forms a term as fl(fl(2 g) * fl(x - y)) - 2 g is exact, so
    TERM_ROUNDINGS = 2 and term32 = term (1 + theta_2) - and adds the K terms of an entry onto zero by float32 atomics in any
    order: K - 1 rounded additions (0 + t is exact), each term passing through at most K - 1 of them.  So
    |entry32 - entry| <= gamma_(K+1) sum |term| <= gamma_(K+2) sum |term| (entry_bound)."""
    a64, b64 = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    B, n, m = a64.shape[0], a64.shape[1], b64.shape[1]
    ga, gb = np.zeros((B, n, 3)), np.zeros((B, m, 3))
    ga_abs, gb_abs = np.zeros((B, n, 3)), np.zeros((B, m, 3))
    ka, kb = np.zeros((B, n), dtype=np.int64), np.zeros((B, m), dtype=np.int64)
    bi = np.arange(B)[:, None]

    def scatter(i, j, g):      # pairs (i, j) [B,k] with weights g [B,k]
        t = 2.0 * np.asarray(g, dtype=np.float64)[:, :, None] * (a64[bi, i] - b64[bi, j])
        bb = np.broadcast_to(bi, i.shape)
        np.add.at(ga, (bb, i), t)
        np.add.at(gb, (bb, j), -t)
        np.add.at(ga_abs, (bb, i), np.abs(t))
        np.add.at(gb_abs, (bb, j), np.abs(t))
        np.add.at(ka, (bb, i), 1)
        np.add.at(kb, (bb, j), 1)

    if g_mob is not None:      # min over b per a-point i, partner aob[i]
        scatter(np.broadcast_to(np.arange(n), (B, n)), np.asarray(aob, dtype=np.int64), g_mob)
    if g_moa is not None:      # min over a per b-point j, partner aoa[j]
        scatter(np.asarray(aoa, dtype=np.int64), np.broadcast_to(np.arange(m), (B, m)), g_moa)
    return ga, gb, ga_abs, gb_abs, ka, kb


def entry_bound(g_abs, k):
    """gamma_(K+2) sum |term| per gradient entry (grad)."""
    return gamma(np.asarray(k)[..., None] + TERM_ROUNDINGS) * g_abs


# --------------------------------------------------------------------------- the float32 formulas, written out

def fma32(a, b, c):
    """Exact float32 fma(a, b, c) of float32 arrays, one rounding: the product of two float32 is exact in float64, TwoSum gives
    p + c = s + e exactly, and rounding s to float32 differs from rounding s + e only where s sits exactly half way between
    two float32 values and e != 0 - there e decides.  (Python's math.fma would do; it exists from 3.13 on.)  No overflow or
    subnormals at the sizes used here."""
    p = np.asarray(a, dtype=np.float32).astype(np.float64) * np.asarray(b, dtype=np.float32).astype(np.float64)
    c = np.asarray(c, dtype=np.float32).astype(np.float64)
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)
    r = s.astype(np.float32)
    r64 = r.astype(np.float64)
    away = np.where(s > r64, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32)
    other = np.nextafter(r, away)                                       # the float32 neighbour on s's side of r
    tie = (s != r64) & (np.abs(other.astype(np.float64) - s) == np.abs(r64 - s)) & (e != 0)
    lo, hi = np.minimum(r, other), np.maximum(r, other)
    return np.where(tie, np.where(e > 0, hi, lo), r).astype(np.float32)


def packed_norm(p):
    """chamfer_pack_kernel's w: fma(z, z, fma(y, y, x * x))."""
    p = np.asarray(p, dtype=np.float32)
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    return fma32(z, z, fma32(y, y, x * x))


def kernel_p32(p, q):
    """chamfer_rowmin_kernel's P of the points p, q [...,3] (broadcast against each other), bit for bit:
    zz = fma(pz, qz, fma(py, qy, px * qx)); P = fma(-2, zz, wp + wq).  Symmetric in p and q."""
    p, q = np.asarray(p, dtype=np.float32), np.asarray(q, dtype=np.float32)
    zz = fma32(p[..., 2], q[..., 2], fma32(p[..., 1], q[..., 1], p[..., 0] * q[..., 0]))
    return fma32(np.float32(-2.0), zz, packed_norm(p) + packed_norm(q))


def kernel_matrix(a, b):
    """kernel_p32 of every pair -> [B,n,m] float32."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return kernel_p32(a[:, :, None, :], b[:, None, :, :])


def plain_matrix(a, b):
    """The C oracle's formula in NumPy float32, no fma: P = (rx + ry) - 2 zz, sums left to right -> [B,n,m] float32."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    ra = (a[..., 0] * a[..., 0] + a[..., 1] * a[..., 1]) + a[..., 2] * a[..., 2]
    rb = (b[..., 0] * b[..., 0] + b[..., 1] * b[..., 1]) + b[..., 2] * b[..., 2]
    A, Bm = a[:, :, None, :], b[:, None, :, :]
    zz = (A[..., 0] * Bm[..., 0] + A[..., 1] * Bm[..., 1]) + A[..., 2] * Bm[..., 2]
    return (ra[:, :, None] + rb[:, None, :]) - np.float32(2.0) * zz


# --------------------------------------------------------------------------- the assertions

def _take(M, idx, axis):
    """M[b, idx[b, j], j] (axis 1) or M[b, i, idx[b, i]] (axis 2)."""
    return np.take_along_axis(M, np.expand_dims(np.asarray(idx, dtype=np.int64), axis), axis=axis).squeeze(axis)


def check_minima(D, Bd, moa, mob):
    """(a) every returned minimum lies in min_interval of its column (moa) / row (mob) -> the worst signed
    (value - float64 minimum) / (bound at the float64 arg-min)."""
    worst = 0.0
    for name, v, axis in (("min_over_a", moa, 1), ("min_over_b", mob, 2)):
        v = np.asarray(v, dtype=np.float64)
        lo, hi = min_interval(D, Bd, axis)
        assert v.shape == lo.shape, (name, v.shape, lo.shape)
        bad = ~((v >= lo) & (v <= hi))      # written so that a NaN is bad
        assert not bad.any(), (name, int(bad.sum()), np.argwhere(bad)[:4].tolist(), v[bad][:4], lo[bad][:4], hi[bad][:4])
        ratio = (v - D.min(axis=axis)) / _take(Bd, D.argmin(axis=axis), axis)
        k = np.abs(ratio).argmax()
        if abs(ratio.flat[k]) > abs(worst):
            worst = float(ratio.flat[k])
    return worst


def check_argmins(D, Bd, aoa, aob):
    """(b) every index in range, and for a returned index c of a row whose float64 arg-min is c*:
    D(c) - Bd(c) <= P32(c) <= P32(c*) <= D(c*) + Bd(c*), hence D(c) - D(c*) <= Bd(c) + Bd(c*)
    -> (the worst (D(c) - D(c*)) / (Bd(c) + Bd(c*)), the number of indices that differ from the float64 arg-min)."""
    worst, flips = 0.0, 0
    for name, idx, axis in (("arg_over_a", aoa, 1), ("arg_over_b", aob, 2)):
        idx = np.asarray(idx)
        star = D.argmin(axis=axis)
        assert idx.shape == star.shape and idx.dtype.kind == "i", (name, idx.shape, idx.dtype)
        assert idx.min() >= 0 and idx.max() < D.shape[axis], (name, int(idx.min()), int(idx.max()), D.shape[axis])
        excess = _take(D, idx, axis) - _take(D, star, axis)
        allow = _take(Bd, idx, axis) + _take(Bd, star, axis)
        bad = ~(excess <= allow)
        assert not bad.any(), (name, int(bad.sum()), np.argwhere(bad)[:4].tolist(), excess[bad][:4], allow[bad][:4])
        worst = max(worst, float((excess / allow).max()))
        flips += int((idx != star).sum())
    return worst, flips


def check_grad(want, ga32, gb32):
    """(f) every entry of the float32 gradients within gamma_(K+2) sum |term| of grad()'s float64 entry; an entry no term lands
    on is exactly 0 -> the worst |difference| / bound."""
    ga, gb, ga_abs, gb_abs, ka, kb = want
    worst = 0.0
    for name, got, ref64, absum, k in (("grad_a", ga32, ga, ga_abs, ka), ("grad_b", gb32, gb, gb_abs, kb)):
        got = np.asarray(got, dtype=np.float64)
        assert got.shape == ref64.shape, (name, got.shape, ref64.shape)
        err, bound = np.abs(got - ref64), entry_bound(absum, k)
        bad = ~(err <= bound)
        assert not bad.any(), (name, int(bad.sum()), np.argwhere(bad)[:4].tolist(), err[bad][:4], bound[bad][:4])
        live = bound > 0
        if live.any():
            worst = max(worst, float((err[live] / bound[live]).max()))
    return worst


def first_copy(x):
    """[B,k]: for every row of x [B,k,3] the lowest index of a row with the same three float32 bit patterns."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    out = np.empty(x.shape[:2], dtype=np.int64)
    for bb in range(x.shape[0]):
        rows = x[bb].view(np.uint32).view([("", np.uint32)] * 3).ravel()
        _, first, inv = np.unique(rows, return_index=True, return_inverse=True)
        out[bb] = first[inv.ravel()]
    return out


def check_first_copy(a, b, aoa, aob):
    """(d) bit copies of a point have bit-equal P whatever the rounding, so a returned index is the lowest of its copies."""
    fa, fb = first_copy(a), first_copy(b)
    aoa, aob = np.asarray(aoa, dtype=np.int64), np.asarray(aob, dtype=np.int64)
    bad1, bad2 = np.take_along_axis(fa, aoa, 1) != aoa, np.take_along_axis(fb, aob, 1) != aob
    assert not bad1.any(), ("arg_over_a", np.argwhere(bad1)[:4].tolist(), aoa[bad1][:4], np.take_along_axis(fa, aoa, 1)[bad1][:4])
    assert not bad2.any(), ("arg_over_b", np.argwhere(bad2)[:4].tolist(), aob[bad2][:4], np.take_along_axis(fb, aob, 1)[bad2][:4])


def check_planted(case, aoa, aob):
    """(d) the planted queries return the planted (lowest) copy -> how many were looked at."""
    for direction, bb, row, want in case.planted:
        got = int((aoa if direction == "over_a" else aob)[bb, row])
        assert got == want, (direction, bb, row, got, want)
    return len(case.planted)


def planted_are_float64_ties(case, D, Bd):
    """The builder's own claim, in float64: at a planted query the float64 minimum is reached by the planted index, every index
    that reaches it is a bit copy of that point, and no other point comes within the rounding bounds of it."""
    fa, fb = first_copy(case.a), first_copy(case.b)
    for direction, bb, row, want in case.planted:
        d, bd, fc = (D[bb, :, row], Bd[bb, :, row], fa[bb]) if direction == "over_a" else (D[bb, row, :], Bd[bb, row, :], fb[bb])
        assert d[want] == d.min() and fc[want] == want, (direction, bb, row, want)
        others = fc != want
        if others.any():
            assert (d[others] - bd[others]).min() > d[want] + bd[want], (direction, bb, row, want)


# --------------------------------------------------------------------------- inputs

def uniform(seed, B, n, m):
    rng = np.random.default_rng(seed)
    return Case(rng.random((B, n, 3), dtype=np.float32), rng.random((B, m, 3), dtype=np.float32), [])


def offset(seed, B, n, m, shift=10.0):
    """The unit cube moved away from the origin: what the expansion form's cancellation costs."""
    c = uniform(seed, B, n, m)
    return Case(c.a + np.float32(shift), c.b + np.float32(shift), [])


def scaled(seed, B, n, m, scale):
    c = uniform(seed, B, n, m)
    return Case(c.a * np.float32(scale), c.b * np.float32(scale), [])


def quarters(k):
    """chamfer_rowmin_kernel's split of a walked cloud of k points -> [tile][wavefront] = (first, end): tiles of TILE points,
    the last one shorter, each in four quarters of (cnt + 3) >> 2 (the last quarters of a short tile are shorter or empty)."""
    out = []
    for base in range(0, k, TILE):
        cnt = min(TILE, k - base)
        per = (cnt + 3) >> 2
        out.append([(base + min(cnt, w * per), base + min(cnt, w * per + per)) for w in range(4)])
    return out


def _plant(rng, X, Y, used_x, used_y, direction, planted, side):
    """Copies of one point at several indices of the walked cloud X, three placements (each its own point, far from the unit
    cube and from each other), and up to two queries per placement in Y: one ON the point, one next to it."""
    k = X.shape[1]
    tiles = quarters(k)

    def free(span):
        return [i for i in range(*span) if i not in used_x]

    groups = []
    # (i) two copies inside one wavefront's quarter of the first tile (the strict `<` of the scan keeps the first)
    for w in (1, 0, 2, 3):
        f = free(tiles[0][w])
        if len(f) >= 2:
            groups.append([f[0], f[-1]])
            used_x.update(groups[-1])
            break
    # (ii) one copy in each of several quarters of the first tile (they meet in LDS), the lowest not in wavefront 0's
    pick = [f[len(f) // 2] for f in (free(tiles[0][w]) for w in (1, 2, 3)) if f]
    if len(pick) < 2:
        pick = [f[len(f) // 2] for f in (free(tiles[0][w]) for w in range(4)) if f]
    if len(pick) >= 2:
        groups.append(pick)
        used_x.update(pick)
    # (iii) copies in different tiles: the lowest in the LAST quarter of the first tile, so that wavefront 0 meets a later copy first
    if len(tiles) >= 2:
        f = free(tiles[0][3])
        pick = f[:1]
        for t in range(1, len(tiles)):
            ft = free(tiles[t][t % 4]) or free((tiles[t][0][0], tiles[t][3][1]))
            pick += ft[len(ft) // 2:len(ft) // 2 + 1]
        if len(pick) >= 2:
            groups.append(pick)
            used_x.update(pick)
    B = X.shape[0]
    for g, idx in enumerate(groups):
        p = (np.array([2.0 + 1.5 * g, 2.0 + 1.5 * side, 0.5]) + 0.25 * rng.random((B, 3))).astype(np.float32)
        X[:, idx] = p[:, None, :]
        rows = [r for r in range(Y.shape[1]) if r not in used_y][:2]
        near = (p + np.array([0.01, -0.005, 0.002], dtype=np.float32)).astype(np.float32)
        for r, q in zip(rows, (p, near) if g % 2 == 0 else (near, p)):
            Y[:, r] = q
            used_y.add(r)
            planted.extend((direction, bb, r, min(idx)) for bb in range(B))


def with_ties(seed, B, n, m):
    """Uniform clouds with exact ties planted in both directions (every duplicate is a bit copy, so its float32 P is bit-equal
    whatever the rounding):
      * the last min(k // 8, 16) rows of each cloud are copies of its row 0, as the loader pads pieces (datapipe._compact),
        with a query of the other cloud next to row 0;
      * _plant's three placements in each cloud with their queries in the other;
      * one b row equal to an a row.
    What does not fit a small cloud is left out.  planted lists (direction, batch, query row, the lowest copy's index)."""
    rng = np.random.default_rng(seed)
    a, b = rng.random((B, n, 3), dtype=np.float32), rng.random((B, m, 3), dtype=np.float32)
    used = {"a": set(), "b": set()}
    planted, padded = [], set()
    for name, x in (("a", a), ("b", b)):
        k = x.shape[1]
        pad = min(k // 8, 16)
        if pad:
            padded.add(name)
            x[:, k - pad:] = x[:, :1]
            used[name].update(range(k - pad, k))
            used[name].add(0)
    order = (("b", b, "a", a), ("a", a, "b", b)) if m >= n else (("a", a, "b", b), ("b", b, "a", a))
    for xn, x, yn, y in order:      # the larger cloud is walked first: its queries go in before the smaller one fills up
        _plant(rng, x, y, used[xn], used[yn], "over_" + xn, planted, side=0 if xn == "a" else 1)
    for xn, x, yn, y in order:
        rows = [r for r in range(y.shape[1]) if r not in used[yn]][:1]
        if xn in padded and rows:
            y[:, rows[0]] = x[:, 0] + np.array([0.002, 0.001, -0.001], dtype=np.float32)
            used[yn].add(rows[0])
            planted.extend(("over_" + xn, bb, rows[0], 0) for bb in range(B))
    ia = [r for r in range(n) if r not in used["a"]][:1]
    jb = [r for r in range(m) if r not in used["b"]][-1:]
    if ia and jb:
        b[:, jb[0]] = a[:, ia[0]]
    return Case(a, b, planted)


def funnel(seed, B, n, m):
    """All of b in a tight cluster, a's point n // 2 next to it (on the +++ side, so all terms landing on it have one sign per
    coordinate) and every other a-point far away: every b-point's partner is the same index, m + 1 atomics land on one
    gradient entry."""
    rng = np.random.default_rng(seed)
    centre = np.array([0.5, 0.4, 0.6])
    b = (centre + 1e-3 * (rng.random((B, m, 3)) - 0.5)).astype(np.float32)
    a = (5.0 + rng.random((B, n, 3))).astype(np.float32)
    a[:, n // 2] = (centre + 0.01).astype(np.float32)
    return Case(a, b, [("over_a", bb, j, n // 2) for bb in range(B) for j in range(m)])
