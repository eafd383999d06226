"""Lattice clouds and exact integer references for the sampling and search kernels (no GPU, no C).

A cloud whose coordinates are k / 8 in float32 (queries may sit at odd multiples of 1 / 16) makes every difference, square
and sum of sqdist3 exact, so a pick depends on no operation order and no contraction: only the selection rules decide -
lowest index wins the arg-max, kNN order is (distance, index), the ball keeps d <= r^2.  On such clouds most rounds of
farthest point sampling and most kNN queries are decided by an exact tie between DIFFERENT points, which random clouds in
[0, 1) never produce.

Everything here counts in units of 1 / 16: a site s is the integer 2 s, an off-lattice query 2 s + 1, a squared distance
an int64 in units of 1 / 256.  The references are written from the rules above, independently of oracle/pzn_oracle.c;
tests/test_lattice_cpu.py holds them against that oracle on every shape tests/test_gpu_ties.py uses, and checks there
that those shapes really are decided by ties (the statistics at the end of this file).
"""
import numpy as np

UNIT = 16                 # integer coordinates are in units of 1 / UNIT
WAVE = 64


# ---------------------------------------------------------------------------------------------------------- inputs

def lattice(n, side, rng):
    """n integer sites [n, 3] in 0 .. side-1: a random subset without repetition while n <= side^3, otherwise every site
    once plus random repeats, the whole shuffled."""
    total = side ** 3
    if n <= total:
        flat = rng.permutation(total)[:n]
    else:
        flat = np.concatenate((np.arange(total), rng.integers(0, total, n - total)))
        rng.shuffle(flat)
    return np.stack((flat // (side * side), (flat // side) % side, flat % side), axis=-1).astype(np.int64)


def to_units(sites, shift=0, half=False):
    """Sites (+ an integer shift, in sites) as integers in units of 1 / 16; half: moved by 1 / 16 along every axis."""
    return (np.asarray(sites, np.int64) + int(shift)) * 2 + (1 if half else 0)


def to_float(units):
    """Integer coordinates in units of 1 / 16 -> float32, exactly."""
    f = (np.asarray(units, np.int64) / UNIT).astype(np.float32)
    assert np.array_equal(f.astype(np.float64) * UNIT, units)
    return f


def cloud(sites, shift=0):
    """The float cloud of integer sites: (sites + shift) / 8 in float32."""
    return to_float(to_units(sites, shift))


def side_for(n, cap=None):
    """The smallest cube that holds n distinct sites; with a cap the cube stays that small and sites repeat (on a sparse
    lattice fewer rounds and queries are decided by a tie)."""
    side = 1
    while side ** 3 < n:
        side += 1
    return side if cap is None else min(side, cap)


def signed_permutations():
    """The 24 proper rotations that map the lattice onto itself, as integer 3x3 matrices (identity first)."""
    import itertools
    out = []
    for perm in itertools.permutations(range(3)):
        for signs in itertools.product((1, -1), repeat=3):
            R = np.zeros((3, 3), np.int64)
            for r in range(3):
                R[r, perm[r]] = signs[r]
            if round(np.linalg.det(R)) == 1:
                out.append(R)
    out.sort(key=lambda R: not np.array_equal(R, np.eye(3, dtype=np.int64)))
    return out


# ------------------------------------------------------------------------------------------------------ references

def _sq(a, b):
    """int64 squared distances [len(a), len(b)] of integer coordinates."""
    d = a[:, None, :].astype(np.int64) - b[None, :, :].astype(np.int64)
    return (d * d).sum(-1)


def fps_int(sites, S, start, stats_T=None):
    """Farthest point sampling of one cloud of integer coordinates [N, 3]: int64 squared distances, running minimum, FIRST
    maximum -> picks [S] int64.  With stats_T (the threads of the kernel form that serves this N) -> (picks, statistics
    of the S - 1 rounds that decide a pick: how many have two or more tied maxima, in how many of those the tied points
    sit in different wavefronts, how many tie at distance 0)."""
    pts = np.asarray(sites, np.int64)
    N = pts.shape[0]
    dist = np.full(N, np.iinfo(np.int64).max, np.int64)
    far = int(start)
    picks = np.empty(S, np.int64)
    tied = cross = zero = 0
    for i in range(S):
        picks[i] = far
        d = pts - pts[far]
        dist = np.minimum(dist, (d * d).sum(-1))
        far = int(np.argmax(dist))                     # numpy's argmax returns the first maximum
        if stats_T is not None and i < S - 1:
            at = np.flatnonzero(dist == dist[far])
            if len(at) >= 2:
                tied += 1
                cross += len(np.unique((at % stats_T) // WAVE)) >= 2
                zero += int(dist[far] == 0)
    if stats_T is None:
        return picks
    return picks, dict(rounds=S - 1, tied=tied, cross=int(cross), zero=zero)


def fps_int_batch(units, S, starts):
    return np.stack([fps_int(units[b], S, starts[b]) for b in range(len(units))])


def knn_int(sites, queries, K):
    """[S, K] int64: the K nearest rows of sites [N, 3] per query [S, 3] in (distance, index) order."""
    d = _sq(np.asarray(queries), np.asarray(sites))
    idx = np.broadcast_to(np.arange(d.shape[1]), d.shape)
    return np.lexsort((idx, d), axis=-1)[:, :K].astype(np.int64)


def ball_int(r2_num, nsample, sites, queries):
    """[S, nsample] int64, the reference's ball query: the first nsample indices (ascending) with squared distance
    <= r2_num (r^2 in units of 1 / 256; any real number), the remaining slots filled with slot 0, which is N itself
    when nothing lies in the ball."""
    d = _sq(np.asarray(queries), np.asarray(sites))
    S, N = d.shape
    out = np.empty((S, nsample), np.int64)
    for s in range(S):
        hits = np.flatnonzero(d[s] <= r2_num)[:nsample]
        out[s, :len(hits)] = hits
        out[s, len(hits):] = hits[0] if len(hits) else N
    return out


def r2_units(radius):
    """radius (a Python float) -> its float32 r^2, as the kernels and the oracle take it, in units of 1 / 256 (exact)."""
    return float(np.float32(float(radius) ** 2)) * (UNIT * UNIT)


# ------------------------------------------------------------------------------------------------ tie statistics

def fps_threads(N, background_cap=None):
    """Threads per cloud of the farthest-point-sampling form that serves N points (csrc/fps.hip); background_cap: the row
    bound of the background entry (max_count, or N)."""
    if background_cap is not None:
        return 256 if background_cap <= 8192 else (512 if background_cap <= 16384 else 1024)
    if N <= 256:
        return 64 if N <= 64 else (128 if N <= 128 else 256)
    return 256 if N <= 4096 else (512 if N <= 8192 else 1024)


def fps_form(N):
    """Which of the main entry's three rounds serves N: 32-bit keys, 64-bit keys, published coordinates."""
    return "key32" if N <= 1024 else ("key64" if N <= 12693 else "published")


def knn_stats(sites, queries, K):
    """Per query: tie - the K-th and (K+1)-th distances are equal (False where N == K); cand / lane_max - what
    select32's first bound lets through (knn.hip: a lane owns the point pairs 128 p + 2 lane, + 1, the bound is the 32nd
    smallest of the 64 lane minima, every point at or below it is a candidate): their number and the most on one lane."""
    sites = np.asarray(sites)
    d = _sq(np.asarray(queries), sites)
    S, N = d.shape
    srt = np.sort(d, axis=-1)
    tie = srt[:, K - 1] == srt[:, K] if N > K else np.zeros(S, bool)
    lane = (np.arange(N) % 128) // 2
    big = np.iinfo(np.int64).max
    cand = np.zeros(S, np.int64)
    lane_max = np.zeros(S, np.int64)
    for s in range(S):
        lmin = np.full(WAVE, big, np.int64)
        np.minimum.at(lmin, lane, d[s])
        tau = np.sort(lmin)[31]
        hit = d[s] <= tau
        cand[s] = hit.sum()
        lane_max[s] = np.bincount(lane[hit], minlength=WAVE).max()
    return dict(tie=tie, cand=cand, lane_max=lane_max)


# ------------------------------------------------------------------------------------------- the cases of the GPU tests
# Shapes, lattices and seeds live here so that tests/test_lattice_cpu.py checks exactly what tests/test_gpu_ties.py runs.

FPS_SIDE_CAP = 10
KNN_SIDE_CAP = 12


def _starts(rng, B, N):
    """Different starts, one of them the last index."""
    st = rng.integers(0, N, size=B)
    st[-1] = N - 1
    return st.astype(np.int64)


def fps_case(N, S=None, side=None, seed=0, shift=0, B=2, identical=False):
    """-> dict(units [B, N, 3] int64, xyz float32, start [B], S).  Every cloud of the batch is its own draw."""
    rng = np.random.default_rng(1000 + 7 * N + seed)
    side = side_for(N, FPS_SIDE_CAP) if side is None else side
    S = min(N, 96) if S is None else S
    if identical:
        sites = np.tile(np.array([3, 1, 2], np.int64), (B, N, 1))
    else:
        sites = np.stack([lattice(N, side, rng) for _ in range(B)])
    units = to_units(sites, shift)
    return dict(N=N, S=S, side=side, units=units, xyz=to_float(units), start=_starts(rng, B, N))


# main entry: N either side of every dispatch edge of pzn_fps_f32 (the powers of two are the `full` shapes), the last
# cloud whose LDS image fits and the first that takes the published form, the largest shapes
FPS_MAIN_N = [1, 2, 63, 64, 65, 128, 129, 256, 257, 511, 512, 513, 1024, 1025, 2047, 2048, 2049, 4096, 4097, 8192, 8193,
              12693, 12694, 16384, 16385, 20000]
# N = 65: the second wavefront holds row 64 alone; on 27 sites with repeats that row, the last to win any tie, stays among
# the tied maxima for most rounds (and with the start on it, the lattice is exhausted after 27 of the 65 picks)
FPS_MAIN_SIDE = {65: 3}
# name -> keyword arguments of fps_case; the three `zero` cases exhaust a small lattice before S picks (S < N), one per form
FPS_SPECIAL = {
    "s_equals_n": dict(N=200, S=200, side=6),
    "identical": dict(N=300, S=64, identical=True),
    "shifted": dict(N=1500, S=96, shift=-40),
    "zero_key32": dict(N=512, S=96, side=4),
    "zero_key64": dict(N=4096, S=600, side=8),
    "zero_published": dict(N=13000, S=600, side=8),
}

# background entry: N -> the launch_published shape it takes (cap <= 2048 / 4096 / 8192 / 16384 / 32768); 600 and 2300
# give an odd number of live register slots, so the pair loop evaluates one padding slot
FPS_BG_N = [600, 2300, 5000, 9000, 17000]
# padded buffers: (rows of the buffer, real rows of each of the three clouds); ceil(c / 256) is odd for 600 and 2300, even
# for 1000, 777 and 1900
FPS_BG_COUNTS = [(2300, (600, 1000, 777)), (5000, (2300, 1900, 2300))]


def fps_bg_case(N):
    return fps_case(N, S=96 if N != 600 else 128, seed=5, B=3, side=8 if N == 600 else None)


def fps_counts_case(N, counts):
    """The buffer of test_fps_vs_oracle: rows >= counts[b] are copies of row 0; starts inside the real rows."""
    rng = np.random.default_rng(2000 + N)
    B = len(counts)
    units = np.stack([to_units(lattice(N, side_for(min(counts), FPS_SIDE_CAP), rng)) for _ in range(B)])
    start = np.empty(B, np.int64)
    for b, c in enumerate(counts):
        units[b, c:] = units[b, 0]
        start[b] = rng.integers(0, c)
    start[-1] = counts[-1] - 1
    return dict(N=N, S=96, counts=tuple(counts), units=units, xyz=to_float(units), start=start)


# merge_resample: (Na, Nb, n_out); unions 200, 256, 330, 700, 1024, 2048, 4096 (MRG_MAX_UNION), n_out = 300 crosses a
# pick-buffer flush
MERGE_SHAPES = [(96, 104, 64), (96, 160, 64), (200, 130, 300), (300, 400, 128), (512, 512, 128), (1024, 1024, 96),
                (2048, 2048, 96)]
# ... each without and with drop lists (the n_out = 300 case without: with drops n_out stays below the distinct kept sites)
MERGE_CASES = [(na, nb, no, d) for na, nb, no in MERGE_SHAPES for d in (False, True) if not (d and no > 128)]


def merge_case(Na, Nb, n_out, with_drops):
    """Two merges (identity pose first, then a 90-degree rotation with a translation in multiples of 1 / 8) of two
    overlapping parts of ONE lattice: about a quarter of b's sites, placed, coincide with sites of a.
    -> dict(a, b float32 [2, ., 3], T [2, 4, 4] float32, start [2], drop_a, drop_b ([2, k] int64 or None),
            union units [2, U, 3] int64 (a, then b as placed), n_out)."""
    rng = np.random.default_rng(3000 + Na + 3 * Nb + (1 if with_drops else 0))
    U = Na + Nb
    shared = Nb // 4
    side = side_for(U)
    rots = signed_permutations()
    a_u, b_u, Ts, unions = [], [], [], []
    for m in range(2):
        pool = lattice(U - shared, side, rng)                      # distinct sites
        a_sites = pool[:Na]
        b_placed = np.concatenate((pool[Na:], a_sites[rng.permutation(Na)[:shared]]))
        b_placed = b_placed[rng.permutation(Nb)]
        R = rots[0] if m == 0 else rots[int(rng.integers(1, len(rots)))]
        t = np.zeros(3, np.int64) if m == 0 else rng.integers(-6, 7, 3)
        b_sites = (b_placed - t) @ R                                # R^T (x - t): T applied to it gives b_placed back
        assert np.array_equal(b_sites @ R.T + t, b_placed)
        T = np.eye(4, dtype=np.float32)
        T[:3, :3] = R
        T[:3, 3] = t / 8.0
        a_u.append(to_units(a_sites)), b_u.append(to_units(b_sites)), Ts.append(T)
        unions.append(np.concatenate((to_units(a_sites), to_units(b_placed))))
    drop_a = drop_b = None
    if with_drops:
        drop_a = np.stack([rng.permutation(Na)[:Na // 10] for _ in range(2)]).astype(np.int64)
        drop_b = np.stack([rng.permutation(Nb)[:Nb // 10] for _ in range(2)]).astype(np.int64)
        drop_a[1, 2] = drop_a[1, 0]                                 # a repeated index
    start = np.array([U - 1, int(rng.integers(0, Na))], np.int64)
    return dict(a=to_float(np.stack(a_u)), b=to_float(np.stack(b_u)), T=np.stack(Ts), start=start, drop_a=drop_a,
                drop_b=drop_b, union=np.stack(unions), n_out=n_out, Na=Na, Nb=Nb)


def merge_kept_distinct(case, m):
    """The number of distinct sites among the kept rows of merge m."""
    U = case["Na"] + case["Nb"]
    kept = np.ones(U, bool)
    if case["drop_a"] is not None:
        kept[case["drop_a"][m]] = False
        kept[case["drop_b"][m] + case["Na"]] = False
    return len(np.unique(case["union"][m][kept], axis=0))


# kNN: name -> (B, N, side, K, lattice queries, off-lattice queries)
def _knn_table():
    t = {}
    for N in (64, 128, 129, 256, 257, 512, 513, 1024, 1025, 2048, 2049, 4096, 4097, 8192):      # every R of knn_select_kernel
        t[f"select_n{N}"] = (2 if N <= 2049 else 1, N, None, 32, 40, 8)
    for N, side in ((300, 4), (2048, 8)):
        t[f"select_n{N}_k1"] = (1, N, side, 1, 40, 8)
    for N in (300, 2048):
        t[f"select_n{N}_k7"] = (1, N, 10 if N == 2048 else None, 7, 40, 8)
        t[f"select_n{N}_k31"] = (1, N, None, 31, 40, 8)
    t["repeat_n2048"] = (1, 2048, 6, 32, 120, 8)                    # repeated sites: the overflow path of select32
    t["repeat_n8192"] = (1, 8192, 8, 32, 120, 8)
    for N in (33, 63, 8193, 13000):                                 # knn32_kernel
        t[f"knn32_n{N}"] = (1, N, 3 if N == 33 else None, 32, min(N, 40), 8)
    t["knn32_n40_k40"] = (1, 40, None, 40, 40, 8)
    for N in (64, 300, 2048):                                       # knn_any_kernel
        for K in (33, 48, 64):
            t[f"any_n{N}_k{K}"] = (1, N, 3 if N == 64 else None, K, 40, 8)
    return t


KNN_CASES = _knn_table()
KNN_OVERFLOW = ("repeat_n2048", "repeat_n8192")
KNN_GROUP = {129: "select_n129", 2048: "select_n2048", 8192: "select_n8192"}


def knn_case(name):
    """-> dict(units [B, N, 3], q_units [B, S, 3] (cloud points, then points 1 / 16 off a site along every axis), xyz, q, K)."""
    B, N, side, K, nq, noff = KNN_CASES[name]
    rng = np.random.default_rng(4000 + sum(map(ord, name)) * 31 + N)
    side = side_for(N, KNN_SIDE_CAP) if side is None else side
    units, q_units = [], []
    for _ in range(B):
        sites = lattice(N, side, rng)
        on = sites[rng.permutation(N)[:nq]]
        off = sites[rng.integers(0, N, noff)]
        units.append(to_units(sites))
        q_units.append(np.concatenate((to_units(on), to_units(off, half=True))))
    units, q_units = np.stack(units), np.stack(q_units)
    return dict(name=name, N=N, K=K, units=units, q_units=q_units, xyz=to_float(units), q=to_float(q_units))


def knn_many_queries_case():
    """B = 64 clouds of 64 points, 512 queries each taken with repetition from the cloud: launch_select reaches 64 queries
    per workgroup (every small case gets 8)."""
    rng = np.random.default_rng(4999)
    B, N, S = 64, 64, 512
    sites = np.stack([lattice(N, 4, rng) for _ in range(B)])
    pick = rng.integers(0, N, (B, S))
    units = to_units(sites)
    q_units = np.take_along_axis(units, pick[:, :, None], axis=1)
    return dict(name="many_queries", N=N, K=32, units=units, q_units=q_units, xyz=to_float(units), q=to_float(q_units))


# ball query
BALL_N = [64, 300, 2048, 13000]
BALL_NSAMPLE = [1, 8, 32]
# radii as Python floats.  0.125: r^2 = 1 / 64 exactly, the axis neighbours lie ON the sphere and are kept.
# sqrt(2) / 8: its square is 0.03125000000000001 in double and rounds to exactly 2 / 64 in float32, so the diagonal
# neighbours lie on the sphere and are kept; the float32 value of sqrt(2) / 8 passed as a float squares to 0.031249998,
# just below 2 / 64, and excludes them.  0.25: three shells further.
BALL_RADII = [0.125, 2.0 ** 0.5 / 8, float(np.float32(2.0 ** 0.5 / 8)), 0.25]
BALL_EMPTY_RADIUS = 0.05      # with off-lattice queries (every point >= sqrt(3) / 16 away) nothing is in the ball


def ball_case(N):
    """-> dict(units [1, N, 3], q_on [1, 48, 3] cloud points, q_off [1, 16, 3] off-lattice points, and their floats)."""
    rng = np.random.default_rng(5000 + N)
    sites = lattice(N, side_for(N), rng)
    on = to_units(sites[rng.permutation(N)[:48]])
    off = to_units(sites[rng.integers(0, N, 16)], half=True)
    units = to_units(sites)[None]
    return dict(N=N, units=units, q_on=on[None], q_off=off[None], xyz=to_float(units), fq_on=to_float(on[None]),
                fq_off=to_float(off[None]))
