"""Inputs of the tests of the joint refinement with a point count per set (ops.joint_refine(..., na=, nb=),
pzn_joint_refine_counts_f32): tests/_joint_ref.py's puzzles with a count per joint and side, their stacking into buffers of one
stride, and the two case families that tests/test_joint_counts_cpu.py (float64 only) and tests/test_gpu_joint_counts.py share.

tests/_joint_ref.py needs nothing new for ragged sets: joint_energy, piece_energy, visit, visit_f32, refine and the interval
functions read len(P.A[e]) and len(P.B[e]), so a Puzzle whose sets differ in size IS the float64 statement of the contract
("every ka / kb of row e is that row's count").

  ragged_puzzle(rng, K, joints, counts, same)   _joint_ref.puzzle with counts[e] = (na_e, nb_e) points for joint e
  stack(cases, cap, fill)                       the launch arguments: sets of stride cap, the rows behind each count = fill
  trajectory_cases(graph), visit_cases(graph)   the two families
  visit_row(P)                                  float64 side of the one-visit check for a case of visit_cases
"""
import numpy as np
import torch

from tests import _icp_ref as ref
from tests import _joint_ref as jr

GRAPHS = ["pair", "chain3", "ring4", "both3", "complete5"]
VISIT_GRAPHS = ["chain3", "ring4", "both3", "complete5"]      # piece 1 has a joint in each role
MARGIN_FACTOR = 16.0         # tests/test_gpu_joint_refine.py's: margins below this many distance bounds leave a case out
STEP_FACTOR = 4.0            # tests/test_gpu_joint_refine.py's rule and reason
TRAJECTORY_CASES, TRAJECTORY_SWEEPS = 16, 2
VISIT_CASES = 24
# With counts of 1..8 the far sides of piece 1's joints may hold one point each: every y of the visit is then one of two
# points, the cross-covariance S = sum w (x - xc)(y - yc)^T has rank 1, and the least-squares rotation is not unique (a whole
# turn about the line of the two points fits equally well).  float64, the kernel and the float32 yardstick each return SOME
# optimum, a turn of order 1 apart, and one such case makes "4 x the largest yardstick error" a bound of order 1 for every
# case.  How well the optimum is determined is a property of the inputs: with S's singular values s1 >= s2 >= s3 and d = the
# sign of det S, a perturbation dS moves the rotation by about |dS| / (s2 + d s3).  Two consequences.  A case ENTERS only
# with (s2 + d s3) / s1 >= GAP_MIN in float64: "float64's candidate lowers E_p, so the kernel had to take its own" needs the
# two candidates to be the same up to rounding.  And the pose check is made twice: against the largest yardstick error of all
# cases as it stands, and against the largest over the cases with a gap of GAP_MIN, which is the one that binds.  2^-10:
# float32 sums perturb S by a few 2^-24 s1, so there every solver is within about 2^-12 of the optimum, and the cases left
# out have a gap of 1e-16 (the rank-1 ones) - nothing lies near the line.  A case that does not enter is held to no pose and
# to no `accepted`, only to what holds for every launch (tests/test_gpu_joint_counts.py's visit_errors says what).
GAP_MIN = 2.0 ** -10
# graph -> cases of trajectory_cases(graph) that the float64 loop leaves out (margin_ratio < MARGIN_FACTOR); asserted on the
# CPU (tests/test_joint_counts_cpu.py), at most 4 of 16 each
TRAJECTORY = {"pair": 0, "chain3": 0, "ring4": 0, "both3": 0, "complete5": 0}


def ragged_puzzle(rng, K, joints, counts, same=False, noise=0.003, angle=np.deg2rad(4.0), shift=0.01, movable=None):
    """_joint_ref.puzzle (its curves, true poses and start poses) where joint e has counts[e] = (na_e, nb_e) points: A[e] is
    [na_e,3] and B[e] is [nb_e,3].  same=True needs na_e = nb_e: B's points are A's in another order."""
    assert len(counts) == len(joints)
    truth = np.stack([ref.rigid(ref.rot(rng.normal(size=3), rng.uniform(0.3, 2.5)), rng.uniform(-0.3, 0.3, 3)) for _ in range(K)])
    A, B, centre, met = [], [], np.zeros((K, 3)), np.zeros(K)
    for e, ((i, j), (na, nb)) in enumerate(zip(joints, counts)):
        W = ref.rot(rng.normal(size=3), rng.uniform(0, np.pi))
        place = rng.uniform(-0.5, 0.5, 3)
        planar = bool(e & 1)
        ra = ref.curve(rng.uniform(0, 1, na), planar) @ W.T + place + rng.normal(scale=noise, size=(na, 3))
        if same:
            assert na == nb
            rb = ra[rng.permutation(na)]
        else:
            rb = ref.curve(rng.uniform(0, 1, nb), planar) @ W.T + place + rng.normal(scale=noise, size=(nb, 3))
        A.append(ref.transform(jr._inverse(truth[i]), ra).astype(np.float32))
        B.append(ref.transform(jr._inverse(truth[j]), rb).astype(np.float32))
        for p, pts in ((i, ra), (j, rb)):
            centre[p] += pts.mean(axis=0)
            met[p] += 1
    G0 = truth.copy()
    for p in range(1, K):
        c = centre[p] / max(met[p], 1)
        Rp = ref.rot(rng.normal(size=3), rng.uniform(-angle, angle))
        G0[p] = ref.rigid(Rp, c - Rp @ c + rng.uniform(-shift, shift, 3)) @ truth[p]
    if movable is None:
        movable = np.arange(K) > 0
    return jr.Puzzle(K, [tuple(x) for x in joints], A, B, G0.astype(np.float32), truth, np.asarray(movable, dtype=bool))


def stack(cases, cap, fill):
    """The launch arguments of Z cases as host tensors -> (a [Z J,ka,3], b [Z J,kb,3], na [Z J] int32, nb [Z J] int32,
    joints [Z,J,2] int32, G0 [Z,K,4,4], movable [Z,K] uint8): cap = (ka, kb) the strides, set e of a holds A[e] in its first
    len(A[e]) rows and `fill` (a float: NaN, 1e30, 0) in every row behind them; b likewise."""
    ka, kb = cap
    rows = [(P, e) for P in cases for e in range(len(P.joints))]
    a = np.full((len(rows), ka, 3), fill, dtype=np.float32)
    b = np.full((len(rows), kb, 3), fill, dtype=np.float32)
    na, nb = np.zeros(len(rows), dtype=np.int32), np.zeros(len(rows), dtype=np.int32)
    for r, (P, e) in enumerate(rows):
        na[r], nb[r] = len(P.A[e]), len(P.B[e])
        assert 1 <= na[r] <= ka and 1 <= nb[r] <= kb
        a[r, :na[r]], b[r, :nb[r]] = P.A[e], P.B[e]
    joints = np.array([P.joints for P in cases], dtype=np.int32)
    G0 = np.stack([P.G0 for P in cases])
    movable = np.stack([P.movable for P in cases]).astype(np.uint8)
    return tuple(torch.from_numpy(x) for x in (a, b, na, nb, joints, G0, movable))


def trajectory_cases(graph):
    """16 cases: same=True, one count per joint drawn from 3..8 and used for both sides."""
    K, joints = jr.GRAPHS[graph]
    rng = np.random.default_rng(7300 + GRAPHS.index(graph))
    out = []
    for _ in range(TRAJECTORY_CASES):
        n = rng.integers(3, 9, size=len(joints))
        out.append(ragged_puzzle(rng, K, joints, [(int(m), int(m)) for m in n], same=True))
    return out


def visit_cases(graph):
    """24 cases: only piece 1 movable, the counts of every joint drawn independently per side from 1..8."""
    K, joints = jr.GRAPHS[graph]
    rng = np.random.default_rng(7400 + GRAPHS.index(graph))
    only = np.arange(K) == 1
    out = []
    for _ in range(VISIT_CASES):
        n = rng.integers(1, 9, size=(len(joints), 2))
        out.append(ragged_puzzle(rng, K, joints, [(int(x), int(y)) for x, y in n], movable=only))
    return out


def visit_row(P):
    """The float64 side of one visit of piece 1 under G0 -> (want [4,4] float64 not rounded, yardstick error = visit_f32
    against it, entered, gap).  gap = (s2 + d s3) / s1 of the visit's cross-covariance in float64.  tests/
    test_gpu_joint_refine.py's rule: a case enters where every nearest-neighbour margin of piece 1's joints exceeds
    MARGIN_FACTOR nearest_bound2 (the kernel cannot have chosen other correspondences) and float64 says the candidate lowers
    E_p beyond the rounding intervals of both sums (the kernel had to take it) - and, here, only where that candidate is the
    one optimum (gap >= GAP_MIN, above)."""
    g0 = jr.f32(P.G0)
    _, corr, margins = jr.piece_energy(P, g0, 1)
    want = jr.visit(P, g0, 1, corr, round32=False)
    yard = ref.pose_err(jr.visit_f32(P, P.G0, 1, corr), want)
    x, y, w = jr._pairs(P, g0, 1, corr, np.float64)
    xd, yd = x - (w[:, None] * x).sum(axis=0) / w.sum(), y - (w[:, None] * y).sum(axis=0) / w.sum()
    S = (w[:, None] * xd).T @ yd
    sv = np.linalg.svd(S, compute_uv=False)
    gap = float((sv[1] + np.sign(np.linalg.det(S)) * sv[2]) / sv[0])
    ends = lambda g, e: (g[P.joints[e][0]], g[P.joints[e][1]])
    entered = gap >= GAP_MIN and all(margins[e] > MARGIN_FACTOR * jr.nearest_bound2(P.A[e], P.B[e], *ends(g0, e)) for e in margins)
    if entered:
        gn = g0.copy()
        gn[1] = jr.f32(want)
        inc = jr.incident(P, 1)
        iv0 = np.array([jr.objective_interval2(P.A[e], P.B[e], *ends(g0, e)) for e in inc])
        iv1 = np.array([jr.objective_interval2(P.A[e], P.B[e], *ends(gn, e)) for e in inc])
        entered = jr.sum_interval(iv1)[1] < jr.sum_interval(iv0)[0]
    return want, yard, bool(entered), gap
