"""Inputs of the tests of the joint refinement with kept rows chosen again (ops.joint_refine(..., ma=, mb=),
pzn_joint_refine_trim_f32): tests/_joint_trim_ref.py's puzzles stacked into launch arguments, the lattice puzzles whose float32
distances are exact, and the two case families that tests/test_joint_trim_cpu.py (float64 only) and
tests/test_gpu_joint_trim.py share.

  stack(cases)                              the launch arguments of TrimPuzzles of one graph and one (ka, kb)
  lattice_puzzle(rng, K, joints, k, counts) integer points under signed axis permutations and integer shifts
  trajectory_cases(graph), visit_cases(graph)   the two families
  trajectory_row(P), visit_row(P)           their float64 sides
"""
import numpy as np
import torch

from tests import _icp_ref as ref
from tests import _joint_ref as jr
from tests import _joint_trim_ref as jt

GRAPHS = ["pair", "chain3", "ring4", "both3", "complete5"]
VISIT_GRAPHS = ["chain3", "ring4", "both3", "complete5"]      # piece 1 has a joint in each role
MARGIN_FACTOR = 16.0         # tests/test_gpu_joint_refine.py's: margins below this many distance bounds leave a case out
STEP_FACTOR = 4.0            # tests/test_gpu_joint_refine.py's rule and reason
GAP_MIN = 2.0 ** -10         # tests/_joint_counts.py's rule and reason: only a unique optimum is compared
TRAJECTORY_CASES, TRAJECTORY_SWEEPS, TRAJECTORY_K = 16, 2, 8
VISIT_CASES, VISIT_K = 24, 9
# graph -> cases of trajectory_cases(graph) that the float64 loop leaves out (a nearest-neighbour margin or a keep margin
# below MARGIN_FACTOR bounds at a pose it evaluated); asserted on the CPU (tests/test_joint_trim_cpu.py), at most 4 of 16 each
TRAJECTORY = {"pair": 0, "chain3": 0, "ring4": 1, "both3": 0, "complete5": 0}
# graph -> cases of visit_cases(graph) that do not enter, at most 6 of 24 each (the same test file)
VISIT = {"chain3": 0, "ring4": 0, "both3": 0, "complete5": 0}


def stack(cases):
    """The launch arguments of Z TrimPuzzles as host tensors -> (a [Z J,ka,3], b [Z J,kb,3], ma [Z,J] int32, mb [Z,J] int32,
    joints [Z,J,2] int32, G0 [Z,K,4,4], movable [Z,K] uint8); every set fills its stride."""
    a = np.stack([A for P in cases for A in P.A]).astype(np.float32)
    b = np.stack([B for P in cases for B in P.B]).astype(np.float32)
    ma = np.array([P.ma for P in cases], dtype=np.int32)
    mb = np.array([P.mb for P in cases], dtype=np.int32)
    joints = np.array([P.joints for P in cases], dtype=np.int32)
    G0 = np.stack([P.G0 for P in cases]).astype(np.float32)
    movable = np.stack([P.movable for P in cases]).astype(np.uint8)
    return tuple(torch.from_numpy(x) for x in (a, b, ma, mb, joints, G0, movable))


def _axis_pose(rng):
    """A signed permutation of the axes with determinant +1 and an integer shift: it moves integer points to integer points
    with every float32 product and sum exact."""
    while True:
        R = np.zeros((3, 3))
        R[np.arange(3), rng.permutation(3)] = rng.choice([-1.0, 1.0], 3)
        if np.linalg.det(R) > 0:
            return ref.rigid(R, rng.integers(-2, 3, 3).astype(np.float64))


def lattice_puzzle(rng, K, joints, k, counts, side=4):
    """K pieces under poses of _axis_pose (piece 0: the identity); every set of a joint is k = (ka, kb) points drawn with
    repetition from the side^3 integer lattice of the root frame (so rows are duplicated and row minima tie), taken into its
    piece's frame (integers again).  Every squared distance under G0 is a small integer, exact in float32 and float64 alike.
    counts [J] of (ma, mb), kept as they are (a count outside [1, k] marks a row the kernel skips) -> TrimPuzzle."""
    ka, kb = (k, k) if np.isscalar(k) else k
    G0 = np.stack([ref.rigid(np.eye(3), np.zeros(3))] + [_axis_pose(rng) for _ in range(K - 1)])
    A, B = [], []
    for i, j in joints:
        ra = rng.integers(0, side, (ka, 3)).astype(np.float64)
        rb = rng.integers(0, side, (kb, 3)).astype(np.float64)
        A.append(ref.transform(jr._inverse(G0[i]), ra).astype(np.float32))
        B.append(ref.transform(jr._inverse(G0[j]), rb).astype(np.float32))
    return jt.TrimPuzzle(K, [tuple(x) for x in joints], A, B, G0.astype(np.float32), G0, np.arange(K) > 0,
                         [int(c[0]) for c in counts], [int(c[1]) for c in counts])


def _family(graph, seed, n_cases, k, same, movable):
    K, joints = jr.GRAPHS[graph]
    rng = np.random.default_rng(seed + GRAPHS.index(graph))
    out = []
    for _ in range(n_cases):
        n = rng.integers((k + 1) // 2, k + 1, size=len(joints))
        P, _, _ = jt.partial_puzzle(rng, K, joints, k, None, same=same, n_mate=n, movable=movable(K), quick=True)
        out.append(jt.with_counts(P, n, n))
    return out


def trajectory_cases(graph):
    """16 cases, k = 8: per joint a count n drawn from 4..8, n mating rows (B's are A's in another order) and 8 - n rows on the
    other faces, ma = mb = n."""
    return _family(graph, 7500, TRAJECTORY_CASES, TRAJECTORY_K, True, lambda K: None)


def visit_cases(graph):
    """24 cases, k = 9 (the scan's tail loop): only piece 1 movable, per joint a count n drawn from 5..9, two samplings of the
    shared curve with their own noise, ma = mb = n."""
    return _family(graph, 7600, VISIT_CASES, VISIT_K, False, lambda K: np.arange(K) == 1)


def trajectory_row(P):
    """-> (the float64 loop's TrimRefined, entered): a case enters where every nearest-neighbour margin AND every keep margin
    met at a pose the loop evaluated exceeds MARGIN_FACTOR nearest_bound2."""
    want = jt.refine(P, TRAJECTORY_SWEEPS)
    return want, bool(want.margin_ratio >= MARGIN_FACTOR and want.keep_ratio >= MARGIN_FACTOR)


def visit_row(P):
    """The float64 side of one visit of piece 1 under G0 -> (want [4,4] float64 not rounded, yardstick error = visit_f32 against
    it, entered, gap, kept {e: (kept_a, kept_b)} under the candidate).  tests/_joint_counts.visit_row's rule with the keep
    margins beside the nearest-neighbour margins, under G0 and under the candidate, and the trimmed intervals: float64 says
    the candidate lowers E_p beyond the rounding intervals of both sums, whichever rows the kernel kept."""
    g0 = jr.f32(P.G0)
    _, each = jt.piece_energy(P, g0, 1)
    want = jt.visit(P, g0, 1, each, round32=False)
    yard = ref.pose_err(jt.visit_f32(P, P.G0, 1, each), want)
    x, y, w = jt._pairs(P, g0, 1, each, np.float64)
    xd, yd = x - (w[:, None] * x).sum(axis=0) / w.sum(), y - (w[:, None] * y).sum(axis=0) / w.sum()
    S = (w[:, None] * xd).T @ yd
    sv = np.linalg.svd(S, compute_uv=False)
    gap = float((sv[1] + np.sign(np.linalg.det(S)) * sv[2]) / sv[0])
    gn = g0.copy()
    gn[1] = jr.f32(want)
    _, each_n = jt.piece_energy(P, gn, 1)
    scale = {e: jr.nearest_bound2(P.A[e], P.B[e], g0[P.joints[e][0]], g0[P.joints[e][1]]) for e in each}
    entered = gap >= GAP_MIN and all(min(o.margin, o.keep_margin) > MARGIN_FACTOR * scale[e] for e, o in each.items()) \
        and all(min(o.margin, o.keep_margin) > MARGIN_FACTOR * scale[e] for e, o in each_n.items())
    if entered:
        inc = jr.incident(P, 1)
        iv0, iv1 = jt.joint_intervals(P, g0, inc)[inc], jt.joint_intervals(P, gn, inc)[inc]
        entered = jr.sum_interval(iv1)[1] < jr.sum_interval(iv0)[0]
    return want, yard, bool(entered), gap, {e: (o.kept_a, o.kept_b) for e, o in each_n.items()}
