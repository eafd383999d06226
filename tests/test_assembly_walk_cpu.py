"""CPU: assembly.walk_rule - the numpy statement the device walk (ops.assemble_walk) is held to bit for bit - against
assembly.assemble and against the joint comprehension of assembly.refine_assembly, on the table kinds of tests/_walk_cases.py:
6 sizes x 5 kinds x 4 seeds = 120 tables.

Discrete outputs (root, edges, edge scores, placed, joints) are equal exactly.  Poses: both sides compose the same float32 pair
poses along the same tree in float64, assemble with numpy's matmul and walk_rule as ((a0 b0 + a1 b1) + a2 b2) + a3 b3.  Two
computations of a 4-term product are each within gamma_4 = 4 u / (1 - 4 u), u = 2^-53, of the exact one relative to sum |a||b|,
and the entries of a pose d edges below the root are bounded by 1 + sum |t_e| over its path, so per piece
|G_rule - G_assemble| <= 16 d_p 2^-53 (1 + sum |t_e|)."""
import numpy as np
import pytest

from tests import _walk_cases as wc

SIZES = (2, 3, 5, 16, 33, 64)
SEEDS = 4


def _host_joints(score, asm, joint_score=None):
    """The joint list as assembly.refine_assembly forms it (its lines, on a host table)."""
    S = np.asarray(score, dtype=np.float64)
    K = S.shape[0]
    placed = np.asarray(asm.placed, dtype=bool)
    if joint_score is None:
        joint_score = max((float(e[2]) for e in asm.edges), default=-np.inf)
    ok = placed[:, None] & placed[None, :] & ~np.eye(K, dtype=bool) & (S <= float(joint_score))
    return [(int(i), int(j)) for i, j in zip(*np.nonzero(ok))]


def _rule_joints(rule, z=0):
    n = int(rule.n_joints[z])
    assert (rule.joints[z, n:] == -1).all() and (rule.joints[z, :n] >= 0).all()
    return [tuple(int(v) for v in row) for row in rule.joints[z, :n]]


def _path_bound(asm, T):
    """Per piece: 16 d_p 2^-53 (1 + sum of |t_e| over the tree path of piece p)."""
    K = len(asm.placed)
    depth, reach = np.zeros(K), np.zeros(K)
    for i, j, _s, new in asm.edges:
        old = i if new == j else j
        depth[new] = depth[old] + 1
        reach[new] = reach[old] + np.linalg.norm(T[i, j, :3, 3].astype(np.float64))
    return 16.0 * depth * 2.0 ** -53 * (1.0 + reach)


@pytest.mark.parametrize("kind", wc.KINDS)
@pytest.mark.parametrize("K", SIZES)
def test_walk_rule_is_assemble(K, kind):
    from puzzlenet_amd import assembly
    S, T, max_score = wc.make(kind, SEEDS, K, 100)
    rule = assembly.walk_rule(S, T, max_score=max_score)
    some_edge = stopped = False
    for z in range(SEEDS):
        asm = assembly.assemble(S[z], T[z], max_score=max_score)
        n = len(asm.edges)
        assert int(rule.root[z]) == asm.root and int(rule.n_edges[z]) == n
        assert [tuple(int(v) for v in e) for e in rule.edges[z, :n]] == [(i, j, new) for i, j, _s, new in asm.edges]
        assert [float(s) for s in rule.edge_score[z, :n]] == [s for _i, _j, s, _n in asm.edges]
        assert (rule.edges[z, n:] == -1).all() and np.isposinf(rule.edge_score[z, n:]).all()
        assert np.array_equal(rule.placed[z].astype(bool), asm.placed)
        err = np.abs(rule.G[z] - asm.G).max(axis=(1, 2))
        bound = _path_bound(asm, T[z])
        assert (err <= bound).all(), (err / np.maximum(bound, 1e-300)).max()
        assert np.array_equal(rule.G[z][~asm.placed], np.tile(np.eye(4), (int((~asm.placed).sum()), 1, 1)))
        assert _rule_joints(rule, z) == _host_joints(S[z], asm)
        some_edge |= n > 0
        stopped |= n < K - 1
    if kind in ("blocks", "max_score") and K > 2:
        assert stopped                     # the kind does what it is there for
    if kind in ("lattice", "random"):
        assert some_edge and not stopped


@pytest.mark.parametrize("K", (3, 16, 33))
def test_joint_lists(K):
    """Default, explicit and +inf joint_score against refine_assembly's comprehension; NaN is never a joint, +inf is one under +inf."""
    from puzzlenet_amd import assembly
    for kind in ("random", "nan30", "blocks", "lattice"):
        S, T, max_score = wc.make(kind, 2, K, 200)
        for z in range(2):
            asm = assembly.assemble(S[z], T[z])
            finite = S[z][np.isfinite(S[z])]
            for js in (None, float(np.median(finite)), float(finite.min()), float("inf")):
                rule = assembly.walk_rule(S[z:z + 1], T[z:z + 1], joint_score=js)
                got = _rule_joints(rule)
                assert got == _host_joints(S[z], asm, js), (kind, z, js)
                assert all(not np.isnan(S[z][i, j]) for i, j in got)
    # one +inf and one NaN entry between placed pieces: under joint_score = +inf the first is a joint, the second never
    S, T, _ = wc.make("random", 1, K, 201)
    S[0, 0, 2], S[0, 2, 1] = np.inf, np.nan
    rule = assembly.walk_rule(S, T, joint_score=float("inf"))
    assert rule.placed.all()
    assert _rule_joints(rule) == [(i, j) for i in range(K) for j in range(K) if i != j and (i, j) != (2, 1)]
    assert _rule_joints(rule) == _host_joints(S[0], assembly.assemble(S[0], T[0]), float("inf"))


def test_count_ignores_the_padding():
    """count < K: the entries with i or j >= count are not read, whatever they hold (NaN; -1, which would win every round)."""
    from puzzlenet_amd import assembly
    K = 16
    for kind in wc.KINDS:
        S, T, max_score = wc.make(kind, 3, K, 300)
        counts = np.array([5, 16, 2], dtype=np.int32)
        for fill in (np.nan, -1.0):
            Sp, Tp = S.copy(), T.copy()
            for z, c in enumerate(counts):
                Sp[z, c:, :], Sp[z, :, c:] = fill, fill
                Tp[z, c:, :], Tp[z, :, c:] = fill, fill
            got = assembly.walk_rule(Sp, Tp, count=counts, max_score=max_score)
            for z, c in enumerate(counts):
                want = assembly.walk_rule(S[z:z + 1, :c, :c], T[z:z + 1, :c, :c], max_score=max_score)
                n = int(want.n_edges[0])
                assert got.root[z] == want.root[0] and got.n_edges[z] == n
                assert np.array_equal(got.edges[z, :c - 1], want.edges[0]) and (got.edges[z, c - 1:] == -1).all()
                assert np.array_equal(got.edge_score[z, :c - 1], want.edge_score[0]) and np.isposinf(got.edge_score[z, c - 1:]).all()
                assert np.array_equal(got.G[z, :c], want.G[0]) and np.array_equal(got.G[z, c:], np.tile(np.eye(4), (K - c, 1, 1)))
                assert np.array_equal(got.placed[z, :c], want.placed[0]) and not got.placed[z, c:].any()
                assert _rule_joints(got, z) == _rule_joints(want)


def test_count_out_of_range_gives_no_root():
    from puzzlenet_amd import assembly
    K = 5
    S, T, _ = wc.make("random", 3, K, 400)
    got = assembly.walk_rule(S, T, count=np.array([1, K + 1, K], dtype=np.int32))
    assert got.root[:2].tolist() == [-1, -1] and got.root[2] >= 0 and got.n_edges.tolist() == [0, 0, K - 1]
    for z in range(2):
        assert not got.placed[z].any() and (got.edges[z] == -1).all() and np.isposinf(got.edge_score[z]).all()
        assert got.n_joints[z] == 0 and (got.joints[z] == -1).all()
        assert np.array_equal(got.G[z], np.tile(np.eye(4), (K, 1, 1)))
    whole = assembly.walk_rule(S[2:], T[2:])
    assert all(np.array_equal(a[2], b[0]) for a, b in zip(got, whole))
