"""CPU: assembly.beam_rule - the numpy statement the device beam walk (ops.assemble_beam) is held to bit for bit - against
assembly.walk_rule at beam = branch = 1, against its own invariants, against a replay of its result's edges in Python floats,
and on planted false matches, where the greedy walk fails and the votes do not.  Tables: tests/_beam_cases.py."""
import numpy as np
import pytest

from tests import _beam_cases as bc

SIZES = (2, 3, 5, 8)
WALK_FIELDS = ("root", "edges", "edge_score", "n_edges", "G", "placed", "joints", "n_joints")


@pytest.mark.parametrize("kind", bc.KINDS)
@pytest.mark.parametrize("K", SIZES)
def test_beam_one_branch_one_is_the_walk(K, kind):
    """B = C = 1 equals walk_rule on every shared field, bit for bit, whatever the weight; ragged counts with 0, 1 and K."""
    from puzzlenet_amd import assembly
    Z = 6
    S, T, M, max_score = bc.make(kind, Z, K, 100)
    for count in (None, bc.ragged(Z, K)):
        want = assembly.walk_rule(S, T, count=count, max_score=max_score)
        for weight in (0.0, 1.0, 7.5):
            got = assembly.beam_rule(S, T, M, count=count, beam=1, branch=1, weight=weight, max_score=max_score)
            for name in WALK_FIELDS:
                g, w = getattr(got, name), getattr(want, name)
                assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (name, weight)
            assert got.cost.shape == (Z, 1) and got.cost.dtype == np.float64 and got.n_hyp.dtype == np.int32
            assert np.array_equal(got.n_hyp, (want.root >= 0).astype(np.int32))
        if count is not None:
            assert want.root[[1, 3]].tolist() == [-1, -1] and np.isposinf(got.cost[[1, 3]]).all()


def _replay_cost(S, T, M, K, edges, root, weight, vlimit):
    """The cost of a hypothesis from its own edges, in Python floats with assembly's scalar helpers."""
    from puzzlenet_amd.assembly import _dot4, _rule_inverse, _rule_product
    inf = float("inf")
    key = lambda a, b: inf if (a == b or S[a, b] != S[a, b]) else float(S[a, b]) + 0.0
    Tf = lambda a, b: T[a, b].astype(np.float64).tolist()
    pose = {int(root): [[1.0 if u == v else 0.0 for v in range(4)] for u in range(4)]}
    cost = 0.0
    for i, j, new in edges:
        Gn = _rule_product(pose[i], Tf(i, j)) if new == j else _rule_product(pose[j], _rule_inverse(Tf(i, j)))
        cost = cost + key(i, j)
        if weight != 0.0:
            total, votes = 0.0, 0
            Mn = M[new].tolist()
            for p in sorted(pose):
                for a, b in ((p, new), (new, p)):
                    if (a, b) == (i, j) or not np.isfinite(key(a, b)) or key(a, b) > vlimit:
                        continue
                    Q = _rule_product(pose[p], Tf(a, b) if a == p else _rule_inverse(Tf(a, b)))
                    q = []
                    for u in range(3):
                        D = [Q[u][v] - Gn[u][v] for v in range(4)]
                        m = [_dot4(Mn[v][0], D[0], Mn[v][1], D[1], Mn[v][2], D[2], Mn[v][3], D[3]) for v in range(4)]
                        q.append(_dot4(D[0], m[0], D[1], m[1], D[2], m[2], D[3], m[3]))
                    total = total + ((q[0] + q[1]) + q[2])
                    votes += 1
            cost = cost + weight * (total / votes if votes else 0.0)
        cost = inf if cost != cost else cost
        pose[new] = Gn
    return cost, pose


@pytest.mark.parametrize("kind", bc.KINDS)
@pytest.mark.parametrize("K", SIZES)
def test_invariants_and_replayed_cost(K, kind):
    from puzzlenet_amd import assembly
    Z = 6
    S, T, M, max_score = bc.make(kind, Z, K, 200)
    count = bc.ragged(Z, K)
    for B, C, weight in ((4, 4, 1.0), (3, 5, 0.0), (8, 8, 1.0)):
        got = assembly.beam_rule(S, T, M, count=count, beam=B, branch=C, weight=weight, max_score=max_score)
        for z in range(Z):
            c, n, h = int(count[z]), int(got.n_edges[z]), int(got.n_hyp[z])
            if not 2 <= c <= K:
                assert h == 0 and got.root[z] == -1 and np.isposinf(got.cost[z]).all() and n == 0 and not got.placed[z].any()
                continue
            assert 1 <= h <= B
            live = got.cost[z, :h]
            assert not np.isnan(live).any() and (np.diff(live) >= 0).all() and np.isposinf(got.cost[z, h:]).all()
            assert int(got.placed[z].sum()) == n + 1 and not got.placed[z, c:].any() and n <= c - 1
            assert (got.edges[z, n:] == -1).all() and np.isposinf(got.edge_score[z, n:]).all()
            limit = float("inf") if max_score is None else max_score
            cost, pose = _replay_cost(S[z], T[z], M[z], K, got.edges[z, :n].tolist(), got.root[z], weight, limit)
            assert cost == got.cost[z, 0] or (cost == 0.0 and got.cost[z, 0] == 0.0), (z, cost, got.cost[z, 0])
            for p, g in pose.items():
                assert got.placed[z, p] and np.array_equal(got.G[z, p], np.array(g))
            for p in np.flatnonzero(got.placed[z] == 0):
                assert np.array_equal(got.G[z, p], np.eye(4))
            # every edge joined the placed set to a piece outside it
            inside = {int(got.root[z])}
            for i, j, new in got.edges[z, :n].tolist():
                assert (new == j and i in inside and j not in inside) or (new == i and j in inside and i not in inside)
                inside.add(new)


def test_vote_score_limits_the_voters():
    """A vote_score below every score leaves no voter: the costs are those of weight 0; NaN means max_score."""
    from puzzlenet_amd import assembly
    S, T, M, _ = bc.make("random", 3, 5, 300)
    none = assembly.beam_rule(S, T, M, beam=4, branch=4, weight=1.0, vote_score=-1.0)
    plain = assembly.beam_rule(S, T, M, beam=4, branch=4, weight=0.0)
    assert all(np.array_equal(a, b) for a, b in zip(none, plain))
    a = assembly.beam_rule(S, T, M, max_score=0.6, vote_score=float("nan"))
    b = assembly.beam_rule(S, T, M, max_score=0.6, vote_score=0.6)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    c = assembly.beam_rule(S, T, M, max_score=0.6, vote_score=0.3)
    assert not np.array_equal(b.cost, c.cost)


def _right(G, placed, root, pose, tol=0.05):
    """Every piece placed and every entry of its pose within tol of the truth pose[root] inv(pose[p])."""
    truth = np.einsum("ab,pbc->pac", pose[root], bc._rigid_inv(pose))
    return bool(placed.all()) and bool((np.abs(G - truth) <= tol).all())


# seeds 0..19 of planted(P = 8, 2 false entries, every pair mates); a prototype of the rule with numpy matmul products gave the
# greedy walk 0 of 40 puzzles right and the default beam 40 of 40.  Seeds at which the exact rule does not show both would be
# listed here (at least 16 of the 20 must stay); none had to be.
PLANTED_DROPPED = ()


def test_planted_false_matches():
    from puzzlenet_amd import assembly
    seeds = [s for s in range(20) if s not in PLANTED_DROPPED]
    assert len(seeds) >= 16
    walk_right, beam_right = [], []
    for seed in seeds:
        S, T, M, pose, _ = bc.planted(1, 8, seed, nfalse=2, share=1.0)
        w = assembly.walk_rule(S, T)
        b = assembly.beam_rule(S, T, M)
        walk_right.append(_right(w.G[0], w.placed[0], int(w.root[0]), pose[0]))
        beam_right.append(_right(b.G[0], b.placed[0], int(b.root[0]), pose[0]))
    print("planted: walk right", walk_right, "beam right", beam_right)
    assert not any(walk_right), [s for s, ok in zip(seeds, walk_right) if ok]
    assert all(beam_right), [s for s, ok in zip(seeds, beam_right) if not ok]
