"""CPU: assembly.forest_beam_rule - the numpy statement the device forest beam (ops.assemble_forest_beam) is held to bit for
bit - against forest_rule at beam = branch = 1, against beam_rule on tables without a restart, against its own invariants and a
replay of its result's edges and restarts in Python floats, and on piles of planted objects, where the forest walk fails and the
forest beam does not.  Tables: tests/_beam_cases.py, tests/_forest_beam_cases.py."""
import numpy as np
import pytest

from tests import _beam_cases as bc
from tests import _forest_beam_cases as fb

SIZES = (2, 3, 5, 8)
FOREST_FIELDS = ("root", "edges", "edge_score", "n_edges", "G", "placed", "joints", "n_joints", "component", "roots", "n_components")
BEAM_FIELDS = ("root", "edges", "edge_score", "n_edges", "G", "placed", "joints", "n_joints", "cost", "n_hyp")


def _same_fields(got, want, names, note):
    for name in names:
        g, w = getattr(got, name), getattr(want, name)
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (name, note)


@pytest.mark.parametrize("kind", bc.KINDS)
@pytest.mark.parametrize("K", SIZES)
def test_beam_one_branch_one_is_the_forest_walk(K, kind):
    """Identity 1: B = C = 1 equals forest_rule on every one of its fields, bit for bit, whatever the weight."""
    from puzzlenet_amd import assembly
    Z = 6
    S, T, M, max_score = bc.make(kind, Z, K, 100)
    for count in (None, bc.ragged(Z, K)):
        want = assembly.forest_rule(S, T, count=count, max_score=max_score)
        for weight in (0.0, 1.0, 7.5):
            got = assembly.forest_beam_rule(S, T, M, count=count, beam=1, branch=1, weight=weight, max_score=max_score)
            assert got._fields == FOREST_FIELDS + ("cost", "n_hyp")
            _same_fields(got, want, FOREST_FIELDS, weight)
            assert got.cost.shape == (Z, 1) and got.cost.dtype == np.float64 and got.n_hyp.dtype == np.int32
            assert np.array_equal(got.n_hyp, (want.root >= 0).astype(np.int32))
        if count is not None:
            assert want.root[[1, 3]].tolist() == [-1, -1] and np.isposinf(got.cost[[1, 3]]).all()
            assert got.n_components[[1, 3]].tolist() == [0, 0] and (got.component[[1, 3]] == -1).all()


@pytest.mark.parametrize("kind", ("random", "lattice", "planted"))
@pytest.mark.parametrize("K", (3, 5, 8))
def test_without_a_restart_it_is_the_beam(K, kind):
    """Identity 2: no live hypothesis ever lacks a candidate -> the ten shared fields are beam_rule's and there is one component."""
    from puzzlenet_amd import assembly
    Z = 6
    S, T, M, _ = bc.make(kind, Z, K, 150)
    for count in (None, bc.ragged(Z, K)):
        for B, C in ((4, 4), (3, 5), (8, 8)):
            for weight in (0.0, 1.0):
                kw = dict(count=count, beam=B, branch=C, weight=weight, max_score=None)
                want = assembly.beam_rule(S, T, M, **kw)
                got = assembly.forest_beam_rule(S, T, M, **kw)
                _same_fields(got, want, BEAM_FIELDS, (B, C, weight))
                assert np.array_equal(got.n_components, (want.root >= 0).astype(np.int32))
    # hence beam = branch = 1 on such a table is the walk
    walk = assembly.walk_rule(S, T)
    _same_fields(assembly.forest_beam_rule(S, T, M, beam=1, branch=1), walk, BEAM_FIELDS[:8], "walk")


def _replay(S, T, M, K, c, edges, component, roots, weight, vlimit, charge):
    """The cost and the poses of a hypothesis from its own edges and restarts, in Python floats with assembly's scalar helpers:
    _replay_cost of tests/test_assembly_beam_cpu.py with the voters of the joined component alone and `charge` per restart.  The
    order of placements is recovered from the result: an edge is placed as soon as its inside end is, a root when no edge can be
    (on a table without -inf a restart's next edge starts in the new component, so this is the order the rule went through)."""
    from puzzlenet_amd.assembly import _dot4, _rule_inverse, _rule_product
    inf = float("inf")
    key = lambda a, b: inf if (a == b or S[a, b] != S[a, b]) else float(S[a, b]) + 0.0
    Tf = lambda a, b: T[a, b].astype(np.float64).tolist()
    eye = [[1.0 if u == v else 0.0 for v in range(4)] for u in range(4)]
    pose, comp = {int(roots[0]): eye}, {int(roots[0]): 0}
    cost, e, q = 0.0, 0, 1
    while len(pose) < c:
        if e < len(edges) and (edges[e][0] if edges[e][2] == edges[e][1] else edges[e][1]) in pose:
            i, j, new = edges[e]
            e += 1
            old = i if new == j else j
            Gn = _rule_product(pose[i], Tf(i, j)) if new == j else _rule_product(pose[j], _rule_inverse(Tf(i, j)))
            cost = cost + key(i, j)
            if weight != 0.0:
                total, votes = 0.0, 0
                Mn = M[new].tolist()
                for p in sorted(pose):
                    if comp[p] != comp[old]:
                        continue
                    for a, b in ((p, new), (new, p)):
                        if (a, b) == (i, j) or not np.isfinite(key(a, b)) or key(a, b) > vlimit:
                            continue
                        Q = _rule_product(pose[p], Tf(a, b) if a == p else _rule_inverse(Tf(a, b)))
                        qs = []
                        for u in range(3):
                            D = [Q[u][v] - Gn[u][v] for v in range(4)]
                            m = [_dot4(Mn[v][0], D[0], Mn[v][1], D[1], Mn[v][2], D[2], Mn[v][3], D[3]) for v in range(4)]
                            qs.append(_dot4(D[0], m[0], D[1], m[1], D[2], m[2], D[3], m[3]))
                        total = total + ((qs[0] + qs[1]) + qs[2])
                        votes += 1
                cost = cost + weight * (total / votes if votes else 0.0)
            pose[new], comp[new] = Gn, comp[old]
        else:
            new = int(roots[q])
            cost = cost + charge
            pose[new], comp[new] = eye, q
            q += 1
        cost = inf if cost != cost else cost
    assert e == len(edges) and q == len(roots)
    return cost, pose, comp


def _tables(kind, Z, K, seed):
    if kind == "pile":                                   # piles of two objects of max(2, K // 2) pieces, with their threshold
        return fb.piles(range(seed, seed + Z), 2, max(2, K // 2))[:3] + (fb.MAX_SCORE,)
    return bc.make(kind, Z, K, seed)


@pytest.mark.parametrize("kind", bc.KINDS + ("pile",))
@pytest.mark.parametrize("K", SIZES)
def test_invariants_and_replay(K, kind):
    from puzzlenet_amd import assembly
    Z = 6
    S, T, M, max_score = _tables(kind, Z, K, 200)
    K = S.shape[1]
    count = bc.ragged(Z, K)
    limit = float("inf") if max_score is None else max_score
    charge = limit if np.isfinite(limit) else 0.0
    for B, C, weight in ((4, 4, 1.0), (3, 5, 0.0), (8, 8, 1.0)):
        got = assembly.forest_beam_rule(S, T, M, count=count, beam=B, branch=C, weight=weight, max_score=max_score)
        for z in range(Z):
            c, n, h, nc = int(count[z]), int(got.n_edges[z]), int(got.n_hyp[z]), int(got.n_components[z])
            if not 2 <= c <= K:
                assert h == 0 and nc == 0 and got.root[z] == -1 and np.isposinf(got.cost[z]).all() and n == 0
                assert not got.placed[z].any() and (got.component[z] == -1).all() and (got.roots[z] == -1).all()
                continue
            assert 1 <= h <= B and n + nc == c
            assert got.placed[z, :c].all() and not got.placed[z, c:].any()
            roots = got.roots[z, :nc].tolist()
            assert len(set(roots)) == nc and (got.roots[z, nc:] == -1).all() and got.root[z] == roots[0]
            assert [int(got.component[z, r]) for r in roots] == list(range(nc))
            assert (got.component[z, :c] >= 0).all() and (got.component[z, c:] == -1).all()
            live = got.cost[z, :h]
            assert not np.isnan(live).any() and (np.diff(live) >= 0).all() and np.isposinf(got.cost[z, h:]).all()
            assert (got.edges[z, n:] == -1).all() and np.isposinf(got.edge_score[z, n:]).all()
            edges = got.edges[z, :n].tolist()
            cost, pose, comp = _replay(S[z], T[z], M[z], K, c, edges, got.component[z], roots, weight, limit, charge)
            assert cost == got.cost[z, 0], (z, cost, got.cost[z, 0])
            assert sorted(pose) == list(range(c)) and [comp[p] for p in range(c)] == got.component[z, :c].tolist()
            for p, g in pose.items():
                assert np.array_equal(got.G[z, p], np.array(g))
            assert np.array_equal(got.G[z, c:], np.tile(np.eye(4), (K - c, 1, 1)))
            # every edge joins an inside piece to an outside one, and the new piece takes the inside end's component
            inside = set()
            for i, j, new in edges:
                old = i if new == j else j
                assert new in (i, j) and new not in inside and new not in roots
                assert got.component[z, new] == got.component[z, old]
                inside.add(new)
            assert len(inside) == n
            for i, j in got.joints[z, :int(got.n_joints[z])].tolist():      # no joint crosses components
                assert i != j and got.component[z, i] == got.component[z, j]
            assert (got.joints[z, int(got.n_joints[z]):] == -1).all()


def test_restart_cost():
    from puzzlenet_amd import assembly
    S, T, M, max_score = bc.make("max_score", 4, 8, 300)
    kw = dict(beam=4, branch=4, max_score=max_score)
    default = assembly.forest_beam_rule(S, T, M, **kw)
    assert (default.n_components > 1).any()
    for same in (float("nan"), None, max_score):         # NaN and None are the explicit default
        got = assembly.forest_beam_rule(S, T, M, restart_cost=same, **kw)
        assert all(np.array_equal(a, b) for a, b in zip(got, default))
    big = assembly.forest_beam_rule(S, T, M, restart_cost=1000.0, **kw)
    assert not np.array_equal(big.cost, default.cost)
    assert (big.cost[:, 0] >= 1000.0 * (big.n_components - 1)).all()
    # a large charge changes the cost and not identity 1
    want = assembly.forest_rule(S, T, max_score=max_score)
    one = assembly.forest_beam_rule(S, T, M, beam=1, branch=1, max_score=max_score, restart_cost=1000.0)
    _same_fields(one, want, FOREST_FIELDS, "restart_cost = 1000")
    assert not np.array_equal(one.cost, assembly.forest_beam_rule(S, T, M, beam=1, branch=1, max_score=max_score).cost)
    # without a threshold a restart happens only at a wall of non-finite keys and is free: two blocks, the cost of the edges alone
    S, T, M, _ = bc.make("blocks", 4, 8, 310)
    free = assembly.forest_beam_rule(S, T, M, weight=0.0)
    zero = assembly.forest_beam_rule(S, T, M, weight=0.0, restart_cost=0.0)
    assert free.n_components.tolist() == [2] * 4 and all(np.array_equal(a, b) for a, b in zip(free, zero))
    for z in range(4):
        total = 0.0
        for s in free.edge_score[z, :int(free.n_edges[z])].tolist():
            total = total + s
        assert total == free.cost[z, 0]


# seeds 0..19 of pile(seed, Q, P): seeds at which the rule does not show both the forest walk wrong and the default forest beam
# right would be listed here per (Q, P) (at least 16 of the 20 must stay); none had to be.
# For the record and not asserted: at (3, 5) the forest walk is right on 0 of 20 piles and the default forest beam on 18 (seeds 3
# and 4 fail).
PILES_DROPPED = {(2, 6): (), (2, 8): ()}


def _pile_right(S, T, M, max_score, pose, object_of, beam):
    from puzzlenet_amd import assembly
    if beam:
        got = assembly.forest_beam_rule(S[None], T[None], M[None], max_score=max_score)
    else:
        got = assembly.forest_rule(S[None], T[None], max_score=max_score)
    return fb.right(got.G[0], got.component[0], got.roots[0], got.n_components[0], pose, object_of)


@pytest.mark.parametrize("QP", sorted(PILES_DROPPED))
def test_planted_piles(QP):
    Q, P = QP
    seeds = [s for s in range(20) if s not in PILES_DROPPED[QP]]
    assert len(seeds) >= 16
    forest_right, beam_right = [], []
    for seed in seeds:
        S, T, M, pose, object_of, max_score = fb.pile(seed, Q, P)
        forest_right.append(_pile_right(S, T, M, max_score, pose, object_of, False))
        beam_right.append(_pile_right(S, T, M, max_score, pose, object_of, True))
    print(f"piles {QP}: forest walk right", forest_right, "forest beam right", beam_right)
    assert not any(forest_right), [s for s, ok in zip(seeds, forest_right) if ok]
    assert all(beam_right), [s for s, ok in zip(seeds, beam_right) if not ok]
