"""CPU: assembly.forest_rule - the numpy statement that ops.assemble_forest is held to (tests/test_gpu_assemble_forest.py) - against
what defines it: its components are single linkage (an independent union-find), its first component is walk_rule's result, and where
the walk completes the two agree in every bit.  Then the score of a sorted pile (assembly.evaluate_pile) on a pile whose objects the
forest must recover and on hand-made cases with counts worked out by hand, and datapipe.pile's indexing on CPU tensors.  The table
kinds are those of tests/_walk_cases.py, none of which holds -inf (the single-linkage statement is for tables without it)."""
import numpy as np
import pytest
import torch

from tests import _walk_cases as wc

Z = 4
KS = (2, 3, 5, 8, 17, 64)


def _limits(kind, K):
    _, _, m = wc.make(kind, 1, K, 0)
    return (m,) if m is not None else (None, 0.3, 1.5)


def _cases():
    return [(kind, K, m) for kind in wc.KINDS for K in KS for m in _limits(kind, K)]


@pytest.fixture(scope="module")
def rules():
    """(kind, K, max_score) -> (S, T, forest_rule's, walk_rule's), each computed once."""
    from puzzlenet_amd import assembly
    out = {}
    for kind, K, m in _cases():
        S, T, _ = wc.make(kind, Z, K, 1100)
        out[kind, K, m] = (S, T, assembly.forest_rule(S, T, max_score=m), assembly.walk_rule(S, T, max_score=m))
    return out


def _linkage(S, c, limit):
    """Connected components of the pieces < c under the entries (i, j), i != j, finite and <= limit: union-find -> a label per
    piece, the lowest member."""
    parent = list(range(c))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a
    for i in range(c):
        for j in range(c):
            s = float(S[i, j])
            if i != j and np.isfinite(s) and (limit is None or s <= limit):
                a, b = find(i), find(j)
                parent[max(a, b)] = min(a, b)
    return [find(p) for p in range(c)]


def _partition(labels):
    groups = {}
    for p, l in enumerate(labels):
        groups.setdefault(int(l), set()).add(p)
    return sorted(sorted(g) for g in groups.values())


@pytest.mark.parametrize("kind,K,m", _cases())
def test_components_are_single_linkage(rules, kind, K, m):
    S, _, f, _ = rules[kind, K, m]
    several = 0
    for z in range(Z):
        assert _partition(f.component[z]) == _partition(_linkage(S[z], K, m))
        nc = int(f.n_components[z])
        several += nc > 1
        # the bookkeeping: components in creation order, a root per component in it, an edge per piece that is no root
        assert sorted(set(f.component[z].tolist())) == list(range(nc)) and (f.roots[z, nc:] == -1).all()
        assert [int(f.component[z, r]) for r in f.roots[z, :nc]] == list(range(nc))
        assert int(f.n_edges[z]) == K - nc and f.root[z] == f.roots[z, 0] and f.placed[z].all()
        new = f.edges[z, :K - nc, 2]
        assert sorted(new.tolist() + f.roots[z, :nc].tolist()) == list(range(K))      # every piece goes inside once
        assert (np.diff(f.component[z, new]) >= 0).all()                              # a component is finished before the next
        assert (f.component[z, f.edges[z, :K - nc, 0]] == f.component[z, f.edges[z, :K - nc, 1]]).all()      # the end inside is in it
    if kind in ("blocks", "max_score") and K >= 5:
        assert several > 0                           # the kinds that leave pieces over do so here


@pytest.mark.parametrize("kind,K,m", _cases())
def test_first_component_is_the_walk(rules, kind, K, m):
    _, _, f, w = rules[kind, K, m]
    full = 0
    for z in range(Z):
        n = int(w.n_edges[z])
        assert f.roots[z, 0] == w.root[z]
        assert np.array_equal(f.edges[z, :n], w.edges[z, :n]) and np.array_equal(f.edge_score[z, :n], w.edge_score[z, :n])
        assert np.array_equal(f.component[z] == 0, w.placed[z].astype(bool))
        at = w.placed[z].astype(bool)
        assert np.array_equal(f.G[z][at], w.G[z][at])
        if w.placed[z].all():                        # the walk completes: every shared output, bit for bit
            full += 1
            assert int(f.n_components[z]) == 1
            for name in w._fields:
                assert np.array_equal(getattr(f, name)[z], getattr(w, name)[z]), name
    if kind in ("lattice", "random") and m is None:
        assert full == Z


def test_joints_stay_inside_a_component(rules):
    for (kind, K, m), (S, _, f, _) in rules.items():
        for z in range(Z):
            n = int(f.n_joints[z])
            js = f.joints[z, :n]
            assert (f.joints[z, n:] == -1).all()
            if int(f.n_edges[z]) == 0:
                assert n == 0
                continue
            limit = float(f.edge_score[z, :int(f.n_edges[z])].max())
            want = [(i, j) for i in range(K) for j in range(K)
                    if i != j and f.component[z, i] == f.component[z, j] and float(S[z, i, j]) <= limit]
            assert [tuple(r) for r in js.tolist()] == want


def test_counts():
    """count smaller than K (the padding is never read), counts outside [2, K], and K = 2 both ways."""
    from puzzlenet_amd import assembly
    K = 8
    counts = np.array([8, 5, 2, 1, 9, 0, -2, 3], dtype=np.int32)
    S, T, _ = wc.make("blocks", len(counts), K, 1200)
    pad_S, pad_T = S.copy(), T.copy()
    for z, c in enumerate(counts):
        c = max(int(c), 0)
        pad_S[z, c:, :], pad_S[z, :, c:], pad_T[z, c:, :], pad_T[z, :, c:] = -1.0, -1.0, np.nan, np.nan
    f = assembly.forest_rule(pad_S, pad_T, count=counts)
    for z, c in enumerate(counts):
        if not 2 <= c <= K:
            assert f.root[z] == -1 and f.n_components[z] == 0 and f.n_edges[z] == 0 and f.n_joints[z] == 0
            assert (f.component[z] == -1).all() and (f.roots[z] == -1).all() and not f.placed[z].any()
            assert np.array_equal(f.G[z], np.tile(np.eye(4), (K, 1, 1)))
            continue
        one = assembly.forest_rule(S[z:z + 1, :c, :c], T[z:z + 1, :c, :c])                   # the pile of c pieces on its own
        assert np.array_equal(f.component[z, :c], one.component[0]) and (f.component[z, c:] == -1).all()
        assert np.array_equal(f.G[z, :c], one.G[0]) and np.array_equal(f.placed[z], np.arange(K) < c)
        assert np.array_equal(f.edges[z, :c - 1], one.edges[0]) and f.n_components[z] == one.n_components[0]
        assert np.array_equal(f.joints[z, :int(f.n_joints[z])], one.joints[0, :int(one.n_joints[0])])
    # K = 2: one finite entry joins the two, none leaves two singletons
    S2 = np.array([[[0, np.nan], [0.5, 0]], [[0, np.inf], [np.nan, 0]]], dtype=np.float32)
    f = assembly.forest_rule(S2, wc.rigid(np.random.default_rng(0), (2, 2, 2)))
    assert f.n_components.tolist() == [1, 2] and f.edges[0].tolist() == [[1, 0, 0]] and f.roots.tolist() == [[1, -1], [0, 1]]
    assert f.component.tolist() == [[0, 0], [0, 1]] and f.n_joints.tolist() == [1, 0] and f.joints[0, 0].tolist() == [1, 0]


def test_a_table_of_nan_is_count_singletons():
    from puzzlenet_amd import assembly
    K = 17
    S = np.full((2, K, K), np.nan, dtype=np.float32)
    T = wc.rigid(np.random.default_rng(1), (2, K, K))
    f = assembly.forest_rule(S, T, count=np.array([K, 6]))
    for z, c in enumerate((K, 6)):
        assert f.n_components[z] == c and f.n_edges[z] == 0 and f.n_joints[z] == 0
        assert f.roots[z, :c].tolist() == list(range(c)) and f.component[z, :c].tolist() == list(range(c))
        assert np.array_equal(f.G[z], np.tile(np.eye(4), (K, 1, 1))) and f.placed[z].sum() == c


# --------------------------------------------------------------------------- a pile whose objects the forest recovers

def _synthetic_pile(seed, Q=3, P=4, n=32):
    """Q objects of P pieces under random rigid poses, shuffled -> (pose [K,4,4], rest [K,n,3], object_of [K])."""
    rng = np.random.default_rng(seed)
    K = Q * P
    return wc.rigid(rng, (K,)).astype(np.float64), rng.random((K, n, 3)), (rng.permutation(K) // P).astype(np.int32)


def test_the_forest_recovers_the_objects_of_a_pile():
    from puzzlenet_amd import assembly
    pose, rest, obj = _synthetic_pile(7)
    K = len(obj)
    Tt, St = assembly.truth_table(pose, obj[:, None] == obj[None, :])                # mates complete inside an object
    f = assembly.forest_rule(St[None], Tt[None])
    ev = assembly.evaluate_pile(f.G[0], f.component[0], pose, rest, obj)
    assert ev.exact and ev.n_components == 3 and int(f.n_components[0]) == 3
    assert ev.pair_precision == ev.pair_recall == ev.pair_pose_recall == 1.0
    together = (obj[:, None] == obj[None, :]) & ~np.eye(K, dtype=bool)
    # rounding level: the table is float32, so an entry of T (at most 4 in size) is off by 2^-24 of itself and an edge displaces a
    # point (at most 4 from the origin) by 4 * 4 * 4 * 2^-24 = 4e-6 at most; two pieces of a four-piece object are at most six
    # edges apart through their root: 2.3e-5, squared 5.3e-10
    print("msd inside the objects: max", ev.msd[together].max())
    assert ev.msd[together].max() < 5.3e-10
    # what was missing: the one-tree walk places one object and leaves the rest where it lies
    a = assembly.assemble(St, Tt)
    assert int(a.placed.sum()) == 4 and len(set(obj[a.placed].tolist())) == 1
    w = assembly.evaluate_pile(a.G, np.where(a.placed, 0, -1), pose, rest, obj)
    assert w.pair_precision == 1.0 and w.pair_recall == pytest.approx(1.0 / 3.0) and not w.exact


def test_evaluate_pile_counts():
    """Two objects of three pieces with the truth's poses; the counts are over the 30 ordered pairs, 12 of which belong."""
    from puzzlenet_amd import assembly
    pose, rest, _ = _synthetic_pile(8, Q=2, P=3)
    obj = np.array([0, 1, 0, 1, 1, 0], dtype=np.int32)
    inv = np.stack([np.linalg.inv(x) for x in pose])

    def truth(comp):                                  # every piece in the frame of the first piece of its component
        first = {int(q): int(np.flatnonzero(comp == q)[0]) for q in set(comp.tolist())}
        return np.stack([pose[first[int(comp[p])]] @ inv[p] for p in range(6)])

    right = assembly.evaluate_pile(truth(obj), obj, pose, rest, obj)
    assert right[:5] == (1.0, 1.0, 1.0, 2, True)
    # both objects in one component: 30 pairs together, 12 of them belong
    merged = np.zeros(6, dtype=np.int32)
    ev = assembly.evaluate_pile(truth(merged), merged, pose, rest, obj)
    assert ev[:5] == (12 / 30, 1.0, 1.0, 1, False)
    # object 0 split into {0, 2} and {5}: 2 + 6 pairs together, all belong; 12 belong, 8 of them together
    split = np.array([0, 1, 0, 1, 1, 2], dtype=np.int32)
    ev = assembly.evaluate_pile(truth(split), split, pose, rest, obj)
    assert ev[:5] == (1.0, 8 / 12, 8 / 12, 3, False)
    # the right partition, piece 4 a unit off: the four ordered pairs with piece 4 lose their pose, nothing else
    G = truth(obj)
    G[4, :3, 3] += np.array([1.0, 0.0, 0.0])
    ev = assembly.evaluate_pile(G, obj, pose, rest, obj)
    assert ev[:5] == (1.0, 1.0, 8 / 12, 2, True)
    assert ev.msd[1, 4] == pytest.approx(1.0) and ev.msd[4, 1] == pytest.approx(1.0) and ev.msd[1, 3] < 1e-12      # (float32 rotations: orthogonal to 1e-7)
    # count = 4: pieces 0 .. 3, two pairs of two; no pair at all gives NaN
    ev = assembly.evaluate_pile(truth(obj), obj, pose, rest, obj, count=4)
    assert ev[:5] == (1.0, 1.0, 1.0, 2, True)
    none = assembly.evaluate_pile(truth(obj), np.arange(6), pose, rest, np.arange(6))
    assert np.isnan(none.pair_precision) and np.isnan(none.pair_recall) and np.isnan(none.pair_pose_recall) and none.exact
    with pytest.raises(ValueError):
        assembly.evaluate_pile(G[:5], obj, pose, rest, obj)


def test_pile_indexing_on_cpu_tensors():
    """datapipe.pile on a Fracture-shaped tuple of CPU tensors: B = 4 samples of P = 3 pieces into Z = 2 piles of Q = 2 objects."""
    from puzzlenet_amd import datapipe
    B, P, n, Q = 4, 3, 5, 2
    Zp, K = B // Q, Q * P
    g = torch.Generator().manual_seed(9)
    tag = torch.arange(B * P, dtype=torch.float32).view(B, P)                        # piece (b, p) carries the number b P + p
    pieces = tag[:, :, None, None].expand(B, P, n, 3).contiguous()
    pose = tag[:, :, None, None].expand(B, P, 4, 4).contiguous() + 0.5
    rest = pieces + 0.25
    cd = torch.rand(B, P, P, generator=g)
    mates = torch.rand(B, P, P, generator=g) < 0.5
    ok = torch.tensor([True, True, False, True])
    blank = torch.zeros(1)
    frac = datapipe.Fracture(pieces, pose, rest, blank, blank, cd, mates, ok, blank, blank, blank, blank, blank)
    perm = torch.stack([torch.randperm(K, generator=g) for _ in range(Zp)])
    for pm in (perm, None):
        pl = datapipe.pile(frac, objects=Q, perm=pm)
        src = perm if pm is not None else torch.arange(K).expand(Zp, K)
        assert pl.pieces.shape == (Zp, K, n, 3) and pl.pose.shape == (Zp, K, 4, 4) and pl.mates.shape == (Zp, K, K)
        assert pl.source.dtype == torch.int32 and pl.object_of.dtype == torch.int32 and pl.mates.dtype == torch.bool
        assert torch.equal(pl.source.long(), src) and torch.equal(pl.object_of.long(), src // P)
        assert pl.ok.tolist() == [True, False]
        for z in range(Zp):
            for a in range(K):
                qa, pa = divmod(int(src[z, a]), P)
                b = z * Q + qa
                assert float(pl.pieces[z, a, 0, 0]) == b * P + pa and float(pl.pose[z, a, 0, 0]) == b * P + pa + 0.5
                assert float(pl.rest[z, a, 0, 0]) == b * P + pa + 0.25
                for c in range(K):
                    qc, pc = divmod(int(src[z, c]), P)
                    if qa == qc:
                        assert bool(pl.mates[z, a, c]) == bool(mates[b, pa, pc]) and float(pl.cd[z, a, c]) == float(cd[b, pa, pc])
                    else:
                        assert not bool(pl.mates[z, a, c]) and float(pl.cd[z, a, c]) == float("inf")
    with pytest.raises(datapipe._lib.PznError):
        datapipe.pile(frac, objects=3)
    with pytest.raises(datapipe._lib.PznError):
        datapipe.pile(frac, objects=Q, perm=perm[:1])
    with pytest.raises(datapipe._lib.PznError):
        datapipe.pile(frac, objects=Q, perm=perm.int())
