"""No GPU: assembly.progressive_joints_rule - the numpy statement that csrc/progjoints.hip is held to - on simulated ledgers, on
exact ties and, end to end with the float64 loop of tests/_joint_ref.py, on puzzles whose contacts are planted
(tests/_progressive_joints.py says what they are, and why both sides of a contact hold the same samples)."""
import numpy as np
import pytest

from puzzlenet_amd import assembly
from tests import _joint_counts as jc
from tests import _joint_ref as jr
from tests import _progressive_joints as pj

SWEEPS = 30
SHAPES = [(3, 4, 64, 16), (2, 5, 96, 20), (4, 6, 32, 24)]      # (Z, P, N, k)


def _sim(n, shape):
    return pj.simulate(np.random.default_rng(5100 + n), *shape)


def _slot(p, q):
    lo, hi = min(p, q), max(p, q)
    return hi * (hi - 1) // 2 + lo


def _plain_sets(sim, r, z):
    """The sets of round r of puzzle z -> {(p, q): (rows of A, rows of B)}, p fixed and q moved; a pair with one empty side has
    an empty list there."""
    lists, moved = [], []
    for s in range(2):
        lst = sim.dropped[r, z, s]
        lst = lst[lst[:, 0] >= 0]
        lists.append(lst)
        moved.append(np.stack([sim.G[z, p, :3, :3] @ sim.pieces[z, p, n].astype(np.float64) + sim.G[z, p, :3, 3] for p, n in lst])
                     if len(lst) else np.zeros((0, 3)))
    sets = {}
    if len(lists[0]) and len(lists[1]):
        for s in range(2):
            D = ((moved[s][:, None, :] - moved[1 - s][None, :, :]) ** 2).sum(-1)
            for (piece, row), near in zip(lists[s], D.argmin(axis=1)):
                there = int(lists[1 - s][near, 0])
                pq = (int(piece), there) if s == 0 else (there, int(piece))
                sets.setdefault(pq, ([], []))[s].append(int(row))
    return sets


@pytest.mark.parametrize("n", range(len(SHAPES)))
def test_rule_properties_on_simulated_ledgers(n):
    Z, P, N, k = SHAPES[n]
    sim = _sim(n, SHAPES[n])
    joints, a, b, na, nb, rows_a, rows_b = assembly.progressive_joints_rule(sim.pieces, sim.G, sim.dropped, least=1)
    J = P * (P - 1) // 2
    assert joints.shape == (Z, J, 2) and a.shape == b.shape == (Z, J, k, 3) and na.shape == nb.shape == (Z, J)
    assert rows_a.shape == rows_b.shape == (Z, J, k)
    assert (joints.dtype, a.dtype, na.dtype, rows_a.dtype) == (np.int32, np.float32, np.int32, np.int64)
    seen = 0
    for z in range(Z):
        for e in range(J):
            p, q = (int(v) for v in joints[z, e])
            if p < 0:
                assert q == -1 and na[z, e] == nb[z, e] == 0 and not a[z, e].any() and not b[z, e].any()
                assert (rows_a[z, e] == -1).all() and (rows_b[z, e] == -1).all()
                continue
            seen += 1
            assert e == _slot(p, q) and (min(p, q), max(p, q)) in sim.opposite[z]
            # direction: p on the fixed side and q on the moved side of the one round that holds both
            rounds = [r for r in range(P - 1) if p in sim.dropped[r, z, 0, :, 0] and q in sim.dropped[r, z, 1, :, 0]]
            assert len(rounds) == 1
            r = rounds[0]
            for piece, s, rows, cnt, pts in ((p, 0, rows_a, na, a), (q, 1, rows_b, nb, b)):
                m = int(cnt[z, e])
                assert 1 <= m <= k and (rows[z, e, m:] == -1).all() and not pts[z, e, m:].any()
                assert np.array_equal(pts[z, e, :m], sim.pieces[z, piece, rows[z, e, :m]])
                # the set is a subsequence of the round's list, in list order
                listed = [int(ro) for pi, ro in sim.dropped[r, z, s] if pi == piece]
                it = iter(listed)
                assert all(any(x == y for y in it) for x in rows[z, e, :m].tolist())
    assert seen > 0
    # the sets restated plainly (matrix products, one argmin per entry): every valid entry is in exactly one set of its round, so
    # per round and piece the sizes of its sets sum to its valid entries; the rule emits the pairs whose two sets are both
    # non-empty (least = 1), with exactly those rows
    for z in range(Z):
        for r in range(P - 1):
            sets = _plain_sets(sim, r, z)
            for s in range(2):
                lst = sim.dropped[r, z, s]
                for piece in set(lst[:, 0].tolist()) - {-1}:
                    sizes = sum(len(v[s]) for (p, q), v in sets.items() if (p, q)[s] == piece)
                    assert sizes == int((lst[:, 0] == piece).sum()), (z, r, s, piece)
            for (p, q), (A, B) in sets.items():
                e = _slot(p, q)
                if A and B:
                    assert joints[z, e].tolist() == [p, q] and rows_a[z, e, :na[z, e]].tolist() == A \
                        and rows_b[z, e, :nb[z, e]].tolist() == B, (z, r, p, q)
                else:
                    assert joints[z, e].tolist() == [-1, -1], (z, r, p, q)


def test_invalid_entries_and_empty_rounds_are_ignored():
    sim = _sim(0, SHAPES[0])
    Z, P, N, k = SHAPES[0]
    want = assembly.progressive_joints_rule(sim.pieces, sim.G, sim.dropped, least=2)
    assert (sim.dropped[:, :, :, :, 0] == -1).any() and any((sim.dropped[r, z] == -1).all() for r in range(P - 1) for z in range(Z))
    # -1 padding replaced by other invalid entries: a piece of P, a row of N, a negative row; and the padding moved about
    rng = np.random.default_rng(3)
    other = sim.dropped.copy()
    pad = other[..., 0] == -1
    kind = rng.integers(0, 3, size=pad.shape)
    other[pad & (kind == 0)] = (P, 0)
    other[pad & (kind == 1)] = (0, N)
    other[pad & (kind == 2)] = (1, -5)
    for x, y in zip(want, assembly.progressive_joints_rule(sim.pieces, sim.G, other, least=2)):
        assert np.array_equal(x, y)
    # a round whose moved side is all padding yields nothing, whatever its fixed side holds
    holed = sim.dropped.copy()
    holed[0, :, 1] = -1
    got = assembly.progressive_joints_rule(sim.pieces, sim.G, holed, least=1)
    rest = assembly.progressive_joints_rule(sim.pieces, sim.G, holed[1:], least=1)
    for x, y in zip(got, rest):
        assert np.array_equal(x, y)
    # a ledger of -1 alone: every output at its fill value
    joints, a, b, na, nb, rows_a, rows_b = assembly.progressive_joints_rule(sim.pieces, sim.G, np.full_like(sim.dropped, -1))
    assert (joints == -1).all() and not a.any() and not b.any() and not na.any() and not nb.any()
    assert (rows_a == -1).all() and (rows_b == -1).all()


@pytest.mark.parametrize("n", range(len(SHAPES)))
def test_least_drops_exactly_the_joints_below_it(n):
    sim = _sim(n, SHAPES[n])
    free = assembly.progressive_joints_rule(sim.pieces, sim.G, sim.dropped, least=1)
    counts = sorted(set(free[3][free[0][..., 0] >= 0].tolist()) | set(free[4][free[0][..., 0] >= 0].tolist()))
    assert len(counts) > 2
    for least in (counts[1], counts[len(counts) // 2], counts[-1] + 1):
        got = assembly.progressive_joints_rule(sim.pieces, sim.G, sim.dropped, least=least)
        stays = (free[3] >= least) & (free[4] >= least)
        assert stays.any() == (least <= counts[-1]) or not stays.any()
        for x, y, fill in zip(got, free, (-1, 0, 0, 0, 0, -1, -1)):
            assert np.array_equal(x[stays], y[stays]) and (x[~stays] == fill).all()


def test_ties_go_to_the_lowest_position():
    pieces, G, dropped, want = pj.lattice()
    joints, a, b, na, nb, rows_a, rows_b = assembly.progressive_joints_rule(pieces, G, dropped, least=3)
    n = len(want)
    assert joints[0].tolist() == [[0, 1], [0, 2], [1, 2]] and na[0].tolist() == [n, n, n] and nb[0].tolist() == [n, n // 2, n // 2]
    assert rows_b[0, 1, :n // 2].tolist() == [y for y in range(n) if want[y] == 0]
    assert rows_b[0, 2, :n // 2].tolist() == [y for y in range(n) if want[y] == 1]
    assert rows_a[0, 1, :n].tolist() == list(range(n)) and rows_a[0, 2, :n].tolist() == list(range(n))
    # least above the halves: the two joints of round 1 go, round 0's stays
    joints = assembly.progressive_joints_rule(pieces, G, dropped, least=n // 2 + 1)[0]
    assert joints[0].tolist() == [[0, 1], [-1, -1], [-1, -1]]


def test_frames_and_movable_of_a_walk_that_stopped_with_several_parts():
    # pieces 0..5: 3 joins 1, then 4 joins 0, then {1, 3} joins 5; piece 2 stays single: parts {0, 4}, {5, 1, 3}, {2}
    edges = [(1, 3, 0.1, None, None), (0, 4, 0.2, None, None), (5, 1, 0.3, None, None)]
    frame = assembly.progressive_frames(6, edges)
    assert frame.tolist() == [0, 5, 2, 5, 0, 5]
    assert (frame != np.arange(6)).tolist() == [False, True, False, True, True, False]
    # the simulated walks' own part is what the edges rebuild (labels = any member: here the slots)
    sim = _sim(2, SHAPES[2])
    Z, P, N, k = SHAPES[2]
    several = 0
    for z in range(Z):
        edges = []
        for r in range(P - 1):
            f, m = (sorted(set(sim.dropped[r, z, s, :, 0].tolist()) - {-1}) for s in range(2))
            if f:
                edges.append((f[0], m[0]))
        part = assembly.progressive_frames(P, edges)
        # a frame piece is a member of its part; the partition is the walk's
        assert all(part[part[p]] == part[p] for p in range(P))
        assert all((part[p] == part[q]) == (sim.part[z, p] == sim.part[z, q]) for p in range(P) for q in range(P))
        several += len(set(part.tolist())) > 1
    assert several > 0


def test_assemble_tool_names_the_table_walk_options(tmp_path):
    """tools/assemble.py --progressive --joint N no longer exits on the pair of options; --joint-keep / --joint-auto beside
    --progressive do, with a message that says where they belong (all before the tool asks for a GPU)."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    run = lambda *args: subprocess.run([sys.executable, os.path.join(root, "tools", "assemble.py"), "--pieces", str(tmp_path / "none.npy"),
                                        "--progressive", "--joint", "5", *args], capture_output=True, text=True)
    for extra in (("--joint-keep", "0.5"), ("--joint-auto",)):
        out = run(*extra)
        assert out.returncode != 0 and "table walks" in out.stderr and "refine_progressive" in out.stderr, out.stderr
    out = run()
    assert "not with --progressive" not in out.stderr and "table walks" not in out.stderr, out.stderr


@pytest.fixture(scope="module")
def end_to_end():
    out = {}
    for K, seed in pj.CASES:
        pl = pj.planted(K, seed)
        outputs = assembly.progressive_joints_rule(pl.pieces[None], pl.G0[None], pl.dropped[:, None], least=3)
        P, used = pj.as_puzzle(pl, outputs)
        out[K, seed] = (pl, outputs, P, jr.refine(P, SWEEPS))
    return out


def test_which_puzzles_the_margin_rule_lets_into_the_short_trajectory_check():
    """The float64 side of tests/test_gpu_progressive_joints.py's trajectory comparison: at M = 40 no puzzle enters, at SHORT_M
    pj.SHORT_ENTERED of 24 do."""
    entered = {pj.M: 0, pj.SHORT_M: 0}
    for m in entered:
        for K, seed in pj.CASES:
            pl = pj.planted(K, seed, m=m)
            outputs = assembly.progressive_joints_rule(pl.pieces[None], pl.G0[None], pl.dropped[:, None], least=3)
            entered[m] += pj.short_trajectory(pl, outputs, jc.TRAJECTORY_SWEEPS, jc.MARGIN_FACTOR)[1]
    assert entered == {pj.M: 0, pj.SHORT_M: pj.SHORT_ENTERED} and 4 * pj.SHORT_ENTERED >= 3 * len(pj.CASES), entered


def test_planted_contacts_are_found_and_the_float64_loop_closes_them(end_to_end):
    """Every condition holds for every one of the 24 puzzles; none is left out."""
    for (K, seed), (pl, outputs, P, got) in end_to_end.items():
        found = sorted((min(i, j), max(i, j)) for i, j in P.joints)
        assert found == sorted(pl.contacts) and len(found) == pj.CONTACTS[K], (K, seed, found)
        assert all(i < j for i, j in P.joints)                                    # the fixed piece is the one placed earlier
        share = pj.purity(pl, outputs)
        before = jr.pose_error(jr.f32(P.G0), pl.truth)[1:].max()
        after = jr.pose_error(got.G, pl.truth)[1:].max()
        print(f"K = {K} seed {seed}: purity {share:.4f}, score {got.score0:.3e} -> {got.score:.3e}, "
              f"largest pose error {before:.4f} -> {after:.4f}")
        assert share >= 0.98, (K, seed, share)
        assert got.score <= got.score0, (K, seed)
        assert after < before, (K, seed, before, after)
