"""CPU: assembly.progressive_round_rule - the numpy statement of ops.progressive_round (csrc/progressive.hip, the rule in
include/pzn.h) - against the per-puzzle definitions it batches: assembly._choose on the compacted table and MergeLedger.merge.  The
rule keeps P slots and lets slots die; ProgressiveAssembler compacts its list.  Row-major order over the live slots is the compacted
order, so every round must choose the same pair, give the same labels and members, and the same poses up to the last place (numpy's
matmul against the fixed-order product, as with walk_rule).  The table kinds are those of tests/_walk_cases.py; the table stays the
same over the rounds, only the rule's own masking of dead slots changes what it sees."""
import numpy as np
import pytest

from tests import _walk_cases as wc

Z = 3
SIZES = (2, 5, 33, 64)


def _same_state(a, b):
    for name, x, y in zip(a._fields, a, b):
        assert x.dtype == y.dtype and x.shape == y.shape, name
        assert x.tobytes() == y.tobytes(), name


def _replay(S, T, max_score=None, count=None):
    """P - 1 rounds of the rule on a fixed table, every round against _choose and MergeLedger on the compacted list -> the rounds'
    took flags [rounds, Z] and the final state."""
    from puzzlenet_amd import assembly
    Zn, P = S.shape[0], S.shape[1]
    counts = [P] * Zn if count is None else [int(c) for c in count]
    state = assembly.progressive_start(Zn, P, count)
    assert state.alive.sum(axis=1).tolist() == [min(max(c, 0), P) for c in counts]
    live = [list(range(min(max(c, 0), P))) for c in counts]
    ledgers = [assembly.MergeLedger(len(l)) for l in live]
    stopped = [False] * Zn
    flags = []
    for _ in range(P - 1):
        new, took, pick = assembly.progressive_round_rule(S, T, state, max_score)
        assert took.dtype == np.uint8 and pick.dtype == np.int64 and pick.shape == (Zn, 2)
        for z in range(Zn):
            l, led = live[z], ledgers[z]
            want = None
            if not stopped[z] and len(l) >= 2:
                want = assembly._choose(S[z][np.ix_(l, l)], max_score)
            if want is None:
                stopped[z] = True
                assert took[z] == 0 and pick[z].tolist() == [0, 0] and new.done[z] == 1
                # nothing but `done` has changed, bit for bit
                for name, x, y in zip(new._fields, new, state):
                    if name != "done":
                        assert x[z].tobytes() == y[z].tobytes(), name
                continue
            ci, cj, s = want
            i, j = l[ci], l[cj]
            assert took[z] == 1 and pick[z].tolist() == [i, j] and new.done[z] == 0
            led.merge(ci, cj, T[z, i, j].astype(np.float64), s)
            l.remove(j)
            ne = int(new.n_edges[z])
            assert ne == len(led.edges) == int(state.n_edges[z]) + 1
            assert new.edges[z, ne - 1].tolist() == [led.edges[-1][0], led.edges[-1][1], i, j]
            assert new.edge_score[z, ne - 1].tobytes() == S[z, i, j].tobytes()
            assert (new.edges[z, ne:] == -1).all() and np.isposinf(new.edge_score[z, ne:]).all()
            assert [s_ for s_ in range(P) if new.alive[z, s_]] == l
            for c, slot in enumerate(l):                 # labels and members of every live part
                members = [p for p in range(P) if new.part[z, p] == slot]
                assert members == sorted(led.members[c]) and min(members) == led.label(c) and led.frame[c] == slot
            n = len(led.G)
            assert np.abs(new.G[z, :n] - led.G).max() <= 1e-12
            assert np.array_equal(new.G[z, n:], np.tile(np.eye(4), (P - n, 1, 1)))
        flags.append(took)
        state = new
    return np.array(flags), state


@pytest.mark.parametrize("kind", wc.KINDS)
@pytest.mark.parametrize("P", SIZES)
def test_rule_is_choose_and_ledger(P, kind):
    S, T, max_score = wc.make(kind, Z, P, 1500)
    flags, state = _replay(S, T, max_score)
    if kind in ("lattice", "random"):
        assert flags.all() and (state.alive.sum(axis=1) == 1).all() and (state.n_edges == P - 1).all()
    if kind == "blocks" and P > 2:
        assert (state.alive.sum(axis=1) == 2).all() and (state.done == 1).all()      # one part per block, nothing joins them
    # P - 1 rounds: a walk that made fewer than P - 1 edges met a stop, and only such a walk did
    assert ((state.done == 1) == (state.n_edges < P - 1)).all() and (state.n_edges == flags.sum(axis=0)).all()
    if kind == "max_score" and P >= 33:
        assert (state.n_edges > 0).all() and (state.n_edges < P - 1).all()      # the limit bites in mid-walk


def test_stop_at_max_score_and_done_stays_done():
    from puzzlenet_amd import assembly
    P = 5
    S, T, _ = wc.make("random", Z, P, 1600)
    firsts = np.sort(np.array([assembly._choose(S[z])[2] for z in range(Z)]))
    limit = float((firsts[0] + firsts[1]) / 2)           # one puzzle starts, the others stop in the first round
    s0 = assembly.progressive_start(Z, P)
    s1, took, pick = assembly.progressive_round_rule(S, T, s0, limit)
    assert took.sum() == 1 and s1.done.sum() == Z - 1
    for z in range(Z):
        if not took[z]:
            assert pick[z].tolist() == [0, 0] and s1.n_edges[z] == 0 and s1.alive[z].all() and (s1.edges[z] == -1).all()
    # later rounds, with and without a limit: a stopped puzzle stays stopped and keeps every bit
    s2, took2, _ = assembly.progressive_round_rule(S, T, s1, None)
    for z in range(Z):
        if not took[z]:
            assert took2[z] == 0
            for name, x, y in zip(s2._fields, s2, s1):
                assert x[z].tobytes() == y[z].tobytes(), name
    # the input state is not changed
    _same_state(s0, assembly.progressive_start(Z, P))


def test_stop_at_an_all_nan_table():
    from puzzlenet_amd import assembly
    P = 5
    S, T, _ = wc.make("random", Z, P, 1700)
    S[1] = np.nan
    S[2] = np.inf
    s0 = assembly.progressive_start(Z, P)
    s1, took, pick = assembly.progressive_round_rule(S, T, s0)
    assert took.tolist() == [1, 0, 0] and s1.done.tolist() == [0, 1, 1] and pick[1:].tolist() == [[0, 0], [0, 0]]
    for name, x, y in zip(s1._fields, s1, s0):
        if name != "done":
            assert x[1:].tobytes() == y[1:].tobytes(), name
    flags, _ = _replay(S, T)
    assert flags[:, 0].all() and not flags[:, 1:].any()


@pytest.mark.parametrize("fill", (float("nan"), -1.0))
def test_count_below_p(fill):
    """Puzzles of fewer pieces than slots; the padding holds NaN or -1 (smaller than every score) and never takes part."""
    P = 9
    counts = np.array([9, 2, 5, 1, 0], dtype=np.int32)
    for kind in ("lattice", "nan30"):
        S, T, _ = wc.make(kind, len(counts), P, 1800)
        for z, c in enumerate(counts):
            S[z, c:, :], S[z, :, c:] = fill, fill
            T[z, c:, :], T[z, :, c:] = fill, fill
        flags, state = _replay(S, T, count=counts)
        assert not flags[:, 3:].any() and flags[0, :3].all()
        assert (state.part == np.arange(P)[None, :])[3:].all() and np.isfinite(state.G).all()
        for z, c in enumerate(counts):
            assert not state.alive[z, c:].any()


def test_argument_errors():
    from puzzlenet_amd import assembly
    S, T, _ = wc.make("random", 2, 4, 1900)
    with pytest.raises(ValueError):
        assembly.progressive_round_rule(S[0], T[0], assembly.progressive_start(2, 4))
    with pytest.raises(ValueError):
        assembly.progressive_round_rule(S, T[:, :3], assembly.progressive_start(2, 4))
