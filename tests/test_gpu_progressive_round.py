"""GPU: ops.progressive_round (csrc/progressive.hip, progressive_round_kernel) against assembly.progressive_round_rule - the numpy
statement of the rule in include/pzn.h, itself held to _choose and MergeLedger in tests/test_progressive_rule_cpu.py - bit for bit in
every state field after every round, the float64 poses included: both sides compose them in IEEE double in the same order, so there
is no tolerance.  The table kinds are those of tests/_walk_cases.py; the table stays the same over the rounds, so between rounds
only the kernel's own masking of dead slots changes what it sees."""
import numpy as np
import pytest
import torch

from tests import _walk_cases as wc

pytestmark = pytest.mark.gpu

Z = 5
IN_FLIGHT = 1024      # puzzles one launch holds at a time (256 workgroups of four wavefronts): more take turns


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _same(state, took, pick, want, what):
    w_state, w_took, w_pick = want
    for name, g, w in zip(w_state._fields, state, w_state):
        w = torch.from_numpy(w)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, tuple(g.shape))
        assert torch.equal(g.cpu(), w), (what, name)
    assert took.dtype == torch.uint8 and pick.dtype == torch.int64
    assert torch.equal(took.cpu(), torch.from_numpy(w_took)), (what, "took")
    assert torch.equal(pick.cpu(), torch.from_numpy(w_pick)), (what, "pick")


def _walk(dev, S, T, max_score=None, count=None, rounds=None):
    """P - 1 rounds on the device and by the rule, compared after every round -> the final device state and the rounds' flags."""
    from puzzlenet_amd import assembly, ops
    Zn, P = S.shape[0], S.shape[1]
    s, t = torch.from_numpy(S).to(dev), torch.from_numpy(T).to(dev)
    state = ops.progressive_state(Zn, P, dev, None if count is None else torch.from_numpy(count).to(dev))
    rule = assembly.progressive_start(Zn, P, count)
    _same(state, torch.zeros(Zn, dtype=torch.uint8), torch.zeros((Zn, 2), dtype=torch.int64),
          (rule, np.zeros(Zn, dtype=np.uint8), np.zeros((Zn, 2), dtype=np.int64)), "start")
    flags = []
    for r in range(P - 1 if rounds is None else rounds):
        took, pick = ops.progressive_round(s, t, state, max_score)
        rule, w_took, w_pick = assembly.progressive_round_rule(S, T, rule, max_score)
        _same(state, took, pick, (rule, w_took, w_pick), f"round {r}")
        flags.append(w_took)
    return state, np.array(flags)


@pytest.mark.parametrize("kind", wc.KINDS)
@pytest.mark.parametrize("P", (2, 5, 33, 64))
def test_kernel_is_the_rule(dev, P, kind):
    S, T, max_score = wc.make(kind, Z, P, 2500)
    state, flags = _walk(dev, S, T, max_score)
    if kind in ("lattice", "random"):
        assert flags.all() and state.n_edges.tolist() == [P - 1] * Z and state.alive.sum(dim=1).tolist() == [1] * Z


@pytest.mark.parametrize("fill", (float("nan"), -1.0))
def test_mixed_counts(dev, fill):
    """Puzzles of 0 .. P pieces in one launch; the padding holds NaN or -1 (smaller than every score) and never takes part."""
    P = 33
    counts = np.array([33, 2, 17, 1, 0, 5, 32], dtype=np.int32)
    for kind in ("lattice", "nan30"):
        S, T, _ = wc.make(kind, len(counts), P, 2600)
        for z, c in enumerate(counts):
            S[z, c:, :], S[z, :, c:] = fill, fill
            T[z, c:, :], T[z, :, c:] = fill, fill
        state, flags = _walk(dev, S, T, count=counts)
        assert not flags[:, [3, 4]].any() and state.done[[3, 4]].tolist() == [1, 1]
        if kind == "lattice":
            assert state.n_edges.tolist() == [max(int(c) - 1, 0) for c in counts]
        assert bool(torch.isfinite(state.G).all())


def test_max_score_stops_some_and_they_stay_stopped(dev):
    """A limit between two first-round minima: some puzzles stop at once and keep every bit while the others walk on; the later
    rounds run without a limit, and a stopped puzzle still does not move."""
    from puzzlenet_amd import assembly, ops
    P = 5
    S, T, _ = wc.make("random", Z, P, 2700)
    firsts = np.sort(np.array([assembly._choose(S[z])[2] for z in range(Z)]))
    limit = float((firsts[1] + firsts[2]) / 2)
    s, t = torch.from_numpy(S).to(dev), torch.from_numpy(T).to(dev)
    state = ops.progressive_state(Z, P, dev)
    fresh = [f.clone() for f in state]
    took, pick = ops.progressive_round(s, t, state, limit)
    assert took.tolist().count(1) == 2
    stopped = (took == 0).nonzero()[:, 0]
    assert pick[stopped].abs().sum().item() == 0 and state.done[stopped].tolist() == [1] * 3
    for r in range(P - 1):
        ops.progressive_round(s, t, state, None)
    for name, f, f0 in zip(state._fields, state, fresh):
        if name != "done":
            assert torch.equal(f[stopped], f0[stopped]), name
    walked = (took == 1).nonzero()[:, 0]
    assert state.n_edges[walked].tolist() == [P - 1] * 2


def test_more_puzzles_than_one_launch_holds(dev):
    n = IN_FLIGHT + 7
    S, T, _ = wc.make("lattice", n, 3, 2800)
    S2, T2, _ = wc.make("random", n, 3, 2801)
    S[::2], T[::2] = S2[::2], T2[::2]
    state, flags = _walk(dev, S, T)
    assert flags.all() and int(state.n_edges.sum()) == 2 * n


def test_two_runs_give_the_same_bits(dev):
    from puzzlenet_amd import ops
    S, T, _ = wc.make("lattice", 64, 33, 2900)
    s, t = torch.from_numpy(S).to(dev), torch.from_numpy(T).to(dev)
    runs = []
    for _ in range(2):
        state = ops.progressive_state(64, 33, dev)
        outs = [ops.progressive_round(s, t, state) for _ in range(32)]
        runs.append(list(state) + [x for o in outs for x in o])
    assert all(torch.equal(x, y) for x, y in zip(*runs))


def test_argument_errors(dev):
    from puzzlenet_amd import _lib, ops
    S, T, _ = wc.make("random", 2, 4, 3000)
    s, t = torch.from_numpy(S).to(dev), torch.from_numpy(T).to(dev)
    st = ops.progressive_state(2, 4, dev)
    real, calls = ops._call, []

    def spy(name, *a, **k):
        calls.append(name)
        return real(name, *a, **k)
    ops._call = spy
    try:
        with pytest.raises(_lib.PznError):
            ops.progressive_round(s.cpu(), t, st)
        with pytest.raises(_lib.PznError):
            ops.progressive_round(s.double(), t, st)
        with pytest.raises(_lib.PznError):
            ops.progressive_round(s, t[:, :3], st)
        with pytest.raises(_lib.PznError):
            ops.progressive_round(s[0], t[0], st)
        with pytest.raises(_lib.PznError):
            ops.progressive_round(s, t, tuple(st))                                      # not a ProgressiveState
        with pytest.raises(_lib.PznError):
            ops.progressive_round(s, t, st._replace(G=st.G.float()))                    # a state of another type
        with pytest.raises(_lib.PznError):
            ops.progressive_round(s, t, st._replace(part=st.part.t().contiguous().t()))  # not contiguous: no in-place update
        with pytest.raises(_lib.PznError):
            ops.progressive_round(s, t, ops.progressive_state(3, 4, dev))
        with pytest.raises(_lib.PznError):
            ops.progressive_round(s, t, st._replace(alive=st.alive.cpu()))
        with pytest.raises(_lib.PznError):
            ops.progressive_round(s, t, st, max_score=float("nan"))
        with pytest.raises(_lib.PznError):
            ops.progressive_state(2, 4, dev, count=torch.zeros(3, dtype=torch.int32, device=dev))
        for P in (1, 65):
            with pytest.raises(_lib.PznUnsupported):
                ops.progressive_round(torch.zeros(1, P, P, device=dev), torch.zeros(1, P, P, 4, 4, device=dev),
                                      ops.progressive_state(1, P, dev))
        assert calls == []                                                              # every refusal came before any launch
        assert ops.progressive_round_supported(2) and ops.progressive_round_supported(64) and not ops.progressive_round_supported(65)
        took, pick = ops.progressive_round(s[:0], t[:0], ops.progressive_state(0, 4, dev))
        assert took.shape == (0,) and pick.shape == (0, 2) and calls == []              # Z = 0 launches nothing
        ops.progressive_round(s, t, st)
        assert calls == ["pzn_progressive_round_f32"]                                   # one launch a round
    finally:
        ops._call = real
