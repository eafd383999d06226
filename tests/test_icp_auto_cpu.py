"""The float64 statement of the pose refinement that finds the overlap share per pair (tests/_icp_auto_ref.py), tested on its
own (no GPU): what the rule is worth on partial contact, its ties, its limits, and the host side of keep="auto"
(assembly.AutoKeep, assembly._keep_counts).

The partial-contact cases are _icp_trim_ref.partial_case / non_mate at ka = kb = 128 with shares 0.3, 0.5, 0.75, 1.0 of the
moved set mating, ten seeds each, default_rng(1000 int(100 share) + seed), 30 steps, AutoKeep's defaults (least 0.25,
power 3).  Figures of this file's run, for the record (nothing below compares with them): the largest mate score 0.00147,
the smallest non-mate score 0.01195.
"""
import numpy as np
import pytest

from tests import _icp_auto_ref as auto
from tests import _icp_ref as ref
from tests import _icp_trim_ref as trim

K = 128
ITERS = 30
SEEDS = 10
LO = auto.least_count(K)


def _angle_deg(T, G):
    R = np.asarray(T, dtype=np.float64)[:3, :3] @ np.asarray(G, dtype=np.float64)[:3, :3].T
    return float(np.degrees(np.arccos(np.clip((np.trace(R) - 1.0) / 2.0, -1.0, 1.0))))


@pytest.fixture(scope="module")
def runs():
    """Per (share, seed): the case, the auto refinement of the mate and of the non-mate, the trimmed one at the TRUE counts."""
    out = []
    for share in auto.SHARES:
        for seed in range(SEEDS):
            rng = np.random.default_rng(1000 * int(100 * share) + seed)
            c = trim.partial_case(rng, K, K, share)
            other = trim.non_mate(rng, c)
            out.append(dict(share=share, seed=seed, case=c,
                            mate=auto.refine(c.a, c.b, c.T0, ITERS, LO, LO, auto.POWER),
                            other=auto.refine(c.a, other, c.T0, ITERS, LO, LO, auto.POWER),
                            true=trim.refine(c.a, c.b, c.T0, ITERS, K, int(round(share * K)))))
    return out


def test_kept_moved_rows_are_mating_rows(runs):
    assert len(runs) == 40
    for r in runs:
        assert r["case"].mating[r["mate"].kept_b].all(), (r["share"], r["seed"])
        assert LO <= r["mate"].m_a <= K and LO <= r["mate"].m_b <= K


def test_scores_separate_mates_from_non_mates_with_no_share_given(runs):
    mate = max(r["mate"].score for r in runs)
    other = min(r["other"].score for r in runs)
    print(f"largest mate score {mate:.5f}, smallest non-mate score {other:.5f}")
    assert mate < other


def test_pose_is_within_twice_the_true_count_refinement(runs):
    for r in runs:
        got, want = _angle_deg(r["mate"].T, r["case"].G), _angle_deg(r["true"].T, r["case"].G)
        assert got <= 2.0 * max(want, 1.0), (r["share"], r["seed"], got, want)


def test_objective_never_rises(runs):
    rose = 0
    for r in runs:
        for run in (r["mate"], r["other"]):
            F = run.objectives
            assert all(y < x for x, y in zip(F, F[1:])) and len(F) == run.iters_used + 1
            assert run.objective == F[-1] and run.objective0 == F[0] and run.objective <= run.objective0
            rose += run.score > run.score0
    print(f"score above score0 in {rose} of {2 * len(runs)} runs (F is what falls)")


def test_least_one_is_the_trimmed_loop_with_every_row_kept():
    rng = np.random.default_rng(21)
    for ka, kb in ((24, 37), (64, 50)):
        c = trim.partial_case(rng, ka, kb, 0.5)
        for power in (1, 3):
            got = auto.refine(c.a, c.b, c.T0, ITERS, ka, kb, power)
            want = trim.refine(c.a, c.b, c.T0, ITERS, ka, kb)
            assert np.array_equal(got.T, want.T) and got.score == want.score and got.score0 == want.score0
            assert got.iters_used == want.iters_used and got.objectives == want.scores and got.objective == want.score
            assert (got.m_a, got.m_b) == (ka, kb) and np.array_equal(got.kept_a, np.arange(ka)) and np.array_equal(got.kept_b, want.kept_b)


def test_ties():
    # all minima zero: every phi is 0, the largest m wins
    for lo in (1, 3, 9):
        assert auto.counts(np.zeros(9), lo, 3) == 9 and auto.count_margin(np.zeros(9), lo, 3) == (0.0 if lo < 9 else np.inf)
    # zeros, then something: phi is 0 up to the last zero, which is the count
    w = np.array([0.5, 0.0, 0.0, 0.25, 0.0])
    assert auto.counts(w, 1, 3) == 3 and auto.counts(w, 4, 3) == 4      # (0.25 / 4^4 = 9.8e-4 against 0.75 / 5^4 = 1.2e-3)
    # equal non-zero phi: S_1 / 1 = S_2 / 2^2 with power 1 -> w = (1, 3); the larger m
    assert auto.phi([1.0, 3.0], 1)[0] == auto.phi([1.0, 3.0], 1)[1] and auto.counts([1.0, 3.0], 1, 1) == 2
    assert auto.count_margin([1.0, 3.0], 1, 1) == 0.0
    assert auto.counts([1.0, 3.0 + 1e-9], 1, 1) == 1 and auto.counts([1.0, 3.0 - 1e-9], 1, 1) == 2
    # a single candidate
    assert auto.counts([2.0, 1.0, 5.0], 3, 2) == 3 and auto.count_margin([2.0, 1.0, 5.0], 3, 2) == np.inf
    # the integer statement of the lattice test says the same
    assert auto.lattice_count([0, 0, 0], 1, 3) == (3, "tie") and auto.lattice_count([1, 3], 1, 1) == (2, "tie")
    assert auto.lattice_count([1, 4], 1, 1) == (1, "unit") and auto.lattice_count([1, 9], 1, 1) == (1, "clear")
    assert auto.lattice_count([5], 1, 3) == (1, "only")
    # the order of the minima does not matter, the kept set follows (value, index)
    rng = np.random.default_rng(5)
    w = rng.integers(0, 4, 40).astype(np.float64)
    m = auto.counts(w, 10, 3)
    assert m == auto.counts(w[::-1], 10, 3) == auto.lattice_count(w.astype(np.int64), 10, 3)[0]


def test_autokeep_to_counts_and_rejections():
    from puzzlenet_amd import _lib, assembly
    counts = assembly._keep_counts
    assert assembly.AutoKeep() == (0.25, 3) and assembly.AutoKeep(power=2).least == 0.25
    assert counts("auto", 128, 128, "t") == (32, 32, 3) == counts(assembly.AutoKeep(), 128, 128, "t")
    got = counts(assembly.AutoKeep(least=(1.0, 0.07), power=1), 128, 100, "t")
    assert got == (128, 7, 1) and (got.lo_f, got.lo_m, got.power) == (128, 7, 1)
    assert counts(assembly.AutoKeep(least=1.0), 8, 8, "t") == (8, 8, 3)            # still the auto launch: every row kept
    assert counts(assembly.AutoKeep(least=1e-6), 8, 5, "t") == (1, 1, 3)
    assert counts(assembly.AutoKeep(least=0.25), 37, 29, "t") == (auto.least_count(37), auto.least_count(29), 3) == (10, 8, 3)
    for bad in (assembly.AutoKeep(power=0), assembly.AutoKeep(power=5), assembly.AutoKeep(power=3.0), assembly.AutoKeep(power=True),
                assembly.AutoKeep(least=0), assembly.AutoKeep(least=0.0), assembly.AutoKeep(least=1.5), assembly.AutoKeep(least=(0.5,)),
                assembly.AutoKeep(least="auto"), "Auto", "AUTO", "", "auto "):
        with pytest.raises(_lib.PznError) as info:
            counts(bad, 128, 128, "t")
        assert not isinstance(info.value, _lib.PznUnsupported), bad
    # floats behave as before
    assert counts(1.0, 128, 128, "t") is None and counts(0.5, 128, 128, "t") == (64, 64)
    # the result types: the trimmed fields, then the three new ones
    tail = ("count_f", "count_m", "objective")
    assert assembly.AutoPairTable._fields == assembly.TrimmedPairTable._fields + tail
    assert assembly.AutoPairBlock._fields == assembly.TrimmedPairBlock._fields + tail
    assert assembly.AutoRefined._fields == assembly.TrimmedRefined._fields + tail
    # the joint refinements refuse an auto table, and say why
    table = assembly.AutoPairTable(*([None] * len(assembly.AutoPairTable._fields)))
    for fn in (assembly.refine_assembly, assembly.refine_assembly_batch):
        with pytest.raises(_lib.PznUnsupported, match="per pair"):
            fn(None, table, None)


def test_the_three_kinds_share_their_extra_fields():
    """assembly._KINDS: no kept sets, kept sets, kept sets with counts.  The Refined, block and table types of a kind are the
    base fields followed by the same extra fields in the same order, and each is rebuilt from a flat list by type(t)(*t)."""
    from puzzlenet_amd import assembly
    extras = [(), ("kept_f", "kept_m"), ("kept_f", "kept_m", "count_f", "count_m", "objective")]
    assert len(assembly._KINDS) == 3
    assert assembly._KINDS[0] == (assembly.Refined, assembly.PairBlock, assembly.PairTable)
    assert assembly._KINDS[1] == (assembly.TrimmedRefined, assembly.TrimmedPairBlock, assembly.TrimmedPairTable)
    assert assembly._KINDS[2] == (assembly.AutoRefined, assembly.AutoPairBlock, assembly.AutoPairTable)
    for counts, kind, extra in zip((None, (3, 2), assembly._AutoCounts(3, 2, 3)), assembly._KINDS, extras):
        assert assembly._kind_of(counts) is kind
        for typ, base in zip(kind, assembly._KINDS[0]):
            assert typ._fields == base._fields + extra, typ
            flat = [object() for _ in typ._fields]
            t = typ(*flat)
            again = type(t)(*t)
            assert type(again) is typ and all(x is y for x, y in zip(again, flat))
            if not extra:
                assert t.kept_f is None and t.kept_m is None
            else:
                assert t.kept_f is flat[len(base._fields)] and t.kept_m is flat[len(base._fields) + 1]


def test_the_margin_rule_leaves_out_at_most_a_quarter():
    """Of the float64 comparisons tests/test_gpu_icp_auto.py makes, how many the margin rule leaves out - from the statement
    and the bounds alone, so it is known here and not on the kernel."""
    left = total = 0
    for shape in auto.FLOAT64_SHAPES:
        ka, kb, _ = shape
        for c in auto.float64_cases(shape):
            total += 1
            left += not auto.count_decided(c, c.T0, auto.least_count(ka), auto.least_count(kb), auto.POWER)
    print(f"count comparisons left out: {left} of {total}")
    assert 4 * left <= total
    cases = auto.trajectory_cases()
    k = auto.TRAJECTORY_K
    out = sum(auto.trajectory_left_out(c, auto.refine(c.a, c.b, c.T0, ITERS, auto.least_count(k), auto.least_count(k), auto.POWER))
              for c in cases)
    print(f"trajectories left out: {out} of {len(cases)}")
    assert 4 * out <= len(cases)


def test_lattice_counts_are_mostly_decided_by_a_tie_or_one_unit():
    for shape in auto.LATTICE_SHAPES:
        ka, kb, P = shape
        _, _, _, ia, ib, it = auto.lattice_case(shape)
        how = []
        for p in range(min(P, 24)):
            e = auto.lattice_expected(ia[p], ib[p], it[p], auto.least_count(ka), auto.least_count(kb), auto.POWER)
            how += [e["how_a"], e["how_b"]]
        close = sum(h in ("tie", "unit") for h in how)
        assert ka == 1 or 2 * close > len(how), (shape, how)
