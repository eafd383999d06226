"""CPU: the float64 statement of the trimmed pose refinement (tests/_icp_trim_ref.py) on its own - what
tests/test_gpu_icp_trim.py holds the kernel to has to be right first, and has to be worth building: on pieces of which only a
share mates, the trimmed refinement lands where ICP on the true mating points lands, and the trimmed score separates mates
from non-mates under one geometric threshold where the untrimmed score refuses the mates.

Figures of this file's cases (float64, 20 seeds per row, 30 steps; pose error = _icp_ref.pose_err to the known motion,
median / max):
  ka, kb, share    ICP on the mating rows alone   today's ICP on all rows   trimmed (keep = ka, share kb)
  64, 64, 0.5      0.0288 / 0.0691                0.519 / 1.363             0.0288 / 0.0691
  96, 160, 0.4     0.0124 / 0.0414                0.548 / 1.470             0.0124 / 0.0414
Scores at k = 128, share 0.5 (THRESHOLD below is chosen from them): every mate's trimmed score <= 0.0041, every mate's
untrimmed score >= 0.042, every non-mate's trimmed score >= 0.030.
"""
import numpy as np
import pytest

from tests import _icp_ref as ref
from tests import _icp_trim_ref as trim

SEEDS = 20
STEPS = 30
THRESHOLD = 0.01      # t: mates' trimmed scores < t / 2 = 0.005 (largest 0.0041), non-mates' and untrimmed mates' > 2 t = 0.02
                      # (smallest 0.030 and 0.042) - see the module docstring


def test_all_rows_kept_is_the_untrimmed_loop():
    rng = np.random.default_rng(11)
    for ka, kb in ((24, 37), (64, 50)):
        c = ref.curve_case(rng, ka, kb, False)
        want = ref.refine(c.a, c.b, c.T0, STEPS)
        got = trim.refine(c.a, c.b, c.T0, STEPS, ka, kb)
        assert got.iters_used == want.iters_used >= 1
        assert np.array_equal(got.T, want.T)
        assert got.score == want.score and got.score0 == want.score0 and got.scores == want.scores
        assert got.kept_a.tolist() == list(range(ka)) and got.kept_b.tolist() == list(range(kb))
        assert got.keep_margin == np.inf


@pytest.mark.parametrize("shape", [(64, 64, 0.5), (96, 160, 0.4)], ids=lambda s: f"{s[0]}x{s[1]}x{s[2]}")
def test_partial_contact_is_recovered(shape):
    ka, kb, share = shape
    e_mate, e_all, e_trim = [], [], []
    for seed in range(SEEDS):
        c = trim.partial_case(np.random.default_rng(9000 + seed), ka, kb, share)
        m = int(c.mating.sum())
        assert m == int(round(share * kb))
        e_mate.append(ref.pose_err(ref.refine(c.a, c.b[c.mating], c.T0, STEPS).T, c.G))
        e_all.append(ref.pose_err(ref.refine(c.a, c.b, c.T0, STEPS).T, c.G))
        e_trim.append(ref.pose_err(trim.refine(c.a, c.b, c.T0, STEPS, ka, m).T, c.G))
    print(f"{shape}: mating rows alone {np.median(e_mate):.4f} / {max(e_mate):.4f}, all rows {np.median(e_all):.3f} / "
          f"{max(e_all):.3f}, trimmed {np.median(e_trim):.4f} / {max(e_trim):.4f}")
    for seed in range(SEEDS):      # every seed
        assert e_trim[seed] <= 1.25 * e_mate[seed] + 1e-3, (seed, e_trim[seed], e_mate[seed])
    assert np.median(e_all) >= 4.0 * np.median(e_trim)


@pytest.fixture(scope="module")
def scored():
    """k = 128, share 0.5, SEEDS cases: per seed the mate's trimmed and untrimmed refinement and the non-mate's, both from
    the mate's start pose."""
    k, rows = 128, []
    for seed in range(SEEDS):
        rng = np.random.default_rng(9100 + seed)
        c = trim.partial_case(rng, k, k, 0.5)
        m = int(c.mating.sum())
        nb = trim.non_mate(rng, c)
        rows.append(dict(mate=trim.refine(c.a, c.b, c.T0, STEPS, k, m), mate_all=ref.refine(c.a, c.b, c.T0, STEPS),
                         other=trim.refine(c.a, nb, c.T0, STEPS, k, m), other_all=ref.refine(c.a, nb, c.T0, STEPS)))
    return rows


def test_one_threshold_separates_trimmed_scores(scored):
    t = THRESHOLD
    mate = [r["mate"].score for r in scored]
    mate_all = [r["mate_all"].score for r in scored]
    other = [r["other"].score for r in scored]
    print(f"mates trimmed <= {max(mate):.4f}, mates untrimmed >= {min(mate_all):.4f}, non-mates trimmed >= {min(other):.4f}")
    assert max(mate) < t / 2
    assert min(other) > 2 * t
    assert min(mate_all) > 2 * t


def _pile_table(scored, kind_mate, kind_other):
    """Six pieces, objects {0, 1, 2} and {3, 4, 5}: an ordered pair inside an object takes a mate's refinement, a pair across
    objects a non-mate's, each seed used once -> score [1,6,6] (+inf on the diagonal), T [1,6,6,4,4]."""
    S = np.full((1, 6, 6), np.inf, dtype=np.float32)
    T = np.tile(np.eye(4, dtype=np.float32), (1, 6, 6, 1, 1))
    n_in = n_out = 0
    for i in range(6):
        for j in range(6):
            if i == j:
                continue
            if i // 3 == j // 3:
                r, n_in = scored[n_in][kind_mate], n_in + 1
            else:
                r, n_out = scored[n_out][kind_other], n_out + 1
            S[0, i, j], T[0, i, j] = r.score, r.T
    assert n_in == 12 and n_out == 18
    return S, T


def test_keep_fraction_to_counts():
    """The counts the pair functions hand to ops.icp_refine: ceil(f k) per side, at least 1, None where every row is kept."""
    from puzzlenet_amd import _lib, assembly
    counts = assembly._keep_counts
    assert counts(1.0, 128, 128, "t") is None and counts((1.0, 1), 128, 64, "t") is None
    assert counts(0.5, 128, 128, "t") == (64, 64) and counts((1.0, 0.25), 128, 100, "t") == (128, 25)
    assert counts(0.3, 128, 128, "t") == (39, 39)                      # 38.4 rounds up
    assert counts(0.07, 100, 100, "t") == (7, 7)                       # 0.07 x 100 = 7.000000000000001 in binary: 7 rows
    assert counts((1e-9, 1.0), 128, 100, "t") == (1, 100)              # at least one row
    assert counts(np.float32(0.5), 8, 9, "t") == (4, 5) and counts([np.float64(0.75), 0.5], 8, 8, "t") == (6, 4)
    for bad in (0.0, -0.5, 1.5, (0.5,), (0.5, 0.5, 0.5), "half", None, (0.5, 0.0), True, float("nan")):
        with pytest.raises(_lib.PznError):
            counts(bad, 128, 128, "t")


def test_forest_rule_sorts_the_pile_by_trimmed_scores_only(scored):
    from puzzlenet_amd import assembly
    S, T = _pile_table(scored, "mate", "other")
    # the counts of this test's refinements are what keep = (1.0, 0.5) means at k = 128, and the table is the trimmed type
    assert assembly._keep_counts((1.0, 0.5), 128, 128, "test") == (scored[0]["mate"].kept_a.size, scored[0]["mate"].kept_b.size)
    table = assembly.TrimmedPairTable(None, T, None, None, None, None, S, None, None, None)
    assert table._fields == assembly.PairTable._fields + ("kept_f", "kept_m") and assembly.PairTable(*table[:8]).kept_f is None
    out = assembly.forest_rule(table.score, table.T, max_score=THRESHOLD)
    assert int(out.n_components[0]) == 2 and int(out.n_edges[0]) == 4
    comp = out.component[0].tolist()
    assert comp[0] == comp[1] == comp[2] != comp[3] == comp[4] == comp[5]
    # the same table with the untrimmed scores: every true mate is refused
    S, T = _pile_table(scored, "mate_all", "other_all")
    out = assembly.forest_rule(S, T, max_score=THRESHOLD)
    assert int(out.n_components[0]) == 6 and int(out.n_edges[0]) == 0
    assert sorted(out.component[0].tolist()) == list(range(6))


def _tied_sets(rng, n):
    """2 n rows each side, every point twice (rows 2 i and 2 i + 1 are equal): equal row minima in pairs."""
    a = np.repeat(rng.uniform(-0.5, 0.5, (n, 3)), 2, axis=0).astype(np.float32)
    b = np.repeat(rng.uniform(-0.5, 0.5, (n, 3)), 2, axis=0).astype(np.float32)
    return a, b


def check_kept(minima, kept, m):
    """kept is the m rows of smallest (minimum, index), ascending -> whether equal minima straddle the cut."""
    kept = np.asarray(kept)
    assert kept.shape == (m,) and (np.diff(kept) > 0).all()
    cut = minima[kept].max()
    out = np.setdiff1d(np.arange(minima.shape[0]), kept)
    assert (minima[out] >= cut).all()
    tied_in, tied_out = kept[minima[kept] == cut], out[minima[out] == cut]
    assert tied_out.size == 0 or tied_in.max() < tied_out.min()      # of equal minima the lowest indices are kept
    return tied_out.size > 0


def test_ties_break_to_the_lowest_index_and_score_never_rises():
    rng = np.random.default_rng(12)
    straddled = 0
    for n, m_a, m_b in ((10, 7, 13), (16, 1, 31), (12, 24, 5)):
        a, b = _tied_sets(rng, n)
        T0 = ref.rigid(ref.rot(rng.normal(size=3), 0.2), rng.uniform(-0.1, 0.1, 3)).astype(np.float32)
        o = trim.objective(a, b, T0, m_a, m_b)
        D = ref.sqdist(a, ref.transform(T0, b))
        straddled += check_kept(D.min(axis=1), o.kept_a, m_a) + check_kept(D.min(axis=0), o.kept_b, m_b)
        if m_a < 2 * n and m_a % 2 == 1:
            assert o.keep_margin == 0.0
        r = trim.refine(a, b, T0, 10, m_a, m_b)
        assert r.score <= r.score0 and all(y < x for x, y in zip(r.scores, r.scores[1:]))
        assert r.kept_a.shape == (m_a,) and r.kept_b.shape == (m_b,)
        Dr = ref.sqdist(a, ref.transform(r.T, b))
        check_kept(Dr.min(axis=1), r.kept_a, m_a), check_kept(Dr.min(axis=0), r.kept_b, m_b)
    assert straddled >= 4
