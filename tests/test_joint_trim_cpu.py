"""CPU: the float64 side and the host side of the joint refinement with kept rows chosen again under the joint poses
(pzn_joint_refine_trim_f32, ops.joint_refine(..., ma=, mb=), assembly.refine_assembly(..., keep=)): the statement
tests/_joint_trim_ref.py against _joint_ref (identity) and on partial-contact puzzles (what the feature is for), the two case
families tests/test_gpu_joint_trim.py holds the kernel to, the `keep` keyword before any tensor is touched, and the header, the
bindings, the registers and the LDS of the new kernel."""
import numpy as np
import pytest

from tests import _joint_ref as jr
from tests import _joint_trim as jm
from tests import _joint_trim_ref as jt

# ---------------------------------------------------------------------------------------------- the statement

@pytest.mark.parametrize("graph", jm.GRAPHS)
def test_full_counts_are_the_untrimmed_statement_value_for_value(graph):
    K, joints = jr.GRAPHS[graph]
    rng = np.random.default_rng(9000 + jm.GRAPHS.index(graph))
    for k in (6, (9, 7)):
        P = jr.puzzle(rng, K, joints, k)
        T = jt.with_counts(P)
        assert T.ma == [len(A) for A in P.A] and T.mb == [len(B) for B in P.B]
        want, got = jr.refine(P, 4), jt.refine(T, 4)
        assert np.array_equal(want.G, got.G) and want.score == got.score and want.score0 == got.score0
        assert want.sweeps_used == got.sweeps_used and want.accepted.tolist() == got.accepted.tolist()
        assert want.scores == got.scores and want.margin_ratio == got.margin_ratio and got.keep_ratio == np.inf
        assert all(np.array_equal(r, np.arange(len(A))) for r, A in zip(got.kept_a, P.A))
        assert all(np.array_equal(r, np.arange(len(B))) for r, B in zip(got.kept_b, P.B))
        g0 = jr.f32(P.G0)
        for p in range(1, K):
            each = jt.piece_energy(T, g0, p)[1]
            corr = {e: (o.c1, o.c2) for e, o in each.items()}
            assert np.array_equal(jt.visit(T, g0, p), jr.visit(P, g0, p))
            assert np.array_equal(jt.visit_f32(T, P.G0, p, each), jr.visit_f32(P, P.G0, p, corr))
        for e, (i, j) in enumerate(joints):
            # (the trimmed form sorts the ends before it adds them: the same interval up to the order of a float64 sum)
            assert jt.objective_interval2(P.A[e], P.B[e], g0[i], g0[j], T.ma[e], T.mb[e]) == \
                pytest.approx(jr.objective_interval2(P.A[e], P.B[e], g0[i], g0[j]), rel=1e-13, abs=0)


def test_kept_rows_are_the_m_smallest_minima_lowest_index_on_ties():
    P = jm.lattice_puzzle(np.random.default_rng(5), 2, [(0, 1)], (12, 9), [(5, 4)])
    o = jt.joint_energy(P, jr.f32(P.G0), 0)
    D = jr._D(P, jr.f32(P.G0), 0)
    for kept, mins, m in ((o.kept_a, D.min(axis=1), 5), (o.kept_b, D.min(axis=0), 4)):
        order = sorted(range(len(mins)), key=lambda r: (mins[r], r))      # the rule, spelt out
        assert kept.tolist() == sorted(order[:m]) and len(set(mins.tolist())) < len(mins)
    assert o.E == D.min(axis=1)[o.kept_a].sum() / 5 + D.min(axis=0)[o.kept_b].sum() / 4


# ---------------------------------------------------------------------------------------------- partial contact

PARTIAL_K, PARTIAL_SWEEPS, PARTIAL_SEEDS, NOISE = 96, 12, 6, 0.003
PARTIAL_GRAPHS = ["chain3", "ring4", "complete5"]
SHARES = [0.5, 0.75]
# Bound of the trimmed statement's error, in units of the oracle's (the untrimmed statement over the true mating rows alone):
# a factor of 4, or 3 x the point noise if that is larger - the kept set may swap a few rows near the ends of the contact.
ORACLE_FACTOR, NOISE_FACTOR = 4.0, 3.0
# Measured over the 36 cases below (12 sweeps): the largest trimmed error / oracle error is 1.00 - with the other faces
# OTHER_GAP away from everything of the opposite piece the kept rows ARE the mating rows at every evaluated pose.  The
# untrimmed statement's largest pose error ends between 0.15 and 1.06 and the trimmed one's between 0.0027 and 0.044, from a
# start of 0.010 to 0.065.
MEASURED_RATIO = 1.00


def _partial(graph, share, seed):
    K, joints = jr.GRAPHS[graph]
    rng = np.random.default_rng(9100 + 100 * PARTIAL_GRAPHS.index(graph) + 10 * int(share * 4) + seed)
    P, mating_a, mating_b = jt.partial_puzzle(rng, K, joints, PARTIAL_K, share, noise=NOISE)
    n = int(round(share * PARTIAL_K))
    assert all(int(m.sum()) == n for m in mating_a + mating_b)
    return P, jt.with_counts(P, [n] * len(joints), [n] * len(joints)), jt.mating_only(P, mating_a, mating_b)


@pytest.mark.parametrize("seed", range(PARTIAL_SEEDS))
@pytest.mark.parametrize("share", SHARES)
@pytest.mark.parametrize("graph", PARTIAL_GRAPHS)
def test_partial_contact_trimmed_lands_where_the_oracle_lands_and_untrimmed_does_not(graph, share, seed):
    """Both sets of every joint have round(share k) rows on the shared curve, the rest on other faces.  The oracle - today's
    statement over the true mating rows alone - is the reference; the trimmed statement, which is told only HOW MANY rows
    mate, is held to ORACLE_FACTOR x its error (or NOISE_FACTOR x the noise); today's statement over the full sets ends
    further from the truth than the trimmed one, in every case."""
    P, T, O = _partial(graph, share, seed)
    full, trim, oracle = jr.refine(P, PARTIAL_SWEEPS), jt.refine(T, PARTIAL_SWEEPS), jr.refine(O, PARTIAL_SWEEPS)
    e0 = jr.pose_error(P.G0, P.truth).max()
    ef, et, eo = (jr.pose_error(x.G, P.truth).max() for x in (full, trim, oracle))
    print(f"{graph} share {share} seed {seed}: start {e0:.4f}, untrimmed {ef:.4f}, trimmed {et:.4f}, oracle {eo:.4f}, "
          f"trimmed / oracle {et / eo:.3f} (measured largest over all cases: {MEASURED_RATIO:.2f})")
    assert trim.score <= trim.score0 and all(y <= x for x, y in zip(trim.scores, trim.scores[1:]))
    assert ef > et, (ef, et)
    assert et <= max(ORACLE_FACTOR * eo, NOISE_FACTOR * NOISE), (et, eo)


# ---------------------------------------------------------------------------------------------- the GPU tests' families

def test_lattice_puzzles_are_exact_in_float32_and_their_minima_tie():
    rng = np.random.default_rng(11)
    K, joints = jr.GRAPHS["both3"]
    P = jm.lattice_puzzle(rng, K, joints, (33, 7), [(33, 1)] * len(joints))
    for A in P.A + P.B:
        assert np.array_equal(A, np.round(A)) and np.abs(A).max() <= 8
    for g in P.G0:
        assert np.array_equal(g, np.round(g)) and np.linalg.det(g[:3, :3].astype(np.float64)) == 1.0
    ties = 0
    for e in range(len(joints)):
        D = jr._D(P, jr.f32(P.G0), e)
        assert np.array_equal(D, np.round(D)) and D.max() < 2 ** 10
        ties += len(D.min(axis=1)) - len(set(D.min(axis=1).tolist()))
    assert ties > 0


@pytest.mark.parametrize("graph", jm.GRAPHS)
def test_trajectory_family_descends_and_at_most_a_quarter_is_left_out(graph):
    cases = jm.trajectory_cases(graph)
    assert len(cases) == jm.TRAJECTORY_CASES == 16
    k = jm.TRAJECTORY_K
    assert all(len(A) == k and len(B) == k for P in cases for A, B in zip(P.A, P.B))
    counts = {m for P in cases for m in P.ma}
    assert counts <= set(range(k // 2, k + 1)) and len(counts) >= 3 and all(P.ma == P.mb for P in cases)
    left = 0
    for P in cases:
        want, entered = jm.trajectory_row(P)
        assert all(y <= x for x, y in zip(want.scores, want.scores[1:])) and want.score < want.score0
        left += not entered
    print(f"{graph}: left out {left} of {len(cases)}")
    assert left == jm.TRAJECTORY[graph] and 4 * left <= len(cases), (graph, left)


@pytest.mark.parametrize("graph", jm.VISIT_GRAPHS)
def test_visit_family_at_most_a_quarter_is_left_out(graph):
    cases = jm.visit_cases(graph)
    assert len(cases) == jm.VISIT_CASES == 24
    k = jm.VISIT_K
    assert all(len(A) == k and len(B) == k for P in cases for A, B in zip(P.A, P.B)) and k % 4 != 0
    assert {m for P in cases for m in P.ma} == set(range((k + 1) // 2, k + 1))
    assert all(P.movable.tolist() == [p == 1 for p in range(P.K)] for P in cases)
    rows = [jm.visit_row(P) for P in cases]
    left = sum(not r[2] for r in rows)
    print(f"{graph}: left out {left} of {len(rows)}, yardstick max {max(r[1] for r in rows):.3e}, smallest gap "
          f"{min(r[3] for r in rows):.1e}")
    assert left == jm.VISIT[graph] and 4 * left <= len(rows), (graph, left)


# ---------------------------------------------------------------------------------------------- the host side

def _tables_of_nones():
    from puzzlenet_amd import assembly
    return {t.__name__: t(*([None] * len(t._fields))) for t in (assembly.PairTable, assembly.TrimmedPairTable, assembly.AutoPairTable)}


def test_keep_keyword_is_decided_before_any_tensor_is_touched():
    from puzzlenet_amd import _lib, assembly
    tables = _tables_of_nones()
    for fn in (assembly.refine_assembly, assembly.refine_assembly_batch):
        for name, table in tables.items():
            # keep together with kept="frozen": the rows are either frozen or chosen again
            for keep in (0.5, (0.5, 1.0), 1.0, "table"):
                with pytest.raises(_lib.PznError, match="keep") as info:
                    fn(None, table, None, kept="frozen", keep=keep)
                assert not isinstance(info.value, _lib.PznUnsupported), (name, keep)
            # no share, no word it knows, and no rule that finds counts
            for bad in (0.0, -0.5, 1.5, (0.5,), (0.5, 0.5, 0.5), (0.5, 2.0), True, "auto", "frozen", "Table", assembly.AutoKeep()):
                with pytest.raises(_lib.PznError, match="keep") as info:
                    fn(None, table, None, keep=bad)
                assert not isinstance(info.value, _lib.PznUnsupported), (name, bad)
            # a bad kept stays an error whatever keep says
            with pytest.raises(_lib.PznError, match="kept"):
                fn(None, table, None, kept="retrim", keep=0.5)
        # keep="table" needs a table that carries counts
        with pytest.raises(_lib.PznError, match="carries counts") as info:
            fn(None, tables["PairTable"], None, keep="table")
        assert not isinstance(info.value, _lib.PznUnsupported)
        # an auto table with keep given is NOT refused: the keyword rules let it through, and what stops the call is the next
        # check, the pieces that are no tensor
        for name, keeps in (("AutoPairTable", (0.5, 1.0, (0.25, 0.75), "table")), ("TrimmedPairTable", (0.5, "table")), ("PairTable", (0.5,))):
            for keep in keeps:
                with pytest.raises(_lib.PznError, match="pieces must be a tensor") as info:
                    fn(None, tables[name], None, keep=keep)
                assert not isinstance(info.value, _lib.PznUnsupported), (name, keep)
        # and without keep the default still refuses it
        with pytest.raises(_lib.PznUnsupported, match="per pair"):
            fn(None, tables["AutoPairTable"], None)


def test_result_type_carries_the_kept_rows_and_counts_behind_today_s_fields():
    from puzzlenet_amd import assembly
    assert assembly.TrimmedJointRefined._fields == assembly.JointRefined._fields + ("kept_f", "kept_m", "count_f", "count_m")


def test_header_declares_and_the_library_exports_the_trim_entry_point():
    from puzzlenet_amd import _lib, build
    old, new = _lib.PARAMS["pzn_joint_refine_f32"], _lib.PARAMS["pzn_joint_refine_trim_f32"]
    assert len(old) == 20 and len(new) == 24
    assert new[2] == "const int32_t* ma" and new[5] == "const int32_t* mb"
    assert new[-3:-1] == ["int32_t* kept_a", "int32_t* kept_b"]
    assert [p for n, p in enumerate(new) if n not in (2, 5, 21, 22)] == old      # the old parameters in the old order around them
    lib = _lib.load()
    assert getattr(lib, "pzn_joint_refine_trim_f32") is not None
    assert "jointtrim.hip" in dict(build.SOURCES) and dict(build.SOURCES)["jointtrim.hip"] == dict(build.SOURCES)["jointrefine.hip"]
    # the sibling's range, its upper end included (68.3 KB of LDS there: the launch raises the kernel's limit)
    from puzzlenet_amd import ops
    ok = ops.joint_refine_trim_supported
    assert ok(64, 64 * 63, 1024, 1024) and ok(1, 0, 1, 1)
    for bad in ((65, 0, 8, 8), (0, 0, 8, 8), (4, 13, 8, 8), (4, -1, 8, 8), (4, 12, 1025, 8), (4, 12, 8, 1025), (4, 12, 0, 8), (4, 12, 8, 0)):
        assert not ok(*bad) and not ops.joint_refine_supported(*bad), bad


def test_trim_kernel_keeps_its_float64_sums_and_solve_in_registers():
    """tests/test_joint_counts_cpu.py's check for the two kernels of jointrefine.hip, for the one of jointtrim.hip: no vector
    register is spilled, there is no private segment, all LDS is dynamic (the launch sizes it), and the file holds this one
    kernel."""
    import os
    import re
    import subprocess
    import tempfile
    from puzzlenet_amd import build
    flags = [f for f in build.COMMON if f not in ("-fPIC", "-fvisibility=hidden")]
    extra = dict(build.SOURCES)["jointtrim.hip"]
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "jointtrim.s")
        cmd = [build.hipcc()] + flags + extra + ["-S", "--cuda-device-only", "-o", out, os.path.join(build.CSRC, "jointtrim.hip")]
        assert subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL).returncode == 0
        text = open(out).read()
    meta = text[text.index("amdhsa.kernels:"):]
    entries = {re.search(r"\.name:\s+(\S+)", e).group(1): e for e in re.split(r"\n  - ", meta)[1:] if re.search(r"\.name:\s+(\S+)", e)}
    names = [n for n in entries if "joint" in n]
    assert len(names) == 1 and "joint_trim_kernel" in names[0], names
    e = entries[names[0]]
    assert int(re.search(r"\.vgpr_spill_count:\s+(\d+)", e).group(1)) == 0
    assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", e).group(1)) == 0
    assert int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", e).group(1)) == 0
    assert int(re.search(r"\.max_flat_workgroup_size:\s+(\d+)", e).group(1)) == 256
