"""The joint refinement that finds the kept counts of every joint under the joint poses (ops.joint_refine(..., auto=),
pzn_joint_refine_auto_f32), on the float64 statement tests/_joint_auto_ref.py alone (no GPU): the identities the statement must
pass, the host side of the `auto` keyword, the committed left-out counts of the float64 comparisons of
tests/test_gpu_joint_auto.py, and what the rule is worth - measured, not assumed."""
import numpy as np
import pytest

from tests import _icp_auto_ref as au
from tests import _joint_auto_ref as ja
from tests import _joint_ref as jr
from tests import _joint_trim as jm
from tests import _joint_trim_ref as jt


# ---------------------------------------------------------------------------------------------- the statement

@pytest.mark.parametrize("graph", jm.GRAPHS)
def test_a_least_share_of_one_is_the_trimmed_statement_at_full_counts(graph):
    K, joints = jr.GRAPHS[graph]
    rng = np.random.default_rng(9000 + jm.GRAPHS.index(graph))
    for _ in range(3):
        P, _, _ = jt.partial_puzzle(rng, K, joints, 8, None, n_mate=rng.integers(4, 9, size=len(joints)), quick=True)
        want = jt.refine(jt.with_counts(P), 3)
        got = ja.refine(ja.with_least(P, least=1.0), 3)
        assert np.array_equal(got.G, want.G) and got.accepted.tolist() == want.accepted.tolist() and got.sweeps_used == want.sweeps_used
        assert got.score == want.score and got.score0 == want.score0 and got.objective == got.score and got.objective0 == got.score0
        assert got.count_a == [8] * len(joints) == got.count_b and int(want.accepted.sum()) > 0
        for e in range(len(joints)):
            assert got.kept_a[e].tolist() == list(range(8)) == got.kept_b[e].tolist() and got.joint_score[e] == want.joint_score[e]


@pytest.mark.parametrize("graph", jm.GRAPHS)
def test_the_objective_never_rises_along_a_run(graph):
    fell = trimmed = 0
    for P in ja.trajectory_cases(graph)[:6]:
        got = ja.refine(P, 4)
        assert all(b <= a for a, b in zip(got.objectives, got.objectives[1:])) and got.objective <= got.objective0
        assert got.objective == pytest.approx(got.objectives[-1], rel=1e-12)
        fell += got.objective < got.objective0
        trimmed += min(got.count_a) < ja.TRAJECTORY_K
        assert all(P.lo_a <= m <= ja.TRAJECTORY_K for m in got.count_a + got.count_b)
    assert fell > 0 and trimmed > 0


def test_counts_of_a_single_joint_are_the_pair_rule_s():
    """One joint, the root fixed: under G0 the joint's row minima are a pair problem's, and its counts _icp_auto_ref.counts of
    them; with the root at the identity they are _icp_auto_ref.objective's of (A, B, G0[1])."""
    rng = np.random.default_rng(9050)
    for n in (5, 8, 12, 16):
        P, _, _ = jt.partial_puzzle(rng, 2, [(0, 1)], 16, None, n_mate=[n], quick=True)
        P = ja.with_least(P)
        g0 = jr.f32(P.G0)
        o = ja.joint_energy(P, g0, 0)
        D = jr._D(P, g0, 0)
        assert o.m_a == au.counts(D.min(axis=1), P.lo_a, P.power) and o.m_b == au.counts(D.min(axis=0), P.lo_b, P.power)
        assert P.lo_a == au.least_count(16) == 4
        # the root at the identity: the pair statement itself
        A0 = [(P.A[0].astype(np.float64) @ g0[0][:3, :3].T + g0[0][:3, 3])]
        Q = ja.AutoPuzzle(2, P.joints, A0, P.B, np.stack([np.eye(4), g0[1]]), P.truth, P.movable, P.lo_a, P.lo_b, P.power)
        q = ja.joint_energy(Q, Q.G0, 0)
        w = au.objective(A0[0], P.B[0].astype(np.float64), g0[1], P.lo_a, P.lo_b, P.power)
        assert (q.m_a, q.m_b) == (w.m_a, w.m_b) == (o.m_a, o.m_b) and q.kept_a.tolist() == w.kept_a.tolist()
        assert q.F == pytest.approx(w.F, rel=1e-12) and q.E == pytest.approx(w.E, rel=1e-12)


def test_lattice_counts_follow_from_integers_and_agree_with_the_float64_statement_off_ties():
    rng = np.random.default_rng(9060)
    K, joints = jr.GRAPHS["ring4"]
    P = jm.lattice_puzzle(rng, K, joints, (37, 29), [(37, 29)] * len(joints))
    clear = 0
    for e in range(len(joints)):
        w = ja.lattice_joint(P, e, 10, 8, 3)
        assert 10 <= w["count_a"] <= 37 and 8 <= w["count_b"] <= 29 and len(w["kept_a"]) == w["count_a"]
        o = ja.joint_energy(ja.with_auto(P, 10, 8, 3), P.G0.astype(np.float64), e)
        assert o.kept_a.tolist() == w["kept_a"].tolist() or w["how_a"] != "clear"
        if w["how_a"] != "tie":      # (on an exact tie the float64 quotients of two equal rationals are equal too: the larger m)
            assert o.m_a == w["count_a"]
        clear += w["how_a"] == "clear"
        assert ja.lattice_joint(P, e, 37, 29, 3)["how_a"] == "only"


# ---------------------------------------------------------------------------------------------- the committed left-out counts

@pytest.mark.parametrize("graph", jm.VISIT_GRAPHS)
def test_visit_family_leaves_out_what_is_committed(graph):
    rows = [ja.visit_row(P) for P in ja.visit_cases(graph)]
    left = sum(not r[2] for r in rows)
    print(f"{graph}: {left} of {len(rows)} left out; largest yardstick error {max(r[1] for r in rows):.2e}")
    assert left == ja.VISIT[graph] and 8 * left <= len(rows), (graph, left)


@pytest.mark.parametrize("graph", jm.GRAPHS)
def test_trajectory_family_leaves_out_what_is_committed(graph):
    rows = [ja.trajectory_row(P) for P in ja.trajectory_cases(graph)]
    left = sum(not entered for _, entered in rows)
    print(f"{graph}: {left} of {len(rows)} left out; accepted visits {[int(w.accepted.sum()) for w, _ in rows]}")
    assert left == ja.TRAJECTORY[graph] and 8 * left <= len(rows), (graph, left)
    assert sum(int(w.accepted.sum()) for w, _ in rows) > 0 and any(min(w.count_a) < ja.TRAJECTORY_K for w, _ in rows)


# ---------------------------------------------------------------------------------------------- does the rule help?

def test_the_rule_is_worth_something_on_shares_that_differ_per_joint(capsys):
    """The mean pose error against the truth of (a) the untrimmed joint refinement, (b) one share for all joints (the mean true
    share), (c) the auto rule with AutoKeep()'s defaults and (d) the oracle over the true mating rows, on ring4 and complete5
    puzzles whose joints draw their shares from _icp_auto_ref.SHARES.  Measured 2026-10 (DESIGN section 5 holds the table):
    ring4 1.229 / 0.855 / 0.0808 / 0.0619, complete5 0.519 / 0.351 / 0.0301 / 0.0148."""
    means = {}
    for graph in ja.SHARE_GRAPHS:
        cases = ja.share_cases(graph)
        assert all(float(c[3].min()) <= 0.5 for c in cases) and any(len(set(c[3].tolist())) > 1 for c in cases)
        rows = np.array([ja.share_variants(c) for c in cases])
        means[graph] = rows.mean(axis=0)
        with capsys.disabled():
            print(f"\n{graph}: mean pose error (a) untrimmed {means[graph][0]:.4f}  (b) one share {means[graph][1]:.4f}  "
                  f"(c) auto {means[graph][2]:.4f}  (d) mating rows only {means[graph][3]:.4f}")
    for graph, (a, b, c, d) in means.items():
        assert c < a, (graph, a, b, c, d)


# ---------------------------------------------------------------------------------------------- the host side

def _tables_of_nones():
    from puzzlenet_amd import assembly
    return {t.__name__: t(*([None] * len(t._fields))) for t in (assembly.PairTable, assembly.TrimmedPairTable, assembly.AutoPairTable)}


def test_auto_keyword_is_decided_before_any_tensor_is_touched():
    from puzzlenet_amd import _lib, assembly
    tables = _tables_of_nones()
    assert assembly.AutoJointRefined._fields == assembly.TrimmedJointRefined._fields + ("objective", "objective0")
    for fn in (assembly.refine_assembly, assembly.refine_assembly_batch):
        for name, table in tables.items():
            # auto with keep, or with kept="frozen": the counts are found, given or frozen
            for extra in (dict(keep=0.5), dict(keep=(0.5, 1.0)), dict(keep="table"), dict(kept="frozen"), dict(kept="frozen", keep=0.5)):
                for auto in (True, assembly.AutoKeep(), assembly.AutoKeep(0.5, 2)):
                    with pytest.raises(_lib.PznError, match="auto") as info:
                        fn(None, table, None, auto=auto, **extra)
                    assert not isinstance(info.value, _lib.PznUnsupported), (name, extra)
            # no rule it knows
            for bad in ("auto", 0.5, 1, (0.25, 3), False, assembly.AutoKeep(least=0.0), assembly.AutoKeep(least=1.5),
                        assembly.AutoKeep(power=0), assembly.AutoKeep(power=5), assembly.AutoKeep(power=2.0)):
                with pytest.raises(_lib.PznError) as info:
                    fn(None, table, None, auto=bad)
                assert not isinstance(info.value, _lib.PznUnsupported), (name, bad)
            # what is accepted is let through to the next check, the pieces that are no tensor - an AutoPairTable included: auto
            # names the choice the default refuses to make
            for auto in (True, assembly.AutoKeep(), assembly.AutoKeep(least=1.0), assembly.AutoKeep((0.25, 0.5), 1)):
                with pytest.raises(_lib.PznError, match="pieces must be a tensor") as info:
                    fn(None, table, None, auto=auto)
                assert not isinstance(info.value, _lib.PznUnsupported), (name, auto)
        # the existing refusals are unchanged: keep does not find counts, and the default refuses an auto table
        for bad in ("auto", assembly.AutoKeep()):
            with pytest.raises(_lib.PznError, match="keep") as info:
                fn(None, tables["AutoPairTable"], None, keep=bad)
            assert not isinstance(info.value, _lib.PznUnsupported)
        with pytest.raises(_lib.PznUnsupported, match="per pair"):
            fn(None, tables["AutoPairTable"], None)
        with pytest.raises(_lib.PznUnsupported, match="per pair"):
            fn(None, tables["AutoPairTable"], None, auto=None)


def test_entry_point_is_declared_and_bound_from_the_header():
    from puzzlenet_amd import _lib, build, ops
    lib = _lib.load()
    assert getattr(lib, "pzn_joint_refine_auto_f32") is not None and getattr(lib, "pzn_joint_refine_auto_supported") is not None
    assert dict(build.SOURCES)["jointauto.hip"] == dict(build.SOURCES)["jointtrim.hip"] and "-ffp-contract=off" in dict(build.SOURCES)["jointauto.hip"]
    ok = ops.joint_refine_auto_supported
    assert ok(64, 64 * 63, 1024, 1024, 1, 1, 4) and ok(64, 64 * 63, 1024, 1024, 1024, 1024, 1) and ok(1, 0, 1, 1, 1, 1, 1)
    for bad in ((65, 0, 8, 8, 2, 2, 3), (4, 13, 8, 8, 2, 2, 3), (4, 12, 1025, 8, 2, 2, 3), (4, 12, 8, 0, 2, 1, 3), (4, 12, 8, 8, 0, 2, 3),
                (4, 12, 8, 8, 2, 0, 3), (4, 12, 8, 8, 9, 2, 3), (4, 12, 8, 8, 2, 9, 3), (4, 12, 8, 8, 2, 2, 0), (4, 12, 8, 8, 2, 2, 5)):
        assert not ok(*bad), bad


def test_auto_kernel_keeps_its_float64_sums_and_ranks_in_registers():
    """tests/test_joint_trim_cpu.py's check for the kernel of jointauto.hip: no vector register is spilled, there is no private
    segment (the ranks of a thread's rows and its 22 float64 sums stay in registers), all LDS is dynamic, and the file holds
    this one kernel."""
    import os
    import re
    import subprocess
    import tempfile
    from puzzlenet_amd import build
    flags = [f for f in build.COMMON if f not in ("-fPIC", "-fvisibility=hidden")]
    extra = dict(build.SOURCES)["jointauto.hip"]
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "jointauto.s")
        cmd = [build.hipcc()] + flags + extra + ["-S", "--cuda-device-only", "-o", out, os.path.join(build.CSRC, "jointauto.hip")]
        assert subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL).returncode == 0
        text = open(out).read()
    meta = text[text.index("amdhsa.kernels:"):]
    entries = {re.search(r"\.name:\s+(\S+)", e).group(1): e for e in re.split(r"\n  - ", meta)[1:] if re.search(r"\.name:\s+(\S+)", e)}
    names = [n for n in entries if "joint" in n]
    assert len(names) == 1 and "joint_auto_kernel" in names[0], names
    e = entries[names[0]]
    assert int(re.search(r"\.vgpr_spill_count:\s+(\d+)", e).group(1)) == 0
    assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", e).group(1)) == 0
    assert int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", e).group(1)) == 0
    assert int(re.search(r"\.max_flat_workgroup_size:\s+(\d+)", e).group(1)) == 256
