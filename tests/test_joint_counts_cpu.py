"""CPU: the float64 side and the host side of the joint refinement with a point count per set (pzn_joint_refine_counts_f32,
ops.joint_refine(..., na=, nb=), assembly.refine_assembly(..., kept=)): the two case families of tests/_joint_counts.py that
tests/test_gpu_joint_counts.py holds the kernel to - how many of their cases the float64 rules leave out, on the same seeds -,
the `kept` keyword before any tensor is touched, and the header, the bindings and the registers of the new kernel."""
import numpy as np
import pytest

from tests import _joint_counts as jc
from tests import _joint_ref as jr


def test_stack_puts_every_set_in_its_first_rows_and_the_fill_behind():
    cases = jc.visit_cases("both3")[:3]
    a, b, na, nb, joints, G0, movable = jc.stack(cases, (8, 9), float("nan"))
    J = len(cases[0].joints)
    assert a.shape == (3 * J, 8, 3) and b.shape == (3 * J, 9, 3) and joints.shape == (3, J, 2) and G0.shape == (3, 3, 4, 4)
    assert na.dtype == nb.dtype == joints.dtype and str(na.dtype) == "torch.int32" and movable.tolist() == [[0, 1, 0]] * 3
    for z, P in enumerate(cases):
        for e in range(J):
            r = z * J + e
            assert int(na[r]) == len(P.A[e]) and int(nb[r]) == len(P.B[e])
            assert np.array_equal(a[r, :na[r]].numpy(), P.A[e]) and bool(a[r, na[r]:].isnan().all())
            assert np.array_equal(b[r, :nb[r]].numpy(), P.B[e]) and bool(b[r, nb[r]:].isnan().all())
    assert len({(int(x), int(y)) for x, y in zip(na, nb)}) > 4          # the counts do differ from joint to joint


@pytest.mark.parametrize("graph", jc.GRAPHS)
def test_ragged_refine_descends_and_the_trajectory_family_stays_in(graph):
    """The float64 loop on sets of different sizes never raises the energy, and the cases it leaves out of the trajectory
    check (a nearest-neighbour margin below MARGIN_FACTOR bounds at a pose it evaluated) are those _joint_counts.TRAJECTORY
    pins: at most 4 of 16."""
    cases = jc.trajectory_cases(graph)
    assert len(cases) == jc.TRAJECTORY_CASES == 16
    counts = {len(A) for P in cases for A in P.A}
    assert counts <= set(range(3, 9)) and len(counts) >= 4
    assert all(len(A) == len(B) for P in cases for A, B in zip(P.A, P.B))
    left = 0
    for P in cases:
        out = jr.refine(P, jc.TRAJECTORY_SWEEPS)
        assert all(y <= x for x, y in zip(out.scores, out.scores[1:])) and out.score < out.score0
        left += out.margin_ratio < jc.MARGIN_FACTOR
    print(f"{graph}: left out {left} of {len(cases)}")
    assert left == jc.TRAJECTORY[graph] and left <= 4, (graph, left)


def test_three_quarters_of_the_one_visit_family_enter():
    entered = total = 0
    for graph in jc.VISIT_GRAPHS:
        cases = jc.visit_cases(graph)
        assert len(cases) == jc.VISIT_CASES == 24
        sizes = {len(s) for P in cases for s in P.A + P.B}
        assert sizes == set(range(1, 9))                                 # count 1 and the float4 tail's 3, 4, 5 are there
        assert any(len(A) != len(B) for P in cases for A, B in zip(P.A, P.B))
        assert all(P.movable.tolist() == [p == 1 for p in range(P.K)] for P in cases)
        rows = [jc.visit_row(P) for P in cases]
        print(f"{graph}: entered {sum(r[2] for r in rows)} of {len(rows)}, yardstick max {max(r[1] for r in rows):.3e}, "
              f"with a unique optimum {sum(r[3] >= jc.GAP_MIN for r in rows)}, their yardstick max "
              f"{max(r[1] for r in rows if r[3] >= jc.GAP_MIN):.3e}, smallest gap {min(r[3] for r in rows):.1e}")
        entered += sum(r[2] for r in rows)
        total += len(rows)
    print(f"all: entered {entered} of {total}")
    assert total == 96 and 4 * entered >= 3 * total, (entered, total)


def _auto_table_of_nones():
    from puzzlenet_amd import assembly
    return assembly.AutoPairTable(*([None] * len(assembly.AutoPairTable._fields)))


def test_kept_keyword_is_decided_before_any_tensor_is_touched():
    from puzzlenet_amd import _lib, assembly
    table = _auto_table_of_nones()
    assert "per pair" in assembly.AUTO_JOINT_MESSAGE and "kept='frozen'" in assembly.AUTO_JOINT_MESSAGE
    for fn in (assembly.refine_assembly, assembly.refine_assembly_batch):
        with pytest.raises(_lib.PznUnsupported, match="per pair"):       # the default still refuses an auto table
            fn(None, table, None)
        with pytest.raises(_lib.PznUnsupported, match="per pair"):
            fn(None, table, None, kept=None)
        for bad in ("Frozen", "retrim", True, 0):
            for t in (table, assembly.PairTable(*([None] * 8))):
                with pytest.raises(_lib.PznError, match="kept") as info:
                    fn(None, t, None, kept=bad)
                assert not isinstance(info.value, _lib.PznUnsupported), bad


def test_header_declares_and_the_library_exports_the_counts_entry_point():
    from puzzlenet_amd import _lib
    old, new = _lib.PARAMS["pzn_joint_refine_f32"], _lib.PARAMS["pzn_joint_refine_counts_f32"]
    assert len(old) == 20 and len(new) == 22
    assert new[2] == "const int32_t* na" and new[5] == "const int32_t* nb"
    assert [p for n, p in enumerate(new) if n not in (2, 5)] == old      # the old parameters in the old order around them
    assert _lib.SIGNATURES["pzn_joint_refine_counts_f32"][0] is _lib.SIGNATURES["pzn_joint_refine_f32"][0]
    assert getattr(_lib.load(), "pzn_joint_refine_counts_f32") is not None


def test_counts_kernel_keeps_its_float64_sums_and_solve_in_registers():
    """tests/test_joint_ref_cpu.py's check for joint_refine_kernel, for the kernel beside it: joint_refine_counts_kernel is
    the same body with two more uniform loads per joint row, and spills no vector register either; and the file still holds
    exactly these two kernels."""
    import os
    import re
    import subprocess
    import tempfile
    from puzzlenet_amd import build
    flags = [f for f in build.COMMON if f not in ("-fPIC", "-fvisibility=hidden")]
    extra = dict(build.SOURCES)["jointrefine.hip"]
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "jointrefine.s")
        cmd = [build.hipcc()] + flags + extra + ["-S", "--cuda-device-only", "-o", out, os.path.join(build.CSRC, "jointrefine.hip")]
        assert subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL).returncode == 0
        text = open(out).read()
    meta = text[text.index("amdhsa.kernels:"):]
    entries = {re.search(r"\.name:\s+(\S+)", e).group(1): e for e in re.split(r"\n  - ", meta)[1:] if re.search(r"\.name:\s+(\S+)", e)}
    names = [n for n in entries if "joint_refine" in n]
    assert len(names) == 2 and sum("joint_refine_counts_kernel" in n for n in names) == 1, names
    for n in names:
        assert int(re.search(r"\.vgpr_spill_count:\s+(\d+)", entries[n]).group(1)) == 0, n
        assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", entries[n]).group(1)) == 0, n
    lds = {n: int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", entries[n]).group(1)) for n in names}
    assert len(set(lds.values())) == 1, lds                              # the counts add nothing to the static LDS either
