"""CPU: the float64 restatement of the joint pose refinement (tests/_joint_ref.py) on its own - what
tests/test_gpu_joint_refine.py holds the kernel to has to be right first - and the counts of cases that the GPU trajectory
test leaves out, on the same seeds."""
import numpy as np
import pytest
import torch

from tests import _icp_ref as ref
from tests import _joint_ref as jr


def test_visit_with_exact_correspondences_and_no_noise_returns_the_truth():
    rng = np.random.default_rng(11)
    K, joints = jr.GRAPHS["ring4"]
    P = jr.puzzle(rng, K, joints, 16, same=True, noise=0.0)
    G = jr.f32(P.G0)
    G[0], G[2] = P.truth[0], P.truth[2]                      # piece 1's neighbours at the truth (float64 values)
    corr = {e: jr.joint_energy(P, P.truth, e)[1:3] for e in jr.incident(P, 1)}      # at the truth: the permutation
    cand = jr.visit(P, G, 1, corr, round32=False)
    assert ref.pose_err(cand, P.truth[1]) <= 1e-6            # the points are float32 roundings of exact images
    # and with the float32 yardstick, from the same pairs
    assert ref.pose_err(jr.visit_f32(P, G.astype(np.float32), 1, corr), P.truth[1]) <= 1e-4


@pytest.mark.parametrize("graph", ["pair", "chain3", "ring4", "both3", "complete5"])
def test_energy_never_rises_along_refine(graph):
    rng = np.random.default_rng(23)
    K, joints = jr.GRAPHS[graph]
    P = jr.puzzle(rng, K, joints, (9, 12))
    out = jr.refine(P, 8)
    assert all(b <= a for a, b in zip(out.scores, out.scores[1:])), out.scores
    assert out.score <= out.score0 and out.score == out.scores[-1]
    assert out.sweeps_used == len(out.scores) - 1 and out.accepted[0] == 0
    # a visit alone never raises the total either
    G = jr.f32(P.G0)
    for p in range(1, K):
        before = jr.total(P, G)[0]
        Ep = jr.piece_energy(P, G, p)[0]
        Gn = G.copy()
        Gn[p] = jr.visit(P, G, p)
        if jr.piece_energy(P, Gn, p)[0] < Ep:
            assert jr.total(P, Gn)[0] < before
            G = Gn


def test_ring_of_four_ends_nearer_the_truth():
    rng = np.random.default_rng(5)
    K, joints = jr.GRAPHS["ring4"]
    for _ in range(4):
        P = jr.puzzle(rng, K, joints, 24, same=True)
        out = jr.refine(P, 30)
        before, after = jr.pose_error(P.G0, P.truth), jr.pose_error(out.G, P.truth)
        assert after[1:].max() < before[1:].max(), (before, after)
        assert out.score < out.score0


def test_two_pieces_one_joint_is_the_pairwise_loop_step_for_step():
    rng = np.random.default_rng(3)
    for n in range(6):
        c = ref.curve_case(rng, 12, 12, planar=bool(n & 1))
        G0 = np.stack([np.eye(4, dtype=np.float32), c.T0])
        P = jr.Puzzle(2, [(0, 1)], [c.a], [c.b], G0, None, np.array([False, True]))
        want = ref.refine(c.a, c.b, c.T0, 30)
        out = jr.refine(P, 30)
        assert out.sweeps_used == want.iters_used and out.accepted.tolist() == [0, want.iters_used]
        np.testing.assert_allclose(out.scores, want.scores, rtol=1e-9, atol=0)
        assert ref.pose_err(out.G[1], want.T) <= 2.0 ** -22      # the same float32 values up to a last-place flip
        assert np.array_equal(out.G[0], np.eye(4))


def test_distance_bound2_covers_float32_written_out_operation_by_operation():
    rng = np.random.default_rng(9)
    K, joints = jr.GRAPHS["pair"]
    P = jr.puzzle(rng, K, joints, (7, 9))
    G = jr.f32(P.G0)
    B2 = jr.distance_bound2(P.A[0], P.B[0], G[0], G[1])
    # float32, operation by operation, against float64
    def move32(T, x):
        T, x = T.astype(np.float32), x.astype(np.float32)
        return np.stack([((T[r, 0] * x[:, 0] + T[r, 1] * x[:, 1]) + T[r, 2] * x[:, 2]) + T[r, 3] for r in range(3)], axis=-1)
    d = move32(P.G0[0], P.A[0])[:, None, :] - move32(P.G0[1], P.B[0])[None, :, :]
    d32 = ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]).astype(np.float64)
    assert d32.dtype == np.float64 and d.dtype == np.float32
    D = ref.sqdist(ref.transform(G[0], P.A[0]), ref.transform(G[1], P.B[0]))
    assert (np.abs(d32 - D) <= B2).all()
    lo, hi = jr.objective_interval2(P.A[0], P.B[0], G[0], G[1])
    assert lo <= jr.joint_energy(P, G, 0)[0] <= hi


# the cases of tests/test_gpu_joint_refine.py's trajectory test: 16 per graph, k = 8, 2 sweeps, same = True
def test_trajectory_cases_left_out():
    from tests.test_gpu_joint_refine import MARGIN_FACTOR, TRAJECTORY, trajectory_cases
    for graph, want in TRAJECTORY.items():
        cases = trajectory_cases(graph)
        left = sum(jr.refine(P, 2).margin_ratio < MARGIN_FACTOR for P in cases)
        print(f"{graph}: left out {left} of {len(cases)}")
        assert left == want and left <= len(cases) // 4, (graph, left)


def test_joint_refine_rejects_cpu_tensors():
    from puzzlenet_amd import _lib, ops
    with pytest.raises(_lib.PznError):
        ops.joint_refine(torch.zeros(1, 8, 3), torch.zeros(1, 8, 3), torch.zeros(1, 1, 2, dtype=torch.int32),
                         torch.eye(4).reshape(1, 1, 4, 4).repeat(1, 2, 1, 1), torch.ones(1, 2, dtype=torch.uint8), 3)


def test_joint_kernel_keeps_its_float64_sums_and_solve_in_registers():
    """joint_refine_kernel carries 22 float64 sums per thread across the joints of a visit and shares icp_refine_kernel's
    Jacobi sweeps: no vector register is spilled and there is no scratch (tests/test_icp_cpu.py's check, for this kernel),
    and the file is built without fma contraction, as icprefine.hip is."""
    import os
    import re
    import subprocess
    import tempfile
    from puzzlenet_amd import build
    flags = [f for f in build.COMMON if f not in ("-fPIC", "-fvisibility=hidden")]
    extra = dict(build.SOURCES)["jointrefine.hip"]
    assert "-ffp-contract=off" in extra and extra == dict(build.SOURCES)["icprefine.hip"]
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "jointrefine.s")
        cmd = [build.hipcc()] + flags + extra + ["-S", "--cuda-device-only", "-o", out, os.path.join(build.CSRC, "jointrefine.hip")]
        assert subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL).returncode == 0
        text = open(out).read()
    meta = text[text.index("amdhsa.kernels:"):]
    entries = [e for e in re.split(r"\n  - ", meta)[1:] if "joint_refine_kernel" in (re.search(r"\.name:\s+(\S+)", e) or [""])[0]]
    assert len(entries) == 1
    e = entries[0]
    assert int(re.search(r"\.vgpr_spill_count:\s+(\d+)", e).group(1)) == 0
    assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", e).group(1)) == 0
