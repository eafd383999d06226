"""CPU: the float64 restatement of the pose refinement (tests/_icp_ref.py) on its own - what tests/test_gpu_icp_refine.py
holds the kernel to has to be right first - and the binding's refusal of CPU tensors."""
import numpy as np
import pytest

from tests import _icp_ref as ref


def _angle(R):
    return float(np.degrees(np.arccos(np.clip((np.trace(R) - 1.0) / 2.0, -1.0, 1.0))))


@pytest.mark.parametrize("planar", [False, True], ids=["space", "planar"])
@pytest.mark.parametrize("k", [(8, 8), (24, 24), (37, 130), (128, 128), (257, 300)], ids=lambda k: f"{k[0]}x{k[1]}")
def test_score_is_monotone_and_motion_is_recovered(k, planar):
    """Every accepted step lowers E strictly, planar loops included (the cross-covariance has rank 2 there).  Where the
    samplings are dense enough for nearest neighbours to mean something (128 points and more on a curve about 2.5 long:
    a spacing of 0.02, below the 0.03 the start is off by), the loop ends at the known motion of two DIFFERENT samplings of
    one noisy curve to within that spacing: 0.02, and the 2 degrees it subtends at the curve's radius of 0.5."""
    rng = np.random.default_rng(100 + k[0] + 7 * planar)
    for _ in range(4):
        c = ref.curve_case(rng, k[0], k[1], planar)
        r = ref.refine(c.a, c.b, c.T0, 40)
        assert all(y < x for x, y in zip(r.scores, r.scores[1:]))
        assert r.score == r.scores[-1] and r.score0 == r.scores[0] and r.iters_used == len(r.scores) - 1
        assert r.iters_used >= 1 and r.score < r.score0
        assert r.T.astype(np.float32).astype(np.float64).tolist() == r.T.tolist()      # float32 values
        R = r.T[:3, :3]
        assert np.abs(R.T @ R - np.eye(3)).max() < 2.0 ** -21 and np.linalg.det(R) > 0
        D0, D1 = c.T0.astype(np.float64) @ np.linalg.inv(c.G), r.T @ np.linalg.inv(c.G)
        tb = ref.transform(c.G, c.b)
        off0 = np.abs(ref.transform(D0, tb) - tb).max()
        off1 = np.abs(ref.transform(D1, tb) - tb).max()
        if min(k) >= 128:
            assert _angle(D1[:3, :3]) < 2.0 and off1 < 0.02, (_angle(D1[:3, :3]), off1)
            assert off1 < off0


def test_step_is_the_least_squares_motion():
    """With exact correspondences of a rigidly moved set, one step returns the motion; and no nearby rigid motion has a
    smaller sum over the pairs."""
    rng = np.random.default_rng(5)
    b = rng.uniform(-0.5, 0.5, (20, 3))
    G = ref.rigid(ref.rot(rng.normal(size=3), 1.1), rng.uniform(-0.3, 0.3, 3))
    a = ref.transform(G, b)
    ident = np.arange(20)
    np.testing.assert_allclose(ref.step(a, b, ident, ident, np.eye(4)), G, atol=1e-13)
    a = a + rng.normal(scale=0.01, size=a.shape)
    c1, c2 = rng.integers(0, 20, 20), rng.integers(0, 20, 20)
    T = ref.step(a, b, c1, c2, np.eye(4))

    def cost(M):
        tb = ref.transform(M, b)
        return ((a - tb[c1]) ** 2).sum() + ((a[c2] - tb) ** 2).sum()
    for _ in range(20):
        d = ref.rigid(ref.rot(rng.normal(size=3), rng.normal(scale=1e-3)), rng.normal(scale=1e-3, size=3))
        assert cost(T) <= cost(d @ T)
    assert np.linalg.det(T[:3, :3]) > 0


def test_reflection_fix():
    """Pairs that a reflection would fit best still give a proper rotation."""
    rng = np.random.default_rng(6)
    b = rng.uniform(-0.5, 0.5, (12, 3))
    a = b * np.array([1.0, 1.0, -1.0])
    ident = np.arange(12)
    T = ref.step(a, b, ident, ident, np.eye(4))
    assert abs(np.linalg.det(T[:3, :3]) - 1.0) < 1e-12


def test_ties_take_the_lowest_index():
    a = np.array([[0.0, 0.0, 0.0]])
    b = np.array([[1.0, 0.0, 0.0], [-1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    _, c1, c2, margin = ref.objective(a, b, np.eye(4))
    assert c1.tolist() == [0] and c2.tolist() == [0, 0, 0] and margin == 0.0


@pytest.mark.parametrize("kind", ["single", "coincident", "collinear"])
def test_degenerate_sets_move_by_translation_only(kind):
    """A single point, coincident points and collinear moved-side points keep the rotation they came with; the translation
    still moves the set onto its partner."""
    rng = np.random.default_rng(7)
    R0 = ref.rot([1.0, 2.0, 3.0], 0.4).astype(np.float32).astype(np.float64)
    T0 = ref.rigid(R0, [0.1, -0.2, 0.05])
    if kind == "single":
        a, b = rng.uniform(-0.5, 0.5, (1, 3)), rng.uniform(-0.5, 0.5, (1, 3))
    elif kind == "coincident":
        a, b = rng.uniform(-0.5, 0.5, (5, 3)), np.tile(rng.uniform(-0.5, 0.5, (1, 3)), (4, 1))
    else:
        a = rng.uniform(-0.5, 0.5, (6, 3))
        b = rng.uniform(-0.5, 0.5, (1, 3)) + np.linspace(-1, 1, 7)[:, None] * rng.normal(size=(1, 3))
    a, b = a.astype(np.float32), b.astype(np.float32)
    r = ref.refine(a, b, T0, 10)
    assert np.array_equal(r.T[:3, :3], R0)
    assert r.score <= r.score0
    if kind == "single":
        assert r.iters_used == 1 and r.score < 1e-12
        np.testing.assert_allclose(ref.transform(r.T, b), a, atol=1e-6)
    # a regular set right next to it does turn
    c = ref.curve_case(rng, 6, 7, False)
    assert not np.array_equal(ref.refine(c.a, c.b, c.T0, 10).T[:3, :3], c.T0[:3, :3].astype(np.float64))


def test_degenerate_threshold_separates_clearly():
    rng = np.random.default_rng(8)
    line = (rng.uniform(-0.5, 0.5, (1, 3)) + np.linspace(-1, 1, 50)[:, None] * rng.normal(size=(1, 3))).astype(np.float32)
    q = line.astype(np.float64) - line.astype(np.float64).mean(axis=0)
    assert ref.is_degenerate(q.T @ q)                                  # float32 rounding off the line: far below 1e-10
    q = ref.curve(rng.uniform(0, 1, 50), True)
    q = q - q.mean(axis=0)
    assert not ref.is_degenerate(q.T @ q)
    assert ref.is_degenerate(np.zeros((3, 3)))


def test_yardstick_is_close_to_the_float64_step():
    rng = np.random.default_rng(9)
    c = ref.curve_case(rng, 64, 65, False)
    _, c1, c2, _ = ref.objective(c.a, c.b, c.T0)
    assert ref.pose_err(ref.step_f32(c.a, c.b, c1, c2, c.T0), ref.step(c.a, c.b, c1, c2, c.T0)) < 1e-5


def test_distance_bound_covers_float32_distances():
    """The bound the GPU tests use holds for float32 arithmetic written out in NumPy (each operation rounds once)."""
    rng = np.random.default_rng(10)
    for _ in range(5):
        c = ref.curve_case(rng, 40, 50, False)
        T = c.T0
        tb = np.empty((50, 3), dtype=np.float32)
        for u in range(3):
            tb[:, u] = ((T[u, 0] * c.b[:, 0] + T[u, 1] * c.b[:, 1]) + T[u, 2] * c.b[:, 2]) + T[u, 3]
        d = c.a[:, None, :] - tb[None, :, :]
        d32 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        assert d32.dtype == np.float32
        err = np.abs(d32.astype(np.float64) - ref.sqdist(c.a, ref.transform(T, c.b)))
        assert (err <= ref.distance_bound(c.a, c.b, T)).all()
        lo, hi = ref.objective_interval(c.a, c.b, T)
        e32 = d32.min(axis=1).mean(dtype=np.float32) + d32.min(axis=0).mean(dtype=np.float32)
        assert lo <= float(e32) <= hi


def test_icp_refine_rejects_cpu_tensors():
    import torch
    from puzzlenet_amd import _lib, ops
    with pytest.raises(_lib.PznError):
        ops.icp_refine(torch.zeros(1, 8, 3), torch.zeros(1, 8, 3), torch.eye(4).reshape(1, 4, 4), 3)


def test_icp_kernel_keeps_its_float64_solve_in_registers():
    """icp_refine_kernel's Jacobi sweeps index their 4x4 matrices with compile-time constants only: no vector register is
    spilled and there is no scratch (a dynamically indexed array would live there)."""
    import os
    import re
    import subprocess
    import tempfile
    from puzzlenet_amd import build
    flags = [f for f in build.COMMON if f not in ("-fPIC", "-fvisibility=hidden")]
    extra = dict(build.SOURCES)["icprefine.hip"]
    assert "-ffp-contract=off" in extra                                  # a refined pose moves points as mergefps.hip does
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "icprefine.s")
        cmd = [build.hipcc()] + flags + extra + ["-S", "--cuda-device-only", "-o", out, os.path.join(build.CSRC, "icprefine.hip")]
        assert subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL).returncode == 0
        text = open(out).read()
    meta = text[text.index("amdhsa.kernels:"):]
    entries = [e for e in re.split(r"\n  - ", meta)[1:] if "icp_refine_kernel" in (re.search(r"\.name:\s+(\S+)", e) or [""])[0]]
    assert len(entries) == 1
    e = entries[0]
    assert int(re.search(r"\.vgpr_spill_count:\s+(\d+)", e).group(1)) == 0
    assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", e).group(1)) == 0
