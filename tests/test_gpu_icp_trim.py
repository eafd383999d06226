"""GPU: ops.icp_refine(..., keep=(m_a, m_b)) (csrc/icprefine.hip, icp_trim_kernel) - the pose refinement for partial contact,
of each direction's rows only the m with the smallest (minimum, index) - against the untrimmed kernel where every row is
kept and against the float64 statement tests/_icp_trim_ref.py elsewhere.

What is compared with what, and where the bounds come from (nothing below is tuned to the kernel):

(a) all rows kept: the same bits as ops.icp_refine in every shared output (the contract), kept_* = 0 .. k-1.
(b) a lattice case: coordinates are multiples of 2^-6 in [0, 1), T0 translates by a lattice vector, iters = 0, m_a and m_b
    are powers of two.  Moved coordinates are multiples of 2^-6 below 2, squared distances multiples of 2^-12 below 12, the
    sum of at most 512 of them stays below 2^13 (25 bits above 2^-12 are never needed: the minima of these dense sets are
    far below 1), the quotients by powers of two and their sum are exact: float32 and float64 form the same numbers, so
    kept_a, kept_b and score0 equal the float64 statement bit for bit.  Every point stands three times in its set, so equal
    minima lie on both sides of the cut (asserted on the float64 side).
(c) kept sets under T0 on curve data: with B = the largest _icp_ref.distance_bound of the case, a float32 row minimum is
    within B of the float64 one.  A kept row r and the n - m dropped rows q satisfy min32(r) <= min32(q), so at most m - 1
    other rows have a float64 minimum below min64(r) - 2 B: min64(r) <= (m+1)-th smallest + 2 B.  Likewise a dropped row's
    minimum is no more than 2 B below the m-th smallest.  Scores: _icp_trim_ref.objective_interval (the sum of the m
    smallest is monotone in every term, so _icp_ref's interval carries over).
(d) trajectory: the float64 loop against the device's, iters_used equal and the final pose within STEP_FACTOR times the
    largest error of the float32 restatement of one step (_icp_trim_ref.step_f32 against step, at the start pose of every
    case of (d): tests/test_gpu_icp_refine.py's tolerance form).  A case is left out when the float64 loop met a
    nearest-neighbour margin or a keep margin (the m-th against the (m+1)-th smallest minimum of a direction) below
    MARGIN_FACTOR = 16 distance bounds (_icp_ref.nearest_bound under T0, as there); at most a quarter may be left out
    (asserted; on the CPU the seeds below leave out LEFT_OUT_CPU).
"""
import numpy as np
import pytest
import torch

from tests import _icp_ref as ref
from tests import _icp_trim_ref as trim

pytestmark = pytest.mark.gpu

STEP_FACTOR = 4.0
MARGIN_FACTOR = 16.0
ITERS = 30
# (ka, kb, P): a thread owns two rows and ka != kb; more problems than the 512-workgroup grid (the LDS image and both masks
# are reused); the LDS limit (few iterations)
SHAPES = [(96, 200, 3), (8, 8, 520), (1024, 1024, 1)]
ITERS_OF = {(1024, 1024, 1): 3}
LEFT_OUT_CPU = {(8, 6, 5): 0, (24, 24, 12): 6}      # (d): cases the float64 loop alone leaves out, of 32
TRAJECTORY_SEED = {8: 6208, 24: 6300}               # chosen so that it stays within a quarter (6224, the first tried at 24, leaves out 9)


def _keeps(shape):
    ka, kb, _ = shape
    return [(1, 1), (2, 2), (ka - 1, kb - 1), (ka, kb), (ka // 2, (3 * kb) // 8), (ka, 1), (2, kb)]


CASES = [(s, m) for s in SHAPES for m in _keeps(s)]


def _ids(c):
    (ka, kb, P), (ma, mb) = c
    return f"{ka}x{kb}x{P}-keep{ma}x{mb}"


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _cases(shape):
    ka, kb, P = shape
    rng = np.random.default_rng(52000 + 7 * ka + 3 * kb + P)
    return [ref.curve_case(rng, ka, kb, planar=bool(p & 1)) for p in range(P)]


def _stack(cases, dev):
    a = torch.from_numpy(np.stack([c.a for c in cases])).to(dev)
    b = torch.from_numpy(np.stack([c.b for c in cases])).to(dev)
    T0 = torch.from_numpy(np.stack([c.T0 for c in cases])).to(dev)
    return a, b, T0


@pytest.fixture(scope="module")
def data(dev):
    """Every shape's cases on the host and on the device: made once."""
    out = {}
    for shape in SHAPES:
        cases = _cases(shape)
        out[shape] = (cases, _stack(cases, dev), ITERS_OF.get(shape, ITERS))
    return out


@pytest.fixture(scope="module")
def bounds(data):
    """Per shape and case: the float64 distances under T0 and the largest distance bound (read by (c))."""
    return {shape: [(ref.sqdist(c.a, ref.transform(c.T0, c.b)), float(ref.distance_bound(c.a, c.b, c.T0).max())) for c in cases]
            for shape, (cases, _, _) in data.items()}


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}x{s[2]}")
def test_all_rows_kept_is_the_untrimmed_kernel(data, shape):
    from puzzlenet_amd import ops
    ka, kb, P = shape
    _, (a, b, T0), iters = data[shape]
    for it in (0, 1, iters):
        want = ops.icp_refine(a, b, T0, it, return_corr=True)
        got = ops.icp_refine(a, b, T0, it, return_corr=True, keep=(ka, kb), return_kept=True)
        assert len(got) == 8
        for name, x, y in zip(("T", "score", "score0", "iters_used", "corr_a", "corr_b"), want, got):
            assert torch.equal(x, y), (it, name)
        assert torch.equal(got[6], torch.arange(ka, dtype=torch.int32, device=a.device).expand(P, ka))
        assert torch.equal(got[7], torch.arange(kb, dtype=torch.int32, device=a.device).expand(P, kb))
    # the untrimmed launch answers return_kept without a trimmed launch
    plain = ops.icp_refine(a, b, T0, 1, return_kept=True)
    assert len(plain) == 6 and torch.equal(plain[4], got[6]) and torch.equal(plain[5], got[7])


def _lattice(rng, n):
    """n rows of multiples of 2^-6 in [0, 1), every point three times in a row (the last rows fill up with new points)."""
    pts = rng.integers(0, 64, (n // 3 + 3, 3)).astype(np.float64) / 64.0
    return np.concatenate((np.repeat(pts[:n // 3], 3, axis=0), pts[n // 3:]))[:n].astype(np.float32)


@pytest.mark.parametrize("shape", [(96, 200, 4, 32, 64), (96, 200, 4, 64, 128), (8, 8, 520, 4, 2), (1024, 1024, 1, 256, 512)],
                         ids=lambda s: "x".join(str(v) for v in s))
def test_lattice_case_equals_the_float64_statement_bit_for_bit(dev, shape):
    from puzzlenet_amd import ops
    ka, kb, P, m_a, m_b = shape
    rng = np.random.default_rng(777 + ka + P)
    A = np.stack([_lattice(rng, ka) for _ in range(P)])
    B = np.stack([_lattice(rng, kb) for _ in range(P)])
    T0 = np.tile(np.eye(4, dtype=np.float32), (P, 1, 1))
    T0[:, :3, 3] = rng.integers(-8, 9, (P, 3)).astype(np.float32) / 64.0
    T, score, score0, used, kept_a, kept_b = (t.cpu().numpy() for t in ops.icp_refine(
        *(torch.from_numpy(x).to(dev) for x in (A, B, T0)), 0, keep=(m_a, m_b), return_kept=True))
    assert np.array_equal(T, T0) and (used == 0).all() and np.array_equal(score, score0)
    straddle_a = straddle_b = 0
    for p in range(P):
        o = trim.objective(A[p], B[p], T0[p], m_a, m_b)
        assert np.array_equal(kept_a[p], o.kept_a) and np.array_equal(kept_b[p], o.kept_b), p
        assert float(score0[p]) == o.E, (p, float(score0[p]), o.E)
        D = ref.sqdist(A[p], ref.transform(T0[p], B[p]))
        r1, r2 = D.min(axis=1), D.min(axis=0)
        straddle_a += int((r1 == r1[o.kept_a].max()).sum() > (r1[o.kept_a] == r1[o.kept_a].max()).sum())
        straddle_b += int((r2 == r2[o.kept_b].max()).sum() > (r2[o.kept_b] == r2[o.kept_b].max()).sum())
    # equal minima on both sides of the cut, in both directions, in at least a quarter of the problems
    assert straddle_a >= max(1, P // 4) and straddle_b >= max(1, P // 4), (straddle_a, straddle_b, P)


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_kept_sets_and_scores_against_float64(data, bounds, case):
    from puzzlenet_amd import ops
    shape, (m_a, m_b) = case
    ka, kb, P = shape
    cases, (a, b, T0), iters = data[shape]
    zero = [t.cpu().numpy() for t in ops.icp_refine(a, b, T0, 0, keep=(m_a, m_b), return_kept=True)]
    full = [t.cpu().numpy() for t in ops.icp_refine(a, b, T0, iters, keep=(m_a, m_b), return_kept=True)]
    T_0, s_0, s0_0, u_0, kept_a, kept_b = zero
    assert kept_a.shape == (P, m_a) and kept_b.shape == (P, m_b) and kept_a.dtype == np.int32
    assert np.array_equal(T_0, T0.cpu().numpy()) and (u_0 == 0).all() and np.array_equal(s_0, s0_0)
    assert np.array_equal(s0_0, full[2])
    worst = -np.inf
    for p, c in enumerate(cases):
        D, B = bounds[shape][p]
        for minima, kept, m, n in ((D.min(axis=1), kept_a[p], m_a, ka), (D.min(axis=0), kept_b[p], m_b, kb)):
            assert (np.diff(kept) > 0).all() and kept[0] >= 0 and kept[-1] < n      # ascending: m different rows
            s = np.sort(minima)
            dropped = np.setdiff1d(np.arange(n), kept)
            if m < n:
                over = minima[kept].max() - s[m]
                under = s[m - 1] - minima[dropped].min()
                worst = max(worst, (over - 2 * B) / B, (under - 2 * B) / B)
                assert over <= 2 * B and under <= 2 * B, (p, over, under, B)
        lo, hi = trim.objective_interval(c.a, c.b, c.T0, m_a, m_b)
        assert lo <= float(s0_0[p]) <= hi, (p, lo, float(s0_0[p]), hi)
        lo, hi = trim.objective_interval(c.a, c.b, full[0][p], m_a, m_b)
        assert lo <= float(full[1][p]) <= hi, (p, lo, float(full[1][p]), hi)
    print(f"{_ids(case)}: largest (excess - 2 B) / B {worst:.3g}")


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_properties(data, dev, case):
    from puzzlenet_amd import ops
    shape, keep = case
    ka, kb, P = shape
    cases, (a, b, T0), iters = data[shape]
    run = ops.icp_refine(a, b, T0, iters, keep=keep, return_corr=True, return_kept=True)
    T, score, score0, used, ca, cb, kept_a, kept_b = run
    assert T.shape == (P, 4, 4) and used.dtype == torch.int32 and kept_a.shape == (P, keep[0]) and kept_b.shape == (P, keep[1])
    assert bool((score <= score0).all())                                               # exactly, every problem
    assert int(used.min()) >= 0 and int(used.max()) <= iters
    assert bool((used[score < score0] >= 1).all()) and bool((score[used == 0] == score0[used == 0]).all())
    assert int(ca.min()) >= 0 and int(ca.max()) < kb and int(cb.min()) >= 0 and int(cb.max()) < ka
    for kept, n in ((kept_a, ka), (kept_b, kb)):
        assert int(kept.min()) >= 0 and int(kept.max()) < n
        assert kept.shape[1] == 1 or bool((kept[:, 1:] > kept[:, :-1]).all())
    # two runs: the same bits in every output
    again = ops.icp_refine(a, b, T0, iters, keep=keep, return_corr=True, return_kept=True)
    assert all(torch.equal(x, y) for x, y in zip(run, again))
    # the returned pose's kept sets are those of an evaluation of it, whether or not the last candidate was rejected
    at = ops.icp_refine(a, b, T, 0, keep=keep, return_kept=True)
    assert torch.equal(at[0], T) and torch.equal(at[1], score) and torch.equal(at[4], kept_a) and torch.equal(at[5], kept_b)
    # row maps: the same bits as the run on the materialised sets
    a_of = torch.arange(P - 1, -1, -1, dtype=torch.long, device=dev)
    b_of = torch.roll(torch.arange(P, dtype=torch.long, device=dev), 1)
    mapped = ops.icp_refine(a, b, T0, iters, a_of=a_of, b_of=b_of, keep=keep, return_corr=True, return_kept=True)
    plain = ops.icp_refine(a[a_of].contiguous(), b[b_of].contiguous(), T0, iters, keep=keep, return_corr=True, return_kept=True)
    assert all(torch.equal(x, y) for x, y in zip(mapped, plain))
    # without return_kept the same launch writes no kept sets
    short = ops.icp_refine(a, b, T0, iters, keep=keep)
    assert len(short) == 4 and all(torch.equal(x, y) for x, y in zip(short, run))


def _trajectory_cases(k, m_a, m_b):
    rng = np.random.default_rng(TRAJECTORY_SEED[k])
    if k == 8:
        return [ref.curve_case(rng, k, k, planar=bool(p & 1)) for p in range(32)]
    return [trim.partial_case(rng, k, k, 0.5, planar=bool(p & 1)) for p in range(32)]


def _left_out(c, want):
    nb = ref.nearest_bound(c.a, c.b, c.T0)
    return want.margin < MARGIN_FACTOR * nb or want.keep_margin < MARGIN_FACTOR * nb


TRAJECTORIES = [(8, 6, 5), (24, 24, 12)]


@pytest.fixture(scope="module")
def yardstick():
    """The largest error of the float32 restatement of one trimmed step, at the start pose of every case of (d)."""
    worst = 0.0
    for k, m_a, m_b in TRAJECTORIES:
        for c in _trajectory_cases(k, m_a, m_b):
            o = trim.objective(c.a, c.b, c.T0, m_a, m_b)
            want = trim.step(c.a, c.b, o.c1, o.c2, o.kept_a, o.kept_b, c.T0)
            worst = max(worst, ref.pose_err(trim.step_f32(c.a, c.b, o.c1, o.c2, o.kept_a, o.kept_b, c.T0), want))
    return worst


@pytest.mark.parametrize("traj", TRAJECTORIES, ids=lambda t: f"k{t[0]}-keep{t[1]}x{t[2]}")
def test_trajectory_follows_the_float64_loop(dev, yardstick, traj):
    from puzzlenet_amd import ops
    k, m_a, m_b = traj
    cases = _trajectory_cases(k, m_a, m_b)
    n = len(cases)
    a, b, T0 = _stack(cases, dev)
    T, score, score0, used, kept_a, kept_b = (t.cpu().numpy() for t in ops.icp_refine(a, b, T0, ITERS, keep=(m_a, m_b),
                                                                                       return_kept=True))
    tol = STEP_FACTOR * yardstick
    left_out, worst = 0, 0.0
    for p, c in enumerate(cases):
        want = trim.refine(c.a, c.b, c.T0, ITERS, m_a, m_b)
        if _left_out(c, want):
            left_out += 1
            continue
        assert int(used[p]) == want.iters_used, (p, int(used[p]), want.iters_used)
        assert np.array_equal(kept_a[p], want.kept_a) and np.array_equal(kept_b[p], want.kept_b), p
        worst = max(worst, ref.pose_err(T[p], want.T))
        assert ref.pose_err(T[p], want.T) <= tol, (p, ref.pose_err(T[p], want.T), tol)
    print(f"{traj}: left out {left_out} of {n} (CPU: {LEFT_OUT_CPU[traj]}), largest pose difference {worst:.3e} (tolerance {tol:.3e})")
    assert left_out == LEFT_OUT_CPU[traj] and left_out <= n // 4, left_out


def test_rejections_launch_nothing(dev, monkeypatch):
    from puzzlenet_amd import _lib, ops
    calls = []
    monkeypatch.setattr(ops, "_call", lambda *a, **k: calls.append(a[0]))
    eye = torch.eye(4, device=dev).reshape(1, 4, 4)
    pts = torch.zeros(1, 8, 3, device=dev)
    for keep in ((0, 8), (8, 0), (9, 8), (8, 9), (-1, 4)):                              # counts out of range
        with pytest.raises(_lib.PznUnsupported):
            ops.icp_refine(pts, pts, eye, 3, keep=keep)
    with pytest.raises(_lib.PznUnsupported):
        ops.icp_refine(pts, torch.zeros(1, 1025, 3, device=dev), eye, 3, keep=(1, 1))   # kb = 1025
    with pytest.raises(_lib.PznUnsupported):
        ops.icp_refine(pts, pts, eye, -1, keep=(4, 4))                                  # iters = -1
    for keep in (4, (4,), (4, 4, 4), (4.0, 4), (0.5, 0.5), (True, 4)):                   # not two ints
        with pytest.raises(_lib.PznError) as info:
            ops.icp_refine(pts, pts, eye, 3, keep=keep)
        assert not isinstance(info.value, _lib.PznUnsupported)
    assert calls == []
    assert ops.icp_refine_trim_supported(8, 8, 1, 8) and ops.icp_refine_trim_supported(1024, 1024, 1024, 1)
    assert not ops.icp_refine_trim_supported(8, 8, 0, 8) and not ops.icp_refine_trim_supported(8, 8, 8, 9)
    assert not ops.icp_refine_trim_supported(1025, 8, 8, 8) and not ops.icp_refine_trim_supported(0, 8, 0, 8)
    # the library refuses them too, before any launch
    lib = _lib.load()
    assert lib.pzn_icp_refine_trim_f32(None, None, None, None, None, 1, 8, 8, 9, 8, 3, None, None, None, None, None, None, None,
                                       None, None) == _lib.CONSTANTS["PZN_EUNSUPPORTED"]
    # no problems: a success that launches nothing
    out = ops.icp_refine(pts[:0], pts[:0], eye[:0], 3, keep=(4, 4), return_kept=True)
    assert out[0].shape == (0, 4, 4) and out[4].shape == (0, 4) and out[5].shape == (0, 4) and calls == []
