"""GPU: ops.icp_refine(..., auto=(lo_a, lo_b, power)) (csrc/icprefine.hip, icp_auto_kernel) - the pose refinement that finds
the overlap share of every pair on the device - against the trimmed kernel where the least counts keep every row, against an
integer restatement on lattice clouds, and against the float64 statement tests/_icp_auto_ref.py elsewhere.

What is compared with what, and where the bounds come from (nothing below is tuned to the kernel):

(a) identity: lo = (ka, kb) leaves one candidate count, r = 1 and F = E: every shared output has the bits of
    keep = (ka, kb) (the contract), the counts are k, objective is score.
(b) lattice: coordinates are multiples of 1 / 8 in [0, 1), T0 translates by a lattice vector, iters = 0.  Squared distances
    are multiples of 1 / 64 and every sum stays below 2^24 units (asserted), so float32 forms them exactly in any order: the
    counts follow from phi compared by cross-multiplication in Python ints, the kept sets from (value, index) order, score
    and objective from the rule's few float32 roundings (_icp_auto_ref.lattice_expected).  Most counts are decided by an
    exact tie between two m or by a gap that one unit less in one minimum would close (asserted).
(c) float64 on partial-contact curve data, under T0: counts and kept sets equal the statement's wherever the count margin
    exceeds _icp_auto_ref.phi_slack and the keep margin _icp_trim_ref.kept_slack (both built from _icp_ref.distance_bound;
    tests/test_icp_auto_cpu.py asserts that this leaves out at most a quarter - here it is none); score lies in
    _icp_trim_ref.objective_interval at the RETURNED counts and pose, under T0 and after the loop.
(d) trajectory: the float64 loop against the device's - iters_used, counts and kept sets equal, the pose within STEP_FACTOR
    times the largest error of the float32 restatement of one step (_icp_trim_ref.step_f32 against step at the start pose of
    every case: test_gpu_icp_trim.py's tolerance form).  Left out: _icp_auto_ref.trajectory_left_out (a margin under 16
    distance bounds, or a count float32 may decide otherwise); at most a quarter, asserted on the CPU.
(e) properties: objective <= the objective of T0 (score <= score0 does NOT hold in general: F is what falls), counts in
    [lo, k], kept rows ascending and -1 exactly past the count, two runs equal bits, the returned sets are those of a fresh
    evaluation of the returned pose, row maps, and rejections that launch nothing.
"""
import numpy as np
import pytest
import torch

from tests import _icp_auto_ref as auto
from tests import _icp_ref as ref
from tests import _icp_trim_ref as trim

pytestmark = pytest.mark.gpu

STEP_FACTOR = 4.0
ITERS = 30
POWER = auto.POWER
# (ka, kb, P): a single row a side; odd sizes, ka != kb; one wavefront's worth a side; several rows per thread on one side;
# the LDS limit; more problems than the 512-workgroup grid
SHAPES = [(1, 1, 3), (37, 29, 8), (64, 64, 8), (300, 70, 4), (1024, 1024, 2), (8, 8, 513)]
NAMES = ("T", "score", "score0", "iters_used", "corr_a", "corr_b", "count_a", "count_b", "objective", "kept_a", "kept_b")


def _id(s):
    return "x".join(str(v) for v in s)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _cases(shape):
    if shape in auto.FLOAT64_SHAPES:
        return auto.float64_cases(shape)
    ka, kb, P = shape
    rng = np.random.default_rng(62000 + 7 * ka + 3 * kb + P)
    return [ref.curve_case(rng, ka, kb, planar=bool(p & 1)) for p in range(P)]


def _stack(cases, dev):
    return tuple(torch.from_numpy(np.stack([getattr(c, f) for c in cases])).to(dev) for f in ("a", "b", "T0"))


@pytest.fixture(scope="module")
def data(dev):
    """Every shape's cases on the host and on the device: made once."""
    return {shape: (cases, _stack(cases, dev)) for shape in SHAPES for cases in (_cases(shape),)}


def _lo(shape):
    return auto.least_count(shape[0]), auto.least_count(shape[1])


@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_every_row_kept_is_the_trimmed_kernel(data, shape):
    from puzzlenet_amd import ops
    ka, kb, P = shape
    _, (a, b, T0) = data[shape]
    for it in (0, ITERS):
        want = ops.icp_refine(a, b, T0, it, return_corr=True, keep=(ka, kb), return_kept=True)
        for power in (1, 3):
            got = ops.icp_refine(a, b, T0, it, return_corr=True, auto=(ka, kb, power), return_kept=True)
            assert len(got) == 11
            for name, x, y in zip(NAMES[:6] + NAMES[9:], want, got[:6] + got[9:]):
                assert torch.equal(x, y), (it, power, name)
            assert torch.equal(got[6], torch.full((P,), ka, dtype=torch.int32, device=a.device))
            assert torch.equal(got[7], torch.full((P,), kb, dtype=torch.int32, device=a.device))
            assert torch.equal(got[8], got[1]), (it, power)      # r = 1: F is E


@pytest.mark.parametrize("shape", auto.LATTICE_SHAPES, ids=_id)
def test_lattice_counts_sets_and_sums_equal_the_integer_restatement(dev, shape):
    from puzzlenet_amd import ops
    ka, kb, P = shape
    A, B, T0, ia, ib, it = auto.lattice_case(shape)
    lo_a, lo_b = _lo(shape)
    how, nonzero = [], 0
    for power in (POWER, 1):
        T, score, score0, used, count_a, count_b, objective, kept_a, kept_b = (t.cpu().numpy() for t in ops.icp_refine(
            *(torch.from_numpy(x).to(dev) for x in (A, B, T0)), 0, auto=(lo_a, lo_b, power), return_kept=True))
        assert np.array_equal(T, T0) and (used == 0).all() and np.array_equal(score, score0)
        for p in range(P):
            e = auto.lattice_expected(ia[p], ib[p], it[p], lo_a, lo_b, power)
            assert (int(count_a[p]), int(count_b[p])) == (e["count_a"], e["count_b"]), (p, power, e["how_a"], e["how_b"])
            for got, want, k in ((kept_a[p], e["kept_a"], ka), (kept_b[p], e["kept_b"], kb)):
                assert np.array_equal(got, np.concatenate((want, np.full(k - len(want), -1)))), (p, power)
            assert score[p] == e["score"] and objective[p] == e["objective"], (p, power, score[p], e["score"], objective[p], e["objective"])
            if power == POWER:
                how += [e["how_a"], e["how_b"]]
                nonzero += e["score"] > 0
    close = sum(h in ("tie", "unit") for h in how)
    print(f"{_id(shape)}: {close} of {len(how)} counts decided by a tie or one unit, {nonzero} of {P} scores above 0")
    assert ka == 1 or 2 * close > len(how), how


@pytest.mark.parametrize("shape", auto.FLOAT64_SHAPES, ids=_id)
def test_counts_sets_and_scores_against_float64(data, shape):
    from puzzlenet_amd import ops
    ka, kb, P = shape
    cases, (a, b, T0) = data[shape]
    lo_a, lo_b = _lo(shape)
    zero = [t.cpu().numpy() for t in ops.icp_refine(a, b, T0, 0, auto=(lo_a, lo_b, POWER), return_kept=True)]
    full = [t.cpu().numpy() for t in ops.icp_refine(a, b, T0, ITERS, auto=(lo_a, lo_b, POWER), return_kept=True)]
    assert np.array_equal(zero[0], T0.cpu().numpy()) and (zero[3] == 0).all() and np.array_equal(zero[1], zero[2])
    assert np.array_equal(zero[2], full[2])
    compared = 0
    for p, c in enumerate(cases):
        if auto.count_decided(c, c.T0, lo_a, lo_b, POWER):
            compared += 1
            o = auto.objective(c.a, c.b, c.T0, lo_a, lo_b, POWER)
            assert (int(zero[4][p]), int(zero[5][p])) == (o.m_a, o.m_b), (p, zero[4][p], zero[5][p], o.m_a, o.m_b)
            assert np.array_equal(zero[7][p][:o.m_a], o.kept_a) and np.array_equal(zero[8][p][:o.m_b], o.kept_b), p
        for run, T in ((zero, c.T0), (full, full[0][p])):
            lo, hi = trim.objective_interval(c.a, c.b, T, int(run[4][p]), int(run[5][p]))
            assert lo <= float(run[1][p]) <= hi, (p, lo, float(run[1][p]), hi)
    print(f"{_id(shape)}: counts and kept sets compared in {compared} of {P} problems")
    assert 4 * compared >= 3 * P


@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_properties(data, dev, shape):
    from puzzlenet_amd import ops
    ka, kb, P = shape
    _, (a, b, T0) = data[shape]
    lo_a, lo_b = _lo(shape)
    kw = dict(auto=(lo_a, lo_b, POWER), return_corr=True, return_kept=True)
    run = ops.icp_refine(a, b, T0, ITERS, **kw)
    T, score, score0, used, ca, cb, count_a, count_b, objective, kept_a, kept_b = run
    assert T.shape == (P, 4, 4) and kept_a.shape == (P, ka) and kept_b.shape == (P, kb)
    assert all(t.dtype == torch.int32 for t in (used, count_a, count_b, kept_a, kept_b)) and objective.dtype == torch.float32
    start = ops.icp_refine(a, b, T0, 0, **kw)
    assert torch.equal(start[2], score0) and torch.equal(start[1], score0)
    assert bool((objective <= start[8]).all())                                         # F falls, exactly, every problem
    assert bool((used[objective < start[8]] >= 1).all()) and bool((objective[used == 0] == start[8][used == 0]).all())
    assert int(used.min()) >= 0 and int(used.max()) <= ITERS
    assert int(ca.min()) >= 0 and int(ca.max()) < kb and int(cb.min()) >= 0 and int(cb.max()) < ka
    for kept, count, lo, k in ((kept_a, count_a, lo_a, ka), (kept_b, count_b, lo_b, kb)):
        assert int(count.min()) >= lo and int(count.max()) <= k
        live = torch.arange(k, device=dev)[None, :] < count[:, None]
        assert bool((kept[~live] == -1).all()) and bool((kept[live] >= 0).all()) and int(kept.max()) < k      # -1 exactly past the count
        rising = (kept[:, 1:] > kept[:, :-1]) | ~live[:, 1:]
        assert bool(rising.all())
    # two runs: the same bits in every output
    again = ops.icp_refine(a, b, T0, ITERS, **kw)
    assert all(torch.equal(x, y) for x, y in zip(run, again))
    # the returned pose's counts, sets and sums are those of an evaluation of it, whether or not the last candidate was rejected
    at = ops.icp_refine(a, b, T, 0, **kw)
    for i in (0, 1, 6, 7, 8, 9, 10):
        assert torch.equal(at[i], run[i]), NAMES[i]
    # row maps: the same bits as the run on the materialised sets
    a_of = torch.arange(P - 1, -1, -1, dtype=torch.long, device=dev)
    b_of = torch.roll(torch.arange(P, dtype=torch.long, device=dev), 1)
    mapped = ops.icp_refine(a, b, T0, ITERS, a_of=a_of, b_of=b_of, **kw)
    plain = ops.icp_refine(a[a_of].contiguous(), b[b_of].contiguous(), T0, ITERS, **kw)
    assert all(torch.equal(x, y) for x, y in zip(mapped, plain))
    # without return_kept and return_corr the same launch writes neither
    short = ops.icp_refine(a, b, T0, ITERS, auto=(lo_a, lo_b, POWER))
    assert len(short) == 7 and all(torch.equal(x, y) for x, y in zip(short, run[:4] + run[6:9]))


@pytest.fixture(scope="module")
def trajectories():
    """The cases of (d), the float64 loop of each, and the largest error of the float32 restatement of one step at the
    start poses."""
    cases = auto.trajectory_cases()
    lo = auto.least_count(auto.TRAJECTORY_K)
    worst = 0.0
    for c in cases:
        o = auto.objective(c.a, c.b, c.T0, lo, lo, POWER)
        want = trim.step(c.a, c.b, o.c1, o.c2, o.kept_a, o.kept_b, c.T0)
        worst = max(worst, ref.pose_err(trim.step_f32(c.a, c.b, o.c1, o.c2, o.kept_a, o.kept_b, c.T0), want))
    return cases, [auto.refine(c.a, c.b, c.T0, ITERS, lo, lo, POWER) for c in cases], worst, lo


def test_trajectory_follows_the_float64_loop(dev, trajectories):
    from puzzlenet_amd import ops
    cases, wants, yardstick, lo = trajectories
    T, score, score0, used, count_a, count_b, objective, kept_a, kept_b = (t.cpu().numpy() for t in ops.icp_refine(
        *_stack(cases, dev), ITERS, auto=(lo, lo, POWER), return_kept=True))
    tol = STEP_FACTOR * yardstick
    left_out, worst = 0, 0.0
    for p, (c, want) in enumerate(zip(cases, wants)):
        if auto.trajectory_left_out(c, want):
            left_out += 1
            continue
        assert int(used[p]) == want.iters_used, (p, int(used[p]), want.iters_used)
        assert (int(count_a[p]), int(count_b[p])) == (want.m_a, want.m_b), p
        assert np.array_equal(kept_a[p][:want.m_a], want.kept_a) and np.array_equal(kept_b[p][:want.m_b], want.kept_b), p
        worst = max(worst, ref.pose_err(T[p], want.T))
        assert ref.pose_err(T[p], want.T) <= tol, (p, ref.pose_err(T[p], want.T), tol)
    print(f"left out {left_out} of {len(cases)}, largest pose difference {worst:.3e} (tolerance {tol:.3e})")
    assert 4 * left_out <= len(cases), left_out


def test_rejections_launch_nothing(dev, monkeypatch):
    from puzzlenet_amd import _lib, ops
    calls = []
    monkeypatch.setattr(ops, "_call", lambda *a, **k: calls.append(a[0]))
    eye = torch.eye(4, device=dev).reshape(1, 4, 4)
    pts = torch.zeros(1, 8, 3, device=dev)
    for bad in ((0, 8, 3), (8, 0, 3), (9, 8, 3), (8, 9, 3), (-1, 4, 3), (4, 4, 0), (4, 4, 5), (4, 4, -1)):      # out of range
        with pytest.raises(_lib.PznUnsupported):
            ops.icp_refine(pts, pts, eye, 3, auto=bad)
    with pytest.raises(_lib.PznUnsupported):
        ops.icp_refine(pts, torch.zeros(1, 1025, 3, device=dev), eye, 3, auto=(1, 1, 3))       # kb = 1025
    with pytest.raises(_lib.PznUnsupported):
        ops.icp_refine(pts, pts, eye, -1, auto=(4, 4, 3))                                      # iters = -1
    for bad in (4, (4, 4), (4, 4, 3, 1), (4.0, 4, 3), (4, 4, 3.0), (0.25, 0.25, 3), (True, 4, 3), "auto"):      # not three ints
        with pytest.raises(_lib.PznError) as info:
            ops.icp_refine(pts, pts, eye, 3, auto=bad)
        assert not isinstance(info.value, _lib.PznUnsupported)
    with pytest.raises(_lib.PznError) as info:                                                 # counts given AND counts found
        ops.icp_refine(pts, pts, eye, 3, keep=(4, 4), auto=(4, 4, 3))
    assert not isinstance(info.value, _lib.PznUnsupported)
    assert calls == []
    assert ops.icp_refine_auto_supported(8, 8, 1, 8, 1) and ops.icp_refine_auto_supported(1024, 1024, 1024, 1, 4)
    assert not ops.icp_refine_auto_supported(8, 8, 0, 8, 3) and not ops.icp_refine_auto_supported(8, 8, 8, 9, 3)
    assert not ops.icp_refine_auto_supported(8, 8, 4, 4, 0) and not ops.icp_refine_auto_supported(8, 8, 4, 4, 5)
    assert not ops.icp_refine_auto_supported(1025, 8, 8, 8, 3) and not ops.icp_refine_auto_supported(0, 8, 0, 8, 3)
    # the library refuses them too, before any launch
    lib = _lib.load()
    assert lib.pzn_icp_refine_auto_f32(None, None, None, None, None, 1, 8, 8, 9, 8, 3, 3, None, None, None, None, None, None, None,
                                       None, None, None, None, None) == _lib.CONSTANTS["PZN_EUNSUPPORTED"]
    assert lib.pzn_icp_refine_auto_f32(None, None, None, None, None, 1, 8, 8, 4, 4, 5, 3, None, None, None, None, None, None, None,
                                       None, None, None, None, None) == _lib.CONSTANTS["PZN_EUNSUPPORTED"]
    # no problems: a success that launches nothing
    out = ops.icp_refine(pts[:0], pts[:0], eye[:0], 3, auto=(4, 4, 3), return_kept=True)
    assert len(out) == 9 and out[0].shape == (0, 4, 4) and out[4].shape == (0,) and out[7].shape == (0, 8) and out[8].shape == (0, 8)
    assert calls == []
