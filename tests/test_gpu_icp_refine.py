"""GPU: ops.icp_refine (csrc/icprefine.hip) - every pair pose refined on its matched point sets in one launch - against the
float64 restatement tests/_icp_ref.py.

What is compared with what, and where the bounds come from (nothing below is tuned to the kernel):

(a) correspondences.  The kernel picks arg-mins of float32 squared distances d32; float64 distances d are the truth.  With
    B = _icp_ref.distance_bound (derived there: TRANSFORM_ROUNDINGS = 4 roundings on the longest path of
    x' = ((r00 x + r01 y) + r02 z) + t0 give |x32' - x'| <= gamma_4 M; the difference adds u |delta|; the squares and their
    two sums, SUM_ROUNDINGS = 3, add gamma_3 d), a returned index c of a row whose float64 arg-min is c* satisfies
    d(c) - B(c) <= d32(c) <= d32(c*) <= d(c*) + B(c*), hence d(c) - d(c*) <= B(c) + B(c*): the assertion.
(b) one step.  With iters = 1 the returned pose is the candidate built from the returned correspondences; it is compared
    with _icp_ref.step (float64) on those same correspondences.  Yardstick: _icp_ref.step_f32, the same step written plainly
    in float32 with sequential sums, on the same cases; the kernel gets STEP_FACTOR = 4 times the LARGEST yardstick error
    (it sums in another order, and its float64 sums and solve can only help).  A case enters where float64 says the candidate
    lowers E beyond the rounding interval of both scores (so the kernel had to take it).
    Measured on an MI355X over the 630 cases below (MEASURED_STEP): the yardstick's largest error is 3.8e-6 (an 8 x 8 case:
    a float32 SVD of a poorly conditioned cross-covariance; 1.7e-7 to 4.4e-7 at 64 points and more), the kernel's largest
    3.0e-8 - half a unit in the last place of a float32 entry near 0.5, i.e. the rounding of its output.
(c) scores: _icp_ref.objective_interval - (a)'s bound carried through the row minima, and a float32 sum of n non-negative
    terms in any order, the division and the final addition within a factor 1 -+ gamma_(n+2).
(d) trajectory (ka = kb in {8, 24}): the float64 loop against the device's, iters_used equal and the final pose within (b)'s
    tolerance; a case is left out when the float64 loop met a nearest-neighbour margin below MARGIN_FACTOR = 16 times the
    distance bound of (a) at its nearest-neighbour pairs UNDER T0 (a flipped neighbour is legitimate there; the bound is
    taken once, at the start pose, where the distances and so the bound are largest: a few more cases are left out than a
    bound followed through the iterations would leave out, never fewer), and at most a quarter
    of the cases may be left out (asserted; on the CPU the seeds below leave out 1 of 32 at k = 8 and 2 of 32 at k = 24).
"""
import numpy as np
import pytest
import torch

from tests import _icp_ref as ref

pytestmark = pytest.mark.gpu

STEP_FACTOR = 4.0            # (b): the kernel's step error may be this many times the float32 restatement's largest
MARGIN_FACTOR = 16.0         # (d): margins below this many distance bounds leave a case out
ORTHO_TOL = 2.0 ** -21       # R^T R - I per entry: three products of float32-rounded entries of an orthonormal matrix
ITERS = 30
# (ka, kb, P): degenerate; smallest regular; more problems than resident workgroups (the grid walk); wave edge; unequal sizes
# with fewer rows than threads; the production size; more rows than threads; the upper limit (few iterations)
SHAPES = [(1, 1, 1), (3, 3, 2), (8, 8, 600), (64, 65, 3), (37, 130, 5), (128, 128, 16), (257, 300, 2), (1024, 1024, 1)]
ITERS_OF = {(1024, 1024, 1): 3}
# step test on an MI355X, all 630 cases: largest yardstick error / largest kernel error
MEASURED_STEP = "yardstick 3.776e-06, kernel 2.980e-08"


def _ids(s):
    return f"{s[0]}x{s[1]}x{s[2]}"


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _cases(shape):
    ka, kb, P = shape
    rng = np.random.default_rng(31000 + 7 * ka + 3 * kb + P)
    return [ref.curve_case(rng, ka, kb, planar=bool(p & 1)) for p in range(P)]


def _stack(cases, dev):
    a = torch.from_numpy(np.stack([c.a for c in cases])).to(dev)
    b = torch.from_numpy(np.stack([c.b for c in cases])).to(dev)
    T0 = torch.from_numpy(np.stack([c.T0 for c in cases])).to(dev)
    return a, b, T0


@pytest.fixture(scope="module")
def runs(dev):
    """Every shape's cases, the one-step run with correspondences and the full run: made once, read by the tests below."""
    from puzzlenet_amd import ops
    out = {}
    for shape in SHAPES:
        cases = _cases(shape)
        a, b, T0 = _stack(cases, dev)
        iters = ITERS_OF.get(shape, ITERS)
        one = ops.icp_refine(a, b, T0, 1, return_corr=True)
        full = ops.icp_refine(a, b, T0, iters)
        out[shape] = dict(cases=cases, dev=(a, b, T0), iters=iters, one=[t.cpu().numpy() for t in one], full_dev=full,
                          full=[t.cpu().numpy() for t in full])
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_step_correspondences_are_float64_nearest_neighbours(runs, shape):
    r = runs[shape]
    ka, kb, P = shape
    T, score, score0, used, ca, cb = r["one"]
    assert ca.shape == (P, ka) and cb.shape == (P, kb) and ca.dtype == np.int32
    worst = 0.0
    for p, c in enumerate(r["cases"]):
        assert ca[p].min() >= 0 and ca[p].max() < kb and cb[p].min() >= 0 and cb[p].max() < ka
        D = ref.sqdist(c.a, ref.transform(c.T0, c.b))
        B = ref.distance_bound(c.a, c.b, c.T0)
        i, j = np.arange(ka), np.arange(kb)
        s1, s2 = D.argmin(axis=1), D.argmin(axis=0)
        over1 = (D[i, ca[p]] - D[i, s1]) - (B[i, ca[p]] + B[i, s1])
        over2 = (D[cb[p], j] - D[s2, j]) - (B[cb[p], j] + B[s2, j])
        worst = max(worst, float(over1.max()), float(over2.max()))
        assert (over1 <= 0).all() and (over2 <= 0).all(), (p, float(over1.max()), float(over2.max()))
    print(f"{_ids(shape)}: largest (excess - bound) {worst:.3e}; flips {sum(int((ca[p] != ref.objective(c.a, c.b, c.T0)[1]).sum()) for p, c in enumerate(r['cases']))}")


@pytest.fixture(scope="module")
def step_errors(runs):
    """(b) over every case of every shape -> {shape: [(yardstick error, kernel error, entered)]}."""
    out = {}
    for shape in SHAPES:
        r = runs[shape]
        T, score, score0, used, ca, cb = r["one"]
        rows = []
        for p, c in enumerate(r["cases"]):
            want = ref.step(c.a, c.b, ca[p], cb[p], c.T0)
            yard = ref.pose_err(ref.step_f32(c.a, c.b, ca[p], cb[p], c.T0), want)
            lo0, _ = ref.objective_interval(c.a, c.b, c.T0)
            _, hi1 = ref.objective_interval(c.a, c.b, want.astype(np.float32))
            entered = hi1 < lo0
            rows.append((yard, ref.pose_err(T[p], want), entered, int(used[p])))
        out[shape] = rows
    return out


def test_step_pose_within_four_times_the_float32_restatement(step_errors):
    yard = max(y for rows in step_errors.values() for y, _, _, _ in rows)
    entered = sum(e for rows in step_errors.values() for _, _, e, _ in rows)
    total = sum(len(rows) for rows in step_errors.values())
    for shape, rows in step_errors.items():
        ent = [r for r in rows if r[2]]
        print(f"{_ids(shape)}: yardstick max {max(r[0] for r in rows):.3e}, kernel max "
              f"{max([r[1] for r in ent], default=float('nan')):.3e}, entered {len(ent)} of {len(rows)}")
    print(f"all shapes: yardstick {yard:.3e}, kernel {max(k for rows in step_errors.values() for _, k, e, _ in rows if e):.3e}")
    assert entered >= 0.9 * total, (entered, total)      # the first step from 8 degrees / 0.03 off lowers E clearly
    for shape, rows in step_errors.items():
        for p, (_, k, e, used) in enumerate(rows):
            if e:
                assert used == 1, (shape, p)
                assert k <= STEP_FACTOR * yard, (shape, p, k, yard)


def test_degenerate_single_points_translate_only(runs):
    """ka = kb = 1: the rotation is T0's, bit for bit, and the translation puts the one point on its partner."""
    r = runs[(1, 1, 1)]
    T, score, score0, used = r["full"]
    c = r["cases"][0]
    assert np.array_equal(T[0, :3, :3], c.T0[:3, :3])
    assert used[0] >= 1 and score[0] < score0[0]
    assert np.abs(ref.transform(T[0], c.b) - c.a).max() <= 4 * ref.U32 * (np.abs(c.a).max() + np.abs(T[0, :3, 3]).max() + 1)


def test_degenerate_collinear_and_regular_side_by_side(dev):
    """Collinear moved points keep the rotation (translation only); the regular problem beside it in the same launch turns."""
    from puzzlenet_amd import ops
    rng = np.random.default_rng(77)
    reg = ref.curve_case(rng, 9, 7, False)
    line = (rng.uniform(-0.3, 0.3, (1, 3)) + np.linspace(-0.5, 0.5, 7)[:, None] * rng.normal(size=(1, 3))).astype(np.float32)
    a = torch.from_numpy(np.stack([reg.a, reg.a])).to(dev)
    b = torch.from_numpy(np.stack([reg.b, line])).to(dev)
    T0 = torch.from_numpy(np.stack([reg.T0, reg.T0])).to(dev)
    T, score, score0, used = (t.cpu().numpy() for t in ops.icp_refine(a, b, T0, 10))
    assert np.array_equal(T[1, :3, :3], reg.T0[:3, :3]) and not np.array_equal(T[1, :3, 3], reg.T0[:3, 3])
    assert used[1] >= 1 and score[1] < score0[1]
    assert not np.array_equal(T[0, :3, :3], reg.T0[:3, :3]) and used[0] >= 1
    want = ref.refine(reg.a, line, reg.T0, 1)
    one = ops.icp_refine(a[1:], b[1:], T0[1:], 1)[0].cpu().numpy()[0]
    np.testing.assert_allclose(one[:3, 3], want.T[:3, 3], rtol=0, atol=4 * ref.U32)


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_properties(runs, dev, shape):
    from puzzlenet_amd import ops
    r = runs[shape]
    ka, kb, P = shape
    a, b, T0 = r["dev"]
    iters = r["iters"]
    T, score, score0, used = r["full"]
    assert T.shape == (P, 4, 4) and score.shape == (P,) and used.dtype == np.int32
    assert (score <= score0).all()                                                    # exactly, every problem
    assert (used >= 0).all() and (used <= iters).all()
    assert (used[score < score0] >= 1).all() and (score[used == 0] == score0[used == 0]).all()
    last = np.array([0, 0, 0, 1], dtype=np.float32)
    assert (T[:, 3, :] == last).all()
    print(f"{_ids(shape)}: iters_used mean {used.mean():.2f} max {used.max()}, score/score0 mean {np.mean(score / score0):.3f}")
    for p, c in enumerate(r["cases"]):
        R = T[p, :3, :3].astype(np.float64)
        assert np.abs(R.T @ R - np.eye(3)).max() <= ORTHO_TOL and np.linalg.det(R) > 0
        lo, hi = ref.objective_interval(c.a, c.b, T[p])
        assert lo <= float(score[p]) <= hi, (p, lo, float(score[p]), hi)
        lo, hi = ref.objective_interval(c.a, c.b, c.T0)
        assert lo <= float(score0[p]) <= hi, (p, lo, float(score0[p]), hi)
    # two runs: the same bits in every output
    again = ops.icp_refine(a, b, T0, iters)
    assert all(torch.equal(x, y) for x, y in zip(r["full_dev"], again))
    # iters = 0 returns T0
    T_0, s_0, s0_0, u_0 = ops.icp_refine(a, b, T0, 0)
    assert torch.equal(T_0, T0) and torch.equal(s_0, s0_0) and torch.equal(s0_0, r["full_dev"][2]) and int(u_0.abs().max()) == 0
    # from the returned pose, a problem that stopped by itself does not move
    Td = r["full_dev"][0]
    T2, s2, s02, u2 = ops.icp_refine(a, b, Td, iters)
    stopped = torch.from_numpy(used < iters).to(dev)
    assert bool(stopped.any()) or shape == (1024, 1024, 1)
    assert int(u2[stopped].abs().max() if bool(stopped.any()) else 0) == 0
    assert torch.equal(T2[stopped], Td[stopped]) and torch.equal(s02[stopped], r["full_dev"][1][stopped])
    # row maps: the same bits as the run on the materialised sets
    a_of = torch.arange(P - 1, -1, -1, dtype=torch.long, device=dev)
    b_of = torch.roll(torch.arange(P, dtype=torch.long, device=dev), 1)
    mapped = ops.icp_refine(a, b, T0, iters, a_of=a_of, b_of=b_of, return_corr=True)
    plain = ops.icp_refine(a[a_of].contiguous(), b[b_of].contiguous(), T0, iters, return_corr=True)
    assert all(torch.equal(x, y) for x, y in zip(mapped, plain))
    # one moved set serving every problem
    zero = torch.zeros(P, dtype=torch.long, device=dev)
    shared = ops.icp_refine(a, b[:1], T0, iters, b_of=zero)
    plain = ops.icp_refine(a, b[:1].expand(P, -1, -1).contiguous(), T0, iters)
    assert all(torch.equal(x, y) for x, y in zip(shared, plain))


@pytest.mark.parametrize("k", [8, 24])
def test_trajectory_follows_the_float64_loop(runs, step_errors, dev, k):
    from puzzlenet_amd import ops
    n = 32
    rng = np.random.default_rng(4100 + k)
    cases = [ref.curve_case(rng, k, k, planar=bool(p & 1)) for p in range(n)]
    a, b, T0 = _stack(cases, dev)
    T, score, score0, used = (t.cpu().numpy() for t in ops.icp_refine(a, b, T0, ITERS))
    tol = STEP_FACTOR * max(y for rows in step_errors.values() for y, _, _, _ in rows)
    left_out, worst = 0, 0.0
    for p, c in enumerate(cases):
        want = ref.refine(c.a, c.b, c.T0, ITERS)
        if want.margin < MARGIN_FACTOR * ref.nearest_bound(c.a, c.b, c.T0):
            left_out += 1
            continue
        assert int(used[p]) == want.iters_used, (p, int(used[p]), want.iters_used)
        worst = max(worst, ref.pose_err(T[p], want.T))
        assert ref.pose_err(T[p], want.T) <= tol, (p, ref.pose_err(T[p], want.T), tol)
    print(f"k = {k}: left out {left_out} of {n}, largest pose difference {worst:.3e} (tolerance {tol:.3e})")
    assert left_out <= n // 4, left_out


def test_rejections_launch_nothing(dev, monkeypatch):
    from puzzlenet_amd import _lib, ops
    calls = []
    monkeypatch.setattr(ops, "_call", lambda *a, **k: calls.append(a[0]))
    eye = torch.eye(4, device=dev).reshape(1, 4, 4)
    pts = torch.zeros(1, 8, 3, device=dev)
    for bad in (lambda: ops.icp_refine(torch.zeros(1, 0, 3, device=dev), pts, eye, 3),              # ka = 0
                lambda: ops.icp_refine(pts, torch.zeros(1, 1025, 3, device=dev), eye, 3),           # kb = 1025
                lambda: ops.icp_refine(pts, pts, eye, -1)):                                         # iters = -1
        with pytest.raises(_lib.PznUnsupported):
            bad()
    for bad in (lambda: ops.icp_refine(torch.zeros(1, 8, 2, device=dev), pts, eye, 3),
                lambda: ops.icp_refine(pts, torch.zeros(8, 3, device=dev), eye, 3),
                lambda: ops.icp_refine(pts, pts, torch.zeros(1, 3, 4, device=dev), 3),
                lambda: ops.icp_refine(pts, pts, torch.eye(4, device=dev).reshape(1, 4, 4).expand(2, 4, 4), 3),   # two poses, one set
                lambda: ops.icp_refine(pts.double(), pts, eye, 3),
                lambda: ops.icp_refine(pts, pts, eye.double(), 3),
                lambda: ops.icp_refine(pts, pts, eye, 3, a_of=torch.zeros(1, dtype=torch.int32, device=dev)),
                lambda: ops.icp_refine(pts, pts, eye, 3, b_of=torch.zeros(2, dtype=torch.long, device=dev)),
                lambda: ops.icp_refine(pts.cpu(), pts, eye, 3)):
        with pytest.raises(_lib.PznError) as info:
            bad()
        assert not isinstance(info.value, _lib.PznUnsupported)
    assert calls == []
    assert ops.icp_refine_supported(1, 1) and ops.icp_refine_supported(1024, 1024)
    assert not ops.icp_refine_supported(0, 8) and not ops.icp_refine_supported(8, 1025)
    # no problems: a success that launches nothing
    T, score, score0, used = ops.icp_refine(pts[:0], pts[:0], eye[:0], 3)
    assert T.shape == (0, 4, 4) and score.shape == (0,) and calls == []
