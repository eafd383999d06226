"""GPU: ops.joint_refine (csrc/jointrefine.hip) - all piece poses of a placed assembly refined jointly over every joint in
one launch - against the float64 restatement tests/_joint_ref.py.

What is compared with what, and where the bounds come from (nothing below is tuned to the kernel):

(a) one visit.  Only piece 1 may move; it has at least two joints, one in each role (so the pair graph is not here);
    sweeps = 1.  The returned pose is compared with _joint_ref.visit on the float64 correspondences.  Yardstick:
    _joint_ref.visit_f32, the same visit written plainly in float32 with sequential sums; the kernel gets STEP_FACTOR = 4
    times the LARGEST yardstick error over all cases (tests/test_gpu_icp_refine.py's rule and reason: it sums in another
    order, and its float64 sums and solve can only help).  The kernel does not return its correspondences, so a case enters
    where it cannot have chosen others - every nearest-neighbour margin of piece 1's joints under G0 exceeds MARGIN_FACTOR =
    16 times _joint_ref.distance_bound2 at the nearest pairs - and where float64 says the candidate lowers E_p beyond the
    rounding intervals of both sums (so the kernel had to take it).  Three quarters of the cases must enter.
    Measured on an MI355X over the 260 cases below (MEASURED_STEP): the yardstick's largest error is 4.0e-6 (a 257 x 300 case
    with eight joints: sequential float32 sums over 4456 pairs), the kernel's largest 8.9e-8 (a 3 x 3 case): the rounding
    of its output plus that of the fp32 images it takes as y.  The 59 cases that do not enter are nearly all those of 64
    and more points a side, where some row of some joint has two neighbours closer than 16 bounds.
(b) properties, every shape and graph: the scores inside _joint_ref.objective_interval2 (the interval of every joint, and a
    float32 sum of J non-negative terms within a factor 1 -+ gamma_J), score = the float32 sum of joint_score in list order
    to the bit, orthonormal rotations, repeatable bits, and the invariances listed in test_properties.  Where a launch holds
    hundreds of puzzles, or a joint has more than 256 points a side, the float64 side looks at a spread of puzzles / joints
    (CHECKED / the joints of _some_joints); everything that compares device bits with device bits looks at all of them.
(c) short trajectory (k = 8, 2 sweeps, same = True): `accepted` equal to the float64 loop's and the poses within (a)'s
    tolerance; a case is left out when the float64 loop met a nearest-neighbour margin below MARGIN_FACTOR bounds (taken under
    G0, per joint); at most a quarter may be left out.  The counts of TRAJECTORY are asserted on the CPU
    (tests/test_joint_ref_cpu.py) on the same seeds.
(d) rejections launch nothing.
"""
import numpy as np
import pytest
import torch

from tests import _icp_ref as ref
from tests import _joint_ref as jr

pytestmark = pytest.mark.gpu

STEP_FACTOR = 4.0            # (a): the kernel's visit error may be this many times the float32 restatement's largest
MARGIN_FACTOR = 16.0         # (a), (c): margins below this many distance bounds leave a case out
ORTHO_TOL = 2.0 ** -21       # R^T R - I per entry: three products of float32-rounded entries of an orthonormal matrix
SWEEPS = 30
# ((ka, kb), Z): degenerate; smallest regular; more puzzles than resident workgroups (the grid walk); wave edge with unequal
# sides; the production size; more rows than threads, unequal; the upper limit (two sweeps)
SHAPES = [((1, 1), 1), ((3, 3), 2), ((8, 8), 600), ((64, 65), 3), ((128, 128), 16), ((257, 300), 2), ((1024, 1024), 1)]
SWEEPS_OF = {((1024, 1024), 1): 2}
GRAPHS = ["pair", "chain3", "ring4", "both3", "complete5"]
VISIT_GRAPHS = ["chain3", "ring4", "both3", "complete5"]      # piece 1 has a joint in each role
# (c): graph -> cases the float64 loop leaves out of 16 (asserted in tests/test_joint_ref_cpu.py)
TRAJECTORY = {"pair": 0, "chain3": 2, "ring4": 0, "both3": 1}
# one-visit test on an MI355X, all cases: largest yardstick error / largest kernel error
MEASURED_STEP = "yardstick 4.045e-06, kernel 8.908e-08 (201 of 260 cases entered)"


def _ids(s):
    return f"{s[0][0]}x{s[0][1]}x{s[1]}"


def _seed(graph, shape):
    return 52000 + 1000 * GRAPHS.index(graph) + 7 * shape[0][0] + 3 * shape[0][1] + shape[1]


def _cases(graph, shape, movable=None):
    K, joints = jr.GRAPHS[graph]
    rng = np.random.default_rng(_seed(graph, shape))
    return [jr.puzzle(rng, K, joints, shape[0], movable=movable) for _ in range(shape[1])]


def trajectory_cases(graph):
    K, joints = jr.GRAPHS[graph]
    rng = np.random.default_rng(6100 + GRAPHS.index(graph))
    return [jr.puzzle(rng, K, joints, 8, same=True) for _ in range(16)]


def checked(Z):
    """The puzzles of a launch that the float64 side looks at."""
    return [z for z in range(Z) if z < 6 or z >= Z - 2 or z % 97 == 0]


def _some_joints(P):
    J = len(P.joints)
    big = max(P.A[0].shape[0], P.B[0].shape[0]) > 256
    return list(range(J)) if not big or J <= 5 else [0, J // 3, (2 * J) // 3, J - 1]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _stack(cases, dev):
    """-> a [Z J,ka,3], b [Z J,kb,3], joints [Z,J,2] int32 (host), G0 [Z,K,4,4], movable [Z,K] uint8."""
    a = torch.from_numpy(np.stack([s for P in cases for s in P.A])).to(dev)
    b = torch.from_numpy(np.stack([s for P in cases for s in P.B])).to(dev)
    joints = torch.from_numpy(np.array([P.joints for P in cases], dtype=np.int32))
    G0 = torch.from_numpy(np.stack([P.G0 for P in cases])).to(dev)
    movable = torch.from_numpy(np.stack([P.movable for P in cases]).astype(np.uint8)).to(dev)
    return a, b, joints, G0, movable


def _host(out):
    return [t.cpu().numpy() for t in out]


@pytest.fixture(scope="module")
def runs(dev):
    """Every graph's and shape's cases and the full run: made once, read by the tests below."""
    from puzzlenet_amd import ops
    out = {}
    for graph in GRAPHS:
        for shape in SHAPES:
            cases = _cases(graph, shape)
            args = _stack(cases, dev)
            sweeps = SWEEPS_OF.get(shape, SWEEPS)
            full = ops.joint_refine(*args, sweeps)
            out[graph, shape] = dict(cases=cases, dev=args, sweeps=sweeps, full_dev=full, full=_host(full))
    return out


@pytest.fixture(scope="module")
def visit_errors(dev):
    """(a) over the looked-at cases of every shape and graph -> {(graph, shape): [(yardstick error, kernel error, entered,
    accepted by the device)]}; asserts that every other piece's pose is G0 bit for bit."""
    from puzzlenet_amd import ops
    out = {}
    for graph in VISIT_GRAPHS:
        K, _ = jr.GRAPHS[graph]
        only = np.arange(K) == 1
        for shape in SHAPES:
            cases = _cases(graph, shape, movable=only)
            args = _stack(cases, dev)
            G, score, score0, js, used, acc = _host(ops.joint_refine(*args, 1))
            G0 = args[3].cpu().numpy()
            assert np.array_equal(np.delete(G, 1, axis=1), np.delete(G0, 1, axis=1))
            assert (np.delete(acc, 1, axis=1) == 0).all() and (score <= score0).all()
            rows = []
            for z in (checked(shape[1]) if shape[1] <= 100 else range(48)):
                P = cases[z]
                g0 = jr.f32(P.G0)
                Ep, corr, margins = jr.piece_energy(P, g0, 1)
                want = jr.visit(P, g0, 1, corr, round32=False)
                yard = ref.pose_err(jr.visit_f32(P, P.G0, 1, corr), want)
                safe = all(margins[e] > MARGIN_FACTOR * jr.nearest_bound2(P.A[e], P.B[e], g0[P.joints[e][0]], g0[P.joints[e][1]])
                           for e in margins)
                entered = False
                if safe:
                    gn = g0.copy()
                    gn[1] = jr.f32(want)
                    inc = jr.incident(P, 1)
                    iv0 = np.array([jr.objective_interval2(P.A[e], P.B[e], g0[P.joints[e][0]], g0[P.joints[e][1]]) for e in inc])
                    iv1 = np.array([jr.objective_interval2(P.A[e], P.B[e], gn[P.joints[e][0]], gn[P.joints[e][1]]) for e in inc])
                    entered = jr.sum_interval(iv1)[1] < jr.sum_interval(iv0)[0]
                rows.append((yard, ref.pose_err(G[z, 1], want), bool(entered), int(acc[z, 1]), int(used[z])))
            out[graph, shape] = rows
    return out


def test_one_visit_pose_within_four_times_the_float32_restatement(visit_errors):
    rows_all = [r for rows in visit_errors.values() for r in rows]
    yard = max(r[0] for r in rows_all)
    entered = sum(r[2] for r in rows_all)
    for (graph, shape), rows in visit_errors.items():
        ent = [r for r in rows if r[2]]
        print(f"{graph} {_ids(shape)}: yardstick max {max(r[0] for r in rows):.3e}, kernel max "
              f"{max([r[1] for r in ent], default=float('nan')):.3e}, entered {len(ent)} of {len(rows)}")
    print(f"all: yardstick {yard:.3e}, kernel {max(r[1] for r in rows_all if r[2]):.3e}, entered {entered} of {len(rows_all)}")
    assert 4 * entered >= 3 * len(rows_all), (entered, len(rows_all))
    for key, rows in visit_errors.items():
        for n, (_, k, e, acc, used) in enumerate(rows):
            if e:
                assert acc == 1 and used == 1, (key, n)
                assert k <= STEP_FACTOR * yard, (key, n, k, yard)


def _seq32(x):
    s = np.float32(0)
    for v in np.asarray(x, dtype=np.float32):
        s = np.float32(s + v)
    return s


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
@pytest.mark.parametrize("graph", GRAPHS)
def test_properties(runs, dev, graph, shape):
    from puzzlenet_amd import ops
    r = runs[graph, shape]
    (ka, kb), Z = shape
    K, joints = jr.GRAPHS[graph]
    J = len(joints)
    cases, sweeps = r["cases"], r["sweeps"]
    a, b, jl, G0, movable = r["dev"]
    G, score, score0, js, used, acc = r["full"]
    assert G.shape == (Z, K, 4, 4) and score.shape == (Z,) and js.shape == (Z, J) and acc.shape == (Z, K)
    assert used.dtype == np.int32 and acc.dtype == np.int32
    assert (score <= score0).all()                                                    # exactly, every puzzle
    assert (used >= 0).all() and (used <= sweeps).all() and (acc >= 0).all() and (acc.max(axis=1) <= used).all()
    assert ((acc.sum(axis=1) > 0) == (used > 0)).all() and (score[used == 0] == score0[used == 0]).all()
    g0 = G0.cpu().numpy()
    assert (acc[:, 0] == 0).all() and np.array_equal(G[:, 0], g0[:, 0])               # piece 0 is not movable
    assert (G[:, :, 3, :] == np.array([0, 0, 0, 1], dtype=np.float32)).all()
    assert np.array_equal(G[acc == 0], g0[acc == 0])
    print(f"{graph} {_ids(shape)}: sweeps_used mean {used.mean():.2f} max {used.max()}, score/score0 mean {np.mean(score / score0):.3f}")
    for z in range(Z):
        assert _seq32(js[z]) == score[z], (z, _seq32(js[z]), score[z])
        R = G[z, :, :3, :3].astype(np.float64)
        assert np.abs(np.swapaxes(R, 1, 2) @ R - np.eye(3)).max() <= ORTHO_TOL and (np.linalg.det(R) > 0).all()
    # sweeps = 0 returns G0, and its scores are those of the start pose
    G_0, s_0, s0_0, js_0, u_0, a_0 = ops.joint_refine(a, b, jl, G0, movable, 0)
    assert torch.equal(G_0, G0) and torch.equal(s_0, s0_0) and torch.equal(s0_0, r["full_dev"][2])
    assert int(u_0.abs().max()) == 0 and int(a_0.abs().max()) == 0
    js_0 = js_0.cpu().numpy()
    for z in checked(Z):
        P = cases[z]
        some = _some_joints(P)
        for g, jsc, tot in ((jr.f32(P.G0), js_0[z], score0[z]), (jr.f32(G[z]), js[z], score[z])):
            iv = np.array([jr.objective_interval2(P.A[e], P.B[e], g[P.joints[e][0]], g[P.joints[e][1]]) if e in some
                           else (np.nan, np.nan) for e in range(J)])
            for e in some:
                assert iv[e, 0] <= float(jsc[e]) <= iv[e, 1], (z, e, iv[e], float(jsc[e]))
            assert _seq32(jsc) == tot
            if len(some) == J:
                lo, hi = jr.sum_interval(iv)
                assert lo <= float(tot) <= hi, (z, lo, float(tot), hi)
                assert iv[:, 0].sum() <= float(jsc.astype(np.float64).sum()) <= iv[:, 1].sum()
    # two runs: the same bits in every output
    again = ops.joint_refine(a, b, jl, G0, movable, sweeps)
    assert all(torch.equal(x, y) for x, y in zip(r["full_dev"], again))
    # from the returned poses, a puzzle that stopped by itself does not move
    Gd = r["full_dev"][0]
    G2, s2, s02, js2, u2, a2 = ops.joint_refine(a, b, jl, Gd, movable, sweeps)
    stopped = torch.from_numpy(used < sweeps).to(dev)
    if bool(stopped.any()):
        assert int(u2[stopped].abs().max()) == 0 and int(a2[stopped].abs().max()) == 0
        assert torch.equal(G2[stopped], Gd[stopped]) and torch.equal(s02[stopped], r["full_dev"][1][stopped])
        assert torch.equal(s2[stopped], s02[stopped]) and torch.equal(js2[stopped], r["full_dev"][3][stopped])
    # Z puzzles in one launch = each puzzle alone
    for z in sorted(set([0, Z // 2, Z - 1])):
        alone = ops.joint_refine(a[z * J:(z + 1) * J], b[z * J:(z + 1) * J], jl[z:z + 1], G0[z:z + 1], movable[z:z + 1], sweeps)
        assert all(torch.equal(x[z:z + 1], y) for x, y in zip(r["full_dev"], alone)), z
    # set maps: the same bits as the run on the materialised sets (and a joint list that is on the device already)
    perm = torch.from_numpy(np.random.default_rng(1).permutation(Z * J)).to(dev)
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(Z * J, device=dev)
    mapped = ops.joint_refine(a[perm].contiguous(), b.flip(0).contiguous(), jl.to(dev), G0, movable, sweeps,
                              a_of=inv.reshape(Z, J), b_of=torch.arange(Z * J - 1, -1, -1, device=dev).reshape(Z, J))
    assert all(torch.equal(x, y) for x, y in zip(r["full_dev"], mapped))
    # an unused row (i = -1, its sets never read as points: NaN) = the list without it
    e = J // 2
    keep = [x for x in range(J) if x != e]
    hole = jl.clone()
    hole[:, e] = -1
    rows = torch.arange(Z * J, device=dev).reshape(Z, J)
    a_nan, b_nan = a.clone(), b.clone()
    a_nan[rows[:, e]] = float("nan")
    b_nan[rows[:, e]] = float("nan")
    with_hole = ops.joint_refine(a_nan, b_nan, hole, G0, movable, sweeps)
    without = ops.joint_refine(a, b, jl[:, keep].contiguous(), G0, movable, sweeps, a_of=rows[:, keep].contiguous(),
                               b_of=rows[:, keep].contiguous())
    for n, (x, y) in enumerate(zip(with_hole, without)):
        if n == 3:
            assert torch.equal(x[:, keep], y) and int((x[:, e] != 0).sum()) == 0
        else:
            assert torch.equal(x, y), n
    # a boolean mask is the same mask
    assert all(torch.equal(x, y) for x, y in zip(r["full_dev"], ops.joint_refine(a, b, jl, G0, movable.bool(), sweeps)))


def test_pieces_without_a_joint_and_fixed_pieces_keep_their_bits(dev):
    """Ring of 4 plus a fifth piece no joint touches; piece 2 is not movable either."""
    from puzzlenet_amd import ops
    rng = np.random.default_rng(88)
    _, joints = jr.GRAPHS["ring4"]
    cases = [jr.puzzle(rng, 5, joints, (9, 11), movable=[False, True, False, True, True]) for _ in range(3)]
    args = _stack(cases, dev)
    G, score, score0, js, used, acc = _host(ops.joint_refine(*args, 10))
    g0 = args[3].cpu().numpy()
    for p in (0, 2, 4):
        assert (acc[:, p] == 0).all() and np.array_equal(G[:, p], g0[:, p])
    assert (acc[:, 1] > 0).all() and (acc[:, 3] > 0).all() and (score < score0).all()


def degenerate_pair(rng, collinear, k=8, noise=0.003, angle=np.deg2rad(4.0), shift=0.01):
    """Two pieces, the joint (0, 1), piece 1 movable: set B is k fp32 points in piece 1's frame - on one line (collinear) or on
    _icp_ref.curve -, set A their image under a known pose plus `noise`, piece 0 at the identity; G0[1] is that pose turned by
    `angle` about a random axis through the image's centre and shifted by `shift` in a random direction."""
    truth = ref.rigid(ref.rot(rng.normal(size=3), rng.uniform(0.3, 2.5)), rng.uniform(-0.3, 0.3, 3))
    if collinear:
        b = (rng.uniform(-0.3, 0.3, (1, 3)) + np.linspace(-0.5, 0.5, k)[:, None] * rng.normal(size=(1, 3))).astype(np.float32)
    else:
        b = ref.curve(rng.uniform(0, 1, k), False).astype(np.float32)
    image = ref.transform(truth, b)
    a = (image + rng.normal(scale=noise, size=(k, 3))).astype(np.float32)
    c, d = image.mean(axis=0), rng.normal(size=3)
    Rp = ref.rot(rng.normal(size=3), angle)
    G1 = ref.rigid(Rp, c - Rp @ c + shift * d / np.linalg.norm(d)) @ truth
    G0 = np.stack([np.eye(4), G1]).astype(np.float32)
    return jr.Puzzle(2, [(0, 1)], [a], [b], G0, np.stack([np.eye(4), truth]), np.array([False, True]))


DEGENERATE_SEED = 4242


def degenerate_cases(k):
    """[the collinear puzzle, the regular one beside it]; k = 1 keeps the first point of every set of the k = 8 layout."""
    rng = np.random.default_rng(DEGENERATE_SEED)
    cases = [degenerate_pair(rng, True), degenerate_pair(rng, False)]
    return [P._replace(A=[P.A[0][:k]], B=[P.B[0][:k]]) for P in cases]


@pytest.mark.parametrize("k", [8, 1])
def test_degenerate_scatter_keeps_the_rotation(dev, k):
    """The degenerate rule (solve_pose in csrc/pzn_rigid.h) in the joint kernel: a moved piece whose points x lie on one line
    (or are one point) keeps its rotation bit for bit and moves by translation only, and that lowers the score; the regular
    puzzle beside it in the same launch turns.  The float64 visit says the same of these inputs (kept rotation; E_p falls
    beyond the rounding intervals of both sums, so the seed makes the fall no last-place matter)."""
    from puzzlenet_amd import ops
    cases = degenerate_cases(k)
    flat = [0, 1] if k == 1 else [0]      # one point is degenerate whatever the set was
    for P in (cases[z] for z in flat):
        g0 = jr.f32(P.G0)
        x = P.B[0].astype(np.float64)
        assert ref.is_degenerate((x - x.mean(axis=0)).T @ (x - x.mean(axis=0)))
        gn = g0.copy()
        gn[1] = jr.visit(P, g0, 1)
        assert np.array_equal(gn[1][:3, :3], g0[1][:3, :3])
        assert jr.objective_interval2(P.A[0], P.B[0], gn[0], gn[1])[1] < jr.objective_interval2(P.A[0], P.B[0], g0[0], g0[1])[0]
    if k > 1:
        x = cases[1].B[0].astype(np.float64)
        assert not ref.is_degenerate((x - x.mean(axis=0)).T @ (x - x.mean(axis=0)))
    G, score, score0, js, used, acc = _host(ops.joint_refine(*_stack(cases, dev), SWEEPS))
    for z, P in enumerate(cases):
        print(f"k = {k}, puzzle {z}: score0 {score0[z]:.6e} score {score[z]:.6e} accepted {acc[z].tolist()} sweeps {used[z]}")
        assert np.array_equal(G[z, 0], P.G0[0]) and acc[z, 0] == 0
        assert acc[z, 1] >= 1 and score[z] <= score0[z]
        if z in flat:
            assert np.array_equal(G[z, 1, :3, :3], P.G0[1, :3, :3]), z
            assert not np.array_equal(G[z, 1, :3, 3], P.G0[1, :3, 3])
        else:
            assert not np.array_equal(G[z, 1, :3, :3], P.G0[1, :3, :3])      # the rule did not fire everywhere


@pytest.mark.parametrize("graph", list(TRAJECTORY))
def test_short_trajectory_follows_the_float64_loop(visit_errors, dev, graph):
    from puzzlenet_amd import ops
    cases = trajectory_cases(graph)
    G, score, score0, js, used, acc = _host(ops.joint_refine(*_stack(cases, dev), 2))
    tol = STEP_FACTOR * max(r[0] for rows in visit_errors.values() for r in rows)
    left_out, worst = 0, 0.0
    for z, P in enumerate(cases):
        want = jr.refine(P, 2)
        if want.margin_ratio < MARGIN_FACTOR:
            left_out += 1
            continue
        assert acc[z].tolist() == want.accepted.tolist() and int(used[z]) == want.sweeps_used, (z, acc[z], want.accepted)
        err = max(ref.pose_err(G[z, p], want.G[p]) for p in range(P.K))
        worst = max(worst, err)
        assert err <= tol, (z, err, tol)
    print(f"{graph}: left out {left_out} of {len(cases)}, largest pose difference {worst:.3e} (tolerance {tol:.3e})")
    assert left_out == TRAJECTORY[graph] and left_out <= len(cases) // 4, left_out


def test_rejections_launch_nothing(dev, monkeypatch):
    from puzzlenet_amd import _lib, ops
    calls = []
    monkeypatch.setattr(ops, "_call", lambda *a, **k: calls.append(a[0]))
    eye = torch.eye(4, device=dev).reshape(1, 1, 4, 4).repeat(1, 3, 1, 1)
    pts = torch.zeros(2, 8, 3, device=dev)
    jl = torch.tensor([[[0, 1], [1, 2]]], dtype=torch.int32)
    mv = torch.ones(1, 3, dtype=torch.uint8, device=dev)
    ok = lambda **k: ops.joint_refine(k.get("a", pts), k.get("b", pts), k.get("jl", jl), k.get("G0", eye), k.get("mv", mv),
                                      k.get("sweeps", 3), a_of=k.get("a_of"), b_of=k.get("b_of"))
    for bad in (lambda: ok(a=torch.zeros(2, 0, 3, device=dev)),                                       # ka = 0
                lambda: ok(b=torch.zeros(2, 1025, 3, device=dev)),                                    # kb = 1025
                lambda: ok(sweeps=-1),
                lambda: ok(G0=torch.eye(4, device=dev).reshape(1, 1, 4, 4).repeat(1, 65, 1, 1),       # K = 65
                           mv=torch.ones(1, 65, dtype=torch.uint8, device=dev)),
                lambda: ok(jl=torch.zeros(1, 7, 2, dtype=torch.int32, device=dev), a=torch.zeros(7, 8, 3, device=dev),
                           b=torch.zeros(7, 8, 3, device=dev))):                                      # J = 7 > K (K - 1)
        with pytest.raises(_lib.PznUnsupported):
            bad()
    for bad in (lambda: ok(a=torch.zeros(2, 8, 2, device=dev)),
                lambda: ok(b=torch.zeros(8, 3, device=dev)),
                lambda: ok(G0=eye[0]),
                lambda: ok(a=pts[:1]),                                                                # one set, two rows, no map
                lambda: ok(a=pts.double()),
                lambda: ok(G0=eye.double()),
                lambda: ok(jl=jl.long()),
                lambda: ok(jl=jl[0]),
                lambda: ok(jl=torch.tensor([[[0, 3], [1, 2]]], dtype=torch.int32)),                   # j = K
                lambda: ok(jl=torch.tensor([[[0, 1], [2, 2]]], dtype=torch.int32)),                   # i = j
                lambda: ok(jl=torch.tensor([[[0, 1], [1, -1]]], dtype=torch.int32)),                  # j < 0 in a used row
                lambda: ok(jl=torch.tensor([[[0, 1], [0, 1]]], dtype=torch.int32)),                   # a pair twice
                lambda: ok(mv=mv.int()),
                lambda: ok(mv=mv[:, :2]),
                lambda: ok(a_of=torch.zeros(1, 2, dtype=torch.int32, device=dev)),
                lambda: ok(b_of=torch.zeros(2, dtype=torch.long, device=dev)),
                lambda: ok(a=pts.cpu()),
                lambda: ok(mv=mv.cpu())):
        with pytest.raises(_lib.PznError) as info:
            bad()
        assert not isinstance(info.value, _lib.PznUnsupported)
    assert calls == []
    assert ops.joint_refine_supported(1, 0, 1, 1) and ops.joint_refine_supported(64, 4032, 1024, 1024)
    assert not ops.joint_refine_supported(65, 1, 8, 8) and not ops.joint_refine_supported(3, 7, 8, 8)
    assert not ops.joint_refine_supported(3, 2, 0, 8) and not ops.joint_refine_supported(3, 2, 8, 1025)
    # no puzzles, or no joints: a success that launches nothing and returns G0 with scores of 0
    G, score, score0, js, used, acc = ops.joint_refine(pts[:0], pts[:0], jl[:0], eye[:0], mv[:0], 3)
    assert G.shape == (0, 3, 4, 4) and score.shape == (0,) and js.shape == (0, 2) and calls == []
    G, score, score0, js, used, acc = ops.joint_refine(pts[:0], pts[:0], jl[:, :0], eye, mv, 3)
    assert torch.equal(G, eye) and js.shape == (1, 0) and calls == []
    assert float(score.abs().max()) == 0 and float(score0.abs().max()) == 0 and int(used.abs().max()) == 0 and int(acc.abs().max()) == 0
