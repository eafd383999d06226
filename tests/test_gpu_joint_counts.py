"""GPU: ops.joint_refine(..., na=, nb=) (joint_refine_counts_kernel, pzn_joint_refine_counts_f32) - the joint refinement with
a point count per set - against the launch without counts (device bits against device bits) and against the float64
restatement tests/_joint_ref.py on ragged sets (tests/_joint_counts.py; nothing below is tuned to the kernel).

Identities, every output torch.equal:
 (1) counts equal to the strides everywhere, on one side or on both, are the launch without counts;
 (2) one count (m_a, m_b) for all sets is the launch without counts on the sets cut to m_a / m_b rows - "the counts replace
     ka / kb and nothing else", at sizes where the float64 margin rule would leave most cases out;
 (3) pair graph: puzzle z of a launch with mixed counts is puzzle z alone on its cut sets;
 (4) what lies behind a count is never read: NaN, 1e30 and zeros there give the same bits;
 (5) the counts are found through the set maps;
 (6) a count outside [1, ka] skips the row like i = -1 does: the launch without the row, and joint_score exactly 0.
Float64 (tests/test_gpu_joint_refine.py's checks and bounds, on the ragged sets):
 (7) properties; (8) one visit; (9) a short trajectory; (10) rejections launch nothing.
(8): STEP_FACTOR x the largest error of _joint_ref.visit_f32, the visit restated plainly in float32, and never the kernel,
is the tolerance; tests/_joint_counts.py says why it is taken over the cases whose optimum is unique, and why only those enter.
"""
import numpy as np
import pytest
import torch

from tests import _icp_ref as ref
from tests import _joint_counts as jc
from tests import _joint_ref as jr
from tests.test_gpu_joint_refine import ORTHO_TOL, _seq32, checked

pytestmark = pytest.mark.gpu

SWEEPS = 30
# name -> (strides (ka, kb), counts of side a, counts of side b, Z, sweeps): every count 1..8 (count 1: the degenerate scatter;
# 3 / 4 / 5 around the float4 tail); the wave edge and unequal strides; na + nb across the 256 rows a pass of the threads owns
# (na = 255, nb = 2 is forced into puzzle 0); the upper limit (its first joint is (1000, 7)); more puzzles than workgroups
# (counts met on the grid walk)
SHAPES = {
    "R1": ((8, 8), range(1, 9), range(1, 9), 64, SWEEPS),
    "R2": ((64, 65), (1, 3, 4, 5, 63, 64), (1, 3, 4, 5, 63, 64, 65), 3, SWEEPS),
    "R3": ((300, 300), (2, 255, 256, 257, 300), (2, 255, 256, 257, 300), 2, SWEEPS),
    "R4": ((1024, 1024), (7, 1000, 1024), (7, 1000, 1024), 1, 2),
    "R5": ((8, 8), range(1, 9), range(1, 9), 600, SWEEPS),
}
FULL = ["R1", "R2", "R3", "R4"]
UNIFORM = {"R1": (5, 3), "R2": (63, 64), "R3": (257, 255), "R4": (1000, 7)}      # (2): one count below the stride for all sets
FILLS = (float("nan"), 1e30, 0.0)
# one-visit check on an MI355X over the 96 cases: largest yardstick error / largest kernel error
MEASURED_STEP = "yardstick 3.637e-01, over unique optima 5.088e-06, kernel 2.132e-07 (93 of 96 cases entered)"


def _ragged_cases(graph, name):
    (ka, kb), ca, cb, Z, _ = SHAPES[name]
    K, joints = jr.GRAPHS[graph]
    rng = np.random.default_rng(83000 + 100 * jc.GRAPHS.index(graph) + int(name[1]))
    ca, cb = list(ca), list(cb)
    out = []
    for z in range(Z):
        counts = [(int(rng.choice(ca)), int(rng.choice(cb))) for _ in joints]
        if name == "R3" and z == 0:
            counts[0] = (255, 2)
        if name == "R3" and z == 1:
            counts[-1] = (2, 257)
        if name == "R4":
            counts[0] = (1000, 7)                  # (one puzzle, and a pair graph has one joint: padding on both sides)
        out.append(jc.ragged_puzzle(rng, K, joints, counts))
    return out


def _full_cases(graph, name):
    (ka, kb), _, _, Z, _ = SHAPES[name]
    K, joints = jr.GRAPHS[graph]
    rng = np.random.default_rng(84000 + 100 * jc.GRAPHS.index(graph) + int(name[1]))
    return [jr.puzzle(rng, K, joints, (ka, kb)) for _ in range(min(Z, 8))]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _to(args, dev):
    """stack()'s tuple with everything but the joint list on the device (the list stays the caller's host copy)."""
    a, b, na, nb, jl, G0, mv = args
    return a.to(dev), b.to(dev), na.to(dev), nb.to(dev), jl, G0.to(dev), mv.to(dev)


def _run(args, sweeps, counts=True, **kw):
    from puzzlenet_amd import ops
    a, b, na, nb, jl, G0, mv = args
    return ops.joint_refine(a, b, jl, G0, mv, sweeps, na=na if counts else None, nb=nb if counts else None, **kw)


def _same(x, y):
    return all(torch.equal(u, v) for u, v in zip(x, y))


def _host(out):
    return [t.cpu().numpy() for t in out]


@pytest.fixture(scope="module")
def runs(dev):
    """Every graph's and shape's ragged cases (NaN behind the counts) and their run: made once, read by the tests below."""
    out = {}
    for graph in jc.GRAPHS:
        for name, shape in SHAPES.items():
            cases = _ragged_cases(graph, name)
            args = _to(jc.stack(cases, shape[0], float("nan")), dev)
            full = _run(args, shape[4])
            out[graph, name] = dict(cases=cases, dev=args, sweeps=shape[4], full_dev=full, full=_host(full))
    return out


@pytest.fixture(scope="module")
def full_inputs(dev):
    """Sets that fill their strides (tests/_joint_ref.puzzle), for (1) and (2), and their run without counts."""
    out = {}
    for graph in jc.GRAPHS:
        for name in FULL:
            cases = _full_cases(graph, name)
            args = _to(jc.stack(cases, SHAPES[name][0], float("nan")), dev)
            assert not bool(args[0].isnan().any()) and not bool(args[1].isnan().any())
            out[graph, name] = (args, _run(args, SHAPES[name][4], counts=False))
    return out


@pytest.mark.parametrize("name", FULL)
@pytest.mark.parametrize("graph", jc.GRAPHS)
def test_full_counts_are_the_launch_without_counts(full_inputs, graph, name):
    args, plain = full_inputs[graph, name]
    a, b, na, nb, jl, G0, mv = args
    (ka, kb), sweeps = SHAPES[name][0], SHAPES[name][4]
    assert int(na.min()) == int(na.max()) == ka and int(nb.min()) == int(nb.max()) == kb
    assert _same(plain, _run(args, sweeps))
    assert _same(plain, _run((a, b, na, None, jl, G0, mv), sweeps))          # na alone: b at its stride
    assert _same(plain, _run((a, b, None, nb, jl, G0, mv), sweeps))          # nb alone
    assert _same(plain, _run((a, b, na.cpu(), nb.cpu(), jl, G0, mv), sweeps))      # host counts: checked and uploaded
    assert bool((plain[1] < plain[2]).any())                                  # (something did move)


@pytest.mark.parametrize("name", FULL)
@pytest.mark.parametrize("graph", jc.GRAPHS)
def test_a_uniform_count_is_the_launch_without_counts_on_cut_sets(full_inputs, graph, name):
    (a, b, na, nb, jl, G0, mv), _ = full_inputs[graph, name]
    ma, mb = UNIFORM[name]
    sweeps = SHAPES[name][4]
    cut = _run((a[:, :ma].contiguous(), b[:, :mb].contiguous(), None, None, jl, G0, mv), sweeps, counts=False)
    # behind the count: the sets' own further points, which a kernel that read them would use
    got = _run((a, b, torch.full_like(na, ma), torch.full_like(nb, mb), jl, G0, mv), sweeps)
    assert _same(cut, got)
    one = _run((a, b[:, :mb].contiguous(), torch.full_like(na, ma), None, jl, G0, mv), sweeps)
    assert _same(cut, one)


@pytest.mark.parametrize("name", ["R1", "R2"])
def test_mixed_counts_pair_graph_each_puzzle_is_itself_alone_on_cut_sets(runs, name):
    r = runs["pair", name]
    a, b, na, nb, jl, G0, mv = r["dev"]
    nah, nbh = na.cpu().tolist(), nb.cpu().tolist()
    assert len(set(zip(nah, nbh))) > 1
    for z in range(len(r["cases"])):
        alone = _run((a[z:z + 1, :nah[z]].contiguous(), b[z:z + 1, :nbh[z]].contiguous(), None, None, jl[z:z + 1], G0[z:z + 1],
                      mv[z:z + 1]), r["sweeps"], counts=False)
        assert all(torch.equal(x[z:z + 1], y) for x, y in zip(r["full_dev"], alone)), (z, nah[z], nbh[z])


@pytest.mark.parametrize("name", list(SHAPES))
@pytest.mark.parametrize("graph", jc.GRAPHS)
def test_padding_is_never_read_and_counts_follow_the_set_maps(runs, dev, graph, name):
    r = runs[graph, name]
    a, b, na, nb, jl, G0, mv = r["dev"]
    Z, J = jl.shape[:2]
    assert bool(a.isnan().any()) and bool(b.isnan().any())                    # the fixture's fill is NaN
    assert not any(bool(t.isnan().any()) for t in r["full_dev"])
    for fill in FILLS[1:]:
        other = _to(jc.stack(r["cases"], SHAPES[name][0], fill), dev)
        assert _same(r["full_dev"], _run(other, r["sweeps"])), fill
    # the sets of a permuted, those of b reversed, the counts with them
    perm = torch.from_numpy(np.random.default_rng(2).permutation(Z * J)).to(dev)
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(Z * J, device=dev)
    mapped = _run((a[perm].contiguous(), b.flip(0).contiguous(), na[perm].contiguous(), nb.flip(0).contiguous(), jl.to(dev), G0, mv),
                  r["sweeps"], a_of=inv.reshape(Z, J), b_of=torch.arange(Z * J - 1, -1, -1, device=dev).reshape(Z, J))
    assert _same(r["full_dev"], mapped)


@pytest.mark.parametrize("name", list(SHAPES))
@pytest.mark.parametrize("graph", jc.GRAPHS)
def test_a_bad_count_skips_the_row(runs, dev, graph, name, monkeypatch):
    """tests/test_gpu_joint_refine.py's unused-row check with the row switched off by its count: row e of every puzzle, which
    is the last set of its buffer only where the launch has one set."""
    from puzzlenet_amd import _lib, ops
    r = runs[graph, name]
    a, b, na, nb, jl, G0, mv = r["dev"]
    (ka, kb), sweeps = SHAPES[name][0], r["sweeps"]
    Z, J = jl.shape[:2]
    e = J // 2
    keep = [x for x in range(J) if x != e]
    rows = torch.arange(Z * J, device=dev).reshape(Z, J)
    without = _run((a, b, na, nb, jl[:, keep].contiguous(), G0, mv), sweeps, a_of=rows[:, keep].contiguous(),
                   b_of=rows[:, keep].contiguous())
    for side, bad in ((2, 0), (2, ka + 1), (3, 0), (3, kb + 1), (2, -1)):
        args = list(r["dev"])
        args[side] = args[side].clone()
        args[side][rows[:, e]] = bad
        holed = _run(args, sweeps)
        for n, (x, y) in enumerate(zip(holed, without)):
            if n == 3:
                assert torch.equal(x[:, keep], y) and int((x[:, e] != 0).sum()) == 0, (side, bad)
            else:
                assert torch.equal(x, y), (side, bad, n)
        # the same counts as the caller's host copy: refused before any launch
        calls = []
        with monkeypatch.context() as m:
            m.setattr(ops, "_call", lambda *a_, **k_: calls.append(a_[0]))
            host = list(r["dev"])
            host[side] = args[side].cpu()
            with pytest.raises(_lib.PznError) as info:
                _run(host, sweeps)
            assert not isinstance(info.value, _lib.PznUnsupported) and calls == []


def _some_joints(P):
    J = len(P.joints)
    big = max(max(len(s) for s in P.A), max(len(s) for s in P.B)) > 256
    return list(range(J)) if not big or J <= 5 else [0, J // 3, (2 * J) // 3, J - 1]


@pytest.mark.parametrize("name", list(SHAPES))
@pytest.mark.parametrize("graph", jc.GRAPHS)
def test_properties(runs, dev, graph, name):
    r = runs[graph, name]
    cases, sweeps = r["cases"], r["sweeps"]
    a, b, na, nb, jl, G0, mv = r["dev"]
    Z, J = jl.shape[:2]
    K = jr.GRAPHS[graph][0]
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
    print(f"{graph} {name}: sweeps_used mean {used.mean():.2f} max {used.max()}, score/score0 mean {np.mean(score / score0):.3f}")
    for z in range(Z):
        assert _seq32(js[z]) == score[z], (z, _seq32(js[z]), score[z])
        R = G[z, :, :3, :3].astype(np.float64)
        assert np.abs(np.swapaxes(R, 1, 2) @ R - np.eye(3)).max() <= ORTHO_TOL and (np.linalg.det(R) > 0).all()
    # sweeps = 0 returns G0, and its scores are those of the start pose
    G_0, s_0, s0_0, js_0, u_0, a_0 = _run(r["dev"], 0)
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
                assert iv[e, 0] <= float(jsc[e]) <= iv[e, 1], (z, e, len(P.A[e]), len(P.B[e]), iv[e], float(jsc[e]))
            assert _seq32(jsc) == tot
            if len(some) == J:
                lo, hi = jr.sum_interval(iv)
                assert lo <= float(tot) <= hi, (z, lo, float(tot), hi)
    # two runs: the same bits in every output
    assert _same(r["full_dev"], _run(r["dev"], sweeps))
    # from the returned poses, a puzzle that stopped by itself does not move
    Gd = r["full_dev"][0]
    G2, s2, s02, js2, u2, a2 = _run((a, b, na, nb, jl, Gd, mv), sweeps)
    stopped = torch.from_numpy(used < sweeps).to(dev)
    if bool(stopped.any()):
        assert int(u2[stopped].abs().max()) == 0 and int(a2[stopped].abs().max()) == 0
        assert torch.equal(G2[stopped], Gd[stopped]) and torch.equal(s02[stopped], r["full_dev"][1][stopped])
        assert torch.equal(s2[stopped], s02[stopped]) and torch.equal(js2[stopped], r["full_dev"][3][stopped])
    # Z puzzles in one launch = each puzzle alone
    for z in sorted(set([0, Z // 2, Z - 1])):
        s = slice(z * J, (z + 1) * J)
        alone = _run((a[s], b[s], na[s], nb[s], jl[z:z + 1], G0[z:z + 1], mv[z:z + 1]), sweeps)
        assert all(torch.equal(x[z:z + 1], y) for x, y in zip(r["full_dev"], alone)), z


@pytest.fixture(scope="module")
def visit_errors(dev):
    """(8) over tests/_joint_counts.visit_cases -> {graph: [(yardstick error, kernel error, entered, accepted, sweeps_used,
    gap)]}.  Asserted here for EVERY case, entered or not - and for a case that does not enter (three of the 96: two with no
    unique optimum, one left out by the margin and interval rule) this is all that is asserted, neither a pose nor `accepted`: every other
    piece's pose is G0 bit for bit, score <= score0, piece 1 is visited once at most and keeps G0's bits if its candidate was
    left, and its rotation is orthonormal."""
    out = {}
    for graph in jc.VISIT_GRAPHS:
        cases = jc.visit_cases(graph)
        args = _to(jc.stack(cases, (8, 8), float("nan")), dev)
        G, score, score0, js, used, acc = _host(_run(args, 1))
        G0 = args[5].cpu().numpy()
        assert np.array_equal(np.delete(G, 1, axis=1), np.delete(G0, 1, axis=1))
        assert (np.delete(acc, 1, axis=1) == 0).all() and (score <= score0).all()
        assert ((acc[:, 1] == 0) | (acc[:, 1] == 1)).all() and (used == acc[:, 1]).all()
        assert np.array_equal(G[acc[:, 1] == 0, 1], G0[acc[:, 1] == 0, 1]) and (score[used == 0] == score0[used == 0]).all()
        R = G[:, 1, :3, :3].astype(np.float64)
        assert np.abs(np.swapaxes(R, 1, 2) @ R - np.eye(3)).max() <= ORTHO_TOL and (np.linalg.det(R) > 0).all()
        rows = []
        for z, P in enumerate(cases):
            want, yard, entered, gap = jc.visit_row(P)
            rows.append((yard, ref.pose_err(G[z, 1], want), entered, int(acc[z, 1]), int(used[z]), gap))
        out[graph] = rows
    return out


def _tolerances(visit_errors):
    rows = [r for rows in visit_errors.values() for r in rows]
    return jc.STEP_FACTOR * max(r[0] for r in rows), jc.STEP_FACTOR * max(r[0] for r in rows if r[5] >= jc.GAP_MIN)


def test_one_visit_pose_within_four_times_the_float32_restatement(visit_errors):
    rows_all = [r for rows in visit_errors.values() for r in rows]
    tol_all, tol = _tolerances(visit_errors)
    entered = sum(r[2] for r in rows_all)
    for graph, rows in visit_errors.items():
        ent = [r for r in rows if r[2]]
        print(f"{graph}: yardstick max {max(r[0] for r in rows):.3e}, over unique optima "
              f"{max(r[0] for r in rows if r[5] >= jc.GAP_MIN):.3e}, kernel max {max(r[1] for r in ent):.3e}, "
              f"entered {len(ent)} of {len(rows)}")
    print(f"all: yardstick {tol_all / jc.STEP_FACTOR:.3e}, over unique optima {tol / jc.STEP_FACTOR:.3e}, kernel "
          f"{max(r[1] for r in rows_all if r[2]):.3e}, entered {entered} of {len(rows_all)}")
    assert 4 * entered >= 3 * len(rows_all), (entered, len(rows_all))
    assert tol <= tol_all
    for graph, rows in visit_errors.items():
        for n, (_, k, e, acc, used, _) in enumerate(rows):
            if e:
                assert acc == 1 and used == 1, (graph, n)
                assert k <= tol_all and k <= tol, (graph, n, k, tol)


@pytest.mark.parametrize("graph", jc.GRAPHS)
def test_short_trajectory_follows_the_float64_loop(visit_errors, dev, graph):
    cases = jc.trajectory_cases(graph)
    args = _to(jc.stack(cases, (8, 8), float("nan")), dev)
    G, score, score0, js, used, acc = _host(_run(args, jc.TRAJECTORY_SWEEPS))
    tol = _tolerances(visit_errors)[1]                 # (8)'s tolerance, the one that binds (every optimum here is unique)
    left_out, worst = 0, 0.0
    for z, P in enumerate(cases):
        want = jr.refine(P, jc.TRAJECTORY_SWEEPS)
        if want.margin_ratio < jc.MARGIN_FACTOR:
            left_out += 1
            continue
        assert acc[z].tolist() == want.accepted.tolist() and int(used[z]) == want.sweeps_used, (z, acc[z], want.accepted)
        err = max(ref.pose_err(G[z, p], want.G[p]) for p in range(P.K))
        worst = max(worst, err)
        assert err <= tol, (z, err, tol)
    print(f"{graph}: left out {left_out} of {len(cases)}, largest pose difference {worst:.3e} (tolerance {tol:.3e})")
    assert left_out == jc.TRAJECTORY[graph] and left_out <= 4, left_out


def test_rejections_launch_nothing(dev, monkeypatch):
    from puzzlenet_amd import _lib, ops
    calls = []
    monkeypatch.setattr(ops, "_call", lambda *a, **k: calls.append(a[0]))
    eye = torch.eye(4, device=dev).reshape(1, 1, 4, 4).repeat(1, 3, 1, 1)
    pts = torch.zeros(2, 8, 3, device=dev)
    jl = torch.tensor([[[0, 1], [1, 2]]], dtype=torch.int32)
    mv = torch.ones(1, 3, dtype=torch.uint8, device=dev)
    n8 = torch.full((2,), 8, dtype=torch.int32, device=dev)
    go = lambda **k: ops.joint_refine(pts, k.get("b", pts), jl, eye, mv, 3, b_of=k.get("b_of"), na=k.get("na"), nb=k.get("nb"))
    for bad in (lambda: go(na=n8.long()),                                         # a wrong dtype: no silent conversion
                lambda: go(nb=n8.float()),
                lambda: go(na=n8[:1]),                                            # one count for two sets
                lambda: go(nb=torch.full((3,), 8, dtype=torch.int32, device=dev)),
                lambda: go(na=n8.reshape(1, 2)),                                  # per joint row [Z,J] instead of per set
                lambda: go(nb=n8.reshape(2, 1)),
                lambda: go(na=[8, 8]),                                            # no tensor
                lambda: go(na=torch.full((2,), 8, dtype=torch.int32, device="meta")),      # neither the GPU nor the host
                lambda: go(na=torch.tensor([8, 9], dtype=torch.int32)),           # host copies are range-checked
                lambda: go(nb=torch.tensor([0, 8], dtype=torch.int32)),
                # a count per SET, not per row: one set that serves both rows has one count
                lambda: go(b=pts[:1], b_of=torch.zeros(1, 2, dtype=torch.long, device=dev), nb=n8)):
        with pytest.raises(_lib.PznError) as info:
            bad()
        assert not isinstance(info.value, _lib.PznUnsupported)
    assert calls == []
    # what is accepted goes to the new entry point, and without counts to the old one
    go(na=n8)
    go(b=pts[:1], b_of=torch.zeros(1, 2, dtype=torch.long, device=dev), nb=torch.tensor([1], dtype=torch.int32))
    go()
    assert calls == ["pzn_joint_refine_counts_f32", "pzn_joint_refine_counts_f32", "pzn_joint_refine_f32"]
    # no puzzles, or no joints: still a success that launches nothing
    G, score, score0, js, used, acc = ops.joint_refine(pts[:0], pts[:0], jl[:, :0], eye, mv, 3, na=n8[:0], nb=n8[:0])
    assert torch.equal(G, eye) and js.shape == (1, 0) and len(calls) == 3
