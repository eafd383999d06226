"""GPU: ops.joint_refine(..., auto=(lo_a, lo_b, power)) (joint_auto_kernel, pzn_joint_refine_auto_f32) - the joint refinement
that finds the two kept counts of every joint at every evaluation, under the poses being tried - against today's launches
(device bits against device bits), against exact integers and against the float64 statement tests/_joint_auto_ref.py (inputs:
tests/_joint_trim.py and that file; nothing below is tuned to the kernel).

 (1) lo = k is today's launch: the six outputs torch.equal with plain ops.joint_refine, objective == score, counts k, kept rows
     0 .. k-1 - at the upper end too, where the LDS image passes 64 KB and the launch raises the kernel's limit;
 (2) exact counts on the integer lattice: every float32 distance and sum is exact and most minima tie, so count_a, count_b and
     the kept rows at sweeps = 0 equal the statement's cross-multiplied integers;
 (3) a star around a root with the identity pose: the counts and kept rows of joint (0, j) are the pair kernel's with T0 = G_j;
 (4) one visit and (5) a short trajectory against the float64 statement, by the method of tests/test_gpu_joint_trim.py;
 (6) invariants on random sets; (7) what is refused launches nothing.
"""
import numpy as np
import pytest
import torch

from tests import _icp_auto_ref as au
from tests import _icp_ref as ref
from tests import _joint_auto_ref as ja
from tests import _joint_ref as jr
from tests import _joint_trim as jm
from tests import _joint_trim_ref as jt
from tests.test_gpu_joint_refine import ORTHO_TOL, _seq32

pytestmark = pytest.mark.gpu

SWEEPS = 6
NAMES = ("G", "score", "score0", "joint_score", "sweeps_used", "accepted", "kept_a", "kept_b", "count_a", "count_b", "objective",
         "objective0")
# (1): (ka, kb) -> Z: one row in all, rows that are no multiple of four on either side, one row per thread with every wavefront
# full, more rows than threads with unequal sides
FULL_SHAPES = {(1, 1): 4, (37, 29): 3, (64, 64): 3, (300, 70): 2}
# (2): (ka, kb) -> Z; (1024, 1024) on the `pair` graph alone: every thread owns four sorted slots of each direction and all four
# wavefronts contribute a total to the scan
LATTICE_SHAPES = {(5, 5): 4, (37, 29): 3, (160, 130): 2}
LATTICE_LARGE = (1024, 1024)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _stack(cases, dev):
    """tests/_joint_trim.stack without the counts: (a, b, joints on the host, G0, movable) of puzzles of one graph."""
    a = np.stack([A for P in cases for A in P.A]).astype(np.float32)
    b = np.stack([B for P in cases for B in P.B]).astype(np.float32)
    joints = torch.from_numpy(np.array([P.joints for P in cases], dtype=np.int32))
    G0 = np.stack([P.G0 for P in cases]).astype(np.float32)
    movable = np.stack([P.movable for P in cases]).astype(np.uint8)
    a, b, G0, movable = (torch.from_numpy(x).to(dev) for x in (a, b, G0, movable))
    return a, b, joints, G0, movable


def _run(args, sweeps, auto, kept=True, **kw):
    from puzzlenet_amd import ops
    a, b, jl, G0, mv = args
    return ops.joint_refine(a, b, jl, G0, mv, sweeps, auto=auto, return_kept=kept, **kw)


def _same(x, y):
    return len(x) == len(y) and all(torch.equal(u, v) for u, v in zip(x, y))


def _host(out):
    return [t.cpu().numpy() for t in out]


def _arange_like(t):
    return torch.arange(t.shape[-1], dtype=torch.int32, device=t.device).expand_as(t)


def _padded(rows, k):
    return np.concatenate((np.asarray(rows, dtype=np.int64), np.full(k - len(rows), -1, dtype=np.int64)))


# ---------------------------------------------------------------------------------------------- (1)

def _is_plain(plain, got, jl, ka, kb):
    assert len(plain) == 6 and len(got) == 12
    for name, x, y in zip(NAMES, plain, got[:6]):
        assert torch.equal(x, y), name
    kept_a, kept_b, count_a, count_b, objective, objective0 = got[6:]
    assert torch.equal(objective, got[1]) and torch.equal(objective0, got[2])      # r = 1: F is E
    live = (jl[..., 0] >= 0).to(got[0].device)      # (every row of these lists is a joint or unused)
    for kept, count, k in ((kept_a, count_a, ka), (kept_b, count_b, kb)):
        assert count.dtype == torch.int32 and kept.dtype == torch.int32 and kept.shape == (*count.shape, k)
        assert torch.equal(count, torch.where(live, k, 0).to(torch.int32))
        assert torch.equal(kept, torch.where(live[..., None], _arange_like(kept), torch.full_like(kept, -1)))


@pytest.mark.parametrize("shape", list(FULL_SHAPES), ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("graph", jm.GRAPHS)
def test_least_counts_of_k_are_today_s_launch(dev, graph, shape):
    from puzzlenet_amd import ops
    ka, kb = shape
    K, joints = jr.GRAPHS[graph]
    rng = np.random.default_rng(95000 + 100 * jm.GRAPHS.index(graph) + ka)
    args = _stack([jr.puzzle(rng, K, joints, shape) for _ in range(FULL_SHAPES[shape])], dev)
    plain = ops.joint_refine(*args, SWEEPS)
    assert ka == 1 or bool((plain[1] < plain[2]).any())      # something did move
    for power in (1, 2, 3, 4):
        _is_plain(plain, _run(args, SWEEPS, (ka, kb, power)), args[2], ka, kb)
    short = _run(args, SWEEPS, (ka, kb, 3), kept=False)      # without the kept rows: the counts and objectives behind the six
    assert len(short) == 10 and _same(short[:6], plain) and short[6].dtype == torch.int32 and torch.equal(short[8], plain[1])


def test_least_counts_of_k_where_the_lds_image_passes_64_kb(dev):
    """tests/test_gpu_joint_trim.py's shape: K = 64 pieces in a chain, J = K (K - 1) rows of which 63 are used, ka = kb = 1024:
    76.3 KB of LDS with the sorted minima.  One sweep, one puzzle."""
    from puzzlenet_amd import ops
    K, k = 64, 1024
    rng = np.random.default_rng(86000)
    P = jr.puzzle(rng, K, [(p, p + 1) for p in range(K - 1)], k)
    J = K * (K - 1)
    jl = torch.full((1, J, 2), -1, dtype=torch.int32)
    jl[0, :K - 1] = torch.tensor(P.joints, dtype=torch.int32)
    a = torch.zeros(J, k, 3)
    b = torch.zeros(J, k, 3)
    a[:K - 1], b[:K - 1] = torch.from_numpy(np.stack(P.A)), torch.from_numpy(np.stack(P.B))
    args = (a.to(dev), b.to(dev), jl, torch.from_numpy(P.G0)[None].to(dev), torch.from_numpy(P.movable.astype(np.uint8))[None].to(dev))
    plain = ops.joint_refine(*args, 1)
    got = _run(args, 1, (k, k, 3))
    assert int(got[5].sum()) > 0
    _is_plain(plain, got, jl, k, k)
    assert int((got[8][0, :K - 1] != k).sum()) == 0 and int(got[8][0, K - 1:].abs().sum()) == 0


# ---------------------------------------------------------------------------------------------- (2)

def _lattice_side(k):
    """Sites per axis: about as many sites as rows, so that minima of 0 and of a few units both occur."""
    return 4 if k < 100 else 6 if k < 1000 else 10


def _lattice_cases(graph, shape, Z):
    K, joints = jr.GRAPHS[graph]
    rng = np.random.default_rng(97000 + 100 * jm.GRAPHS.index(graph) + shape[0])
    return [jm.lattice_puzzle(rng, K, joints, shape, [shape] * len(joints), side=_lattice_side(shape[0])) for _ in range(Z)]


def _lattice_check(dev, cases, shape):
    ka, kb = shape
    J = len(cases[0].joints)
    args = _stack(cases, dev)
    how, tied = [], 0
    for lo_a, lo_b in ((1, 1), (-(-ka // 4), -(-kb // 4)), (ka, kb)):
        for power in (1, 3):
            G, score, score0, js, used, acc, kept_a, kept_b, count_a, count_b, obj, obj0 = _host(_run(args, 0, (lo_a, lo_b, power)))
            assert np.array_equal(G, args[3].cpu().numpy()) and np.array_equal(score, score0) and np.array_equal(obj, obj0)
            assert not used.any() and not acc.any()
            for z, P in enumerate(cases):
                for e in range(J):
                    w = ja.lattice_joint(P, e, lo_a, lo_b, power)
                    assert (int(count_a[z, e]), int(count_b[z, e])) == (w["count_a"], w["count_b"]), (z, e, lo_a, lo_b, power, w["how_a"],
                                                                                                   w["how_b"])
                    assert np.array_equal(kept_a[z, e], _padded(w["kept_a"], ka)) and np.array_equal(kept_b[z, e], _padded(w["kept_b"], kb))
                    if lo_a < ka and power == 3:
                        how += [w["how_a"], w["how_b"]]
                        tied += w["tied"]
    close = sum(h in ("tie", "unit") for h in how)
    print(f"{ka}x{kb}: {close} of {len(how)} counts decided by a tie or by one unit; {tied} repeated row minima")
    return close, len(how), tied


@pytest.mark.parametrize("shape", list(LATTICE_SHAPES), ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("graph", jm.GRAPHS)
def test_exact_counts_on_the_integer_lattice(dev, graph, shape):
    close, n, tied = _lattice_check(dev, _lattice_cases(graph, shape, LATTICE_SHAPES[shape]), shape)
    assert tied > 0 and 2 * close > n, (close, n, tied)      # the minima tie, and most counts are decided by a tie or one unit


def test_exact_counts_on_the_integer_lattice_with_four_sorted_slots_a_thread(dev):
    close, n, tied = _lattice_check(dev, _lattice_cases("pair", LATTICE_LARGE, 2), LATTICE_LARGE)
    assert tied > 0 and 2 * close > n, (close, n, tied)


# ---------------------------------------------------------------------------------------------- (3)

@pytest.mark.parametrize("shape", [(37, 29), (300, 70)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_a_star_around_an_identity_root_finds_the_pair_kernel_s_counts(dev, shape):
    """Joint (0, j) under G0 = (identity, G_j) is the pair problem (A fixed, B moved by T0 = G_j): the same images, distances,
    ranks and prefix sums, hence the same integers."""
    from puzzlenet_amd import ops
    ka, kb = shape
    K = 5
    joints = [(0, j) for j in range(1, K)]
    rng = np.random.default_rng(98000 + ka)
    cases = []
    for z in range(3):
        n = [int(round(s * min(ka, kb))) for s in rng.choice(au.SHARES, size=len(joints))]
        P, _, _ = jt.partial_puzzle(rng, K, joints, min(ka, kb), None, n_mate=n, quick=True)
        # (partial_puzzle makes square sets: side A is padded with rows of its own to ka, side B cut or padded to kb)
        A = [np.concatenate((x, x[rng.integers(0, len(x), ka - len(x))])) if ka > len(x) else x[:ka] for x in P.A]
        B = [np.concatenate((x, x[rng.integers(0, len(x), kb - len(x))])) if kb > len(x) else x[:kb] for x in P.B]
        A = [ref.transform(P.truth[0], x).astype(np.float32) for x in A]      # the root's frame becomes the root frame
        G0 = P.G0.copy()
        G0[0] = np.eye(4, dtype=np.float32)
        cases.append(jr.Puzzle(K, P.joints, A, B, G0, P.truth, P.movable))
    args = _stack(cases, dev)
    a, b, jl, G0, mv = args
    lo = (au.least_count(ka), au.least_count(kb), au.POWER)
    got = _run(args, 0, lo)
    T0 = G0[:, 1:].reshape(-1, 4, 4).contiguous()
    pair = ops.icp_refine(a, b, T0, 0, auto=lo, return_kept=True)
    count_a, count_b, _, kept_a, kept_b = pair[4:]
    assert torch.equal(got[8].reshape(-1), count_a) and torch.equal(got[9].reshape(-1), count_b)
    assert torch.equal(got[6].reshape(-1, ka), kept_a) and torch.equal(got[7].reshape(-1, kb), kept_b)
    assert len(set(count_a.tolist())) > 1 and int(count_a.min()) < ka      # the counts do differ per joint


# ---------------------------------------------------------------------------------------------- (4)

@pytest.fixture(scope="module")
def visit_errors(dev):
    """One visit of piece 1 over tests/_joint_auto_ref.visit_cases -> {graph: [(yardstick error, kernel error, entered)]}.
    Asserted here: for EVERY case every other piece keeps G0's bits, objective <= objective0, piece 1 is visited once at most
    and keeps G0's bits if its candidate was left; for an entered case the candidate is taken, the counts and kept rows under
    the returned poses are the statement's."""
    out = {}
    for graph in jm.VISIT_GRAPHS:
        cases = ja.visit_cases(graph)
        args = _stack(cases, dev)
        P0 = cases[0]
        G, score, score0, js, used, acc, kept_a, kept_b, count_a, count_b, obj, obj0 = _host(_run(args, 1, (P0.lo_a, P0.lo_b, P0.power)))
        G0 = args[3].cpu().numpy()
        assert np.isfinite(G).all() and np.array_equal(np.delete(G, 1, axis=1), np.delete(G0, 1, axis=1))
        assert (np.delete(acc, 1, axis=1) == 0).all() and (obj <= obj0).all()
        assert ((acc[:, 1] == 0) | (acc[:, 1] == 1)).all() and (used == acc[:, 1]).all()
        assert np.array_equal(G[acc[:, 1] == 0, 1], G0[acc[:, 1] == 0, 1]) and (obj[used == 0] == obj0[used == 0]).all()
        R = G[:, 1, :3, :3].astype(np.float64)
        assert np.abs(np.swapaxes(R, 1, 2) @ R - np.eye(3)).max() <= ORTHO_TOL and (np.linalg.det(R) > 0).all()
        rows = []
        for z, P in enumerate(cases):
            want, yard, entered, gap, each = ja.visit_row(P)
            if entered:
                assert acc[z, 1] == 1 and used[z] == 1, (graph, z)
                for e, o in each.items():
                    assert (int(count_a[z, e]), int(count_b[z, e])) == (o.m_a, o.m_b), (graph, z, e)
                    assert np.array_equal(kept_a[z, e], _padded(o.kept_a, ja.VISIT_K)), (graph, z, e)
                    assert np.array_equal(kept_b[z, e], _padded(o.kept_b, ja.VISIT_K)), (graph, z, e)
                assert _seq32(js[z]) == score[z]
            rows.append((yard, ref.pose_err(G[z, 1], want), entered))
        out[graph] = rows
    return out


def _tolerance(visit_errors):
    return jm.STEP_FACTOR * max(r[0] for rows in visit_errors.values() for r in rows)


def test_one_visit_pose_within_four_times_the_float32_restatement(visit_errors):
    tol = _tolerance(visit_errors)
    for graph, rows in visit_errors.items():
        ent = [r for r in rows if r[2]]
        print(f"{graph}: yardstick max {max(r[0] for r in rows):.3e}, kernel max {max(r[1] for r in ent):.3e}, entered {len(ent)} of "
              f"{len(rows)}")
        assert len(rows) - len(ent) <= ja.VISIT[graph] and 8 * (len(rows) - len(ent)) <= len(rows), graph
        for n, (_, k, e) in enumerate(rows):
            if e:
                assert k <= tol, (graph, n, k, tol)


# ---------------------------------------------------------------------------------------------- (5)

@pytest.mark.parametrize("graph", jm.GRAPHS)
def test_short_trajectory_follows_the_float64_statement(visit_errors, dev, graph):
    cases = ja.trajectory_cases(graph)
    args = _stack(cases, dev)
    P0 = cases[0]
    G, score, score0, js, used, acc, kept_a, kept_b, count_a, count_b, obj, obj0 = _host(
        _run(args, ja.TRAJECTORY_SWEEPS, (P0.lo_a, P0.lo_b, P0.power)))
    G0 = args[3].cpu().numpy()
    tol = _tolerance(visit_errors)
    assert np.isfinite(G).all() and (obj <= obj0).all() and np.array_equal(G[:, 0], G0[:, 0]) and (acc[:, 0] == 0).all()
    left_out, worst = 0, 0.0
    for z, P in enumerate(cases):
        want, entered = ja.trajectory_row(P)
        assert _seq32(js[z]) == score[z]
        if not entered:
            left_out += 1
            continue
        assert acc[z].tolist() == want.accepted.tolist() and int(used[z]) == want.sweeps_used, (z, acc[z], want.accepted)
        for e in range(len(P.joints)):
            assert (int(count_a[z, e]), int(count_b[z, e])) == (want.count_a[e], want.count_b[e]), (z, e)
            assert np.array_equal(kept_a[z, e], _padded(want.kept_a[e], ja.TRAJECTORY_K)), (z, e)
            assert np.array_equal(kept_b[z, e], _padded(want.kept_b[e], ja.TRAJECTORY_K)), (z, e)
        err = max(ref.pose_err(G[z, p], want.G[p]) for p in range(P.K))
        worst = max(worst, err)
        assert err <= tol, (z, err, tol)
    print(f"{graph}: left out {left_out} of {len(cases)}, largest pose difference {worst:.3e} (tolerance {tol:.3e})")
    assert left_out <= ja.TRAJECTORY[graph] and 8 * left_out <= len(cases), left_out


# ---------------------------------------------------------------------------------------------- (6)

@pytest.mark.parametrize("graph", jm.GRAPHS)
def test_invariants_on_random_sets(dev, graph):
    ka, kb, Z = 37, 29, 4
    K, joints = jr.GRAPHS[graph]
    J = len(joints)
    rng = np.random.default_rng(99000 + jm.GRAPHS.index(graph))
    cases = []
    for _ in range(Z):
        P, _, _ = jt.partial_puzzle(rng, K, joints, ka, None, n_mate=rng.integers(10, ka + 1, size=J), quick=True)
        cases.append(jr.Puzzle(K, P.joints, P.A, [B[:kb] for B in P.B], P.G0, P.truth, P.movable))
    args = _stack(cases, dev)
    a, b, jl, G0, mv = args
    lo = (au.least_count(ka), au.least_count(kb), au.POWER)
    full = _run(args, SWEEPS, lo)
    G, score, score0, js, used, acc, kept_a, kept_b, count_a, count_b, obj, obj0 = full
    assert bool((obj <= obj0).all()) and bool((obj < obj0).any()) and bool(torch.isfinite(G).all())
    assert int(count_a.min()) >= lo[0] and int(count_a.max()) <= ka and int(count_b.min()) >= lo[1] and int(count_b.max()) <= kb
    assert int(count_a.min()) < ka                                                   # something was trimmed
    assert torch.equal((kept_a >= 0).sum(-1).to(torch.int32), count_a) and torch.equal((kept_b >= 0).sum(-1).to(torch.int32), count_b)
    for z in range(Z):
        assert _seq32(js[z].cpu().numpy()) == float(score[z])
    assert _same(full, _run(args, SWEEPS, lo))                                       # two launches: the same bits
    for z in (0, Z - 1):                                                             # a puzzle alone: its bits of the batch
        s = slice(z * J, (z + 1) * J)
        alone = _run((a[s], b[s], jl[z:z + 1], G0[z:z + 1], mv[z:z + 1]), SWEEPS, lo)
        assert all(torch.equal(x[z:z + 1], y) for x, y in zip(full, alone)), z
    # a row with a bad (i, j) on a device list (a host list is refused): score 0, counts 0, kept rows all -1, and the others
    # as if the row were switched off
    for e, bad in ((0, (0, 0)), (J - 1, (K, 0)), (J // 2, (1, -1))):
        holed, off = jl.clone(), jl.clone()
        holed[:, e] = torch.tensor(bad, dtype=torch.int32)
        off[:, e] = -1
        got = _run((a, b, holed.to(dev), G0, mv), 2, lo)
        assert _same(got, _run((a, b, off, G0, mv), 2, lo)), (e, bad)
        assert int((got[3][:, e] != 0).sum()) == 0 and int(got[8][:, e].abs().sum()) == 0 and int(got[9][:, e].abs().sum()) == 0
        assert int((got[6][:, e] != -1).sum()) == 0 and int((got[7][:, e] != -1).sum()) == 0
        if J > 1:
            rest = [x for x in range(J) if x != e]
            assert bool((got[8][:, rest] >= lo[0]).all()) and bool((got[6][:, rest][..., 0] >= 0).all())


# ---------------------------------------------------------------------------------------------- (7)

def test_rejections_launch_nothing(dev, monkeypatch):
    from puzzlenet_amd import _lib, ops
    calls = []
    monkeypatch.setattr(ops, "_call", lambda *a, **k: calls.append(a[0]))
    eye = torch.eye(4, device=dev).reshape(1, 1, 4, 4).repeat(1, 3, 1, 1)
    pts = torch.zeros(2, 8, 3, device=dev)
    jl = torch.tensor([[[0, 1], [1, 2]]], dtype=torch.int32)
    mv = torch.ones(1, 3, dtype=torch.uint8, device=dev)
    m8 = torch.full((1, 2), 8, dtype=torch.int32, device=dev)
    n8 = torch.full((2,), 8, dtype=torch.int32, device=dev)
    go = lambda sweeps=3, **k: ops.joint_refine(pts, pts, jl, eye, mv, sweeps, **k)
    for bad in ((0, 2, 3), (2, 0, 3), (9, 2, 3), (2, 9, 3), (2, 2, 0), (2, 2, 5)):      # lo of 0 or above k, power of 0 or 5
        with pytest.raises(_lib.PznUnsupported, match="1 <= power <= 4"):
            go(auto=bad)
    with pytest.raises(_lib.PznUnsupported):
        go(sweeps=-1, auto=(2, 2, 3))
    big = torch.zeros(2, 1025, 3, device=dev)
    with pytest.raises(_lib.PznUnsupported):                                            # k out of range
        ops.joint_refine(big, big, jl, eye, mv, 3, auto=(2, 2, 3))
    eye65 = torch.eye(4, device=dev).reshape(1, 1, 4, 4).repeat(1, 65, 1, 1)
    with pytest.raises(_lib.PznUnsupported):                                            # K out of range
        ops.joint_refine(pts, pts, jl, eye65, torch.ones(1, 65, dtype=torch.uint8, device=dev), 3, auto=(2, 2, 3))
    for bad in (dict(auto=(2, 2, 3), ma=m8), dict(auto=(2, 2, 3), mb=m8), dict(auto=(2, 2, 3), na=n8), dict(auto=(2, 2, 3), nb=n8),
                dict(auto=(2, 2)), dict(auto=(2.0, 2, 3)), dict(auto=(True, 2, 3)), dict(auto="auto")):
        with pytest.raises(_lib.PznError) as info:
            go(**bad)
        assert not isinstance(info.value, _lib.PznUnsupported)
    assert calls == []
    go(auto=(2, 2, 3))
    go(auto=[8, 8, 1], return_kept=True)
    go()
    assert calls == ["pzn_joint_refine_auto_f32"] * 2 + ["pzn_joint_refine_f32"]
    # no puzzles, or no joints: G0 with scores of 0, counts of shape [Z, 0], and no launch
    out = ops.joint_refine(pts[:0], pts[:0], jl[:, :0], eye, mv, 3, auto=(2, 2, 3), return_kept=True)
    assert len(out) == 12 and torch.equal(out[0], eye) and out[3].shape == (1, 0) and out[6].shape == (1, 0, 8)
    assert out[8].shape == out[9].shape == (1, 0) and out[8].dtype == torch.int32
    assert float(out[1].abs().sum()) == float(out[10].abs().sum()) == float(out[11].abs().sum()) == 0.0
    out = ops.joint_refine(pts[:0], pts[:0], jl[:0], eye[:0], mv[:0], 3, auto=(2, 2, 3))
    assert len(out) == 10 and out[0].shape == (0, 3, 4, 4) and out[6].shape == (0, 2) and out[8].shape == (0,)
    assert len(calls) == 3
