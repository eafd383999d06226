"""GPU: ops.joint_refine(..., ma=, mb=, return_kept=) (joint_trim_kernel, pzn_joint_refine_trim_f32) - the joint refinement
whose kept rows are chosen again at every evaluation - against today's launch (device bits against device bits) and against
the float64 statement tests/_joint_trim_ref.py (inputs: tests/_joint_trim.py; nothing below is tuned to the kernel).

 (1) full counts, as tensors or as None, are pzn_joint_refine_f32: all six outputs torch.equal, kept rows 0 .. k-1 - at the
     sibling's upper end too, where the LDS image passes 64 KB and the launch raises the kernel's limit;
 (2) exact kept sets: integer points under axis permutations, so every float32 distance is exact and many minima tie; kept_a,
     kept_b equal the statement's at sweeps = 0 and joint_score its energy to the rounding of the two means; a count of 0 or
     of k + 1 skips the row;
 (3) one visit and (4) short trajectories against the float64 statement, by the method of tests/test_gpu_joint_counts.py;
 (5) repeatability; (6) what is refused launches nothing.
"""
import numpy as np
import pytest
import torch

from tests import _icp_ref as ref
from tests import _joint_ref as jr
from tests import _joint_trim as jm
from tests import _joint_trim_ref as jt
from tests.test_gpu_joint_refine import ORTHO_TOL, _seq32

pytestmark = pytest.mark.gpu

SWEEPS = 30
U32 = 2.0 ** -24
# (1): (ka, kb) -> (Z, sweeps): the float4 tail, the wave edge with unequal sides, more rows than threads, the upper limit
FULL_SHAPES = {(8, 8): (24, SWEEPS), (7, 5): (24, SWEEPS), (64, 65): (3, SWEEPS), (257, 300): (2, SWEEPS), (1024, 1024): (1, 2)}
# (2): (ka, kb) -> Z: k no multiple of 4 (the scan's tail loop), and ka + kb > 256 with ka != kb (a thread owns two rows)
LATTICE_SHAPES = {(5, 5): 24, (7, 7): 24, (33, 33): 8, (160, 130): 4}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _to(args, dev):
    """stack()'s tuple with everything but the joint list on the device (the list stays the caller's host copy)."""
    a, b, ma, mb, jl, G0, mv = args
    return a.to(dev), b.to(dev), ma.to(dev), mb.to(dev), jl, G0.to(dev), mv.to(dev)


def _run(args, sweeps, counts=True, kept=True, **kw):
    from puzzlenet_amd import ops
    a, b, ma, mb, jl, G0, mv = args
    return ops.joint_refine(a, b, jl, G0, mv, sweeps, ma=ma if counts else None, mb=mb if counts else None, return_kept=kept, **kw)


def _same(x, y):
    return len(x) == len(y) and all(torch.equal(u, v) for u, v in zip(x, y))


def _host(out):
    return [t.cpu().numpy() for t in out]


def _arange_like(t):
    return torch.arange(t.shape[-1], dtype=torch.int32, device=t.device).expand_as(t)


# ---------------------------------------------------------------------------------------------- (1)

@pytest.mark.parametrize("shape", list(FULL_SHAPES), ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("graph", jm.GRAPHS)
def test_full_counts_are_today_s_kernel(dev, graph, shape):
    Z, sweeps = FULL_SHAPES[shape]
    K, joints = jr.GRAPHS[graph]
    rng = np.random.default_rng(85000 + 100 * jm.GRAPHS.index(graph) + shape[0])
    cases = [jt.with_counts(jr.puzzle(rng, K, joints, shape)) for _ in range(Z)]
    args = _to(jm.stack(cases), dev)
    a, b, ma, mb, jl, G0, mv = args
    assert int(ma.min()) == int(ma.max()) == shape[0] and int(mb.min()) == int(mb.max()) == shape[1]
    plain = _run(args, sweeps, counts=False, kept=False)
    assert len(plain) == 6 and bool((plain[1] < plain[2]).any())                    # today's tuple, and something did move
    got = _run(args, sweeps)
    assert len(got) == 8 and _same(plain, got[:6])
    assert torch.equal(got[6], _arange_like(got[6])) and torch.equal(got[7], _arange_like(got[7]))
    assert got[6].shape == (Z, len(joints), shape[0]) and got[7].shape == (Z, len(joints), shape[1]) and got[6].dtype == torch.int32
    assert _same(got, _run((a, b, ma, None, jl, G0, mv), sweeps))                   # ma alone: b at its full size
    assert _same(got, _run((a, b, None, mb, jl, G0, mv), sweeps))
    assert _same(got, _run(args, sweeps, counts=False))                             # return_kept alone: every row kept
    assert _same(plain, _run(args, sweeps, kept=False))                             # counts without the kept rows
    assert _same(got, _run((a, b, ma.cpu(), mb.cpu(), jl, G0, mv), sweeps))         # host counts: checked and uploaded


def test_full_counts_where_the_lds_image_passes_64_kb(dev):
    """K = 64 pieces in a chain, J = K (K - 1) rows of which 63 are used, ka = kb = 1024: 68.3 KB of LDS, above what a kernel
    may ask for by default (today's kernel needs 56.3 KB there).  One sweep, one puzzle."""
    K, k = 64, 1024
    rng = np.random.default_rng(86000)
    P = jr.puzzle(rng, K, [(p, p + 1) for p in range(K - 1)], k)
    J = K * (K - 1)
    jl = torch.full((1, J, 2), -1, dtype=torch.int32)
    jl[0, :K - 1] = torch.tensor(P.joints, dtype=torch.int32)
    a = torch.zeros(J, k, 3)
    b = torch.zeros(J, k, 3)
    a[:K - 1], b[:K - 1] = torch.from_numpy(np.stack(P.A)), torch.from_numpy(np.stack(P.B))
    full = torch.full((1, J), k, dtype=torch.int32)
    args = _to((a, b, full, full.clone(), jl, torch.from_numpy(P.G0)[None], torch.from_numpy(P.movable.astype(np.uint8))[None]), dev)
    plain = _run(args, 1, counts=False, kept=False)
    got = _run(args, 1)
    assert _same(plain, got[:6]) and int(got[5].sum()) > 0
    for kept in got[6:]:
        assert torch.equal(kept[0, :K - 1], _arange_like(kept[0, :K - 1])) and int((kept[0, K - 1:] != -1).sum()) == 0


# ---------------------------------------------------------------------------------------------- (2)

def _lattice_cases(graph, shape):
    ka, kb = shape
    K, joints = jr.GRAPHS[graph]
    rng = np.random.default_rng(87000 + 100 * jm.GRAPHS.index(graph) + ka)
    side = 4 if ka < 100 else 5
    out = []
    for z in range(LATTICE_SHAPES[shape]):
        counts = [(int(rng.choice([1, ka - 1, ka])), int(rng.choice([1, kb - 1, kb]))) for _ in joints]
        if z == 0:
            counts[0] = (1, kb)                      # each of m = 1, k - 1, k on either side at least once
        if z == 1:
            counts[-1] = (ka - 1, 1)
        if z == 2:
            counts[0] = (ka, kb - 1)
        out.append(jm.lattice_puzzle(rng, K, joints, shape, counts, side=side))
    return out


@pytest.mark.parametrize("shape", list(LATTICE_SHAPES), ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("graph", jm.GRAPHS)
def test_exact_kept_sets_on_the_integer_lattice(dev, graph, shape):
    ka, kb = shape
    cases = _lattice_cases(graph, shape)
    J = len(cases[0].joints)
    G, score, score0, js, used, acc, kept_a, kept_b = _host(_run(_to(jm.stack(cases), dev), 0))
    assert np.array_equal(G, np.stack([P.G0 for P in cases])) and np.array_equal(score, score0) and not used.any() and not acc.any()
    tied = 0
    for z, P in enumerate(cases):
        g = jr.f32(P.G0)
        for e in range(J):
            o = jt.joint_energy(P, g, e)
            D = jr._D(P, g, e)
            tied += len(D.min(axis=1)) - len(set(D.min(axis=1).tolist()))
            for got, want, m, k in ((kept_a[z, e], o.kept_a, P.ma[e], ka), (kept_b[z, e], o.kept_b, P.mb[e], kb)):
                assert got[:m].tolist() == want.tolist() and (got[m:] == -1).all() and got.shape == (k,), (z, e, m)
            # the kept minima are small integers and their float32 sums exact: two rounded quotients and their rounded sum
            assert abs(float(js[z, e]) - o.E) <= 3 * U32 * o.E, (z, e, float(js[z, e]), o.E)
        assert _seq32(js[z]) == score[z]
    assert tied > 0                                                                    # the minima do tie


@pytest.mark.parametrize("shape", [(5, 5), (160, 130)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("graph", jm.GRAPHS)
def test_a_count_of_zero_or_above_k_skips_the_row(dev, graph, shape):
    from puzzlenet_amd import _lib
    ka, kb = shape
    cases = _lattice_cases(graph, shape)[:4]
    args = _to(jm.stack(cases), dev)
    a, b, ma, mb, jl, G0, mv = args
    J = jl.shape[1]
    for e, (side, bad) in zip((0, J - 1, J // 2, 0), ((2, 0), (2, ka + 1), (3, 0), (3, kb + 1))):
        holed = list(args)
        holed[side] = args[side].clone()
        holed[side][:, e] = bad
        got = _run(holed, 2)
        off = jl.clone()
        off[:, e] = -1
        want = _run((a, b, ma, mb, off, G0, mv), 2)                                    # the row switched off by its (i, j)
        assert _same(got, want), (e, side, bad)
        assert int((got[3][:, e] != 0).sum()) == 0 and int((got[6][:, e] != -1).sum()) == 0 and int((got[7][:, e] != -1).sum()) == 0
        if J > 1:
            assert bool((got[6][:, [x for x in range(J) if x != e]][..., 0] >= 0).all())
        host = list(holed)
        host[side] = holed[side].cpu()                                                 # the caller's host copy: refused
        with pytest.raises(_lib.PznError) as info:
            _run(host, 2)
        assert not isinstance(info.value, _lib.PznUnsupported)


# ---------------------------------------------------------------------------------------------- (3)

@pytest.fixture(scope="module")
def visit_errors(dev):
    """One visit of piece 1 over tests/_joint_trim.visit_cases -> {graph: [(yardstick error, kernel error, entered)]}.
    Asserted here: for EVERY case, entered or not, every other piece keeps G0's bits, score <= score0, piece 1 is visited once
    at most and keeps G0's bits if its candidate was left, its rotation is orthonormal; for an entered case the candidate is
    taken, the rows kept under the returned poses are the statement's, and every E_e lies inside the trimmed interval."""
    out = {}
    for graph in jm.VISIT_GRAPHS:
        cases = jm.visit_cases(graph)
        args = _to(jm.stack(cases), dev)
        G, score, score0, js, used, acc, kept_a, kept_b = _host(_run(args, 1))
        G0 = args[5].cpu().numpy()
        assert np.isfinite(G).all() and np.array_equal(np.delete(G, 1, axis=1), np.delete(G0, 1, axis=1))
        assert (np.delete(acc, 1, axis=1) == 0).all() and (score <= score0).all()
        assert ((acc[:, 1] == 0) | (acc[:, 1] == 1)).all() and (used == acc[:, 1]).all()
        assert np.array_equal(G[acc[:, 1] == 0, 1], G0[acc[:, 1] == 0, 1]) and (score[used == 0] == score0[used == 0]).all()
        R = G[:, 1, :3, :3].astype(np.float64)
        assert np.abs(np.swapaxes(R, 1, 2) @ R - np.eye(3)).max() <= ORTHO_TOL and (np.linalg.det(R) > 0).all()
        rows = []
        for z, P in enumerate(cases):
            want, yard, entered, gap, kept = jm.visit_row(P)
            if entered:
                assert acc[z, 1] == 1 and used[z] == 1, (graph, z)
                for e, (wa, wb) in kept.items():
                    assert kept_a[z, e, :P.ma[e]].tolist() == wa.tolist() and (kept_a[z, e, P.ma[e]:] == -1).all(), (graph, z, e)
                    assert kept_b[z, e, :P.mb[e]].tolist() == wb.tolist() and (kept_b[z, e, P.mb[e]:] == -1).all(), (graph, z, e)
                iv = jt.joint_intervals(P, jr.f32(G[z]))
                for e in range(len(P.joints)):
                    assert iv[e, 0] <= float(js[z, e]) <= iv[e, 1], (graph, z, e, iv[e], float(js[z, e]))
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
        assert len(rows) - len(ent) == jm.VISIT[graph] and 4 * len(ent) >= 3 * len(rows), graph
        for n, (_, k, e) in enumerate(rows):
            if e:
                assert k <= tol, (graph, n, k, tol)


# ---------------------------------------------------------------------------------------------- (4), (5)

@pytest.mark.parametrize("graph", jm.GRAPHS)
def test_short_trajectory_follows_the_float64_statement(visit_errors, dev, graph):
    cases = jm.trajectory_cases(graph)
    args = _to(jm.stack(cases), dev)
    full = _run(args, jm.TRAJECTORY_SWEEPS)
    G, score, score0, js, used, acc, kept_a, kept_b = _host(full)
    G0 = args[5].cpu().numpy()
    tol = _tolerance(visit_errors)
    assert np.isfinite(G).all() and (score <= score0).all() and np.array_equal(G[:, 0], G0[:, 0]) and (acc[:, 0] == 0).all()
    left_out, worst = 0, 0.0
    for z, P in enumerate(cases):
        want, entered = jm.trajectory_row(P)
        assert _seq32(js[z]) == score[z]
        if not entered:
            left_out += 1
            continue
        assert acc[z].tolist() == want.accepted.tolist() and int(used[z]) == want.sweeps_used, (z, acc[z], want.accepted)
        for e in range(len(P.joints)):
            assert kept_a[z, e, :P.ma[e]].tolist() == want.kept_a[e].tolist() and (kept_a[z, e, P.ma[e]:] == -1).all(), (z, e)
            assert kept_b[z, e, :P.mb[e]].tolist() == want.kept_b[e].tolist() and (kept_b[z, e, P.mb[e]:] == -1).all(), (z, e)
        iv = jt.joint_intervals(P, jr.f32(G[z]))
        for e in range(len(P.joints)):
            assert iv[e, 0] <= float(js[z, e]) <= iv[e, 1], (z, e, iv[e], float(js[z, e]))
        err = max(ref.pose_err(G[z, p], want.G[p]) for p in range(P.K))
        worst = max(worst, err)
        assert err <= tol, (z, err, tol)
    print(f"{graph}: left out {left_out} of {len(cases)}, largest pose difference {worst:.3e} (tolerance {tol:.3e})")
    assert left_out == jm.TRAJECTORY[graph] and 4 * left_out <= len(cases), left_out
    # two launches: the same bits; a puzzle alone at Z = 1: its bits of the batch
    assert _same(full, _run(args, jm.TRAJECTORY_SWEEPS))
    a, b, ma, mb, jl, G0d, mv = args
    J = jl.shape[1]
    for z in (0, len(cases) // 2, len(cases) - 1):
        s = slice(z * J, (z + 1) * J)
        alone = _run((a[s], b[s], ma[z:z + 1], mb[z:z + 1], jl[z:z + 1], G0d[z:z + 1], mv[z:z + 1]), jm.TRAJECTORY_SWEEPS)
        assert all(torch.equal(x[z:z + 1], y) for x, y in zip(full, alone)), z
    # the counts travel with the rows, the sets through the maps
    perm = torch.from_numpy(np.random.default_rng(3).permutation(len(cases) * J)).to(dev)
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(len(cases) * J, device=dev)
    mapped = _run((a[perm].contiguous(), b.flip(0).contiguous(), ma, mb, jl, G0d, mv), jm.TRAJECTORY_SWEEPS, a_of=inv.reshape(-1, J),
                  b_of=torch.arange(len(cases) * J - 1, -1, -1, device=dev).reshape(-1, J))
    assert _same(full, mapped)


# ---------------------------------------------------------------------------------------------- (6)

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
    go = lambda **k: ops.joint_refine(pts, pts, k.pop("jl", jl), eye, mv, 3, **k)
    for bad in (lambda: go(ma=m8.long()),                                         # a wrong dtype: no silent conversion
                lambda: go(mb=m8.float()),
                lambda: go(ma=m8.reshape(2)),                                     # per set instead of per joint row [Z,J]
                lambda: go(mb=m8[:, :1]),
                lambda: go(ma=[[8, 8]]),                                          # no tensor
                lambda: go(ma=torch.full((1, 2), 8, dtype=torch.int32, device="meta")),
                lambda: go(ma=torch.tensor([[8, 9]], dtype=torch.int32)),         # host copies are range-checked
                lambda: go(mb=torch.tensor([[0, 8]], dtype=torch.int32)),
                lambda: go(ma=m8, na=n8),                                         # counts per row with counts per set
                lambda: go(mb=m8, nb=n8),
                lambda: go(na=n8, return_kept=True)):
        with pytest.raises(_lib.PznError) as info:
            bad()
        assert not isinstance(info.value, _lib.PznUnsupported)
    assert calls == []
    # what is accepted goes to the new entry point, and without counts to the old ones
    go(ma=m8)
    go(mb=torch.tensor([[1, 8]], dtype=torch.int32))
    go(return_kept=True)
    # a host count on an unused row of the caller's host list is not held to the range
    go(jl=torch.tensor([[[0, 1], [-1, -1]]], dtype=torch.int32), ma=torch.tensor([[8, 0]], dtype=torch.int32))
    go()
    go(na=n8)
    assert calls == ["pzn_joint_refine_trim_f32"] * 4 + ["pzn_joint_refine_f32", "pzn_joint_refine_counts_f32"]
    # no puzzles, or no joints: still a success that launches nothing
    out = ops.joint_refine(pts[:0], pts[:0], jl[:, :0], eye, mv, 3, ma=m8[:, :0], mb=m8[:, :0], return_kept=True)
    assert torch.equal(out[0], eye) and out[3].shape == (1, 0) and out[6].shape == (1, 0, 8) and len(calls) == 6
