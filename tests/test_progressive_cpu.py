"""CPU: the host bookkeeping of progressive assembly (puzzlenet_amd.assembly.MergeLedger, float64, no GPU) on hand-built
rigid tables, the restatement tests/_merge_ref.py against a from-scratch numpy sampling, and the register allocation of
the merge kernel (cross-compiled, read from the code-object metadata)."""
import os
import re
import subprocess
import tempfile

import numpy as np
import torch

from puzzlenet_amd import build
from tests import _merge_ref


def _rigid(rng):
    q, r = np.linalg.qr(rng.standard_normal((3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    g = np.eye(4)
    g[:3, :3] = q
    g[:3, 3] = rng.standard_normal(3)
    return g


def _inv(g):
    out = np.eye(4)
    out[:3, :3] = g[:3, :3].T
    out[:3, 3] = -g[:3, :3].T @ g[:3, 3]
    return out


def _walk(score, T, max_score=None):
    """The progressive rounds on a hand-built table: the merged part keeps the fixed part's row and column (it lives in
    that part's frame), the moved part's row and column leave."""
    from puzzlenet_amd.assembly import MergeLedger, _choose
    S, P = np.array(score, dtype=np.float64), np.array(T, dtype=np.float64)
    led = MergeLedger(S.shape[0])
    while S.shape[0] > 1:
        pick = _choose(S, max_score)
        if pick is None:
            break
        i, j, s = pick
        n = led.merge(i, j, P[i, j], s)
        assert n == (i if i < j else i - 1)
        S = np.delete(np.delete(S, j, 0), j, 1)
        P = np.delete(np.delete(P, j, 0), j, 1)
    return led


def test_ledger_on_a_consistent_table_ends_where_assemble_does():
    """The consistent-table case of test_assembly_cpu.py: every piece lands at inv(G*_f) G*_k, f the piece whose frame its
    part lives in; re-rooted at assemble's root, that is assemble's G."""
    from puzzlenet_amd.assembly import assemble
    rng = np.random.default_rng(5)
    K = 6
    Gs = np.stack([_rigid(rng) for _ in range(K)])
    T = np.stack([np.stack([_inv(Gs[i]) @ Gs[j] for j in range(K)]) for i in range(K)])
    score = rng.uniform(0.1, 1.0, (K, K))
    led = _walk(score, T)
    assert len(led.members) == 1 and sorted(led.members[0]) == list(range(K)) and len(led.edges) == K - 1
    assert led.G.dtype == np.float64 and led.label(0) == 0
    f = led.frame[0]
    assert np.array_equal(led.G[f], np.eye(4))
    for k in range(K):
        assert np.abs(led.G[k] - _inv(Gs[f]) @ Gs[k]).max() < 1e-10
    a = assemble(score, T)
    assert led.edges[0][:2] == (a.edges[0][0], a.edges[0][1])      # the same first pair: the smallest score
    for k in range(K):
        assert np.abs(_inv(led.G[a.root]) @ led.G[k] - a.G[k]).max() < 1e-10


def test_ledger_composition_members_and_labels():
    """Two merges by hand: 3 joins 1 (fixed 1), then that part joins 2 as the MOVED side: every member's pose is
    composed from the left, labels are the lowest member, later parts move down one place."""
    from puzzlenet_amd.assembly import MergeLedger
    rng = np.random.default_rng(7)
    A, B = _rigid(rng), _rigid(rng)
    led = MergeLedger(4)
    n = led.merge(1, 3, A, 0.25, "da", "db")
    assert n == 1 and led.members == [[0], [1, 3], [2]] and led.frame == [0, 1, 2]
    assert led.edges == [(1, 3, 0.25, "da", "db")]
    assert np.array_equal(led.G[3], A) and np.array_equal(led.G[1], np.eye(4))
    n = led.merge(2, 1, B, 0.5)                      # parts: 0 = {0}, 1 = {1, 3}, 2 = {2}
    assert n == 1 and led.members == [[0], [2, 1, 3]] and led.frame == [0, 2]
    assert led.edges[1] == (2, 1, 0.5, None, None) and led.label(1) == 1
    assert np.abs(led.G[1] - B).max() == 0 and np.abs(led.G[3] - B @ A).max() < 1e-15
    assert np.array_equal(led.G[0], np.eye(4)) and np.array_equal(led.G[2], np.eye(4))


def test_walk_stops_at_max_score():
    rng = np.random.default_rng(3)
    K = 4
    T = np.stack([np.stack([_rigid(rng) for _ in range(K)]) for _ in range(K)])
    score = np.full((K, K), 5.0)
    score[1, 0] = 0.5
    led = _walk(score, T, max_score=1.0)
    assert led.members == [[1, 0], [2], [3]] and led.frame == [1, 2, 3]
    assert [e[:3] for e in led.edges] == [(1, 0, 0.5)]
    none = _walk(score, T, max_score=0.1)
    assert none.edges == [] and none.members == [[0], [1], [2], [3]]
    assert np.array_equal(none.G, np.tile(np.eye(4), (K, 1, 1)))


def _numpy_merge(a, b, T, start, n_out, drop_a, drop_b):
    """From scratch, one float32 scalar operation at a time."""
    f = np.float32
    rows = [tuple(f(v) for v in r) for r in a]
    for x, y, z in b:
        x, y, z = f(x), f(y), f(z)
        rows.append(tuple(f(f(f(f(T[r][0] * x) + f(T[r][1] * y)) + f(T[r][2] * z)) + T[r][3]) for r in range(3)))
    U = len(rows)
    dropped = [False] * U
    for r in drop_a:
        dropped[int(r)] = True
    for r in drop_b:
        dropped[len(a) + int(r)] = True
    dist = [f(0.0) if d else f(1e10) for d in dropped]
    far = int(start)
    if dropped[far]:
        far = next((far + o) % U for o in range(U) if not dropped[(far + o) % U])
    src = []
    for _ in range(n_out):
        src.append(far)
        c = rows[far]
        best, arg = None, 0
        for u, p in enumerate(rows):
            dx, dy, dz = f(p[0] - c[0]), f(p[1] - c[1]), f(p[2] - c[2])
            d = f(f(f(dx * dx) + f(dy * dy)) + f(dz * dz))
            dist[u] = min(dist[u], d)
            if best is None or dist[u] > best:      # strict: the lowest index of equal distances stays
                best, arg = dist[u], u
        far = arg
    return np.array([rows[s] for s in src], dtype=np.float32), np.array(src, dtype=np.int64)


def test_merge_ref_against_numpy_on_a_small_union():
    g = torch.Generator().manual_seed(9)
    a, b = torch.rand(1, 12, 3, generator=g), torch.rand(1, 20, 3, generator=g)
    T = torch.from_numpy(_rigid(np.random.default_rng(9))).float()[None]
    drop_a, drop_b = torch.tensor([[3, 3, 0]]), torch.tensor([[19, 1, 7, 8]])
    for start, da, db in ((15, None, None), (3, drop_a, drop_b), (31, drop_a, drop_b)):      # 31 = b row 19: wraps to a row 1
        pts, src = _merge_ref.merge_resample(a, b, T, torch.tensor([start]), 16, da, db)
        want_p, want_s = _numpy_merge(a[0].numpy(), b[0].numpy(), T[0].numpy(), start, 16,
                                      [] if da is None else da[0].tolist(), [] if db is None else db[0].tolist())
        assert np.array_equal(src[0].numpy(), want_s), start
        assert np.array_equal(pts[0].numpy(), want_p), start
        if da is not None:
            assert not set(src[0].tolist()) & ({0, 3} | {12 + r for r in (19, 1, 7, 8)})
    assert int(_merge_ref.merge_resample(a, b, T, torch.tensor([31]), 16, drop_a, drop_b)[1][0, 0]) == 1


def test_merge_kernel_does_not_spill():
    """merge_resample_kernel keeps up to 16 rows and their running distances per thread in registers for all rounds: no
    spilled register, no scratch, in any of its instantiations."""
    flags = [f for f in build.COMMON if f not in ("-fPIC", "-fvisibility=hidden")]
    extra = dict(build.SOURCES)["mergefps.hip"]
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "mergefps.s")
        cmd = [build.hipcc()] + flags + extra + ["-S", "--cuda-device-only", "-o", out, os.path.join(build.CSRC, "mergefps.hip")]
        assert subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL).returncode == 0
        text = open(out).read()
    meta = text[text.index("amdhsa.kernels:"):]
    entries = [e for e in re.split(r"\n  - ", meta)[1:] if "merge_resample_kernel" in (re.search(r"\.name:\s+(\S+)", e) or [""])[0]]
    assert len(entries) == 5
    for e in entries:
        spills = int(re.search(r"\.vgpr_spill_count:\s+(\d+)", e).group(1))
        sspills = int(re.search(r"\.sgpr_spill_count:\s+(\d+)", e).group(1))
        scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", e).group(1))
        assert spills == 0 and sspills == 0 and scratch == 0, f"{spills} + {sspills} spilled registers, {scratch} bytes of scratch per lane"
