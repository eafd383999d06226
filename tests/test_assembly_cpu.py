"""CPU: the greedy walk of puzzlenet_amd.assembly.assemble on hand-built pair tables (float64 on the host, no GPU), and
the register allocation of the pair-head kernel (cross-compiled, read from the code-object metadata)."""
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from puzzlenet_amd import build


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


def _one_placed_end(edges, root):
    seen = {root}
    for i, j, _s, new in edges:
        assert (i in seen) != (j in seen), (i, j, seen)
        assert new == (j if i in seen else i)
        seen.add(new)
    return seen


def test_consistent_table():
    """Poses that come from one set of ground-truth frames: whatever tree the scores pick, every piece lands at
    inv(G*_root) G*_k."""
    from puzzlenet_amd.assembly import assemble
    rng = np.random.default_rng(5)
    K = 6
    Gs = np.stack([_rigid(rng) for _ in range(K)])
    T = np.stack([np.stack([_inv(Gs[i]) @ Gs[j] for j in range(K)]) for i in range(K)])
    score = rng.uniform(0.1, 1.0, (K, K))
    a = assemble(score, T)
    assert a.placed.all() and a.placed.dtype == bool
    assert len(a.edges) == K - 1
    assert _one_placed_end(a.edges, a.root) == set(range(K))
    for k in range(K):
        assert np.abs(a.G[k] - _inv(Gs[a.root]) @ Gs[k]).max() < 1e-10
    # tensors are taken as well as arrays
    import torch
    b = assemble(torch.from_numpy(score).float(), torch.from_numpy(T).float())
    assert b.root == a.root and [e[:2] for e in b.edges] == [e[:2] for e in a.edges]


def test_forced_tree():
    """Low scores only on the chain 2 - 0 - 4 - 1 - 3, its edges stored in mixed orientation; every other pose is an
    unrelated rigid motion, so G is right only if exactly the chain is walked, and the inverse branch runs where the
    unplaced piece holds the fixed role."""
    from puzzlenet_amd.assembly import assemble
    rng = np.random.default_rng(11)
    K = 5
    T = np.stack([np.stack([_rigid(rng) for _ in range(K)]) for _ in range(K)])
    score = rng.uniform(10.0, 20.0, (K, K))
    chain = [(2, 0, 0.1), (4, 0, 0.2), (4, 1, 0.3), (3, 1, 0.4)]      # (fixed, moved, score): root 2, then 0, 4, 1, 3
    for i, j, s in chain:
        score[i, j] = s
    a = assemble(score, T)
    assert a.root == 2 and a.placed.all()
    assert [(i, j) for i, j, _s, _n in a.edges] == [(i, j) for i, j, _s in chain]
    assert [s for _i, _j, s, _n in a.edges] == sorted(s for _i, _j, s in chain)
    assert [n for *_e, n in a.edges] == [0, 4, 1, 3]
    G0 = T[2, 0]                                 # fixed end placed: G[0] = G[2] T[2,0]
    G4 = G0 @ _inv(T[4, 0])                      # moved end placed: G[4] = G[0] inv(T[4,0])
    G1 = G4 @ T[4, 1]
    G3 = G1 @ _inv(T[3, 1])
    for k, g in ((2, np.eye(4)), (0, G0), (4, G4), (1, G1), (3, G3)):
        assert np.abs(a.G[k] - g).max() < 1e-12, k


def test_ties_and_threshold():
    from puzzlenet_amd.assembly import assemble
    rng = np.random.default_rng(3)
    K = 4
    T = np.stack([np.stack([_rigid(rng) for _ in range(K)]) for _ in range(K)])
    # every score equal: the first row-major off-diagonal pair is (0, 1), then (0, 2), (0, 3)
    a = assemble(np.ones((K, K)), T)
    assert a.root == 0 and [(i, j) for i, j, *_ in a.edges] == [(0, 1), (0, 2), (0, 3)]
    # two components {0, 1} and {2, 3}, every bridge at 5.0
    score = np.full((K, K), 5.0)
    score[1, 0] = 0.5
    score[0, 1] = 0.5          # a tie with (1, 0): the first row-major position is (0, 1)
    score[2, 3] = 0.7
    cut = assemble(score, T, max_score=1.0)
    assert cut.root == 0 and [(i, j) for i, j, *_ in cut.edges] == [(0, 1)]
    assert cut.placed.tolist() == [True, True, False, False]
    assert np.array_equal(cut.G[2], np.eye(4)) and np.array_equal(cut.G[3], np.eye(4))
    assert np.abs(cut.G[1] - T[0, 1]).max() < 1e-12
    full = assemble(score, T)
    assert full.placed.all() and [(i, j) for i, j, *_ in full.edges] == [(0, 1), (0, 2), (2, 3)]


def test_pair_head_kernel_does_not_spill():
    """pair_head_fwd_kernel keeps the first-layer result of a tile, the working tiles of the chain and the prefetched rows
    in registers across its loop over the moved pieces: no spilled register, no scratch."""
    flags = [f for f in build.COMMON if f not in ("-fPIC", "-fvisibility=hidden")]
    extra = dict(build.SOURCES)["pointmlp.hip"]
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "pointmlp.s")
        cmd = [build.hipcc()] + flags + extra + ["-S", "--cuda-device-only", "-o", out, os.path.join(build.CSRC, "pointmlp.hip")]
        assert subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL).returncode == 0
        text = open(out).read()
    meta = text[text.index("amdhsa.kernels:"):]
    entries = [e for e in re.split(r"\n  - ", meta)[1:] if "pair_head_fwd_kernel" in (re.search(r"\.name:\s+(\S+)", e) or [""])[0]]
    assert len(entries) == 1
    spills = int(re.search(r"\.vgpr_spill_count:\s+(\d+)", entries[0]).group(1))
    scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", entries[0]).group(1))
    assert spills == 0 and scratch == 0, f"{spills} spilled registers, {scratch} bytes of scratch per lane"
