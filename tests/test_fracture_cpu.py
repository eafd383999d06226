"""CPU: the numpy statement of the fracture kernel (datapipe.fracture_rule) held to its own promises on the shapes the GPU test
compares the kernel on, and the score of an assembly (assembly.truth_table, assembly.evaluate) on planted errors."""
import numpy as np
import pytest
import torch

from tests import _fracture as fr

# samples per shape: enough that both outcomes (every step valid / a step without a valid candidate) occur where they should;
# the seed is fixed, so the outcome is too
SAMPLES = {1000: 8, 1025: 8, 4096: 6, 10000: 4, 32768: 2, 65536: 2, 333: 32, 2048: 16}


def _run(shape, seed):
    from puzzlenet_amd import datapipe
    M, P, K, n_min = shape
    B = SAMPLES[M]
    raw = fr.clouds(B, M, seed)
    normals, u_anchor, u_start, _ = fr.draws(B, P, K, seed + 1)
    recs = [datapipe.fracture_rule(raw[b], normals[b], u_anchor[b], u_start[b], P, n_min, M) for b in range(B)]
    for b, r in enumerate(recs):
        fr.check_invariants(raw[b], normals[b], u_anchor[b], u_start[b], n_min, M, r)
    return recs


@pytest.mark.parametrize("shape", fr.OK_SHAPES, ids=str)
def test_rule_invariants_where_cuts_are_valid(shape):
    recs = _run(shape, 100 + shape[0] % 97)
    n_ok = sum(r["ok"] for r in recs)
    print(shape, "ok", n_ok, "of", len(recs), "smallest piece", min(int(r["counts"].min()) for r in recs))
    assert 2 * n_ok >= len(recs)                                   # the valid path is in the comparison
    assert all(r["counts"].min() >= shape[3] for r in recs if r["ok"])


@pytest.mark.parametrize("shape", fr.NOT_OK_SHAPES, ids=str)
def test_rule_invariants_where_some_cuts_are_not(shape):
    recs = _run(shape, 200 + shape[0] % 97)
    n_ok = sum(r["ok"] for r in recs)
    print(shape, "ok", n_ok, "of", len(recs))
    assert n_ok < len(recs)                                        # the most-balanced path is in the comparison


def test_rule_cap_truncates_and_clears_ok():
    from puzzlenet_amd import datapipe
    M, P, K = 4096, 2, 8
    raw = fr.clouds(1, M, 5)[0]
    normals, u_anchor, u_start, _ = (t[0] for t in fr.draws(1, P, K, 6))
    full = datapipe.fracture_rule(raw, normals, u_anchor, u_start, P, 128, M)
    cut = datapipe.fracture_rule(raw, normals, u_anchor, u_start, P, 128, 1500)
    assert full["ok"] and full["counts"].max() > 1500 and not cut["ok"]
    fr.check_invariants(raw, normals, u_anchor, u_start, 128, 1500, cut)
    assert np.array_equal(cut["label"], full["label"]) and np.array_equal(cut["counts"], full["counts"])


def test_rule_duplicates_and_a_repeated_anchor():
    """Coincident points evaluate alike, so they stay together; a point repeated through the whole target is its own anchor."""
    from puzzlenet_amd import datapipe
    M, P, K = 600, 4, 3
    raw = fr.clouds(1, M, 9)[0]
    raw[1::2] = raw[0::2]                                          # every point twice
    normals, u_anchor, u_start, _ = (t[0] for t in fr.draws(1, P, K, 10))
    r = datapipe.fracture_rule(raw, normals, u_anchor, u_start, P, 20, M)
    fr.check_invariants(raw, normals, u_anchor, u_start, 20, M, r)
    assert np.array_equal(r["label"][0::2], r["label"][1::2])
    same = np.repeat(raw[:1], 64, axis=0)                          # one point 64 times: every candidate leaves all of it up
    r = datapipe.fracture_rule(same, normals, u_anchor, u_start, P, 1, 64)
    fr.check_invariants(same, normals, u_anchor, u_start, 1, 64, r)
    assert not r["ok"] and r["counts"].tolist() == [64, 0, 0, 0] and not r["cand"].any()


def test_draw_fracture_batch_layout():
    from puzzlenet_amd import datapipe
    B, P, K = 3, 5, 4
    normals, u_anchor, u_start, twist = fr.draws(B, P, K, 3)
    assert normals.shape == (B, P - 1, K, 3) and u_anchor.shape == (B, P - 1, K) and u_start.shape == (B, P)
    assert twist.shape == (B, P, 6)
    assert np.allclose(np.linalg.norm(normals, axis=-1), 1.0, atol=1e-15)
    assert np.allclose(np.linalg.norm(twist, axis=-1), 0.8, atol=1e-12)
    assert (0 <= u_anchor).all() and (u_anchor < 1).all() and (0 <= u_start).all() and (u_start < 1).all()
    again = fr.draws(B, P, K, 3)
    assert all(np.array_equal(a, b) for a, b in zip((normals, u_anchor, u_start, twist), again))      # a seed means one batch
    width = datapipe._fracture_cols(P, K)[-1].stop
    assert width == 3 * (P - 1) * K + (P - 1) * K + P + 6 * P


# --------------------------------------------------------------------------- the score

def _rot(axis, deg):
    axis = np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    th = np.radians(deg)
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def _poses(P, seed):
    rng = np.random.RandomState(seed)
    out = np.tile(np.eye(4), (P, 1, 1))
    for p in range(P):
        out[p, :3, :3] = _rot(rng.randn(3), rng.uniform(-170, 170))
        out[p, :3, 3] = rng.randn(3)
    return out


def _inv(T):
    out = np.eye(4)
    out[:3, :3], out[:3, 3] = T[:3, :3].T, -T[:3, :3].T @ T[:3, 3]
    return out


def _truth(pose, root):
    return np.stack([pose[root] @ _inv(pose[p]) for p in range(len(pose))])


def _sample(P=5, n=64, seed=0):
    rng = np.random.RandomState(seed)
    return _poses(P, seed + 1), rng.rand(P, n, 3) - 0.5


def test_truth_table_pairs_are_inverse_and_assemble_to_the_truth():
    from puzzlenet_amd import assembly
    pose, rest = _sample()
    P = len(pose)
    mates = np.zeros((P, P), dtype=bool)
    for i, j in ((0, 3), (3, 1), (1, 4), (2, 4)):                  # a connected chain, hand made
        mates[i, j] = mates[j, i] = True
    cd = np.random.RandomState(3).rand(P, P) * 0.01
    cd = cd + cd.T
    T, S = assembly.truth_table(pose, mates, cd)
    assert T.shape == (P, P, 4, 4) and S.shape == (P, P)
    for i in range(P):
        for j in range(P):
            assert np.abs(T[i, j] @ T[j, i] - np.eye(4)).max() < 1e-12
    assert np.isinf(S[~mates]).all() and np.isinf(np.diag(S)).all() and np.array_equal(S[mates], cd[mates])
    a = assembly.assemble(S, T)
    assert a.placed.all()
    ev = assembly.evaluate(a.G, a.placed, pose, rest, a.root, a.edges, mates)
    print("rot_deg", ev.rot_deg.max(), "msd", ev.msd.max())
    assert ev.rot_deg.max() < 1e-9 and ev.msd.max() < 1e-20 and ev.part_accuracy == 1.0 and ev.part_ok.all()
    assert ev.edge_precision == 1.0
    # tensors are taken as arrays are; without mates every pair is a candidate at score 0
    T2, S2 = assembly.truth_table(torch.from_numpy(pose).float())
    assert np.abs(T2 - T).max() < 1e-5 and np.array_equal(np.isinf(S2), np.eye(P, dtype=bool)) and not S2[~np.eye(P, dtype=bool)].any()


def test_evaluate_planted_rotation_and_translation():
    from puzzlenet_amd import assembly
    pose, rest = _sample(seed=4)
    P, root = len(pose), 2
    placed = np.ones(P, dtype=bool)
    rng = np.random.RandomState(8)
    for theta in (1e-6, 0.37, 45.0, 179.5):
        G = _truth(pose, root)
        E = np.eye(4)
        E[:3, :3] = _rot(rng.randn(3), theta)
        G[1] = E @ G[1]
        ev = assembly.evaluate(G, placed, pose, rest, root)
        assert abs(ev.rot_deg[1] - theta) < 1e-9, (theta, ev.rot_deg[1])
        assert np.delete(ev.rot_deg, 1).max() < 1e-9 and np.delete(ev.msd, 1).max() < 1e-20
    d = np.array([0.03, -0.04, 0.12])
    G = _truth(pose, root)
    G[4, :3, 3] += d
    ev = assembly.evaluate(G, placed, pose, rest, root)
    assert abs(ev.trans[4] - np.linalg.norm(d)) < 1e-12 and abs(ev.msd[4] - d @ d) < 1e-12 and ev.rot_deg[4] < 1e-9
    assert not ev.part_ok[4] and ev.part_ok[[0, 1, 3]].all() and ev.part_accuracy == 0.75      # |d|^2 = 0.0169 >= tol = 0.01
    assert assembly.evaluate(G, placed, pose, rest, root, tol=0.02).part_accuracy == 1.0
    assert ev.edge_precision is None


def test_evaluate_does_not_depend_on_the_root():
    from puzzlenet_amd import assembly
    pose, rest = _sample(seed=6)
    P = len(pose)
    placed = np.ones(P, dtype=bool)
    rng = np.random.RandomState(2)
    G = _truth(pose, 0)
    for p in range(1, P):                                          # an error on every piece but the root
        E = np.eye(4)
        E[:3, :3], E[:3, 3] = _rot(rng.randn(3), rng.uniform(0, 20)), 0.05 * rng.randn(3)
        G[p] = G[p] @ E
    ev0 = assembly.evaluate(G, placed, pose, rest, 0)
    new = 3
    # the same assembly in piece 3's frame: everything moved by the TRUE change of frame
    G3 = np.stack([pose[new] @ _inv(pose[0]) @ G[p] for p in range(P)])
    ev3 = assembly.evaluate(G3, placed, pose, rest, new)
    assert np.abs(ev3.rot_deg - ev0.rot_deg).max() < 1e-9 and np.abs(ev3.msd - ev0.msd).max() < 1e-12
    assert np.array_equal(ev3.part_ok, ev0.part_ok)


def test_evaluate_unplaced_pieces_and_edge_precision():
    from puzzlenet_amd import assembly
    pose, rest = _sample(seed=12)
    P, root = len(pose), 1
    G = _truth(pose, root)
    placed = np.array([True, True, False, True, False])
    ev = assembly.evaluate(G, placed, pose, rest, root)
    assert ev.msd.max() < 1e-20 and ev.part_ok.tolist() == [True, True, False, True, False]      # right, but not placed
    assert ev.part_accuracy == 0.5
    mates = np.zeros((P, P), dtype=bool)
    mates[0, 1] = mates[1, 0] = mates[1, 3] = mates[3, 1] = True
    edges = [(1, 0, 0.001, 0), (3, 1, 0.002, 3), (0, 4, 0.5, 4), (2, 4, 0.7, 2)]
    assert assembly.evaluate(G, placed, pose, rest, root, edges, mates).edge_precision == 0.5
    assert assembly.evaluate(G, placed, pose, rest, root, edges).edge_precision is None
    assert assembly.evaluate(G, placed, pose, rest, root, None, mates).edge_precision is None
    with pytest.raises(ValueError):
        assembly.evaluate(G[:3], placed, pose, rest, root)
