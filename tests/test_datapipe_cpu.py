"""Data-pipeline fixtures against the CPU oracle: the reference's numpy FPS (dataset.py:1147-1163:
float64 `distance` array holding float32 values, first maximum) must be what the fp32 oracle FPS computes on the cut
pieces, draw for draw — that is what lets the GPU pipeline run `pzn_fps_f32` on them."""
import numpy as np
import pytest

from oracle import point_ops as orc


def _pieces(G, c):
    raw = G[f"c{c}_raw"]
    dis = raw.astype(np.float64) @ G[f"c{c}_normal"].reshape(3, 1) + G[f"c{c}_z"]
    up = raw[(dis >= 0)[:, 0]]
    down = raw[(dis < 0)[:, 0]]
    return up, down


def test_cut_sizes_match_the_reference(golden_data):
    G = golden_data
    for c in range(int(G["cases"])):
        up, down = _pieces(G, c)
        assert up.shape[0] == int(G[f"c{c}_n_up"]) and down.shape[0] == int(G[f"c{c}_n_down"])


def test_oracle_fps_reproduces_dataset_fps(golden_data):
    G = golden_data
    n = int(G["N"])
    for c in range(int(G["cases"])):
        up, down = _pieces(G, c)
        for piece, start, want in ((up, G[f"c{c}_s_up"], G[f"c{c}_up"]), (down, G[f"c{c}_s_down"], G[f"c{c}_down"])):
            idx = orc.farthest_point_sample(piece[None], n, np.array([int(start)], np.int64))[0]
            assert np.array_equal(piece[idx], want)          # same points in the same selection order, bit for bit
        # padding a piece with copies of its first point (what the GPU pipeline does) changes nothing
        pad = np.concatenate([down, np.repeat(down[:1], 777, 0)], 0)
        idx = orc.farthest_point_sample(pad[None], n, np.array([int(G[f"c{c}_s_down"])], np.int64))[0]
        assert np.array_equal(pad[idx], G[f"c{c}_down"])


def test_boundary_fixture_is_consistent(golden_data):
    G = golden_data
    for c in range(int(G["cases"])):
        assert int(G[f"c{c}_fpc_idx"].sum()) == 128 and int(G[f"c{c}_rpc_idx"].sum()) == 128
        # the masks mark exactly the 128 smallest chamfer distances of each piece
        for cd, mask in ((G[f"c{c}_cd_over_down"], G[f"c{c}_fpc_idx"]), (G[f"c{c}_cd_over_up"], G[f"c{c}_rpc_idx"])):
            assert cd[mask > 0].max() <= np.sort(cd)[128] + 1e-12


def test_draws_follow_the_reference_order(golden_data):
    """datapipe.draws_like_reference consumes numpy's / torch's global generators exactly as the reference's
    plane_split -> fps(up) -> fps(down) -> RandomTransformSE3 sequence does (seeds of make_golden_data.py)."""
    import torch
    from puzzlenet_amd import datapipe
    G = golden_data
    for c in range(int(G["cases"])):
        np.random.seed(1000 + c)
        torch.manual_seed(7000 + c)
        d = datapipe.draws_like_reference(G[f"c{c}_raw"], n=int(G["N"]), mag=0.8)
        assert np.array_equal(d["normal"], G[f"c{c}_normal"]) and np.array_equal(d["z"], G[f"c{c}_z"])
        assert d["s_up"] == int(G[f"c{c}_s_up"]) and d["s_down"] == int(G[f"c{c}_s_down"])
        assert np.array_equal(d["twist"], G[f"c{c}_twist"])


def _region_points(raw, rec, tab):
    s1 = (np.dot(raw, np.asarray(rec["normal1"]).reshape(3, 1)) + rec["z1"] >= 0).reshape(-1)
    s2 = (np.dot(raw, np.asarray(rec["normal2"]).reshape(3, 1)) + rec["z2"] >= 0).reshape(-1)
    code = 2 * s1.astype(np.int64) + s2.astype(np.int64)
    return np.vstack([raw[((int(t) >> code) & 1) == 1] for t in tab if int(t)])


def _oracle_accept(raw):
    """chamfer distance of the two 128-point boundaries of a candidate pair, with the oracle's FPS and chamfer
    (dataset.py:1250-1253: the pair is kept when this is <= 0.015)."""
    def accept(rec):
        U = _region_points(raw, rec, rec["u_tab"])
        D = _region_points(raw, rec, rec["d_tab"])
        U = U[orc.farthest_point_sample(U[None], 1024, np.array([rec["s_u"]], np.int64))[0]]
        D = D[orc.farthest_point_sample(D[None], 1024, np.array([rec["s_d"]], np.int64))[0]]
        over_u, _, over_d, _ = orc.chamfer(D[None], U[None])          # min over D per U-point, min over U per D-point
        ub = U[np.argsort(over_u[0], kind="stable")[:128]]
        db = D[np.argsort(over_d[0], kind="stable")[:128]]
        c1, _, c2, _ = orc.chamfer(db[None], ub[None])
        return float(c1.mean() + c2.mean())
    return accept


def test_double_cut_planner_follows_the_reference(golden_data2):
    """datapipe.plan_double_cut_like_reference, seeded as make_golden_data2.py seeded the reference's
    MovedCADDataset2(CADDataset(split_twice=True)).__getitem__, takes the same branch and makes the same draws: one case
    per kind of pair (single cut, half vs rest, half vs the other piece, the two halves; upper and lower piece; and a
    candidate the reference rejected).  The pieces the recipe names, sampled by the oracle FPS, are the reference's."""
    import torch
    from puzzlenet_amd import datapipe
    from tests.conftest import golden_cloud
    G = golden_data2
    kinds = set()
    for seed in G["seeds"].tolist():
        raw = golden_cloud(seed, G["M"])
        k = f"s{seed}_"
        np.random.seed(3000 + seed)
        torch.manual_seed(9000 + seed)
        rec = datapipe.plan_double_cut_like_reference(raw, _oracle_accept(raw), n=int(G["N"]), mag=0.8)
        for name in ("normal1", "z1", "normal2", "z2", "u_tab", "d_tab", "twist"):
            assert np.array_equal(np.asarray(rec[name]), G[k + name]), (seed, name)
        assert rec["s_u"] == int(G[k + "s_u"]) and rec["s_d"] == int(G[k + "s_d"])
        U = _region_points(raw, rec, rec["u_tab"])
        D = _region_points(raw, rec, rec["d_tab"])
        assert np.array_equal(U[orc.farthest_point_sample(U[None], 1024, np.array([rec["s_u"]], np.int64))[0]], G[k + "up"])
        assert np.array_equal(D[orc.farthest_point_sample(D[None], 1024, np.array([rec["s_d"]], np.int64))[0]], G[k + "down"])
        kinds.add(str(G[k + "kind"]))
    assert {"single", "single_after_rejection", "half_vs_rest", "half_vs_rest_lower", "half_vs_other", "half_vs_other_lower",
            "halves", "halves_lower"} <= kinds


def test_solid_cut_masks_against_the_restated_meshes():
    """datapipe.solid_cut_mask (the reference's sphere / cylinder / cone cuts, dataset.py:716-763) against the oracle's
    restatement of what the reference computes: open3d 0.15.2's create_sphere / create_cylinder / create_cone meshes at
    resolution 50 (vertex formulas in oracle/solids.py), moved by the reference's draws, membership = strictly inside
    every face plane (brute force over all 9800 / 500 / 100 triangles).  The product evaluates the same polyhedra in
    closed form (three plane tests for the sphere, one or two for the others): the two must agree POINT FOR POINT,
    including points within 1e-5 of a face or an edge.  (open3d itself is not in the image: pinned to the restatement.)
    Also: the rotation against the axis-angle properties open3d documents, and the smooth solids (exact_solid=True)
    differ from the meshes only inside the tessellation's band."""
    import numpy as np
    import torch
    from oracle import solids
    from puzzlenet_amd import datapipe as dp
    rng = np.random.default_rng(5)
    for kind in ("sphere", "cylinder", "cone"):
        V0, T0 = {"sphere": solids.create_sphere(0.5, 50), "cylinder": solids.create_cylinder(0.6, 1.0, 50),
                  "cone": solids.create_cone(1.0, 2.0, 50)}[kind]
        assert len(V0) == {"sphere": 4902, "cylinder": 252, "cone": 52}[kind]          # open3d's vertex counts
        assert len(T0) == {"sphere": 9800, "cylinder": 500, "cone": 100}[kind]
        for trial in range(3):
            rot, shift = rng.random(3), rng.random(3) / 3
            R = dp.rotation_from_axis_angle(torch.from_numpy(rot)[None])[0].numpy()
            np.testing.assert_allclose(R, solids.rotation_from_axis_angle(rot), atol=1e-14)
            np.testing.assert_allclose(R @ rot, rot, atol=1e-12)
            np.testing.assert_allclose(R @ R.T, np.eye(3), atol=1e-12)
            np.testing.assert_allclose(np.trace(R), 1 + 2 * np.cos(np.linalg.norm(rot)), atol=1e-12)
            V, T = solids.solid_mesh(kind, rot, shift)
            cen = V.mean(0)
            bulk = rng.random((20000, 3)) * 2.4 - 1.2
            fc, ec = V[T].mean(1), 0.5 * (V[T[:, 0]] + V[T[:, 1]])
            near_f = cen + (fc - cen) * rng.choice([0.999, 0.9999, 0.99999, 1.00001, 1.0001, 1.001], size=(len(fc), 1))
            near_e = cen + (ec - cen) * rng.choice([0.9999, 0.99999, 1.00001, 1.0001], size=(len(ec), 1))
            P = np.concatenate([bulk, near_f, near_e]).astype(np.float32)
            want = solids.solid_cut_mask(P.astype(np.float64), kind, rot, shift)
            t = torch.from_numpy(P)[None]
            got = dp.solid_cut_mask(t, kind, torch.from_numpy(rot)[None], torch.from_numpy(shift)[None])[0].numpy()
            assert np.array_equal(got, want), (kind, trial, int((got != want).sum()))
            assert 0 < got[:20000].mean() < 1
            # the smooth solid of the same name: same answer except inside the tessellation's band under the surface
            smooth = dp.solid_cut_mask(t, kind, torch.from_numpy(rot)[None], torch.from_numpy(shift)[None], exact_solid=True)[0].numpy()
            diff = smooth != got
            assert not (got & ~smooth).any()                       # the mesh is inscribed: never inside it but outside the solid
            assert diff[:20000].mean() < 5e-3
    # apex and base of the cone as open3d builds it (create_cone(radius=1, height=2) then translate (0,0,-1)), unrotated
    zero = torch.zeros(1, 3, dtype=torch.float64)
    probe = torch.tensor([[[0.0, 0.0, 0.9], [0.0, 0.0, 1.1], [0.9, 0.0, -0.95], [1.05, 0.0, -0.95], [0.0, 0.0, -1.05]]])
    assert dp.solid_cut_mask(probe, "cone", zero + 1e-12, None).tolist() == [[True, False, True, False, False]]


@pytest.mark.parametrize("mode", ["plane", "solid", "double"])
def test_feeder_draws_keep_the_meaning_of_a_seed(mode):
    """The host draws of a PairFeeder batch, per mode, against the generator calls written out: the same calls on the
    RandomState and on the torch Generator, with the same shapes, in the same order, land in the same staging columns - for
    two consecutive batches.  (The GPU tests pin "same seed, same batches"; this pins what the seed means.)"""
    import torch
    from puzzlenet_amd import datapipe
    B, K, seed, mag = 3, 4, 7, 0.8
    draw = {"plane": datapipe.draw_plane_batch, "solid": datapipe.draw_solid_batch, "double": datapipe.draw_double_batch}[mode]
    width = {"plane": 3 * K + K + 2 + 6, "solid": 6 * K + 2 + 6, "double": (K + 7) * 4 + 7 + 6}[mode]
    rng, gen = np.random.RandomState(seed), torch.Generator().manual_seed(seed)
    want_rng, want_gen = np.random.RandomState(seed), torch.Generator().manual_seed(seed)
    for _ in range(2):
        got = np.full((B, width), np.nan)
        draw(rng, gen, B, K, mag, got)
        r = want_rng
        if mode == "plane":
            blocks = [r.rand(B, 3 * K), r.rand(B, K) / 3, r.rand(B, 2)]
        elif mode == "solid":
            blocks = [datapipe.solid_draws(r, B, K).reshape(B, 6 * K), r.rand(B, 2)]
        else:
            blocks = [r.rand(B, 3 * K), r.rand(B, K) / 3, r.rand(B, 21), r.rand(B, 7) / 3, r.rand(B, 7)]
        x = torch.randn(B, 6, generator=want_gen, dtype=torch.float64)
        blocks.append((x / x.norm(p=2, dim=1, keepdim=True) * mag).numpy())
        want = np.concatenate(blocks, axis=1)
        assert want.shape == got.shape and np.array_equal(got, want)


@pytest.mark.parametrize("clouds", [1, 2])
def test_fps_start_draws_keep_the_meaning_of_a_seed(clouds, monkeypatch):
    """The host draws of a sampling plan against the generator calls written out: per cloud, in order, randint(0, N, (rows,))
    for the level-1 starts and randint(0, 512, (rows,)) for the level-2 starts - exactly these calls and no other, from the
    generator that is passed and, with None, from the global one.  (One cloud: assembly's pieces; two: predict5's pair,
    Encoder's two levels before Encoder2's.)"""
    import torch
    from puzzlenet_amd import model5_b
    rows, N, seed = 5, 1000, 11
    n1 = model5_b.PCTransformer_nonsort.SA_LEVELS[0][0]
    assert n1 == 512
    real, calls = torch.randint, []

    def spy(*a, **k):
        calls.append((a, k.get("generator")))
        return real(*a, **k)
    want_gen = torch.Generator().manual_seed(seed)
    want = [real(0, n_, (rows,), generator=want_gen) for _ in range(clouds) for n_ in (N, 512)]
    gen = torch.Generator().manual_seed(seed)
    monkeypatch.setattr(torch, "randint", spy)
    got = model5_b.draw_fps_starts(clouds, rows, N, gen)
    torch.manual_seed(seed)
    got_global = model5_b.draw_fps_starts(clouds, rows, N, None)
    after = real(0, 1 << 30, (4,))
    monkeypatch.setattr(torch, "randint", real)
    per_cloud = [((0, N, (rows,)), gen), ((0, 512, (rows,)), gen)]
    assert calls == per_cloud * clouds + [(a, None) for a, _ in per_cloud] * clouds
    assert len(got) == len(got_global) == 2 * clouds
    for g, gg, w in zip(got, got_global, want):
        assert g.dtype == torch.long and g.device.type == "cpu" and torch.equal(g, w) and torch.equal(gg, w)
    # the global generator was consumed by exactly these calls: what it gives next is what follows them
    torch.manual_seed(seed)
    for _ in range(clouds):
        real(0, N, (rows,)), real(0, 512, (rows,))
    assert torch.equal(after, real(0, 1 << 30, (4,)))
