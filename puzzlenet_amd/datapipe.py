"""Training-pair construction on the GPU: the reference's `CADDataset` — single cut
(dataset.py:1165-1190) and the double-cut variants of `__getitem__` (:1203-1355) — and `BuildingDataset` (:1370-1429),
each followed by `MovedCADDataset2.__getitem__` (:98-105), batched, on the kernels of the hot path.

    raw cloud [M,3]  --plane cut (dataset.py:761-775)-->  up / down  --numpy FPS to N (:1147-1163)-->  N-point pieces
        --get_boundary (:1357-1367: chamfer both ways, the 128 points nearest to the other piece + 0/1 masks)-->
        --RandomTransformSE3 (se_math/transforms.py:151-197: unit twist * mag, exp, apply to `up`)-->
    (down, moved_up, igt, up, down_boundary, up_boundary, down_mask, up_mask)  == the 8-tuple the model consumes.

The reference does this per sample in 64 CPU workers (train.py:101: numpy FPS loops over ~5-12 k points); here a batch
is a handful of launches: the FPS of both pieces is `pzn_fps_f32` on the compacted pieces (padded with copies of their
first point: a copy never beats the original under the first-maximum rule, so the selection sequence is the
reference's), the boundary is `pzn_chamfer_fwd_f32` + top-k, the motion `pzn_se3_exp_fwd_f32`.

Randomness stays OUTSIDE: the caller passes the draws (plane normal / offset, FPS start indices, unit twists) — e.g.
`draws_like_reference` replays numpy / torch generators in the reference's order — so results can be compared draw for
draw with the reference's functions (tests/golden/make_golden_data.py -> data.npz).  The double-cut variants are the
same machinery on REGIONS of two planes (`make_pairs_regions`; `plan_double_cut_like_reference` replays the
reference's branch decisions and draws); `building_pairs` is the item contract of `BuildingDataset` (two given pieces).
The solid cuts (sphere, cylinder, cone: dataset.py:716-758) are `solid_cut_mask` + `make_pairs_solid`: the reference
asks open3d (0.15.2, README.md:25) for the signed distance to a tessellated mesh and keeps `distance < 0`.  open3d is not
in this image, so its published mesh construction is restated (oracle/solids.py: vertex formulas of create_sphere /
create_cylinder / create_cone at resolution 50) and `solid_cut_mask` evaluates membership of exactly those convex
polyhedra in closed form; tests/test_datapipe_cpu.py holds it to the oracle's brute-force face-plane test point for
point.  Parity is pinned to that restatement, not to the library itself (no fixture can be produced here).

For a loader that runs BESIDE the training step there is `PairFeeder`: a fresh batch per step on a background stream, cut by
a plane (`cut_pairs`: csrc/datapipe.hip) or by one of the three solids (`PairFeeder(..., cut="sphere" | "cylinder" | "cone")`
-> `cut_pairs_solid`: csrc/solidcut.hip; both kernels are the one body of csrc/pzn_cut.h).  Either cut is ONE launch per batch: K candidate draws per sample (`solid_draws`
for the solids), the first that leaves >= n points in both pieces taken on the device (the reference's re-draw loop,
dataset.py:1175-1180), both pieces compacted in point order and padded, the FPS start indices.  The solid kernel tests the
same polyhedra as `solid_cut_mask`, face plane by face plane with the rotation families folded (no atan2 / acos per point);
tests/test_gpu_solid_feeder.py holds its pieces to the oracle's masks bit for bit.
`PairFeeder(..., split_twice=True)` is the reference's second sampling mode (`train.py --random_slice`, dataset.py:1203-1355):
the double cuts, decided and compacted on the device in one launch (`double_cut_rule` states the rule, csrc/doublecut.hip runs
it, `cut_pairs_double` samples the pair and its fallback and applies the reference's acceptance test without a host round trip).
`PairFeeder(..., pieces=P | (lo, hi))` cuts pairs out of P-piece fractures (no counterpart in the reference): the fracture's
cuts, the choice of the pair and the compaction of its pieces alone are one launch (`fracture_pair_rule` states the rule,
csrc/fracture.hip runs it, `cut_pairs_fracture` samples the pair and its fallback as `cut_pairs_double` does).
The four modes share one `next_batch` (staging turn, pinned upload, events) and one tail from the compacted pieces to the
8-tuple (`_sample`, `_picks`, `_finish`); a mode is a staging layout, a host draw function and a builder.
"""
import collections

import numpy as np
import torch

from . import _lib, ops, se3


def draws_like_reference(raw, n=1024, mag=0.8, max_tries=100):
    """The random draws of one sample in the reference's order, from numpy's and torch's GLOBAL generators (seed them as
    the reference run would): plane normal `np.random.rand(3,1)` and offset `np.random.rand(1)/3` (dataset.py:767-769),
    re-drawn while a piece holds fewer than n points (:1176-1180); FPS starts `np.random.randint(0, n_piece)` for up
    then down (:1153, called at :1181-1182); the twist `randn(1,6)` normalised to `mag` (transforms.py:163-168).
    raw: [M,3] float32 numpy array (host side: the piece sizes decide the range of the start indices).
    -> dict(normal[3] f64, z[1] f64, s_up, s_down, twist[6] f32)"""
    raw = np.asarray(raw, dtype=np.float32)
    for _ in range(max_tries):
        normal = np.random.rand(3, 1)
        z = np.random.rand(1) / 3
        dis = np.dot(raw, normal) + z
        n_up, n_down = int((dis >= 0).sum()), int((dis < 0).sum())
        if n_up >= n and n_down >= n:
            break
    else:
        raise _lib.PznError(f"draws_like_reference: no plane left {n} points on both sides in {max_tries} tries")
    s_up = int(np.random.randint(0, n_up))
    s_down = int(np.random.randint(0, n_down))
    x = torch.randn(1, 6)
    x = x / x.norm(p=2, dim=1, keepdim=True) * mag
    return dict(normal=normal.reshape(3), z=z.reshape(1), s_up=s_up, s_down=s_down, twist=x.reshape(6).numpy())


def plane_cut_mask(raw, normal, z):
    """dataset.py:767-772: `dis = points . normal + z`, up = dis >= 0.  The reference multiplies float32 points with
    float64 draws, i.e. evaluates in float64: so does this (one fused pass over B*M*3 values)."""
    dis = (raw.to(torch.float64) * normal.to(torch.float64).unsqueeze(1)).sum(-1)
    # numpy's dot of a row with the 3-vector sums in index order; so does the line above after the product
    dis = dis + z.to(torch.float64).reshape(-1, 1)
    return dis >= 0


def rotation_from_axis_angle(w):
    """open3d.geometry.get_rotation_matrix_from_axis_angle(w): Rodrigues rotation by |w| about w / |w| (the reference
    feeds np.random.rand(3,1), dataset.py:735, :751).  w [B,3] float64 -> R [B,3,3] float64."""
    w = w.to(torch.float64)
    th = w.norm(dim=1, keepdim=True).clamp_min(1e-300)
    k = w / th
    K = torch.zeros(w.shape[0], 3, 3, dtype=torch.float64, device=w.device)
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0] = -k[:, 2], k[:, 1], k[:, 2]
    K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -k[:, 0], -k[:, 1], k[:, 0]
    th = th.unsqueeze(-1)
    eye = torch.eye(3, dtype=torch.float64, device=w.device).expand_as(K)
    return eye + torch.sin(th) * K + (1 - torch.cos(th)) * (K @ K)


_MESH_RES = 50        # resolution of the reference's three meshes (dataset.py:717, :733, :750)


def _sphere_poly_inside(q, radius, res):
    """Strictly inside the polyhedron of open3d's create_sphere(radius, res) centred at the origin (oracle/solids.py has
    the vertex formulas): rings at polar angles alpha_i = i pi / res, 2 res meridians.  The polyhedron is convex and
    contains the origin, so q is inside iff it is on the inner side of the face its ray from the origin pierces; that
    face lies in q's own meridian sector (meridian edges project to meridians) and in its own latitude band or a
    neighbouring one (ring chords project to great-circle arcs that bulge across the latitude circle by less than a
    band): three plane tests.  q [...,3] float64."""
    step = torch.pi / res
    rho = q.norm(dim=-1).clamp_min(1e-300)
    alpha = torch.acos((q[..., 2] / rho).clamp(-1.0, 1.0))
    theta = torch.atan2(q[..., 1], q[..., 0])
    theta = torch.where(theta < 0, theta + 2 * torch.pi, theta)
    j = torch.clamp((theta / step).floor(), 0, 2 * res - 1)
    i0 = torch.clamp((alpha / step).floor(), 0, res - 1)
    t0, t1 = j * step, (j + 1) * step

    def ring(i, t):          # vertex of ring i (0 = north pole, res = south pole) on meridian t
        a = i * step
        return torch.stack([radius * torch.sin(a) * torch.cos(t), radius * torch.sin(a) * torch.sin(t), radius * torch.cos(a)], -1)

    inside = torch.ones(q.shape[:-1], dtype=torch.bool, device=q.device)
    for di in (-1, 0, 1):
        i = torch.clamp(i0 + di, 0, res - 1)
        # three non-collinear corners of the face (band i, sector j): a triangle at the poles, a planar trapezoid elsewhere
        a_ = ring(i, t0)
        b_ = torch.where((i == 0).unsqueeze(-1), ring(i + 1, t0), ring(i, t1))
        c_ = ring(i + 1, t1)
        n = torch.cross(b_ - a_, c_ - a_, dim=-1)
        n = n * torch.sign((n * a_).sum(-1, keepdim=True) + (n * c_).sum(-1, keepdim=True))      # outward (origin inside)
        n = n / n.norm(dim=-1, keepdim=True)
        inside &= (n * q).sum(-1) < (n * c_).sum(-1)
    return inside


def _ngon_inside(x, y, radius, res):
    """Strictly inside the regular res-gon with vertices radius (cos(2 pi j / res), sin(2 pi j / res))."""
    step = 2 * torch.pi / res
    theta = torch.atan2(y, x)
    theta = torch.where(theta < 0, theta + 2 * torch.pi, theta)
    j = torch.clamp((theta / step).floor(), 0, res - 1)
    phi = (j + 0.5) * step                                   # outward normal of the edge (V_j, V_j+1)
    return x * torch.cos(phi) + y * torch.sin(phi) < radius * torch.cos(torch.tensor(step / 2, dtype=x.dtype, device=x.device))


def solid_cut_mask(raw, kind, rot=None, shift=None, exact_solid=False):
    """up-mask (signed distance < 0 = strictly INSIDE the closed mesh) of the reference's mesh cuts:
      "sphere"   (dataset.py:716-730): create_sphere(0.5, 50), centre = shift (np.random.rand(3,1)/3)
      "cylinder" (:732-747): create_cylinder(0.6, 1, 50) about z, rotated by the axis-angle vector rot
                 (np.random.rand(3,1)) about the origin, then translated by shift (np.random.rand(3,1)/3)
      "cone"     (:749-763): create_cone(1, 2, 50) translated by (0,0,-1) (base at z = -1, apex at z = +1), rotated by
                 rot about the origin
    evaluated on the POLYHEDRA open3d 0.15.2 builds (resolution 50: a 4902-vertex UV sphere, a 50-gon prism, a 50-gon
    pyramid; vertex formulas restated in oracle/solids.py) in closed form: the meshes are convex, so membership is a
    handful of plane tests per point.  exact_solid=True: the smooth solids instead (round 3's form; differs in a band of
    <= 0.1 % of the radius under the surface).  raw [B,M,3] fp32, rot / shift [B,3] float64 (the draws) -> bool [B,M];
    float64 like the plane cut."""
    p = raw.to(torch.float64)
    res = _MESH_RES
    if kind == "sphere":
        d = p - shift.to(torch.float64).unsqueeze(1)
        if exact_solid:
            return (d * d).sum(-1) < 0.25
        return _sphere_poly_inside(d, 0.5, res)
    R = rotation_from_axis_angle(rot)                     # mesh point = R x (+ shift): x = R^T (p - shift)
    if kind == "cylinder":
        q = torch.einsum("bji,bmj->bmi", R, p - shift.to(torch.float64).unsqueeze(1))
        if exact_solid:
            return (q[..., 0] ** 2 + q[..., 1] ** 2 < 0.36) & (q[..., 2].abs() < 0.5)
        return _ngon_inside(q[..., 0], q[..., 1], 0.6, res) & (q[..., 2].abs() < 0.5)
    if kind == "cone":
        q = torch.einsum("bji,bmj->bmi", R, p)
        h = q[..., 2] + 1.0                               # height above the base plane, apex at h = 2
        if exact_solid:
            rad = (q[..., 0] ** 2 + q[..., 1] ** 2).sqrt()
            return (h > 0) & (h < 2) & (rad < 1.0 - h / 2)
        # side face of sector j: the plane through the apex (0,0,2) and the base edge (V_j, V_j+1); its outward normal is
        # (cos(phi) 2, sin(phi) 2, cos(step / 2)) up to scale, phi = (j + 1/2) step: 2 (x cos phi + y sin phi) + c h < 2 c
        step = 2 * torch.pi / res
        theta = torch.atan2(q[..., 1], q[..., 0])
        theta = torch.where(theta < 0, theta + 2 * torch.pi, theta)
        j = torch.clamp((theta / step).floor(), 0, res - 1)
        phi = (j + 0.5) * step
        c = torch.cos(torch.tensor(step / 2, dtype=torch.float64, device=q.device))
        side = 2.0 * (q[..., 0] * torch.cos(phi) + q[..., 1] * torch.sin(phi)) + c * h < 2.0 * c
        return (h > 0) & side
    raise _lib.PznError(f"solid_cut_mask: unknown solid {kind!r}")


def make_pairs_mask(raw, mask, start_up, start_down, twist, n=1024, k=128, cap=None, background=False):
    """The pair construction from a given up-mask [B,M] (whatever cut produced it): raw [B,M,3] fp32 on the GPU + the draws ->
    the 8-tuple (down, moved_up, igt, up, down_boundary, up_boundary, down_mask, up_mask) and `ok` [B] (both pieces of the cut
    hold >= n points: the reference re-draws the cut otherwise, dataset.py:1176-1180 - the caller re-draws for the rows where
    ok is False).  background=True: the sampling as the small-footprint launch that skips the padding (for a side stream
    beside a training step: PairFeeder)."""
    if not raw.is_cuda:
        raise _lib.PznError("datapipe.make_pairs_mask runs on the GPU (puzzlenet_amd has no CPU fallback)")
    raw = raw.to(torch.float32).contiguous()
    B, M, _ = raw.shape
    cap = M if cap is None else int(cap)
    up_piece, n_up = _compact(raw, mask, cap)
    down_piece, n_down = _compact(raw, ~mask, cap)
    ok = (n_up >= n) & (n_down >= n) & (n_up <= cap) & (n_down <= cap)      # (a piece larger than `cap` would be truncated)
    # one FPS launch for both pieces of every sample (a workgroup per piece: 2B workgroups instead of 2 x B)
    both = fps_to_n(torch.cat([up_piece, down_piece], 0), torch.cat([n_up, n_down], 0),
                    torch.cat([start_up.reshape(-1), start_down.reshape(-1)], 0), n, background=background)
    up, down = both[:B].contiguous(), both[B:].contiguous()
    downb, upb, down_mask, up_mask = boundary(down, up, k)
    moved, igt = move(up, twist)
    return (down, moved, igt, up, downb, upb, down_mask, up_mask), ok


def make_pairs_solid(raw, kind, rot, shift, start_up, start_down, twist, n=1024, k=128, cap=None):
    """CADDataset with slice = sphere_split / cylinder_split / cone_split (dataset.py:1463-1546 keys *_sphere, *_cyl,
    *_cone; BASELINE configs[0] "bed_sphere"): the mesh's inside is `up` (parity: see the module header)."""
    return make_pairs_mask(raw, solid_cut_mask(raw, kind, rot, shift), start_up, start_down, twist, n, k, cap)


def _compact(raw, mask, cap):
    """Rows of `raw` where mask, in their original order, padded to `cap` rows with copies of the first kept row.
    -> (packed [B,cap,3], count [B])"""
    B, M, _ = raw.shape
    count = mask.sum(1)
    # stable partition: kept rows first, original order inside each part
    order = torch.sort((~mask).to(torch.int8), dim=1, stable=True)[1]
    packed = torch.gather(raw, 1, order[:, :cap].unsqueeze(-1).expand(-1, -1, 3))
    pos = torch.arange(cap, device=raw.device).unsqueeze(0)
    first = packed[:, :1, :]
    return torch.where((pos < count.unsqueeze(1)).unsqueeze(-1), packed, first.expand(-1, cap, -1)).contiguous(), count


def fps_to_n(piece, count, start, n, background=False):
    """dataset.py:1147-1163 on every piece of the batch: farthest point sampling from `start`, points returned in
    selection order.  piece [B,cap,3] from _compact (padding = copies of row 0)."""
    if int(piece.shape[1]) > 32768:
        raise _lib.PznUnsupported(f"fps_to_n: pieces of up to {piece.shape[1]} points (the FPS kernel holds <= 32768)")
    idx = ops.farthest_point_sample(piece, n, start.to(torch.int64), background=background, counts=count if background else None)
    return torch.gather(piece, 1, idx.unsqueeze(-1).expand(-1, -1, 3))


def boundary(down, up, k=128):
    """dataset.py:1357-1367 `get_boundary(self.down, self.up)`: the k points of each piece that lie nearest to the
    other piece, and their 0/1 masks.  -> (down_boundary [B,k,3], up_boundary [B,k,3], down_mask [B,N], up_mask [B,N])"""
    cd_over_up, cd_over_down = ops.chamfer(down, up)          # min over `down` per up-point, min over `up` per down-point
    top_up = torch.topk(-cd_over_up, k, dim=1)[1]
    top_down = torch.topk(-cd_over_down, k, dim=1)[1]
    upb = torch.gather(up, 1, top_up.unsqueeze(-1).expand(-1, -1, 3))
    downb = torch.gather(down, 1, top_down.unsqueeze(-1).expand(-1, -1, 3))
    down_mask = torch.zeros(down.shape[:2], dtype=torch.float32, device=down.device).scatter_(1, top_down, 1.0)
    up_mask = torch.zeros(up.shape[:2], dtype=torch.float32, device=up.device).scatter_(1, top_up, 1.0)
    return downb, upb, down_mask, up_mask


def move(up, twist):
    """transforms.py:176-186: g = exp(x), p1 = g . p0, igt = g."""
    g = se3.exp(twist.to(torch.float32))
    moved = se3.transform(g, up.permute(0, 2, 1)).permute(0, 2, 1).contiguous()
    return moved, g


def make_pairs(raw, normal, z, start_up, start_down, twist, n=1024, k=128, cap=None, background=False):
    """make_pairs_mask for the plane cut of dataset.py:761-775: normal [B,3], z [B] float64 draws."""
    if not raw.is_cuda:
        raise _lib.PznError("datapipe.make_pairs runs on the GPU (puzzlenet_amd has no CPU fallback)")
    raw = raw.to(torch.float32).contiguous()
    return make_pairs_mask(raw, plane_cut_mask(raw, normal, z), start_up, start_down, twist, n, k, cap, background)


def _feeder_cap(who, raw, cap):
    """The guard of the cut_pairs* forms: -> rows a piece may hold."""
    if not raw.is_cuda:
        raise _lib.PznError(f"datapipe.{who} runs on the GPU (puzzlenet_amd has no CPU fallback)")
    cap = raw.shape[1] if cap is None else int(cap)
    if cap > 32768:
        raise _lib.PznUnsupported(f"{who}: pieces of up to {cap} points (the FPS kernel holds <= 32768)")
    return cap


# The tail of a feeder batch, from the compacted pieces of a cut to the 8-tuple, in three stages on [2B, ...] stacks (up rows,
# then down rows).  A valid cut leaves >= n points on either side, so a piece holds <= M - n (the promise made to the
# small-footprint FPS); rows of samples without a valid cut are re-drawn by the caller.
def _sample(pieces, counts, start, n, M):                                                        # dataset.py:1147-1163
    idx = ops.farthest_point_sample(pieces, n, start, background=True, counts=counts, max_count=max(M - n, n))
    return ops.index_points(pieces, idx)


def _picks(both, k):                                                                             # dataset.py:1357-1367
    B = both.shape[0] // 2
    cd_over_up, cd_over_down = ops.chamfer(both[B:], both[:B])
    top = ops.topk_rows(torch.cat([cd_over_up, cd_over_down], 0).neg_(), k)                      # [2B,k]: up picks, down picks
    return top, ops.index_points(both, top)


def _finish(both, top, bnd, twist):
    B, n = both.shape[0] // 2, both.shape[1]
    masks = ops.pick_mask(top, n)
    g = se3.exp(twist.to(torch.float32))                                                         # transforms.py:176-186
    up, down = both[:B], both[B:]
    moved = se3.transform_points(g, up)
    return down, moved, g, up, bnd[B:], bnd[:B], masks[B:], masks[:B]


def _pair_tail(pieces, counts, start, ok, twist, n, k, M):
    """pieces [2B,cap,3], counts / start [2B], ok [B] of a single cut -> (the 8-tuple, ok [B] with the piece sizes held to n)"""
    B = ok.shape[0]
    both = _sample(pieces, counts, start, n, M)
    top, bnd = _picks(both, k)
    return _finish(both, top, bnd, twist), ok & (counts[:B] >= n) & (counts[B:] >= n)


def cut_pairs(raw, normals, zs, u, twist, n=1024, k=128, cap=None):
    """make_pairs for a loader that runs BESIDE the training step (PairFeeder): the cut with its re-draw (K candidate planes per
    sample, the first valid one taken on the device), both pieces compacted and padded, the FPS start indices - one launch
    (csrc/datapipe.hip, ops.cut_compact); sampling by the small-footprint FPS that skips the padding; boundary picks by
    ops.topk_rows; masks by one launch.  raw [B,M,3]; normals [B,K,3], zs [B,K], u [B,2] float64 draws; twist [B,6].
    -> ((down, moved_up, igt, up, down_boundary, up_boundary, down_mask, up_mask), ok [B], plane [B,4])"""
    cap = _feeder_cap("cut_pairs", raw, cap)
    pieces, counts, start, plane, ok = ops.cut_compact(raw, normals, zs, u, n, cap)
    return _pair_tail(pieces, counts, start, ok, twist, n, k, raw.shape[1]) + (plane,)


def solid_draws(rng, B, K):
    """K candidate solids per sample from ONE rng.rand(B, K, 6): columns 0-2 the axis-angle vector np.random.rand(3,1)
    (dataset.py:732, :749), columns 3-5 the translation np.random.rand(3,1)/3 (:718, :733).  -> [B,K,6] float64"""
    p = rng.rand(B, K, 6)
    p[:, :, 3:] /= 3
    return p


def cut_pairs_solid(raw, kind, params, u, twist, n=1024, k=128, cap=None):
    """cut_pairs with a sphere / cylinder / cone cut (dataset.py:715-759; the mesh's inside is `up`) in front: K candidate
    solids per sample, the first valid one taken on the device, both pieces compacted and padded, the FPS start indices -
    one launch (csrc/solidcut.hip, ops.cut_compact_solid); the rest is cut_pairs' tail.  raw [B,M,3]; kind "sphere" |
    "cylinder" | "cone"; params [B,K,6] (rot, shift: solid_draws), u [B,2] float64 draws; twist [B,6].
    -> ((down, moved_up, igt, up, down_boundary, up_boundary, down_mask, up_mask), ok [B], chosen [B,6])"""
    cap = _feeder_cap("cut_pairs_solid", raw, cap)
    pieces, counts, start, chosen, _, ok = ops.cut_compact_solid(raw, kind, params, u, n, cap)
    return _pair_tail(pieces, counts, start, ok, twist, n, k, raw.shape[1]) + (chosen,)


DoubleCut = collections.namedtuple("DoubleCut", "kind planes tabs rejected cd U D Ub Db")
DoubleCut.__doc__ = """What cut_pairs_double decided per sample: kind [B] int32 (SINGLE .. HALVES), planes [B,2,4] float64 (normal, z of
plane 1 and plane 2; plane 2 zero for SINGLE), tabs [B,4] int32 (u_tab, d_tab), rejected [B] bool (the HALF_VS_OTHER pair was
replaced by its fallback), cd [B] float32 (chamfer distance of the primary pair's boundaries) and the PRIMARY pair itself
(U, D [B,n,3]; Ub, Db [B,k,3]), from which cd can be recomputed."""


def cut_pairs_double(raw, normals1, zs1, normals2, zs2, u, twist, n=1024, n_rich=None, k=128, cap=None):
    """cut_pairs for the reference's double cuts (dataset.py:1203-1355, split_twice=True; the rule: double_cut_rule): steps 1-7
    - branch decisions, region tables, the two-segment compaction of U, D and the HALF_VS_OTHER fallback pair, start indices -
    are one launch (csrc/doublecut.hip, ops.cut_compact_double); then the sampling of the primary and of the fallback rows (the
    second launch runs rounds for the HALF_VS_OTHER samples only: the other rows carry counts = -1), the primary pair's
    boundary, step 8 (`cd` of the two boundaries against 0.015, :1253-1256) as a device-side select, and cut_pairs' tail on the
    final pair.  Nothing here reads a value back to the host.  raw [B,M,3]; normals1 [B,K,3], zs1 [B,K], normals2 [B,7,3],
    zs2 [B,7], u [B,7] float64 draws; twist [B,6]; n_rich: None = 3000 n / 1024.
    -> ((D, moved U, igt, U, D boundary, U boundary, D mask, U mask), ok [B], DoubleCut)"""
    cap = _feeder_cap("cut_pairs_double", raw, cap)
    B, M, _ = raw.shape
    n_rich = 3000 * n // 1024 if n_rich is None else int(n_rich)
    pieces, counts, start, kind, planes, tabs, ok = ops.cut_compact_double(raw, normals1, zs1, normals2, zs2, u, n, n_rich, cap)
    # [2B,n,3] each: U rows, D rows (U holds >= n points, so D holds <= M - n; the fallback is a valid single cut)
    primary = _sample(pieces[:2 * B], counts[:2 * B], start[:2 * B], n, M)
    fallback = _sample(pieces[2 * B:], counts[2 * B:], start[2 * B:], n, M)
    _, bnd = _picks(primary, k)
    cd1, cd2 = ops.chamfer(bnd[B:], bnd[:B])                                                     # :1253-1254
    cd = cd1.mean(1) + cd2.mean(1)
    rejected = double_cut_rejects(kind, cd)
    both = torch.where(rejected.repeat(2).view(2 * B, 1, 1), fallback, primary)
    top, fbnd = _picks(both, k)
    record = DoubleCut(kind, planes, tabs, rejected, cd, primary[:B], primary[B:], bnd[:B], bnd[B:])
    return _finish(both, top, fbnd, twist), ok & (counts[:B] >= n) & (counts[B:2 * B] >= n), record


FracturePair = collections.namedtuple("FracturePair", "kind pair rejected cd label planes target cand U D Ub Db")
FracturePair.__doc__ = """What cut_pairs_fracture decided per sample: kind [B] int32 (SIBLING, NEIGHBOUR), pair [B,4] int32 (the labels of U, D and
of the fallback pair, -1: none), rejected [B] bool (the NEIGHBOUR pair was replaced by the sibling pair), cd [B] float32 (chamfer
distance of the primary pair's boundaries), the fracture itself (label [B,M] uint8, planes [B,P-1,4] float64, target / cand
[B,P-1] int32; rows of the cuts a sample did not make are zero) and the PRIMARY pair (U, D [B,n,3]; Ub, Db [B,k,3]), from which cd
can be recomputed."""


CurvedFracturePair = collections.namedtuple("CurvedFracturePair", FracturePair._fields + ("anchor",))
CurvedFracturePair.__doc__ = """FracturePair of a curved cut (cut_pairs_fracture(..., frames=, half_curv=)): planes holds the tangent planes at the
anchors, and anchor [B,P-1] int32 the cloud row of the anchor taken at every step (zero for the cuts a sample did not make)."""


ErodedFracturePair = collections.namedtuple("ErodedFracturePair", FracturePair._fields + ("anchor", "erode", "lost"))
ErodedFracturePair.__doc__ = """FracturePair of an eroded cut (cut_pairs_fracture(..., erode=)): anchor [B,P-1] int32 the cloud row of the
anchor taken at every step (the chip's centre), erode [B,P-1,4] float64 the (w_up, w_dn, depth, rho) the cuts were made with, and
lost [B,P-1] int32 the points lost at every step (label ops.FRACTURE_LOST; zero for the cuts a sample did not make)."""

ErodedCurvedFracturePair = collections.namedtuple("ErodedCurvedFracturePair", CurvedFracturePair._fields + ("erode", "lost"))
ErodedCurvedFracturePair.__doc__ = """CurvedFracturePair of an eroded cut: then erode and lost, as ErodedFracturePair holds them."""


def cut_pairs_fracture(raw, normals, u_anchor, pieces, u, twist, n=1024, k=128, neighbours=0.5, cap=None, frames=None,
                       half_curv=None, erode=None):
    """cut_pairs for pairs cut out of a fracture (the rule: fracture_pair_rule): every cloud cut into pieces[b] pieces, the pair
    chosen and only its pieces - and the fallback's - compacted in one launch (csrc/fracture.hip, ops.fracture_pair; the cuts
    leave >= n points on both sides, n_min = n); then, as cut_pairs_double does, the sampling of the primary and of the fallback
    rows (one launch for both; rounds run for the fallback rows of the NEIGHBOUR samples only: the other rows carry
    counts = -1), the primary pair's boundary, step 8 (`cd` of the two boundaries against CD_ACCEPT) as a device-side select,
    and cut_pairs' tail on the final pair.  Nothing here reads a value back to the host.  raw [B,M,3]; normals [B,P-1,K,3],
    u_anchor [B,P-1,K], u [B,7] float64 draws; pieces: ops.fracture_pair's; twist [B,6].
    -> ((D, moved U, igt, U, D boundary, U boundary, D mask, U mask), ok [B], FracturePair)
    frames [B,P-1,K,3,3] and half_curv [B,P-1,K,2] float64, with normals=None: the cuts are curved (ops.fracture_pair_curved; the
    rule: fracture_pair_curved_rule) and the record is a CurvedFracturePair, which adds `anchor`.
    erode [B,P-1,4] float64 = (w_up, w_dn, depth, rho) per step (draw_erosion): material is lost along every cut, in the same one
    launch (ops.fracture_pair_eroded; the rule: fracture_pair_eroded_rule), and the record is the one of its form extended by
    `anchor` (where it lacks one), `erode` and `lost`: an ErodedFracturePair or ErodedCurvedFracturePair.  None is the call
    without erosion.  `cd` and the acceptance test of step 8 are taken on the ERODED pieces: a gap g between two boundaries adds
    about 2 g^2 to cd, which is held against the unchanged CD_ACCEPT = 0.015."""
    cap = _feeder_cap("cut_pairs_fracture", raw, cap)
    B, M, _ = raw.shape
    anchor = lost = None
    curved = _curved("cut_pairs_fracture", normals, frames, half_curv)
    if erode is not None:
        packed, counts, start, kind, pair, label, planes, target, cand, anchor, lost, ok = ops.fracture_pair_eroded(
            raw, normals, u_anchor, pieces, u, erode, n, neighbours, cap, frames=frames, half_curv=half_curv)
    elif curved:
        packed, counts, start, kind, pair, label, planes, target, cand, anchor, ok = ops.fracture_pair_curved(
            raw, frames, half_curv, u_anchor, pieces, u, n, neighbours, cap)
    else:
        packed, counts, start, kind, pair, label, planes, target, cand, ok = ops.fracture_pair(raw, normals, u_anchor, pieces, u, n,
                                                                                              neighbours, cap)
    # [2B,n,3] each: U rows, D rows (every cut left >= n points on its other side, so a piece holds <= M - n).  The primary and
    # the fallback rows are sampled in ONE launch: a sampling launch lasts its n dependent rounds however few workgroups run them
    # (measured: the fallback rows of half the samples alone cost what the primary rows cost), and the picks of a row do not
    # depend on the rows beside it
    sampled = _sample(packed, counts, start, n, M)
    primary, fallback = sampled[:2 * B], sampled[2 * B:]
    _, bnd = _picks(primary, k)
    cd1, cd2 = ops.chamfer(bnd[B:], bnd[:B])
    cd = cd1.mean(1) + cd2.mean(1)
    rejected = fracture_pair_rejects(kind, cd)
    both = torch.where(rejected.repeat(2).view(2 * B, 1, 1), fallback, primary)
    top, fbnd = _picks(both, k)
    record = FracturePair(kind, pair, rejected, cd, label, planes, target, cand, primary[:B], primary[B:], bnd[:B], bnd[B:])
    if erode is not None:
        record = (ErodedCurvedFracturePair if curved else ErodedFracturePair)(*record, anchor, erode, lost)
    elif anchor is not None:
        record = CurvedFracturePair(*record, anchor)
    return _finish(both, top, fbnd, twist), ok & (counts[:B] >= n) & (counts[B:2 * B] >= n), record


def _cols(*widths):
    """Column slices of a staging row that holds blocks of these widths side by side."""
    c = np.cumsum((0,) + widths)
    return [slice(int(lo), int(hi)) for lo, hi in zip(c[:-1], c[1:])]


def _plane_cols(K):             # normals, offsets, start fractions, twist
    return _cols(3 * K, K, 2, 6)


def _solid_cols(K):             # (rot, shift) candidates, start fractions, twist
    return _cols(6 * K, 2, 6)


def _double_cols(K):            # plane 1: normals, offsets; plane 2: normals, offsets; uniforms; twist
    return _cols(3 * K, K, 3 * ops.DOUBLE_CUT_TRIES, ops.DOUBLE_CUT_TRIES, ops.DOUBLE_CUT_UNIFORMS, 6)


def _draw_twist(gen, mag, out):                                                 # transforms.py:163-168
    x = torch.randn(out.shape[0], 6, generator=gen, dtype=torch.float64)
    out[:] = (x / x.norm(p=2, dim=1, keepdim=True) * mag).numpy()


# The host draws of one feeder batch, per mode: (rng: np.random.RandomState, gen: torch.Generator, B, K candidates, mag, out:
# the [B, width] float64 staging row as a numpy array).  No GPU is needed.  The calls made on rng and gen, their shapes and
# their order are what a seed MEANS (tests/test_datapipe_cpu.py restates them).
def draw_plane_batch(rng, gen, B, K, mag, out):
    normals, zs, u, tw = _plane_cols(K)
    out[:, normals] = rng.rand(B, 3 * K)                                        # plane normals, dataset.py:767
    out[:, zs] = rng.rand(B, K) / 3                                             # plane offsets, :769
    out[:, u] = rng.rand(B, 2)                                                  # FPS start points as fractions of the piece sizes, :1153
    _draw_twist(gen, mag, out[:, tw])


def draw_solid_batch(rng, gen, B, K, mag, out):
    params, u, tw = _solid_cols(K)
    out[:, params] = solid_draws(rng, B, K).reshape(B, 6 * K)                   # dataset.py:718, 732-733, 749
    out[:, u] = rng.rand(B, 2)                                                  # FPS start points as fractions of the piece sizes, :1153
    _draw_twist(gen, mag, out[:, tw])


def draw_double_batch(rng, gen, B, K, mag, out):
    normals1, zs1, normals2, zs2, u, tw = _double_cols(K)
    T = ops.DOUBLE_CUT_TRIES
    out[:, normals1] = rng.rand(B, 3 * K)                                       # plane 1: normals, dataset.py:767
    out[:, zs1] = rng.rand(B, K) / 3                                            # plane 1: offsets, :769
    out[:, normals2] = rng.rand(B, 3 * T)                                       # plane 2: the draw of :1226 / :1296 and its six re-draws
    out[:, zs2] = rng.rand(B, T) / 3
    out[:, u] = rng.rand(B, ops.DOUBLE_CUT_UNIFORMS)                            # u_seed, u_se, u_choice, u_sU, u_sD, u_sFU, u_sFD
    _draw_twist(gen, mag, out[:, tw])


# The builders: the uploaded staging row d [B, width] -> (the 8-tuple, ok, the PairBatch fields that say what was cut)
def _build_plane(f, d):
    B, K = d.shape[0], f.K
    normals, zs, u, tw = _plane_cols(K)
    tensors, ok, plane = cut_pairs(f.raw, d[:, normals].reshape(B, K, 3), d[:, zs], d[:, u], d[:, tw], n=f.n, k=f.k)
    return tensors, ok, dict(plane=(plane[:, :3], plane[:, 3]))


def _build_solid(f, d):
    B, K = d.shape[0], f.K
    params, u, tw = _solid_cols(K)
    tensors, ok, chosen = cut_pairs_solid(f.raw, f.cut, d[:, params].reshape(B, K, 6), d[:, u], d[:, tw], n=f.n, k=f.k)
    return tensors, ok, dict(cut=(f.cut, chosen[:, :3], chosen[:, 3:]))


def _build_double(f, d):
    B, K, T = d.shape[0], f.K, ops.DOUBLE_CUT_TRIES
    normals1, zs1, normals2, zs2, u, tw = _double_cols(K)
    tensors, ok, record = cut_pairs_double(f.raw, d[:, normals1].reshape(B, K, 3), d[:, zs1], d[:, normals2].reshape(B, T, 3),
                                           d[:, zs2], d[:, u], d[:, tw], n=f.n, k=f.k)
    return tensors, ok, dict(double=record, plane=(record.planes[:, 0, :3], record.planes[:, 0, 3]))


_FeederMode = collections.namedtuple("_FeederMode", "cols draw build")
_PLANE_MODE = _FeederMode(_plane_cols, draw_plane_batch, _build_plane)
_SOLID_MODE = _FeederMode(_solid_cols, draw_solid_batch, _build_solid)
_DOUBLE_MODE = _FeederMode(_double_cols, draw_double_batch, _build_double)


class PairBatch(list):
    """The 8-tuple of a training batch + `ready`: the event behind which its tensors exist (they were produced on the
    feeder's stream), + `ok` [B] (a valid cut was among the candidates)."""
    ready = None
    ok = None
    plane = None      # (normal [B,3], z [B]) float64: the plane each sample was cut with (cut="plane")
    cut = None        # (kind, rot [B,3], shift [B,3]) float64: the solid each sample was cut with (cut=a solid)
    double = None     # DoubleCut: kind, planes, region tables, the acceptance test's outcome (split_twice=True)
    fracture = None   # FracturePair: kind, labels of the pair, the acceptance test's outcome, the fracture itself (pieces=...)


class PairFeeder:
    """What the reference's DataLoader(num_workers=64) over CADDataset + MovedCADDataset2 does for the trainer (train.py:101-104,
    dataset.py:1165-1190, 98-105): a FRESH batch of pairs per step from resident raw clouds - plane cut with re-draw, FPS of
    both pieces to n points, boundary labels, random rigid motion - built by cut_pairs on a background stream, so that batch
    k + 1 is cut and sampled while step k trains.  The host part of a batch is a handful of draws (K candidate planes, two
    uniform numbers for the FPS start points, a twist) from PRIVATE generators and one pinned, asynchronous upload: nothing
    in next_batch() waits for the device.  engine.TrainStep.step(next_batch=feeder.next_batch()) orders its streams behind
    `ready` and keeps the tensors alive across the streams that read them.
    split_twice=True (cut="plane" only): the reference's `train.py --random_slice`, i.e. CADDataset(split_twice=True) - the
    double cuts of dataset.py:1203-1355 by cut_pairs_double, with n_rich = 3000 n / 1024; batch.double says what was cut.
    pieces=P or (lo, hi) (cut="plane", split_twice=False only; 2 <= lo <= hi <= 16): pairs cut out of a fracture - every sample
    is cut into lo + floor(u (hi - lo + 1)) pieces (u drawn per sample on the host) and one pair of final pieces is taken, the
    two sides of the last cut or, for a share `neighbours` of the samples, a drawn pair with those two as its fallback
    (fracture_pair_rule, cut_pairs_fracture); batch.fracture says what was cut and batch.plane stays None.
    curvature=c (with pieces only; c >= 0, finite): c > 0 breaks along curved surfaces, paraboloids through the anchor with
    principal curvatures drawn in [-c, c] (fracture_pair_curved_rule; 2.0 is the curvature of the reference's radius-0.5 sphere);
    batch.fracture is then a CurvedFracturePair.  0.0 is the plane mode: its staging columns, its draws, its bits.
    erosion=e, chip=(depth, radius) (with pieces only; finite, >= 0): material is lost along every cut - per step a band
    w_up, w_dn ~ U[0, e) and a chip of depth ~ U[0, depth) within rho ~ U[0, radius) of the anchor (fracture_pair_eroded_rule,
    draw_erosion) - so the pairs no longer mate perfectly; batch.fracture is then an ErodedFracturePair or
    ErodedCurvedFracturePair.  The mode has 4 (P - 1) more staging columns, drawn from rng after the mode's other draws.  erosion
    0 or None with no chip keeps the modes above: their staging columns, their draws, their bits."""

    def __init__(self, raw, device, n=1024, k=128, mag=0.8, candidates=16, seed=0, cut="plane", split_twice=False, pieces=None,
                 neighbours=0.5, curvature=None, erosion=None, chip=None):
        if cut != "plane" and cut not in ops.SOLID_KINDS:
            raise _lib.PznError(f"PairFeeder: cut={cut!r} (one of 'plane', 'sphere', 'cylinder', 'cone')")
        if split_twice and cut != "plane":
            raise _lib.PznUnsupported(f"PairFeeder: split_twice=True cuts with planes (cut={cut!r})")
        if pieces is not None:
            if cut != "plane" or split_twice:
                raise _lib.PznUnsupported(f"PairFeeder: pieces={pieces!r} fractures with planes, one pair per sample "
                                          f"(cut={cut!r}, split_twice={bool(split_twice)})")
            lo, hi = (pieces, pieces) if isinstance(pieces, (int, np.integer)) else pieces
            lo, hi = int(lo), int(hi)
            if not 2 <= lo <= hi <= 16:
                raise _lib.PznUnsupported(f"PairFeeder: pieces={pieces!r} (an int P or a pair (lo, hi), 2 <= lo <= hi <= 16)")
            pieces = (lo, hi)
        if not 0.0 <= float(neighbours) <= 1.0:
            raise _lib.PznError(f"PairFeeder: neighbours={neighbours!r} (a share of the samples, in [0, 1])")
        if curvature is not None:
            if pieces is None:
                raise _lib.PznUnsupported(f"PairFeeder: curvature={curvature!r} bends the cuts of a fracture (pieces=...)")
            if not isinstance(curvature, (int, float, np.integer, np.floating)) or not 0.0 <= float(curvature) < np.inf:
                raise _lib.PznError(f"PairFeeder: curvature={curvature!r} (the largest principal curvature, finite and >= 0)")
        if (erosion is not None or chip is not None) and pieces is None:
            raise _lib.PznUnsupported(f"PairFeeder: erosion={erosion!r}, chip={chip!r} erode the cuts of a fracture (pieces=...)")
        self.erosion, self.chip, eroded = _erosion_args("PairFeeder", erosion, chip)
        self.curvature = 0.0 if curvature is None else float(curvature)
        self.pieces, self.neighbours = pieces, float(neighbours)
        self.cut, self.split_twice = cut, bool(split_twice)
        raw = torch.as_tensor(raw, dtype=torch.float32)
        if raw.dim() != 3 or raw.shape[2] != 3:
            raise _lib.PznError("PairFeeder: raw clouds as [B, M, 3]")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.PznError("PairFeeder runs on the GPU (puzzlenet_amd has no CPU fallback)")
        self.raw = raw.to(self.device).contiguous()
        self.n, self.k, self.mag, self.K = int(n), int(k), float(mag), int(candidates)
        self.rng = np.random.RandomState(seed)
        self.gen = torch.Generator().manual_seed(seed)
        self.stream = torch.cuda.Stream(device=self.device)
        B = self.raw.shape[0]
        self._mode = _DOUBLE_MODE if self.split_twice else (_PLANE_MODE if cut == "plane" else _SOLID_MODE)
        if self.pieces is not None:
            self._mode = (_fracture_pair_curved_mode(*self.pieces, self.curvature) if self.curvature > 0.0 else
                          _fracture_pair_mode(*self.pieces))
            if eroded:
                self._mode = _eroded_mode(self._mode, self.pieces[1], self.erosion, self.chip)
        # one pinned staging block per batch in flight (two: the upload of batch k + 1 may still be queued when k + 2 is drawn)
        self._width = self._mode.cols(self.K)[-1].stop
        self._stage = [torch.empty((B, self._width), dtype=torch.float64, pin_memory=True) for _ in range(3)]
        self._turn = 0
        self._busy = [None] * 3

    def next_batch(self):
        st = self._stage[self._turn]
        if self._busy[self._turn] is not None:
            self._busy[self._turn].synchronize()          # (three batches back: long done)
        self._mode.draw(self.rng, self.gen, self.raw.shape[0], self.K, self.mag, st.numpy())
        with torch.cuda.stream(self.stream):
            d = st.to(self.device, non_blocking=True)
            up_ev = torch.cuda.Event()
            up_ev.record(self.stream)
            self._busy[self._turn] = up_ev
            tensors, ok, what = self._mode.build(self, d)
            ready = torch.cuda.Event()
            ready.record(self.stream)
        self._turn = (self._turn + 1) % 3
        out = PairBatch(tensors)
        out.ready, out.ok = ready, ok
        for field, value in what.items():
            setattr(out, field, value)
        return out

    def close(self):
        self.stream.synchronize()
        self._busy = [None] * 3


# ---------------------------------------------------------------------------------------------------------------------
# Double-cut variants (dataset.py:1203-1355) and BuildingDataset (:1370-1429)
#
# Every pair the reference's `CADDataset.__getitem__` can return is (U, D) = two point sets defined by the sides of at
# most two planes: plane 1 cuts the cloud into up / down (:1208), plane 2 cuts `up` (slice_seed 1) or `down`
# (slice_seed 2) into uppc / downpc (:1222, :1296).  A REGION is a set of (side of plane 1, side of plane 2) cells,
# written as a 4-bit table with bit 2*s1 + s2 (s = 1: dis >= 0); a piece is an ordered list of up to two regions
# (np.vstack((other, down)) at :1237 keeps `other` first: the order decides which point a start index names).
UP, DOWN = 0b1100, 0b0011                      # sides of plane 1, either side of plane 2
UP_UPPC, UP_DOWNPC = 0b1000, 0b0100            # plane 2 inside `up`
DOWN_UPPC, DOWN_DOWNPC = 0b0010, 0b0001        # plane 2 inside `down`


def _compact_segments(raw, seg, cap):
    """Rows with seg 0, then rows with seg 1 (original order inside each), padded to `cap` with copies of the first
    kept row; seg 2 = left out.  -> (packed [B,cap,3], count [B])"""
    count = (seg < 2).sum(1)
    order = torch.sort(seg.to(torch.int8), dim=1, stable=True)[1]
    packed = torch.gather(raw, 1, order[:, :cap].unsqueeze(-1).expand(-1, -1, 3))
    pos = torch.arange(cap, device=raw.device).unsqueeze(0)
    first = packed[:, :1, :]
    return torch.where((pos < count.unsqueeze(1)).unsqueeze(-1), packed, first.expand(-1, cap, -1)).contiguous(), count


def _segments(code, tab):
    """code [B,M] in 0..3, tab [B,2] region tables -> segment id 0 / 1 / 2 (left out) per point."""
    in0 = (tab[:, 0:1] >> code) & 1
    in1 = (tab[:, 1:2] >> code) & 1
    return torch.where(in0 == 1, torch.zeros_like(code), torch.where(in1 == 1, torch.ones_like(code), torch.full_like(code, 2)))


def pairs_from_pieces(U, D, twist, k=128):
    """(U, D) N-point pieces -> the 8-tuple of MovedCADDataset2.__getitem__ (:98-105) on top of get_boundary(D, U)
    (:1357-1367): (D, moved U, igt, U, D boundary, U boundary, D mask, U mask)."""
    Db, Ub, Dm, Um = boundary(D, U, k)
    moved, igt = move(U, twist)
    return D, moved, igt, U, Db, Ub, Dm, Um


def make_pairs_regions(raw, normal1, z1, normal2, z2, u_tab, d_tab, start_u, start_d, twist, n=1024, k=128, cap=None):
    """The general form of make_pairs: raw [B,M,3] on the GPU, two planes per sample, and for each of the two pieces an
    ordered pair of region tables (u_tab, d_tab: int64 [B,2]; a second table of 0 = single region).  U = FPS(n) of the
    points of u_tab from start_u, D likewise; -> (8-tuple, ok [B]).  The single cut is u_tab = (UP, 0), d_tab = (DOWN, 0)."""
    if not raw.is_cuda:
        raise _lib.PznError("datapipe.make_pairs_regions runs on the GPU (puzzlenet_amd has no CPU fallback)")
    raw = raw.to(torch.float32).contiguous()
    B, M, _ = raw.shape
    cap = M if cap is None else int(cap)
    s1 = plane_cut_mask(raw, normal1, z1)
    s2 = plane_cut_mask(raw, normal2, z2)
    code = 2 * s1.to(torch.int64) + s2.to(torch.int64)
    u_piece, n_u = _compact_segments(raw, _segments(code, u_tab.to(raw.device)), cap)
    d_piece, n_d = _compact_segments(raw, _segments(code, d_tab.to(raw.device)), cap)
    ok = (n_u >= n) & (n_d >= n) & (n_u <= cap) & (n_d <= cap)
    both = fps_to_n(torch.cat([u_piece, d_piece], 0), torch.cat([n_u, n_d], 0),
                    torch.cat([start_u.reshape(-1), start_d.reshape(-1)], 0), n)
    U, D = both[:B].contiguous(), both[B:].contiguous()
    return pairs_from_pieces(U, D, twist, k), ok


def building_pairs(fpcs, rpcs, twist, k=128):
    """BuildingDataset.__getitem__ (:1423-1429) for a batch: the item is (rpc, fpc, get_boundary(fpc, rpc)), i.e. U = the
    roof cloud, D = the facade cloud, both given (no cut, no sampling); -> the 8-tuple of MovedCADDataset2 on top."""
    if not (fpcs.is_cuda and rpcs.is_cuda):
        raise _lib.PznError("datapipe.building_pairs runs on the GPU (puzzlenet_amd has no CPU fallback)")
    return pairs_from_pieces(rpcs.to(torch.float32).contiguous(), fpcs.to(torch.float32).contiguous(), twist, k)


# The double cut as the FEEDER samples it (PairFeeder(split_twice=True)): the same decision tree from draws made up front.
SINGLE, HALF_VS_REST, HALF_VS_OTHER, HALVES = range(4)       # `kind` codes (ops.DOUBLE_CUT_KINDS names them as the plan does)
CD_ACCEPT = 0.015                                            # dataset.py:1255, :1322


def double_cut_rejects(kind, cd):
    """Step 8 of double_cut_rule (numpy arrays or tensors): the pair is replaced by its fallback."""
    return (kind == HALF_VS_OTHER) & (cd > CD_ACCEPT)


def _value64(pts, plane):
    """p . normal + z as plane_cut_mask and the kernels evaluate it: float64, every operation individually rounded,
    ((x n0 + y n1) + z n2) + offset.  pts [M,3] float32, plane [4] float64 -> float64 [M]"""
    p = np.asarray(pts, dtype=np.float32).astype(np.float64)
    plane = np.asarray(plane, dtype=np.float64)
    return ((p[:, 0] * plane[0] + p[:, 1] * plane[1]) + p[:, 2] * plane[2]) + plane[3]


def _side64(pts, plane):
    """side(p, plane) = (_value64 >= 0).  pts [M,3] float32, plane [4] float64 -> bool [M]"""
    return _value64(pts, plane) >= 0


def region_rows(raw, code, tab):
    """Rows of the piece tab = (first region table, second): the points whose cell `code` is in the first, then the others whose
    cell is in the second, each in the cloud's order (_segments + _compact_segments without the padding).  numpy."""
    in0 = ((int(tab[0]) >> code) & 1) == 1
    in1 = (((int(tab[1]) >> code) & 1) == 1) & ~in0
    return np.concatenate([raw[in0], raw[in1]], axis=0)


def double_cut_rule(raw, planes1, planes2, u, n=1024, n_rich=3000, cap=None):
    """The sampling rule of PairFeeder(split_twice=True) for ONE sample, in numpy on the host, float64: the statement that
    pzn_cut_compact_double_f32 (steps 1-7) and cut_pairs_double (step 8) implement and the tests hold them to.  It reproduces
    the DISTRIBUTION of CADDataset.__getitem__ with split_twice=True (dataset.py:1203-1355) from draws made up front; it does not
    replay the reference's generator order (plan_double_cut_like_reference does).
      raw      [M,3] float32
      planes1  [K,4] float64: K candidates (normal = rand(3), z = rand() / 3) for plane 1, as the plane feeder draws them
      planes2  [7,4] float64: the first draw of plane 2 and the six re-draws of `while time <= 5` (:1227, :1300)
      u        [7] uniforms: u_seed, u_se, u_choice, u_sU, u_sD, u_sFU, u_sFD
      n        points per piece, where the reference hard-wires 1024
      n_rich   points a piece must hold to be cut again: the reference's 3000 (:1214-1217).  The reference only exists at
               n = 1024; the feeder scales the threshold with n and passes 3000 n // 1024
      cap      rows a piece may hold (None: M)
    The rule:
      1. a = |up|, b = M - a by plane-1 candidate 0.
      2. seed = min(2, floor(3 u_seed)); seed 1 with a < n_rich becomes 2; THEN seed 2 with b < n_rich becomes 1 (:1214-1217).
      3. seed 0: SINGLE.
      4. inner = up (seed 1) or down (seed 2), the other piece holds c points; the first of the 7 plane-2 candidates that leaves
         >= n points on both sides within inner gives uppc (side 1) / downpc (side 0); none: SINGLE.
      5. se = min(2, floor(3 u_se)), choice = min(1, floor(2 u_choice)):
         se 0 or c < n: HALF_VS_REST, U = the chosen half, D = the other half's rows, then the other piece's (np.vstack, :1239);
         se 1: HALF_VS_OTHER, U = the chosen half, D = the other piece; fallback pair = (up, down) of plane-1 candidate 0 (valid:
               inner holds >= 2 n points and c >= n);
         se 2: HALVES, U = uppc, D = downpc (the `re_now` branch only makes draws whose results it overwrites, :1283-1285).
      6. SINGLE: U = up, D = down of the first plane-1 candidate, counted from 0, with >= n points on both sides (`self.slice`
         starting from the split already made); none: the most balanced one, the first among equals, ok = False.
      7. start = clamp(floor(u count), 0, count - 1) with u_sU, u_sD for U, D and u_sFU, u_sFD for the fallback pieces.
      8. (on the sampled pieces, so not here: double_cut_rejects) HALF_VS_OTHER only: cd = mean(cd1) + mean(cd2) of the chamfer
         distances between the two 128-point boundaries of get_boundary(D, U); cd > 0.015: the fallback pair, sampled from its
         own start indices, replaces the pair (:1253-1256, :1320-1323).
    -> dict(kind, planes [2,4] (plane 2 zero for SINGLE), u_tab [2], d_tab [2], pieces: [U, D, fallback U, fallback D] row
       arrays (None where there is no fallback), counts [4] (-1 there), start [4], ok)"""
    raw = np.asarray(raw, dtype=np.float32)
    planes1, planes2, u = (np.asarray(t, dtype=np.float64) for t in (planes1, planes2, u))
    M, K = raw.shape[0], planes1.shape[0]
    cap = M if cap is None else int(cap)
    s1 = _side64(raw, planes1[0])
    a = int(s1.sum())
    b = M - a
    seed = min(2, int(np.floor(3 * u[0])))
    if seed == 1 and a < n_rich:
        seed = 2
    if seed == 2 and b < n_rich:
        seed = 1
    kind, p1, p2 = SINGLE, planes1[0], np.zeros(4)
    u_tab, d_tab = (UP, 0), (DOWN, 0)
    if seed != 0:
        inner = s1 if seed == 1 else ~s1
        c = M - int(inner.sum())
        for t in range(planes2.shape[0]):
            s2 = _side64(raw, planes2[t])
            if int((inner & s2).sum()) >= n and int((inner & ~s2).sum()) >= n:
                A, Bt, other = (UP_UPPC, UP_DOWNPC, DOWN) if seed == 1 else (DOWN_UPPC, DOWN_DOWNPC, UP)
                se, choice = min(2, int(np.floor(3 * u[1]))), min(1, int(np.floor(2 * u[2])))
                first, second = (A, Bt) if choice == 0 else (Bt, A)
                if se == 0 or c < n:
                    kind, u_tab, d_tab = HALF_VS_REST, (first, 0), (second, other)
                elif se == 1:
                    kind, u_tab, d_tab = HALF_VS_OTHER, (first, 0), (other, 0)
                else:
                    kind, u_tab, d_tab = HALVES, (A, 0), (Bt, 0)
                p2 = planes2[t]
                break
    ok = True
    if kind == SINGLE:
        ups = [a] + [int(_side64(raw, planes1[k]).sum()) for k in range(1, K)]
        valid = [k for k in range(K) if ups[k] >= n and M - ups[k] >= n]
        ok = bool(valid)
        pick = valid[0] if valid else int(np.argmax([min(x, M - x) for x in ups]))      # (argmax: the first among equals)
        p1 = planes1[pick]
    code = 2 * _side64(raw, p1).astype(np.int64) + _side64(raw, p2).astype(np.int64)
    tabs = [u_tab, d_tab] + ([(UP, 0), (DOWN, 0)] if kind == HALF_VS_OTHER else [])
    pieces = [region_rows(raw, code, t) for t in tabs] + [None] * (4 - len(tabs))
    counts = np.array([-1 if r is None else len(r) for r in pieces], dtype=np.int64)
    start = np.array([0 if cnt < 0 else max(0, min(cnt - 1, int(np.floor(u[3 + i] * cnt)))) for i, cnt in enumerate(counts)],
                     dtype=np.int64)
    return dict(kind=kind, planes=np.stack([p1, p2]), u_tab=np.array(u_tab, np.int64), d_tab=np.array(d_tab, np.int64),
                pieces=pieces, counts=counts, start=start, ok=bool(ok and counts.max() <= cap))


# ---------------------------------------------------------------------------------------------------------------------
# Fracture: a cloud cut into P pieces with known answers (no counterpart in the reference, which ships pairs only) - the input
# of assembly.py's multi-piece walks and, with assembly.evaluate, their score.

def _start_index(u, cnt):
    """start_index of csrc/pzn_cut.h: floor(u cnt) held to [0, cnt - 1] (0 for an empty piece)."""
    return max(0, min(int(cnt) - 1, int(np.floor(np.float64(u) * np.float64(cnt)))))


def _pad_rows(rows, cap, first_of_cloud):
    """pad_piece of csrc/pzn_cut.h: the first `cap` rows of a piece, rows beyond its count copies of its first row (of the
    cloud's first row when it is empty).  -> [cap,3] float32"""
    keep = rows[:cap]
    fill = rows[0] if len(rows) else first_of_cloud
    return np.concatenate([keep, np.broadcast_to(fill, (cap - len(keep), 3))], axis=0).astype(np.float32)


def fracture_rule(raw, normals, u_anchor, u_start, P, n_min, cap=None):
    """The fracture of ONE sample, in numpy on the host: the statement that pzn_fracture_f32 (csrc/fracture.hip) implements and
    the tests hold it to, bit for bit.
      raw       [M,3] float32
      normals   [P-1,K,3] float64: unit vectors, K candidates per cut
      u_anchor  [P-1,K] float64 uniforms in [0,1): which point of the target a candidate plane goes through
      u_start   [P] float64 uniforms in [0,1): the FPS start of every piece
      n_min     points both sides of a cut must hold;  cap: rows a piece may hold (None: M)
    All points start with label 0.  Step s = 1 .. P-1:
      1. the target t is the label with the most points among 0 .. s-1 (ties: the lowest label);
      2. candidate k is the plane with normal normals[s-1,k] through the ANCHOR, the r-th point of the target in the cloud's
         order, r = start_index(u_anchor[s-1,k], count[t]) (a plane through one of the target's own points always meets it);
      3. its offset is -((x n0 + y n1) + z n2) of the anchor, float64, every operation rounded on its own, and the side test
         is _side64's expression: the anchor itself evaluates to exactly 0 and is on the up side;
      4. the FIRST candidate that leaves >= n_min target points on both sides is taken; none: the most balanced one, the first
         among equals (the single cut's rule);
      5. the up side keeps label t, the down side becomes label s.
    -> dict(label [M] uint8, counts [P] int64, pieces: P arrays [cap,3] (the rows of a label in the cloud's order, padded as
       pad_piece does; an empty piece is the cloud's first row throughout), order [M] int32 (the cloud row of every position of
       the concatenated pieces = the stable argsort of label), start [P] int64 = start_index(u_start[p], counts[p]),
       planes [P-1,4] float64, target [P-1] int32, cand [P-1] int32, ok: every step had a valid candidate and every count <= cap)"""
    raw = np.asarray(raw, dtype=np.float32)
    normals, u_anchor, u_start = (np.asarray(t, dtype=np.float64) for t in (normals, u_anchor, u_start))
    r = _fracture_pieces(raw, _plane_side(normals), u_anchor, u_start, int(P), n_min, cap)
    del r["anchor"], r["lost"]
    return r


def _fracture_pieces(raw, side, u_anchor, u_start, P, n_min, cap, erode=None):
    """fracture_rule / fracture_curved_rule / fracture_eroded_rule behind their argument conversions: the steps with `side` and
    `erode` (see _fracture_steps), then the pieces.  -> the rule's dict with anchor [P-1] int32, the cloud row of the anchor taken
    at every step, and lost [P-1] int32, the points lost at every step (zero without erosion)"""
    M = raw.shape[0]
    cap = M if cap is None else int(cap)
    label, planes, target, cand, anchor, lost, ok = _fracture_steps(raw, side, u_anchor, P, P - 1, n_min, erode)
    counts = np.bincount(label, minlength=P)[:P].astype(np.int64)
    order = np.argsort(label, kind="stable").astype(np.int32)
    pieces = [_pad_rows(raw[label == p], cap, raw[0]) for p in range(P)]
    start = np.array([_start_index(u_start[p], counts[p]) for p in range(P)], dtype=np.int64)
    return dict(label=label, counts=counts, pieces=pieces, order=order, start=start, planes=planes, target=target, cand=cand,
                anchor=anchor, lost=lost, ok=bool(ok and counts.max() <= cap))


def _plane_side(normals):
    """The side function of fracture_rule: normals [P-1,K,3] float64 -> side(s, k, a, pts) with a [3] float64 the anchor and pts
    [m,3] float32 the target's points -> (the plane [4] through a with normal normals[s,k], up [m] bool = f >= 0, f [m] float64 =
    _value64, the value whose sign is taken)"""
    def side(s, k, a, pts):
        n = normals[s, k]
        plane = np.array([n[0], n[1], n[2], -((a[0] * n[0] + a[1] * n[1]) + a[2] * n[2])])
        f = _value64(pts, plane)
        return plane, f >= 0, f
    return side


def quadric_value(pts, a, frame, half_curv):
    """f of fracture_curved_rule: pts [m,3] float32, a [3] float64 the anchor, frame [3,3] float64 (rows e1, e2, n), half_curv [2]
    float64 (c1, c2) -> f [m] float64 = (h + (c1 s1) s1) + (c2 s2) s2 with d = pts - a (the float32 coordinates widened, three
    subtractions), s1 = (d0 e1[0] + d1 e1[1]) + d2 e1[2], s2 and h likewise with e2 and n; every operation rounded on its own."""
    p = np.asarray(pts, dtype=np.float32).astype(np.float64)
    d0, d1, d2 = p[:, 0] - a[0], p[:, 1] - a[1], p[:, 2] - a[2]
    s1, s2, h = ((d0 * e[0] + d1 * e[1]) + d2 * e[2] for e in frame)
    return (h + (half_curv[0] * s1) * s1) + (half_curv[1] * s2) * s2


def _quadric_side(frames, half_curv):
    """The side function of fracture_curved_rule: frames [P-1,K,3,3], half_curv [P-1,K,2] float64 -> side(s, k, a, pts) as
    _plane_side's -> (the TANGENT plane [4] at a, (n, -((ax n0 + ay n1) + az n2)), up [m] bool = f >= 0, f = quadric_value)"""
    def side(s, k, a, pts):
        n = frames[s, k, 2]
        plane = np.array([n[0], n[1], n[2], -((a[0] * n[0] + a[1] * n[1]) + a[2] * n[2])])
        f = quadric_value(pts, a, frames[s, k], half_curv[s, k])
        return plane, f >= 0, f
    return side


def _fracture_steps(raw, side, u_anchor, P, steps, n_min, erode=None):
    """Steps s = 1 .. steps (<= P - 1) of fracture_rule on raw [M,3] float32; u_anchor [P-1,K] float64; side(s - 1, k, anchor,
    target points) -> (the plane recorded for candidate k, its up side, the value f whose sign that is): _plane_side or
    _quadric_side.  erode [P-1,4] float64 = (w_up, w_dn, depth, rho) per step, or None: the steps of fracture_eroded_rule, where a
    member of the target is lost (label FRACTURE_LOST) iff -w_dn < f < w_up, or -depth < f < depth and r2 < rho rho, a candidate
    is judged by what it leaves on both sides, and a step whose target is empty is not made.
    -> (label [M] uint8, planes [P-1,4], target [P-1], cand [P-1], anchor [P-1] (the cloud row of the anchor taken), lost [P-1]
    (the points lost) with the rows of the steps not made zero, every step had a valid candidate)"""
    M, K = raw.shape[0], u_anchor.shape[1]
    p64 = raw.astype(np.float64)
    label = np.zeros(M, dtype=np.uint8)
    planes = np.zeros((P - 1, 4), dtype=np.float64)
    target, cand, anchor, lost = (np.zeros(P - 1, dtype=np.int32) for _ in range(4))
    ok = True
    for s in range(1, steps + 1):
        count = np.bincount(label, minlength=P)[:P]                   # (the lost points are counted for no label)
        t = int(np.argmax(count[:s]))                                 # (argmax: the first among equals)
        members = np.flatnonzero(label == t)
        n_t = len(members)
        target[s - 1] = t
        if n_t == 0:                                                  # everything has been lost: the step is not made
            ok = False
            continue
        best = None
        for k in range(K):
            row = members[_start_index(u_anchor[s - 1, k], n_t)]
            plane, up, f = side(s - 1, k, p64[row], raw[members])
            gone = np.zeros(n_t, dtype=bool)
            if erode is not None:
                w_up, w_dn, depth, rho = erode[s - 1]
                d = p64[members] - p64[row]
                r2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
                gone = ((f < w_up) & (f > -w_dn)) | ((f < depth) & (f > -depth) & (r2 < rho * rho))
            n_up, n_dn = int((up & ~gone).sum()), int((~up & ~gone).sum())
            valid = n_up >= n_min and n_dn >= n_min
            if valid or best is None or min(n_up, n_dn) > best[0]:
                best = (min(n_up, n_dn), k, plane, up, row, gone)
            if valid:
                break
        else:
            ok = False
        _, cand[s - 1], planes[s - 1], up, anchor[s - 1], gone = best
        label[members[~up]] = s
        label[members[gone]] = FRACTURE_LOST
        lost[s - 1] = gone.sum()
    return label, planes, target, cand, anchor, lost, ok


def fracture_curved_rule(raw, frames, half_curv, u_anchor, u_start, P, n_min, cap=None):
    """fracture_rule along curved surfaces: the statement that pzn_fracture_curved_f32 (csrc/fracture.hip) implements and the tests
    hold it to, bit for bit.  Candidate k of step s is a second-order patch through the anchor a, a paraboloid in a tangent frame:
      frames     [P-1,K,3,3] float64: an orthonormal frame (rows e1, e2, n) per candidate, taken as given
      half_curv  [P-1,K,2] float64: c1 = kappa1 / 2, c2 = kappa2 / 2 - a bowl (c1 c2 > 0), a cylinder (c2 = 0), a saddle
                 (c1 c2 < 0), the plane with normal n (0, 0)
    and a point is on the up side iff quadric_value >= 0 (float64, every operation rounded on its own): the anchor has d = 0, so it
    evaluates to exactly 0 and is on the up side, and the surface always meets the target.  Steps 1, 2, 4 and 5 of fracture_rule -
    the target, the anchor's rank from u_anchor, the first valid candidate else the first most balanced one, up keeps t and down
    becomes s - and the other arguments are unchanged.
    -> fracture_rule's dict, where planes [P-1,4] is the TANGENT plane at the anchor, (n, -((ax n0 + ay n1) + az n2)), and with
       anchor [P-1] int32, the cloud row of the anchor taken at every step"""
    raw = np.asarray(raw, dtype=np.float32)
    frames, half_curv, u_anchor, u_start = (np.asarray(t, dtype=np.float64) for t in (frames, half_curv, u_anchor, u_start))
    r = _fracture_pieces(raw, _quadric_side(frames, half_curv), u_anchor, u_start, int(P), n_min, cap)
    del r["lost"]
    return r


FRACTURE_LOST = ops.FRACTURE_LOST                            # the label of a point lost along a cut


def _eroded_side(who, normals, frames, half_curv):
    """The side function of the eroded rules: _plane_side of normals, or _quadric_side of frames and half_curv with normals=None"""
    if _curved(who, normals, frames, half_curv):
        return _quadric_side(np.asarray(frames, dtype=np.float64), np.asarray(half_curv, dtype=np.float64))
    return _plane_side(np.asarray(normals, dtype=np.float64))


def fracture_eroded_rule(raw, normals, u_anchor, u_start, erode, P, n_min, cap=None, frames=None, half_curv=None):
    """fracture_rule (normals) or fracture_curved_rule (frames and half_curv, with normals=None) with EROSION - at every cut the
    target's points close to the taken surface are lost and belong to no piece: the statement that pzn_fracture_eroded_f32
    (csrc/fracture.hip) implements and the tests hold it to, bit for bit.
      erode  [P-1,4] float64 = (w_up, w_dn, depth, rho) per step, taken as given
    For candidate k of step s through the anchor a, f is the value whose sign the side test takes (_value64 of the plane through
    a, quadric_value), float64, every operation rounded on its own.  A member x of the target is LOST under that candidate iff
      band: -w_dn < f < w_up, or
      chip: -depth < f < depth and r2 < rho rho, with d = x - a (the float32 coordinates widened, three subtractions) and
            r2 = (d0 d0 + d1 d1) + d2 d2 - at the anchor, the one point known to lie on the surface.
    All comparisons are strict: zeros lose nothing, and neither does a NaN; with w_up > 0 and w_dn > 0 the anchor itself (f = 0) is lost.  Up is the
    members with f >= 0 that are not lost, down those with f < 0 that are not lost.  A candidate is valid iff BOTH hold >= n_min
    points after the loss, and its balance is the smaller of the two; the first valid candidate is taken, else the first most
    balanced one; up keeps t, down becomes s, the lost points get label FRACTURE_LOST (255) and are never counted or targeted
    again.  A step whose target holds no point (everything has been lost) is not made: its rows of planes, cand, anchor and lost
    are zero, target is t, ok is False.  f is the offset along n to the surface, so across a cut the kept points of the two sides
    are >= w_up + w_dn apart along n.
    -> the dict of the rule of its form with anchor [P-1] int32 (for planes too: the chip's centre) and lost [P-1] int32 (the
       points lost at every step); counts excludes the lost points (counts.sum() + lost.sum() == M) and order, the stable argsort
       of label, holds the lost rows behind the last piece, in the cloud's order"""
    raw = np.asarray(raw, dtype=np.float32)
    u_anchor, u_start, erode = (np.asarray(t, dtype=np.float64) for t in (u_anchor, u_start, erode))
    side = _eroded_side("fracture_eroded_rule", normals, frames, half_curv)
    return _fracture_pieces(raw, side, u_anchor, u_start, int(P), n_min, cap, erode)


def fracture_pair_eroded_rule(raw, normals, u_anchor, u, erode, pieces, P, n_min, neighbours, cap=None, frames=None, half_curv=None):
    """fracture_pair_rule (normals) or fracture_pair_curved_rule (frames and half_curv, with normals=None) with the erosion of
    fracture_eroded_rule (erode [P-1,4] float64; rows from P_b - 1 on are not read): the statement that
    pzn_fracture_pair_eroded_f32 implements.  The pair is chosen as without erosion and its pieces are the eroded ones.
    -> fracture_pair_rule's dict with anchor and lost [P-1] int32 (rows from P_b - 1 on are zero)"""
    raw = np.asarray(raw, dtype=np.float32)
    u_anchor, u, erode = (np.asarray(t, dtype=np.float64) for t in (u_anchor, u, erode))
    side = _eroded_side("fracture_pair_eroded_rule", normals, frames, half_curv)
    return _fracture_pair(raw, side, u_anchor, u, pieces, P, n_min, neighbours, cap, erode)


def draw_erosion(rng, B, P, erosion, chip=(0.0, 0.0)):
    """The erosion draws of a fracture batch -> erode [B,P-1,4] float64 = (w_up, w_dn, depth, rho) per step: one rng.rand(B, P-1, 4),
    scaled to w_up, w_dn ~ U[0, erosion), depth ~ U[0, chip[0]), rho ~ U[0, chip[1])."""
    return rng.rand(B, P - 1, 4) * np.array([erosion, erosion, chip[0], chip[1]], dtype=np.float64)


def _erosion_args(who, erosion, chip):
    """erosion and chip=(depth, radius) of the feeder and the tools: finite and >= 0 -> (erosion, (depth, radius), any of them > 0)"""
    number = (int, float, np.integer, np.floating)
    e = 0.0 if erosion is None else erosion
    c = (0.0, 0.0) if chip is None else tuple(chip)
    if not isinstance(e, number) or len(c) != 2 or not all(isinstance(v, number) for v in c) or \
            not all(0.0 <= float(v) < np.inf for v in (e,) + c):
        raise _lib.PznError(f"{who}: erosion={erosion!r}, chip={chip!r} (the widest band and the chip's (depth, radius): finite "
                            f"and >= 0)")
    e, c = float(e), (float(c[0]), float(c[1]))
    return e, c, e > 0.0 or (c[0] > 0.0 and c[1] > 0.0)


# A training pair cut out of a fracture, as the FEEDER samples it (PairFeeder(pieces=...)).
SIBLING, NEIGHBOUR = 0, 1                                    # `kind` codes (ops.FRACTURE_PAIR_KINDS names them)


def fracture_pair_rejects(kind, cd):
    """Step 8 of fracture_pair_rule (numpy arrays or tensors): the drawn pair is replaced by the sibling pair."""
    return (kind == NEIGHBOUR) & (cd > CD_ACCEPT)


def fracture_pair_rule(raw, normals, u_anchor, u, pieces, P, n_min, neighbours, cap=None):
    """The training pair of ONE sample cut out of a fracture, in numpy on the host: the statement that pzn_fracture_pair_f32
    (csrc/fracture.hip, steps 1-7) and cut_pairs_fracture (step 8) implement and the tests hold them to, bit for bit.
      raw        [M,3] float32
      normals    [P-1,K,3], u_anchor [P-1,K] float64: as fracture_rule takes them
      u          [7] float64 uniforms: u_kind, u_a, u_c, u_sU, u_sD, u_sFU, u_sFD
      pieces     P_b, this sample's number of pieces, 2 <= P_b <= P
      n_min      points both sides of a cut must hold;  cap: rows a piece may hold (None: M)
      neighbours the share of samples whose pair is drawn among all final pieces, in [0, 1]
    The rule:
      1. steps 1-5 of fracture_rule for s = 1 .. P_b - 1 (the draw rows of later steps are not read; planes, target and cand
         rows from P_b - 1 on are zero).
      2. the SIBLING pair is U = target[P_b-2], the up side of the last cut, which keeps its label, and D = P_b - 1, its down
         side: both are final pieces, and they touch along the whole of that cut.
      3. the kind is NEIGHBOUR iff P_b >= 3 and u_kind < neighbours, with a = min(P_b - 1, floor(u_a P_b)),
         c' = min(P_b - 2, floor(u_c (P_b - 1))), c = c' + (c' >= a) - an ordered pair of distinct final pieces - unless {a, c}
         is the sibling pair in either order: then, and otherwise, the kind is SIBLING.
      4. SIBLING: the primary pair is the sibling pair and there is no fallback (counts -1, pieces None, start 0, as
         double_cut_rule lays out a missing fallback).
      5. NEIGHBOUR: the primary pair is (U, D) = (a, c) and the fallback is the sibling pair.
      6. the four pieces [U, D, fallback U, fallback D] are the rows of their labels in the cloud's order, padded as pad_piece
         does; start = start_index(u_sU / u_sD / u_sFU / u_sFD, count).
      7. ok: every step made had a valid candidate and every written piece fits in cap.  With n_min = n every cut of an ok
         sample left >= n points on both sides, and a later cut of either side leaves >= n on both of its sides again, so every
         final piece - whichever pair is drawn - holds >= n points.
      8. (on the sampled pieces, so not here: fracture_pair_rejects) NEIGHBOUR only: cd = mean(cd1) + mean(cd2) of the chamfer
         distances between the two k-point boundaries; cd > CD_ACCEPT: the fallback pair, sampled from its own start indices,
         replaces the pair.
    -> dict(kind, pair [4] int32 labels (-1: none), pieces: four [cap,3] arrays (None where there is no fallback), counts [4]
       (-1 there), start [4], label [M] uint8, planes [P-1,4], target [P-1], cand [P-1], ok)"""
    raw = np.asarray(raw, dtype=np.float32)
    normals, u_anchor, u = (np.asarray(t, dtype=np.float64) for t in (normals, u_anchor, u))
    r = _fracture_pair(raw, _plane_side(normals), u_anchor, u, pieces, P, n_min, neighbours, cap)
    del r["anchor"], r["lost"]
    return r


def fracture_pair_curved_rule(raw, frames, half_curv, u_anchor, u, pieces, P, n_min, neighbours, cap=None):
    """fracture_pair_rule with the cuts of fracture_curved_rule (frames [P-1,K,3,3], half_curv [P-1,K,2] float64 in place of
    normals): the statement that pzn_fracture_pair_curved_f32 implements.  -> fracture_pair_rule's dict, where planes holds the
    tangent planes, and with anchor [P-1] int32 (rows from P_b - 1 on are zero)"""
    raw = np.asarray(raw, dtype=np.float32)
    frames, half_curv, u_anchor, u = (np.asarray(t, dtype=np.float64) for t in (frames, half_curv, u_anchor, u))
    r = _fracture_pair(raw, _quadric_side(frames, half_curv), u_anchor, u, pieces, P, n_min, neighbours, cap)
    del r["lost"]
    return r


def _fracture_pair(raw, side, u_anchor, u, pieces, P, n_min, neighbours, cap, erode=None):
    """fracture_pair_rule / fracture_pair_curved_rule / fracture_pair_eroded_rule behind their argument conversions -> the rule's
    dict with anchor and lost [P-1]"""
    M, P, Pb = raw.shape[0], int(P), int(pieces)
    if not 2 <= Pb <= P or not 0.0 <= neighbours <= 1.0 or u.shape != (7,):
        raise _lib.PznError(f"fracture_pair_rule: pieces = {Pb} of P = {P}, neighbours = {neighbours}, u {u.shape}")
    cap = M if cap is None else int(cap)
    label, planes, target, cand, anchor, lost, ok = _fracture_steps(raw, side, u_anchor, P, Pb - 1, n_min, erode)
    sibling = (int(target[Pb - 2]), Pb - 1)
    kind, pair = SIBLING, sibling + (-1, -1)
    if Pb >= 3 and u[0] < neighbours:
        a = min(Pb - 1, int(np.floor(u[1] * np.float64(Pb))))
        c = min(Pb - 2, int(np.floor(u[2] * np.float64(Pb - 1))))
        c += c >= a
        if (a, c) != sibling and (c, a) != sibling:
            kind, pair = NEIGHBOUR, (a, c) + sibling
    rows = [None if p < 0 else raw[label == p] for p in pair]
    counts = np.array([-1 if r is None else len(r) for r in rows], dtype=np.int64)
    start = np.array([0 if cnt < 0 else _start_index(u[3 + i], cnt) for i, cnt in enumerate(counts)], dtype=np.int64)
    return dict(kind=kind, pair=np.array(pair, dtype=np.int32), pieces=[None if r is None else _pad_rows(r, cap, raw[0]) for r in rows],
                counts=counts, start=start, label=label, planes=planes, target=target, cand=cand, anchor=anchor, lost=lost,
                ok=bool(ok and counts.max() <= cap))


Fracture = collections.namedtuple("Fracture", "pieces pose rest src top cd mates ok label planes target cand counts")
Fracture.__doc__ = """A K-piece sample with its answers (datapipe.fracture): pieces [B,P,n,3] the moved pieces (the model's input, [P,n,3]
per sample as assembly.match_pairs takes them), pose [B,P,4,4] the motion of every piece (pieces = pose rest), rest [B,P,n,3]
the pieces where they belong, src [B,P,n] int64 the cloud row of every sampled point, top [B,P,P,k] int64 the k rows of piece a
nearest to piece b, cd [B,P,P] float32 the chamfer distance of the two picked boundaries, mates [B,P,P] bool the pieces that
touch, ok [B] bool, and the kernel's label [B,M] uint8, planes [B,P-1,4] float64, target / cand [B,P-1] int32 and counts [B,P]
int64."""


CurvedFracture = collections.namedtuple("CurvedFracture", Fracture._fields + ("anchor", "frames", "half_curv"))
CurvedFracture.__doc__ = """Fracture along curved surfaces (datapipe.fracture(..., frames=, half_curv=)): the fields of Fracture, where planes
[B,P-1,4] holds the tangent plane at the anchor, then anchor [B,P-1] int32 (the cloud row of the anchor taken at every step) and the
frames [B,P-1,K,3,3] and half_curv [B,P-1,K,2] float64 the cuts were made with: candidate cand[b,s] of them, through
raw[b, anchor[b,s]], is the surface between target[b,s] and s + 1."""


def _curved(who, normals, frames, half_curv):
    """frames and half_curv of the fracture forms: both (-> True; the normals are not read) or neither (-> False)"""
    if (frames is None) != (half_curv is None):
        raise _lib.PznError(f"{who}: frames and half_curv come together (a curved cut), or neither (planes)")
    if frames is not None and normals is not None:
        raise _lib.PznError(f"{who}: normals with frames and half_curv (a curved cut's normal is the third row of its frame; pass "
                            f"normals=None)")
    return frames is not None


ErodedFracture = collections.namedtuple("ErodedFracture", Fracture._fields + ("anchor", "erode", "lost"))
ErodedFracture.__doc__ = """Fracture with material lost along every cut (datapipe.fracture(..., erode=)): the fields of Fracture, where label
holds ops.FRACTURE_LOST (255) for the points that belong to no piece and counts excludes them, then anchor [B,P-1] int32 (the cloud
row of the anchor taken at every step, the chip's centre), erode [B,P-1,4] float64 (the (w_up, w_dn, depth, rho) the cuts were made
with) and lost [B,P-1] int32 (the points lost at every step): counts.sum(1) + lost.sum(1) == M."""

ErodedCurvedFracture = collections.namedtuple("ErodedCurvedFracture", CurvedFracture._fields + ("erode", "lost"))
ErodedCurvedFracture.__doc__ = """CurvedFracture with material lost along every cut: then erode and lost, as ErodedFracture holds them."""


def fracture(raw, normals, u_anchor, u_start, twist, n=1024, n_min=None, k=128, cap=None, frames=None, half_curv=None,
             erode=None):
    """A batch of P-piece samples with ground truth: every cloud cut into P pieces in one launch (ops.fracture, csrc/fracture.hip;
    the rule: fracture_rule), every piece sampled to n points and moved, and which pieces touch.  raw [B,M,3] f32 on the GPU;
    normals [B,P-1,K,3], u_anchor [B,P-1,K], u_start [B,P] float64 draws (draw_fracture_batch); twist [B,P,6]; n_min: points both
    sides of a cut must hold (None: n).  Nothing here reads a value back to the host.  -> Fracture:
      rest    the cut's P B compacted pieces sampled by the feeder's FPS from the kernel's start indices (no promise about the
              piece sizes is made to it: without a valid cut a piece may hold the whole cloud)
      src     order[offset of piece p + FPS index]: raw[b, src[b,p,i]] == rest[b,p,i] bit for bit (ok samples)
      pose    se3.exp(twist);  pieces = se3.transform_points(pose, rest)
      top     top[b,a,c] = ops.topk_rows of minus the second output of ops.chamfer(rest[b,a], rest[b,c]): the k rows of piece a
              nearest to piece c (the diagonal: a piece against itself)
      cd      mean + mean of ops.chamfer(rest[b,a][top[b,a,c]], rest[b,c][top[b,c,a]]) - what cut_pairs_double calls cd
      mates   cd <= CD_ACCEPT (the reference's 0.015, dataset.py:1255), False on the diagonal
      ok      the kernel's ok (a valid candidate at every step, every piece within cap) and every piece holds >= n points
    frames [B,P-1,K,3,3] and half_curv [B,P-1,K,2] float64 (draw_fracture_curved_batch), with normals=None: the cuts are curved
    (ops.fracture_curved; the rule: fracture_curved_rule) and a CurvedFracture comes back - the same fields, then anchor, frames,
    half_curv.
    erode [B,P-1,4] float64 = (w_up, w_dn, depth, rho) per step (draw_erosion): material is lost along every cut, in the same one
    launch (ops.fracture_eroded; the rule: fracture_eroded_rule), and the result is the one of its form extended by anchor (where
    it lacks one), erode and lost: an ErodedFracture or ErodedCurvedFracture.  None is the call without erosion.  The lost points
    are in no piece, so no `src` row names one; `cd` and `mates` are taken on the ERODED pieces: a gap g between two boundaries
    adds about 2 g^2 to cd, which is held against the unchanged CD_ACCEPT = 0.015."""
    cap = _feeder_cap("fracture", raw, cap)
    curved = _curved("fracture", normals, frames, half_curv)
    n, k = int(n), int(k)
    n_min = n if n_min is None else int(n_min)
    B, M, P = raw.shape[0], raw.shape[1], u_start.shape[-1]
    if not isinstance(twist, torch.Tensor) or not twist.is_cuda or tuple(twist.shape) != (B, P, 6):
        raise _lib.PznError(f"fracture: twist as [B, P, 6] = [{B}, {P}, 6] on the GPU; got {tuple(twist.shape)}")
    if erode is not None:
        packed, counts, start, label, order, planes, target, cand, anchor, lost, ok = ops.fracture_eroded(
            raw, normals, u_anchor, u_start, erode, n_min, cap, frames=frames, half_curv=half_curv)
    elif curved:
        packed, counts, start, label, order, planes, target, cand, anchor, ok = ops.fracture_curved(raw, frames, half_curv, u_anchor,
                                                                                                     u_start, n_min, cap)
    else:
        packed, counts, start, label, order, planes, target, cand, ok = ops.fracture(raw, normals, u_anchor, u_start, n_min, cap)
    idx = ops.farthest_point_sample(packed, n, start, background=True, counts=counts, max_count=0)      # [P B,n]
    rest = ops.index_points(packed, idx).view(P, B, n, 3).transpose(0, 1).contiguous()               # dataset.py:1147-1163
    cnt = counts.view(P, B)
    at = (cnt.cumsum(0) - cnt).view(P * B, 1) + idx                    # position in the concatenated pieces
    src = torch.gather(order.to(torch.int64).repeat(P, 1), 1, at.clamp_(max=M - 1)).view(P, B, n).transpose(0, 1).contiguous()
    pose = se3.exp(twist.to(torch.float32).contiguous())                                                # [B,P,4,4]
    moved = se3.transform_points(pose.view(B * P, 4, 4), rest.view(B * P, n, 3)).view(B, P, n, 3)
    # boundaries: every ordered pair (a, c) of a sample is one chamfer problem (ops.chamfer splits more than it takes at once)
    A = rest.view(B, P, 1, n, 3).expand(B, P, P, n, 3).reshape(B * P * P, n, 3)
    C = rest.view(B, 1, P, n, 3).expand(B, P, P, n, 3).reshape(B * P * P, n, 3)
    _, d_a = ops.chamfer(A, C)
    top = ops.topk_rows(d_a.neg_(), k)                                                               # [B P P,k]
    bnd = ops.index_points(A, top).view(B, P, P, k, 3)
    cd1, cd2 = ops.chamfer(bnd.reshape(B * P * P, k, 3), bnd.transpose(1, 2).reshape(B * P * P, k, 3))
    cd = (cd1.mean(1) + cd2.mean(1)).view(B, P, P)
    mates = (cd <= CD_ACCEPT) & ~torch.eye(P, dtype=torch.bool, device=raw.device)
    f = Fracture(moved, pose, rest, src, top.view(B, P, P, k), cd, mates, ok & (cnt >= n).all(0), label, planes, target, cand,
                 cnt.t().contiguous())
    if erode is not None:
        return ErodedCurvedFracture(*f, anchor, frames, half_curv, erode, lost) if curved else ErodedFracture(*f, anchor, erode, lost)
    return CurvedFracture(*f, anchor, frames, half_curv) if curved else f


Pile = collections.namedtuple("Pile", "pieces pose rest object_of source mates cd ok")
Pile.__doc__ = """Z piles that hold the pieces of Q objects each, with their answers (datapipe.pile): pieces [Z,K,n,3] the moved pieces
(K = Q P; assembly.match_puzzles takes them), pose [Z,K,4,4], rest [Z,K,n,3], object_of [Z,K] int32 the object 0 .. Q-1 of every
piece, source [Z,K] int32 its slot q P + p before the shuffle, mates [Z,K,K] bool the fracture's inside an object and False across,
cd [Z,K,K] float32 the fracture's inside an object and +inf across, ok [Z] bool (every object of the pile is ok)."""


def pile(frac, objects, perm=None):
    """Regroup a Fracture of any form (curved, eroded) of B = Z Q samples into Z piles of the pieces of Q = `objects` objects each: pile z holds
    the K = Q P pieces of samples z Q .. z Q + Q - 1, piece p of object q in slot q P + p, then shuffled: position k of pile z
    holds slot perm[z,k] (perm [Z,K] int64, every row a permutation of 0 .. K-1, on the fracture's device; None: the identity),
    so the objects are no contiguous blocks.  -> Pile.  assembly.truth_table(pile.pose[z], pile.mates[z], pile.cd[z]) is the table
    a perfect matcher returns for pile z, +inf between the objects.  Indexing only, on the device the fracture lives on; nothing
    waits for it."""
    Q = int(objects)
    B, P = frac.pose.shape[0], frac.pose.shape[1]
    if Q < 1 or B % Q:
        raise _lib.PznError(f"pile: objects = {Q} does not divide the fracture's B = {B} samples")
    Z, K = B // Q, Q * P
    dev = frac.pose.device
    if perm is None:
        perm = torch.arange(K, dtype=torch.int64, device=dev).expand(Z, K)
    if not isinstance(perm, torch.Tensor) or perm.dtype != torch.int64 or tuple(perm.shape) != (Z, K) or perm.device != dev:
        raise _lib.PznError(f"pile: perm as int64 [Z, K] = [{Z}, {K}] on {dev}; got {getattr(perm, 'dtype', type(perm))} "
                            f"{tuple(getattr(perm, 'shape', ()))}")
    z = torch.arange(Z, device=dev)[:, None]
    pieces, pose, rest = (t.reshape(Z, K, *t.shape[2:])[z, perm] for t in (frac.pieces, frac.pose, frac.rest))
    object_of = perm // P
    same = object_of[:, :, None] == object_of[:, None, :]
    # entry (a, c) of a pile is entry (p_a, p_c) of its object's sample where a and c are of one object (masked elsewhere)
    b = z[:, :, None] * Q + object_of[:, :, None]
    pa, pc = (perm % P)[:, :, None], (perm % P)[:, None, :]
    mates = frac.mates[b, pa, pc] & same
    cd = torch.where(same, frac.cd[b, pa, pc], frac.cd.new_full((), float("inf")))
    return Pile(pieces, pose, rest, object_of.to(torch.int32), perm.to(torch.int32), mates, cd, frac.ok.view(Z, Q).all(dim=1))


def _fracture_cols(P, K):       # normals, anchor draws, start fractions, twists
    return _cols(3 * (P - 1) * K, (P - 1) * K, P, 6 * P)


def draw_fracture_batch(rng, gen, B, P, K, mag, out):
    """The host draws of one fracture batch into out [B, width] float64 (columns: _fracture_cols(P, K)): candidate normals
    randn(3) normalised, the anchor and start uniforms from rng, one twist per piece from gen."""
    normals, u_anchor, u_start, tw = _fracture_cols(P, K)
    _draw_fracture_cuts(rng, B, P, K, out, normals, u_anchor)
    out[:, u_start] = rng.rand(B, P)
    twist = np.empty((B * P, 6), dtype=np.float64)
    _draw_twist(gen, mag, twist)
    out[:, tw] = twist.reshape(B, 6 * P)


def _draw_fracture_cuts(rng, B, P, K, out, normals, u_anchor):
    """The cut draws of a fracture (both fracture forms): candidate normals randn(3) normalised, then the anchor uniforms."""
    v = rng.randn(B, (P - 1) * K, 3)
    out[:, normals] = (v / np.linalg.norm(v, axis=2, keepdims=True)).reshape(B, -1)
    out[:, u_anchor] = rng.rand(B, (P - 1) * K)


def _fracture_curved_cols(P, K):        # frames, half curvatures, anchor draws, start fractions, twists
    return _cols(9 * (P - 1) * K, 2 * (P - 1) * K, (P - 1) * K, P, 6 * P)


def _draw_fracture_curved_cuts(rng, B, P, K, curvature, out, frames, half_curv, u_anchor):
    """The cut draws of a curved fracture (both forms): those of _draw_fracture_cuts (normals, anchor uniforms), then per candidate
    a tangent rng.randn(3), made orthogonal to the normal n (Gram-Schmidt) and normalised - the coordinate axis least aligned with
    n in its place where less than 1e-12 of it is left - as e1, e2 = n x e1, and the curvatures rng.rand(2) mapped to
    [-curvature, curvature], stored as halves."""
    R = (P - 1) * K
    cuts = np.empty((B, 4 * R), dtype=np.float64)
    _draw_fracture_cuts(rng, B, P, K, cuts, slice(0, 3 * R), slice(3 * R, 4 * R))
    n = cuts[:, :3 * R].reshape(B, R, 3)
    out[:, u_anchor] = cuts[:, 3 * R:]
    t = rng.randn(B, R, 3)
    e1 = t - (t * n).sum(2, keepdims=True) * n
    short = np.linalg.norm(e1, axis=2) < 1e-12
    if short.any():
        axis = np.eye(3)[np.argmin(np.abs(n[short]), axis=1)]
        e1[short] = axis - (axis * n[short]).sum(1, keepdims=True) * n[short]
    e1 /= np.linalg.norm(e1, axis=2, keepdims=True)
    out[:, frames] = np.stack([e1, np.cross(n, e1), n], axis=2).reshape(B, 9 * R)
    out[:, half_curv] = ((2.0 * rng.rand(B, R, 2) - 1.0) * curvature / 2.0).reshape(B, 2 * R)


def draw_fracture_curved_batch(rng, gen, B, P, K, mag, curvature, out):
    """draw_fracture_batch for curved cuts into out [B, width] float64 (columns: _fracture_curved_cols(P, K)): the cut draws of
    _draw_fracture_curved_cuts with curvatures up to `curvature`, then the start uniforms and the twists as the plane form draws
    them."""
    frames, half_curv, u_anchor, u_start, tw = _fracture_curved_cols(P, K)
    _draw_fracture_curved_cuts(rng, B, P, K, curvature, out, frames, half_curv, u_anchor)
    out[:, u_start] = rng.rand(B, P)
    twist = np.empty((B * P, 6), dtype=np.float64)
    _draw_twist(gen, mag, twist)
    out[:, tw] = twist.reshape(B, 6 * P)


def fracture_curved_draws(rng, gen, B, P, K, mag, curvature):
    """draw_fracture_curved_batch into a fresh row, split: -> (frames [B,P-1,K,3,3], half_curv [B,P-1,K,2], u_anchor [B,P-1,K],
    u_start [B,P], twist [B,P,6]), float64 numpy arrays."""
    cols = _fracture_curved_cols(P, K)
    out = np.empty((B, cols[-1].stop), dtype=np.float64)
    draw_fracture_curved_batch(rng, gen, B, P, K, mag, curvature, out)
    frames, half_curv, u_anchor, u_start, tw = cols
    return (out[:, frames].reshape(B, P - 1, K, 3, 3), out[:, half_curv].reshape(B, P - 1, K, 2),
            out[:, u_anchor].reshape(B, P - 1, K), out[:, u_start].copy(), out[:, tw].reshape(B, P, 6))


def fracture_arguments(rng, gen, B, P, K, mag, curvature, erosion=0.0, chip=(0.0, 0.0)):
    """The host draws of a fracture batch as the keyword arguments of datapipe.fracture that follow `raw` (float64 numpy arrays):
    fracture_draws' for curvature 0 (planes), fracture_curved_draws' with normals=None above it.  What the tools' --curvature
    does.  With an erosion or a chip = (depth, radius) above 0 (the tools' --erosion and --chip), `erode` as well: draw_erosion's,
    drawn from rng after the other draws, which stay what they are without it."""
    if not 0.0 <= curvature < np.inf:
        raise _lib.PznError(f"fracture_arguments: curvature={curvature!r} (the largest principal curvature, finite and >= 0)")
    erosion, chip, eroded = _erosion_args("fracture_arguments", erosion, chip)
    if curvature == 0:
        args = dict(zip(("normals", "u_anchor", "u_start", "twist"), fracture_draws(rng, gen, B, P, K, mag)))
    else:
        names = ("frames", "half_curv", "u_anchor", "u_start", "twist")
        args = dict(zip(names, fracture_curved_draws(rng, gen, B, P, K, mag, curvature)), normals=None)
    if eroded:
        args["erode"] = draw_erosion(rng, B, P, erosion, chip)
    return args


def _fracture_pair_curved_cols(P, K):   # frames, half curvatures, anchor draws, the number of pieces, uniforms, twist
    return _cols(9 * (P - 1) * K, 2 * (P - 1) * K, (P - 1) * K, 1, ops.FRACTURE_PAIR_UNIFORMS, 6)


def draw_fracture_pair_curved_batch(rng, gen, B, lo, hi, K, mag, curvature, out):
    """draw_fracture_pair_batch for curved cuts into out [B, width] float64 (columns: _fracture_pair_curved_cols(hi, K)): the cut
    draws of _draw_fracture_curved_cuts for P = hi, then the number of pieces, the seven uniforms and the twist as the plane form
    draws them."""
    frames, half_curv, u_anchor, pc, u, tw = _fracture_pair_curved_cols(hi, K)
    _draw_fracture_curved_cuts(rng, B, hi, K, curvature, out, frames, half_curv, u_anchor)
    out[:, pc] = np.minimum(hi, lo + np.floor(rng.rand(B, 1) * (hi - lo + 1)))
    out[:, u] = rng.rand(B, ops.FRACTURE_PAIR_UNIFORMS)                         # u_kind, u_a, u_c, u_sU, u_sD, u_sFU, u_sFD
    _draw_twist(gen, mag, out[:, tw])


def _build_fracture_pair_curved(f, d, erode=None):
    B, K, P = d.shape[0], f.K, f.pieces[1]
    frames, half_curv, u_anchor, pc, u, tw = _fracture_pair_curved_cols(P, K)
    tensors, ok, record = cut_pairs_fracture(f.raw, None, d[:, u_anchor].reshape(B, P - 1, K), d[:, pc].reshape(B).to(torch.int32),
                                             d[:, u], d[:, tw], n=f.n, k=f.k, neighbours=f.neighbours,
                                             frames=d[:, frames].reshape(B, P - 1, K, 3, 3),
                                             half_curv=d[:, half_curv].reshape(B, P - 1, K, 2), erode=erode)
    return tensors, ok, dict(fracture=record)


def _fracture_pair_curved_mode(lo, hi, curvature):
    """The feeder mode of PairFeeder(pieces=(lo, hi), curvature=c) with c > 0, as _fracture_pair_mode binds the range."""
    return _FeederMode(lambda K: _fracture_pair_curved_cols(hi, K),
                       lambda rng, gen, B, K, mag, out: draw_fracture_pair_curved_batch(rng, gen, B, lo, hi, K, mag, curvature, out),
                       _build_fracture_pair_curved)


def _fracture_pair_cols(P, K):  # normals, anchor draws, the number of pieces, uniforms, twist
    return _cols(3 * (P - 1) * K, (P - 1) * K, 1, ops.FRACTURE_PAIR_UNIFORMS, 6)


def draw_fracture_pair_batch(rng, gen, B, lo, hi, K, mag, out):
    """The host draws of one PairFeeder(pieces=(lo, hi)) batch into out [B, width] float64 (columns: _fracture_pair_cols(hi, K)):
    the cut draws of draw_fracture_batch for P = hi (a sample with fewer pieces leaves the later rows unread), the number of
    pieces lo + floor(u (hi - lo + 1)) from one rng.rand(B), the seven uniforms of fracture_pair_rule, one twist per sample."""
    normals, u_anchor, pc, u, tw = _fracture_pair_cols(hi, K)
    _draw_fracture_cuts(rng, B, hi, K, out, normals, u_anchor)
    out[:, pc] = np.minimum(hi, lo + np.floor(rng.rand(B, 1) * (hi - lo + 1)))
    out[:, u] = rng.rand(B, ops.FRACTURE_PAIR_UNIFORMS)                         # u_kind, u_a, u_c, u_sU, u_sD, u_sFU, u_sFD
    _draw_twist(gen, mag, out[:, tw])


def _build_fracture_pair(f, d, erode=None):
    B, K, P = d.shape[0], f.K, f.pieces[1]
    normals, u_anchor, pc, u, tw = _fracture_pair_cols(P, K)
    tensors, ok, record = cut_pairs_fracture(f.raw, d[:, normals].reshape(B, P - 1, K, 3), d[:, u_anchor].reshape(B, P - 1, K),
                                             d[:, pc].reshape(B).to(torch.int32), d[:, u], d[:, tw], n=f.n, k=f.k,
                                             neighbours=f.neighbours, erode=erode)
    return tensors, ok, dict(fracture=record)


def _fracture_pair_mode(lo, hi):
    """The feeder mode of PairFeeder(pieces=(lo, hi)): the protocol's cols(K) and draw(rng, gen, B, K, mag, out) with the range
    bound."""
    return _FeederMode(lambda K: _fracture_pair_cols(hi, K),
                       lambda rng, gen, B, K, mag, out: draw_fracture_pair_batch(rng, gen, B, lo, hi, K, mag, out),
                       _build_fracture_pair)


def _eroded_mode(mode, P, erosion, chip):
    """The feeder mode of PairFeeder(pieces=(lo, P), erosion=, chip=): the fracture-pair mode `mode` (planes or surfaces) with
    4 (P - 1) more staging columns behind its own, the erosion of every step, drawn by draw_erosion from rng after the mode's own
    draws; its builder passes them on as `erode`."""
    def cols(K):
        own = mode.cols(K)
        return own + [slice(own[-1].stop, own[-1].stop + 4 * (P - 1))]

    def draw(rng, gen, B, K, mag, out):
        mode.draw(rng, gen, B, K, mag, out)
        out[:, cols(K)[-1]] = draw_erosion(rng, B, P, erosion, chip).reshape(B, 4 * (P - 1))

    def build(f, d):
        return mode.build(f, d, erode=d[:, cols(f.K)[-1]].reshape(d.shape[0], P - 1, 4))

    return _FeederMode(cols, draw, build)


def fracture_draws(rng, gen, B, P, K, mag):
    """draw_fracture_batch into a fresh row, split: -> (normals [B,P-1,K,3], u_anchor [B,P-1,K], u_start [B,P], twist [B,P,6]),
    float64 numpy arrays."""
    cols = _fracture_cols(P, K)
    out = np.empty((B, cols[-1].stop), dtype=np.float64)
    draw_fracture_batch(rng, gen, B, P, K, mag, out)
    normals, u_anchor, u_start, tw = cols
    return (out[:, normals].reshape(B, P - 1, K, 3), out[:, u_anchor].reshape(B, P - 1, K), out[:, u_start].copy(),
            out[:, tw].reshape(B, P, 6))


def _plane_draw():
    return np.random.rand(3, 1), np.random.rand(1) / 3          # dataset.py:767-769 (z=None)


def _side(pts, normal, z):
    return (np.dot(pts, normal) + z >= 0).reshape(-1)            # :770-771


def plan_double_cut_like_reference(raw, accept, n=1024, mag=0.8):
    """The branch decisions and random draws of ONE `CADDataset.__getitem__` call with split_twice=True
    (dataset.py:1203-1355) followed by MovedCADDataset2 (:98-105), made from numpy's and torch's GLOBAL generators in the
    reference's order (seed them as the reference run would), as a recipe for make_pairs_regions.
      raw     [M,3] float32 numpy array (host side: piece sizes steer the branches and the start-index ranges)
      accept  callable(recipe without motion) -> float: the chamfer distance of the two boundaries of the candidate pair —
              the one decision of the reference that needs the pieces themselves (:1250-1253, :1322-1325: the pair is
              kept when it is <= 0.015).  Called at most once.
    -> dict(kind, normal1, z1, normal2, z2, u_tab, d_tab, s_u, s_d, twist)"""
    raw = np.asarray(raw, dtype=np.float32)
    none = (np.zeros((3, 1)), np.zeros(1))

    def recipe(kind, planes, u_tab, d_tab, s_u, s_d):
        (n1, z1), (n2, z2) = planes
        return dict(kind=kind, normal1=n1.reshape(3), z1=z1.reshape(1), normal2=n2.reshape(3), z2=z2.reshape(1),
                    u_tab=np.array(u_tab, np.int64), d_tab=np.array(d_tab, np.int64), s_u=int(s_u), s_d=int(s_d))

    def single(p1, s1):                                          # self.slice(pc, None, up, down), :1192-1201
        while int(s1.sum()) < n or int((~s1).sum()) < n:
            p1 = _plane_draw()
            s1 = _side(raw, *p1)
        s_u = np.random.randint(0, int(s1.sum()))
        s_d = np.random.randint(0, int((~s1).sum()))
        return recipe("single", (p1, none), (UP, 0), (DOWN, 0), s_u, s_d)

    def item():
        slice_seed = int(torch.randint(0, 3, (1,)))              # :1206-1207
        p1 = _plane_draw()                                       # :1208
        s1 = _side(raw, *p1)
        n_up, n_down = int(s1.sum()), int((~s1).sum())
        if slice_seed == 1 and n_up < 3000:                      # :1211-1214
            slice_seed = 2
        if slice_seed == 2 and n_down < 3000:
            slice_seed = 1
        if slice_seed == 0:
            return single(p1, s1)
        inner = s1 if slice_seed == 1 else ~s1                   # the piece that is cut again
        n_other = n_down if slice_seed == 1 else n_up            # the piece that is not
        sub = raw[inner]
        p2 = _plane_draw()                                       # :1222 / :1296
        s2 = _side(sub, *p2)
        tries = 0
        while tries <= 5 and (int(s2.sum()) < n or int((~s2).sum()) < n):
            p2 = _plane_draw()
            s2 = _side(sub, *p2)
            tries += 1
        n_a, n_b = int(s2.sum()), int((~s2).sum())               # uppc, downpc
        if n_a < n or n_b < n:                                   # :1226-1227
            return single(p1, s1)
        A, Bt = (UP_UPPC, UP_DOWNPC) if slice_seed == 1 else (DOWN_UPPC, DOWN_DOWNPC)
        OTHER = DOWN if slice_seed == 1 else UP
        se = int(torch.randint(0, 3, (1,)))                      # :1229 / :1302
        if se == 0 or n_other < n:                               # U = one half, D = the other half + the other piece
            choice = int(torch.randint(0, 2, (1,)))
            first, second = (A, Bt) if choice == 0 else (Bt, A)
            n_first, n_second = (n_a, n_b) if choice == 0 else (n_b, n_a)
            s_u = np.random.randint(0, n_first)
            s_d = np.random.randint(0, n_second + n_other)
            return recipe("half_vs_rest", (p1, p2), (first, 0), (second, OTHER), s_u, s_d)
        if se == 1:                                              # U = one half, D = the other PIECE, kept if they touch
            choice = int(torch.randint(0, 2, (1,)))
            first = A if choice == 0 else Bt
            s_u = np.random.randint(0, n_a if choice == 0 else n_b)
            s_d = np.random.randint(0, n_other)
            cand = recipe("half_vs_other", (p1, p2), (first, 0), (OTHER, 0), s_u, s_d)
            if float(accept(cand)) > 0.015:                      # :1250-1253 / :1322-1325
                return single(p1, s1)
            return cand
        s_u = np.random.randint(0, n_a)                          # se == 2: the two halves, :1255-1256 / :1326-1327
        s_d = np.random.randint(0, n_b)
        re_now = np.random.rand(1)                               # :1260 / :1330
        if not (re_now > (0.7 if slice_seed == 1 else 0.6)) and n_other >= 1200:
            np.random.randint(0, n_other + n)                    # :1281 / :1350: two more FPS runs whose results the
            np.random.randint(0, n)                              # reference overwrites (:1282-1283, :1351-1352)
        return recipe("halves", (p1, p2), (A, 0), (Bt, 0), s_u, s_d)

    rec = item()
    x = torch.randn(1, 6)                                        # MovedCADDataset2: rigid_transform(up), transforms.py:163-168
    x = x / x.norm(p=2, dim=1, keepdim=True) * mag
    torch.randn(1, 6)                                            # rigid_transform(upb), dataset.py:101: drawn, result unused
    rec["twist"] = x.reshape(6).numpy()
    return rec
