"""Float64 truth of the pooled level's backward (include/pzn.h: pzn_pool_wgrad_f32, pzn_sa_level_bwd_pt_f32), the inputs its
tests share, the condition under which fp32 must reproduce the truth bit for bit, and a restatement of the launch rules that
decide which kernel paths a shape reaches.  Shared by tests/test_pool_bwd_ref_cpu.py (the truth against autograd, the
condition, the paths, the sharpness of the probes) and tests/test_gpu_pool_bwd_exact.py (the kernels against the truth).

The contract, for dout, out [G, C2], argmax [G, C2] in 0..31, W2 [C2, C1], Pp [B*N, C1], Q [G, C1], idx [B, S, 32] in 0..N-1,
xyz [B, N, 3], new_xyz [B, S, 3], G = B*S, group g = b*S + s, its k-th neighbour the point j = b*N + idx[b, s, k]:
    gv[g, c]      = dout[g, c] if out[g, c] > 0 else 0
    h[(g,k), :]   = relu(Pp[j] + Q[g])
    dW2[c, :]     = sum_g gv[g, c] h[(g, argmax[g, c]), :]            db2[c] = sum_g gv[g, c]
    dh[(g,k), :]  = [Pp[j] + Q[g] > 0] * sum over {c: argmax[g, c] == k} of gv[g, c] W2[c, :]
    dP[j, :]      = sum of dh over the rows (g, k) that gathered j
    dW1[:, 0:3]   = sum over rows of dh[(g,k), :]^T (xyz[j] - new_xyz[g])        db1 = column sums of dh
argmax and out are INPUTS of the backward: the tests choose them freely, no forward pass is involved.  Nothing below is taken
from the kernels: the truth is the dense statement (the gradient scattered to [G*32, C2], plain matrix products, one
index_add), so it shares neither the hit lists nor the walks with what it judges.

Exact probes.  Inputs on dyadic grids (exact_inputs): dout in {+-1, +-2}, W2 integers in [-2, 2], Pp and Q multiples of 1/4 in
[-4, 4], xyz and new_xyz multiples of 1/4 in [0, 1], out in {0, 1} with ~45 % zeros.  Then every term of every output is a
multiple of that output's grid unit (UNITS), and so is every partial sum in any order; while the sum of |term| of an element,
in grid units, stays below 2^24 (exact_margin, from the truth alone) every such partial sum is an fp32 value: the kernel must
equal the truth bit for bit whatever its summation order, atomics included.  Pp + Q == 0 happens on its own (~3 % of the
gates) and must gate off.

Float case.  For random fp32 inputs the truth also returns, per element, the sum of |term| and the number of terms n; the
kernel's value is held to gamma_(n+3) * sum|term| (float_bound): a term passes through at most n roundings on any summation
tree of fused multiply-adds, plus the row add h = fl(Pp + Q), the final add into the output, and one spare.  The gate has the
same sign in fp32 and float64 (rounding keeps the sign of a non-zero sum)."""
import collections
import zlib

import numpy as np
import torch

SEED = 2203
LIMIT = float(1 << 24)
U32 = 2.0 ** -24
OUTPUTS = ("dW2", "db2", "dP", "dW1", "db1")
UNITS = {"dW2": 0.25, "db2": 1.0, "dP": 1.0, "dW1": 0.25, "db1": 1.0}      # the grid every term of the output lies on
MUTATIONS = ("drop_hit", "gate_at_zero", "double_row")

Truth = collections.namedtuple("Truth", "value abs count")      # per output: float64 value, sum of |term|, number of terms


def _f64(a):
    return (a.detach().cpu() if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))).double()


def _i64(a):
    return (a.detach().cpu() if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))).long()


def _backward(dout, argmax, out, W2, Pp, Q, idx, xyz, new_xyz, mutate=None):
    dout, out, W2, Pp, Q, xyz, new_xyz = map(_f64, (dout, out, W2, Pp, Q, xyz, new_xyz))
    argmax, idx = _i64(argmax), _i64(idx)
    B, S, K = idx.shape
    assert K == 32
    G, BN = B * S, Pp.shape[0]
    N, C1, C2 = BN // B, Pp.shape[1], W2.shape[0]
    R = G * 32
    assert BN == B * N and dout.shape == (G, C2) and W2.shape == (C2, C1) and Q.shape == (G, C1)
    assert 0 <= int(idx.min()) and int(idx.max()) < N and 0 <= int(argmax.min()) and int(argmax.max()) < 32

    gv = torch.where(out.reshape(G, C2) > 0, dout, torch.zeros_like(dout))
    if mutate == "drop_hit":            # one live (group, channel) pair forgotten
        g, c = (int(v) for v in torch.nonzero(gv)[0])
        gv[g, c] = 0.0
    point = (torch.arange(B)[:, None, None] * N + idx).reshape(G, 32)           # the point each row gathered
    pre = Pp[point] + Q[:, None, :]                                             # [G, 32, C1]
    gate = ((pre >= 0) if mutate == "gate_at_zero" else (pre > 0)).reshape(R, C1).double()
    h = pre.clamp_min(0.0).reshape(R, C1)
    del pre
    dy = torch.zeros(G, 32, C2, dtype=torch.float64)                            # one non-zero per live (g, c)
    dy.scatter_(1, argmax.reshape(G, 1, C2), gv.reshape(G, 1, C2))
    dy = dy.reshape(R, C2)
    live = (gv != 0).double()

    res = {}
    res["dW2"] = Truth(dy.T @ h, dy.abs().T @ h, live.sum(0)[:, None].expand(C2, C1).clone())
    res["db2"] = Truth(gv.sum(0), gv.abs().sum(0), live.sum(0))
    del h
    dh = gate * (dy @ W2)                                                       # [R, C1]
    dh_abs = gate * (dy.abs() @ W2.abs())
    dh_cnt = gate * (dy != 0).double().sum(1, keepdim=True)                     # the hits of the row, where its gate is on
    del dy, gate
    weight = torch.ones(R, 1, dtype=torch.float64)
    if mutate == "double_row":          # one row that carries a gradient added twice to its point
        weight[int(torch.nonzero(dh.abs().sum(1))[0])] = 2.0
    flat = point.reshape(R)
    res["dP"] = Truth(*(torch.zeros(BN, C1, dtype=torch.float64).index_add_(0, flat, t) for t in (dh * weight, dh_abs, dh_cnt)))
    rel = xyz.reshape(BN, 3)[flat] - new_xyz.reshape(G, 3).repeat_interleave(32, dim=0)
    res["dW1"] = Truth(dh.T @ rel, dh_abs.T @ rel.abs(), dh_cnt.sum(0)[:, None].expand(C1, 3).clone())
    res["db1"] = Truth(dh.sum(0), dh_abs.sum(0), dh_cnt.sum(0))
    return res


def reference(dout, argmax, out, W2, Pp, Q, idx, xyz, new_xyz):
    """{output name: Truth(value, sum of |term|, number of terms)} in float64; dW1 is its three coordinate columns [C1, 3]."""
    return _backward(dout, argmax, out, W2, Pp, Q, idx, xyz, new_xyz)


def mutated(kind, *inputs):
    """The truth with one deliberate mistake (MUTATIONS): what the exact probes must be able to tell from the right answer."""
    assert kind in MUTATIONS
    return _backward(*inputs, mutate=kind)


def gamma(k):
    k = torch.as_tensor(k, dtype=torch.float64)
    return k * U32 / (1.0 - k * U32)


def float_bound(truth):
    """gamma_(n+3) * sum|term| per element."""
    return gamma(truth.count + 3.0) * truth.abs


# --------------------------------------------------------------------------- the exactness condition

def on_grids(t):
    """The inputs lie on the grids the condition is stated for."""
    def mult(x, unit, lo, hi):
        x = np.asarray(x, dtype=np.float64)
        return bool(np.array_equal(np.round(x / unit) * unit, x) and x.min() >= lo and x.max() <= hi)
    return (mult(t["dout"], 1.0, -2, 2) and mult(t["W2"], 1.0, -2, 2) and mult(t["Pp"], 0.25, -4, 4) and mult(t["Q"], 0.25, -4, 4)
            and mult(t["xyz"], 0.25, 0, 1) and mult(t["new_xyz"], 0.25, 0, 1) and mult(t["out"], 1.0, 0, 1))


def exact_margin(truth, prefill=None):
    """{output: the largest sum of |term| (plus |prefill|) of an element, in grid units}: each must stay below LIMIT = 2^24."""
    m = {}
    for name in OUTPUTS:
        a = truth[name].abs
        if prefill is not None and name in prefill:
            p = _f64(prefill[name]).abs()
            a = a + (p[:, 0:3] if name == "dW1" else p)
        m[name] = float(a.max()) / UNITS[name]
    return m


def prefill(shape, D):
    """Integers in [-8, 8] for the outputs that are added to; dW1 is the whole [C1, 3 + D] weight gradient, whose columns 3..
    must come back as they went in."""
    B, N, S, C1, C2 = shape
    rng = np.random.default_rng([SEED, 77, *shape])
    draw = lambda *s: rng.integers(-8, 9, size=s).astype(np.float64)
    return {"dW2": draw(C2, C1), "db2": draw(C2), "dW1": draw(C1, 3 + D), "db1": draw(C1)}


# --------------------------------------------------------------------------- the launch rules, restated
# A RESTATEMENT of launch code, to be updated together with it: wgrad_grid_x, the XCD split and the walk of
# pool_wgrad_kernel / pool_wgrad_regen_kernel (csrc/poolbwd.hip), `pc` and the chunks of pool_point_kernel (csrc/sapool.hip).
# The tests use it only to assert that the case table still reaches the paths it was chosen for.

PB_COLS = 128       # hidden columns per workgroup
PR_NB = 4           # groups per batch of the regenerated-row ring (two batches)


def wgrad_walk(G, C1):
    """The weight-gradient pass: ny column slices, gx workgroups per slice; with gx % 8 == 0 XCD x takes the contiguous
    eighth [x gx8, (x+1) gx8) of the groups and its gx / 8 workgroups stride through it, else workgroup x takes x, x + gx, ...
    -> dict(ny, gx, xcd, stride, groups=[groups of every workgroup, in walk order])."""
    ny = C1 // PB_COLS
    gx = min(G, 256 // ny)
    xcd = gx % 8 == 0
    walks = []
    for x in range(gx):
        first, stride, end = x, gx, G
        if xcd:
            gx8 = (G + 7) >> 3
            first, stride, end = (x & 7) * gx8 + (x >> 3), gx >> 3, min(((x & 7) + 1) * gx8, G)
        walks.append(list(range(first, end, stride)))
    assert sorted(g for w in walks for g in w) == list(range(G))        # every group once
    return dict(ny=ny, gx=gx, xcd=xcd, stride=stride, groups=walks)


def point_chunk(N, S):
    """pool_point_kernel's points per chunk: ~64 list entries, clamped to 1 .. 32."""
    return max(1, min(32, (64 * N) // (S * 32)))


def paths(case, t):
    """What the case reaches, from its shape and its planted inputs -> a dict of plain figures."""
    B, N, S, C1, C2 = case.shape
    G = B * S
    w = wgrad_walk(G, C1)
    n = [len(v) for v in w["groups"]]
    live = (np.asarray(t["out"]) > 0) & (np.asarray(t["dout"]) != 0)
    hits = np.zeros((G, 32), dtype=np.int64)
    np.add.at(hits, (np.repeat(np.arange(G), C2), np.asarray(t["argmax"]).reshape(-1)), live.reshape(-1).astype(np.int64))
    idx = np.asarray(t["idx"])
    lists = np.stack([np.bincount(idx[b].reshape(-1), minlength=N) for b in range(B)])          # [B, N] entries per point
    pc = point_chunk(N, S)
    pad = (-N) % pc
    chunks = np.pad(lists, ((0, 0), (0, pad))).reshape(B, -1, pc).sum(-1)
    srt = np.sort(idx, axis=-1)
    pre = np.asarray(t["Pp"]).reshape(B, N, C1)[np.arange(B)[:, None, None], idx] + np.asarray(t["Q"]).reshape(B, S, 1, C1)
    return dict(
        xcd=w["xcd"], gx=w["gx"], ny=w["ny"], min_groups=min(n), max_groups=max(n), batches=-(-max(n) // PR_NB),
        ragged=any(v % PR_NB for v in n if v > PR_NB), empty_workgroups=sum(v == 0 for v in n),
        uneven=len(set(n)) > 1, cloud_steps=w["stride"] / S, cpw=C2 // 16, pc=pc,
        pc_unclamped=(64 * N) / (S * 32), empty_chunks=int((chunks == 0).sum()), chunks=int(chunks.size),
        max_row_hits=int(hits.max()), dead_groups=int((hits.sum(1) == 0).sum()), max_list=int(lists.max()),
        unused_points=int((lists == 0).sum()), first_last_unused=bool((lists[:, 0] == 0).all() and (lists[:, -1] == 0).all()),
        one_point_groups=int((srt[..., 0] == srt[..., -1]).sum()), duplicates=int((srt[..., 1:] == srt[..., :-1]).sum()),
        zero_gates=int((pre == 0).sum()), zero_dout_live=int(((np.asarray(t["out"]) > 0) & (np.asarray(t["dout"]) == 0)).sum()))


def inverse_lists(idx, N):
    """pzn_knn_inverse_lists by NumPy's stable sort: off [B, N+1], rows [B, S*32] (ascending within a point), pts [B, S*32]."""
    idx = np.asarray(idx)
    B = idx.shape[0]
    flat = idx.reshape(B, -1)
    rows = np.argsort(flat, axis=1, kind="stable")
    pts = np.take_along_axis(flat, rows, axis=1)
    off = np.zeros((B, N + 1), dtype=np.int64)
    for b in range(B):
        off[b, 1:] = np.cumsum(np.bincount(flat[b], minlength=N))
    return off.astype(np.int32), rows.astype(np.int32), pts.astype(np.int32)


# --------------------------------------------------------------------------- the case table

Case = collections.namedtuple("Case", "name shape plant why")
CASES = collections.OrderedDict()
PLANT_A = (3, 80, 70, 128, 128)       # planted structure runs on two small shapes, C2 = 128 and C2 = 256: a plain walk of
PLANT_B = (2, 64, 150, 256, 256)      # one group per workgroup, and an XCD walk of two column slices with 2 or 3 groups


def _case(*shapes):
    def register(fn):
        for shape in shapes:
            name = fn.__name__ + "-" + "x".join(map(str, shape))
            CASES[name] = Case(name, tuple(shape), fn, " ".join(fn.__doc__.split()))
        return fn
    return register


@_case((5, 96, 500, 128, 128))
def xcd_three_batches(rng, t, shape):
    """G = 2500 at C1 = 128: 256 workgroups, the XCD walk over eighths of 313 groups (the last one 309), 9 or 10 groups per
    workgroup: three batches of the ring (dma_small(b + 2), the reuse of batch b - 1's tiles), a ragged last batch of 1 or 2
    groups, workgroup ranges of unequal length.  S = 500 is no multiple of the walk's stride of 32: clouds change mid-walk."""


@_case((5, 64, 288, 256, 256))
def two_slices_cpw16(rng, t, shape):
    """C1 = C2 = 256: two column slices of 128 workgroups, XCD eighths of 180 groups, 11 or 12 groups per workgroup; 16 channels
    per wavefront, so a batch's 4 groups x 16 channels fill all 64 lanes of the (arg-max, out, dout) loads."""


@_case((2, 64, 384, 384, 128))
def plain_walk_c1_384(rng, t, shape):
    """C1 = 384 != C2 = 128: three column slices of 85 workgroups, not a multiple of 8, so the plain strided walk with 9 or 10
    groups per workgroup - the only way to more than one group per workgroup off the XCD walk."""


@_case((40, 64, 8, 128, 64))
def small_clouds_c2_64(rng, t, shape):
    """G = 320 with S = 8 below the XCD walk's stride of 32: a step of the walk crosses four clouds, the running cloud remainder
    of the row DMA takes several steps per group.  C2 = 64: pool_hits_kernel<1>, pool_wgrad_regen_kernel<4>, and the dynamic
    LDS of pool_point_kernel is exactly the 32 KB its final reduction reuses."""


@_case((1, 64, 260, 128, 64))
def empty_workgroups(rng, t, shape):
    """G = 260 over 256 workgroups: the last XCD's range holds 29 groups for 32 workgroups, three workgroups walk nothing and
    must still write their (zero) partial tile and bias sums."""


@_case((1, 64, 5, 128, 256), (1, 64, 8, 256, 64))
def few_groups(rng, t, shape):
    """G = 5 (plain walk, 5 workgroups) and G = 8 (XCD walk of one workgroup per XCD, two slices): the fixed-order reduction
    sums fewer partials than it has wavefronts."""


@_case((3, 1024, 8, 128, 128))
def sparse_chunks(rng, t, shape):
    """N >= 16 S: pc clamps to 32; the neighbours come from three of every cloud's 32 chunks, so most chunks hold no entry and
    write nothing but zeros."""
    B, N, S, _, _ = shape
    pool = np.concatenate([np.arange(c * 32, c * 32 + 32) for c in (0, 13, 31)])
    t["idx"] = pool[rng.integers(0, pool.size, size=(B, S, 32))]


@_case((2, 40, 90, 128, 128))
def one_point_chunks(rng, t, shape):
    """S * 32 >= 64 N: pc clamps to 1, every point a chunk of ~72 entries, i.e. two trips of 64."""


@_case(PLANT_A, PLANT_B)
def rows_of_many_hits(rng, t, shape):
    """argmax[g, :] constant for every fifth group: all the group's live channels hit one row, more than 64 (the h0 loop and
    the refill of hslot); the first of them has every channel live, C2 = 128 or 256 hits: whole trips of 64 and nothing left."""
    G = t["argmax"].shape[0]
    for g in range(0, G, 5):
        t["argmax"][g, :] = (7 * g + 3) % 32
    t["out"][0, :] = 1.0


@_case(PLANT_A, PLANT_B)
def dead_groups(rng, t, shape):
    """out <= 0 on every channel of the first group, the last one, and six consecutive ones (a whole batch of the ring): no row
    offset moves, no hit is written, the weight pass adds zeros."""
    G = t["out"].shape[0]
    for g in [0, G - 1] + list(range(9, 15)):
        t["out"][g, :] = 0.0


@_case(PLANT_A, PLANT_B)
def zero_dout(rng, t, shape):
    """dout == 0 on a third of the channels, live ones included, and on every channel of two groups whose out is > 0
    everywhere: a live channel with a zero gradient is no hit."""
    t["dout"][rng.random(t["dout"].shape) < 1 / 3] = 0.0
    for g in (2, 11):
        t["dout"][g, :] = 0.0
        t["out"][g, :] = 1.0


@_case(PLANT_A, PLANT_B)
def hub_point(rng, t, shape):
    """idx[:, :, 0] is one point of the cloud for every group: its inverse list has at least S = 70 or 150 rows, two or three
    64-entry trips with the running sum carried across them."""
    N = shape[1]
    t["idx"][:, :, 0] = N // 3


@_case(PLANT_A, PLANT_B)
def duplicate_neighbours(rng, t, shape):
    """Every sixth group gathers ONE point 32 times, every sixth (offset 3) holds 16 pairs of duplicates: a point's list has
    several rows of the same group, each with its own hits."""
    idx = t["idx"].reshape(-1, 32)
    idx[0::6, :] = idx[0::6, :1]
    idx[3::6, 1::2] = idx[3::6, 0::2]


@_case(PLANT_A, PLANT_B)
def ungathered_points(rng, t, shape):
    """Nobody gathers the first and the last point of a cloud, nor points 4 pc .. 7 pc - 1 (three whole chunks): their dP rows
    are the zeros written at a chunk's start, end, and for chunks without any entry."""
    B, N, S, _, _ = shape
    pc = point_chunk(N, S)
    banned = {0, N - 1} | set(range(4 * pc, 7 * pc))
    allowed = np.array([j for j in range(N) if j not in banned])
    t["idx"] = allowed[rng.integers(0, allowed.size, size=(B, S, 32))]


def exact_inputs(case):
    """The case's dyadic inputs as float64 / int64 NumPy arrays (module docstring), its planted structure applied."""
    B, N, S, C1, C2 = case.shape
    G = B * S
    rng = np.random.default_rng([SEED, zlib.crc32(case.name.encode())])
    t = dict(
        dout=rng.choice(np.array([-2.0, -1.0, 1.0, 2.0]), size=(G, C2)),
        out=(rng.random((G, C2)) >= 0.45).astype(np.float64),
        argmax=rng.integers(0, 32, size=(G, C2)),
        idx=rng.integers(0, N, size=(B, S, 32)),
        W2=rng.integers(-2, 3, size=(C2, C1)).astype(np.float64),
        Pp=rng.integers(-16, 17, size=(B * N, C1)) / 4.0,
        Q=rng.integers(-16, 17, size=(G, C1)) / 4.0,
        xyz=rng.integers(0, 5, size=(B, N, 3)) / 4.0,
        new_xyz=rng.integers(0, 5, size=(B, S, 3)) / 4.0)
    case.plant(rng, t, case.shape)
    return t


FLOAT_SHAPES = [(5, 96, 500, 128, 128), (5, 64, 288, 256, 256)]


def float_inputs(shape):
    """Random fp32 inputs (as float32 NumPy arrays) with ~45 % of the channels dead."""
    B, N, S, C1, C2 = shape
    G = B * S
    rng = np.random.default_rng([SEED, 99, *shape])
    f = lambda x: x.astype(np.float32)
    return dict(
        dout=f(rng.standard_normal((G, C2))), out=f(rng.standard_normal((G, C2)) + 0.12),
        argmax=rng.integers(0, 32, size=(G, C2)), idx=rng.integers(0, N, size=(B, S, 32)),
        W2=f(rng.standard_normal((C2, C1)) / np.sqrt(C1)), Pp=f(rng.standard_normal((B * N, C1))),
        Q=f(0.5 * rng.standard_normal((G, C1))), xyz=f(rng.random((B, N, 3))), new_xyz=f(rng.random((B, S, 3))))


ARGS = ("dout", "argmax", "out", "W2", "Pp", "Q", "idx", "xyz", "new_xyz")


def truth_of(t):
    return reference(*(t[k] for k in ARGS))
