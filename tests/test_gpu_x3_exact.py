"""Exact integer probes of the six bf16x3 products, kernel by kernel (csrc/pzn_x3.h; tests/_x3_probe.py builds the operands
and proves them exact, tests/test_x3_probe_cpu.py shows on the CPU that a lost product or plane changes the integers).

Every comparison is `==` on fp32 bits against an int64 reference: operands are integers for which each kept plane
product and every partial sum is an fp32 value, so any summation order - split-K atomics included - gives the same
bits.  Each case runs the three operand classes (3,1), (1,3), (2,2) over a probe set of at most eight launches whose
sparse operand reaches every reduction index (tile tails first).  Modes x3 and auto are the subject; f32 (the exact-fp32
MFMA, where the library has one for the entry point) is the control: exact by construction, so a failure there means the
probe is wrong, not the kernel.

Part a: nn.Linear in its three directions, on column slices, and scaled by powers of two.  Part b: forward values of the
chained and special kernels (set-abstraction level, shared MLP + max, the heads' three-layer chains, out projection + max
over the points, the attention blocks' weight gradients); the targeted product gets the class operands, the other
products of a chain a selection matrix (class 1), and every product of the chain is proven exact on the actual operands.

Engine names in the ids are the engine a shape is EXPECTED to take in the split-precision modes, by the shape predicates
of csrc/gemm.hip restated below; nothing here verifies which kernel ran, and the predicates leave out what does not depend
on the shape class (16-byte alignment, the LDS room pick_nt needs, the compile-time ws / df switches):
  ws       weight-stationary (wsgemm.hip): rows >= 4096, outputs >= 32 and % 4 == 0, reduction >= 16 and % 4 == 0
  df       direct-fragment weight gradient (dfgemm.hip): M >= 2048, M % 16 == 0, ceil(N/64) * ceil(K/64) <= 64
  fewrow   split-K with an atomic epilogue: M <= 128 and reduction >= 256
  general  the tile engine of gemm.hip (weight gradient: its split over the rows)
The slice test's ids name its forward only: pzn_linear_slice_dgrad_f32 always takes the general engine, and the slice
weight gradient takes it at both shapes (4100 % 16 != 0, 300 < 2048).
"""
import functools

import numpy as np
import pytest
import torch

from tests import _x3_probe as xp

pytestmark = pytest.mark.gpu
SEED = 1905


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _set_mode(mode):
    from puzzlenet_amd import _lib
    lib = _lib.load()
    old = lib.pzn_gemm_get_precision()
    _lib.check(lib.pzn_gemm_set_precision({"f32": 0, "x3": 1, "auto": 2}[mode]), "set_precision")
    return lib, old


@pytest.fixture
def precision(request):
    """The matrix-core path of one run: set, yield, restore."""
    lib, old = _set_mode(request.param)
    yield request.param
    lib.pzn_gemm_set_precision(old)


# The mode is the innermost parameter (the top decorator varies fastest), so the three runs of one case follow each other
# and share its operands and reference through a small cache.
ALL_MODES = pytest.mark.parametrize("precision", ["x3", "auto", "f32"], indirect=True)
# Entry points without an exact-fp32 engine ('unsupported' in mode f32, or the mode is not read): no control run exists.
X3_MODES = pytest.mark.parametrize("precision", ["x3", "auto"], indirect=True)
_cached = functools.lru_cache(maxsize=24)      # one case's probe set: three classes times at most eight launches


def _t(dev, x, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=dtype)).to(dev)


def _same(got, want, what):
    """got (device tensor) == want (fp32 numpy) bit for bit as numbers; the message names the first wrong entry."""
    g = got.detach().cpu().numpy()
    assert g.shape == want.shape, (what, g.shape, want.shape)
    if not np.array_equal(g, want):
        bad = np.argwhere(g != want)
        i = tuple(int(v) for v in bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {g.size} entries differ; first at {i}: got {g[i]!r}, want {want[i]!r}")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _cstr(cls):
    return f"class({cls[0]},{cls[1]})"


# ------------------------------------------------------------------------------------------ a. nn.Linear, three directions

SHAPES = [(129, 67, 33), (130, 35, 130), (1, 16, 64),                            # (M, Kin, Nout)
          (7, 257, 33), (64, 520, 70),
          (4096, 16, 32), (4100, 68, 96), (4112, 132, 256),
          (2048, 5, 7), (2048, 20, 40), (2048, 40, 20), (2064, 68, 96),
          (1000, 67, 128), (4099, 33, 130)]


def _ws(rows, outs, red):
    return rows >= 4096 and outs >= 32 and outs % 4 == 0 and red >= 16 and red % 4 == 0


def _engine(direction, M, Kin, Nout):
    if direction == "fwd":
        return "ws" if _ws(M, Nout, Kin) else "fewrow" if M <= 128 and Kin >= 256 else "general"
    if direction == "dgrad":
        return "ws" if _ws(M, Kin, Nout) else "fewrow" if M <= 128 and Nout >= 256 else "general"
    df = M >= 2048 and M % 16 == 0 and -(-Nout // 64) * -(-Kin // 64) <= 64
    return "df" if df else "general"


def _ids(direction):
    return [f"{_engine(direction, *s)}-{s[0]}x{s[1]}x{s[2]}" for s in SHAPES]


@_cached
def _fwd_case(M, Kin, Nout, cls, launch, epilogue):
    """x[M,Kin] dense, W[Nout,Kin] row-sparse; epilogue: integer bias and ReLU."""
    x, wt, room = xp.make_pair(cls, M, Kin, Nout, "b", launch, SEED)
    bias = xp.addend(np.random.default_rng([SEED, launch, M, Nout]), (Nout,), room) if epilogue else None
    y = xp.ref_bias(xp.check(x, wt, bias=bias, cls=cls), bias)
    return x, wt.T, bias, xp.as_f32(xp.ref_relu(y) if epilogue else y)


@ALL_MODES
@pytest.mark.parametrize("epilogue", [False, True], ids=["plain", "bias-relu"])
@pytest.mark.parametrize("M,Kin,Nout", SHAPES, ids=_ids("fwd"))
def test_linear_forward_exact(dev, precision, M, Kin, Nout, epilogue):
    """ops.linear forward: y = relu(x W^T + b) and y = x W^T."""
    from puzzlenet_amd import ops
    for cls in xp.CLASSES:
        _, launches = xp.probe_plan(cls, Kin, Nout)
        for launch in range(launches):
            x, w, bias, want = _fwd_case(M, Kin, Nout, cls, launch, epilogue)
            y = ops.linear(_t(dev, x), _t(dev, w), None if bias is None else _t(dev, bias), relu=epilogue)
            _same(y, want, f"y {_cstr(cls)} launch {launch}")


@_cached
def _dgrad_case(M, Kin, Nout, cls, launch):
    """dy[M,Nout] dense, gated by y_relu (a quarter exact zeros); W[Nout,Kin] sparse along Nout (column-sparse)."""
    dy, w, _ = xp.make_pair(cls, M, Nout, Kin, "b", launch, SEED + 1)
    y_relu = np.random.default_rng([SEED, 1, launch, M, Nout]).integers(0, 4, size=(M, Nout)).astype(np.float64)
    dx = xp.check(xp.ref_gate(dy, y_relu), w, cls=cls)
    return dy, y_relu, w, xp.as_f32(dx)


@ALL_MODES
@pytest.mark.parametrize("M,Kin,Nout", SHAPES, ids=_ids("dgrad"))
def test_linear_input_gradient_exact(dev, precision, M, Kin, Nout):
    """pzn_linear_dgrad_f32, as ops.linear's backward calls it: dx = (dy * [y_relu > 0]) W."""
    from puzzlenet_amd import _lib
    for cls in xp.CLASSES:
        _, launches = xp.probe_plan(cls, Nout, Kin)
        for launch in range(launches):
            dy, y_relu, w, want = _dgrad_case(M, Kin, Nout, cls, launch)
            d_dy, d_y, d_w = _t(dev, dy), _t(dev, y_relu), _t(dev, w)
            dx = torch.full((M, Kin), float("nan"), device=dev)
            _lib.call("pzn_linear_dgrad_f32", d_dy.data_ptr(), d_y.data_ptr(), d_w.data_ptr(), M, Kin, Nout, None,
                      dx.data_ptr(), _stream())
            _same(dx, want, f"dx {_cstr(cls)} launch {launch}")


@_cached
def _wgrad_case(M, Kin, Nout, cls, launch, accumulate):
    """dy[M,Nout] sparse along M, x[M,Kin] dense; accumulate: dW / db hold integers already."""
    dyt, x, room = xp.make_pair(cls, Nout, M, Kin, "a", launch, SEED + 2)
    rng = np.random.default_rng([SEED, 2, launch, M, Nout])
    nz = int((dyt[0] != 0).sum())
    room_db = xp.LIMIT - 1 - nz * int(np.abs(dyt).max())
    dw0 = xp.addend(rng, (Nout, Kin), room) if accumulate else None
    db0 = xp.addend(rng, (Nout,), room_db) if accumulate else None
    dw = xp.check(dyt, x, init=dw0, cls=cls)
    db = xp.ref_colsum(dyt.T)
    assert int((np.abs(dyt).sum(axis=1) + (0 if db0 is None else np.abs(db0))).max()) < xp.LIMIT      # c3 of the column sums
    if accumulate:
        dw, db = dw + xp.i64(dw0), db + xp.i64(db0)
    return dyt.T, x, dw0, db0, xp.as_f32(dw), xp.as_f32(db)


@ALL_MODES
@pytest.mark.parametrize("accumulate", [False, True], ids=["overwrite", "accumulate"])
@pytest.mark.parametrize("M,Kin,Nout", SHAPES, ids=_ids("wgrad"))
def test_linear_weight_and_bias_gradient_exact(dev, precision, M, Kin, Nout, accumulate):
    """pzn_linear_wgrad_f32, as ops.linear's backward calls it: dW = dy^T x, db = column sums of dy."""
    from puzzlenet_amd import _lib
    for cls in xp.CLASSES:
        _, launches = xp.probe_plan(cls, M, Nout)
        for launch in range(launches):
            dy, x, dw0, db0, want_dw, want_db = _wgrad_case(M, Kin, Nout, cls, launch, accumulate)
            d_dy, d_x = _t(dev, dy), _t(dev, x)
            dw = _t(dev, dw0) if accumulate else torch.full((Nout, Kin), float("nan"), device=dev)
            db = _t(dev, db0) if accumulate else torch.full((Nout,), float("nan"), device=dev)
            _lib.call("pzn_linear_wgrad_f32", d_dy.data_ptr(), None, d_x.data_ptr(), M, Kin, Nout, dw.data_ptr(), db.data_ptr(),
                      int(accumulate), _stream())
            _same(dw, want_dw, f"dW {_cstr(cls)} launch {launch}")
            _same(db, want_db, f"db {_cstr(cls)} launch {launch}")


# ---- the same three products on a column slice of a wider weight

@_cached
def _slice_case(M, Kin, Nout, cls, launch):
    k0, ldw = 4, Kin + 12
    rng = np.random.default_rng([SEED, 3, launch, M, Nout])
    wide = lambda: xp.draw(rng, (Nout, ldw), 3, 19)           # what surrounds the slice: large, and never to be read
    out = {}
    x, wt, room = xp.make_pair(cls, M, Kin, Nout, "b", launch, SEED + 3)
    bias, y0 = xp.addend(rng, (Nout,), room), xp.addend(rng, (M, Nout), room)
    wf = wide()
    wf[:, k0:k0 + Kin] = wt.T
    p = xp.check(x, wt, bias=bias, cls=cls)
    xp.check(x, wt, init=y0, cls=cls)                         # (accumulating ignores the bias)
    out["fwd"] = (x, wf, bias, y0, xp.as_f32(p + xp.i64(bias)), xp.as_f32(p + xp.i64(y0)))
    dy, w, room = xp.make_pair(cls, M, Nout, Kin, "b", launch, SEED + 4)
    add = xp.addend(rng, (M, Kin), room)
    wf = wide()
    wf[:, k0:k0 + Kin] = w
    p = xp.check(dy, w, init=add, cls=cls)
    out["dgrad"] = (dy, wf, add, xp.as_f32(p), xp.as_f32(p + xp.i64(add)))
    dyt, x, room = xp.make_pair(cls, Nout, M, Kin, "a", launch, SEED + 5)
    wf = wide()
    wf[:, k0:k0 + Kin] = xp.addend(rng, (Nout, Kin), room)
    db0 = xp.addend(rng, (Nout,), xp.LIMIT - 1 - int(np.abs(dyt).sum(axis=1).max()))
    want = wf.copy()
    want[:, k0:k0 + Kin] += xp.check(dyt, x, init=wf[:, k0:k0 + Kin], cls=cls)
    out["wgrad"] = (dyt.T, x, wf, db0, xp.as_f32(xp.i64(want)), xp.as_f32(xp.ref_colsum(dyt.T) + xp.i64(db0)))
    return k0, ldw, out


@ALL_MODES
@pytest.mark.parametrize("M,Kin,Nout", [(4100, 68, 96), (300, 64, 70)], ids=["fwd-ws-4100x68x96", "fwd-general-300x64x70"])
def test_linear_slice_entry_points_exact(dev, precision, M, Kin, Nout):
    """pzn_linear_slice_{fwd,dgrad,wgrad}_f32 on columns 4 .. 4 + Kin of a weight with row stride Kin + 12: forward with the
    bias and accumulating, input gradient without and with an addend, weight gradient adding into the slice (the columns
    beside it stay as they are)."""
    from puzzlenet_amd import _lib
    for cls in xp.CLASSES:
        launches = max(xp.probe_plan(cls, Kin, Nout)[1], xp.probe_plan(cls, Nout, Kin)[1], xp.probe_plan(cls, M, Nout)[1])
        for launch in range(launches):
            k0, ldw, case = _slice_case(M, Kin, Nout, cls, launch)
            tag = f"{_cstr(cls)} launch {launch}"
            x, wf, bias, y0, want_b, want_acc = case["fwd"]
            d_x, d_w, d_b = _t(dev, x), _t(dev, wf), _t(dev, bias)
            for acc, want in ((0, want_b), (1, want_acc)):
                y = _t(dev, y0) if acc else torch.full((M, Nout), float("nan"), device=dev)
                _lib.call("pzn_linear_slice_fwd_f32", d_x.data_ptr(), d_w.data_ptr() + 4 * k0, ldw, d_b.data_ptr(), M, Kin, Nout,
                          acc, y.data_ptr(), _stream())
                _same(y, want, f"slice fwd accumulate={acc} {tag}")
            dy, wf, add, want_plain, want_add = case["dgrad"]
            d_dy, d_w, d_add = _t(dev, dy), _t(dev, wf), _t(dev, add)
            for addend, want in ((None, want_plain), (d_add, want_add)):
                dx = torch.full((M, Kin), float("nan"), device=dev)
                _lib.call("pzn_linear_slice_dgrad_f32", d_dy.data_ptr(), d_w.data_ptr() + 4 * k0, ldw, M, Kin, Nout,
                          None if addend is None else addend.data_ptr(), dx.data_ptr(), _stream())
                _same(dx, want, f"slice dgrad addend={addend is not None} {tag}")
            dy, x, wf, db0, want_w, want_db = case["wgrad"]
            d_dy, d_x, dw, db = _t(dev, dy), _t(dev, x), _t(dev, wf), _t(dev, db0)
            _lib.call("pzn_linear_slice_wgrad_f32", d_dy.data_ptr(), d_x.data_ptr(), M, Kin, Nout, dw.data_ptr() + 4 * k0, ldw,
                      db.data_ptr(), _stream())
            _same(dw, want_w, f"slice wgrad dW {tag}")
            _same(db, want_db, f"slice wgrad db {tag}")


# ---- scaled: the non-reduced axes times powers of two 2^-40 .. 2^40

@_cached
def _scaled_case(direction, M, Kin, Nout, cls, launch):
    rng = np.random.default_rng([SEED, 6, launch, M, Nout])
    if direction == "fwd":
        a, b, _ = xp.make_pair(cls, M, Kin, Nout, "b", launch, SEED + 6)
    elif direction == "dgrad":
        a, b, _ = xp.make_pair(cls, M, Nout, Kin, "b", launch, SEED + 7)
    else:
        a, b, _ = xp.make_pair(cls, Nout, M, Kin, "a", launch, SEED + 8)
    sa, sb = xp.pow2_scales(rng, a.shape[0]), xp.pow2_scales(rng, b.shape[1])
    a_s, b_s = a * sa[:, None], b * sb[None, :]
    # integer planes (>= 1) times scales >= 2^-40: no plane of a scaled operand is below 2^-40, far above 2^-100
    tiny = min(float(np.abs(p[p != 0]).min()) for t in (a_s, b_s) for p in xp.split3(t.astype(np.float32)) if (p != 0).any())
    assert tiny >= 2.0 ** -40
    ref = xp.check(a_s, b_s, cls=cls, scale_a=sa, scale_b=sb)
    sums = xp.as_f32(a.sum(axis=1)[:, None], sa)[:, 0] if direction == "wgrad" else None
    return a_s, b_s, xp.as_f32(ref, sa, sb), sums


@ALL_MODES
@pytest.mark.parametrize("direction,M,Kin,Nout", [
    ("fwd", 129, 67, 33), ("fwd", 7, 257, 33), ("fwd", 4100, 68, 96), ("dgrad", 129, 67, 33), ("dgrad", 4100, 68, 96),
    ("wgrad", 2064, 68, 96), ("wgrad", 1000, 67, 128)],
    ids=["fwd-general", "fwd-fewrow", "fwd-ws", "dgrad-general", "dgrad-ws", "wgrad-df", "wgrad-general"])
def test_linear_scaled_exact(dev, precision, direction, M, Kin, Nout):
    """Rows of a and columns of b (never the reduced axis) times powers of two in 2^-40 .. 2^40, no bias: the result is the
    scaled integers exactly - the split works on the significand whatever the exponent, within the range the probes
    cover (smallest plane >= 2^-40 here; where plane 3 would underflow is not probed)."""
    from puzzlenet_amd import _lib, ops
    red, outs = {"fwd": (Kin, Nout), "dgrad": (Nout, Kin), "wgrad": (M, Nout)}[direction]
    for cls in xp.CLASSES:
        for launch in range(xp.probe_plan(cls, red, outs)[1]):
            a, b, want, sums = _scaled_case(direction, M, Kin, Nout, cls, launch)
            tag = f"scaled {direction} {_cstr(cls)} launch {launch}"
            if direction == "fwd":
                _same(ops.linear(_t(dev, a), _t(dev, b.T), None, relu=False), want, tag)
            elif direction == "dgrad":
                d_dy, d_w = _t(dev, a), _t(dev, b)
                dx = torch.full((M, Kin), float("nan"), device=dev)
                _lib.call("pzn_linear_dgrad_f32", d_dy.data_ptr(), None, d_w.data_ptr(), M, Kin, Nout, None, dx.data_ptr(), _stream())
                _same(dx, want, tag)
            else:
                d_dy, d_x = _t(dev, a.T), _t(dev, b)
                dw, db = torch.full((Nout, Kin), float("nan"), device=dev), torch.full((Nout,), float("nan"), device=dev)
                _lib.call("pzn_linear_wgrad_f32", d_dy.data_ptr(), None, d_x.data_ptr(), M, Kin, Nout, dw.data_ptr(), db.data_ptr(),
                          0, _stream())
                _same(dw, want, tag)
                _same(db, sums, tag + " db")


# ------------------------------------------------------------------------------------------ b. chained and special kernels

def _selection(n_out, n_in, rng=None):
    """W[n_out, n_in] with one non-zero per row, at column (row mod n_in): 1, or a random sign with rng.  A class-1 operand
    that hands its input on unchanged, so the other products of a chain stay exact whatever the planes of their input."""
    w = np.zeros((n_out, n_in))
    w[np.arange(n_out), np.arange(n_out) % n_in] = 1.0 if rng is None else rng.integers(0, 2, size=n_out) * 2.0 - 1.0
    return w


def _argmax_attains(y, arg, out, what):
    """y[G, rows, C] int64 reference rows, arg[G, C] the kernel's row: it must attain the maximum (ties are common with
    integers; which of the tied rows is named is pinned elsewhere)."""
    a = arg.detach().cpu().numpy().astype(np.int64)
    assert a.min() >= 0 and a.max() < y.shape[1], what
    picked = np.take_along_axis(y, a[:, None, :], axis=1)[:, 0, :]
    assert np.array_equal(picked, out), what


# ---- the set-abstraction level: out = max_k relu(relu(P[idx] + Q) W2^T + b2)

@_cached
def _sa_case(B, N, S, C1, C2, cls, launch):
    """Integer P, Q, idx, W2, b2.  P holds the class values; Q is 0 or -2^20 (the ReLU then zeroes that column of the
    group: Q takes part, and P + Q stays an exact integer of the same class or zero); W2 row-sparse."""
    v, w2t, room = xp.make_pair(cls, B * N, C1, C2, "b", launch, SEED + 10)
    rng = np.random.default_rng([SEED, 10, launch, B, S, C1, C2])
    G = B * S
    q = np.where(rng.integers(0, 8, size=(G, C1)) == 0, -float(1 << 20), 0.0)
    idx = rng.integers(0, N, size=(B, S, 32))
    b2 = xp.addend(rng, (C2,), room)
    rows = v.reshape(B, N, C1)[np.arange(B)[:, None, None], idx] + q.reshape(B, S, 1, C1)         # [B, S, 32, C1]
    assert np.abs(rows).max() < xp.LIMIT
    rows = np.maximum(rows, 0.0).reshape(G * 32, C1)
    y = xp.ref_relu(xp.ref_bias(xp.check(rows, w2t, bias=b2, cls=cls), b2))
    return v, q, idx, w2t.T, b2, y.reshape(G, 32, C2), xp.ref_max_rows(y, 32)


@X3_MODES
@pytest.mark.parametrize("C1,C2", [(128, 128), (256, 256), (256, 64), (256, 128)])
@pytest.mark.parametrize("B,N,S", [(1, 40, 8), (3, 50, 33), (2, 70, 65)], ids=["G8", "G99", "G130"])
def test_sa_level_forward_exact(dev, precision, B, N, S, C1, C2):
    """pzn_sa_level_fwd_f32 (weight-stationary kernel, generated rows), pzn_sa_level_fwd_ws_f32 (streamed weight planes
    where C1 = C2, else the former) and pzn_sa_level_prep_weights_f32 + pzn_sa_level_fwd_packed_f32 (C1 = C2): `out` exact,
    `argmax` names a row that attains it."""
    from puzzlenet_amd import _lib
    lib = _lib.load()
    G = B * S
    nbytes = lib.pzn_sa_level_fwd_workspace_bytes(C1, C2)
    assert nbytes == (C1 * C2 * 6 if C1 == C2 else 0)
    for cls in xp.CLASSES:
        for launch in range(xp.probe_plan(cls, C1, C2)[1]):
            v, q, idx, w2, b2, y, want = _sa_case(B, N, S, C1, C2, cls, launch)
            P, Q, W2, b2d = _t(dev, v), _t(dev, q), _t(dev, w2), _t(dev, b2)
            I = _t(dev, idx, np.int64)
            st = _stream()
            entries = ["fwd", "fwd_ws"] + (["packed"] if nbytes else [])
            for entry in entries:
                out = torch.full((G, C2), float("nan"), device=dev)
                arg = torch.full((G, C2), -1, dtype=torch.int32, device=dev)
                ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
                if entry == "fwd":
                    _lib.call("pzn_sa_level_fwd_f32", P.data_ptr(), Q.data_ptr(), I.data_ptr(), W2.data_ptr(), b2d.data_ptr(), B, N, S,
                              C1, C2, out.data_ptr(), arg.data_ptr(), st)
                elif entry == "fwd_ws":
                    _lib.call("pzn_sa_level_fwd_ws_f32", P.data_ptr(), Q.data_ptr(), I.data_ptr(), W2.data_ptr(), b2d.data_ptr(), B, N,
                              S, C1, C2, out.data_ptr(), arg.data_ptr(), ws.data_ptr() if nbytes else None, st)
                else:
                    _lib.call("pzn_sa_level_prep_weights_f32", W2.data_ptr(), C1, C2, ws.data_ptr(), st)
                    _lib.call("pzn_sa_level_fwd_packed_f32", P.data_ptr(), Q.data_ptr(), I.data_ptr(), b2d.data_ptr(), B, N, S, C1, C2,
                              out.data_ptr(), arg.data_ptr(), ws.data_ptr(), st)
                tag = f"sa level {entry} {_cstr(cls)} launch {launch}"
                _same(out, xp.as_f32(want), tag)
                _argmax_attains(y, arg, want, tag + " argmax")


# ---- ops.shared_mlp_max: relu(x W1^T + b1) -> relu(. W2^T + b2) -> max over 32 rows

@_cached
def _smm_case(R, C0, C1, C2, layer, cls, launch):
    """The targeted layer gets the class operands, the other one a selection matrix (class 1)."""
    rng = np.random.default_rng([SEED, 11, launch, R, C0, layer])
    M = R * 32
    if layer == 1:
        x, w1t, room = xp.make_pair(cls, M, C0, C1, "b", launch, SEED + 11)
        b1 = xp.addend(rng, (C1,), room // 2)
        h = xp.ref_relu(xp.ref_bias(xp.check(x, w1t, bias=b1, cls=cls), b1))
        w2 = _selection(C2, C1, rng)
        b2 = xp.addend(rng, (C2,), room // 2)
        y = xp.check(h, w2.T, bias=b2)
        w1 = w1t.T
    else:
        a, w2t, room = xp.make_pair(cls, M, C1, C2, "b", launch, SEED + 12)
        x = a[:, :C0]
        w1, b1 = _selection(C1, C0), np.zeros(C1)
        h = xp.ref_relu(xp.check(x, w1.T, bias=b1, cls=(cls[0], 1)))
        b2 = xp.addend(rng, (C2,), room)
        y = xp.check(h, w2t, bias=b2, cls=cls)
        w2 = w2t.T
    out = xp.ref_max_rows(xp.ref_relu(xp.ref_bias(y, b2)), 32)
    return x, w1, b1, w2, b2, xp.as_f32(out)


@ALL_MODES
@pytest.mark.parametrize("layer", [1, 2])
@pytest.mark.parametrize("B,S,C0,C1,C2", [(1, 5, 20, 32, 48), (4, 32, 68, 128, 128)])
def test_shared_mlp_max_forward_exact(dev, precision, B, S, C0, C1, C2, layer):
    from puzzlenet_amd import ops
    red, outs = ((C0, C1), (C1, C2))[layer - 1]
    for cls in xp.CLASSES:
        for launch in range(xp.probe_plan(cls, red, outs)[1]):
            x, w1, b1, w2, b2, want = _smm_case(B * S, C0, C1, C2, layer, cls, launch)
            y = ops.shared_mlp_max(_t(dev, x).view(B, S, 32, C0), _t(dev, w1), _t(dev, b1), _t(dev, w2), _t(dev, b2))
            _same(y.reshape(B * S, C2), want, f"shared_mlp_max layer {layer} {_cstr(cls)} launch {launch}")


# ---- the boundary heads' three-layer chains (csrc/pointmlp.hip): ops.point_mlp3 and ops.pair_head

@_cached
def _mlp3_weights(rows, C2, C3, n_g, layer, cls, launch):
    """64 -> 64 -> C2 -> C3 with the class operands in `layer` and selection matrices elsewhere; n_g > 0: a global half
    g[n_g, 64] W1g^T of the first layer (it may only add to the targeted layer 1: elsewhere W1g = 0 keeps the rows'
    class).  Returns x[rows, 64], g, (W1g, W1x, b1, W2, b2, W3, b3) and the classes to check each layer against."""
    dims = (64, 64, C2, C3)
    rng = np.random.default_rng([SEED, 13, launch, rows, C2, layer, n_g])
    a, bt, room = xp.make_pair(cls, rows, dims[layer - 1], dims[layer], "b", launch, SEED + 13)
    x = np.zeros((rows, 64))
    x[:, :a.shape[1]] = a
    ws, bs, classes = [], [], []
    for l in (1, 2, 3):
        if l == layer:
            ws.append(bt.T)
            bs.append(xp.addend(rng, (dims[l],), room // 4))
            classes.append(cls)
        else:
            ws.append(_selection(dims[l], dims[l - 1], rng if l > layer else None))
            bs.append(xp.addend(rng, (dims[l],), 7) if l > layer else np.zeros(dims[l]))
            classes.append((cls[0], 1) if l < layer else None)
    g = w1g = None
    if n_g:
        g = rng.integers(-3, 4, size=(n_g, 64)).astype(np.float64)
        w1g = _selection(64, 64, rng) if layer == 1 else np.zeros((64, 64))
    return x, g, w1g, ws, bs, tuple(classes)


def _mlp3_ref(x_rows, bias1_rows, ws, bs, classes):
    """The chain on materialised rows in int64, every layer proven exact: (x W1x^T + bias1) -> ReLU -> W2, b2 -> ReLU -> W3, b3."""
    h = xp.ref_relu(xp.check(x_rows, ws[0].T, bias=bias1_rows, cls=classes[0]) + xp.i64(bias1_rows))
    h = xp.ref_relu(xp.ref_bias(xp.check(h, ws[1].T, bias=bs[1], cls=classes[1]), bs[1]))
    return xp.ref_bias(xp.check(h, ws[2].T, bias=bs[2], cls=classes[2]), bs[2])


@_cached
def _point_mlp3_case(B, N, C2, C3, per_cloud, layer, cls, launch):
    x, g, w1g, ws, bs, classes = _mlp3_weights(B * N, C2, C3, B if per_cloud else 0, layer, cls, launch)
    if per_cloud:
        c = xp.ref_bias(xp.check(g, w1g.T, bias=bs[0]), bs[0])                       # [B, 64], the per-cloud bias
        bias1 = np.repeat(c, N, axis=0).astype(np.float64)
    else:
        bias1 = np.broadcast_to(bs[0], (B * N, 64))
    return x, g, w1g, ws, bs, xp.as_f32(_mlp3_ref(x, bias1, ws, bs, classes))


@X3_MODES
@pytest.mark.parametrize("layer", [1, 2, 3])
@pytest.mark.parametrize("B,N,C2,C3,per_cloud", [(1, 32, 32, 2, True), (3, 160, 64, 64, False)])
def test_point_mlp3_forward_exact(dev, precision, B, N, C2, C3, per_cloud, layer):
    """ops.point_mlp3 forward, each of its three products in turn with the class operands."""
    from puzzlenet_amd import ops
    assert ops.point_mlp3_available(64, 64, C2, C3)
    dims = (64, 64, C2, C3)
    for cls in xp.CLASSES:
        for launch in range(xp.probe_plan(cls, dims[layer - 1], dims[layer])[1]):
            x, g, w1g, ws, bs, want = _point_mlp3_case(B, N, C2, C3, per_cloud, layer, cls, launch)
            w1 = np.concatenate([w1g, ws[0]], axis=1) if per_cloud else ws[0]
            y = ops.point_mlp3(_t(dev, x).view(B, N, 64), _t(dev, w1), _t(dev, bs[0]), _t(dev, ws[1]), _t(dev, bs[1]),
                               _t(dev, ws[2]), _t(dev, bs[2]), g=_t(dev, g).view(B, 1, 64) if per_cloud else None)
            _same(y.reshape(B * N, C3), want, f"point_mlp3 layer {layer} {_cstr(cls)} launch {launch}")


@_cached
def _pair_head_case(Kf, Km, N, layer, cls, launch):
    x, g, w1g, ws, bs, classes = _mlp3_weights(Kf * N, 32, 2, Km, layer, cls, launch)
    c = xp.ref_bias(xp.check(g, w1g.T, bias=bs[0]), bs[0]).astype(np.float64)        # [Km, 64]
    x_pairs = np.broadcast_to(x.reshape(Kf, 1, N, 64), (Kf, Km, N, 64)).reshape(-1, 64)
    c_pairs = np.broadcast_to(c.reshape(1, Km, 1, 64), (Kf, Km, N, 64)).reshape(-1, 64)
    return x, g, w1g, ws, bs, xp.as_f32(_mlp3_ref(x_pairs, c_pairs, ws, bs, classes)).reshape(Kf, Km, N, 2)


@X3_MODES
@pytest.mark.parametrize("layer", [1, 2, 3])
@pytest.mark.parametrize("Kf,Km,N", [(1, 1, 32), (3, 5, 96)])
def test_pair_head_forward_exact(dev, precision, Kf, Km, N, layer):
    """ops.pair_head (the 128 -> 64 -> 32 -> 2 chain over every (fixed, moved) pair), each product in turn."""
    from puzzlenet_amd import ops
    dims = (64, 64, 32, 2)
    for cls in xp.CLASSES:
        for launch in range(xp.probe_plan(cls, dims[layer - 1], dims[layer])[1]):
            x, g, w1g, ws, bs, want = _pair_head_case(Kf, Km, N, layer, cls, launch)
            y = ops.pair_head(_t(dev, x).view(Kf, N, 64), _t(dev, g), _t(dev, np.concatenate([w1g, ws[0]], axis=1)), _t(dev, bs[0]),
                              _t(dev, ws[1]), _t(dev, bs[1]), _t(dev, ws[2]), _t(dev, bs[2]))
            _same(y, want, f"pair_head layer {layer} {_cstr(cls)} launch {launch}")


# ---- the encoder's out projection with the max over the points (csrc/outproj.hip)

OUTPROJ_LAUNCHES = 3        # (nz = 16 on the 1280-long reduction: 32 * 16 * 3 >= 1280)


@_cached
def _outproj_case(B, cls, launch):
    L, E, Nout = 256, 256, 1024
    x, wt, room = xp.make_pair(cls, B * L, 5 * E, Nout, "b", launch, SEED + 14, max_launches=OUTPROJ_LAUNCHES)
    bias = xp.addend(np.random.default_rng([SEED, 14, launch, B]), (Nout,), room)
    y = xp.ref_bias(xp.check(x, wt, bias=bias, cls=cls), bias)
    return x, wt.T, bias, y.reshape(B, L, Nout), xp.ref_max_points(y.reshape(B, L, Nout))


@X3_MODES
@pytest.mark.parametrize("B", [2, 5])
def test_outproj_maxpts_forward_exact(dev, precision, B):
    """pzn_outproj_maxpts_fwd_f32 with and without `out`: the projection, its maximum over the 256 points, and an arg-max
    that attains it."""
    from puzzlenet_amd import _lib, ops
    L, E, Nout = 256, 256, 1024
    M = B * L
    lib = _lib.load()
    ws = torch.empty(lib.pzn_outproj_maxpts_workspace_bytes(L, E, 5, Nout), dtype=torch.uint8, device=dev)
    assert ws.numel() > 0
    for cls in xp.CLASSES:
        nz, launches = xp.probe_plan(cls, 5 * E, Nout, max_launches=OUTPROJ_LAUNCHES)
        assert xp.covered(5 * E, Nout, nz, launches).all()
        for launch in range(launches):
            x, w, bias, y, ymax = _outproj_case(B, cls, launch)
            xd = [_t(dev, x[:, i * E:(i + 1) * E]) for i in range(5)]
            wd, bd = _t(dev, w), _t(dev, bias)
            for need_out in (True, False):
                out = torch.full((M, Nout), float("nan"), device=dev) if need_out else None
                fmax = torch.full((B, Nout), float("nan"), device=dev)
                arg = torch.full((B, Nout), -1, dtype=torch.int32, device=dev)
                _lib.call("pzn_outproj_maxpts_fwd_f32", ops._ptrs(xd), 5, wd.data_ptr(), bd.data_ptr(), B, L, E, Nout,
                          out.data_ptr() if need_out else None, fmax.data_ptr(), arg.data_ptr(), ws.data_ptr(), _stream())
                tag = f"outproj out={need_out} {_cstr(cls)} launch {launch}"
                if need_out:
                    _same(out, xp.as_f32(y.reshape(M, Nout)), tag)
                _same(fmax, xp.as_f32(ymax), tag + " max")
                _argmax_attains(y, arg, ymax, tag + " argmax")


# ---- the attention blocks' weight gradients in one launch (csrc/attnwgrad.hip)

@_cached
def _attn_wgrad_case(M, cls, launch, accumulate):
    """dWo = dz^T t, dWq/k/v = dq/dk/dv^T x and the four column sums: the gradients sparse along M, t and x dense."""
    E, dk = 256, 64
    rng = np.random.default_rng([SEED, 15, launch, M])
    dzt, t, room = xp.make_pair(cls, E, M, E, "a", launch, SEED + 15)
    dvt, x, _ = xp.make_pair(cls, E, M, E, "a", launch, SEED + 16)
    dqt = xp.make_pair(cls, dk, M, E, "a", launch, SEED + 17)[0]
    dkt = xp.make_pair(cls, dk, M, E, "a", launch, SEED + 18)[0]
    ins = dict(dz=dzt.T, t=t, dq=dqt.T, dk=dkt.T, dv=dvt.T, x=x)
    want, init = [], []
    for gt, act in ((dqt, x), (dkt, x), (dvt, x), (dzt, t)):                        # dWq dbq dWk dbk dWv dbv dWo dbo
        colsum = np.abs(gt).sum(axis=1)
        w0 = xp.addend(rng, (gt.shape[0], E), room) if accumulate else None
        b0 = xp.addend(rng, (gt.shape[0],), xp.LIMIT - 1 - int(colsum.max())) if accumulate else None
        dw, db = xp.check(gt, act, init=w0, cls=cls), xp.ref_colsum(gt.T)
        assert int((colsum + (0 if b0 is None else np.abs(b0))).max()) < xp.LIMIT
        if accumulate:
            dw, db = dw + xp.i64(w0), db + xp.i64(b0)
        want += [xp.as_f32(dw), xp.as_f32(db)]
        init += [w0, b0]
    return ins, init, want


@ALL_MODES
@pytest.mark.parametrize("accumulate", [False, True], ids=["overwrite", "accumulate"])
@pytest.mark.parametrize("M", [64, 1280])
def test_attention_weight_gradients_exact(dev, precision, M, accumulate):
    """pzn_attn_fused_wgrads at E = 256, dk = 64 (mode f32: the general weight-gradient kernels): all eight outputs."""
    from puzzlenet_amd import _lib
    E, dk = 256, 64
    shapes = ((dk, E), (dk,), (dk, E), (dk,), (E, E), (E,), (E, E), (E,))
    for cls in xp.CLASSES:
        for launch in range(xp.probe_plan(cls, M, E)[1]):
            ins, init, want = _attn_wgrad_case(M, cls, launch, accumulate)
            d = {k: _t(dev, v) for k, v in ins.items()}
            outs = [_t(dev, i0) if accumulate else torch.full(s, float("nan"), device=dev) for i0, s in zip(init, shapes)]
            _lib.call("pzn_attn_fused_wgrads", d["dz"].data_ptr(), d["t"].data_ptr(), d["dq"].data_ptr(), d["dk"].data_ptr(),
                      d["dv"].data_ptr(), d["x"].data_ptr(), M, E, dk, *[o.data_ptr() for o in outs], int(accumulate), _stream())
            for name, got, w in zip("dWq dbq dWk dbk dWv dbv dWo dbo".split(), outs, want):
                _same(got, w, f"attn wgrads {name} {_cstr(cls)} launch {launch}")
