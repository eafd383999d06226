"""Exact integer probes of the bf16x3 product (csrc/pzn_x3.h), CPU side: numpy only, nothing here touches a GPU.

A matrix-core kernel splits each operand into three bf16 planes and sums the six products (1,1) (1,2) (2,1) (1,3) (2,2)
(3,1) in fp32.  With integer operands for which every kept product and every partial sum is an integer below 2^24, the
result is the integer product whatever the order of the sum, so a kernel is compared with `==`, and a plane that is
lost, stale or misplaced gives a wrong integer.  Three operand classes (planes of a, planes of b) are exact under the
full recipe - planes(a) + planes(b) <= 4 makes the three dropped products vanish - and between them need each of the six:

    class (3,1) needs (3,1) (2,1) (1,1)      class (1,3) needs (1,3) (1,2) (1,1)      class (2,2) needs (2,2) (2,1) (1,2) (1,1)

Every product here is a[M,K] @ b[K,N]: one operand dense, the other with `nz` non-zeros per output along K, placed
deterministically (sparse_positions).  `check` proves c1-c4 for the operands at hand before anything is launched; the
int64 references of the operations built on the product are at the end.
"""
import math

import numpy as np

CLASSES = ((3, 1), (1, 3), (2, 2))
PRODUCTS = ((0, 0), (0, 1), (1, 0), (0, 2), (1, 1), (2, 0))      # the six kept (plane of a, plane of b), zero-based
LIMIT = 1 << 24                                                  # integers below it are fp32 values, and so are their sums
TILE = 32                                                        # outputs per placement group (the narrowest MFMA tile)
MAX_LAUNCHES = 8


# ------------------------------------------------------------------------------------------ the split, in numpy

def bf16(x):
    """fp32 -> the nearest bf16 (ties to even) as an fp32 value: v_cvt_pk_bf16_f32 on finite inputs."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    r = (u + (np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1)))) & np.uint32(0xFFFF0000)
    return r.view(np.float32)


def split3(x):
    """pzn_x3.h split3: x1 = bf16(x), x2 = bf16(x - x1), x3 = bf16(x - x1 - x2); remainders are fp32 subtractions."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    p1 = bf16(x)
    r = x - p1
    p2 = bf16(r)
    r2 = r - p2
    return p1, p2, bf16(r2)


def planes(x):
    """Number of non-zero planes of every element (0 for a zero)."""
    return sum((p != 0).astype(np.int8) for p in split3(x))


def six_products(a, b, drop=(), pa=None, pb=None):
    """The recipe emulated: a[M,K] @ b[K,N] as the sum, in fp32, of the kept plane products.  drop: products left out, as
    one-based (plane of a, plane of b).  pa / pb: the planes to use instead of split3's (to damage them)."""
    pa = split3(a) if pa is None else pa
    pb = split3(b) if pb is None else pb
    acc = np.zeros((pa[0].shape[0], pb[0].shape[1]), dtype=np.float32)
    for i, j in reversed(PRODUCTS):                              # small terms first, as mma_x3 issues them
        if (i + 1, j + 1) not in drop:
            acc = acc + pa[i] @ pb[j]
    return acc


# ------------------------------------------------------------------------------------------ operand builders

def widths(cls, nz):
    """(bits of a, bits of b, room): widths with bits(a) + bits(b) + ceil(log2 nz) <= 24 for the class, and what is left
    below 2^24 for a bias or an initial content beside the largest possible sum of nz products.  A class-3 operand takes
    18 or 19 bits (17 is the least the class allows on paper, but an odd 17-bit value always fits two planes), a class-2
    operand 9 to 11, a class-1 operand 1 to 3."""
    total = 24 - max(0, math.ceil(math.log2(nz)))
    if cls == (2, 2):
        ba = bb = min(11, total // 2)
        ok = ba >= 9
    else:
        b3 = min(19, total - 1)
        b1 = min(3, total - b3)
        ok = b3 >= 18 and b1 >= 1
        ba, bb = (b3, b1) if cls == (3, 1) else (b1, b3)
    if not ok:
        raise ValueError(f"class {cls} has no widths for nz = {nz}")
    assert ba + bb + max(0, math.ceil(math.log2(nz))) <= 24
    return ba, bb, LIMIT - 1 - nz * ((1 << ba) - 1) * ((1 << bb) - 1)


def max_nz(cls):
    return 64 if cls == (2, 2) else 32


def draw(rng, shape, p, bits):
    """Integers (as float64) of `bits` bits with random sign, the top and the bottom bit set, and exactly p non-zero
    planes: an entry with another count is drawn again."""
    lo, hi = {1: (1, 8), 2: (9, 16), 3: (17, 24)}[p]
    assert lo <= bits <= hi, (p, bits)
    n = int(np.prod(shape))
    out = np.zeros(n, dtype=np.int64)
    todo = np.arange(n)
    for _ in range(200):
        if todo.size == 0:
            break
        v = np.ones(todo.size, dtype=np.int64)
        if bits > 1:
            v |= np.int64(1) << np.int64(bits - 1)
        if bits > 2:
            v |= rng.integers(0, 1 << (bits - 2), size=todo.size, dtype=np.int64) << np.int64(1)
        v *= rng.integers(0, 2, size=todo.size, dtype=np.int64) * 2 - 1
        out[todo] = v
        todo = todo[planes(v.astype(np.float32)) != p]
    assert todo.size == 0, f"no {bits}-bit value with {p} planes found for {todo.size} entries"
    return out.reshape(shape).astype(np.float64)


def priority_indices(K):
    """Reduction indices a placement serves first: the first and the last, and around a K tail (K % 16, K % 32 - the k
    extent of one and of two MFMA steps) the last index before it and every index of it."""
    pri = [0, K - 1]
    for step in (16, 32):
        if K % step and K > step:
            pri += list(range(K - K % step - 1, K))
    seen, out = set(), []
    for k in pri:
        if k not in seen:
            seen.add(k)
            out.append(k)
    return out


def _order(K):
    pri = priority_indices(K)
    rest = sorted(set(range(K)) - set(pri))
    return np.array(pri + rest, dtype=np.int64)


def choose_nz(cls, K, n_out, max_launches=MAX_LAUNCHES):
    """The smallest power of two >= 4 with which max_launches launches reach every reduction index in a group of TILE
    outputs, capped by what the class's widths allow and by K."""
    t = min(TILE, n_out)
    nz = 4
    while nz < max_nz(cls) and t * nz * max_launches < K:
        nz *= 2
    return min(nz, K)


def n_launches(K, n_out, nz, max_launches=MAX_LAUNCHES):
    """Launches of one probe set: enough for every group of TILE outputs to reach every reduction index, and for a ragged
    last group to reach the priority indices; at most max_launches."""
    t = min(TILE, n_out)
    need = -(-K // (t * nz))
    r = n_out % t
    if r:
        need = max(need, -(-min(K, len(priority_indices(K))) // (r * nz)))
    return max(1, min(max_launches, need))


def sparse_positions(K, n_out, nz, launch):
    """[n_out, nz] reduction indices of the sparse operand's non-zeros: output n of a group of TILE takes entries
    launch * TILE * nz + (n % TILE) * nz ... + nz - 1 (mod K) of the index order 'priority indices, then the rest' (a
    ragged last group of r outputs: launch * r * nz + ..., so that it reaches the priority indices first)."""
    assert 1 <= nz <= K
    t = min(TILE, n_out)
    n = np.arange(n_out)
    size = np.where(n < n_out - n_out % t, t, n_out % t)         # a ragged last group advances by its own size
    base = launch * size * nz + (n % t) * nz
    return _order(K)[(base[:, None] + np.arange(nz)[None, :]) % K]


def covered(K, n_out, nz, launches):
    """[groups, K] bool: which reduction indices each group of TILE outputs has reached over the probe set."""
    t = min(TILE, n_out)
    groups = -(-n_out // t)
    hit = np.zeros((groups, K), dtype=bool)
    for l in range(launches):
        pos = sparse_positions(K, n_out, nz, l)
        for g in range(groups):
            hit[g, pos[g * t:(g + 1) * t].ravel()] = True
    return hit


def make_pair(cls, M, K, N, sparse, launch, seed, nz=None, max_launches=MAX_LAUNCHES):
    """Operands of one probe: a[M,K], b[K,N] (float64 holding integers) of class cls for a @ b.  sparse = 'b': every column
    of b has nz non-zeros (outputs grouped along N); sparse = 'a': every row of a has (outputs grouped along M).  Returns
    (a, b, room): room = what a bias / initial content may add in magnitude (c3)."""
    n_out = N if sparse == "b" else M
    nz = choose_nz(cls, K, n_out, max_launches) if nz is None else min(nz, K)
    ba, bb, room = widths(cls, nz)
    rng = np.random.default_rng([seed, launch, cls[0], cls[1], M, K, N])
    pos = sparse_positions(K, n_out, nz, launch)
    if sparse == "b":
        a = draw(rng, (M, K), cls[0], ba)
        b = np.zeros((K, N))
        b[pos, np.arange(N)[:, None]] = draw(rng, (N, nz), cls[1], bb)
    else:
        b = draw(rng, (K, N), cls[1], bb)
        a = np.zeros((M, K))
        a[np.arange(M)[:, None], pos] = draw(rng, (M, nz), cls[0], ba)
    return a, b, room


def probe_plan(cls, K, n_out, max_launches=MAX_LAUNCHES):
    """(nz, launches) of the probe set of one shape and class."""
    nz = choose_nz(cls, K, n_out, max_launches)
    return nz, n_launches(K, n_out, nz, max_launches)


def addend(rng, shape, room):
    """Integer bias / initial content: random sign, magnitude below min(room, 2^22) + 1."""
    m = int(min(room, 1 << 22))
    return rng.integers(-m, m + 1, size=shape).astype(np.float64)


def pow2_scales(rng, n, lo=-40, hi=40):
    """n powers of two 2^lo .. 2^hi (float64), both ends present when n >= 2."""
    e = rng.integers(lo, hi + 1, size=n)
    if n >= 2:
        e[0], e[-1] = lo, hi
    return np.ldexp(1.0, e)


# ------------------------------------------------------------------------------------------ the proof obligations

def check(a, b, bias=None, init=None, cls=None, scale_a=None, scale_b=None):
    """Assert, for a[M,K] @ b[K,N] (+ bias[N] or [M,N]) (+ init[M,N]), in int64:
      c1  every entry is an integer - of a after dividing row m by scale_a[m], of b after dividing column n by scale_b[n]
          (powers of two, constant along the reduction axis);
      c2  planes(a[m,k]) + planes(b[k,n]) <= 4 wherever both are non-zero, so the three dropped products are zero;
      c3  sum_k |a||b| + |bias| + |init| < 2^24 for every output (in the unscaled integers);
      c4  with cls = (pa, pb): every non-zero of a has exactly pa planes, of b exactly pb.
    Returns the int64 product of the unscaled integers."""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    assert a.ndim == 2 and b.ndim == 2 and a.shape[1] == b.shape[0], (a.shape, b.shape)
    for s, name in ((scale_a, "scale_a"), (scale_b, "scale_b")):
        if s is not None:
            m, _ = np.frexp(np.asarray(s, dtype=np.float64))
            assert np.all(m == 0.5), f"c1: {name} is not a power of two"
    ai = a if scale_a is None else a / np.asarray(scale_a, dtype=np.float64)[:, None]
    bi = b if scale_b is None else b / np.asarray(scale_b, dtype=np.float64)[None, :]
    for x, name in ((ai, "a"), (bi, "b"), (bias, "bias"), (init, "init")):
        if x is not None:
            x = np.asarray(x, dtype=np.float64)
            assert np.all(np.isfinite(x)) and np.all(x == np.rint(x)), f"c1: {name} holds a non-integer"
            assert np.all(np.abs(x) < LIMIT), f"c1: {name} holds an integer that is no fp32 value"
    a32, b32 = a.astype(np.float32), b.astype(np.float32)
    assert np.array_equal(a32.astype(np.float64), a) and np.array_equal(b32.astype(np.float64), b), "c1: not fp32 values"
    pa, pb = planes(a32), planes(b32)
    if int(pa.max(initial=0)) + int(pb.max(initial=0)) > 4:      # (else no pair can exceed 4)
        meet = np.zeros((a.shape[0], b.shape[1]), dtype=np.float32)
        for i, j in ((3, 2), (2, 3), (3, 3)):
            meet += (pa == i).astype(np.float32) @ (pb == j).astype(np.float32)
        assert not meet.any(), f"c2: {int((meet > 0).sum())} outputs sum a pair with more than four planes"
    tot = np.rint(np.abs(ai) @ np.abs(bi)).astype(np.int64)      # (float64 sums of integers far below 2^53: exact)
    for x in (bias, init):
        if x is not None:
            tot = tot + np.rint(np.abs(np.asarray(x, dtype=np.float64))).astype(np.int64)
    assert int(tot.max(initial=0)) < LIMIT, f"c3: sum |a||b| + |bias| + |init| reaches {int(tot.max())} >= 2^24"
    if cls is not None:
        for p, want, name in ((pa, cls[0], "a"), (pb, cls[1], "b")):
            bad = (p != 0) & (p != want)
            assert not bad.any(), f"c4: {int(bad.sum())} non-zeros of {name} do not have exactly {want} planes"
    return np.rint(ai @ bi).astype(np.int64)


# ------------------------------------------------------------------------------------------ int64 references

def i64(x):
    x = np.asarray(x, dtype=np.float64)
    assert np.all(x == np.rint(x))
    return np.rint(x).astype(np.int64)


def ref_product(a, b):
    """a @ b of integer operands in int64 (through float64, exact while every sum stays below 2^53; check bounds it by
    2^24)."""
    return np.rint(np.asarray(a, dtype=np.float64) @ np.asarray(b, dtype=np.float64)).astype(np.int64)


def ref_bias(y, bias):
    return y if bias is None else y + i64(bias)


def ref_relu(y):
    return np.maximum(y, 0)


def ref_gate(dy, y_relu):
    """dy * [y_relu > 0]: the ReLU gate on a gradient operand."""
    return np.where(np.asarray(y_relu) > 0, np.asarray(dy, dtype=np.float64), 0.0)


def ref_max_rows(y, rows=32):
    """y[R * rows, C] -> max over each group of `rows` consecutive rows: [R, C]."""
    return y.reshape(-1, rows, y.shape[-1]).max(axis=1)


def ref_max_points(y):
    """y[B, L, C] -> max over the points: [B, C]."""
    return y.max(axis=1)


def ref_colsum(dy):
    return i64(dy).sum(axis=0)


def as_f32(y, scale_rows=None, scale_cols=None):
    """An int64 reference as the fp32 array a kernel must return bit for bit, optionally times the power-of-two scales."""
    y = np.asarray(y).astype(np.float64)
    if scale_rows is not None:
        y = y * np.asarray(scale_rows, dtype=np.float64)[:, None]
    if scale_cols is not None:
        y = y * np.asarray(scale_cols, dtype=np.float64)[None, :]
    out = y.astype(np.float32)
    assert np.array_equal(out.astype(np.float64), y), "the reference is no fp32 value"
    return out
