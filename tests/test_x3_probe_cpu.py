"""The exact-integer probes of tests/_x3_probe.py discriminate: on the CPU emulation of pzn_x3.h's recipe every class is
exact under the six products, the loss of any one product - everywhere, or only beyond a K tail boundary - changes the
integer result of some class, and `check` refuses operands that would not be exact.  tests/test_gpu_x3_exact.py puts the
same operands through the kernels."""
import numpy as np
import pytest

from tests import _x3_probe as xp

CATCHES = {(3, 1): {(3, 1), (2, 1), (1, 1)}, (1, 3): {(1, 3), (1, 2), (1, 1)}, (2, 2): {(2, 2), (2, 1), (1, 2), (1, 1)}}
SIX = tuple((i + 1, j + 1) for i, j in xp.PRODUCTS)


def _pair(cls, M=40, K=68, N=70, sparse="b", launch=0, **kw):
    return xp.make_pair(cls, M, K, N, sparse, launch, seed=11, **kw)


def test_split_is_exact_and_plane_counts_are_as_stated():
    rng = np.random.default_rng(0)
    x = rng.standard_normal(20000).astype(np.float32)
    p1, p2, p3 = xp.split3(x)
    assert np.array_equal(p1.astype(np.float64) + p2.astype(np.float64) + p3.astype(np.float64), x.astype(np.float64))
    for p in (p1, p2, p3):
        assert not (p.view(np.uint32) & 0xFFFF).any()                       # bf16 values
    assert np.array_equal(xp.bf16(np.array([1.00390625, 1.01171875], np.float32)), np.array([1.0, 1.015625], np.float32))   # ties to even
    # plain draws: every 11-bit value (top and bottom bit set) has two planes, ~75 % of the 19-bit ones three, none more
    v11 = ((1 << 10) | (np.arange(1 << 9) << 1) | 1).astype(np.float32)
    assert set(np.unique(xp.planes(v11))) == {2}
    v19 = ((1 << 18) | (np.arange(1 << 17) << 1) | 1).astype(np.float32)
    c = xp.planes(v19)
    assert int(c.max()) == 3 and 0.70 < float((c == 3).mean()) < 0.80
    v17 = ((1 << 16) | (np.arange(1 << 15) << 1) | 1).astype(np.float32)
    assert int(xp.planes(v17).max()) == 2                                   # why a class-3 operand takes 18 bits or more
    for p, bits in ((1, 1), (1, 3), (1, 8), (2, 9), (2, 11), (2, 16), (3, 18), (3, 19)):
        d = xp.draw(rng, (300,), p, bits)
        assert set(np.unique(xp.planes(d.astype(np.float32)))) == {p}
        assert np.all(np.abs(d) < (1 << bits)) and np.all(np.abs(d) >= (1 << (bits - 1))) and np.all(d % 2 == 1)
        assert 0 < int((d < 0).sum()) < d.size


@pytest.mark.parametrize("cls", xp.CLASSES)
@pytest.mark.parametrize("sparse", ["a", "b"])
def test_full_recipe_is_exact_on_each_class(cls, sparse):
    a, b, room = _pair(cls, sparse=sparse)
    rng = np.random.default_rng(1)
    bias = xp.addend(rng, (b.shape[1],), room // 2)
    init = xp.addend(rng, (a.shape[0], b.shape[1]), room // 2)
    ref = xp.check(a, b, bias=bias, init=init, cls=cls)
    assert np.array_equal(ref, xp.ref_product(a, b))
    got = xp.six_products(a.astype(np.float32), b.astype(np.float32))
    assert np.array_equal(got, xp.as_f32(ref))
    nzs = (b != 0).sum(axis=0) if sparse == "b" else (a != 0).sum(axis=1)
    assert len(set(nzs.tolist())) == 1 and int(nzs[0]) == xp.choose_nz(cls, 68, 70 if sparse == "b" else 40)


@pytest.mark.parametrize("drop", SIX)
def test_each_dropped_product_changes_some_class(drop):
    caught = set()
    for cls in xp.CLASSES:
        a, b, _ = _pair(cls)
        ref = xp.as_f32(xp.check(a, b, cls=cls))
        got = xp.six_products(a.astype(np.float32), b.astype(np.float32), drop=(drop,))
        if not np.array_equal(got, ref):
            caught.add(cls)
    assert caught == {cls for cls in xp.CLASSES if drop in CATCHES[cls]}


@pytest.mark.parametrize("operand", ["a", "b"])
@pytest.mark.parametrize("plane", [2, 3])
def test_plane_lost_only_beyond_a_k_tail_is_caught(operand, plane):
    """Planes 2 / 3 of one operand zero on the last 4 of K = 68 only (a stale or missing fragment in a tail step): over
    the probe set of some class the integer result changes, in every group of outputs."""
    K, tail = 68, 4
    hit = False
    for cls in xp.CLASSES:
        nz, launches = xp.probe_plan(cls, K, 70)
        for launch in range(launches):
            a, b, _ = _pair(cls, K=K, launch=launch)
            ref = xp.as_f32(xp.check(a, b, cls=cls))
            pa, pb = list(xp.split3(a.astype(np.float32))), list(xp.split3(b.astype(np.float32)))
            if operand == "a":
                pa[plane - 1] = pa[plane - 1].copy()
                pa[plane - 1][:, K - tail:] = 0
            else:
                pb[plane - 1] = pb[plane - 1].copy()
                pb[plane - 1][K - tail:, :] = 0
            got = xp.six_products(None, None, pa=pa, pb=pb)
            wrong = (got != ref).any(axis=0)                                # per output column
            if wrong.any():
                hit = True
                groups = [wrong[g:g + xp.TILE].any() for g in range(0, 64, xp.TILE)]
                assert all(groups)                                          # (launch 0 holds the tail: priority indices)
    assert hit


@pytest.mark.parametrize("K,n_out", [(67, 33), (35, 130), (16, 64), (257, 33), (520, 70), (16, 32), (68, 96), (132, 256),
                                     (129, 67), (4112, 256), (4100, 96), (2064, 96), (1000, 128), (4099, 130), (1280, 1024),
                                     (2048, 40), (2048, 20), (256, 128), (5, 2048), (7, 2048)])
@pytest.mark.parametrize("cls", xp.CLASSES)
def test_placement_reaches_every_reduction_index(cls, K, n_out):
    """Within eight launches every full group of 32 outputs reaches every reduction index, a ragged last group the
    priority indices; the non-zeros of one output are distinct."""
    nz, launches = xp.probe_plan(cls, K, n_out)
    assert launches <= xp.MAX_LAUNCHES
    xp.widths(cls, nz)
    pos = xp.sparse_positions(K, n_out, nz, 0)
    assert all(len(set(r)) == nz for r in pos.tolist())
    hit = xp.covered(K, n_out, nz, launches)
    t = min(xp.TILE, n_out)
    assert hit[: n_out // t].all()
    assert hit[:, xp.priority_indices(K)].all()


@pytest.mark.parametrize("cls", [(3, 1), (1, 3)])
def test_narrow_output_long_reduction_coverage_is_partial_and_known(cls):
    """The one listed shape where the budget does not reach: a weight gradient with 7 (or 20) outputs over 2048 rows.  Class
    (2,2) takes nz = 64 and covers it; classes (3,1) / (1,3) stop at nz = 32 (18 + 1 + 5 bits), i.e. 7 * 32 * 8 = 1792 rows,
    priority indices included."""
    nz, launches = xp.probe_plan(cls, 2048, 7)
    assert (nz, launches) == (32, 8)
    hit = xp.covered(2048, 7, nz, launches)
    assert int(hit.sum()) == 1792 and hit[:, xp.priority_indices(2048)].all()
    assert xp.covered(2048, 7, *xp.probe_plan((2, 2), 2048, 7)).all()


def test_check_rejects_what_would_not_be_exact():
    a, b, room = _pair((3, 1))
    xp.check(a, b, cls=(3, 1))
    bad = a.copy()
    bad[0, 0] += 0.5
    with pytest.raises(AssertionError, match="c1"):
        xp.check(bad, b)
    with pytest.raises(AssertionError, match="c1"):
        xp.check(a, b, scale_a=np.full(a.shape[0], 3.0))
    a2, b2, _ = _pair((2, 2))
    with pytest.raises(AssertionError, match="c2"):
        xp.check(a, b2)                                                     # class 3 meets class 2
    with pytest.raises(AssertionError, match="c3"):
        xp.check(a, b, bias=np.full(b.shape[1], float(room + (1 << 22))))
    with pytest.raises(AssertionError, match="c3"):
        xp.check(a, b * 4)                                                  # same planes, four times the sum
    with pytest.raises(AssertionError, match="c4"):
        xp.check(a, b, cls=(2, 1))
    # a scale constant along the reduction axis is accepted, and the reference stays the integers'
    sa, sb = xp.pow2_scales(np.random.default_rng(2), a.shape[0]), xp.pow2_scales(np.random.default_rng(3), b.shape[1])
    ref = xp.check(a * sa[:, None], b * sb[None, :], cls=(3, 1), scale_a=sa, scale_b=sb)
    assert np.array_equal(ref, xp.ref_product(a, b))
    got = xp.six_products((a * sa[:, None]).astype(np.float32), (b * sb[None, :]).astype(np.float32))
    assert np.array_equal(got, xp.as_f32(ref, sa, sb))


def test_references_of_the_operations():
    y = np.array([[3, -4], [-1, 2], [5, -6], [0, 1]], dtype=np.int64)
    assert np.array_equal(xp.ref_relu(xp.ref_bias(y, np.array([1.0, -1.0]))), [[4, 0], [0, 1], [6, 0], [1, 0]])
    assert np.array_equal(xp.ref_max_rows(y, 2), [[3, 2], [5, 1]])
    assert np.array_equal(xp.ref_max_points(y.reshape(2, 2, 2)), [[3, 2], [5, 1]])
    assert np.array_equal(xp.ref_colsum(y), [7, -7])
    assert np.array_equal(xp.ref_gate(y, np.array([[1, 0], [0, 2], [0, 0], [3, 3]])), [[3, 0], [0, 2], [0, 0], [0, 1]])


def test_why_the_probes_exist_three_products_pass_the_relative_bound():
    """On unit-scale randn operands at (512, 64, 128), max|diff| / max|ref| of a kernel that computes only (1,1) (1,2) (2,1)
    is below the 1e-5 of the dense tests: the tolerance tests cannot see half of the recipe missing."""
    rng = np.random.default_rng(5)
    a = rng.standard_normal((512, 64)).astype(np.float32)
    b = (rng.standard_normal((64, 128)) / 8).astype(np.float32)
    ref = a.astype(np.float64) @ b.astype(np.float64)
    rel = lambda got: float(np.abs(got.astype(np.float64) - ref).max() / np.abs(ref).max())
    half = rel(xp.six_products(a, b, drop=((1, 3), (2, 2), (3, 1))))
    full = rel(xp.six_products(a, b))
    assert half < 1e-5
    assert full < half
