"""tests/_chamfer_ref.py on its own, before it judges a kernel (tests/test_gpu_chamfer.py): the C oracle's chamfer
(oracle/pzn_oracle.c, the same expansion form in float32 without fma) must pass the very assertions the device is held to, on
every input kind; the float32 formulas written out in NumPy stay inside the derived bound; grad() is torch's float64 autograd;
the planted ties are ties in float64 at every shape the GPU test uses.  Run with -s for the figures."""
import fractions

import numpy as np
import pytest
import torch

from oracle import point_ops as orc
from tests import _chamfer_ref as ref

# (B, n, m): one pair; fewer rows than a wavefront; a row block edge; unequal sizes; square; a walked cloud of two tiles
SHAPES = [(1, 1, 1), (3, 1, 7), (2, 3, 130), (2, 65, 64), (2, 300, 77), (1, 300, 300), (1, 70, 600)]
KINDS = {
    "uniform": lambda s, B, n, m: ref.uniform(s, B, n, m),
    "offset10": lambda s, B, n, m: ref.offset(s, B, n, m),
    "scale1e-3": lambda s, B, n, m: ref.scaled(s, B, n, m, 1e-3),
    "scale100": lambda s, B, n, m: ref.scaled(s, B, n, m, 100.0),
    "ties": lambda s, B, n, m: ref.with_ties(s, B, n, m),
    "funnel": lambda s, B, n, m: ref.funnel(s, B, n, m),
}


def _seed(B, n, m):
    return 7000 + 131 * B + 17 * n + m


def _round32_exact(s):
    """Round a Fraction to the nearest float32, ties to even, by comparing the candidates exactly."""
    f = np.float32(float(s))
    cands = {float(f), float(np.nextafter(f, np.float32(np.inf))), float(np.nextafter(f, np.float32(-np.inf)))}
    best = min(cands, key=lambda c: (abs(fractions.Fraction(c) - s), int(np.float32(c).view(np.uint32)) & 1))
    return np.float32(best)


def test_fma32_rounds_once():
    rng = np.random.default_rng(3)
    a = rng.standard_normal(1500).astype(np.float32) * np.float32(3.0)
    b = rng.standard_normal(1500).astype(np.float32)
    c = (rng.standard_normal(1500) * 10.0 ** rng.integers(-6, 2, 1500)).astype(np.float32)
    # products that land exactly half way between two float32 values, pushed off the tie by an addend far below float64's
    # resolution of the product: rounding the float64 sum would go to even, the single rounding follows the addend
    t = np.float32(1.0) + np.float32(2.0 ** -12)
    a = np.concatenate((a, [t, t, t, -t]))
    b = np.concatenate((b, [t, t, t, t]))
    c = np.concatenate((c, np.array([2.0 ** -60, -2.0 ** -60, 0.0, 2.0 ** -60], dtype=np.float32)))
    got = ref.fma32(a, b, c)
    want = np.array([_round32_exact(fractions.Fraction(float(x)) * fractions.Fraction(float(y)) + fractions.Fraction(float(z)))
                     for x, y, z in zip(a, b, c)], dtype=np.float32)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert got[-4] > got[-3] == got[-2]     # the addend decides; without one the tie goes to even


@pytest.mark.parametrize("kind", list(KINDS))
def test_oracle_and_formulas_pass_the_device_assertions(kind):
    """(a) and (b) of tests/test_gpu_chamfer.py on the oracle's results, and |P32 - D| <= Bd for both float32 formulas."""
    worst_formula = 0.0
    for B, n, m in SHAPES:
        c = KINDS[kind](_seed(B, n, m), B, n, m)
        D, Bd = ref.truth(c.a, c.b), ref.distance_bound(c.a, c.b)
        moa, aoa, mob, aob = orc.chamfer(c.a, c.b)
        wa = ref.check_minima(D, Bd, moa, mob)
        wb, flips = ref.check_argmins(D, Bd, aoa, aob)
        for P in (ref.plain_matrix(c.a, c.b), ref.kernel_matrix(c.a, c.b)):
            r = float((np.abs(P.astype(np.float64) - D) / Bd).max())
            assert r <= 1.0, (kind, B, n, m, r)
            worst_formula = max(worst_formula, r)
        # the oracle IS plain_matrix: same minima bit for bit, first index of the minimum
        P = ref.plain_matrix(c.a, c.b)
        assert np.array_equal(moa, P.min(axis=1)) and np.array_equal(mob, P.min(axis=2))
        assert np.array_equal(aoa, P.argmin(axis=1)) and np.array_equal(aob, P.argmin(axis=2))
        print(f"{kind} {B}x{n}x{m}: oracle (min - truth) / bound {wa:+.3f}, arg-min excess / bound {wb:.3f}, flips {flips}")
    print(f"{kind}: largest |P32 - D| / Bd over both formulas {worst_formula:.3f}")


@pytest.mark.parametrize("shape", SHAPES[2:], ids=lambda s: "x".join(map(str, s)))
def test_oracle_returns_the_lowest_index_of_a_tie(shape):
    """(d) on the oracle: bit-equal float32 minima exist by construction, and the index is the lowest of them."""
    c = ref.with_ties(_seed(*shape), *shape)
    assert c.planted
    ref.planted_are_float64_ties(c, ref.truth(c.a, c.b), ref.distance_bound(c.a, c.b))
    moa, aoa, mob, aob = orc.chamfer(c.a, c.b)
    ref.check_first_copy(c.a, c.b, aoa, aob)
    assert ref.check_planted(c, aoa, aob) == len(c.planted)
    P = ref.plain_matrix(c.a, c.b)
    ties = 0
    for direction, bb, row, want in c.planted:
        col = P[bb, :, row] if direction == "over_a" else P[bb, row, :]
        at_min = np.flatnonzero(col == col.min())
        assert at_min[0] == want
        ties += int(len(at_min) > 1)
    assert ties == len(c.planted)           # every planted query is an exact float32 tie


def test_planted_ties_hold_at_the_device_shapes():
    """The builder's claims in float64 at every shape the GPU test runs it at, and where the copies fall in the kernel's walk:
    one placement inside a quarter, one across quarters, one across tiles wherever the cloud has them."""
    for shape in ref.TIE_SHAPES:
        c = ref.with_ties(ref.seed_of("ties", shape), *shape)
        assert c.planted, shape
        ref.planted_are_float64_ties(c, ref.truth(c.a, c.b), ref.distance_bound(c.a, c.b))
        for direction, x, y in (("over_a", c.a, c.b), ("over_b", c.b, c.a)):
            k = x.shape[1]
            q = ref.quarters(k)
            where = lambda i: (i // ref.TILE, next(w for w in range(4) if q[i // ref.TILE][w][0] <= i < q[i // ref.TILE][w][1]))
            fc = ref.first_copy(x)[0]
            kinds = set()
            for first in {w for d, bb, r, w in c.planted if d == direction and bb == 0}:
                spots = [where(i) for i in np.flatnonzero(fc == first)]
                assert len(spots) >= 2, (shape, direction, first)
                kinds.add("tiles" if len({t for t, _ in spots}) > 1 else "quarters" if len(set(spots)) > 1 else "inside")
            if k >= 16:
                assert {"inside", "quarters"} <= kinds, (shape, direction, kinds)
            if k > ref.TILE and y.shape[1] >= 16:      # (a cloud of 3 rows has no room for the third placement's query)
                assert "tiles" in kinds, (shape, direction, kinds)
    B, n, m = ref.FUNNEL_SHAPE
    c = ref.funnel(ref.seed_of("funnel", ref.FUNNEL_SHAPE), B, n, m)
    ref.planted_are_float64_ties(c, ref.truth(c.a, c.b), ref.distance_bound(c.a, c.b))


@pytest.mark.parametrize("weights", ["both", "first", "second"])
def test_grad_is_float64_autograd(weights):
    for B, n, m in [(1, 1, 1), (3, 1, 7), (2, 65, 64), (2, 300, 77)]:
        c = ref.uniform(_seed(B, n, m), B, n, m)
        rng = np.random.default_rng(5)
        g1 = rng.standard_normal((B, m)).astype(np.float32) if weights != "second" else None
        g2 = rng.standard_normal((B, n)).astype(np.float32) if weights != "first" else None
        D = ref.truth(c.a, c.b)
        ga, gb, ga_abs, gb_abs, ka, kb = ref.grad(c.a, c.b, D.argmin(axis=1), D.argmin(axis=2), g1, g2)
        ta = torch.from_numpy(c.a).double().requires_grad_(True)
        tb = torch.from_numpy(c.b).double().requires_grad_(True)
        P = ((ta[:, :, None, :] - tb[:, None, :, :]) ** 2).sum(-1)
        loss = 0.0
        if g1 is not None:
            loss = loss + (P.min(dim=1)[0] * torch.from_numpy(g1).double()).sum()
        if g2 is not None:
            loss = loss + (P.min(dim=2)[0] * torch.from_numpy(g2).double()).sum()
        loss.backward()
        for got, want in ((ga, ta.grad.numpy()), (gb, tb.grad.numpy())):
            assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
        terms = (0 if g1 is None else B * m) + (0 if g2 is None else B * n)
        assert ka.sum() == terms and kb.sum() == terms
        assert (ga_abs >= np.abs(ga) * (1 - 1e-12)).all() and (gb_abs >= np.abs(gb) * (1 - 1e-12)).all()
        assert ((ka == 0)[..., None] <= (ga_abs == 0)).all()


def test_distance_bound_scaling():
    """What the expansion form costs a caller.  Scaling the clouds by s scales the bound by s^2; moving the unit cube by +10
    multiplies every coordinate square by 100 to 121 and more (a coordinate near 0 becomes 10), so the LARGEST bound grows by
    about 100 to 150 while the MEAN grows by about 378: the mean of |a|^2 + |b|^2 + 2 sum |a_c b_c| over the unit cube is
    1 + 1 + 2 * 3/4 = 3.5, over [10, 11)^3 it is 4 * 3 * 10.5^2 + 2 * 3 / 12 = 1323.5."""
    B, n, m = 1, 300, 300
    u = ref.uniform(11, B, n, m)
    o = ref.offset(11, B, n, m)
    bu, bo = ref.distance_bound(u.a, u.b), ref.distance_bound(o.a, o.b)
    g5 = float(ref.gamma(5))
    print(f"unit cube: mean bound {bu.mean():.3e}, largest {bu.max():.3e}; +10: mean {bo.mean():.3e}, largest {bo.max():.3e}; "
          f"ratios {bo.mean() / bu.mean():.1f} and {bo.max() / bu.max():.1f}")
    assert abs(bu.mean() / g5 / 3.5 - 1) < 0.05 and abs(bo.mean() / g5 / 1323.5 - 1) < 0.01
    assert bu.max() <= 12 * g5 and 1200 * g5 <= bo.max() <= 1452 * g5
    for s in (2.0 ** -10, 128.0):      # powers of two: the scaled inputs are exact, and so is the factor
        c = ref.scaled(11, B, n, m, s)
        assert np.allclose(ref.distance_bound(c.a, c.b), s * s * bu, rtol=1e-14, atol=0)
    for s in (1e-3, 100.0):            # the scaled float32 inputs are rounded: 2^-24 per coordinate, squared terms
        c = ref.scaled(11, B, n, m, s)
        assert np.allclose(ref.distance_bound(c.a, c.b), s * s * bu, rtol=4 * ref.U32, atol=0)
    # relative to the nearest-neighbour distances the minima are about
    Du = ref.truth(u.a, u.b)
    i = np.arange(n)
    j = Du[0].argmin(axis=1)
    print(f"nearest-neighbour distance, median {np.median(Du[0, i, j]):.3e}: bound / distance at the median pair "
          f"{np.median(bu[0, i, j] / Du[0, i, j]):.2e} (unit cube), {np.median(bo[0, i, j] / Du[0, i, j]):.2e} (+10)")
