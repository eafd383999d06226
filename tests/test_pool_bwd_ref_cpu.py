"""tests/_pool_bwd_ref.py on its own, before it judges a kernel (tests/test_gpu_pool_bwd_exact.py): the truth equals torch's
float64 autograd of the dense formulation and a loop statement of the contract (values, sums of |term|, term counts); every
case of the table keeps the exactness condition, with its margin printed (run with -s); the restated launch rules say that the
table still reaches the paths it was chosen for; and a truth with one hit dropped, one gate flipped at zero or one row counted
twice is told from the right one by the exact comparison."""
import functools

import numpy as np
import pytest
import torch

from tests import _pool_bwd_ref as ref


@functools.lru_cache(maxsize=None)
def _inputs(name):
    return ref.exact_inputs(ref.CASES[name])


@functools.lru_cache(maxsize=None)
def _paths(name):
    return ref.paths(ref.CASES[name], _inputs(name))


def _name(fn, shape):
    return fn + "-" + "x".join(map(str, shape))


# --------------------------------------------------------------------------- the truth against autograd and against loops

def _tiny(seed, B, N, S, C1, C2):
    g = torch.Generator().manual_seed(seed)
    G = B * S
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    t = dict(feat=r(B * N, C1), W1x=r(C1, 3), b1=r(C1), W2=r(C2, C1), b2=r(C2), xyz=r(B, N, 3), new_xyz=r(B, S, 3),
             dout=r(G, C2), out=r(G, C2) + 0.1,
             argmax=torch.randint(0, 32, (G, C2), generator=g), idx=torch.randint(0, N, (B, S, 32), generator=g))
    t["idx"][0, 0, :] = t["idx"][0, 0, 0]            # a group of one point
    t["argmax"][1, :] = 4                            # every channel of a group on one row
    t["out"][2, :] = -1.0                            # a dead group
    return t


@pytest.mark.parametrize("B,N,S,C1,C2", [(2, 5, 3, 8, 6), (1, 3, 6, 4, 8), (3, 40, 2, 8, 8)])
def test_truth_equals_autograd_of_the_dense_form(B, N, S, C1, C2):
    """Dense form: dy[G*32, C2] holds dout at (arg-max row, channel) of every live channel; L = sum(dy * (h W2^T + b2)) with
    h = relu(feat[j] + W1x (xyz[j] - new_xyz[g]) + b1) = relu(Pp[j] + Q[g]).  Autograd's gradients of L by W2, b2, feat, W1x
    and b1 are dW2, db2, dP, dW1[:, 0:3] and db1."""
    t = _tiny(100 * B + S, B, N, S, C1, C2)
    G, R = B * S, B * S * 32
    leaves = {k: t[k].clone().requires_grad_(True) for k in ("feat", "W1x", "b1", "W2", "b2")}
    point = (torch.arange(B)[:, None, None] * N + t["idx"]).reshape(R)
    rel = t["xyz"].reshape(-1, 3)[point] - t["new_xyz"].reshape(G, 3).repeat_interleave(32, dim=0)
    h = torch.relu(leaves["feat"][point] + rel @ leaves["W1x"].T + leaves["b1"])
    dy = torch.zeros(G, 32, C2, dtype=torch.float64)
    dy.scatter_(1, t["argmax"].reshape(G, 1, C2), torch.where(t["out"] > 0, t["dout"], torch.zeros_like(t["dout"])).reshape(G, 1, C2))
    (dy.reshape(R, C2) * (h @ leaves["W2"].T + leaves["b2"])).sum().backward()
    with torch.no_grad():
        Pp = t["feat"] + t["xyz"].reshape(-1, 3) @ t["W1x"].T
        Q = t["b1"] - t["new_xyz"].reshape(G, 3) @ t["W1x"].T
    got = ref.reference(t["dout"], t["argmax"], t["out"], t["W2"], Pp, Q, t["idx"], t["xyz"], t["new_xyz"])
    for name, leaf in (("dW2", "W2"), ("db2", "b2"), ("dP", "feat"), ("dW1", "W1x"), ("db1", "b1")):
        want = leaves[leaf].grad
        assert got[name].value.shape == want.shape, name
        assert float(want.abs().max()) > 0, name
        torch.testing.assert_close(got[name].value, want, rtol=1e-12, atol=1e-12, msg=name)


@pytest.mark.parametrize("B,N,S,C1,C2", [(2, 5, 3, 8, 6), (1, 3, 6, 4, 8)])
def test_truth_equals_the_contract_written_as_loops(B, N, S, C1, C2):
    """Values, sums of |term| and term counts of all five outputs, hit by hit."""
    t = _tiny(7 + N, B, N, S, C1, C2)
    G = B * S
    Pp, Q = t["feat"], t["b1"].expand(G, C1) + t["new_xyz"].reshape(G, 3) @ t["W1x"].T
    got = ref.reference(t["dout"], t["argmax"], t["out"], t["W2"], Pp, Q, t["idx"], t["xyz"], t["new_xyz"])
    shapes = {"dW2": (C2, C1), "db2": (C2,), "dP": (B * N, C1), "dW1": (C1, 3), "db1": (C1,)}
    val = {k: np.zeros(s) for k, s in shapes.items()}
    ab = {k: np.zeros(s) for k, s in shapes.items()}
    cnt = {k: np.zeros(s) for k, s in shapes.items()}

    def add(name, where, term):
        val[name][where] += term
        ab[name][where] += np.abs(term)
        cnt[name][where] += 1

    n = {k: v.numpy() for k, v in t.items()}
    Ppn, Qn = Pp.numpy(), Q.numpy()
    for g in range(G):
        b = g // S
        for c in range(C2):
            if not n["out"][g, c] > 0 or n["dout"][g, c] == 0:
                continue
            gv, k = n["dout"][g, c], n["argmax"][g, c]
            j = b * N + n["idx"][b, g % S, k]
            pre = Ppn[j] + Qn[g]
            add("db2", c, gv)
            add("dW2", c, gv * np.maximum(pre, 0.0))
            d = n["xyz"].reshape(-1, 3)[j] - n["new_xyz"].reshape(G, 3)[g]
            for col in range(C1):
                if pre[col] > 0:
                    term = gv * n["W2"][c, col]
                    add("dP", (j, col), term)
                    add("db1", col, term)
                    add("dW1", col, term * d)
    for name in ref.OUTPUTS:
        np.testing.assert_allclose(got[name].value.numpy(), val[name], rtol=1e-12, atol=1e-12, err_msg=name)
        np.testing.assert_allclose(got[name].abs.numpy(), ab[name], rtol=1e-12, atol=1e-12, err_msg=name + " abs")
        assert np.array_equal(got[name].count.numpy(), cnt[name]), name + " count"


def test_inverse_lists_by_hand():
    idx = np.zeros((1, 1, 32), dtype=np.int64)
    idx[0, 0, :4] = [2, 0, 2, 1]
    off, rows, pts = ref.inverse_lists(idx, 3)
    assert off.tolist() == [[0, 29, 30, 32]]
    assert rows[0, :29].tolist() == [1] + list(range(4, 32)) and rows[0, 29:].tolist() == [3, 0, 2]
    assert pts[0, 28:].tolist() == [0, 1, 2, 2]


# --------------------------------------------------------------------------- the condition, case by case

@pytest.mark.parametrize("name", list(ref.CASES))
def test_exactness_condition_holds(name):
    """From the truth alone: inputs on their grids, and the largest sum of |term| + |prefill| of every output, in grid units,
    below 2^24 - then the float64 truth is an fp32 array and any fp32 summation order reproduces it."""
    case = ref.CASES[name]
    assert case.why
    t = _inputs(name)
    assert ref.on_grids(t)
    truth = ref.truth_of(t)
    margin = ref.exact_margin(truth, ref.prefill(case.shape, 5))
    worst = max(margin, key=margin.get)
    print(f"{name}: largest sum|term| {margin[worst]:.3g} grid units ({worst}), 2^24 / that = {ref.LIMIT / margin[worst]:.1f}")
    for out, m in margin.items():
        assert m < ref.LIMIT, (out, m)
        v = truth[out].value
        assert torch.equal(v.float().double(), v), out
        assert torch.equal(v / ref.UNITS[out], torch.round(v / ref.UNITS[out])), out
        assert float(v.abs().max()) > 0, out
    assert _paths(name)["zero_gates"] > 0                 # Pp + Q == 0 occurs on its own


def test_margin_of_the_two_largest_cases():
    """The issue's figures: ~3e5 grid units on dW1 at the two largest shapes, a factor ~50 under 2^24 = 1.68e7."""
    for name in (_name("xcd_three_batches", (5, 96, 500, 128, 128)), _name("two_slices_cpw16", (5, 64, 288, 256, 256))):
        m = ref.exact_margin(ref.truth_of(_inputs(name)))
        print(name, {k: f"{v:.3g}" for k, v in m.items()})
        assert max(m, key=m.get) == "dW1"
        assert 30 * max(m.values()) < ref.LIMIT


# --------------------------------------------------------------------------- the paths the table was chosen for

def test_walk_restatement_small():
    w = ref.wgrad_walk(20, 128)                     # 20 workgroups: plain
    assert not w["xcd"] and w["groups"][3] == [3]
    w = ref.wgrad_walk(33, 256)                     # 33 workgroups: plain, one group each
    assert w["gx"] == 33 and w["ny"] == 2 and not w["xcd"]
    w = ref.wgrad_walk(1000, 256)                   # 128 workgroups, XCD eighths of 125, stride 16
    assert w["xcd"] and w["groups"][0] == list(range(0, 125, 16)) and w["groups"][9] == list(range(126, 250, 16))
    assert [ref.point_chunk(*a) for a in ((2048, 512), (2048, 256), (1024, 8), (40, 90))] == [8, 16, 32, 1]


def test_table_reaches_its_paths():
    p = {name: _paths(name) for name in ref.CASES}
    A, Bs = ref.PLANT_A, ref.PLANT_B

    q = p[_name("xcd_three_batches", (5, 96, 500, 128, 128))]
    assert q["xcd"] and q["gx"] == 256 and (q["min_groups"], q["max_groups"]) == (9, 10)
    assert q["batches"] == 3 and q["ragged"] and q["uneven"] and q["cpw"] == 8
    q = p[_name("two_slices_cpw16", (5, 64, 288, 256, 256))]
    assert q["xcd"] and (q["ny"], q["gx"]) == (2, 128) and (q["min_groups"], q["max_groups"]) == (11, 12)
    assert q["batches"] == 3 and q["ragged"] and q["cpw"] == 16
    q = p[_name("plain_walk_c1_384", (2, 64, 384, 384, 128))]
    assert not q["xcd"] and (q["ny"], q["gx"]) == (3, 85) and (q["min_groups"], q["max_groups"]) == (9, 10) and q["ragged"]
    q = p[_name("small_clouds_c2_64", (40, 64, 8, 128, 64))]
    assert q["xcd"] and q["cloud_steps"] == 4 and q["cpw"] == 4 and q["max_groups"] == 2
    q = p[_name("empty_workgroups", (1, 64, 260, 128, 64))]
    assert q["xcd"] and q["empty_workgroups"] == 3 and q["max_groups"] == 2
    q = p[_name("few_groups", (1, 64, 5, 128, 256))]
    assert not q["xcd"] and q["gx"] == 5
    q = p[_name("few_groups", (1, 64, 8, 256, 64))]
    assert q["xcd"] and (q["ny"], q["gx"]) == (2, 8)
    q = p[_name("sparse_chunks", (3, 1024, 8, 128, 128))]
    assert q["pc"] == 32 and q["pc_unclamped"] > 32 and 2 * q["empty_chunks"] > q["chunks"]
    q = p[_name("one_point_chunks", (2, 40, 90, 128, 128))]
    assert q["pc"] == 1 and q["pc_unclamped"] < 1 and q["max_list"] > 64

    for shape in (A, Bs):
        S, C2 = shape[2], shape[4]
        assert p[_name("rows_of_many_hits", shape)]["max_row_hits"] == C2 > 64
        assert p[_name("dead_groups", shape)]["dead_groups"] >= 8
        q = p[_name("zero_dout", shape)]
        assert q["zero_dout_live"] > 0 and q["dead_groups"] >= 2
        assert p[_name("hub_point", shape)]["max_list"] >= S > 64
        q = p[_name("duplicate_neighbours", shape)]
        assert q["one_point_groups"] >= 10 and q["duplicates"] >= 16 * 10
        q = p[_name("ungathered_points", shape)]
        assert q["first_last_unused"] and q["empty_chunks"] >= 3 * shape[0]
    assert p[_name("hub_point", Bs)]["max_list"] > 128          # three trips
    # the properties the table as a whole must keep
    assert any(q["batches"] >= 3 and q["xcd"] for q in p.values()) and any(q["batches"] >= 3 and not q["xcd"] for q in p.values())
    assert any(q["empty_workgroups"] for q in p.values()) and any(q["ragged"] for q in p.values())
    assert {q["cpw"] for q in p.values()} == {4, 8, 16}


# --------------------------------------------------------------------------- the probes are sharp

def _differs(a, b):
    return {name for name in ref.OUTPUTS if not torch.equal(a[name].value.float(), b[name].value.float())}


@pytest.mark.parametrize("name", [_name("hub_point", ref.PLANT_A), _name("small_clouds_c2_64", (40, 64, 8, 128, 64))])
def test_mutated_truth_fails_the_exact_comparison(name):
    """The comparison the device test makes (fp32 equality of every output) between the truth and a truth with one mistake:
    one hit dropped changes db2 by that gradient; a gate that lets an exact zero through changes dP but not dW2 (the row's
    value is 0 either way); one row added twice changes dP."""
    t = _inputs(name)
    args = [t[k] for k in ref.ARGS]
    truth = ref.truth_of(t)
    assert _differs(truth, ref.truth_of(t)) == set()
    d = _differs(truth, ref.mutated("drop_hit", *args))
    assert {"db2", "dW2", "dP"} <= d, d
    d = _differs(truth, ref.mutated("gate_at_zero", *args))
    assert "dP" in d and "db1" in d and not ({"dW2", "db2"} & d), d
    d = _differs(truth, ref.mutated("double_row", *args))
    assert "dP" in d and not ({"dW2", "db2"} & d), d
