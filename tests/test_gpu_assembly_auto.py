"""GPU: keep="auto" through the assembly functions - match_puzzles / match_pairs / pair_block / refine_pairs, the walks on such a
table, and the joint refinements' refusal of it - with the closed-form model of tests/test_gpu_assembly.py.  The kernel itself
is held to integers and to float64 in tests/test_gpu_icp_auto.py; here every auto field is compared, torch.equal, with a
direct ops.icp_refine(..., auto=...) on sets gathered by hand from the table's OWN picks and poses, where nothing is noisy.

Two calls of match_puzzles need not agree bit for bit in the fields behind the few-row layers (tests/test_gpu_assembly_batch.py);
a field is therefore compared with today's call by torch.equal where two of today's calls are torch.equal, and by the atomic
rule of tests/test_gpu_assembly_refine.py where they are not (tests/test_gpu_assembly_trim.py's way)."""
import pytest
import torch

from oracle import model_ref as mr

pytestmark = pytest.mark.gpu

Z, P, N, TOP = 2, 3, 1024, 128
REFINE = 4
LO = 32                 # ceil(0.25 * TOP): AutoKeep's default least
POWER = 3
ATOMIC_REL = 5e-6       # tests/test_gpu_assembly_refine.py's
AUTO_CALL = "pzn_icp_refine_auto_f32"


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def model(dev):
    from puzzlenet_amd import model5_b as mb
    m = mb.TouchedRegraster(mr.Cfg())
    mr.fill_params(m)
    m.to(dev)
    return m


@pytest.fixture(scope="module")
def tables(dev, model):
    from puzzlenet_amd import assembly, ops
    g = torch.Generator().manual_seed(1619)
    assert model.num_points == N
    pieces = torch.rand(Z, P, N, 3, generator=g).to(dev)
    start = (torch.randint(0, N, (Z, P), generator=g), torch.randint(0, 512, (Z, P), generator=g))
    trace = {}

    def traced(key, **kw):
        real, calls = ops._call, []

        def spy(name, *a, **k):
            calls.append(name)
            return real(name, *a, **k)
        ops._call = spy
        try:
            out = assembly.match_puzzles(model, pieces, k=TOP, start=start, **kw)
        finally:
            ops._call = real
        trace[key] = calls
        return out
    return dict(pieces=pieces, start=start, trace=trace, plain=traced("plain", keep=1.0), plain2=traced("plain2"),
                fine=traced("fine", refine=REFINE), fine2=traced("fine2", refine=REFINE),
                auto=traced("auto", refine=REFINE, keep="auto"), auto0=traced("auto0", refine=0, keep=assembly.AutoKeep()))


def _rel(a, b):
    a, b = a.double(), b.double()
    fin = torch.isfinite(b)
    assert torch.equal(fin, torch.isfinite(a))
    return float((a[fin] - b[fin]).abs().max() / b[fin].abs().max().clamp_min(1e-30))


def _same_as_far_as_reproducible(a, a2, b, names):
    for name in names:
        x, x2, y = getattr(a, name), getattr(a2, name), getattr(b, name)
        if torch.equal(x, x2):
            assert torch.equal(x, y), name
        else:
            assert x.dtype == torch.float32, f"{name}: two of today's calls differ in an index field"
            assert _rel(y, x) <= ATOMIC_REL, name


def _gathered(pieces, top_f, top_m):
    """The picked sets of every ordered pair of one puzzle by plain indexing: Bf [K K,k,3], Bm [K K,k,3]."""
    K = pieces.shape[0]
    Bf = torch.stack([pieces[i][top_f[i, j]] for i in range(K) for j in range(K)])
    Bm = torch.stack([pieces[j][top_m[j]] for i in range(K) for j in range(K)])
    return Bf.contiguous(), Bm.contiguous()


def _masked(score, K):
    return score.view(K, K).masked_fill(torch.eye(K, dtype=torch.bool, device=score.device), float("inf"))


def _is_the_direct_launch(pieces, t, T0, iters):
    """One puzzle's auto table (or block: masked = False) against ops.icp_refine(auto=) on hand-gathered sets from T0."""
    from puzzlenet_amd import ops
    K = pieces.shape[0]
    Bf, Bm = _gathered(pieces, t.top_f, t.top_m)
    T, score, score0, used, count_f, count_m, objective, kept_f, kept_m = ops.icp_refine(
        Bf, Bm, T0.reshape(K * K, 4, 4).contiguous(), iters, auto=(LO, LO, POWER), return_kept=True)
    assert torch.equal(t.T, T.view(K, K, 4, 4)) and torch.equal(t.score, _masked(score, K))
    assert torch.equal(t.kept_f, kept_f.view(K, K, TOP)) and torch.equal(t.kept_m, kept_m.view(K, K, TOP))
    assert torch.equal(t.count_f, count_f.view(K, K)) and torch.equal(t.count_m, count_m.view(K, K))
    assert torch.equal(t.objective, objective.view(K, K))
    return score, score0, used, count_f, count_m


def _puzzle(t, z):
    return type(t)(*(f[z] for f in t))


def test_auto_table_is_the_direct_auto_launch(tables):
    from puzzlenet_amd import assembly, se3
    t, pieces = tables["auto"], tables["pieces"]
    assert type(t) is assembly.AutoPairTable
    assert t._fields == assembly.PairTable._fields + ("kept_f", "kept_m", "count_f", "count_m", "objective")
    assert t.kept_f.shape == (Z, P, P, TOP) and t.kept_m.shape == (Z, P, P, TOP) and t.kept_f.dtype == torch.int32
    assert t.count_f.shape == (Z, P, P) and t.count_f.dtype == torch.int32 and t.objective.shape == (Z, P, P)
    # one auto launch in place of today's untrimmed one, nothing else changes
    calls, today = tables["trace"]["auto"], tables["trace"]["fine"]
    assert calls == [(AUTO_CALL if c == "pzn_icp_refine_f32" else c) for c in today] and calls.count(AUTO_CALL) == 1
    # every field but T, score and the new ones is the keep = 1.0 table's
    others = [n for n in assembly.PairTable._fields if n not in ("T", "score")]
    _same_as_far_as_reproducible(tables["fine"], tables["fine2"], t, others)
    _same_as_far_as_reproducible(tables["plain"], tables["plain2"], t, others)
    moved = 0
    for z in range(Z):
        score, score0, used, count_f, count_m = _is_the_direct_launch(pieces[z], _puzzle(t, z), se3.exp(t.twist[z]), REFINE)
        moved += int(used.sum())
        assert int(count_f.min()) >= LO and int(count_f.max()) <= TOP and int(count_m.min()) >= LO and int(count_m.max()) <= TOP
        # -1 exactly past the count
        live = torch.arange(TOP, device=pieces.device)[None, :] < count_f[:, None]
        assert bool((t.kept_f[z].view(P * P, TOP)[~live] == -1).all()) and bool((t.kept_f[z].view(P * P, TOP)[live] >= 0).all())
    assert moved >= 1 and not torch.equal(t.T, se3.exp(t.twist))


def test_refine_zero_goes_through_the_auto_launch_with_no_step(tables):
    from puzzlenet_amd import assembly, se3
    t, pieces = tables["auto0"], tables["pieces"]
    assert type(t) is assembly.AutoPairTable
    calls, today = tables["trace"]["auto0"], tables["trace"]["plain"]
    assert calls.count(AUTO_CALL) == 1 and "pzn_icp_refine_f32" not in calls and "pzn_icp_refine_trim_f32" not in calls
    assert len(calls) < len(today)                                            # it replaces the transform and the chamfer
    assert torch.equal(t.T, se3.exp(t.twist))
    for z in range(Z):
        score, score0, used, _, _ = _is_the_direct_launch(pieces[z], _puzzle(t, z), t.T[z], 0)
        assert torch.equal(score, score0) and int(used.abs().max()) == 0
    _same_as_far_as_reproducible(tables["plain"], tables["plain2"], t, [n for n in assembly.PairTable._fields if n not in ("T", "score")])


def test_match_puzzles_is_match_pairs_per_puzzle(tables, model):
    from puzzlenet_amd import assembly, se3
    t, pieces = tables["auto"], tables["pieces"]
    for z in range(Z):
        one = assembly.match_pairs(model, pieces[z], k=TOP, start=tuple(s[z] for s in tables["start"]), refine=REFINE, keep="auto")
        assert type(one) is assembly.AutoPairTable
        for name in assembly.AutoPairTable._fields:
            assert getattr(one, name).shape == getattr(t, name).shape[1:] and getattr(one, name).dtype == getattr(t, name).dtype, name
        # what does not pass the few-row layers has the same bits; the rest is the same launch on its own twist
        for name in ("de_fpcb", "de_mrpcb", "top_f", "top_m", "x2"):
            assert torch.equal(getattr(one, name), getattr(t, name)[z]), name
        assert _rel(one.twist, t.twist[z]) <= 1e-4
        _is_the_direct_launch(pieces[z], one, se3.exp(one.twist), REFINE)


def test_pair_block_is_pair_block_batch_of_one_puzzle(tables, model):
    from puzzlenet_amd import assembly, se3
    pieces, start = tables["pieces"], tables["start"]
    z = 1
    codes = assembly.encode_pieces(model, pieces[z], TOP, tuple(s[z] for s in start))
    one = assembly.pair_block(model, pieces[z], codes, pieces[z], codes, TOP, REFINE, assembly.AutoKeep(least=0.25, power=3))
    lifted = assembly.PieceCodes(*(f[None] for f in codes))
    batch = assembly.pair_block_batch(model, pieces[z][None], lifted, pieces[z][None], lifted, TOP, REFINE, "auto")
    assert type(one) is assembly.AutoPairBlock and type(batch) is assembly.AutoPairBlock
    assert one._fields == assembly.PairBlock._fields + ("kept_f", "kept_m", "count_f", "count_m", "objective")
    for name in one._fields:
        x, y = getattr(one, name), getattr(batch, name)
        assert y.shape == (1,) + x.shape and x.dtype == y.dtype, name
    assert torch.equal(one.de_fpcb, batch.de_fpcb[0]) and torch.equal(one.top_f, batch.top_f[0])
    assert _rel(one.twist, batch.twist[0]) <= 1e-4
    for blk in (one, assembly.AutoPairBlock(*(f[0] for f in batch))):
        K = P
        r = assembly.refine_pairs(pieces[z], blk.top_f, pieces[z], codes.top_m, se3.exp(blk.twist), iters=REFINE, keep="auto")
        assert type(r) is assembly.AutoRefined and r._fields == assembly.Refined._fields + ("kept_f", "kept_m", "count_f", "count_m", "objective")
        assert torch.equal(blk.T, r.T) and torch.equal(blk.score, r.score) and torch.equal(blk.kept_f, r.kept_f)
        assert torch.equal(blk.kept_m, r.kept_m) and torch.equal(blk.count_f, r.count_f) and torch.equal(blk.count_m, r.count_m)
        assert torch.equal(blk.objective, r.objective) and r.score0.shape == (K, K) and r.iters_used.dtype == torch.int32


def test_the_walks_take_the_table_and_the_joint_refinements_refuse_it(tables, monkeypatch):
    from puzzlenet_amd import _lib, assembly, ops
    t, pieces = tables["auto"], tables["pieces"]
    asm = assembly.assemble_batch(t.score, t.T)
    rule = assembly.walk_rule(t.score, t.T)
    assert [int(r) for r in asm.root.cpu()] == [int(r) for r in rule.root] and bool(asm.placed.bool().all())
    assert torch.equal(asm.joints.cpu(), torch.from_numpy(rule.joints))
    whole = assembly.assemble_forest_batch(t.score, t.T)
    assert [int(n) for n in whole.n_components.cpu()] == [1] * Z and torch.equal(whole.G, asm.G)
    low = 0.5 * float(t.score.min())                                          # below every score: nothing joins
    forest = assembly.assemble_forest_batch(t.score, t.T, max_score=low)
    want = assembly.forest_rule(t.score, t.T, max_score=low)
    assert forest.G.shape == (Z, P, 4, 4) and [int(n) for n in forest.n_components.cpu()] == [int(n) for n in want.n_components] == [P] * Z
    one = assembly.assemble(t.score[0], t.T[0])
    assert len(one.edges) == P - 1
    calls = []
    monkeypatch.setattr(ops, "_call", lambda *a, **k: calls.append(a[0]))
    with pytest.raises(_lib.PznUnsupported, match="per pair"):
        assembly.refine_assembly_batch(pieces, t, asm, sweeps=5)
    with pytest.raises(_lib.PznUnsupported, match="per pair"):
        assembly.refine_assembly(pieces[0], _puzzle(t, 0), one, sweeps=5)
    assert calls == []


def test_bad_auto_keep_raises_before_any_launch(tables, monkeypatch):
    from puzzlenet_amd import _lib, assembly, ops
    calls = []
    monkeypatch.setattr(ops, "_call", lambda *a, **k: calls.append(a[0]))
    t, pieces = tables["auto"], tables["pieces"]
    for keep in ("Auto", "automatic", assembly.AutoKeep(power=0), assembly.AutoKeep(power=5), assembly.AutoKeep(least=0),
                 assembly.AutoKeep(least=(0.5, 0.0)), assembly.AutoKeep(power=2.5)):
        with pytest.raises(_lib.PznError) as info:
            assembly.refine_pairs(pieces[0], t.top_f[0], pieces[0], t.top_m[0], t.T[0], iters=REFINE, keep=keep)
        assert not isinstance(info.value, _lib.PznUnsupported)
    assert calls == []
