"""GPU: the joint refinements on a table made with keep="auto" (refine_assembly / refine_assembly_batch with kept="frozen":
a kept count per joint through pzn_joint_refine_counts_f32), with the closed-form model and the pieces of
tests/test_gpu_assembly_auto.py.  The kernel is held to the launch without counts and to float64 in
tests/test_gpu_joint_counts.py; here the assembly functions are compared, torch.equal, with a direct ops.joint_refine on sets
gathered by hand from the table's OWN fields (kept_*[..., :count], NaN behind), where nothing is noisy."""
import pytest
import torch

from oracle import model_ref as mr

pytestmark = pytest.mark.gpu

Z, P, N, TOP = 2, 3, 1024, 128
REFINE = 4
SWEEPS = 5
COUNTS_CALL = "pzn_joint_refine_counts_f32"


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def tables(dev):
    from puzzlenet_amd import assembly
    from puzzlenet_amd import model5_b as mb
    model = mb.TouchedRegraster(mr.Cfg())
    mr.fill_params(model)
    model.to(dev)
    g = torch.Generator().manual_seed(1619)
    assert model.num_points == N
    pieces = torch.rand(Z, P, N, 3, generator=g).to(dev)
    start = (torch.randint(0, N, (Z, P), generator=g), torch.randint(0, 512, (Z, P), generator=g))
    make = lambda keep: assembly.match_puzzles(model, pieces, k=TOP, start=start, refine=REFINE, keep=keep)
    return dict(pieces=pieces, auto=make("auto"), whole=make(assembly.AutoKeep(least=1.0)), trim=make(0.5))


def _spied(fn):
    from puzzlenet_amd import ops
    real, calls = ops._call, []

    def spy(name, *a, **k):
        calls.append(name)
        return real(name, *a, **k)
    ops._call = spy
    try:
        out = fn()
    finally:
        ops._call = real
    return out, calls


def _puzzle(t, z):
    return type(t)(*(f[z] for f in t))


def _by_hand(pieces, t, asm, sweeps):
    """ops.joint_refine on the kept rows of every ordered pair, picked by plain indexing: 2 Z P^2 sets of stride k, the first
    count rows the kept points and NaN behind them."""
    from puzzlenet_amd import ops
    dev = pieces.device
    a = torch.full((Z * P * P, TOP, 3), float("nan"), device=dev)
    b = torch.full((Z * P * P, TOP, 3), float("nan"), device=dev)
    for z in range(Z):
        for i in range(P):
            for j in range(P):
                s, cf, cm = (z * P + i) * P + j, int(t.count_f[z, i, j]), int(t.count_m[z, i, j])
                a[s, :cf] = pieces[z, i][t.top_f[z, i, j][t.kept_f[z, i, j, :cf].long()]]
                b[s, :cm] = pieces[z, j][t.top_m[z, j][t.kept_m[z, i, j, :cm].long()]]
    ji, jj = asm.joints[..., 0].long(), asm.joints[..., 1].long()
    first = torch.arange(Z, dtype=torch.long, device=dev)[:, None]
    of = torch.where(ji >= 0, (first * P + ji) * P + jj, torch.zeros_like(ji))
    return ops.joint_refine(a, b, asm.joints, asm.G.to(torch.float32), asm.movable, sweeps, a_of=of, b_of=of,
                            na=t.count_f.reshape(-1), nb=t.count_m.reshape(-1))


def _keeps_the_fixed(out, asm):
    """score <= score0; the root of every component and every unplaced piece keep asm.G's bits."""
    assert bool((out.score <= out.score0).all())
    fixed = ~asm.movable.bool()
    assert bool(fixed.any()) and torch.equal(out.G[fixed], asm.G.to(torch.float32)[fixed])
    assert int(out.accepted[fixed].abs().max()) == 0


def test_batch_refinement_of_an_auto_table_is_the_direct_launch_on_its_kept_rows(tables):
    from puzzlenet_amd import assembly
    t, pieces = tables["auto"], tables["pieces"]
    assert type(t) is assembly.AutoPairTable
    off = ~torch.eye(P, dtype=torch.bool, device=pieces.device).expand(Z, P, P)
    assert len(set(t.count_f[off].tolist())) > 1 and int(t.count_f[off].min()) < TOP      # the counts do differ per pair
    asm = assembly.assemble_batch(t.score, t.T)
    out, calls = _spied(lambda: assembly.refine_assembly_batch(pieces, t, asm, sweeps=SWEEPS, kept="frozen"))
    assert calls == ["pzn_gather_fwd_f32", COUNTS_CALL]                       # one gather, one launch
    G, score, score0, _, used, accepted = _by_hand(pieces, t, asm, SWEEPS)
    assert torch.equal(out.G, G) and torch.equal(out.score, score) and torch.equal(out.score0, score0)
    assert torch.equal(out.sweeps_used, used) and torch.equal(out.accepted, accepted) and out.joints is asm.joints
    _keeps_the_fixed(out, asm)
    assert int(out.accepted.sum()) > 0 and bool((out.score < out.score0).any())
    # per puzzle: refine_assembly on that puzzle's table and its own greedy walk
    for z in range(Z):
        tz = _puzzle(t, z)
        one, calls = _spied(lambda: assembly.refine_assembly(pieces[z], tz, assembly.assemble(tz.score, tz.T), sweeps=SWEEPS,
                                                             kept="frozen"))
        assert calls == ["pzn_gather_fwd_f32", COUNTS_CALL]
        assert torch.equal(out.G[z], one.G) and torch.equal(out.score[z], one.score) and torch.equal(out.score0[z], one.score0)
        assert torch.equal(out.accepted[z], one.accepted) and torch.equal(out.sweeps_used[z], one.sweeps_used)
        n = int(asm.n_joints[z])
        assert one.joints == [tuple(int(v) for v in r) for r in asm.joints[z, :n].cpu()]


def test_an_auto_table_that_keeps_every_row_is_the_untrimmed_table(tables):
    """AutoKeep(least=1.0): every count is k and kept_* is 0 .. k-1, so freezing the kept sets is refining the table's picks:
    include/pzn.h's "lo = k is the untrimmed launch bit for bit", one level up."""
    from puzzlenet_amd import assembly
    t, pieces = tables["whole"], tables["pieces"]
    assert type(t) is assembly.AutoPairTable
    assert int(t.count_f.min()) == int(t.count_f.max()) == TOP and int(t.count_m.min()) == int(t.count_m.max()) == TOP
    plain = assembly.PairTable(*t[:len(assembly.PairTable._fields)])
    asm = assembly.assemble_batch(t.score, t.T)
    frozen, calls = _spied(lambda: assembly.refine_assembly_batch(pieces, t, asm, sweeps=SWEEPS, kept="frozen"))
    today, calls_today = _spied(lambda: assembly.refine_assembly_batch(pieces, plain, asm, sweeps=SWEEPS))
    assert calls[-1] == COUNTS_CALL and calls_today[-1] == "pzn_joint_refine_f32"
    for name in ("G", "score", "score0", "sweeps_used", "accepted"):
        assert torch.equal(getattr(frozen, name), getattr(today, name)), name
    assert int(frozen.accepted.sum()) > 0


def test_kept_frozen_changes_nothing_for_tables_of_one_size(tables):
    from puzzlenet_amd import assembly
    pieces = tables["pieces"]
    for t in (tables["trim"], assembly.PairTable(*tables["whole"][:len(assembly.PairTable._fields)])):
        asm = assembly.assemble_batch(t.score, t.T)
        named, calls = _spied(lambda: assembly.refine_assembly_batch(pieces, t, asm, sweeps=SWEEPS, kept="frozen"))
        default, calls0 = _spied(lambda: assembly.refine_assembly_batch(pieces, t, asm, sweeps=SWEEPS))
        assert calls == calls0 == ["pzn_gather_fwd_f32", "pzn_joint_refine_f32"]      # the same launch as ever
        for name in ("G", "score", "score0", "sweeps_used", "accepted"):
            assert torch.equal(getattr(named, name), getattr(default, name)), name
        tz = _puzzle(t, 0)
        walk = assembly.assemble(tz.score, tz.T)
        one = assembly.refine_assembly(pieces[0], tz, walk, sweeps=SWEEPS, kept="frozen")
        one0 = assembly.refine_assembly(pieces[0], tz, walk, sweeps=SWEEPS)
        assert torch.equal(one.G, one0.G) and torch.equal(one.score, one0.score) and torch.equal(one.accepted, one0.accepted)
    assert type(tables["trim"]) is assembly.TrimmedPairTable and tables["trim"].kept_f.shape[-1] == TOP // 2


def test_the_defaults_still_refuse_and_a_bad_kept_is_an_error_before_any_launch(tables, monkeypatch):
    from puzzlenet_amd import _lib, assembly, ops
    t, pieces = tables["auto"], tables["pieces"]
    asm = assembly.assemble_batch(t.score, t.T)
    one = assembly.assemble(t.score[0], t.T[0])
    calls = []
    monkeypatch.setattr(ops, "_call", lambda *a, **k: calls.append(a[0]))
    with pytest.raises(_lib.PznUnsupported, match="per pair"):
        assembly.refine_assembly_batch(pieces, t, asm, sweeps=SWEEPS)
    with pytest.raises(_lib.PznUnsupported, match="per pair"):
        assembly.refine_assembly(pieces[0], _puzzle(t, 0), one, sweeps=SWEEPS, kept=None)
    for bad in ("Frozen", "retrim", True, 0):
        with pytest.raises(_lib.PznError) as info:
            assembly.refine_assembly_batch(pieces, t, asm, sweeps=SWEEPS, kept=bad)
        assert not isinstance(info.value, _lib.PznUnsupported)
        with pytest.raises(_lib.PznError) as info:
            assembly.refine_assembly(pieces[0], _puzzle(t, 0), one, sweeps=SWEEPS, kept=bad)
        assert not isinstance(info.value, _lib.PznUnsupported)
    assert calls == []


def test_a_forest_over_an_auto_table_is_refined_component_by_component(tables):
    from puzzlenet_amd import assembly
    t, pieces = tables["auto"], tables["pieces"]
    off = ~torch.eye(P, dtype=torch.bool, device=pieces.device).expand(Z, P, P)
    # the largest of the puzzles' smallest scores: every puzzle has an entry at or below it, and the puzzle it comes from has no
    # other (the reverse direction of a pair is an entry of its own), so that pile splits into a pair and a piece alone
    limit = float(t.score.masked_fill(~off, float("inf")).reshape(Z, -1).min(dim=1).values.max())
    forest = assembly.assemble_forest_batch(t.score, t.T, max_score=limit)
    assert int(forest.n_components.max()) == 2 and int(forest.n_components.min()) >= 1
    out, calls = _spied(lambda: assembly.refine_assembly_batch(pieces, t, forest, sweeps=SWEEPS, kept="frozen"))
    assert calls == ["pzn_gather_fwd_f32", COUNTS_CALL]
    _keeps_the_fixed(out, forest)
    assert int((~forest.movable.bool()).sum()) == int(forest.n_components.sum())      # a root per component, every piece in one
    G, score, score0, _, used, accepted = _by_hand(pieces, t, forest, SWEEPS)
    assert torch.equal(out.G, G) and torch.equal(out.score, score) and torch.equal(out.accepted, accepted)
