"""GPU: the joint refinements with the counts of every joint FOUND under the joint poses (refine_assembly /
refine_assembly_batch with auto=: pzn_joint_refine_auto_f32), with the closed-form model and the pieces of
tests/test_gpu_assembly_joint_auto.py.  The kernel is held to today's launches, to exact integers and to float64 in
tests/test_gpu_joint_auto.py; here the assembly functions are compared, torch.equal, with each other and with a direct
ops.joint_refine(auto=) on sets gathered by hand, on tables made with keep = 1.0, keep = 0.5 and keep = "auto": the sets are
the full picked ones whatever kept fields the table carries."""
import pytest
import torch

from oracle import model_ref as mr
from tests.test_gpu_assembly_joint_auto import N, P, REFINE, SWEEPS, TOP, Z, _puzzle, _spied

pytestmark = pytest.mark.gpu

AUTO_CALL = "pzn_joint_refine_auto_f32"
FIELDS = ("G", "score", "score0", "sweeps_used", "accepted", "kept_f", "kept_m", "count_f", "count_m", "objective", "objective0")


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
    return dict(pieces=pieces, whole=make(1.0), trim=make(0.5), auto=make("auto"))


def _by_hand(pieces, t, asm, sweeps, auto):
    """ops.joint_refine(auto=) on the full picked sets of every ordered pair and of every moved piece, by plain indexing."""
    from puzzlenet_amd import ops
    dev = pieces.device
    a = torch.stack([pieces[z, i][t.top_f[z, i, j]] for z in range(Z) for i in range(P) for j in range(P)])
    b = torch.stack([pieces[z, j][t.top_m[z, j]] for z in range(Z) for j in range(P)])
    ji, jj = asm.joints[..., 0].long(), asm.joints[..., 1].long()
    first = torch.arange(Z, dtype=torch.long, device=dev)[:, None]
    a_of = torch.where(ji >= 0, (first * P + ji) * P + jj, torch.zeros_like(ji))
    b_of = torch.where(ji >= 0, first * P + jj, torch.zeros_like(ji))
    return ops.joint_refine(a, b, asm.joints, asm.G.to(torch.float32), asm.movable, sweeps, a_of=a_of, b_of=b_of, auto=auto,
                            return_kept=True)


@pytest.mark.parametrize("name", ["whole", "trim", "auto"])
def test_batch_refinement_with_counts_found_is_the_direct_launch_and_the_per_puzzle_one(tables, name):
    from puzzlenet_amd import assembly
    t, pieces = tables[name], tables["pieces"]
    assert type(t) is {"whole": assembly.PairTable, "trim": assembly.TrimmedPairTable, "auto": assembly.AutoPairTable}[name]
    asm = assembly.assemble_batch(t.score, t.T)
    out, calls = _spied(lambda: assembly.refine_assembly_batch(pieces, t, asm, sweeps=SWEEPS, auto=True))
    assert calls == ["pzn_gather_fwd_f32", AUTO_CALL] and type(out) is assembly.AutoJointRefined      # one gather, one launch
    lo = -(-TOP // 4)      # AutoKeep(): ceil(0.25 k)
    G, score, score0, _, used, accepted, kept_a, kept_b, count_a, count_b, objective, objective0 = _by_hand(pieces, t, asm, SWEEPS,
                                                                                                         (lo, lo, 3))
    for field, want in zip(FIELDS, (G, score, score0, used, accepted, kept_a, kept_b, count_a, count_b, objective, objective0)):
        assert torch.equal(getattr(out, field), want), field
    assert out.joints is asm.joints and bool((out.objective <= out.objective0).all()) and int(out.accepted.sum()) > 0
    live = asm.joints[..., 0] >= 0
    assert int(out.count_f[live].min()) >= lo and int(out.count_f[live].max()) <= TOP and int(out.count_f[~live].abs().sum()) == 0
    assert torch.equal((out.kept_f >= 0).sum(-1).to(torch.int32), out.count_f) and out.kept_f.shape == (Z, P * (P - 1), TOP)
    fixed = ~asm.movable.bool()
    assert bool(fixed.any()) and torch.equal(out.G[fixed], asm.G.to(torch.float32)[fixed])
    same = assembly.refine_assembly_batch(pieces, t, asm, sweeps=SWEEPS, auto=assembly.AutoKeep())      # True names the defaults
    assert all(torch.equal(getattr(out, f), getattr(same, f)) for f in FIELDS)
    for z in range(Z):      # per puzzle: refine_assembly on that puzzle's table and its own greedy walk
        tz = _puzzle(t, z)
        one, calls = _spied(lambda: assembly.refine_assembly(pieces[z], tz, assembly.assemble(tz.score, tz.T), sweeps=SWEEPS, auto=True))
        assert calls == ["pzn_gather_fwd_f32", AUTO_CALL] and type(one) is assembly.AutoJointRefined
        n = int(asm.n_joints[z])
        assert one.joints == [tuple(int(v) for v in r) for r in asm.joints[z, :n].cpu()]
        for field in FIELDS:
            got, want = getattr(out, field)[z], getattr(one, field)
            assert torch.equal(got[:n] if field in FIELDS[5:9] else got, want), (z, field)


def test_a_least_share_of_one_is_the_untrimmed_batch_refinement(tables):
    from puzzlenet_amd import assembly
    t, pieces = tables["whole"], tables["pieces"]
    asm = assembly.assemble_batch(t.score, t.T)
    found, calls = _spied(lambda: assembly.refine_assembly_batch(pieces, t, asm, sweeps=SWEEPS, auto=assembly.AutoKeep(least=1.0)))
    today, calls_today = _spied(lambda: assembly.refine_assembly_batch(pieces, t, asm, sweeps=SWEEPS))
    assert calls[-1] == AUTO_CALL and calls_today[-1] == "pzn_joint_refine_f32"
    for field in ("G", "score", "score0", "sweeps_used", "accepted"):
        assert torch.equal(getattr(found, field), getattr(today, field)), field
    live = asm.joints[..., 0] >= 0
    assert torch.equal(found.objective, found.score) and int((found.count_f[live] != TOP).sum()) == 0 and int(found.accepted.sum()) > 0


def test_the_refused_combinations_raise_before_any_launch(tables, monkeypatch):
    from puzzlenet_amd import _lib, assembly, ops
    t, pieces = tables["auto"], tables["pieces"]
    asm = assembly.assemble_batch(t.score, t.T)
    one = assembly.assemble(t.score[0], t.T[0])
    calls = []
    monkeypatch.setattr(ops, "_call", lambda *a, **k: calls.append(a[0]))
    both = (lambda **k: assembly.refine_assembly_batch(pieces, t, asm, sweeps=SWEEPS, **k),
            lambda **k: assembly.refine_assembly(pieces[0], _puzzle(t, 0), one, sweeps=SWEEPS, **k))
    for bad in (dict(auto=True, keep=0.5), dict(auto=True, keep="table"), dict(auto=True, kept="frozen"),
                dict(auto=assembly.AutoKeep(), keep=(0.5, 1.0)), dict(auto="auto"), dict(auto=0.5), dict(auto=1),
                dict(auto=assembly.AutoKeep(least=0.0)), dict(auto=assembly.AutoKeep(power=5)), dict(auto=assembly.AutoKeep(power=2.0)),
                dict(keep="auto"), dict(keep=assembly.AutoKeep())):      # the last two: refused as ever
        for fn in both:
            with pytest.raises(_lib.PznError) as info:
                fn(**bad)
            assert not isinstance(info.value, _lib.PznUnsupported), bad
    for fn in both:      # and the default still refuses an AutoPairTable
        with pytest.raises(_lib.PznUnsupported, match="per pair"):
            fn()
    assert calls == []
