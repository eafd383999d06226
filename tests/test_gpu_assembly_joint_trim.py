"""GPU: refine_assembly(..., keep=) and refine_assembly_batch(..., keep=) - the joint refinement that chooses the kept rows of
every joint again under the joint poses (pzn_joint_refine_trim_f32) - on match_puzzles tables made with keep=1.0, keep=0.5
and keep="auto", with the closed-form model of tests/test_gpu_assembly_joint_auto.py.  The kernel is held to today's launch and
to float64 in tests/test_gpu_joint_trim.py; here the batch function is compared, torch.equal, with the per-puzzle one and with
a direct ops.joint_refine on sets gathered by hand."""
import pytest
import torch

from oracle import model_ref as mr

pytestmark = pytest.mark.gpu

Z, P, N, TOP = 4, 4, 1024, 128
REFINE = 4
SWEEPS = 5
TRIM_CALL = "pzn_joint_refine_trim_f32"
FIELDS = ("G", "score", "score0", "sweeps_used", "accepted")


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
    g = torch.Generator().manual_seed(1621)
    assert model.num_points == N
    pieces = torch.rand(Z, P, N, 3, generator=g).to(dev)
    start = (torch.randint(0, N, (Z, P), generator=g), torch.randint(0, 512, (Z, P), generator=g))
    make = lambda keep: assembly.match_puzzles(model, pieces, k=TOP, start=start, refine=REFINE, keep=keep)
    t = dict(pieces=pieces, whole=make(1.0), trim=make(0.5), auto=make("auto"))
    assert type(t["whole"]) is assembly.PairTable and type(t["trim"]) is assembly.TrimmedPairTable
    assert type(t["auto"]) is assembly.AutoPairTable
    return t


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


def _by_hand(pieces, t, asm, ma, mb, sweeps):
    """ops.joint_refine on the FULL sets of every ordered pair and moved piece, picked by plain indexing."""
    from puzzlenet_amd import ops
    dev = pieces.device
    a = torch.stack([pieces[z, i][t.top_f[z, i, j]] for z in range(Z) for i in range(P) for j in range(P)])
    b = torch.stack([pieces[z, j][t.top_m[z, j]] for z in range(Z) for j in range(P)])
    ji, jj = asm.joints[..., 0].long(), asm.joints[..., 1].long()
    first = torch.arange(Z, dtype=torch.long, device=dev)[:, None]
    live = ji >= 0
    a_of = torch.where(live, (first * P + ji) * P + jj, torch.zeros_like(ji))
    b_of = torch.where(live, first * P + jj, torch.zeros_like(ji))
    return ops.joint_refine(a, b, asm.joints, asm.G.to(torch.float32), asm.movable, sweeps, a_of=a_of, b_of=b_of, ma=ma, mb=mb,
                            return_kept=True), a_of


CASES = [("whole", 0.5), ("trim", 0.5), ("trim", "table"), ("auto", 0.5), ("auto", "table")]


@pytest.mark.parametrize("name,keep", CASES, ids=[f"{n}-{k}" for n, k in CASES])
def test_batch_is_the_per_puzzle_refinement_and_the_direct_launch(tables, name, keep):
    from puzzlenet_amd import assembly
    t, pieces = tables[name], tables["pieces"]
    dev = pieces.device
    asm = assembly.assemble_batch(t.score, t.T)
    J = P * (P - 1)
    out, calls = _spied(lambda: assembly.refine_assembly_batch(pieces, t, asm, sweeps=SWEEPS, keep=keep))
    assert calls == ["pzn_gather_fwd_f32", TRIM_CALL]                              # one gather, the one new entry point
    assert type(out) is assembly.TrimmedJointRefined and out.joints is asm.joints
    assert out.kept_f.shape == (Z, J, TOP) and out.kept_m.shape == (Z, J, TOP) and out.count_f.shape == (Z, J)
    assert bool((out.score <= out.score0).all())
    fixed = ~asm.movable.bool()
    assert torch.equal(out.G[fixed], asm.G.to(torch.float32)[fixed]) and int(out.accepted[fixed].abs().max()) == 0
    # the counts: the fraction's ceil(f k), or the table's own
    live = asm.joints[..., 0] >= 0
    if keep == 0.5:
        assert int(out.count_f.min()) == int(out.count_f.max()) == TOP // 2 == int(out.count_m.min()) == int(out.count_m.max())
    elif name == "trim":
        assert int(out.count_f.min()) == int(out.count_f.max()) == t.kept_f.shape[-1] == TOP // 2
    else:
        ji, jj = asm.joints[..., 0].long().clamp(min=0), asm.joints[..., 1].long().clamp(min=0)
        z = torch.arange(Z, device=dev)[:, None].expand(Z, J)
        assert torch.equal(out.count_f[live], t.count_f[z, ji, jj][live].to(torch.int32))
        assert torch.equal(out.count_m[live], t.count_m[z, ji, jj][live].to(torch.int32))
        assert len(set(out.count_f[live].tolist())) > 1                               # they do differ per joint
    # the kept rows: count of them, ascending, then -1; all -1 on an unused row
    for kept, count in ((out.kept_f, out.count_f), (out.kept_m, out.count_m)):
        n_kept = (kept >= 0).sum(dim=-1)
        assert torch.equal(n_kept[live], count[live].long()) and int(n_kept[~live].sum()) == 0
        behind = torch.arange(TOP, device=dev).expand_as(kept) >= count[..., None]
        assert bool((kept[live][behind[live]] == -1).all()) and bool((kept[live].diff(dim=-1)[~behind[live][:, 1:]] > 0).all())
    # the direct launch on the full sets, whatever the table carries
    (G, score, score0, _, used, accepted, kept_a, kept_b), _ = _by_hand(pieces, t, asm, out.count_f, out.count_m, SWEEPS)
    assert torch.equal(out.G, G) and torch.equal(out.score, score) and torch.equal(out.score0, score0)
    assert torch.equal(out.sweeps_used, used) and torch.equal(out.accepted, accepted)
    assert torch.equal(out.kept_f, kept_a) and torch.equal(out.kept_m, kept_b)
    assert int(out.accepted.sum()) > 0
    # per puzzle: refine_assembly on that puzzle's table and its own greedy walk, bit for bit
    for z in range(Z):
        tz = _puzzle(t, z)
        one, calls = _spied(lambda: assembly.refine_assembly(pieces[z], tz, assembly.assemble(tz.score, tz.T), sweeps=SWEEPS, keep=keep))
        assert calls == ["pzn_gather_fwd_f32", TRIM_CALL] and type(one) is assembly.TrimmedJointRefined
        for f in FIELDS:
            assert torch.equal(getattr(out, f)[z], getattr(one, f)), (z, f)
        n = int(asm.n_joints[z])
        assert one.joints == [tuple(int(v) for v in r) for r in asm.joints[z, :n].cpu()]
        for f in ("kept_f", "kept_m", "count_f", "count_m"):
            assert torch.equal(getattr(out, f)[z, :n], getattr(one, f)), (z, f)


def test_keep_none_is_today_s_path_and_keep_one_today_s_launch(tables):
    from puzzlenet_amd import assembly
    pieces = tables["pieces"]
    for name in ("whole", "trim"):
        t = tables[name]
        asm = assembly.assemble_batch(t.score, t.T)
        today, calls0 = _spied(lambda: assembly.refine_assembly_batch(pieces, t, asm, sweeps=SWEEPS))
        named, calls = _spied(lambda: assembly.refine_assembly_batch(pieces, t, asm, sweeps=SWEEPS, keep=None))
        assert calls == calls0 == ["pzn_gather_fwd_f32", "pzn_joint_refine_f32"] and type(named) is assembly.JointRefined
        for f in FIELDS:
            assert torch.equal(getattr(today, f), getattr(named, f)), f
        tz = _puzzle(t, 0)
        walk = assembly.assemble(tz.score, tz.T)
        one0, one = (assembly.refine_assembly(pieces[0], tz, walk, sweeps=SWEEPS, **kw) for kw in ({}, {"keep": None}))
        assert type(one) is assembly.JointRefined and all(torch.equal(getattr(one0, f), getattr(one, f)) for f in FIELDS)
    # keep = 1.0: the untrimmed launch over the FULL sets - on the untrimmed table that is today's result
    t = tables["whole"]
    asm = assembly.assemble_batch(t.score, t.T)
    today = assembly.refine_assembly_batch(pieces, t, asm, sweeps=SWEEPS)
    whole, calls = _spied(lambda: assembly.refine_assembly_batch(pieces, t, asm, sweeps=SWEEPS, keep=1.0))
    assert calls == ["pzn_gather_fwd_f32", "pzn_joint_refine_f32"] and type(whole) is assembly.TrimmedJointRefined
    assert all(torch.equal(getattr(today, f), getattr(whole, f)) for f in FIELDS)
    live = asm.joints[..., 0] >= 0
    full = torch.arange(TOP, dtype=torch.int32, device=pieces.device)
    assert bool((whole.kept_f[live] == full).all()) and bool((whole.kept_f[~live] == -1).all()) and int(whole.count_m.min()) == TOP
    # and on a trimmed table keep = 1.0 reads the full sets, not the table's kept rows
    other = assembly.refine_assembly_batch(pieces, tables["trim"], assembly.assemble_batch(tables["trim"].score, tables["trim"].T),
                                           sweeps=SWEEPS, keep=1.0)
    assert other.kept_f.shape[-1] == TOP


def test_an_auto_table_with_keep_is_not_refused_and_bad_keywords_launch_nothing(tables, monkeypatch):
    from puzzlenet_amd import _lib, assembly, ops
    t, pieces = tables["auto"], tables["pieces"]
    asm = assembly.assemble_batch(t.score, t.T)
    out = assembly.refine_assembly_batch(pieces, t, asm, sweeps=SWEEPS, keep="table")      # not refused
    assert type(out) is assembly.TrimmedJointRefined and bool((out.score <= out.score0).all())
    calls = []
    monkeypatch.setattr(ops, "_call", lambda *a, **k: calls.append(a[0]))
    one = assembly.assemble(t.score[0], t.T[0])
    for kw in (dict(keep=0.5, kept="frozen"), dict(keep="table", kept="frozen"), dict(keep="auto"), dict(keep=0.0), dict(keep=(0.5, 1.5))):
        with pytest.raises(_lib.PznError) as info:
            assembly.refine_assembly_batch(pieces, t, asm, sweeps=SWEEPS, **kw)
        assert not isinstance(info.value, _lib.PznUnsupported)
        with pytest.raises(_lib.PznError) as info:
            assembly.refine_assembly(pieces[0], _puzzle(t, 0), one, sweeps=SWEEPS, **kw)
        assert not isinstance(info.value, _lib.PznUnsupported)
    with pytest.raises(_lib.PznError, match="carries counts"):
        assembly.refine_assembly_batch(pieces, tables["whole"], asm, sweeps=SWEEPS, keep="table")
    with pytest.raises(_lib.PznUnsupported, match="per pair"):                              # the default still refuses
        assembly.refine_assembly_batch(pieces, t, asm, sweeps=SWEEPS)
    assert calls == []
