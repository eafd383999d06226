"""GPU: keep < 1 through the assembly functions - match_puzzles / match_pairs / refine_pairs and the joint refinements on a
table that carries kept sets - with the closed-form model of tests/test_gpu_assembly.py.  The trimmed kernel itself is held to
float64 in tests/test_gpu_icp_trim.py; here every trimmed field is compared, torch.equal, with a direct ops.icp_refine(...,
keep=...) or ops.joint_refine on sets gathered by hand from the table's OWN picks and poses, where nothing is noisy.

Two calls of match_puzzles need not agree bit for bit in the fields behind the few-row layers (tests/test_gpu_assembly_batch.py);
a field is therefore compared with today's call by torch.equal where two of today's calls are torch.equal, and by the atomic
rule of tests/test_gpu_assembly_refine.py where they are not."""
import numpy as np
import pytest
import torch

from oracle import model_ref as mr

pytestmark = pytest.mark.gpu

Z, P, N, TOP = 2, 3, 1024, 128
REFINE = 4
KEEP = 0.5
M = 64                  # ceil(KEEP * TOP)
ATOMIC_REL = 5e-6       # tests/test_gpu_assembly_refine.py's


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
    g = torch.Generator().manual_seed(1618)
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
    return dict(pieces=pieces, start=start, trace=trace, plain=traced("plain"), plain2=traced("plain2"), one=traced("one", keep=1.0),
                fine=traced("fine", refine=REFINE), fine2=traced("fine2", refine=REFINE),
                trim=traced("trim", refine=REFINE, keep=KEEP), trim0=traced("trim0", refine=0, keep=KEEP))


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


def _gathered(pieces, t):
    """The picked sets of every ordered pair by plain indexing: Bf [Z P P,k,3], Bm [Z P P,k,3] (the moved piece's set repeated)."""
    Bf = torch.stack([pieces[z, i][t.top_f[z, i, j]] for z in range(Z) for i in range(P) for j in range(P)])
    Bm = torch.stack([pieces[z, j][t.top_m[z, j]] for z in range(Z) for i in range(P) for j in range(P)])
    return Bf.contiguous(), Bm.contiguous()


def _masked(score):
    return score.view(Z, P, P).masked_fill(torch.eye(P, dtype=torch.bool, device=score.device), float("inf"))


def test_keep_one_is_todays_table(tables):
    from puzzlenet_amd import assembly
    t = tables["one"]
    assert type(t) is assembly.PairTable and t.kept_f is None and t.kept_m is None
    assert type(tables["plain"]) is assembly.PairTable and tables["plain"].kept_f is None
    _same_as_far_as_reproducible(tables["plain"], tables["plain2"], t, assembly.PairTable._fields)
    assert tables["trace"]["one"] == tables["trace"]["plain"]                 # the same launches
    assert not any("icp" in c for c in tables["trace"]["one"])


def test_trimmed_table_is_the_direct_trimmed_launch(tables):
    from puzzlenet_amd import assembly, ops, se3
    t, pieces = tables["trim"], tables["pieces"]
    assert type(t) is assembly.TrimmedPairTable and t._fields == assembly.PairTable._fields + ("kept_f", "kept_m")
    assert t.kept_f.shape == (Z, P, P, M) and t.kept_m.shape == (Z, P, P, M) and t.kept_f.dtype == torch.int32
    # one trimmed launch in place of today's untrimmed one, nothing else changes
    calls, today = tables["trace"]["trim"], tables["trace"]["fine"]
    assert calls == [("pzn_icp_refine_trim_f32" if c == "pzn_icp_refine_f32" else c) for c in today]
    assert calls.count("pzn_icp_refine_trim_f32") == 1
    others = [n for n in assembly.PairTable._fields if n not in ("T", "score")]
    _same_as_far_as_reproducible(tables["fine"], tables["fine2"], t, others)
    Bf, Bm = _gathered(pieces, t)
    T0 = se3.exp(t.twist).reshape(Z * P * P, 4, 4)
    T, score, score0, used, kept_f, kept_m = ops.icp_refine(Bf, Bm, T0, REFINE, keep=(M, M), return_kept=True)
    assert torch.equal(t.T, T.view(Z, P, P, 4, 4)) and torch.equal(t.score, _masked(score))
    assert torch.equal(t.kept_f, kept_f.view(Z, P, P, M)) and torch.equal(t.kept_m, kept_m.view(Z, P, P, M))
    assert bool((score <= score0).all()) and int(used.max()) >= 1 and not torch.equal(t.T, se3.exp(t.twist))
    # the trimmed score of a pair is never above today's score of its start pose: it is a mean over the smaller half
    d1, d2 = ops.chamfer(Bf, se3.transform_points(T0, Bm))
    assert bool((score0 <= d1.mean(dim=1) + d2.mean(dim=1)).all())


def test_refine_zero_is_the_trimmed_score_of_the_networks_pose(tables):
    from puzzlenet_amd import assembly, ops, se3
    t, pieces = tables["trim0"], tables["pieces"]
    assert type(t) is assembly.TrimmedPairTable
    calls, today = tables["trace"]["trim0"], tables["trace"]["plain"]
    assert calls.count("pzn_icp_refine_trim_f32") == 1 and "pzn_icp_refine_f32" not in calls
    assert len(calls) < len(today)                                            # it replaces the transform and the chamfer
    assert torch.equal(t.T, se3.exp(t.twist))
    Bf, Bm = _gathered(pieces, t)
    T, score, score0, used, kept_f, kept_m = ops.icp_refine(Bf, Bm, t.T.reshape(Z * P * P, 4, 4), 0, keep=(M, M), return_kept=True)
    assert torch.equal(t.score, _masked(score)) and torch.equal(score, score0) and int(used.abs().max()) == 0
    assert torch.equal(t.kept_f, kept_f.view(Z, P, P, M)) and torch.equal(t.kept_m, kept_m.view(Z, P, P, M))
    _same_as_far_as_reproducible(tables["plain"], tables["plain2"], t, [n for n in assembly.PairTable._fields if n not in ("T", "score")])


def test_keep_per_side_and_the_per_puzzle_functions(tables, model):
    from puzzlenet_amd import assembly, ops
    t, pieces = tables["trim"], tables["pieces"]
    z = 1
    r = assembly.refine_pairs(pieces[z], t.top_f[z], pieces[z], t.top_m[z], t.T[z], iters=REFINE, keep=(1.0, 0.25))
    assert type(r) is assembly.TrimmedRefined and r.kept_f.shape == (P, P, TOP) and r.kept_m.shape == (P, P, TOP // 4)
    Bf, Bm = _gathered(pieces, t)
    sl = slice(z * P * P, (z + 1) * P * P)
    want = ops.icp_refine(Bf[sl], Bm[sl], t.T[z].reshape(P * P, 4, 4), REFINE, keep=(TOP, TOP // 4), return_kept=True)
    for got, w in zip(r, want):
        assert torch.equal(got.reshape(w.shape), w)
    assert torch.equal(r.kept_f, torch.arange(TOP, dtype=torch.int32, device=pieces.device).expand(P, P, TOP))
    plain = assembly.refine_pairs(pieces[z], t.top_f[z], pieces[z], t.top_m[z], t.T[z], iters=REFINE)
    assert type(plain) is assembly.Refined and plain.kept_f is None and len(plain) == 4
    one = assembly.match_pairs(model, pieces[z], k=TOP, start=tuple(s[z] for s in tables["start"]), refine=REFINE, keep=KEEP)
    assert type(one) is assembly.TrimmedPairTable and one.kept_f.shape == (P, P, M) and one.T.shape == (P, P, 4, 4)
    assert torch.equal(one.top_m, t.top_m[z]) and torch.equal(one.x2, t.x2[z])
    # ceil(f k), at least 1; every row kept on both sides is today's path
    assert assembly._keep_counts(0.3, 128, 128, "t") == (39, 39) and assembly._keep_counts((1e-9, 1.0), 128, 100, "t") == (1, 100)
    assert assembly._keep_counts(1.0, 128, 128, "t") is None and assembly._keep_counts((1.0, 1), 128, 128, "t") is None


def test_bad_keep_raises_before_any_launch(tables, model, monkeypatch):
    from puzzlenet_amd import _lib, assembly, ops
    calls = []
    monkeypatch.setattr(ops, "_call", lambda *a, **k: calls.append(a[0]))
    t, pieces = tables["trim"], tables["pieces"]
    for keep in (0.0, -0.5, 1.5, (0.5,), (0.5, 0.5, 0.5), "half", None, (0.5, 0.0), True):
        with pytest.raises(_lib.PznError):
            assembly.refine_pairs(pieces[0], t.top_f[0], pieces[0], t.top_m[0], t.T[0], iters=REFINE, keep=keep)
    assert calls == []


def _assembly_of(rule, z):
    from puzzlenet_amd import assembly
    n = int(rule.n_edges[z])
    edges = [(int(i), int(j), float(s), int(new)) for (i, j, new), s in zip(rule.edges[z, :n], rule.edge_score[z, :n])]
    return assembly.Assembly(int(rule.root[z]), edges, rule.G[z], rule.placed[z].astype(bool))


def test_joint_refinement_freezes_the_kept_sets(tables):
    from puzzlenet_amd import assembly, ops
    t, pieces = tables["trim"], tables["pieces"]
    dev = pieces.device
    asm = assembly.assemble_batch(t.score, t.T, joint_score=float("inf"))
    rule = assembly.walk_rule(t.score, t.T, joint_score=float("inf"))
    assert torch.equal(asm.joints.cpu(), torch.from_numpy(rule.joints))
    real, calls = ops._call, []

    def spy(name, *a, **k):
        calls.append(name)
        return real(name, *a, **k)
    ops._call = spy
    try:
        out = assembly.refine_assembly_batch(pieces, t, asm, sweeps=30)
    finally:
        ops._call = real
    assert calls == ["pzn_gather_fwd_f32", "pzn_joint_refine_f32"]            # the existing kernel, one gather, one launch
    # the kept rows of every ordered pair by plain indexing, then ops.joint_refine itself
    a = torch.stack([pieces[z, i][t.top_f[z, i, j][t.kept_f[z, i, j].long()]] for z in range(Z) for i in range(P) for j in range(P)])
    b = torch.stack([pieces[z, j][t.top_m[z, j][t.kept_m[z, i, j].long()]] for z in range(Z) for i in range(P) for j in range(P)])
    assert a.shape == (Z * P * P, M, 3) and b.shape == (Z * P * P, M, 3)
    ji, jj = asm.joints[..., 0].long(), asm.joints[..., 1].long()
    first = torch.arange(Z, dtype=torch.long, device=dev)[:, None]
    of = torch.where(ji >= 0, (first * P + ji) * P + jj, torch.zeros_like(ji))
    G, score, score0, _, used, accepted = ops.joint_refine(a.contiguous(), b.contiguous(), asm.joints, asm.G.to(torch.float32),
                                                           asm.movable, 30, a_of=of, b_of=of)
    assert torch.equal(out.G, G) and torch.equal(out.score, score) and torch.equal(out.score0, score0)
    assert torch.equal(out.sweeps_used, used) and torch.equal(out.accepted, accepted)
    assert bool((out.score <= out.score0).all()) and int(out.accepted.sum()) > 0
    # its start energy is the sum of the untrimmed score over the kept rows: not the table's trimmed scores re-trimmed
    for z in range(Z):
        one = assembly.refine_assembly(pieces[z], type(t)(*(f[z] for f in t)), _assembly_of(rule, z), sweeps=30,
                                       joint_score=float("inf"))
        n = int(rule.n_joints[z])
        assert one.joints == [tuple(int(v) for v in r) for r in rule.joints[z, :n]] and n == P * (P - 1)
        assert torch.equal(out.G[z], one.G) and torch.equal(out.score[z], one.score) and torch.equal(out.score0[z], one.score0)
        assert torch.equal(out.accepted[z], one.accepted) and torch.equal(out.sweeps_used[z], one.sweeps_used)
