"""GPU: ops.merge_resample (csrc/mergefps.hip) - transform, union, drop lists and farthest point sampling in one launch -
bit for bit against the CPU restatement tests/_merge_ref.py and against the existing FPS kernel."""
import pytest
import torch

from tests import _merge_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _inputs(dev, seed, M, Na, Nb, starts):
    from puzzlenet_amd import se3
    g = torch.Generator().manual_seed(seed)
    a = torch.rand(M, Na, 3, generator=g)
    b = torch.rand(M, Nb, 3, generator=g)
    twist = (torch.rand(M, 6, generator=g) - 0.5) * 2.0
    T = se3.exp(twist.to(dev)).cpu()
    return a, b, T, torch.tensor(starts, dtype=torch.long)


def _run(dev, a, b, T, start, n_out, drop_a=None, drop_b=None):
    from puzzlenet_amd import ops
    d = lambda t: None if t is None else t.to(dev)
    out, src = ops.merge_resample(d(a), d(b), d(T), d(start), n_out, d(drop_a), d(drop_b))
    assert out.shape == (a.shape[0], n_out, 3) and out.dtype == torch.float32
    assert src.shape == (a.shape[0], n_out) and src.dtype == torch.int64
    return out.cpu(), src.cpu()


@pytest.fixture(scope="module")
def big(dev):
    """Na = Nb = n_out = 1024, M = 3, no drops, one start inside b's range: inputs, the device's result and the
    restatement's, computed once."""
    a, b, T, start = _inputs(dev, 31, 3, 1024, 1024, [5, 1500, 1023])
    got = _run(dev, a, b, T, start, 1024)
    want = _merge_ref.merge_resample(a, b, T, start, 1024)
    return dict(a=a, b=b, T=T, start=start, got=got, want=want)


def test_bit_exact_no_drops(big):
    assert torch.equal(big["got"][1], big["want"][1])
    assert torch.equal(big["got"][0], big["want"][0])


def test_bit_exact_with_drops(dev, big):
    a, b, T = big["a"], big["b"], big["T"]
    g = torch.Generator().manual_seed(32)
    drop_a = torch.stack([torch.randperm(1024, generator=g)[:128] for _ in range(3)])
    drop_b = torch.stack([torch.randperm(1024, generator=g)[:128] for _ in range(3)])
    drop_a[1, 7] = drop_a[1, 3]                                     # a repeated index
    start = torch.tensor([int(drop_a[0, 0]), 1024 + int(drop_b[1, 5]), 77], dtype=torch.long)      # two starts on dropped rows
    if bool((drop_a[2] == 77).any()):
        start[2] = 78
    got = _run(dev, a, b, T, start, 1024, drop_a, drop_b)
    want = _merge_ref.merge_resample(a, b, T, start, 1024, drop_a, drop_b)
    assert torch.equal(got[1], want[1])
    assert torch.equal(got[0], want[0])
    for m in range(3):
        dropped = set(drop_a[m].tolist()) | set((drop_b[m] + 1024).tolist())
        assert not dropped & set(got[1][m].tolist()), m
    assert int(got[1][0, 0]) != int(start[0]) and int(got[1][1, 0]) != int(start[1])


def test_bit_exact_odd_sizes(dev):
    """Sizes that are no multiple of 64, a union of exactly one row per thread (96 + 160 = 256), n_out below Na."""
    a, b, T, start = _inputs(dev, 33, 2, 96, 160, [200, 3])
    g = torch.Generator().manual_seed(34)
    drop_a = torch.stack([torch.randperm(96, generator=g)[:10] for _ in range(2)])
    for da in (None, drop_a):
        got = _run(dev, a, b, T, start, 64, da, None)
        want = _merge_ref.merge_resample(a, b, T, start, 64, da, None)
        assert torch.equal(got[1], want[1]) and torch.equal(got[0], want[0])


@pytest.mark.parametrize("Na,Nb,n_out", [(100, 100, 64),        # 1 row per thread, register slots left empty
                                         (200, 130, 300),       # 2 rows per thread, not full; one pick-buffer flush at 256
                                         (300, 400, 128)])      # 4 rows per thread, not full
@pytest.mark.parametrize("with_drops", [False, True])
def test_bit_exact_partly_filled_workgroup(dev, Na, Nb, n_out, with_drops):
    """Unions of up to 1024 rows that do not fill the workgroup's register slots: the arg-max with bounds tests."""
    a, b, T, start = _inputs(dev, 36 + Na, 2, Na, Nb, [Na + Nb - 1, 3])
    g = torch.Generator().manual_seed(37)
    drop_a = torch.stack([torch.randperm(Na, generator=g)[:10] for _ in range(2)]) if with_drops else None
    got = _run(dev, a, b, T, start, n_out, drop_a, None)
    want = _merge_ref.merge_resample(a, b, T, start, n_out, drop_a, None)
    assert torch.equal(got[1], want[1]) and torch.equal(got[0], want[0])


def test_bit_exact_largest_union(dev):
    a, b, T, start = _inputs(dev, 35, 1, 2048, 2048, [3000])
    got = _run(dev, a, b, T, start, 2048)
    want = _merge_ref.merge_resample(a, b, T, start, 2048)
    assert torch.equal(got[1], want[1]) and torch.equal(got[0], want[0])


def test_identity_pose_is_the_fps_kernel(dev, big):
    from puzzlenet_amd import ops
    a, b, start = big["a"], big["b"], big["start"]
    eye = torch.eye(4).repeat(3, 1, 1)
    out, src = _run(dev, a, b, eye, start, 1024)
    union = torch.cat((a, b), dim=1)
    want = ops.farthest_point_sample(union.to(dev), 1024, start.to(dev)).cpu()
    assert torch.equal(src, want)
    assert torch.equal(out, torch.gather(union, 1, want.unsqueeze(-1).expand(-1, -1, 3)))


def test_output_prefixes_are_its_own_fps_samples(dev, big):
    """The merged part comes out in pick order, so its first 512 points are its FPS-512 sample started at point 0 and the
    first 256 of those the FPS-256 sample of that (what ProgressiveAssembler's sampling plan relies on)."""
    from puzzlenet_amd import ops
    out = big["got"][0].to(dev)
    zeros = torch.zeros(3, dtype=torch.long, device=dev)
    f1 = ops.farthest_point_sample(out, 512, zeros).cpu()
    assert torch.equal(f1, torch.arange(512).expand(3, -1))
    f2 = ops.farthest_point_sample(out[:, :512].contiguous(), 256, zeros).cpu()
    assert torch.equal(f2, torch.arange(256).expand(3, -1))


def test_repeatable(dev, big):
    again = _run(dev, big["a"], big["b"], big["T"], big["start"], 1024)
    assert torch.equal(again[0], big["got"][0]) and torch.equal(again[1], big["got"][1])


def test_errors(dev, big):
    from puzzlenet_amd import _lib, ops
    a, b, T, start = (big[n] for n in ("a", "b", "T", "start"))
    with pytest.raises(_lib.PznError):
        ops.merge_resample(a, b, T, start)                                           # CPU tensors
    big_a = torch.zeros(1, 4096, 3, device=dev)
    one = torch.zeros(1, 1, 3, device=dev)
    eye, s0 = torch.eye(4, device=dev)[None], torch.zeros(1, dtype=torch.long, device=dev)
    with pytest.raises(_lib.PznUnsupported):
        ops.merge_resample(big_a, one, eye, s0, 16)                                   # a union of 4097 rows
    with pytest.raises(_lib.PznUnsupported):
        ops.merge_resample(one, one, eye, s0, 3)                                      # more picks than rows
    assert ops.merge_resample_supported(2048, 2048, 2048) and ops.merge_resample_supported(1, 1, 2)
    assert not ops.merge_resample_supported(2049, 2048, 16)
