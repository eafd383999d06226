"""GPU: ops.pair_head (csrc/pointmlp.hip, pair_head_fwd_kernel) - the fixed-side boundary head of an all-pairs table, one
launch for every (fixed piece, moved piece) pair - against float64 on the CPU."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _rel(a, b):
    a = a.detach().cpu().double()
    b = b.detach().cpu().double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _inputs(Kf, Km, N, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(Kf, N, 64, generator=g)
    gl = torch.randn(Km, 64, generator=g)
    W1, b1 = torch.randn(64, 128, generator=g) / 8, 0.1 * torch.randn(64, generator=g)
    W2, b2 = torch.randn(32, 64, generator=g) / 8, 0.1 * torch.randn(32, generator=g)
    W3, b3 = torch.randn(2, 32, generator=g) / 32 ** 0.5, 0.1 * torch.randn(2, generator=g)
    return x, gl, W1, b1, W2, b2, W3, b3


# a lone tile / rectangular and odd, fewer tiles than one workgroup's wavefronts / 33 tiles per piece: piece boundaries that
# no workgroup boundary meets / the benchmarked size (four moved pieces per work item) / a ragged last chunk of moved
# pieces (2, 2, 2, 1) / more tiles than wavefronts in the grid: the walk over several work items with the next rows in flight
@pytest.mark.parametrize("Kf,Km,N", [(1, 1, 32), (3, 5, 96), (2, 7, 1056), (16, 16, 1024), (16, 7, 1024), (65, 3, 1024)])
def test_pair_head_vs_float64(dev, Kf, Km, N):
    """y[i, j] = the MLPFpcb chain on cat([g_j.repeat(N, 1), x_i], -1), written out as F.linear chains in float64; the
    bound is the one tests/test_gpu_dense.py::test_point_mlp3_vs_float64 holds for the same chain."""
    from puzzlenet_amd import ops
    x, gl, W1, b1, W2, b2, W3, b3 = t = _inputs(Kf, Km, N, 100 + Kf + Km)
    xd, gd, W1d, b1d, W2d, b2d, W3d, b3d = (a.double() for a in t)
    xin = torch.cat([gd[None, :, None, :].expand(Kf, Km, N, 64), xd[:, None].expand(Kf, Km, N, 64)], dim=-1)
    ref = F.linear(F.relu(F.linear(F.relu(F.linear(xin, W1d, b1d)), W2d, b2d)), W3d, b3d)
    d = [a.to(dev) for a in t]
    y = ops.pair_head(*d)
    assert y.shape == (Kf, Km, N, 2)
    print(f"pair_head ({Kf}, {Km}, {N}): rel {_rel(y, ref):.3e}")
    assert _rel(y, ref) < 1e-5
    assert torch.equal(ops.pair_head(*d), y)


def test_pair_head_rejects_what_it_does_not_take(dev):
    from puzzlenet_amd import _lib, ops
    assert ops.pair_head_supported(1024, 32, 2) and not ops.pair_head_supported(40, 32, 2)
    assert not ops.pair_head_supported(1024, 64, 64)
    t = _inputs(2, 2, 40, 1)
    with pytest.raises(_lib.PznError):
        ops.pair_head(*(a.to(dev) for a in t))
    with pytest.raises(_lib.PznError):
        ops.pair_head(*_inputs(2, 2, 32, 1))      # CPU tensors
