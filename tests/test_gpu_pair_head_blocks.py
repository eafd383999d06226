"""GPU: ops.pair_head_blocks (csrc/pointmlp.hip, pair_head_fwd_kernel behind pzn_pair_head_blocks_fwd_f32) - the fixed-side
boundary head of Z pair tables in one launch, block-diagonal - against ops.pair_head on every puzzle's slices, bit for bit: the
arithmetic of a work item does not know which puzzle its tile belongs to, only which bias rows and output rows are its own.
ops.pair_head itself is held to float64 in tests/test_gpu_pair_head.py."""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _inputs(Z, Kf, Km, N, seed, dev):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(Z, Kf, N, 64, generator=g)
    gl = torch.randn(Z, Km, 64, generator=g)
    W1, b1 = torch.randn(64, 128, generator=g) / 8, 0.1 * torch.randn(64, generator=g)
    W2, b2 = torch.randn(32, 64, generator=g) / 8, 0.1 * torch.randn(32, generator=g)
    W3, b3 = torch.randn(2, 32, generator=g) / 32 ** 0.5, 0.1 * torch.randn(2, generator=g)
    return tuple(a.to(dev) for a in (x, gl, W1, b1, W2, b2, W3, b3))


# The launch has 2048 wavefront slots and splits the j range while the tiles of ALL puzzles are fewer: 12 tiles, every moved piece
# its own chunk / the row form / the column form (one moved piece: nothing to split) / 1024 tiles: chunks of 2 and 1 / 768 tiles
# and 7 moved pieces: chunks of 3, 3 and a ragged 1 / 2048 tiles: the j range is not split / 1040 puzzles of two one-tile pieces:
# 2080 items for 2048 wavefronts, so a wavefront's grid stride takes it from puzzle z to puzzle z + 1024
SHAPES = [(3, 2, 5, 64), (3, 1, 4, 64), (3, 4, 1, 64), (4, 8, 3, 1024), (3, 8, 7, 1024), (8, 8, 3, 1024), (1040, 2, 2, 32)]


@pytest.mark.parametrize("Z,Kf,Km,N", SHAPES)
def test_blocks_are_pair_head_per_puzzle(dev, Z, Kf, Km, N):
    from puzzlenet_amd import ops
    x, gl, *w = _inputs(Z, Kf, Km, N, 200 + Z + Kf + Km, dev)
    y = ops.pair_head_blocks(x, gl, *w)
    assert y.shape == (Z, Kf, Km, N, 2) and y.dtype == torch.float32
    # (the many-puzzle shape: both ends of the grid stride and a sample in between)
    for z in (range(Z) if Z <= 8 else (0, 1, 15, 16, 500, 1023, 1024, 1025, Z - 1)):
        assert torch.equal(y[z], ops.pair_head(x[z], gl[z], *w)), z
    assert torch.equal(ops.pair_head_blocks(x, gl, *w), y)                  # two runs, the same bits


def test_rejects_what_it_does_not_take(dev):
    from puzzlenet_amd import _lib, ops
    real, calls = ops._call, []

    def spy(name, *a, **k):
        calls.append(name)
        return real(name, *a, **k)
    ops._call = spy
    try:
        assert ops.pair_head_blocks_supported(1024, 32, 2) and not ops.pair_head_blocks_supported(40, 32, 2)
        assert not ops.pair_head_blocks_supported(1024, 64, 64)
        with pytest.raises(_lib.PznUnsupported):
            ops.pair_head_blocks(*_inputs(2, 2, 2, 40, 1, dev))             # N is no multiple of 32
        x, gl, W1, b1, W2, b2, W3, b3 = t = _inputs(2, 2, 3, 32, 2, dev)
        with pytest.raises(_lib.PznUnsupported):
            ops.pair_head_blocks(x, gl, W1, b1, torch.cat((W2, W2)), torch.cat((b2, b2)), torch.randn(64, 64, device=dev),
                                 torch.randn(64, device=dev))               # a 64 -> 64 -> 64 tail
        with pytest.raises(_lib.PznError):
            ops.pair_head_blocks(*(a.cpu() for a in t))
        with pytest.raises(_lib.PznError):
            ops.pair_head_blocks(x[0], gl, W1, b1, W2, b2, W3, b3)          # no leading Z
        with pytest.raises(_lib.PznError):
            ops.pair_head_blocks(x, gl[:1], W1, b1, W2, b2, W3, b3)         # the moved pieces of another number of puzzles
        with pytest.raises(_lib.PznError):
            ops.pair_head_blocks(x, gl, W1[:, :100], b1, W2, b2, W3, b3)
        assert calls == []                                                  # every refusal came before any launch
        empty = ops.pair_head_blocks(x[:0], gl[:0], W1, b1, W2, b2, W3, b3)
        assert empty.shape == (0, 2, 3, 32, 2) and calls == []              # Z = 0 launches nothing
    finally:
        ops._call = real
