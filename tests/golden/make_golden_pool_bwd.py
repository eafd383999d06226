#!/usr/bin/env python3
"""Backward of the per-point set-abstraction level at two small shapes (B = 2), recorded on a GPU.

    python tests/golden/make_golden_pool_bwd.py [OUT.npz]      ->  tests/golden/pool_bwd.npz

The inputs are regenerated from their seed (torch's CPU generator), so only the shapes, the seed and the outputs are stored:
the feature gradient (dP W1[:, 3:]), dW1[:, 0:3] and db1 (the walk by point of csrc/sapool.hip) and dW2, db2 (the weight-gradient
pass of csrc/poolbwd.hip).  EXACT ones are summed in a fixed order, so a build that keeps the kernels' summation orders
reproduces them bit for bit; dW1[:, 0:3] and db1 meet in one set of fp32 atomics per workgroup of the walk by point, so they
repeat only to summation-order noise (ATOL_REL of the largest entry).  The script runs the level twice and refuses to write
a fixture that does not repeat."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "pool_bwd.npz")

# (B, N, S, D, C1, C2): the first level's channel counts and the second level's
SHAPES = ((2, 256, 64, 64, 128, 128), (2, 128, 32, 128, 256, 256))
SEED = 71
EXACT = ("out", "dfeat", "dW2", "db2")
ATOL_REL = 5e-6


def close(a, b):
    return float((a.double() - b.double()).abs().max()) <= ATOL_REL * float(b.double().abs().max())


def level_case(shape, seed=SEED):
    """CPU inputs of one level.  The second layer's bias is shifted down so that about 45 % of the pooled channels are
    dead (ReLU off), as in a trained state."""
    B, N, S, D, C1, C2 = shape
    g = torch.Generator().manual_seed(seed + C1)
    xyz = torch.rand(B, N, 3, generator=g)
    feat = torch.randn(B, N, D, generator=g)
    w1 = torch.randn(C1, 3 + D, generator=g) / (3 + D) ** 0.5
    b1 = 0.1 * torch.randn(C1, generator=g)
    w2 = torch.randn(C2, C1, generator=g) / C1 ** 0.5
    b2 = 0.1 * torch.randn(C2, generator=g) - 1.1
    go = torch.randn(B, S, C2, generator=g)
    return xyz, feat, w1, b1, w2, b2, go


def level_grads(shape, dev, seed=SEED):
    """-> {name: CPU tensor}: the level's forward on given centroids, then its backward."""
    from puzzlenet_amd import ops
    B, N, S, D, C1, C2 = shape
    xyz, feat, w1, b1, w2, b2, go = level_case(shape, seed)
    xyz_d, new_xyz = xyz.to(dev), xyz[:, :S].contiguous().to(dev)
    idx = ops.knn(xyz_d, new_xyz, 32)
    f = feat.to(dev).requires_grad_(True)
    ps = [t.to(dev).requires_grad_(True) for t in (w1, b1, w2, b2)]
    assert ops.sa_level_fused_supported(f, idx, ps[0], ps[2])
    out = ops.sa_mlp_max(xyz_d, f, new_xyz, idx, *ps)
    (out * go.to(dev)).sum().backward()
    torch.cuda.synchronize()
    return {"out": out.detach().cpu(), "dfeat": f.grad.cpu(), "dW1xyz": ps[0].grad[:, :3].contiguous().cpu(),
            "db1": ps[1].grad.cpu(), "dW2": ps[2].grad.cpu(), "db2": ps[3].grad.cpu()}


def key(shape, name):
    return "c%d_%s" % (shape[4], name)


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else OUT
    dev = torch.device("cuda:0")
    rec = {"seed": np.int64(SEED), "shapes": np.array(SHAPES, dtype=np.int64)}
    for shape in SHAPES:
        a, b = level_grads(shape, dev), level_grads(shape, dev)
        for name in a:
            assert torch.equal(a[name], b[name]) if name in EXACT else close(a[name], b[name]), (shape, name)
            rec[key(shape, name)] = a[name].numpy()
        live = float((a["out"] > 0).float().mean())
        print(shape, "live channels %.3f" % live)
    np.savez_compressed(out_path, **rec)
    print(out_path, os.path.getsize(out_path), "bytes")


if __name__ == "__main__":
    main()
