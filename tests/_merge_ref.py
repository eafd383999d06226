"""CPU restatement of ops.merge_resample (csrc/mergefps.hip), in torch float32 elementwise operations whose order is the
kernel's pinned order, with the reference's farthest-point-sampling loop (the form of _fps_from in test_gpu_assembly.py)."""
import torch


def transform_rows(T, b):
    """x' = ((R00 x + R01 y) + R02 z) + t0 and likewise y', z': every product and sum is its own float32 torch op."""
    T = T.to(torch.float32)
    b = b.to(torch.float32)
    x, y, z = b[..., 0], b[..., 1], b[..., 2]
    rows = []
    for r in range(3):
        acc = T[r, 0] * x
        acc = acc + T[r, 1] * y
        acc = acc + T[r, 2] * z
        acc = acc + T[r, 3]
        rows.append(acc)
    return torch.stack(rows, dim=-1)


def merge_one(a, b, T, start, n_out, drop_a=None, drop_b=None):
    """One merge on the CPU: a[Na,3], b[Nb,3], T[4,4], start (union index) -> (points [n_out,3], src [n_out] int64)."""
    Na, Nb = a.shape[0], b.shape[0]
    U = Na + Nb
    union = torch.cat((a.to(torch.float32), transform_rows(T, b)), dim=0)
    distance = torch.ones(U) * 1e10
    dropped = torch.zeros(U, dtype=torch.bool)
    if drop_a is not None and len(drop_a):
        dropped[torch.as_tensor(drop_a, dtype=torch.long)] = True
    if drop_b is not None and len(drop_b):
        dropped[torch.as_tensor(drop_b, dtype=torch.long) + Na] = True
    distance[dropped] = 0.0      # a dropped row starts at 0; min keeps it there
    farthest = int(start)
    if bool(dropped[farthest]) and not bool(dropped.all()):      # the first kept row at or after the start, wrapping round
        order = (torch.arange(U) + farthest) % U
        farthest = int(order[~dropped[order]][0])
    src = torch.zeros(n_out, dtype=torch.long)
    for i in range(n_out):
        src[i] = farthest
        centroid = union[farthest].view(1, 3)
        dist = torch.sum((union - centroid) ** 2, -1)
        distance = torch.min(distance, dist)
        farthest = int(torch.max(distance, -1)[1])
    return union[src], src


def merge_resample(a, b, T, start, n_out=None, drop_a=None, drop_b=None):
    """The batch form, argument for argument ops.merge_resample on CPU tensors -> (points [M,n_out,3], src [M,n_out])."""
    M = a.shape[0]
    n_out = a.shape[1] if n_out is None else n_out
    outs = [merge_one(a[m], b[m], T[m], int(start[m]), n_out, None if drop_a is None else drop_a[m],
                      None if drop_b is None else drop_b[m]) for m in range(M)]
    return torch.stack([o[0] for o in outs]), torch.stack([o[1] for o in outs])
