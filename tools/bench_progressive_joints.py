"""Time the joint refinement of finished progressive parts beside the walk that built them.

    python tools/bench_progressive_joints.py [--batch 64] [--pieces 8] [--n 1024] [--k 128] [--sweeps 30] [--out FILE]

Z fractured puzzles (tools/eval_assembly.py's inputs: synthetic clouds cut by datapipe.fracture, closed-form weights - the poses
mean nothing, the launches and their sizes are the real ones) go through assembly.assemble_progressive_batch; on its ledger one
ops.progressive_joints launch and the whole assembly.refine_progressive_batch call are timed with device events, the median of
--repeats after --warmup calls, and the walk itself the same way over --walk-repeats.  Prints the three times, the joints found
and the library launches of one refine_progressive_batch call.  Needs a GPU; there is no CPU path."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch


def timed(fn, warmup, repeats):
    """-> the milliseconds of `repeats` calls of fn between device events, after `warmup` calls."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--pieces", type=int, default=8)
    ap.add_argument("--m", type=int, default=20000, help="points of every synthetic cloud")
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--k", type=int, default=128)
    ap.add_argument("--sweeps", type=int, default=30)
    ap.add_argument("--least", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--walk-repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/bench_progressive_joints.py needs a GPU: puzzlenet_amd has no CPU path")
    from oracle import model_ref
    from puzzlenet_amd import assembly, datapipe, model5_b, ops
    dev = torch.device("cuda:0")
    B, P, N = args.batch, args.pieces, args.n
    model = model5_b.TouchedRegraster(model_ref.Cfg(num_points=N))
    model_ref.fill_params(model)
    model.to(dev)
    rng = np.random.RandomState(args.seed)
    raw = (rng.rand(B, args.m, 3) - 0.5).astype(np.float32)
    draws = datapipe.fracture_arguments(rng, torch.Generator().manual_seed(args.seed), B, P, 16, 0.8, 2.0)
    to = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    with torch.no_grad():
        f = datapipe.fracture(to(raw), n=N, k=args.k, cap=min(args.m, 32768), **{name: to(d) for name, d in draws.items()})
        s1, s2 = (s.view(B, P) for s in model5_b.draw_fps_starts(1, B * P, N, torch.Generator().manual_seed(args.seed)))
        walk = lambda: assembly.assemble_progressive_batch(model, f.pieces, k=args.k, start=(s1, s2),
                                                           generator=torch.Generator().manual_seed(args.seed))
        t_walk = timed(walk, 1, args.walk_repeats)
        pr = walk()
        t_joints = timed(lambda: ops.progressive_joints(f.pieces, pr.G, pr.dropped, args.least), args.warmup, args.repeats)
        t_refine = timed(lambda: assembly.refine_progressive_batch(f.pieces, pr, args.sweeps, args.least), args.warmup, args.repeats)
        calls = []
        real = ops._call
        ops._call = lambda name, *a, **k: (calls.append(name), real(name, *a, **k))[1]
        try:
            jr = assembly.refine_progressive_batch(f.pieces, pr, args.sweeps, args.least)
        finally:
            ops._call = real
        used = (jr.joints[..., 0] >= 0)
        host = torch.stack((used.double().sum(dim=1).mean(), pr.n_edges.double().mean(), jr.count_f[used].double().mean(),
                            jr.count_m[used].double().mean(), jr.score0.double().mean(), jr.score.double().mean(),
                            jr.sweeps_used.double().mean())).cpu().tolist()
    med = statistics.median
    span = lambda t: f"median {med(t):.3f} ms of {len(t)} ({min(t):.3f} .. {max(t):.3f})"
    lines = [
        f"{B} fractured puzzles of {P} pieces of {N} points, k = {args.k}, closed-form weights; device events on {torch.cuda.get_device_name(0)}",
        f"assemble_progressive_batch ({P - 1} lockstep rounds, construction included): {span(t_walk)}",
        f"ops.progressive_joints (one launch, grid {pr.dropped.shape[0]} x {B}, its seven outputs allocated and filled): {span(t_joints)}",
        f"refine_progressive_batch ({args.sweeps} sweeps at most, least = {args.least}): {span(t_refine)}",
        f"library launches of one refine_progressive_batch call: {calls}",
        f"per puzzle {host[1]:.2f} edges and {host[0]:.2f} joints of {P * (P - 1) // 2} slots, mean set {host[2]:.1f} fixed / "
        f"{host[3]:.1f} moved rows of {args.k}; mean summed score {host[4]:.6f} -> {host[5]:.6f}, {host[6]:.1f} sweeps",
        f"the two launches are {100 * med(t_refine) / med(t_walk):.2f} % of the walk's time",
    ]
    print("\n".join(lines))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
