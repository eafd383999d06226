"""The assembly score of a model as a mean over a batch of fractured puzzles, with one download at the end:

    python tools/eval_assembly.py [--batch 64] [--pieces 8] [--m 20000] [--k 128] [--candidates 16] [--mag 0.8] [--seed 0]
                                  [--curvature 2.0] [--ckpt model.ckpt] [--refine N] [--joint N] [--max-score S]

B seeded uniform clouds of M points are each cut into P pieces that belong together (datapipe.fracture, along curved surfaces
with principal curvatures up to --curvature, along planes with --curvature 0; every piece sampled to
the model's N points and moved by its own pose), then the chain of puzzlenet_amd.assembly runs on the whole batch on the device:
match_puzzles (every piece encoded once, the encoders on full batches; --refine N: every pair pose refined on its picked
boundaries by at most N ICP steps), assemble_batch (the greedy walk and the joint list of all puzzles, one launch), with --joint N
refine_assembly_batch (all placed poses of every puzzle refined together over every joint, at most N sweeps, one launch), and
evaluate_batch against the fracture's truth.  Nothing waits for the device until the metrics - a few numbers per puzzle - are
downloaded once.  Prints the means over the valid fractures: part accuracy, edge precision, and over the placed pieces other
than the root the rotation error in degrees, the translation error and the mean squared distance; with --joint both before and
after the joint refinement.  Without --ckpt the weights are the closed-form pseudo-random ones and the poses mean nothing.
Needs a GPU; there is no CPU path."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch


def metrics(ev, asm, ok):
    """One row of means (over the valid puzzles) on the device: part accuracy, edge precision (over the puzzles with an edge),
    rotation, translation, msd (over the placed pieces other than the root), the share of pieces placed."""
    P = ev.msd.shape[1]
    valid = ok.double()
    n = valid.sum()
    others = (torch.arange(P, device=ok.device)[None, :] != asm.root[:, None]) & ok[:, None]
    counted = (asm.placed & others).double()
    mean_pieces = lambda x: (x * counted).sum() / counted.sum()
    has_edge = ok & (asm.n_edges > 0)
    edge_precision = torch.where(has_edge, ev.edge_precision, torch.zeros_like(ev.edge_precision)).sum() / has_edge.double().sum()
    return torch.stack(((ev.part_accuracy * valid).sum() / n, edge_precision, mean_pieces(ev.rot_deg), mean_pieces(ev.trans),
                        mean_pieces(ev.msd), counted.sum() / others.double().sum()))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=64, help="B: clouds, one puzzle each")
    ap.add_argument("--pieces", type=int, default=8, help="P: pieces per puzzle (2 .. 16)")
    ap.add_argument("--m", type=int, default=20000, help="points of every synthetic cloud")
    ap.add_argument("--n", type=int, default=1024, help="points per piece (the model's)")
    ap.add_argument("--k", type=int, default=128, help="boundary points picked per piece and pair")
    ap.add_argument("--candidates", type=int, default=16, help="candidate surfaces per cut")
    ap.add_argument("--curvature", type=float, default=2.0,
                    help="largest principal curvature of a break surface (2.0: a sphere of radius 0.5; 0: planes)")
    ap.add_argument("--mag", type=float, default=0.8, help="magnitude of every piece's twist")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--ckpt", default=None, help="reference checkpoint (puzzlenet_amd.checkpoint); closed-form weights if absent")
    ap.add_argument("--refine", type=int, default=0, help="ICP steps at most per pair pose on the picked boundary points (0: none)")
    ap.add_argument("--joint", type=int, default=0, help="sweeps at most of the joint refinement after the walk (0: none)")
    ap.add_argument("--max-score", type=float, default=None, help="stop placing pieces above this boundary distance")
    args = ap.parse_args()
    if args.refine < 0 or args.joint < 0:
        sys.exit("--refine, --joint: 0 or a number of steps / sweeps")
    if not torch.cuda.is_available():
        sys.exit("tools/eval_assembly.py needs a GPU: puzzlenet_amd has no CPU path")
    from puzzlenet_amd import assembly, checkpoint, datapipe, model5_b
    dev = torch.device("cuda:0")
    B, P, M, N = args.batch, args.pieces, args.m, args.n
    if args.ckpt:
        model = checkpoint.build_from_reference_checkpoint(args.ckpt, num_points=N, device=dev)
        print(f"weights: {args.ckpt}")
    else:
        from oracle import model_ref
        model = model5_b.TouchedRegraster(model_ref.Cfg(num_points=N))
        model_ref.fill_params(model)
        model.to(dev)
        print("weights: no --ckpt given, closed-form pseudo-random weights (oracle.model_ref.fill_params): the poses mean nothing")
    model.fps_generator = torch.Generator().manual_seed(args.seed)

    rng = np.random.RandomState(args.seed)
    raw = (rng.rand(B, M, 3) - 0.5).astype(np.float32)
    if not 0.0 <= args.curvature < float("inf"):
        sys.exit(f"--curvature {args.curvature}: finite and >= 0")
    draws = datapipe.fracture_arguments(rng, torch.Generator().manual_seed(args.seed), B, P, args.candidates, args.mag, args.curvature)
    to = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    with torch.no_grad():
        f = datapipe.fracture(to(raw), n=N, k=args.k, cap=min(M, 32768), **{name: to(d) for name, d in draws.items()})
        table = assembly.match_puzzles(model, f.pieces, k=args.k, refine=args.refine)
        asm = assembly.assemble_batch(table.score, table.T, max_score=args.max_score)
        rows = [metrics(assembly.evaluate_batch(asm.G, asm.placed, f.pose, f.rest, asm.root, asm.edges, asm.n_edges, f.mates), asm, f.ok)]
        extra = torch.zeros(3, dtype=torch.float64, device=dev)
        if args.joint:
            jr = assembly.refine_assembly_batch(f.pieces, table, asm, sweeps=args.joint)
            rows.append(metrics(assembly.evaluate_batch(jr.G, asm.placed, f.pose, f.rest, asm.root, asm.edges, asm.n_edges, f.mates),
                                asm, f.ok))
            extra = torch.stack((jr.score0.double().mean(), jr.score.double().mean(), jr.sweeps_used.double().mean()))
        head = torch.stack((f.ok.double().sum(), asm.n_joints.double().mean(), asm.n_edges.double().mean()))
        host = torch.cat([head, extra] + rows).cpu().tolist()                       # the one download
    print(f"{B} clouds of {M} points into {P} pieces of {N}: {int(host[0])} valid fractures; per puzzle {host[2]:.2f} edges, "
          f"{host[1]:.1f} joints")
    names = ("part accuracy", "edge precision", "rotation (deg)", "translation", "msd", "share placed")
    for label, at in (("greedy walk", 6),) + ((("after the joint refinement", 12),) if args.joint else ()):
        print(f"{label}: " + ", ".join(f"{n} {v:.6g}" for n, v in zip(names, host[at:at + 6])))
    if args.joint:
        print(f"joint refinement: mean summed score {host[3]:.6f} -> {host[4]:.6f}, {host[5]:.1f} sweeps")


if __name__ == "__main__":
    main()
