"""Put K pieces together: the all-pairs table of puzzlenet_amd.assembly.match_pairs, the greedy walk of assemble(), the
assembled cloud.

    python tools/assemble.py --pieces pieces.npy [--ckpt model.ckpt] [--k 128] [--max-score S] [--out PREFIX] [--progressive]
                             [--refine N] [--keep F|auto] [--joint N] [--joint-keep F|table] [--joint-auto [LEAST]] [--gt PREFIX_gt.npz] [--beam B] [--branch C] [--vote-weight W] [--forest]

pieces.npy holds [K, N, 3] float32 (N = the model's points per piece).  Prints the score table and the edges in
placement order, writes PREFIX_G.npy ([K,4,4], each piece into the root's frame) and PREFIX_cloud.npy ([K,N,3]).
--progressive: assembly.assemble_progressive instead - after every placement the two parts are merged and resampled to N
points and matched again -; PREFIX_G.npy then maps each piece into the frame of the part that holds it, PREFIX_cloud.npy
is the [N,3] part around the first pair, PREFIX_piece_id.npy / PREFIX_row_id.npy say where each of its points came from.
--refine N: every pair pose is refined on its picked boundary points before it is used (assembly.refine_pairs: symmetric
point-to-point ICP, at most N accepted steps, one launch per table or per round); 0, the default, uses the network's poses.
--joint N: after the walk all placed poses are refined together over every joint - every pair of
placed pieces that scores no worse than the walk's worst edge - by at most N sweeps of assembly.refine_assembly (one launch);
PREFIX_G.npy and PREFIX_cloud.npy are then the refined ones, and with --gt the assembly is scored before and after.  With
--progressive the joints are read off the rows the merges left out (assembly.refine_progressive: two launches; every piece but
its part's frame piece moves; PREFIX_G.npy holds the refined poses, the merged cloud stays the walk's; not with --keep-matched,
--joint-keep or --joint-auto).  With
--keep auto every joint is refined over the rows its own pair kept (refine_assembly(..., kept="frozen"): a count per joint).
--joint-keep F|table (with --joint): the kept rows of every joint are chosen again under the joint poses, at every evaluation
(refine_assembly(..., keep=)): the share F of the full picked sets, or the counts the table carries (--keep F < 1 or auto).
--joint-auto [LEAST] (with --joint, exclusive with --joint-keep): the two counts of every joint are FOUND at every evaluation, under
the joint poses (refine_assembly(..., auto=AutoKeep(least=LEAST)), LEAST = 0.25 when left out); prints the mean count per joint.
--beam B (the table walk only, with --branch C and --vote-weight W): the beam walk of assembly.assemble_beam_batch in place of the
greedy one - B hypotheses, each extended by its C smallest entries, a child charged W times what the other placed pieces'
entries say against its pose -; everything after the walk is the same.
--forest (the table walk only): the pieces may be a pile of several objects - the forest walk of assembly.assemble_forest_batch in
place of the greedy one: where the walk stops (a score that is not finite or above --max-score), the pieces left over start a new
component from a new root, until every piece is in one.  Prints the components; PREFIX_G.npy maps each piece into the frame of its
own component's root, PREFIX_component.npy holds the component of every piece, and --joint N refines every component in one launch
(assembly.refine_assembly_batch).  Not with --gt, which holds the truth of one object.
--forest --beam B (with --branch C and --vote-weight W): the forest beam of assembly.assemble_forest_beam_batch in place of the
forest walk - the beam walk inside every component, a piece charged by the votes of the component it joins, a new component
charged --max-score -; everything after the walk is --forest's.
--gt PREFIX_gt.npz (written by tools/fracture.py beside the pieces): the assembly is scored against the truth - per piece the
rotation error in degrees, the translation error and the mean squared distance of its points from where they belong, the share
of pieces placed right (assembly.evaluate) and, for the greedy walk, the share of its edges between pieces that touch.  A truth
cut with tools/fracture.py --erosion says so: the share of the cloud lost along the breaks is printed, and the poses are scored
against the eroded pieces where they belong.
Needs a GPU; there is no CPU path."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch


def report(ev):
    """assembly.evaluate's fields, one line per piece."""
    for p in range(len(ev.msd)):
        print(f"  piece {p}: rot {ev.rot_deg[p]:9.4f} deg, trans {ev.trans[p]:.6f}, msd {ev.msd[p]:.3e}, "
              f"{'ok' if ev.part_ok[p] else 'NOT ok'}")
    print(f"part accuracy {ev.part_accuracy:.3f}" + ("" if ev.edge_precision is None else f", edge precision {ev.edge_precision:.3f}"))


def forest(args, x, table):
    """--forest: the forest walk over the table of a pile - with --beam the forest beam -, its components, and with --joint their
    refinement in one launch."""
    from puzzlenet_amd import assembly
    one = type(table)(*(f[None] for f in table))
    if args.beam:
        moment = assembly.boundary_moments(x[None], one.top_m)
        fb = assembly.assemble_forest_beam_batch(one.score, one.T, moment, beam=args.beam, branch=args.branch, weight=args.vote_weight,
                                                 max_score=args.max_score)
        print(f"forest beam: beam {args.beam}, branch {args.branch}, vote weight {args.vote_weight:g}; cost {float(fb.cost[0, 0]):.6f}")
    else:
        fb = assembly.assemble_forest_batch(one.score, one.T, max_score=args.max_score)
    G = fb.G[0]
    comp, n, nc = fb.component[0].tolist(), int(fb.n_edges[0]), int(fb.n_components[0])
    for (i, j, new), s in zip(fb.edges[0, :n].tolist(), fb.edge_score[0, :n].tolist()):
        print(f"  place piece {new} in component {comp[new]}: pair (fixed {i}, moved {j}), score {s:.6f}")
    for q, r in enumerate(fb.roots[0, :nc].tolist()):
        print(f"component {q}: root piece {r}, pieces {[p for p, c in enumerate(comp) if c == q]}")
    if args.joint:
        jr = assembly.refine_assembly_batch(x[None], one, fb, sweeps=args.joint, **joint_kw(args))
        G = jr.G[0].double()
        print(f"joint refinement over {int(fb.n_joints[0])} joints: summed score {float(jr.score0[0]):.6f} -> {float(jr.score[0]):.6f}, "
              f"{int(jr.sweeps_used[0])} sweeps, candidates taken per piece {jr.accepted[0].tolist()}"
              + (mean_counts(jr) if args.joint_auto is not None else ""))
    np.save(args.out + "_G.npy", G.cpu().numpy())
    np.save(args.out + "_component.npy", np.asarray(comp, dtype=np.int32))
    np.save(args.out + "_cloud.npy", assembly.apply(x, G).cpu().numpy())
    print(f"wrote {args.out}_G.npy, {args.out}_component.npy, {args.out}_cloud.npy (every component in its own root's frame)")


def joint_keep_arg(text):
    """--joint-keep: a share in (0, 1], or the word table (the counts the table carries)."""
    return "table" if text == "table" else float(text)


def joint_kw(args):
    """The keywords of the joint refinement: --joint-keep chooses the kept rows again under the joint poses (keep=); without it a
    table made with --keep auto is refined over the rows its pairs kept (kept="frozen")."""
    if args.joint_auto is not None:
        from puzzlenet_amd import assembly
        return {"auto": assembly.AutoKeep(least=args.joint_auto)}
    if args.joint_keep is not None:
        return {"keep": args.joint_keep}
    return {"kept": "frozen" if args.keep == "auto" else None}


def mean_counts(jr):
    """--joint-auto: the mean counts found per joint, over the used joint rows (an unused row holds 0) -> text."""
    live = jr.count_f > 0
    n = max(int(live.sum()), 1)
    return f", mean count per joint {float(jr.count_f[live].sum()) / n:.1f} fixed / {float(jr.count_m[live].sum()) / n:.1f} moved of {jr.kept_f.shape[-1]}"


def keep_arg(text):
    """--keep: a share in (0, 1], or the word auto (the share found per pair on the device)."""
    return "auto" if text == "auto" else float(text)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--pieces", required=True, help=".npy file with [K, N, 3] float32 pieces")
    ap.add_argument("--ckpt", default=None, help="reference checkpoint (puzzlenet_amd.checkpoint); closed-form weights if absent")
    ap.add_argument("--k", type=int, default=128, help="boundary points picked per piece and pair")
    ap.add_argument("--max-score", type=float, default=None, help="stop placing pieces above this boundary distance")
    ap.add_argument("--out", default="assembly", help="prefix of the two .npy files written")
    ap.add_argument("--seed", type=int, default=0, help="seed of the FPS start indices")
    ap.add_argument("--progressive", action="store_true", help="merge placed parts, resample and match again after every placement")
    ap.add_argument("--keep-matched", action="store_true", help="--progressive: keep the matched boundary points in the merged part")
    ap.add_argument("--refine", type=int, default=0, help="ICP steps at most per pair pose on the picked boundary points (0: none)")
    ap.add_argument("--keep", type=keep_arg, default=1.0, help="partial contact: the share of the picked boundary points of each side "
                    "that counts in a pair's score and refinement, those closest to the other side (1.0: all; not with --progressive), "
                    "or the word auto: the share is found per pair on the device (with --joint the kept sets are refined as the pair refinement left them: kept='frozen')")
    ap.add_argument("--joint", type=int, default=0, help="sweeps at most of the joint refinement after the walk (0: none)")
    ap.add_argument("--joint-keep", type=joint_keep_arg, default=None, help="with --joint: the kept rows of every joint are chosen again "
                    "under the joint poses - F: the share in (0, 1] of the picked boundary points of each side that counts, or the "
                    "word table: the counts the table carries (--keep F < 1 or auto); the full picked sets are read, not the table's kept rows")
    ap.add_argument("--joint-auto", type=float, nargs="?", const=0.25, default=None, metavar="LEAST", help="with --joint, exclusive with "
                    "--joint-keep: the two counts of every joint are found at every evaluation, under the joint poses (refine_assembly's "
                    "auto=AutoKeep(least=LEAST); LEAST: the least share in (0, 1] kept of each side, 0.25 when left out); prints the mean "
                    "count per joint beside the scores")
    ap.add_argument("--gt", default=None, help="PREFIX_gt.npz of tools/fracture.py: score the assembly against the truth")
    ap.add_argument("--beam", type=int, default=0, help="B: the beam walk with B hypotheses in place of the greedy walk (1 .. 8; 0: greedy)")
    ap.add_argument("--branch", type=int, default=4, help="C: with --beam, the candidates every hypothesis is extended by (1 .. 8)")
    ap.add_argument("--vote-weight", type=float, default=1.0, help="W: with --beam, the weight of the placed pieces' votes in a child's cost")
    ap.add_argument("--forest", action="store_true", help="a pile of several objects: the forest walk, a component per object")
    args = ap.parse_args()
    if args.forest and (args.progressive or args.gt):
        sys.exit("--forest: the table walk only (not with --progressive), and without --gt")
    if args.beam and (args.progressive or not (1 <= args.beam <= 8 and 1 <= args.branch <= 8) or args.vote_weight != args.vote_weight):
        sys.exit("--beam B, --branch C: 1 .. 8, --vote-weight: a number, and not with --progressive")
    if args.refine < 0:
        sys.exit("--refine: 0 or a number of steps")
    if (args.keep != "auto" and not 0.0 < args.keep <= 1.0) or (args.keep != 1.0 and args.progressive):
        sys.exit("--keep: a share in (0, 1] or the word auto, and 1.0 with --progressive (the progressive walk does not trim)")
    if args.joint < 0:
        sys.exit("--joint: 0 or a number of sweeps")
    if args.progressive and (args.joint_keep is not None or args.joint_auto is not None):
        sys.exit("--joint-keep, --joint-auto: options of the table walks; --progressive --joint N refines over the rows the merges "
                 "left out, chosen once (assembly.refine_progressive)")
    if args.progressive and args.joint and args.keep_matched:
        sys.exit("--progressive --joint N reads the joints off the rows the merges left out: not with --keep-matched")
    if args.joint_keep is not None and (not args.joint or (args.joint_keep != "table" and not 0.0 < args.joint_keep <= 1.0)
                                        or (args.joint_keep == "table" and args.keep == 1.0)):
        sys.exit("--joint-keep: with --joint N, a share in (0, 1] or the word table (which needs --keep F < 1 or auto)")
    if args.joint_auto is not None and (not args.joint or args.joint_keep is not None or not 0.0 < args.joint_auto <= 1.0):
        sys.exit("--joint-auto: with --joint N and without --joint-keep, a least share in (0, 1]")

    if not torch.cuda.is_available():
        sys.exit("tools/assemble.py needs a GPU: puzzlenet_amd has no CPU path")
    from puzzlenet_amd import assembly, checkpoint, model5_b
    dev = torch.device("cuda:0")
    pieces = np.load(args.pieces)
    if pieces.ndim != 3 or pieces.shape[2] != 3:
        sys.exit(f"{args.pieces}: expected [K, N, 3], got {pieces.shape}")
    K, N, _ = pieces.shape
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

    x = torch.from_numpy(np.ascontiguousarray(pieces, dtype=np.float32)).to(dev)
    gt = np.load(args.gt) if args.gt else None
    if gt is not None and gt["pose"].shape != (K, 4, 4):
        sys.exit(f"{args.gt}: the truth of {gt['pose'].shape[0]} pieces, {args.pieces} holds {K}")
    if gt is not None and "lost" in gt:
        print(f"{args.gt}: an eroded fracture, {100.0 * gt['lost'].sum() / gt['label'].shape[0]:.1f} % of the cloud lost along the "
              f"breaks, {int(gt['mates'].sum()) // 2} pairs of mates")
    if args.progressive:
        pa = assembly.ProgressiveAssembler(model, x, k=args.k, max_score=args.max_score, drop_matched=not args.keep_matched,
                                           generator=torch.Generator().manual_seed(args.seed), refine=args.refine)
        res = pa.run()
        for a, b, s, _da, _db in res.edges:
            print(f"  merge: part of piece {b} into part of piece {a}, score {s:.6f}")
        left = [k for k in range(K) if not res.placed[k]]
        if left:
            print(f"not in the part around the first pair: {left} ({res.parts.shape[0]} parts left)")
        def score_against_gt(G, when):
            if gt is not None and res.placed.any():
                part = next(q for q, mem in enumerate(pa.members) if int(np.flatnonzero(res.placed)[0]) in mem)
                root = pa.ledger.frame[part]
                print(f"against {args.gt} (the part around the first pair, in piece {root}'s frame){when}:")
                report(assembly.evaluate(G, res.placed, gt["pose"], gt["rest"], root))
        G = res.G
        if args.joint and res.edges:
            score_against_gt(G, ", before the joint refinement")
            jr = assembly.refine_progressive(x, res, sweeps=args.joint)
            G = jr.G.double().cpu().numpy()
            print(f"joint refinement over {int((jr.joints[:, 0] >= 0).sum())} joints: summed score {float(jr.score0):.6f} -> "
                  f"{float(jr.score):.6f}, {int(jr.sweeps_used)} sweeps, candidates taken per piece {jr.accepted.tolist()}")
        np.save(args.out + "_G.npy", G)
        for name, t in (("cloud", res.cloud), ("piece_id", res.piece_id), ("row_id", res.row_id)):
            np.save(f"{args.out}_{name}.npy", t.cpu().numpy())
        print(f"wrote {args.out}_G.npy, {args.out}_cloud.npy, {args.out}_piece_id.npy, {args.out}_row_id.npy")
        score_against_gt(G, ", after the joint refinement" if args.joint and res.edges else "")
        return
    table = assembly.match_pairs(model, x, k=args.k, refine=args.refine, keep=args.keep)
    if args.forest:
        return forest(args, x, table)
    if args.beam:
        moment = assembly.boundary_moments(x[None], table.top_m[None])
        b = assembly.assemble_beam_batch(table.score[None], table.T[None], moment, beam=args.beam, branch=args.branch,
                                         weight=args.vote_weight, max_score=args.max_score)
        n = int(b.n_edges[0])
        edges = [(i, j, s, new) for (i, j, new), s in zip(b.edges[0, :n].tolist(), b.edge_score[0, :n].tolist())]
        result = assembly.Assembly(int(b.root[0]), edges, b.G[0].cpu().numpy(), b.placed[0].cpu().numpy())
        print(f"beam walk: beam {args.beam}, branch {args.branch}, vote weight {args.vote_weight:g}; cost {float(b.cost[0, 0]):.6f}")
    else:
        result = assembly.assemble(table.score, table.T, max_score=args.max_score)

    score = table.score.cpu().numpy()
    print(f"score[fixed i, moved j] ({K} pieces of {N} points, k = {args.k}):")
    with np.printoptions(precision=5, suppress=True, linewidth=200):
        print(score)
    print(f"root: piece {result.root}")
    for i, j, s, new in result.edges:
        print(f"  place piece {new}: pair (fixed {i}, moved {j}), score {s:.6f}")
    left = [k for k in range(K) if not result.placed[k]]
    if left:
        print(f"not placed: {left}")
    G = result.G
    if args.joint:
        if gt is not None:
            print(f"against {args.gt} (in the root's frame), before the joint refinement:")
            report(assembly.evaluate(G, result.placed, gt["pose"], gt["rest"], result.root, result.edges, gt["mates"]))
        jr = assembly.refine_assembly(x, table, result, sweeps=args.joint, **joint_kw(args))
        G = jr.G.double().cpu().numpy()
        print(f"joint refinement over {len(jr.joints)} joints: summed score {float(jr.score0):.6f} -> {float(jr.score):.6f}, "
              f"{int(jr.sweeps_used)} sweeps, candidates taken per piece {jr.accepted.tolist()}"
              + (mean_counts(jr) if args.joint_auto is not None else ""))
    np.save(args.out + "_G.npy", G)
    np.save(args.out + "_cloud.npy", assembly.apply(x, G).cpu().numpy())
    print(f"wrote {args.out}_G.npy, {args.out}_cloud.npy")
    if gt is not None:
        print(f"against {args.gt} (in the root's frame){', after the joint refinement' if args.joint else ''}:")
        report(assembly.evaluate(G, result.placed, gt["pose"], gt["rest"], result.root, result.edges, gt["mates"]))


if __name__ == "__main__":
    main()
