"""The assembly score of a model as a mean over a batch of fractured puzzles, with one download at the end:

    python tools/eval_assembly.py [--batch 64] [--pieces 8] [--m 20000] [--k 128] [--candidates 16] [--mag 0.8] [--seed 0]
                                  [--curvature 2.0] [--erosion E [--chip DEPTH RADIUS]] [--ckpt model.ckpt] [--refine N] [--keep F|auto] [--joint N] [--joint-keep F|table] [--joint-auto [LEAST]] [--max-score S]
                                  [--progressive] [--time R] [--json out.json] [--beam B] [--branch C] [--vote-weight W]
                                  [--objects Q]

B seeded uniform clouds of M points are each cut into P pieces that belong together (datapipe.fracture, along curved surfaces
with principal curvatures up to --curvature, along planes with --curvature 0; with --erosion E [--chip DEPTH RADIUS] material is
lost along every break, a band of up to E on either side and a chip of up to DEPTH within RADIUS of the anchor
(datapipe.fracture(..., erode=)), so the pieces no longer mate perfectly, and the lost share is printed; every piece sampled to
the model's N points and moved by its own pose), then the chain of puzzlenet_amd.assembly runs on the whole batch on the device:
match_puzzles (every piece encoded once, the encoders on full batches; --refine N: every pair pose refined on its picked
boundaries by at most N ICP steps), assemble_batch (the greedy walk and the joint list of all puzzles, one launch), with --joint N
refine_assembly_batch (all placed poses of every puzzle refined together over every joint, at most N sweeps, one launch), and
evaluate_batch against the fracture's truth.  Nothing waits for the device until the metrics - a few numbers per puzzle - are
downloaded once.  --beam B (with --branch C, --vote-weight W) also runs the beam walk scored by the placed pieces' votes
(boundary_moments and assemble_beam_batch, one launch) on the same table and prints its means beside the greedy walk's, with
--joint both before and after the joint refinement of its own result.  Prints the means over the valid fractures: part accuracy, edge precision, and over the placed pieces other
than the root the rotation error in degrees, the translation error and the mean squared distance; with --joint both before and
after the joint refinement; --joint-keep F|table has that refinement choose the kept rows of every joint again under the joint
poses (refine_assembly_batch(..., keep=): the share F of the full picked sets, or the counts the table carries); --joint-auto
[LEAST] (exclusive with --joint-keep) has it FIND the two counts of every joint at every evaluation, under the joint poses
(refine_assembly_batch(..., auto=AutoKeep(least=LEAST)), LEAST = 0.25 when left out) and prints the mean count per joint.  --progressive reports the same means for the progressive walk (assemble_progressive_batch: all
puzzles in lockstep, P - 1 rounds, every round one choice launch, one merge launch, one encoder batch and two blocked pair blocks)
beside the greedy one, on the same fractures and table starts, still with the one download; with --joint N a second progressive
row follows, after refine_progressive_batch (the joints read off the rows the merges left out, two launches; --joint-keep and
--joint-auto stay options of the table walks and do not reach it).  --time R (with --progressive) then
times the batched progressive walk and, beside it, a loop of assemble_progressive over the same puzzles - the per-puzzle path, which
downloads its table every round - R times each in turn after one warm-up of each, a host clock around work that ends in a device
synchronise, and counts the library launches of one round; --json writes those numbers to a file.  Without --ckpt the weights are the closed-form pseudo-random ones and the poses mean nothing.
--objects Q sorts mixed piles in place of puzzles: the B fractures are regrouped into B / Q piles of the Q P pieces of Q objects each
under a seeded shuffle (datapipe.pile), matched as one puzzle of Q P pieces, walked by the forest walk (assemble_forest_batch, one
launch; --max-score is the boundary distance above which two pieces do not belong together), with --joint refined component by
component in the same one launch, and scored by evaluate_pile_batch: pair precision, pair recall and pair pose recall over the
ordered pairs of pieces, the number of components and the share of piles sorted exactly, as means over the valid piles.
--objects Q --beam B (with --branch C, --vote-weight W) also runs the forest beam (boundary_moments and assemble_forest_beam_batch,
one launch: the beam walk with the forest walk's restarts, a restart charged --max-score) on the same tables and prints its row
beside the forest walk's, with --joint both rows after the joint refinement of their own results too.
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


def sort_piles(args, model, f, dev):
    """--objects Q: the forest walk over piles of Q fractures each - with --beam B the forest beam beside it, on the same tables -
    and the pile metrics as means over the valid piles."""
    from puzzlenet_amd import assembly, datapipe
    B, P, Q = f.pose.shape[0], f.pose.shape[1], args.objects
    Z, K = B // Q, Q * P
    g = torch.Generator().manual_seed(args.seed)
    perm = torch.stack([torch.randperm(K, generator=g) for _ in range(Z)]).to(dev)
    pile = datapipe.pile(f, objects=Q, perm=perm)
    table = assembly.match_puzzles(model, pile.pieces, k=args.k, refine=args.refine, keep=args.keep)
    forest = assembly.assemble_forest_batch(table.score, table.T, max_score=args.max_score)
    walks = [("forest walk", forest)]
    if args.beam:
        moment = assembly.boundary_moments(pile.pieces, table.top_m)
        walks.append((f"forest beam (beam {args.beam}, branch {args.branch}, vote weight {args.vote_weight:g})",
                      assembly.assemble_forest_beam_batch(table.score, table.T, moment, beam=args.beam, branch=args.branch,
                                                          weight=args.vote_weight, max_score=args.max_score)))
    valid = pile.ok.double()

    def row(G, asm):
        ev = assembly.evaluate_pile_batch(G, asm.component, pile.pose, pile.rest, pile.object_of)
        mean = lambda x: torch.nansum(x.double() * valid) / (valid * ~torch.isnan(x.double())).sum()
        return torch.stack([mean(x) for x in (ev.pair_precision, ev.pair_recall, ev.pair_pose_recall, ev.n_components, ev.exact)])

    labels, rows, heads, counts = [], [], [valid.sum()[None]], []
    for label, asm in walks:
        labels.append(label)
        rows.append(row(asm.G, asm))
        extra = torch.zeros(3, dtype=torch.float64, device=dev)
        if args.joint:
            jr = assembly.refine_assembly_batch(pile.pieces, table, asm, sweeps=args.joint, **joint_kw(args))
            labels.append(f"{label.split(' (')[0]} after the joint refinement")
            rows.append(row(jr.G, asm))
            extra = torch.stack((jr.score0.double().mean(), jr.score.double().mean(), jr.sweeps_used.double().mean()))
            if args.joint_auto is not None:
                counts.append(mean_counts(jr))
        heads.append(torch.cat((torch.stack((asm.n_joints.double().mean(), asm.n_edges.double().mean())), extra)))
    if args.beam:
        heads.append((walks[1][1].edges == forest.edges).all(dim=2).all(dim=1).double().mean()[None])
    host = torch.cat(heads + rows + counts).cpu().tolist()                          # the one download (the mean counts at its end)
    print(f"{Z} piles of {Q} objects, {K} pieces of {f.pieces.shape[2]} points each: {int(host[0])} valid piles")
    at = 1 + 5 * len(walks) + (1 if args.beam else 0)
    names = ("pair precision", "pair recall", "pair pose recall", "components", "share sorted exactly")
    for n, label in enumerate(labels):
        print(f"{label}: " + ", ".join(f"{name} {v:.6g}" for name, v in zip(names, host[at + 5 * n:at + 5 * n + 5])))
    for n, (label, _) in enumerate(walks):
        h = host[1 + 5 * n:6 + 5 * n]
        print(f"{label.split(' (')[0]}: per pile {h[1]:.2f} edges, {h[0]:.1f} joints"
              + (f"; joint refinement: mean summed score {h[2]:.6f} -> {h[3]:.6f}, {h[4]:.1f} sweeps" if args.joint else "")
              + (f", mean count per joint {host[len(host) - 2 * len(walks) + 2 * n]:.1f} fixed / "
                 f"{host[len(host) - 2 * len(walks) + 2 * n + 1]:.1f} moved of {args.k}" if counts else ""))
    if args.beam:
        print(f"forest beam: the forest walk's edges in {100 * host[at - 1]:.1f} % of the piles")


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
    """--joint-auto: the mean counts found per joint over the used joint rows (an unused row holds 0), on the device -> [2]."""
    live = (jr.count_f > 0).double()
    return torch.stack(((jr.count_f.double() * live).sum(), (jr.count_m.double() * live).sum())) / live.sum().clamp(min=1.0)


def keep_arg(text):
    """--keep: a share in (0, 1], or the word auto (the share found per pair on the device)."""
    return "auto" if text == "auto" else float(text)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=64, help="B: clouds, one puzzle each")
    ap.add_argument("--pieces", type=int, default=8, help="P: pieces per puzzle (2 .. 16)")
    ap.add_argument("--m", type=int, default=20000, help="points of every synthetic cloud")
    ap.add_argument("--n", type=int, default=1024, help="points per piece (the model's)")
    ap.add_argument("--k", type=int, default=128, help="boundary points picked per piece and pair")
    ap.add_argument("--candidates", type=int, default=16, help="candidate surfaces per cut")
    ap.add_argument("--erosion", type=float, default=0.0, help="widest band lost on either side of a break (0: nothing is lost)")
    ap.add_argument("--chip", type=float, nargs=2, default=(0.0, 0.0), metavar=("DEPTH", "RADIUS"),
                    help="deepest and widest chip lost around the point a break goes through")
    ap.add_argument("--curvature", type=float, default=2.0,
                    help="largest principal curvature of a break surface (2.0: a sphere of radius 0.5; 0: planes)")
    ap.add_argument("--mag", type=float, default=0.8, help="magnitude of every piece's twist")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--ckpt", default=None, help="reference checkpoint (puzzlenet_amd.checkpoint); closed-form weights if absent")
    ap.add_argument("--refine", type=int, default=0, help="ICP steps at most per pair pose on the picked boundary points (0: none)")
    ap.add_argument("--keep", type=keep_arg, default=1.0, help="partial contact: the share of the picked boundary points of each side "
                    "that counts in a pair's score and refinement, those closest to the other side (1.0: all; the progressive "
                    "walks do not trim), or the word auto: the share is found per pair on the device (with --joint the kept sets are refined as the pair refinement left them: kept='frozen')")
    ap.add_argument("--joint", type=int, default=0, help="sweeps at most of the joint refinement after the walk (0: none)")
    ap.add_argument("--joint-keep", type=joint_keep_arg, default=None, help="with --joint: the kept rows of every joint are chosen again "
                    "under the joint poses - F: the share in (0, 1] of the picked boundary points of each side that counts, or the "
                    "word table: the counts the table carries (--keep F < 1 or auto); the full picked sets are read, not the table's kept rows")
    ap.add_argument("--joint-auto", type=float, nargs="?", const=0.25, default=None, metavar="LEAST", help="with --joint, exclusive with "
                    "--joint-keep: the two counts of every joint are found at every evaluation, under the joint poses "
                    "(refine_assembly_batch's auto=AutoKeep(least=LEAST); LEAST: the least share in (0, 1] kept of each side, 0.25 when "
                    "left out); prints the mean count per joint beside the scores")
    ap.add_argument("--max-score", type=float, default=None, help="stop placing pieces above this boundary distance")
    ap.add_argument("--progressive", action="store_true", help="also the progressive walk of the whole batch, in lockstep")
    ap.add_argument("--time", type=int, default=0, help="with --progressive: repeats of the timed batched walk and per-puzzle loop")
    ap.add_argument("--json", default=None, help="with --time: write the timings and launch counts to this file")
    ap.add_argument("--beam", type=int, default=0, help="B: also the beam walk with B hypotheses - with --objects, the forest beam (1 .. 8; 0: the greedy walk alone)")
    ap.add_argument("--branch", type=int, default=4, help="C: with --beam, the candidates every hypothesis is extended by (1 .. 8)")
    ap.add_argument("--vote-weight", type=float, default=1.0, help="W: with --beam, the weight of the placed pieces' votes in a child's cost")
    ap.add_argument("--objects", type=int, default=1,
                    help="Q: sort piles of the pieces of Q objects each with the forest walk (Q divides --batch, Q P <= 64; 1: puzzles)")
    args = ap.parse_args()
    if args.objects < 1 or args.batch % args.objects or args.objects * args.pieces > 64:
        sys.exit("--objects Q: Q >= 1 divides --batch, and Q * --pieces <= 64")
    if args.objects > 1 and args.progressive:
        sys.exit("--objects goes with the forest walk alone: no --progressive")
    if args.refine < 0 or args.joint < 0:
        sys.exit("--refine, --joint: 0 or a number of steps / sweeps")
    if args.joint_keep is not None and (not args.joint or (args.joint_keep != "table" and not 0.0 < args.joint_keep <= 1.0)
                                        or (args.joint_keep == "table" and args.keep == 1.0)):
        sys.exit("--joint-keep: with --joint N, a share in (0, 1] or the word table (which needs --keep F < 1 or auto)")
    if args.joint_auto is not None and (not args.joint or args.joint_keep is not None or not 0.0 < args.joint_auto <= 1.0):
        sys.exit("--joint-auto: with --joint N and without --joint-keep, a least share in (0, 1]")
    if args.keep != "auto" and not 0.0 < args.keep <= 1.0:
        sys.exit("--keep: a share in (0, 1] or the word auto")
    if args.time < 0 or (args.time and not args.progressive) or (args.json and not args.time):
        sys.exit("--time R >= 0 goes with --progressive, --json with --time")
    if args.beam and not (1 <= args.beam <= 8 and 1 <= args.branch <= 8 and args.vote_weight == args.vote_weight):
        sys.exit("--beam B, --branch C: 1 .. 8; --vote-weight: a number")
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
    try:
        draws = datapipe.fracture_arguments(rng, torch.Generator().manual_seed(args.seed), B, P, args.candidates, args.mag,
                                            args.curvature, args.erosion, tuple(args.chip))
    except datapipe._lib.PznError as e:
        sys.exit(f"--erosion {args.erosion} --chip {args.chip[0]} {args.chip[1]}: {e}")
    to = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    with torch.no_grad():
        f = datapipe.fracture(to(raw), n=N, k=args.k, cap=min(M, 32768), **{name: to(d) for name, d in draws.items()})
        if "erode" in draws:
            print(f"erosion {args.erosion}, chip {tuple(args.chip)}: {100.0 * float(f.lost.sum()) / (B * M):.1f} % of the points lost along "
                  f"the breaks, {float(f.mates.sum()) / 2 / B:.1f} mates per puzzle")
        if args.objects > 1:
            return sort_piles(args, model, f, dev)
        # the FPS starts of the table, drawn as match_puzzles draws them, so that the progressive walk can start from the same ones
        s1, s2 = (s.view(B, P) for s in model5_b.draw_fps_starts(1, B * P, N, model.fps_generator))
        table = assembly.match_puzzles(model, f.pieces, k=args.k, start=(s1, s2), refine=args.refine, keep=args.keep)
        asm = assembly.assemble_batch(table.score, table.T, max_score=args.max_score)
        rows = [metrics(assembly.evaluate_batch(asm.G, asm.placed, f.pose, f.rest, asm.root, asm.edges, asm.n_edges, f.mates), asm, f.ok)]
        extra = torch.zeros(3, dtype=torch.float64, device=dev)
        counts = []
        if args.joint:
            jr = assembly.refine_assembly_batch(f.pieces, table, asm, sweeps=args.joint, **joint_kw(args))
            if args.joint_auto is not None:
                counts.append(mean_counts(jr))
            rows.append(metrics(assembly.evaluate_batch(jr.G, asm.placed, f.pose, f.rest, asm.root, asm.edges, asm.n_edges, f.mates),
                                asm, f.ok))
            extra = torch.stack((jr.score0.double().mean(), jr.score.double().mean(), jr.sweeps_used.double().mean()))
        if args.progressive:
            walk = lambda: assembly.assemble_progressive_batch(model, f.pieces, k=args.k, start=(s1, s2), max_score=args.max_score,
                                                               generator=torch.Generator().manual_seed(args.seed), refine=args.refine)
            pr = walk()
            rows.append(metrics(assembly.evaluate_batch(pr.G, pr.placed, f.pose, f.rest, pr.root, pr.edges, pr.n_edges, f.mates), pr, f.ok))
            rows.append(torch.stack((pr.n_edges.double().mean(),)))
            if args.joint:
                pj = assembly.refine_progressive_batch(f.pieces, pr, sweeps=args.joint)
                rows.append(metrics(assembly.evaluate_batch(pj.G, pr.placed, f.pose, f.rest, pr.root, pr.edges, pr.n_edges, f.mates),
                                    pr, f.ok))
                rows.append(torch.stack((pj.score0.double().mean(), pj.score.double().mean(), pj.sweeps_used.double().mean())))
        if args.beam:
            moment = assembly.boundary_moments(f.pieces, table.top_m)
            bm = assembly.assemble_beam_batch(table.score, table.T, moment, beam=args.beam, branch=args.branch, weight=args.vote_weight,
                                              max_score=args.max_score)
            rows.append(metrics(assembly.evaluate_batch(bm.G, bm.placed, f.pose, f.rest, bm.root, bm.edges, bm.n_edges, f.mates), bm, f.ok))
            if args.joint:
                bj = assembly.refine_assembly_batch(f.pieces, table, bm, sweeps=args.joint, **joint_kw(args))
                rows.append(metrics(assembly.evaluate_batch(bj.G, bm.placed, f.pose, f.rest, bm.root, bm.edges, bm.n_edges, f.mates),
                                    bm, f.ok))
            same = (bm.edges == asm.edges).all(dim=2).all(dim=1).double().mean()
            rows.append(torch.stack((bm.n_edges.double().mean(), same)))
        head = torch.stack((f.ok.double().sum(), asm.n_joints.double().mean(), asm.n_edges.double().mean()))
        host = torch.cat([head, extra] + rows + counts).cpu().tolist()              # the one download (the mean counts at its end)
    print(f"{B} clouds of {M} points into {P} pieces of {N}: {int(host[0])} valid fractures; per puzzle {host[2]:.2f} edges, "
          f"{host[1]:.1f} joints")
    names = ("part accuracy", "edge precision", "rotation (deg)", "translation", "msd", "share placed")
    at_p = 18 if args.joint else 12
    at_b = at_p + ((16 if args.joint else 7) if args.progressive else 0)
    beam_label = f"beam walk (beam {args.beam}, branch {args.branch}, vote weight {args.vote_weight:g})"
    for label, at in (("greedy walk", 6),) + ((("after the joint refinement", 12),) if args.joint else ()) \
            + ((("progressive walk", at_p),) if args.progressive else ()) \
            + ((("progressive walk after the joint refinement", at_p + 7),) if args.progressive and args.joint else ()) \
            + (((beam_label, at_b),) if args.beam else ()) \
            + ((("beam walk after the joint refinement", at_b + 6),) if args.beam and args.joint else ()):
        print(f"{label}: " + ", ".join(f"{n} {v:.6g}" for n, v in zip(names, host[at:at + 6])))
    if args.joint:
        print(f"joint refinement: mean summed score {host[3]:.6f} -> {host[4]:.6f}, {host[5]:.1f} sweeps"
              + (f", mean count per joint {host[-2]:.1f} fixed / {host[-1]:.1f} moved of {args.k}" if counts else ""))
    if args.progressive:
        print(f"progressive walk: per puzzle {host[at_p + 6]:.2f} edges in {P - 1} lockstep rounds")
        if args.joint:
            print(f"progressive walk, joint refinement over the rows the merges left out: mean summed score {host[at_p + 13]:.6f} -> "
                  f"{host[at_p + 14]:.6f}, {host[at_p + 15]:.1f} sweeps"
                  + (" (--joint-keep / --joint-auto are options of the table walks: the progressive sets are chosen once)"
                     if args.joint_keep is not None or args.joint_auto is not None else ""))
    if args.beam:
        at = at_b + (12 if args.joint else 6)
        print(f"beam walk: per puzzle {host[at]:.2f} edges; the greedy walk's tree in {100 * host[at + 1]:.1f} % of the puzzles")
    if args.time:
        time_progressive(args, model, f, (s1, s2), walk)


def time_progressive(args, model, f, start, walk):
    """The batched progressive walk against a loop of assemble_progressive over the same puzzles, in turn, and the library launches
    of one round of each."""
    import json
    import statistics
    import time
    from puzzlenet_amd import assembly, ops
    B, P = f.pieces.shape[0], f.pieces.shape[1]
    s1, s2 = start

    def loop():
        g = torch.Generator().manual_seed(args.seed)
        return [assembly.assemble_progressive(model, f.pieces[z], k=args.k, start=(s1[z], s2[z]), max_score=args.max_score, generator=g,
                                              refine=args.refine) for z in range(B)]

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def launches(fn):
        real, calls = ops._call, []

        def spy(name, *a, **k):
            calls.append(name)
            return real(name, *a, **k)
        ops._call = spy
        try:
            fn()
        finally:
            ops._call = real
        return len(calls)

    with torch.no_grad():
        clock(walk), clock(loop)                                                  # warm-up: every shape of both paths
        ms = {"batched": [], "loop": []}
        for _ in range(args.time):
            ms["batched"].append(clock(walk))
            ms["loop"].append(clock(loop))
        pb = assembly.ProgressiveBatch(model, f.pieces, k=args.k, start=start, max_score=args.max_score, refine=args.refine)
        one = assembly.ProgressiveAssembler(model, f.pieces[0], k=args.k, start=(s1[0], s2[0]), max_score=args.max_score,
                                            refine=args.refine)
        n_round, n_one = launches(pb.step), launches(one.step)
    out = {"puzzles": B, "pieces": P, "points": f.pieces.shape[2], "k": args.k, "refine": args.refine, "repeats": args.time,
           "batched_ms": ms["batched"], "loop_ms": ms["loop"],
           "batched_ms_median": statistics.median(ms["batched"]), "loop_ms_median": statistics.median(ms["loop"]),
           "rounds_batched": P - 1, "rounds_loop_at_most": B * (P - 1),
           "library_launches_per_round_batched": n_round, "library_launches_per_round_one_puzzle": n_one,
           "what": "wall time (host clock, device synchronised) of assemble_progressive_batch over all puzzles, construction included, "
                   "and of a loop of assemble_progressive over the same puzzles in the same process, alternating, after one warm-up each"}
    print(f"batched progressive walk: median {out['batched_ms_median']:.1f} ms of {args.time} ({min(ms['batched']):.1f} .. "
          f"{max(ms['batched']):.1f}); loop of assemble_progressive: median {out['loop_ms_median']:.1f} ms ({min(ms['loop']):.1f} .. "
          f"{max(ms['loop']):.1f}); library launches per round: {n_round} for {B} puzzles, {n_one} for one")
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
