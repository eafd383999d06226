"""All-pairs matching of K = 16 pieces of N = 1024 points (fp32, closed-form weights, seeded pieces): the factored table of
puzzlenet_amd.assembly.match_pairs (a) against what a user had before it (b) - predict5(training=False) over the 240
ordered pairs in batches of 64, followed by the same top-k / chamfer scoring - alternated in one process; then the
pair-head kernel alone against the 16 point_mlp3 launches of match_pairs' fallback on the same inputs (the library's own
event pair around every kernel launch, ops.ktimer_start / ktimer_stop), beside the bytes each must move.

    python tools/bench_assembly.py [--reps 20] [--out profiles/assembly_k16.json]
    python tools/bench_assembly.py --progressive [--reps 20] [--out profiles/assembly_progressive_k16.json]
    python tools/bench_assembly.py --refine [--reps 20] [--out profiles/assembly_refine_k16.json]
    python tools/bench_assembly.py --batch 64 [--reps 10] [--out profiles/assembly_batch.json]
    python tools/bench_assembly.py --beam [--batch 64] [--reps 20] [--out profiles/assembly_beam.json]
    python tools/bench_assembly.py --forest [--batch 64] [--reps 20] [--out profiles/assemble_forest.txt]
    python tools/bench_assembly.py --forest-beam [--batch 64] [--reps 20] [--out profiles/assemble_forest_beam.txt]

--progressive measures instead (a) ops.merge_resample against the unfused chain se3.transform_points -> cat ->
farthest_point_sample -> index_points on the same inputs (Na = Nb = 1024 and 2048, M = 1 and 16; device time between two
events around 20 back-to-back calls, five repeats, alternated) and (b) one ProgressiveAssembler.step() at K = 16 against
match_pairs on the same 15 parts, what a round cost before it (host wall time around a synchronised call, alternated).

--refine measures instead (a) assembly.refine_pairs - 30 ICP iterations at most over the 256 pairs of the K = 16 table, one
launch, every pair stopping by the accept rule - against the torch composition a user would write today with public calls
(transform, torch.cdist and two arg-mins, two gathers, centring, bmm, torch.linalg.svd with the sign fix, compose; ops.chamfer
for the final score) on the same boundaries and poses, once with 30 fixed iterations (it has no accept rule) and once with as
many iterations as the LONGEST pair of the fused launch ran (iters_used max + 1: the matched count, since the launch lasts as
long as its longest problem); device time between two events around each call, alternated in one process; per-iteration
figures and the library's launches beside them; (a') assembly.refine_assembly on the greedy walk over the same table and
over its first 8 pieces' - the time of its one kernel, 30 sweeps at most, with the default joint set and with every ordered
pair as a joint (there is nothing earlier to compare it with), and the K = 8 default-joints figure again on the keep = 0.5
table and on the auto table (kept="frozen": joint_refine_counts_kernel, a count per joint; field joint_refine_counts_kernel_ms,
with the joints' mean counts); (a'') the trimmed launch of refine_pairs at keep = 0.5 on the
same boundaries and poses beside the untrimmed one - the time of each one's kernel per launch (the library's own event pair),
each in a run of its own launches in one process; (a''') the auto launch (keep = "auto": the share found per pair on the
device) the same way, with its ratio to the trimmed launch; and (b) match_pairs with refine = 30 against refine = 0 (host wall time around
a synchronised call, alternated).

--batch Z measures instead the whole chain on Z fractured puzzles of P = 8 pieces (datapipe.fracture on seeded clouds of 20000
points; N = 1024, k = 128, the same FPS starts on both sides): (a) through the batched functions - match_puzzles, assemble_batch,
with joint refinement refine_assembly_batch (30 sweeps at most), evaluate_batch, one download of the means - and (b) as the loop
over the per-puzzle functions match_pairs, assemble, refine_assembly, evaluate; once without and once with the joint refinement;
host wall time around a call that ends in a device synchronise, the two alternated in one process; beside them the per-launch
device time of assemble_walk_kernel (the library's own event pair, ops.ktimer_start / ktimer_stop) and the part accuracy either
path reports (closed-form weights: the number means nothing, it only has to be the same question).

--beam [--batch Z] measures instead, on Z = 64 fractured puzzles of P = 8 and of P = 16 pieces (the same clouds and starts as
--batch): the per-launch device time of assemble_beam_kernel (assembly.assemble_beam_batch, weight 1) at (beam, branch) = (1, 1),
(4, 4) and (8, 8), of assemble_walk_kernel on the same tables (the library's own event pair, ops.ktimer_start / ktimer_stop), and
the device time of the match_puzzles call that made the table - the cost the walk stands beside.

--forest [--batch Z] measures instead, on Z = 64 tables of tests/_walk_cases.py of K = 16 and of K = 64 pieces, the per-launch
device time of assemble_forest_kernel (ops.assemble_forest) beside assemble_walk_kernel on the same tables (the library's own event
pair): kind `random` without a threshold - one component, the cost of the state the forest adds - and kind `max_score` - the walk
stops in mid-range and the forest restarts many times.

--forest-beam [--batch Z] measures instead the per-launch device time of assemble_forest_beam_kernel (ops.assemble_forest_beam,
weight 1; the library's own event pair) at K = 16 and 64 and (beam, branch) = (1, 1), (4, 4) and (8, 8) on two kinds of table:
tables without a restart (kind `random` of tests/_beam_cases.py, no threshold) beside assemble_beam_kernel on the same tables - the
two do the same work there but for a few bytes of bookkeeping per child -, and tables with restarts (kind `max_score`, and the
planted piles of tests/_forest_beam_cases.py: 2 objects of 8 pieces, 4 of 16) beside assemble_forest_kernel.

Needs a GPU (there is no CPU path)."""
import argparse
import functools
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch

K, N, TOP, BATCH = 16, 1024, 128, 64


def _timed(fn, reps):
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms


def _spread(ms):
    s = sorted(ms)
    return {"median_ms": statistics.median(s), "min_ms": s[0], "max_ms": s[-1], "p10_ms": s[len(s) // 10], "p90_ms": s[(9 * len(s)) // 10],
            "reps": len(s)}


def _device_ms(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def _kernel_us(fn, name, reps, warmup):
    """Mean device time in us of the launches of the one kernel whose name holds `name`, over `reps` calls of fn after `warmup`
    untimed ones (the library's own event pair per launch, ops.ktimer_start / ktimer_stop)."""
    from puzzlenet_amd import ops
    for _ in range(warmup):
        fn()
    ops.ktimer_start()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    rows = ops.ktimer_stop()
    hit = [v for k_, v in rows.items() if name in k_]
    if len(hit) != 1 or hit[0][0] != reps:
        sys.exit(f"kernel timer: expected {reps} launches of {name} in one row, got {rows}")
    return 1e3 * hit[0][1] / hit[0][0]


def progressive(args):
    from oracle import model_ref as mr
    from puzzlenet_amd import assembly, model5_b, ops, se3
    dev = torch.device("cuda:0")
    result = {"tool": "tools/bench_assembly.py --progressive", "device": torch.cuda.get_device_name(0), "dtype": "float32",
              "merge": [], "k": TOP}
    g = torch.Generator().manual_seed(16)
    for n in (1024, 2048):
        for M in (1, 16):
            a, b = torch.rand(M, n, 3, generator=g).to(dev), torch.rand(M, n, 3, generator=g).to(dev)
            T = se3.exp(((torch.rand(M, 6, generator=g) - 0.5)).to(dev))
            start = torch.randint(0, 2 * n, (M,), generator=g).to(dev)

            def fused():
                return ops.merge_resample(a, b, T, start, n)

            def chain():
                u = torch.cat((a, se3.transform_points(T, b)), dim=1)
                return ops.index_points(u, ops.farthest_point_sample(u, n, start))

            with torch.no_grad():
                if not torch.equal(fused()[0], chain()):
                    # (the chain's transform rounds in its own order: equal picks are not promised, only the same work)
                    result.setdefault("note", "fused and chained outputs differ in some bits (transform rounding order)")
                for _ in range(args.warmup):
                    fused(), chain()
                f_ms, c_ms = [], []
                for _ in range(5):
                    f_ms.append(_device_ms(fused, 20))
                    c_ms.append(_device_ms(chain, 20))
            row = {"Na": n, "Nb": n, "n_out": n, "M": M, "fused_ms": sorted(f_ms), "chain_ms": sorted(c_ms),
                   "fused_median_ms": statistics.median(f_ms), "chain_median_ms": statistics.median(c_ms)}
            row["chain_over_fused"] = row["chain_median_ms"] / row["fused_median_ms"]
            print(json.dumps(row))
            result["merge"].append(row)

    model = model5_b.TouchedRegraster(mr.Cfg(num_points=N))
    mr.fill_params(model)
    model.to(dev)
    pieces = torch.rand(K, N, 3, generator=g).to(dev)
    s1, s2 = torch.randint(0, N, (K,), generator=g), torch.randint(0, 512, (K,), generator=g)
    step_ms, full_ms = [], []
    for rep in range(args.warmup + args.reps):
        asm = assembly.ProgressiveAssembler(model, pieces, k=TOP, start=(s1, s2), generator=torch.Generator().manual_seed(rep))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        edge = asm.step()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        if edge is None or asm.parts.shape[0] != K - 1:
            sys.exit("the first round made no edge")
        parts, starts = asm.parts, asm.starts
        ms = _timed(lambda: assembly.match_pairs(model, parts, k=TOP, start=starts), 1)
        if rep >= args.warmup:
            step_ms.append((t1 - t0) * 1e3)
            full_ms += ms
    result["round_K16"] = {"K": K, "N": N, "step": _spread(step_ms), "match_pairs_15_parts": _spread(full_ms),
                           "full_over_step_median": statistics.median(full_ms) / statistics.median(step_ms)}
    print(json.dumps(result["round_K16"]))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(result, indent=1) + "\n")


def refine(args):
    from oracle import model_ref as mr
    from puzzlenet_amd import assembly, model5_b, ops, se3
    ITERS = 30
    dev = torch.device("cuda:0")
    model = model5_b.TouchedRegraster(mr.Cfg(num_points=N))
    mr.fill_params(model)
    model.to(dev)
    g = torch.Generator().manual_seed(16)
    pieces = torch.rand(K, N, 3, generator=g).to(dev)
    start = (torch.randint(0, N, (K,), generator=g), torch.randint(0, 512, (K,), generator=g))
    with torch.no_grad():
        table = assembly.match_pairs(model, pieces, k=TOP, start=start)
        Bf = ops.index_points(pieces, table.top_f.reshape(K, K * TOP)).view(K * K, TOP, 3)
        Bm = ops.index_points(pieces, table.top_m)
        Bm_pairs = Bm.unsqueeze(0).expand(K, -1, -1, -1).reshape(K * K, TOP, 3).contiguous()
        T0 = table.T.reshape(K * K, 4, 4).contiguous()

    def fused():
        return assembly.refine_pairs(pieces, table.top_f, pieces, table.top_m, table.T, ITERS)

    def composition(iters):
        """What a user writes today with public calls only: `iters` fixed iterations (no accept rule: that would need the score,
        i.e. one more pass over the distances per iteration), every step a separate launch or several."""
        T = T0
        with torch.no_grad():
            for _ in range(iters):
                D = torch.cdist(Bf, se3.transform_points(T, Bm_pairs))               # [P, k, k]
                i1, i2 = D.argmin(dim=2), D.argmin(dim=1)                            # per fixed point, per moved point
                p = torch.cat((Bf, torch.gather(Bf, 1, i2.unsqueeze(-1).expand(-1, -1, 3))), dim=1)
                q = torch.cat((torch.gather(Bm_pairs, 1, i1.unsqueeze(-1).expand(-1, -1, 3)), Bm_pairs), dim=1)
                pc, qc = p.mean(dim=1, keepdim=True), q.mean(dim=1, keepdim=True)
                S = torch.bmm((q - qc).transpose(1, 2), p - pc)
                U, _s, Vh = torch.linalg.svd(S)
                V = Vh.transpose(1, 2)
                d = torch.sign(torch.linalg.det(torch.bmm(V, U.transpose(1, 2))))
                V = torch.cat((V[:, :, :2], V[:, :, 2:] * d.view(-1, 1, 1)), dim=2)
                R = torch.bmm(V, U.transpose(1, 2))
                t = pc.transpose(1, 2) - torch.bmm(R, qc.transpose(1, 2))
                T = torch.cat((torch.cat((R, t), dim=2), T0[:, 3:, :]), dim=1).contiguous()
            d1, d2 = ops.chamfer(Bf, se3.transform_points(T, Bm_pairs))
            return T, d1.mean(dim=1) + d2.mean(dim=1)

    with torch.no_grad():
        r = fused()
    # the launch lasts as long as its longest problem: iters_used accepted candidates and the one that ended its loop
    longest = min(ITERS, int(r.iters_used.max()) + 1)
    Tc, sc = composition(ITERS)
    for _ in range(args.warmup):
        fused(), composition(ITERS), composition(longest)
    f_ms, c_ms, m_ms = [], [], []
    for _ in range(args.reps):               # alternated in one process
        f_ms.append(_device_ms(fused, 1))
        c_ms.append(_device_ms(lambda: composition(ITERS), 1))
        m_ms.append(_device_ms(lambda: composition(longest), 1))
    # kernel launches of the library in one call of each (torch's own kernels of the composition are not in this count)
    ops.ktimer_start()
    fused()
    torch.cuda.synchronize()
    k_f = ops.ktimer_stop()
    icp = [v for name, v in k_f.items() if "icp_refine_kernel" in name]
    # the trimmed launch at keep = 0.5 of both sides beside the untrimmed one: kernel time per launch

    def trimmed():
        return assembly.refine_pairs(pieces, table.top_f, pieces, table.top_m, table.T, ITERS, keep=0.5)

    # (each kernel in a run of its own launches, the sequence the untrimmed kernel had before there was a second one)
    u_ms = [_kernel_us(fused, "icp_refine_kernel", 1, 0) / 1e3 for _ in range(args.reps)]
    for _ in range(args.warmup):
        trimmed()
    t_ms = [_kernel_us(trimmed, "icp_trim_kernel", 1, 0) / 1e3 for _ in range(args.reps)]
    rt = trimmed()
    trim = {"keep": 0.5, "icp_refine_kernel_ms": _spread(u_ms), "icp_trim_kernel_ms": _spread(t_ms),
            "trim_over_untrimmed_median": statistics.median(t_ms) / statistics.median(u_ms),
            "iters_used_mean": float(rt.iters_used.float().mean()), "iters_used_max": int(rt.iters_used.max())}
    print(json.dumps({"trimmed_launch": trim}))
    # the auto launch (the share found per pair and per evaluated pose, AutoKeep's defaults) on the same boundaries and poses

    def found():
        return assembly.refine_pairs(pieces, table.top_f, pieces, table.top_m, table.T, ITERS, keep="auto")

    for _ in range(args.warmup):
        found()
    a_ms = [_kernel_us(found, "icp_auto_kernel", 1, 0) / 1e3 for _ in range(args.reps)]
    ra = found()
    auto = {"keep": "auto", "least": assembly.AutoKeep().least, "power": assembly.AutoKeep().power, "icp_auto_kernel_ms": _spread(a_ms),
            "auto_over_trim_median": statistics.median(a_ms) / statistics.median(t_ms),
            "auto_over_untrimmed_median": statistics.median(a_ms) / statistics.median(u_ms),
            "iters_used_mean": float(ra.iters_used.float().mean()), "iters_used_max": int(ra.iters_used.max()),
            "count_f_mean": float(ra.count_f.float().mean()), "count_m_mean": float(ra.count_m.float().mean())}
    print(json.dumps({"auto_launch": auto}))
    # the joint refinement of the greedy assembly (assembly.refine_assembly: one launch of joint_refine_kernel, 30 sweeps at
    # most) at K = 8 (the first 8 pieces' sub-table) and K = 16: the default joint set and every ordered pair
    joint = {}
    for Kj in (8, K):
        sub = assembly.PairTable(None, table.T[:Kj, :Kj].contiguous(), None, None, table.top_f[:Kj, :Kj].contiguous(),
                                 table.top_m[:Kj].contiguous(), table.score[:Kj, :Kj].contiguous(), None)
        asm = assembly.assemble(sub.score, sub.T)
        for label, limit in (("default_joints", None), ("all_pairs", float("inf"))):
            run = lambda: assembly.refine_assembly(pieces[:Kj], sub, asm, sweeps=ITERS, joint_score=limit)
            for _ in range(args.warmup):
                run()
            ops.ktimer_start()
            jr = run()
            torch.cuda.synchronize()
            k_j = ops.ktimer_stop()
            ms = [v[1] for name, v in k_j.items() if "joint_refine_kernel" in name]
            joint[f"K{Kj}_{label}"] = {"joints": len(jr.joints), "sweeps_used": int(jr.sweeps_used), "kernel_ms": ms[0] if ms else None,
                                       "device_ms": _spread([_device_ms(run, 1) for _ in range(args.reps)]),
                                       "score_over_score0": float(jr.score / jr.score0)}
    print(json.dumps({"joint_refine_kernel_ms": joint}))
    # the same K = 8 default-joints measurement on tables that carry kept sets, refined above from the same poses: the
    # kept-fraction table (keep = 0.5: 64 rows a side, pzn_joint_refine_f32) and the auto table (a count per joint, sets of
    # stride k, pzn_joint_refine_counts_f32 through kept="frozen"), with the mean counts of the joints' sets beside the time
    joint_counts = {}
    eye8 = torch.eye(8, dtype=torch.bool, device=dev)
    for label, rr, kind, kept in (("keep_0.5", rt, assembly.TrimmedPairTable, None), ("keep_auto", ra, assembly.AutoPairTable, "frozen")):
        extra = [getattr(rr, f)[:8, :8].contiguous() for f in kind._fields[8:]]
        sub = kind(None, rr.T[:8, :8].contiguous(), None, None, table.top_f[:8, :8].contiguous(), table.top_m[:8].contiguous(),
                   rr.score[:8, :8].masked_fill(eye8, float("inf")), None, *extra)
        asm = assembly.assemble(sub.score, sub.T)
        run = lambda: assembly.refine_assembly(pieces[:8], sub, asm, sweeps=ITERS, kept=kept)
        for _ in range(args.warmup):
            run()
        ops.ktimer_start()
        jr = run()
        torch.cuda.synchronize()
        k_j = ops.ktimer_stop()
        ms = [v[1] for name, v in k_j.items() if "joint_refine" in name]      # (either kernel: the launch says which)
        ji, jj = (torch.tensor(x, device=dev) for x in zip(*jr.joints))
        cf = sub.count_f[ji, jj].float().mean() if kept else sub.kept_f.shape[-1]
        cm = sub.count_m[ji, jj].float().mean() if kept else sub.kept_m.shape[-1]
        joint_counts[f"K8_default_joints_{label}"] = {
            "kernel": next((name for name in k_j if "joint_refine" in name), None), "joints": len(jr.joints),
            "count_f_mean": float(cf), "count_m_mean": float(cm), "stride": sub.kept_f.shape[-1],
            "sweeps_used": int(jr.sweeps_used), "kernel_ms": ms[0] if ms else None,
            "device_ms": _spread([_device_ms(run, 1) for _ in range(args.reps)]), "score_over_score0": float(jr.score / jr.score0)}
    print(json.dumps({"joint_refine_counts_kernel_ms": joint_counts}))
    off = ~torch.eye(K, dtype=torch.bool, device=dev)
    f_med, c_med, m_med = statistics.median(f_ms), statistics.median(c_ms), statistics.median(m_ms)
    result = {"tool": "tools/bench_assembly.py --refine", "device": torch.cuda.get_device_name(0), "dtype": "float32", "K": K,
              "N": N, "k": TOP, "pairs": K * K, "iters": ITERS,
              "refine_pairs_device": _spread(f_ms),
              "torch_composition_fixed_iters_device": _spread(c_ms),
              "torch_composition_matched_device": dict(_spread(m_ms), iterations=longest),
              "composition_fixed_over_refine_pairs_median": c_med / f_med,
              "composition_matched_over_refine_pairs_median": m_med / f_med,
              "per_iteration_ms": {"refine_pairs_per_candidate_of_longest_pair": f_med / longest,
                                   "composition": c_med / ITERS},
              "refine_pairs_library_launches": {k_: v[0] for k_, v in k_f.items()},
              "icp_refine_kernel_ms": icp[0][1] if icp else None,
              "trimmed_launch": trim,
              "auto_launch": auto,
              "joint_refine_kernel_ms": joint,
              "joint_refine_counts_kernel_ms": joint_counts,
              "iters_used_mean": float(r.iters_used.float().mean()), "iters_used_max": int(r.iters_used.max()),
              "score_over_score0_mean_off_diagonal": float((r.score[off] / r.score0[off]).mean()),
              "composition_fixed_score_over_score0_mean_off_diagonal": float((sc.view(K, K)[off] / r.score0[off]).mean())}
    print(json.dumps(result))
    w0, w1 = [], []
    for _ in range(args.reps):
        w0 += _timed(lambda: assembly.match_pairs(model, pieces, k=TOP, start=start), 1)
        w1 += _timed(lambda: assembly.match_pairs(model, pieces, k=TOP, start=start, refine=ITERS), 1)
    result["match_pairs_wall"] = {"refine_0": _spread(w0), f"refine_{ITERS}": _spread(w1),
                                  "added_median_ms": statistics.median(w1) - statistics.median(w0)}
    print(json.dumps(result["match_pairs_wall"]))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(result, indent=1) + "\n")


def batch(args):
    import numpy as np
    from oracle import model_ref as mr
    from puzzlenet_amd import assembly, datapipe, model5_b, ops
    Z, P, M, CAND, SWEEPS = args.batch, 8, 20000, 16, 30
    dev = torch.device("cuda:0")
    model = model5_b.TouchedRegraster(mr.Cfg(num_points=N))
    mr.fill_params(model)
    model.to(dev)
    rng = np.random.RandomState(16)
    raw = (rng.rand(Z, M, 3) - 0.5).astype(np.float32)
    draws = datapipe.fracture_draws(rng, torch.Generator().manual_seed(16), Z, P, CAND, 0.8)
    to = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    g = torch.Generator().manual_seed(17)
    s1, s2 = torch.randint(0, N, (Z, P), generator=g), torch.randint(0, 512, (Z, P), generator=g)
    with torch.no_grad():
        f = datapipe.fracture(to(raw), *(to(d) for d in draws), n=N, k=TOP)
    torch.cuda.synchronize()

    def batched(sweeps):
        with torch.no_grad():
            table = assembly.match_puzzles(model, f.pieces, k=TOP, start=(s1, s2))
            asm = assembly.assemble_batch(table.score, table.T)
            G = assembly.refine_assembly_batch(f.pieces, table, asm, sweeps=sweeps).G if sweeps else asm.G
            ev = assembly.evaluate_batch(G, asm.placed, f.pose, f.rest, asm.root, asm.edges, asm.n_edges, f.mates)
            return float(ev.part_accuracy.mean().cpu())                           # the one download

    def looped(sweeps):
        acc = []
        for z in range(Z):
            t = assembly.match_pairs(model, f.pieces[z], k=TOP, start=(s1[z], s2[z]))
            a = assembly.assemble(t.score, t.T)
            G = assembly.refine_assembly(f.pieces[z], t, a, sweeps=sweeps).G if sweeps else a.G
            acc.append(assembly.evaluate(G, a.placed, f.pose[z], f.rest[z], a.root, a.edges, f.mates[z]).part_accuracy)
        return float(np.mean(acc))

    result = {"tool": f"tools/bench_assembly.py --batch {Z}", "device": torch.cuda.get_device_name(0), "dtype": "float32", "Z": Z,
              "P": P, "N": N, "k": TOP, "M": M, "valid_fractures": int(f.ok.sum()), "timing": "host wall around a synchronised call, ms"}
    for label, sweeps in (("walk_only", 0), (f"joint_{SWEEPS}", SWEEPS)):
        for _ in range(args.warmup):
            acc_b, acc_l = batched(sweeps), looped(sweeps)
        b_ms, l_ms = [], []
        for _ in range(args.reps):              # alternated: both see the same clocks and the same neighbours on the box
            b_ms += _timed(lambda: batched(sweeps), 1)
            l_ms += _timed(lambda: looped(sweeps), 1)
        result[label] = {"batched": _spread(b_ms), "per_puzzle_loop": _spread(l_ms),
                         "loop_over_batched_median": statistics.median(l_ms) / statistics.median(b_ms),
                         "part_accuracy_batched": acc_b, "part_accuracy_loop": acc_l}
        print(json.dumps({label: result[label]}))
    with torch.no_grad():
        table = assembly.match_puzzles(model, f.pieces, k=TOP, start=(s1, s2))
        assembly.assemble_batch(table.score, table.T)
        ops.ktimer_start()
        for _ in range(args.reps):
            assembly.assemble_batch(table.score, table.T)
        torch.cuda.synchronize()
        rows = ops.ktimer_stop()
    hit = [v for name, v in rows.items() if "assemble_walk_kernel" in name]
    if len(hit) != 1:
        sys.exit(f"kernel timer: expected one row for assemble_walk_kernel, got {sorted(rows)}")
    result["assemble_walk_kernel"] = {"launches_timed": hit[0][0], "us_per_launch": 1e3 * hit[0][1] / hit[0][0], "puzzles_per_launch": Z,
                                      "K": P}
    print(json.dumps({"assemble_walk_kernel": result["assemble_walk_kernel"]}))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(json.dumps(result, indent=1) + "\n")


def beam(args):
    import numpy as np
    from oracle import model_ref as mr
    from puzzlenet_amd import assembly, datapipe, model5_b, ops
    Z, M, CAND = args.batch or 64, 20000, 16
    dev = torch.device("cuda:0")
    model = model5_b.TouchedRegraster(mr.Cfg(num_points=N))
    mr.fill_params(model)
    model.to(dev)
    result = {"tool": f"tools/bench_assembly.py --beam --batch {Z}", "device": torch.cuda.get_device_name(0), "dtype": "float32", "Z": Z,
              "N": N, "k": TOP, "M": M, "weight": 1.0,
              "timing": "kernels: the library's own event pair per launch (ops.ktimer_*), us; match_puzzles: device time between two "
                        "events around one call, ms"}

    kernel_us = functools.partial(_kernel_us, reps=args.reps, warmup=1)

    for P in (8, 16):
        rng = np.random.RandomState(16)
        raw = (rng.rand(Z, M, 3) - 0.5).astype(np.float32)
        draws = datapipe.fracture_draws(rng, torch.Generator().manual_seed(16), Z, P, CAND, 0.8)
        to = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
        g = torch.Generator().manual_seed(17)
        s1, s2 = torch.randint(0, N, (Z, P), generator=g), torch.randint(0, 512, (Z, P), generator=g)
        with torch.no_grad():
            f = datapipe.fracture(to(raw), *(to(d) for d in draws), n=N, k=TOP)
            match = lambda: assembly.match_puzzles(model, f.pieces, k=TOP, start=(s1, s2))
            for _ in range(args.warmup):
                table = match()
            match_ms = sorted(_device_ms(match, 1) for _ in range(args.reps))
            moment = assembly.boundary_moments(f.pieces, table.top_m)
            row = {"P": P, "match_puzzles_device_ms": _spread(match_ms),
                   "assemble_walk_kernel_us": kernel_us(lambda: assembly.assemble_batch(table.score, table.T), "assemble_walk_kernel")}
            greedy = assembly.assemble_batch(table.score, table.T)
            for B, C in ((1, 1), (4, 4), (8, 8)):
                run = lambda: assembly.assemble_beam_batch(table.score, table.T, moment, beam=B, branch=C)
                us = kernel_us(run, "assemble_beam_kernel")
                same = float((run().edges == greedy.edges).all(dim=2).all(dim=1).double().mean().cpu())
                row[f"assemble_beam_kernel_us_B{B}_C{C}"] = us
                row[f"share_of_puzzles_with_the_greedy_tree_B{B}_C{C}"] = same
            row["beam_8_8_over_match_puzzles"] = row["assemble_beam_kernel_us_B8_C8"] * 1e-3 / row["match_puzzles_device_ms"]["median_ms"]
        print(json.dumps(row))
        result[f"P{P}"] = row
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(json.dumps(result, indent=1) + "\n")


def forest(args):
    """The forest walk's launch beside the greedy walk's on the same tables (the table kinds of tests/_walk_cases.py): `random`
    without a threshold - one component, the cost of the added state - and `max_score` - the walk stops in mid-range and the
    forest restarts many times."""
    from puzzlenet_amd import ops
    from tests import _walk_cases as wc
    Z = args.batch or 64
    dev = torch.device("cuda:0")

    kernel_us = functools.partial(_kernel_us, reps=args.reps, warmup=max(args.warmup, 1))

    lines = [f"tools/bench_assembly.py --forest --batch {Z} --reps {args.reps} on {torch.cuda.get_device_name(0)}",
             "the library's own event pair per launch (ops.ktimer_*), mean over the timed launches after the warm-up, us;",
             f"Z = {Z} tables of tests/_walk_cases.py (seed 2000), one launch each; assemble_walk_kernel is the one built beside the",
             "forest kernel (its result tail takes a component per piece and is handed 0)", ""]
    for kind in ("random", "max_score"):
        for K in (16, 64):
            S, T, m = wc.make(kind, Z, K, 2000)
            s, t = torch.from_numpy(S).to(dev), torch.from_numpy(T).to(dev)
            out = ops.assemble_forest(s, t, max_score=m)
            walk = kernel_us(lambda: ops.assemble_walk(s, t, max_score=m), "assemble_walk_kernel")
            frst = kernel_us(lambda: ops.assemble_forest(s, t, max_score=m), "assemble_forest_kernel")
            lines.append(f"{kind:9s} K = {K:2d}: assemble_walk_kernel {walk:8.1f} us, assemble_forest_kernel {frst:8.1f} us, forest / walk "
                         f"{frst / walk:5.2f}; components per pile {float(out[10].double().mean()):.1f}, forest edges per pile "
                         f"{float(out[3].double().mean()):.1f}")
            print(lines[-1])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


def forest_beam(args):
    """The forest beam's launch beside the beam's on tables without a restart, and beside the forest walk's on tables with
    restarts (kind `max_score`) and on planted piles."""
    from puzzlenet_amd import ops
    from tests import _beam_cases as bc
    from tests import _forest_beam_cases as fb
    Z = args.batch or 64
    dev = torch.device("cuda:0")

    kernel_us = functools.partial(_kernel_us, reps=args.reps, warmup=max(args.warmup, 1))

    lines = [f"tools/bench_assembly.py --forest-beam --batch {Z} --reps {args.reps} on {torch.cuda.get_device_name(0)}",
             "the library's own event pair per launch (ops.ktimer_*), mean over the timed launches after the warm-up, us;",
             f"Z = {Z} tables, one launch each, weight 1", "",
             "tables without a restart (tests/_beam_cases.py, kind random, seed 2100, no threshold): beside assemble_beam_kernel"]
    say = lambda line: (lines.append(line), print(line))
    for K in (16, 64):
        S, T, M, _ = bc.make("random", Z, K, 2100)
        s, t, m = (torch.from_numpy(x).to(dev) for x in (S, T, M))
        for B, C in ((1, 1), (4, 4), (8, 8)):
            a, b = ops.assemble_beam(s, t, m, beam=B, branch=C), ops.assemble_forest_beam(s, t, m, beam=B, branch=C)
            if not all(torch.equal(x, y) for x, y in zip(a, b[:8] + b[11:])):
                sys.exit(f"K = {K}, beam {B}, branch {C}: the forest beam is not the beam on a table without a restart")
            beam_us = kernel_us(lambda: ops.assemble_beam(s, t, m, beam=B, branch=C), "assemble_beam_kernel")
            fb_us = kernel_us(lambda: ops.assemble_forest_beam(s, t, m, beam=B, branch=C), "assemble_forest_beam_kernel")
            say(f"random    K = {K:2d} B = {B} C = {C}: assemble_beam_kernel {beam_us:9.1f} us, assemble_forest_beam_kernel {fb_us:9.1f} us, "
                f"forest beam / beam {fb_us / beam_us:5.2f}")
    say("")
    say("tables with restarts (kind max_score, seed 2100; planted piles of tests/_forest_beam_cases.py, seeds 0 .. Z - 1, 2 objects of 8")
    say("pieces and 4 of 16, max_score 0.03): beside assemble_forest_kernel")
    for kind, K in (("max_score", 16), ("max_score", 64), ("piles 2x8", 16), ("piles 4x16", 64)):
        if kind == "max_score":
            S, T, M, ms = bc.make(kind, Z, K, 2100)
        else:
            S, T, M, _, _, ms = fb.piles(range(Z), 2 if K == 16 else 4, 8 if K == 16 else 16)
        s, t, m = (torch.from_numpy(x).to(dev) for x in (S, T, M))
        frst = kernel_us(lambda: ops.assemble_forest(s, t, max_score=ms), "assemble_forest_kernel")
        greedy = ops.assemble_forest(s, t, max_score=ms)
        for B, C in ((1, 1), (4, 4), (8, 8)):
            out = ops.assemble_forest_beam(s, t, m, beam=B, branch=C, max_score=ms)
            same = float((out[1] == greedy[1]).all(dim=2).all(dim=1).double().mean())
            fb_us = kernel_us(lambda: ops.assemble_forest_beam(s, t, m, beam=B, branch=C, max_score=ms), "assemble_forest_beam_kernel")
            say(f"{kind:10s} K = {K:2d} B = {B} C = {C}: assemble_forest_kernel {frst:8.1f} us, assemble_forest_beam_kernel {fb_us:9.1f} us, "
                f"forest beam / forest {fb_us / frst:7.2f}; components per pile {float(out[10].double().mean()):.1f}, the forest walk's "
                f"edges in {100 * same:.0f} % of the piles")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--progressive", action="store_true")
    ap.add_argument("--refine", action="store_true")
    ap.add_argument("--batch", type=int, default=0, help="Z: time the batched chain on Z fractured puzzles against the per-puzzle loop")
    ap.add_argument("--beam", action="store_true", help="time the beam walk's launch beside the greedy walk's and match_puzzles")
    ap.add_argument("--forest", action="store_true", help="time the forest walk's launch beside the greedy walk's on the same tables")
    ap.add_argument("--forest-beam", action="store_true",
                    help="time the forest beam's launch beside the beam's and the forest walk's on the same tables")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out is None:
        name = "assembly_progressive_k16.json" if args.progressive else ("assembly_refine_k16.json" if args.refine else "assembly_k16.json")
        name = "assembly_batch.json" if args.batch else name
        name = "assembly_beam.json" if args.beam else name
        name = "assemble_forest.txt" if args.forest else name
        name = "assemble_forest_beam.txt" if args.forest_beam else name
        args.out = os.path.join(ROOT, "profiles", name)
    if args.reps < (5 if args.batch else 20):
        sys.exit("--reps: at least 20 timed repetitions each (--batch, whose loop side takes seconds a repetition: at least 5)")
    if not torch.cuda.is_available():
        sys.exit("tools/bench_assembly.py needs a GPU: puzzlenet_amd has no CPU path")
    if args.forest_beam:
        return forest_beam(args)
    if args.forest:
        return forest(args)
    if args.beam:
        return beam(args)
    if args.batch:
        return batch(args)
    if args.progressive:
        return progressive(args)
    if args.refine:
        return refine(args)

    from oracle import model_ref as mr
    from puzzlenet_amd import assembly, model5_b, ops, se3
    dev = torch.device("cuda:0")
    model = model5_b.TouchedRegraster(mr.Cfg(num_points=N))
    mr.fill_params(model)
    model.to(dev)
    model.fps_generator = torch.Generator().manual_seed(7)
    g = torch.Generator().manual_seed(16)
    pieces = torch.rand(K, N, 3, generator=g).to(dev)
    off = [(i, j) for i in range(K) for j in range(K) if i != j]
    I = torch.tensor([p[0] for p in off], device=dev)
    J = torch.tensor([p[1] for p in off], device=dev)

    def factored():
        return assembly.match_pairs(model, pieces, k=TOP).score

    def pair_batches():
        """predict5 on the materialised pairs, 64 at a time, and the scoring of match_pairs on each batch."""
        scores = []
        with torch.no_grad():
            for a in range(0, len(off), BATCH):
                fpc, mrpc = pieces[I[a:a + BATCH]], pieces[J[a:a + BATCH]]
                out, _, de_fpcb, de_mrpcb = model.predict5([fpc, mrpc], fpc.shape[0], training=False)
                T = se3.exp(out)
                top_f = ops.topk_rows(torch.softmax(de_fpcb, dim=1)[:, 1, :], TOP)
                top_m = ops.topk_rows(torch.softmax(de_mrpcb, dim=1)[:, 1, :], TOP)
                Bf = ops.index_points(fpc, top_f)
                Bm = se3.transform_points(T, ops.index_points(mrpc, top_m))
                d1, d2 = ops.chamfer(Bf, Bm)
                scores.append(d1.mean(dim=1) + d2.mean(dim=1))
        return torch.cat(scores)

    for _ in range(args.warmup):
        factored()
        pair_batches()
    ms_a, ms_b = [], []
    for _ in range(args.reps):              # alternated: both see the same clocks and the same neighbours on the box
        ms_a += _timed(factored, 1)
        ms_b += _timed(pair_batches, 1)
    a, b = _spread(ms_a), _spread(ms_b)

    # ---- the fixed-side boundary head alone: one pair_head launch against the fallback's 16 point_mlp3 launches
    with torch.no_grad():
        gen = torch.Generator().manual_seed(3)
        local = torch.randn(K, N, 64, generator=gen).to(dev)
        gvec = torch.randn(K, 64, generator=gen).to(dev)
        seq = model.MLPFpcb
        l1, l2, l3 = seq[0], seq[2], seq[4]
        par = (l1.weight, l1.bias, l2.weight, l2.bias, l3.weight, l3.bias)

        def fast():
            return ops.pair_head(local, gvec, *par)

        def fallback():
            return [ops.point_mlp3(local, *par, g=gvec[j:j + 1].expand(K, -1).reshape(K, 1, 64).contiguous()) for j in range(K)]

        for _ in range(args.warmup):
            fast()
            fallback()

        def kernel_time(fn, name):
            ops.ktimer_start()
            for _ in range(args.reps):
                fn()
            torch.cuda.synchronize()
            rows = ops.ktimer_stop()
            hit = [v for k_, v in rows.items() if name in k_]
            if len(hit) != 1:
                sys.exit(f"kernel timer: expected one row for {name}, got {sorted(rows)}")
            others = {k_: v for k_, v in rows.items() if name not in k_}
            return hit[0], others

        (n_f, ms_f), rest_f = kernel_time(fast, "pair_head_fwd_kernel")
        (n_s, ms_s), rest_s = kernel_time(fallback, "point_mlp3_fwd_kernel")
    us_fast = 1e3 * ms_f / n_f                              # per launch = per table
    us_slow = 1e3 * ms_s / n_s * K                          # 16 launches per table
    weights = 4 * (64 * 64 + 32 * 64 + 32 + 2 * 32 + 2)
    bytes_fast = 4 * K * N * 64 + 4 * K * 64 + weights + 4 * K * K * N * 2
    bytes_slow = K * (4 * K * N * (64 + 64 + 32 + 2) + 4 * K * 64 + weights)
    flop = 2 * K * N * (64 * 64 + K * (64 * 32 + 32 * 2))
    mfma_us = 1e6 * flop / (2500e12 / 6)                    # six bf16 MFMAs per fp32 product
    hbm_us = 1e6 * bytes_fast / 8e12
    bound = "MFMA" if mfma_us >= hbm_us else "HBM"
    result = {
        "tool": "tools/bench_assembly.py", "device": torch.cuda.get_device_name(0), "K": K, "N": N, "k": TOP, "dtype": "float32",
        "pairs": len(off), "pair_batch": BATCH,
        "match_pairs": a, "predict5_pair_batches": b, "speedup_median": b["median_ms"] / a["median_ms"],
        "pair_head_fwd_kernel": {
            "kernel_us_per_table": us_fast, "launches_timed": n_f, "bytes": bytes_fast, "flop": flop,
            "mfma_bound_us": mfma_us, "hbm_bound_us": hbm_us, "bound": bound,
            "fraction_of_bound": max(mfma_us, hbm_us) / us_fast,
            "other_kernels_us_per_table": {k_: 1e3 * v[1] / args.reps for k_, v in rest_f.items()}},
        "point_mlp3_fallback": {
            "kernel_us_per_table": us_slow, "launches_per_table": K, "launches_timed": n_s, "bytes": bytes_slow,
            "hbm_bound_us": 1e6 * bytes_slow / 8e12,
            "other_kernels_us_per_table": {k_: 1e3 * v[1] / args.reps for k_, v in rest_s.items()}},
        "pair_head_over_fallback": us_slow / us_fast,
    }
    line = json.dumps(result)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(result, indent=1) + "\n")
    if not a["median_ms"] < b["median_ms"]:
        sys.exit(f"match_pairs ({a['median_ms']:.3f} ms) is not faster than predict5 over the pair batches ({b['median_ms']:.3f} ms)")


if __name__ == "__main__":
    main()
