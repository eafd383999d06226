"""GPU training-pair construction (puzzlenet_amd/datapipe.py): pairs per second for raw clouds of M points cut, sampled
to N, labelled and moved — next to the training step's consumption rate, and to the reference-style numpy FPS of ONE
piece on one host core (the dominant cost of the reference's per-sample CPU pipeline).

    python tools/bench_datapipe.py [--cut {plane,sphere,cylinder,cone}] [--random_slice] [--reps 30] [--fracture]
                                   [--pieces P] [--curvature 2.0] [--erosion E [--chip DEPTH RADIUS]]

Then the loader's batch as PairFeeder builds it, B = 64, M = 10000, N = 2048, 16 candidates: datapipe.cut_pairs (plane) and, with
--cut a solid, datapipe.cut_pairs_solid of that kind next to the tensor form datapipe.make_pairs_solid on the same clouds with the
one candidate the kernel took - one process, the forms alternating inside every repetition, a device synchronise around each.
--random_slice: datapipe.cut_pairs_double (the double cuts, PairFeeder(split_twice=True)) beside the plane batch on the same clouds,
and its cut launch and its two sampling launches beside the plane batch's, each alone between two device events.
--fracture: only the fracture (datapipe.fracture), B = 64, M = 10000, P = 8 pieces, 16 candidates, pieces of >= 256 points: the
ops.fracture launch and the single cut's ops.cut_compact launch on the same clouds, alternating, each alone between two device
events, and the whole datapipe.fracture call (n = 256, k = 64) on a host clock around a device synchronise; the three medians
and the ratio of the two launches are written to profiles/fracture_batch.txt.
--pieces P: only the fracture feeder's batch (datapipe.cut_pairs_fracture, PairFeeder(pieces=P)) beside the plane batch on the same
clouds, B = 64, M = 10000, N = 2048, 16 candidates, alternating inside every repetition; and its cut launch and its two sampling
launches beside the plane batch's, each alone between two device events (profiles/fracture_feeder_batch.txt holds a run).
--curvature C (with --fracture or --pieces; default 2.0, 0: planes only): the curved forms beside the plane forms on the same
clouds, normals and anchors - the ops.fracture_curved launch and the whole curved datapipe.fracture call with --fracture, the
ops.fracture_pair_curved launch and the curved cut_pairs_fracture batch with --pieces - and the ratios curved / plane
(profiles/fracture_curved_batch.txt holds a run).
--erosion E [--chip DEPTH RADIUS] (with --fracture or --pieces; default 0: off): only the eroded forms beside the forms without
erosion, on the same clouds and draws, planes and (--curvature > 0) surfaces: with --fracture the ops.fracture_eroded launch and the
launch of the same form without erosion, alternating, each alone between two device events, and what erosion does to the contact
(valid samples, mates per sample, the lost share, with and without); with --pieces the ops.fracture_pair_eroded launch and the
cut_pairs_fracture batch the same way.  Medians, ratios and contact figures go to profiles/fracture_eroded_batch.txt, one block per
mode."""
import argparse, os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from puzzlenet_amd import datapipe
ap = argparse.ArgumentParser()
ap.add_argument("--cut", choices=["plane", "sphere", "cylinder", "cone"], default="plane")
ap.add_argument("--random_slice", action="store_true")
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--fracture", action="store_true")
ap.add_argument("--pieces", type=int, default=0)
ap.add_argument("--curvature", type=float, default=2.0)
ap.add_argument("--erosion", type=float, default=0.0)
ap.add_argument("--chip", type=float, nargs=2, default=(0.0, 0.0), metavar=("DEPTH", "RADIUS"))
a = ap.parse_args()
dev = torch.device('cuda:0')
g = torch.Generator().manual_seed(0)


def _again(rng):
    """A generator in rng's state: the curved draws begin with the plane draws' normals and anchors."""
    twin = np.random.RandomState()
    twin.set_state(rng.get_state())
    return twin


def bench_fracture(reps, curvature):
    from puzzlenet_amd import ops
    B, M, P, K, n, k = 64, 10000, 8, 16, 256, 64
    rng = np.random.RandomState(0)
    raw = torch.from_numpy((rng.rand(B, M, 3) - 0.5).astype(np.float32)).to(dev)
    twin = _again(rng)
    normals, u_anchor, u_start, twist = (torch.from_numpy(np.ascontiguousarray(t)).to(dev)
                                         for t in datapipe.fracture_draws(rng, torch.Generator().manual_seed(0), B, P, K, 0.8))
    pn, pz, pu = torch.from_numpy(rng.rand(B, K, 3)).to(dev), torch.from_numpy(rng.rand(B, K) / 3 - 0.4).to(dev), torch.from_numpy(rng.rand(B, 2)).to(dev)
    f = datapipe.fracture(raw, normals, u_anchor, u_start, twist, n=n, k=k)
    print('fracture: valid %d/%d, smallest piece %d, mates per sample %.1f' % (int(f.ok.sum()), B, int(f.counts.min()), float(f.mates.sum()) / 2 / B), flush=True)
    launches = {"ops.fracture (P = 8)": lambda: ops.fracture(raw, normals, u_anchor, u_start, n, M),
                "ops.cut_compact (the single cut)": lambda: ops.cut_compact(raw, pn, pz, pu, n, M)}
    if curvature > 0:
        frames, half_curv, c_anchor, c_start, c_twist = (
            torch.from_numpy(np.ascontiguousarray(t)).to(dev)
            for t in datapipe.fracture_curved_draws(twin, torch.Generator().manual_seed(0), B, P, K, 0.8, curvature))
        assert torch.equal(frames[:, :, :, 2], normals) and torch.equal(c_anchor, u_anchor)
        fc = datapipe.fracture(raw, None, c_anchor, c_start, c_twist, n=n, k=k, frames=frames, half_curv=half_curv)
        print('curved fracture, curvature %g: valid %d/%d, smallest piece %d, mates per sample %.1f, mean candidate taken %.2f (planes: %.2f)' % (
            curvature, int(fc.ok.sum()), B, int(fc.counts.min()), float(fc.mates.sum()) / 2 / B, float(fc.cand.float().mean()),
            float(f.cand.float().mean())), flush=True)
        launches["ops.fracture_curved (P = 8)"] = lambda: ops.fracture_curved(raw, frames, half_curv, c_anchor, c_start, n, M)
    lt = {name: [] for name in launches}
    whole, whole_curved = [], []
    for rep in range(reps + 3):                          # (three warm-up rounds of everything)
        for name, fn in launches.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize(); e0.record()
            fn()
            e1.record(); e1.synchronize()
            if rep >= 3:
                lt[name].append(e0.elapsed_time(e1) * 1e3)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        datapipe.fracture(raw, normals, u_anchor, u_start, twist, n=n, k=k)
        torch.cuda.synchronize()
        if rep >= 3:
            whole.append((time.perf_counter() - t0) * 1e3)
        if curvature > 0:
            torch.cuda.synchronize(); t0 = time.perf_counter()
            datapipe.fracture(raw, None, c_anchor, c_start, c_twist, n=n, k=k, frames=frames, half_curv=half_curv)
            torch.cuda.synchronize()
            if rep >= 3:
                whole_curved.append((time.perf_counter() - t0) * 1e3)
    fr_us, cut_us = (float(np.median(lt[name])) for name in list(launches)[:2])
    lines = ['tools/bench_datapipe.py --fracture --reps %d: B = %d, M = %d, P = %d, K = %d, n_min = n = %d, k = %d (medians of %d)' % (reps, B, M, P, K, n, k, reps)]
    for name in list(launches)[:2]:
        t = np.sort(np.array(lt[name]))
        lines.append('launch: %-34s %.0f us between events (min %.0f, max %.0f)' % (name, np.median(t), t[0], t[-1]))
    lines.append('ratio fracture / cut_compact: %.2f (%d cuts and a %d-way partition against 1 cut and a 2-way one)' % (fr_us / cut_us, P - 1, P))
    t = np.sort(np.array(whole))
    lines.append('datapipe.fracture, the whole call: %.2f ms per batch on the host clock (min %.2f, max %.2f), valid %d/%d' % (np.median(t), t[0], t[-1], int(f.ok.sum()), B))
    print('\n'.join(lines), flush=True)
    out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'fracture_batch.txt')
    with open(out, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')
    if curvature > 0:
        t, w = np.sort(np.array(lt["ops.fracture_curved (P = 8)"])), np.sort(np.array(whole_curved))
        print('launch: %-34s %.0f us between events (min %.0f, max %.0f), curvature %g' % ("ops.fracture_curved (P = 8)", np.median(t), t[0], t[-1], curvature))
        print('ratio fracture_curved / fracture: %.2f (three dot products and four more float64 operations per side test against one dot product)' % (np.median(t) / fr_us))
        print('datapipe.fracture with surfaces, the whole call: %.2f ms per batch on the host clock (min %.2f, max %.2f), valid %d/%d' % (
            np.median(w), w[0], w[-1], int(fc.ok.sum()), B), flush=True)


def bench_pieces(P, reps, curvature):
    from puzzlenet_amd import ops
    B, M, N, K = 64, 10000, 2048, 16
    rng = np.random.RandomState(0)
    raw = torch.from_numpy((rng.rand(B, M, 3) - 0.5).astype(np.float32)).to(dev)
    twin = _again(rng)
    cols = datapipe._fracture_pair_cols(P, K)
    row = np.empty((B, cols[-1].stop))
    datapipe.draw_fracture_pair_batch(rng, torch.Generator().manual_seed(0), B, P, P, K, 0.8, row)
    d = torch.from_numpy(row).to(dev)
    normals, u_anchor = d[:, cols[0]].reshape(B, P - 1, K, 3).contiguous(), d[:, cols[1]].reshape(B, P - 1, K).contiguous()
    pieces, u7, tw = d[:, cols[2]].reshape(B).to(torch.int32), d[:, cols[3]].contiguous(), d[:, cols[4]].contiguous()
    pn, pz, pu = torch.from_numpy(rng.rand(B, K, 3)).to(dev), torch.from_numpy(rng.rand(B, K) / 3 - 0.4).to(dev), torch.from_numpy(rng.rand(B, 2)).to(dev)
    _, ok, rec = datapipe.cut_pairs_fracture(raw, normals, u_anchor, pieces, u7, tw, n=N)
    _, pok, _ = datapipe.cut_pairs(raw, pn, pz, pu, tw, n=N)
    n_nb = int((rec.kind == datapipe.NEIGHBOUR).sum())
    print('fracture pairs, P = %d: valid %d/%d (plane: %d/%d), NEIGHBOUR %d, replaced by the sibling pair %d' % (
        P, int(ok.sum()), B, int(pok.sum()), B, n_nb, int(rec.rejected.sum())), flush=True)
    forms = {"plane: cut_pairs": lambda: datapipe.cut_pairs(raw, pn, pz, pu, tw, n=N),
             "fracture: cut_pairs_fracture (P = %d)" % P: lambda: datapipe.cut_pairs_fracture(raw, normals, u_anchor, pieces, u7, tw, n=N)}
    mc = max(M - N, N)
    p2, c2, s2, _, _ = ops.cut_compact(raw, pn, pz, pu, N, M)
    p4, c4, s4 = ops.fracture_pair(raw, normals, u_anchor, pieces, u7, N, 0.5, M)[:3]
    launches = {"cut_compact (plane)": lambda: ops.cut_compact(raw, pn, pz, pu, N, M),
                "fracture_pair (P = %d)" % P: lambda: ops.fracture_pair(raw, normals, u_anchor, pieces, u7, N, 0.5, M),
                "FPS of the plane pair": lambda: ops.farthest_point_sample(p2, N, s2, background=True, counts=c2, max_count=mc),
                "FPS of the primary pair": lambda: ops.farthest_point_sample(p4[:2 * B], N, s4[:2 * B], background=True, counts=c4[:2 * B], max_count=mc),
                "FPS of the fallback pair (%d of %d samples)" % (n_nb, B):
                    lambda: ops.farthest_point_sample(p4[2 * B:], N, s4[2 * B:], background=True, counts=c4[2 * B:], max_count=mc),
                "FPS of all four rows, one launch (what runs)": lambda: ops.farthest_point_sample(p4, N, s4, background=True, counts=c4, max_count=mc)}
    if curvature > 0:
        ccols = datapipe._fracture_pair_curved_cols(P, K)
        crow = np.empty((B, ccols[-1].stop))
        datapipe.draw_fracture_pair_curved_batch(twin, torch.Generator().manual_seed(0), B, P, P, K, 0.8, curvature, crow)
        c = torch.from_numpy(crow).to(dev)
        frames, half_curv = c[:, ccols[0]].reshape(B, P - 1, K, 3, 3).contiguous(), c[:, ccols[1]].reshape(B, P - 1, K, 2).contiguous()
        c_anchor, c_u7, c_tw = c[:, ccols[2]].reshape(B, P - 1, K).contiguous(), c[:, ccols[4]].contiguous(), c[:, ccols[5]].contiguous()
        assert torch.equal(frames[:, :, :, 2], normals) and torch.equal(c_anchor, u_anchor)
        curved = lambda: datapipe.cut_pairs_fracture(raw, None, c_anchor, pieces, c_u7, c_tw, n=N, frames=frames, half_curv=half_curv)
        _, cok, crec = curved()
        print('curved fracture pairs, P = %d, curvature %g: valid %d/%d, NEIGHBOUR %d, replaced by the sibling pair %d' % (
            P, curvature, int(cok.sum()), B, int((crec.kind == datapipe.NEIGHBOUR).sum()), int(crec.rejected.sum())), flush=True)
        forms["curved: cut_pairs_fracture (P = %d)" % P] = curved
        launches["fracture_pair_curved (P = %d)" % P] = lambda: ops.fracture_pair_curved(raw, frames, half_curv, c_anchor, pieces, c_u7, N, 0.5, M)
    times, ltimes = {name: [] for name in forms}, {name: [] for name in launches}
    for rep in range(reps + 3):                          # (three warm-up rounds of everything; the forms alternate)
        for name, fn in forms.items():
            torch.cuda.synchronize(); t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if rep >= 3:
                times[name].append((time.perf_counter() - t0) * 1e3)
        for name, fn in launches.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize(); e0.record()
            fn()
            e1.record(); e1.synchronize()
            if rep >= 3:
                ltimes[name].append(e0.elapsed_time(e1) * 1e3)
    print('tools/bench_datapipe.py --pieces %d --reps %d: B = %d, M = %d, N = %d, K = %d, neighbours = 0.5 (medians of %d)' % (P, reps, B, M, N, K, reps))
    for name, t in times.items():
        t = np.sort(np.array(t))
        print('%-45s %.2f ms per batch on the host clock (min %.2f, max %.2f)' % (name, np.median(t), t[0], t[-1]), flush=True)
    for name, t in ltimes.items():
        t = np.sort(np.array(t))
        print('launch: %-45s %.0f us between events (min %.0f, max %.0f)' % (name, np.median(t), t[0], t[-1]), flush=True)
    if curvature > 0:
        med = lambda d, name: float(np.median(d[name]))
        print('ratio fracture_pair_curved / fracture_pair: %.2f; ratio of the batches, curved / plane fracture: %.2f' % (
            med(ltimes, "fracture_pair_curved (P = %d)" % P) / med(ltimes, "fracture_pair (P = %d)" % P),
            med(times, "curved: cut_pairs_fracture (P = %d)" % P) / med(times, "fracture: cut_pairs_fracture (P = %d)" % P)), flush=True)


def _events(launches, reps):
    """Every launch alone between two device events, the launches alternating -> {name: sorted microseconds}"""
    lt = {name: [] for name in launches}
    for rep in range(reps + 3):                          # (three warm-up rounds of everything)
        for name, fn in launches.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize(); e0.record()
            fn()
            e1.record(); e1.synchronize()
            if rep >= 3:
                lt[name].append(e0.elapsed_time(e1) * 1e3)
    return {name: np.sort(np.array(t)) for name, t in lt.items()}


def _write_block(lines):
    """Print a mode's block and put it into profiles/fracture_eroded_batch.txt in place of that mode's block of an earlier run"""
    print('\n'.join(lines), flush=True)
    out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'fracture_eroded_batch.txt')
    blocks = [b for b in (open(out).read().split('\n\n') if os.path.exists(out) else []) if b.strip()]
    mode = lines[0].split(' --reps')[0]
    blocks = [b.strip('\n') for b in blocks if not b.startswith(mode)] + ['\n'.join(lines)]
    with open(out, 'w') as fh:
        fh.write('\n\n'.join(sorted(blocks)) + '\n')


def _forms(rng, twin, B, P, K, curvature):
    """The plane draws and (curvature > 0) the curved ones on the same normals and anchors -> {form: keyword arguments of
    datapipe.fracture behind raw, on the device}"""
    up = lambda t: None if t is None else torch.from_numpy(np.ascontiguousarray(t)).to(dev)
    forms = {"planes": {k: up(v) for k, v in datapipe.fracture_arguments(rng, torch.Generator().manual_seed(0), B, P, K, 0.8, 0.0).items()}}
    if curvature > 0:
        forms["surfaces"] = {k: up(v) for k, v in datapipe.fracture_arguments(twin, torch.Generator().manual_seed(0), B, P, K, 0.8, curvature).items()}
    return forms


def bench_fracture_eroded(reps, curvature, erosion, chip):
    from puzzlenet_amd import ops
    B, M, P, K, n, k = 64, 10000, 8, 16, 256, 64
    rng = np.random.RandomState(0)
    raw = torch.from_numpy((rng.rand(B, M, 3) - 0.5).astype(np.float32)).to(dev)
    forms = _forms(rng, _again(rng), B, P, K, curvature)
    erode = torch.from_numpy(datapipe.draw_erosion(rng, B, P, erosion, chip)).to(dev)
    lines = ['tools/bench_datapipe.py --fracture --erosion %g --chip %g %g --reps %d: B = %d, M = %d, P = %d, K = %d, n_min = n = %d, k = %d (medians of %d)' % (
        erosion, chip[0], chip[1], reps, B, M, P, K, n, k, reps)]
    launches = {}
    for name, d in forms.items():
        for tag, kw in (("without erosion", {}), ("eroded", dict(erode=erode))):
            f = datapipe.fracture(raw, n=n, k=k, **d, **kw)
            lost = float(f.lost.sum()) / (B * M) if kw else 0.0
            lines.append('contact, %-8s %-16s valid %d/%d, smallest piece %d, mates per sample %.2f, lost share %.3f' % (
                name + ':', tag + ':', int(f.ok.sum()), B, int(f.counts.min()), float(f.mates.sum()) / 2 / B, lost))
        cut = dict(frames=d["frames"], half_curv=d["half_curv"]) if d["normals"] is None else {}
        if cut:
            launches[name + ": ops.fracture_curved"] = lambda d=d: ops.fracture_curved(raw, d["frames"], d["half_curv"], d["u_anchor"], d["u_start"], n, M)
        else:
            launches[name + ": ops.fracture"] = lambda d=d: ops.fracture(raw, d["normals"], d["u_anchor"], d["u_start"], n, M)
        launches[name + ": ops.fracture_eroded"] = lambda d=d, cut=cut: ops.fracture_eroded(raw, d["normals"], d["u_anchor"], d["u_start"], erode, n, M, **cut)
    lt = _events(launches, reps)
    for name, t in lt.items():
        lines.append('launch: %-34s %.0f us between events (min %.0f, max %.0f)' % (name, np.median(t), t[0], t[-1]))
    names = list(lt)
    for plain, eroded in zip(names[0::2], names[1::2]):
        lines.append('ratio eroded / without, %s: %.2f (one 64-bit sum in place of a 32-bit one per candidate, about ten more float64 operations per member, one more scan for `order`)' % (
            plain.split(':')[0], np.median(lt[eroded]) / np.median(lt[plain])))
    _write_block(lines)


def bench_pieces_eroded(P, reps, curvature, erosion, chip):
    from puzzlenet_amd import ops
    B, M, N, K = 64, 10000, 2048, 16
    rng = np.random.RandomState(0)
    raw = torch.from_numpy((rng.rand(B, M, 3) - 0.5).astype(np.float32)).to(dev)
    forms = _forms(rng, _again(rng), B, P, K, curvature)
    up = lambda t: torch.from_numpy(np.ascontiguousarray(t)).to(dev)
    pieces, u7 = torch.full((B,), P, dtype=torch.int32, device=dev), up(rng.rand(B, ops.FRACTURE_PAIR_UNIFORMS))
    erode = up(datapipe.draw_erosion(rng, B, P, erosion, chip))
    lines = ['tools/bench_datapipe.py --pieces %d --erosion %g --chip %g %g --reps %d: B = %d, M = %d, N = %d, K = %d, neighbours = 0.5 (medians of %d)' % (
        P, erosion, chip[0], chip[1], reps, B, M, N, K, reps)]
    launches, batches = {}, {}
    for name, d in forms.items():
        cut = dict(frames=d["frames"], half_curv=d["half_curv"]) if d["normals"] is None else {}
        tw = d["twist"][:, 0].contiguous()
        for tag, kw in (("without erosion", {}), ("eroded", dict(erode=erode))):
            batch = lambda d=d, cut=cut, kw=kw, tw=tw: datapipe.cut_pairs_fracture(raw, d["normals"], d["u_anchor"], pieces, u7, tw, n=N, **cut, **kw)
            _, ok, rec = batch()
            lines.append('pairs, %-8s %-16s valid %d/%d, NEIGHBOUR %d, replaced by the sibling pair %d, lost share %.3f' % (
                name + ':', tag + ':', int(ok.sum()), B, int((rec.kind == datapipe.NEIGHBOUR).sum()), int(rec.rejected.sum()),
                float(rec.lost.sum()) / (B * M) if kw else 0.0))
            batches['%s: cut_pairs_fracture, %s' % (name, tag)] = batch
        if cut:
            launches[name + ": ops.fracture_pair_curved"] = lambda d=d: ops.fracture_pair_curved(raw, d["frames"], d["half_curv"], d["u_anchor"], pieces, u7, N, 0.5, M)
        else:
            launches[name + ": ops.fracture_pair"] = lambda d=d: ops.fracture_pair(raw, d["normals"], d["u_anchor"], pieces, u7, N, 0.5, M)
        launches[name + ": ops.fracture_pair_eroded"] = lambda d=d, cut=cut: ops.fracture_pair_eroded(raw, d["normals"], d["u_anchor"], pieces, u7, erode, N, 0.5, M, **cut)
    times = {name: [] for name in batches}
    for rep in range(reps + 3):                          # (three warm-up rounds of everything; the forms alternate)
        for name, fn in batches.items():
            torch.cuda.synchronize(); t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if rep >= 3:
                times[name].append((time.perf_counter() - t0) * 1e3)
    lt = _events(launches, reps)
    for name, t in times.items():
        t = np.sort(np.array(t))
        lines.append('%-50s %.2f ms per batch on the host clock (min %.2f, max %.2f)' % (name, np.median(t), t[0], t[-1]))
    for name, t in lt.items():
        lines.append('launch: %-40s %.0f us between events (min %.0f, max %.0f)' % (name, np.median(t), t[0], t[-1]))
    names, bnames = list(lt), list(times)
    for i in range(0, len(names), 2):
        lines.append('ratio eroded / without, %s: launch %.2f, batch %.2f' % (
            names[i].split(':')[0], np.median(lt[names[i + 1]]) / np.median(lt[names[i]]), np.median(times[bnames[i + 1]]) / np.median(times[bnames[i]])))
    _write_block(lines)


if (a.erosion or any(a.chip)) and not (a.fracture or a.pieces):
    sys.exit("--erosion / --chip: with --fracture or --pieces (only a fracture has breaks to erode)")
if a.fracture:
    if a.erosion or any(a.chip):
        bench_fracture_eroded(a.reps, a.curvature, a.erosion, tuple(a.chip))
    else:
        bench_fracture(a.reps, a.curvature)
    sys.exit(0)
if a.pieces:
    if a.erosion or any(a.chip):
        bench_pieces_eroded(a.pieces, a.reps, a.curvature, a.erosion, tuple(a.chip))
    else:
        bench_pieces(a.pieces, a.reps, a.curvature)
    sys.exit(0)
for (B, M, N) in [(64, 6000, 1024), (64, 10000, 2048), (64, 12000, 2048)]:
    raw = (torch.rand(B, M, 3, generator=g) - 0.5).to(dev)
    normal = torch.rand(B, 3, generator=g, dtype=torch.float64).to(dev)
    z = (torch.rand(B, generator=g, dtype=torch.float64) / 3 - 0.4).to(dev)      # cuts that leave both sides populated
    s = torch.zeros(B, dtype=torch.int64, device=dev)
    tw = torch.randn(B, 6, generator=g); tw = (tw / tw.norm(dim=1, keepdim=True) * 0.8).to(dev)
    for _ in range(2):
        out, ok = datapipe.make_pairs(raw, normal, z, s, s, tw, n=N)
    torch.cuda.synchronize()
    t0 = time.perf_counter(); it = 5
    for _ in range(it):
        out, ok = datapipe.make_pairs(raw, normal, z, s, s, tw, n=N)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / it
    print('B=%d M=%d -> N=%d: %.2f ms per batch = %.0f pairs/s (valid cuts %d/%d)' % (B, M, N, dt * 1e3, B / dt, int(ok.sum()), B), flush=True)
# reference-style numpy FPS of one 5000-point piece to 2048 (dataset.py:1147-1163)
pts = (np.random.rand(5000, 3) - 0.5).astype(np.float32)
t0 = time.perf_counter()
distance = np.ones((5000,)) * 1e10; far = 0; cent = np.zeros(2048)
for i in range(2048):
    cent[i] = far
    d = np.sum((pts - pts[far]) ** 2, -1)
    m = d < distance; distance[m] = d[m]; far = np.argmax(distance, -1)
print('numpy FPS 5000 -> 2048 on one host core: %.1f ms per piece' % ((time.perf_counter() - t0) * 1e3))

# the feeder's batch (PairFeeder.next_batch without the host draws and the upload), forms alternating
B, M, N, K = 64, 10000, 2048, 16
rng = np.random.RandomState(0)
raw = (torch.rand(B, M, 3, generator=g) - 0.5).to(dev)
u = torch.from_numpy(rng.rand(B, 2)).to(dev)
tw = torch.randn(B, 6, generator=g, dtype=torch.float64); tw = (tw / tw.norm(dim=1, keepdim=True) * 0.8).to(dev)
normals = torch.from_numpy(rng.rand(B, K, 3)).to(dev)
zs = torch.from_numpy(rng.rand(B, K) / 3 - 0.4).to(dev)
forms = {"plane: cut_pairs": lambda: datapipe.cut_pairs(raw, normals, zs, u, tw, n=N)[1]}
if a.cut != "plane":
    params = torch.from_numpy(datapipe.solid_draws(rng, B, K)).to(dev)
    _, ok, chosen = datapipe.cut_pairs_solid(raw, a.cut, params, u, tw, n=N)
    print('%s: valid cuts among %d candidates %d/%d' % (a.cut, K, int(ok.sum()), B), flush=True)
    rot, shift, s0 = chosen[:, :3].contiguous(), chosen[:, 3:].contiguous(), torch.zeros(B, dtype=torch.int64, device=dev)
    forms[a.cut + ": cut_pairs_solid"] = lambda: datapipe.cut_pairs_solid(raw, a.cut, params, u, tw, n=N)[1]
    forms[a.cut + ": make_pairs_solid (tensor form, one candidate)"] = lambda: datapipe.make_pairs_solid(raw, a.cut, rot, shift, s0, s0, tw, n=N)[1]
launches = {}
if a.random_slice:
    from puzzlenet_amd import ops
    T, Q = ops.DOUBLE_CUT_TRIES, ops.DOUBLE_CUT_UNIFORMS
    normals2, zs2 = torch.from_numpy(rng.rand(B, T, 3)).to(dev), torch.from_numpy(rng.rand(B, T) / 3 - 0.4).to(dev)
    u7 = torch.from_numpy(rng.rand(B, Q)).to(dev)
    _, ok, rec = datapipe.cut_pairs_double(raw, normals, zs, normals2, zs2, u7, tw, n=N)
    print('double cut: valid %d/%d, kinds (single, half vs rest, half vs other, halves) %s, replaced by the fallback %d' % (
        int(ok.sum()), B, torch.bincount(rec.kind.long(), minlength=4).tolist(), int(rec.rejected.sum())), flush=True)
    forms["plane: cut_pairs_double"] = lambda: datapipe.cut_pairs_double(raw, normals, zs, normals2, zs2, u7, tw, n=N)[1]
    # the launches the double cut adds or changes, each alone between two events
    n_rich, mc = 3000 * N // 1024, max(M - N, N)
    p2, c2, s2, _, _ = ops.cut_compact(raw, normals, zs, u, N, M)
    p4, c4, s4 = ops.cut_compact_double(raw, normals, zs, normals2, zs2, u7, N, n_rich, M)[:3]
    launches["cut_compact (plane)"] = lambda: ops.cut_compact(raw, normals, zs, u, N, M)
    launches["cut_compact_double"] = lambda: ops.cut_compact_double(raw, normals, zs, normals2, zs2, u7, N, n_rich, M)
    launches["FPS of the plane pair"] = lambda: ops.farthest_point_sample(p2, N, s2, background=True, counts=c2, max_count=mc)
    launches["FPS of the primary pair"] = lambda: ops.farthest_point_sample(p4[:2 * B], N, s4[:2 * B], background=True, counts=c4[:2 * B], max_count=mc)
    launches["FPS of the fallback pair (%d of %d samples)" % (int((c4[2 * B:3 * B] >= 0).sum()), B)] = \
        lambda: ops.farthest_point_sample(p4[2 * B:], N, s4[2 * B:], background=True, counts=c4[2 * B:], max_count=mc)
times = {name: [] for name in forms}
for rep in range(a.reps + 3):
    for name, fn in forms.items():
        torch.cuda.synchronize(); t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if rep >= 3:                                     # (three warm-up rounds of every form)
            times[name].append(time.perf_counter() - t0)
for name, t in times.items():
    t = np.sort(np.array(t)) * 1e3
    print('B=%d M=%d -> N=%d  %-55s %.2f ms per batch (median of %d; min %.2f, max %.2f)' % (B, M, N, name, np.median(t), len(t), t[0], t[-1]), flush=True)
ltimes = {name: [] for name in launches}
for rep in range(a.reps + 3):
    for name, fn in launches.items():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(); e0.record()
        fn()
        e1.record(); e1.synchronize()
        if rep >= 3:
            ltimes[name].append(e0.elapsed_time(e1))
for name, t in ltimes.items():
    t = np.sort(np.array(t)) * 1e3
    print('B=%d M=%d -> N=%d  launch: %-47s %.0f us between events (median of %d; min %.0f, max %.0f)' % (B, M, N, name, np.median(t), len(t), t[0], t[-1]), flush=True)
