"""End to end on the GPU: resident raw clouds -> datapipe.PairFeeder (plane cut with re-draw, FPS of both pieces, boundary
labels, random motion on a background stream: the reference's loader processes, train.py:101-104 + dataset.py:1165-1190 +
:98-105) -> engine.TrainStep, a fresh batch every step, nothing synchronises.

    python tools/train_from_raw.py [--batch 64] [--points 2048] [--raw 10000] [--steps 20] [--cut {plane,sphere,cylinder,cone}]
                                     [--random_slice] [--pieces P [--pieces_min L] [--neighbours q] [--curvature C]
                                     [--erosion E [--chip DEPTH RADIUS]]]

--cut sphere | cylinder | cone: the reference's mesh cuts (dataset.py:715-759; "bed_sphere" is its documented training
command) in place of the plane.  The cone (apex and base one unit from the origin) holds every point within 0.447 of the
origin, so for it the shells are twice as large.
--random_slice: the reference's flag of the same name (CADDataset(split_twice=True), dataset.py:1203-1355): the double cuts, with
the plane only.
--pieces P [--pieces_min L] [--neighbours q]: pairs cut out of fractures of L .. P pieces (L = P without --pieces_min), a share q of
them drawn among all final pieces (PairFeeder(pieces=(L, P), neighbours=q)); with the plane only, without --random_slice.
--curvature C (with --pieces; default 2.0, the curvature of the reference's radius-0.5 sphere): the fractures break along curved
surfaces with principal curvatures in [-C, C] (PairFeeder(..., curvature=C)); 0: along planes.
--erosion E [--chip DEPTH RADIUS] (with --pieces; default 0: off): material is lost along every break of the fractures, a band of up
to E on either side and a chip of up to DEPTH within RADIUS of the anchor (PairFeeder(..., erosion=E, chip=(DEPTH, RADIUS))), so
the training pairs no longer mate perfectly.
"""
import argparse, os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import Cfg
from puzzlenet_amd import datapipe, engine, model5_b

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--points", type=int, default=2048)
ap.add_argument("--raw", type=int, default=10000)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--cut", choices=["plane", "sphere", "cylinder", "cone"], default="plane")
ap.add_argument("--random_slice", action="store_true")
ap.add_argument("--pieces", type=int, default=0)
ap.add_argument("--pieces_min", type=int, default=0)
ap.add_argument("--neighbours", type=float, default=0.5)
ap.add_argument("--curvature", type=float, default=2.0)
ap.add_argument("--erosion", type=float, default=0.0)
ap.add_argument("--chip", type=float, nargs=2, default=None, metavar=("DEPTH", "RADIUS"))
a = ap.parse_args()
pieces = None if not a.pieces else (a.pieces_min or a.pieces, a.pieces)
curvature = a.curvature if pieces else None      # (the feeder refuses a curvature without pieces: the other cuts have none)
erosion = dict(erosion=a.erosion, chip=a.chip) if a.erosion or a.chip else {}      # (and an erosion: only a fracture has breaks)
dev = torch.device("cuda:0")
B, N, M = a.batch, a.points, a.raw
rng = np.random.RandomState(0)
u = rng.randn(B, M, 3).astype(np.float32)
u /= np.linalg.norm(u, axis=2, keepdims=True)
raw = (u * (0.25 + 0.2 * rng.rand(B, 1, 3).astype(np.float32))).astype(np.float32)      # ellipsoid shells, one per sample
if a.cut == "cone":
    raw *= 2
cfg = Cfg(); cfg.num_points = N
torch.manual_seed(0)
model = model5_b.TouchedRegraster(cfg).to(dev)
feeder = datapipe.PairFeeder(raw, dev, n=N, seed=0, cut=a.cut, split_twice=a.random_slice, pieces=pieces, neighbours=a.neighbours,
                             curvature=curvature, **erosion)
runner = engine.TrainStep(model, feeder.next_batch(), cfg.lr, world=1)
nxt = feeder.next_batch()
losses, mem, oks, doubles, fractures = [], [], [nxt.ok], [nxt.double], [nxt.fracture]
for it in range(a.steps + 3):
    if it == 3:
        torch.cuda.synchronize(); t0 = time.perf_counter()
    losses.append(runner.step(next_batch=nxt))
    nxt = feeder.next_batch()
    oks.append(nxt.ok)
    doubles.append(nxt.double)
    fractures.append(nxt.fracture)
    if it % 50 == 0:
        mem.append(torch.cuda.memory_allocated() >> 20)      # (no synchronisation: the allocator's own count)
torch.cuda.synchronize()
dt = time.perf_counter() - t0
print("loss first / last: %.4f / %.4f" % (float(losses[0]), float(losses[-1])))
ls = torch.stack([l.detach().float().reshape(()) for l in losses])
print("every loss finite:", bool(torch.isfinite(ls).all()), " MiB allocated every 50 steps:", mem)
print("cut %s: every batch cut validly:" % a.cut, all(bool(o.all()) for o in oks))
if a.random_slice:
    kinds = torch.bincount(torch.cat([d.kind for d in doubles]).long(), minlength=4).tolist()
    print("double cuts: single / half vs rest / half vs other / halves:", kinds, " pairs replaced by their fallback:",
          int(torch.cat([d.rejected for d in doubles]).sum()))
if pieces:
    kinds = torch.bincount(torch.cat([f.kind for f in fractures]).long(), minlength=2).tolist()
    print("fractures of %d .. %d pieces: sibling / neighbour pairs:" % pieces, kinds, " neighbour pairs replaced by the sibling pair:",
          int(torch.cat([f.rejected for f in fractures]).sum()))
print("%.2f ms per step of %d fresh pairs from %d-point raw clouds = %.0f pairs/s" % (1e3 * dt / a.steps, B, M, B * a.steps / dt))
runner.close(); feeder.close()
