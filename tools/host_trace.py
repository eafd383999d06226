#!/usr/bin/env python3
"""What the host layer enqueues and what comes out, for comparing two versions of puzzlenet_amd's Python files over ONE built
library, bit for bit.

    python tools/host_trace.py [--root DIR] [--out trace.txt] [--dump tensors.pt]
    python tools/host_trace.py --diff a.pt b.pt
    python tools/host_trace.py --table spread.txt other.txt [...]

The first form runs, on the closed-form weights of oracle.model_ref.fill_params and the ts_batch* tensors of
tests/golden/loss.npz, with seeded global and private generators:
  (a) predict5(training=False, need=True);
  (b) two engine.TrainStep.step() calls with the plan prefetch on, with two_streams on and then off (a fresh model each);
  (c) match_pairs on the first 3 clouds, refine = 0 and refine = 5;
  (d) assemble_progressive on the same 3 clouds.
It wraps ops._call and prints, per section and per stream (numbered in the order the section first uses them), the sequence of
(entry point, integer arguments), then the sha256 of every output tensor, of the losses and of every parameter gradient; the
last line of each section is the sha256 of its call sequences.  --root: the directory puzzlenet_amd is imported from (another
version's Python files beside a copy of the same libpzn.so and include/); --dump: the tensors themselves, for --diff.
The second form prints, per tensor, the largest element difference between two dumps; the third sets such outputs side by
side: the first is the spread between one version's own two runs, every other one is held to it (the same bits where the
spread is 0, within 4 x the spread elsewhere)."""
import argparse
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def sha(t):
    return hashlib.sha256(np.ascontiguousarray(t.detach().cpu().numpy()).tobytes()).hexdigest()[:16]


class Trace:
    def __init__(self, ops, out):
        self.ops, self.out, self.tensors = ops, out, {}
        self.real = ops._call
        self.calls = None
        ops._call = self._spy

    def _spy(self, name, *args, **kw):
        if self.calls is not None:
            ints = tuple(a for a in args if isinstance(a, int) and not isinstance(a, bool) and 0 <= a < (1 << 31))
            self.calls.setdefault(self.ops._stream(), []).append((name, ints))
        return self.real(name, *args, **kw)

    def section(self, tag, fn):
        """fn() -> {name: tensor}; prints the section's per-stream call sequences and its tensors' hashes."""
        self.calls = {}
        named = fn()
        torch.cuda.synchronize()
        calls, self.calls = self.calls, None
        h = hashlib.sha256()
        print(f"== {tag}", file=self.out)
        for k, seq in enumerate(calls.values()):
            print(f"-- stream {k}: {len(seq)} calls", file=self.out)
            for name, ints in seq:
                line = f"{name} {' '.join(map(str, ints))}"
                h.update(f"{k} {line}\n".encode())
                print(f"   {line}", file=self.out)
        for name, t in named.items():
            self.tensors[f"{tag}/{name}"] = t.detach().cpu()
            print(f"## {tag}/{name} {tuple(t.shape)} {sha(t)}", file=self.out)
        print(f"== {tag} call sequences {h.hexdigest()[:16]}", file=self.out)


def run(args):
    sys.path.insert(0, ROOT)
    if args.root:
        sys.path.insert(0, os.path.abspath(args.root))
    from oracle import model_ref as mr
    from puzzlenet_amd import assembly, engine, model5_b, ops
    out = open(args.out, "w") if args.out else sys.stdout
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    G = np.load(os.path.join(ROOT, "tests", "golden", "loss.npz"))
    batch = [torch.from_numpy(np.ascontiguousarray(G[f"ts_batch{i}"])).to(dev) for i in range(8)]
    tr = Trace(ops, out)

    def model(two_streams=True):
        m = model5_b.TouchedRegraster(mr.Cfg(loss_mode=1, use_emd2=True, use_cd2=True, use_emd3=True))
        mr.fill_params(m)
        m.to(dev)
        m.two_streams = two_streams
        m.fps_generator = torch.Generator().manual_seed(101)
        ops.clear_grad_sinks()
        torch.manual_seed(7)
        return m

    def predict():
        m = model()
        with torch.no_grad():
            r = m.predict5(batch, batch[0].shape[0], need=True, training=False)
        return {n: t for n, t in zip("out _ x2 attention mrpc_x2 mrpc_attention de_fpcb de_mrpcb".split(), r) if n != "_"}
    tr.section("a predict5", predict)

    for two in (True, False):
        def steps():
            m = model(two)
            named = {}
            with engine.TrainStep(m, batch, 1e-3, world=1, prefetch=True, fps_generator=m.fps_generator) as r:
                for k in range(2):
                    named[f"step{k}/loss"] = r.step().detach().clone()
                    torch.cuda.synchronize()
                    for n, p in m.named_parameters():
                        if p.grad is not None:
                            named[f"step{k}/grad/{n}"] = p.grad.detach().clone()
            return named
        tr.section(f"b train two_streams={two}", steps)

    pieces = batch[0][:3].contiguous()
    for refine in (0, 5):
        tr.section(f"c match_pairs refine={refine}",
                   lambda: {n: t for n, t in assembly.match_pairs(model(), pieces, refine=refine)._asdict().items()})

    def progressive():
        p = assembly.assemble_progressive(model(), pieces, generator=torch.Generator().manual_seed(9))
        named = {"G": torch.from_numpy(p.G), "cloud": p.cloud, "piece_id": p.piece_id, "row_id": p.row_id, "parts": p.parts}
        named["edges"] = torch.tensor([[e[0], e[1], e[2]] for e in p.edges], dtype=torch.float64).reshape(-1, 3)
        return named
    tr.section("d assemble_progressive", progressive)
    if args.dump:
        torch.save(tr.tensors, args.dump)
    if args.out:
        out.close()


def diff(a, b):
    A, B = torch.load(a), torch.load(b)
    assert list(A) == list(B), "the two dumps hold different tensors"
    for k in A:
        x, y = A[k].double(), B[k].double()
        same = x.shape == y.shape and torch.equal(A[k], B[k])
        if x.shape != y.shape:
            d = float("nan")
        else:      # (equal elements differ by 0, the +inf of a masked diagonal too)
            d = float(torch.where(x == y, torch.zeros_like(x), x - y).abs().max()) if x.numel() else 0.0
        print(f"{'same' if same else 'DIFF'} {d:.6e} {float(x.abs().max()) if x.numel() else 0.0:.6e} {k}")


def table(spread, others):
    """The --diff output of one version's two runs (its spread) beside the --diff outputs of other pairs of runs: per tensor
    the spread, each other difference, and the verdict on each: `same` bits where the spread is 0, else within 4 x spread."""
    rows = [[ln.split(None, 3) for ln in open(f).read().splitlines()] for f in [spread] + list(others)]
    print("tensor | spread (" + spread + ") | " + " | ".join(others))
    bad = [0] * len(others)
    for per in zip(*rows):
        s = float(per[0][1])
        cells = []
        for k, o in enumerate(per[1:]):
            assert o[3] == per[0][3]
            d = float(o[1])
            ok = o[0] == "same" if per[0][0] == "same" else d <= 4 * s
            bad[k] += not ok
            cells.append(f"{d:.3e} {'ok' if ok else 'BITS DIFFER' if per[0][0] == 'same' else f'{d / s:.1f}x' if s else 'over 0'}")
        print(f"{per[0][3]} | {s:.3e} | " + " | ".join(cells))
    print("not held: " + ", ".join(f"{o}: {b} of {len(rows[0])}" for o, b in zip(others, bad)))


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--root")
    ap.add_argument("--out")
    ap.add_argument("--dump")
    ap.add_argument("--diff", nargs=2, metavar=("A", "B"))
    ap.add_argument("--table", nargs="+", metavar="DIFF", help="the --diff output of the spread, then those held against it")
    a = ap.parse_args()
    if a.table:
        table(a.table[0], a.table[1:])
    elif a.diff:
        diff(*a.diff)
    else:
        run(a)
