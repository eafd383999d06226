"""Inputs that the tests of the progressive pose graph share (ops.progressive_joints, assembly.progressive_joints_rule,
assembly.refine_progressive_batch): tests/test_progressive_joints_cpu.py and tests/test_gpu_progressive_joints.py.  Nothing here is
tuned to the kernel.

  planted(K, seed)             a puzzle whose contacts are known, its ledger and drifted start poses
  as_puzzle(pl, outputs)       the rule's (or the kernel's) outputs of one puzzle as a tests/_joint_ref.Puzzle of ragged sets
  purity(pl, outputs)          the share of the set rows that belong to their joint's planted contact
  simulate(rng, Z, P, N, k)    random merge orders on the host: ledgers with parts on both sides, -1 rounds, -1 padding
  lattice()                    nearest neighbours decided by exact ties

The planted puzzle.  K pieces with random true poses; the contact graph is the chain (p, p + 1), the closing edge (0, K - 1) and 2
random chords: K + 2 contacts (6, 8 and 10 at K = 4, 6, 8).  Every contact is one tests/_icp_ref.curve of M = 40 points in a random
orientation at a random place, and BOTH sides hold the same samples in another order, each with its own 0.001 noise.  Independently
sampled sides (planted(..., same=False)) are not used at M = 40: there the energy floor is the sample spacing, not the pose - under
the float64 loop of tests/_joint_ref.py, 30 sweeps, the energies only went 2.2e-2..6.9e-2 -> 1.6e-2..5.5e-2, the largest pose
error was still 0.063 afterwards and it rose in one of the 24 puzzles (with another generator of such inputs, in 5 of 24) - a
property of those inputs, not of the rule.  With the same samples on both sides the same loop lowered the largest pose error in 24
of 24 (K = 4, 6, 8, seeds 0..7), e.g. 0.026 -> 0.0005 and 0.134 -> 0.052, the latter the worst value after it (K = 8, seed 7); at
least 0.989 of every puzzle's set rows belonged to their planted contact, and the energies went 1.8e-3..3.6e-2 -> 6.2e-5..2.0e-3
(tests/test_progressive_joints_cpu.py asserts all of it).  A piece is the concatenation of its contacts' points in its own frame
(float32).  The ledger: round r merges piece r + 1 into the part {0..r}; its fixed list is the shuffled fixed-side points of every
contact between the two, padded with (-1, -1) to k = 4 M, the moved list likewise.  Start poses: the truth with a drift that
accumulates along the chain, per step up to 3 degrees about the piece's centre and up to 0.008 per axis, composed.

The comparison of a short trajectory with the float64 loop (tests/test_gpu_joint_counts.py's check: its margin rule, its tolerance)
needs nearest neighbours that float32 cannot decide otherwise.  Among the 400 to 800 set rows of a puzzle at M = 40 one always
lies almost halfway between two rows of the other side: the smallest margin the float64 loop met in two sweeps was 0.08 to 8.8
distance bounds, below the rule's 16 in all 24 puzzles, so the rule leaves every one of them out.  The same puzzles at SHORT_M = 8
points a contact (planted(..., m=SHORT_M), seeds of their own) are what that comparison runs on: 22 of the 24 enter, which
tests/test_progressive_joints_cpu.py asserts.
"""
import collections

import numpy as np

from tests import _icp_ref as ref
from tests import _joint_ref as jr

M = 40                       # points per contact and side
SHORT_M = 8                  # the same for the short-trajectory comparison (the header says why)
SHORT_ENTERED = 22           # of the 24 puzzles at SHORT_M, those the margin rule lets in (float64 only; asserted on the CPU)
CHORDS = 2
NOISE = 0.001
DRIFT_ANGLE, DRIFT_SHIFT = np.deg2rad(3.0), 0.008
CASES = [(K, seed) for K in (4, 6, 8) for seed in range(8)]
CONTACTS = {4: 6, 6: 8, 8: 10}

Planted = collections.namedtuple("Planted", "K N k contacts pieces own G0 truth dropped part")


def planted(K, seed, same=True, m=M):
    """same=False: the two sides of a contact are sampled independently (the header says why no test uses that); m: the points
    per contact and side.
    -> Planted: contacts [(i, j)] with i < j; pieces [K,N,3] float32 (N = the largest piece, shorter ones padded with copies
    of a far point that no list names); own [K,N] int (the contact of every row, -1 on padding); G0, truth [K,4,4] float64 in
    piece 0's frame (G0[0] = truth[0] = the identity); dropped [K-1,2,k,2] int64; part [K] (all 0)."""
    rng = np.random.default_rng(91000 + 100 * K + seed + 10000 * (m != M))
    contacts = [(p, p + 1) for p in range(K - 1)] + [(0, K - 1)]
    free = [(i, j) for i in range(K) for j in range(i + 1, K) if (i, j) not in contacts]
    contacts += [free[c] for c in sorted(rng.choice(len(free), size=min(CHORDS, len(free)), replace=False))]
    world = np.stack([ref.rigid(ref.rot(rng.normal(size=3), rng.uniform(0.3, 2.5)), rng.uniform(-0.3, 0.3, 3)) for _ in range(K)])
    rows = [[] for _ in range(K)]                 # per piece: (contact, points in the root frame)
    for c, (i, j) in enumerate(contacts):
        W = ref.rot(rng.normal(size=3), rng.uniform(0, np.pi))
        place = rng.uniform(-0.5, 0.5, 3)
        base = ref.curve(rng.uniform(0, 1, m), bool(c & 1)) @ W.T + place
        rows[i].append((c, base + rng.normal(scale=NOISE, size=(m, 3))))
        other = base[rng.permutation(m)] if same else ref.curve(rng.uniform(0, 1, m), bool(c & 1)) @ W.T + place
        rows[j].append((c, other + rng.normal(scale=NOISE, size=(m, 3))))
    N = max(sum(len(x) for _, x in r) for r in rows)
    pieces = np.full((K, N, 3), 50.0, dtype=np.float32)
    own = np.full((K, N), -1, dtype=np.int64)
    centre = np.zeros((K, 3))
    for p in range(K):
        pts = np.concatenate([x for _, x in rows[p]])
        centre[p] = pts.mean(axis=0)
        pieces[p, :len(pts)] = ref.transform(jr._inverse(world[p]), pts).astype(np.float32)
        own[p, :len(pts)] = np.concatenate([np.full(len(x), c) for c, x in rows[p]])
    to0 = jr._inverse(world[0])                    # the part lives in piece 0's frame
    truth = np.stack([to0 @ world[p] for p in range(K)])
    G0, drift = truth.copy(), np.eye(4)
    for p in range(1, K):
        c = ref.transform(to0, centre[p][None])[0]
        Rp = ref.rot(rng.normal(size=3), rng.uniform(-DRIFT_ANGLE, DRIFT_ANGLE))
        drift = ref.rigid(Rp, c - Rp @ c + rng.uniform(-DRIFT_SHIFT, DRIFT_SHIFT, 3)) @ drift
        G0[p] = drift @ truth[p]
    k = 4 * m
    dropped = np.full((K - 1, 2, k, 2), -1, dtype=np.int64)
    for r in range(K - 1):
        q = r + 1
        sides = ([], [])
        for c, (i, j) in enumerate(contacts):
            if j == q and i <= r:
                sides[0].extend((i, int(n)) for n in np.flatnonzero(own[i] == c))
                sides[1].extend((q, int(n)) for n in np.flatnonzero(own[q] == c))
        for s in range(2):
            assert 0 < len(sides[s]) <= k
            dropped[r, s, :len(sides[s])] = np.array(sides[s])[rng.permutation(len(sides[s]))]
    return Planted(K, N, k, contacts, pieces, own, G0, truth, dropped, np.zeros(K, dtype=np.int32))


def as_puzzle(pl, outputs, z=0):
    """Puzzle z of the seven outputs (joints, a, b, na, nb, rows_a, rows_b) as a tests/_joint_ref.Puzzle: the used rows in slot
    order, the sets cut to their counts, G0 rounded to float32, every piece but 0 movable -> (Puzzle, the slots used)."""
    joints, a, b, na, nb = (np.asarray(x) for x in outputs[:5])
    used = [e for e in range(joints.shape[1]) if joints[z, e, 0] >= 0]
    P = jr.Puzzle(pl.K, [tuple(int(v) for v in joints[z, e]) for e in used], [a[z, e, :na[z, e]] for e in used],
                  [b[z, e, :nb[z, e]] for e in used], pl.G0.astype(np.float32), pl.truth, np.arange(pl.K) > 0)
    return P, used


def short_trajectory(pl, outputs, sweeps, factor):
    """The float64 loop over `sweeps` sweeps on the sets of `outputs` -> (its _joint_ref.JointRefined, whether the margin rule
    lets the puzzle in: every nearest-neighbour margin it met is at least `factor` distance bounds)."""
    want = jr.refine(as_puzzle(pl, outputs)[0], sweeps)
    return want, want.margin_ratio >= factor


def purity(pl, outputs, z=0):
    """The share of the set rows (both sides, all joints) that belong to the planted contact of their joint's pair."""
    joints, _, _, na, nb, rows_a, rows_b = (np.asarray(x) for x in outputs)
    good = total = 0
    for e in range(joints.shape[1]):
        p, q = (int(v) for v in joints[z, e])
        if p < 0:
            continue
        c = pl.contacts.index((min(p, q), max(p, q))) if (min(p, q), max(p, q)) in pl.contacts else -2
        for piece, rows, n in ((p, rows_a, na), (q, rows_b, nb)):
            got = pl.own[piece, rows[z, e, :n[z, e]]]
            good += int((got == c).sum())
            total += len(got)
    return good / max(total, 1)


Simulated = collections.namedtuple("Simulated", "pieces G dropped part opposite")


def simulate(rng, Z, P, N, k, stop=0.25, pad=0.3, spread=0.6):
    """Z random walks on the host -> Simulated(pieces [Z,P,N,3] float32, G [Z,P,4,4] float64, dropped [P-1,Z,2,k,2] int64, part
    [Z,P] int32, opposite [Z] sets of unordered pairs some round put on opposite sides).  Every round a puzzle merges two random
    live parts - both may hold several pieces - or, with probability `stop`, stops for good (its later rounds are all -1, so
    its walk ends with several parts).  A merge's lists: k (piece, row) pairs drawn from the members of each part, of which
    every entry is -1 padding with probability `pad` (never a whole side).  The poses are random rigid motions near the
    identity and the points uniform in a cube of side `spread`, so the parts overlap and nearest neighbours fall on every member."""
    pieces = rng.uniform(-spread / 2, spread / 2, size=(Z, P, N, 3)).astype(np.float32)
    G = np.stack([[ref.rigid(ref.rot(rng.normal(size=3), rng.uniform(-0.5, 0.5)), rng.uniform(-0.1, 0.1, 3)) for _ in range(P)]
                  for _ in range(Z)])
    dropped = np.full((P - 1, Z, 2, k, 2), -1, dtype=np.int64)
    part = np.tile(np.arange(P, dtype=np.int32), (Z, 1))
    opposite = [set() for _ in range(Z)]
    stopped = np.zeros(Z, dtype=bool)
    for r in range(P - 1):
        for z in range(Z):
            stopped[z] |= r > 0 and rng.uniform() < stop
            if stopped[z]:
                continue
            i, j = (int(s) for s in rng.choice(np.unique(part[z]), size=2, replace=False))
            for s, slot in ((0, i), (1, j)):
                members = np.flatnonzero(part[z] == slot)
                keep = rng.uniform(size=k) >= pad
                keep[rng.integers(k)] = True
                pi = rng.choice(members, size=k)
                dropped[r, z, s, keep, 0] = pi[keep]
                dropped[r, z, s, keep, 1] = rng.integers(0, N, size=k)[keep]
            opposite[z] |= {(min(p, q), max(p, q)) for p in np.flatnonzero(part[z] == i) for q in np.flatnonzero(part[z] == j)}
            part[z][part[z] == j] = i
    return Simulated(pieces, G, dropped, part, opposite)


def lattice():
    """One puzzle of P = 3 pieces whose nearest neighbours are decided by exact ties: every point has small integer coordinates,
    every pose is the identity, so every distance is an exact integer.  Round 0 merges piece 1 into piece 0, round 1 merges
    piece 2 into the part {0, 1}.  In round 1 every moved point (piece 2, at x = 1) lies exactly between a point of piece 0 (x = 0)
    and a point of piece 1 (x = 2) at the same (y, z): the tie goes to the lower list position, and the fixed list alternates
    the two pieces, so which piece wins changes from point to point -> (pieces [1,3,N,3], G [1,3,4,4], dropped [2,1,2,k,2],
    want: {moved row: the fixed piece it must face})."""
    n = 6
    N, k = n, 2 * n
    pieces = np.zeros((1, 3, N, 3), dtype=np.float32)
    for y in range(n):
        pieces[0, 0, y] = (0, y, 0)
        pieces[0, 1, y] = (2, y, 0)
        pieces[0, 2, y] = (1, y, 0)
    G = np.tile(np.eye(4), (1, 3, 1, 1))
    dropped = np.full((2, 1, 2, k, 2), -1, dtype=np.int64)
    # round 0: pieces 0 and 1 row by row (distance 4 to the own row, 5 to its neighbours: no tie)
    dropped[0, 0, 0, :n] = [(0, y) for y in range(n)]
    dropped[0, 0, 1, :n] = [(1, y) for y in range(n)]
    # round 1: the fixed list names row y of piece 0 before row y of piece 1 for even y, after it for odd y
    fixed = []
    for y in range(n):
        fixed += [(0, y), (1, y)] if y % 2 == 0 else [(1, y), (0, y)]
    dropped[1, 0, 0] = fixed
    dropped[1, 0, 1, :n] = [(2, y) for y in range(n)]
    want = {y: (0 if y % 2 == 0 else 1) for y in range(n)}
    return pieces, G, dropped, want
