"""Multi-piece assembly: match every ordered pair of K pieces with each piece encoded ONCE, then
put the pieces together by the distance between the matched boundaries (the reference's README describes this end use and
ships no code for it).  Every device function takes Z puzzles at once; the per-puzzle functions are the same code at Z = 1.

In eval mode nothing in predict5 mixes batch rows (BatchNorm1d(num_points) uses its running statistics, everything else
is per row), so the all-pairs table factors exactly.

Per piece (encode_pieces -> PieceCodes, one call over all Z K pieces, so the encoders see full batches):
  * Encoder and Encoder2 run once per piece (2 K encoder rows instead of 2 K (K - 1)) on ONE sampling / neighbour plan per
    piece: FPS and kNN depend on coordinates only.
  * Pose head: the first tfMLP layer on cat([ffpc_i, fmrpc_j]) is U_i + V_j with U = ffpc W1[:, :1024]^T and
    V = fmrpc W1[:, 1024:]^T + b1.
  * Moved-side boundary head: both "global" vectors are the max over the MOVED piece's local features (TouchedRegraster.moved_branch,
    the reference's line 741), so de_mrpcb and its top-k depend on j only: K rows.

Per pair (pair_block_batch -> PairBlock, the one statement of these stages, block-diagonal over the puzzles; pair_block is
its Z = 1 case):
  * the other four pose-head layers on the rows relu(U_i + V_j), then se3.exp;
  * Fixed-side boundary head: de_fpcb[i, j] = MLPFpcb(cat([g_j, local_i])), the only per-point work that depends on the
    pair: one launch of ops.pair_head_blocks (csrc/pointmlp.hip, pair_head_fwd_kernel), which computes the first-layer
    product of a tile once and loops over the moved pieces in registers (_pair_fixed_head, with the fallback for other shapes);
  * softmax, top-k, one gather per side, then the transform and the chamfer: the score of a pair;
  * refine = N > 0 instead of those two: every pair pose moves to where the two picked boundaries meet, symmetric
    point-to-point ICP on the k picked points of each side, all pairs in ONE launch (_refine_gathered: ops.icp_refine,
    csrc/icprefine.hip; refine_pairs is the same on boundaries the caller names), at most N accepted steps from the network's
    pose.  It lowers exactly the quantity the walks rank by, so T and score are the refined ones (score never above the
    unrefined chamfer of the same rows); twist stays the network's output (the project has no SE(3) logarithm).  refine = 0
    is the default, and not one launch more.

The table: match_puzzles is one encode_pieces, one square pair_block_batch and the diagonal fill (_match_puzzles, _table);
match_pairs is match_puzzles on pieces[None].

The walks over a table:
  * assemble: greedy, on the host in float64 - the reference the device walks are tested against, as evaluate is for
    evaluate_batch.
  * assemble_batch: the greedy walk and the joint list of Z puzzles in one launch (ops.assemble_walk, csrc/assemblewalk.hip;
    walk_rule is its numpy statement).
  * assemble_beam_batch: a beam in place of the greedy walk, which takes the smallest entry every round and never checks it.
    `beam` hypotheses live side by side, each extended by its `branch` smallest entries, and a child pays its entry's score
    plus `weight` times what the entries of the other placed pieces say against its pose - how far apart, in the mean square,
    the two predictions put the new piece's picked boundary points, read off one 4x4 second-moment matrix per piece
    (boundary_moments) -: the cycles a spanning tree never asks.  One launch (ops.assemble_beam, csrc/assemblebeam.hip;
    beam_rule is its numpy statement).
  * assemble_forest_batch: the greedy walk for a pile that holds the pieces of several objects.  The walks above grow one tree
    from one root and leave what it does not reach unplaced; here the pieces left over start a new component from a new root,
    until every piece is in one - which pieces belong together, and how each group goes together.  One launch
    (ops.assemble_forest, csrc/assemblewalk.hip; forest_rule is its numpy statement).  evaluate_pile / evaluate_pile_batch
    score a sorted pile against datapipe.pile's answers.
  * assemble_forest_beam_batch: the beam for such a pile.  The forest walk is greedy inside every component, and the beam grows
    one tree; here a beam hypothesis that finds no admissible entry restarts from a new root as the forest walk does, at the
    price `restart_cost` (by default max_score, what single linkage under a threshold charges a component), and a piece is
    charged by the votes of the component it joins alone.  One launch (ops.assemble_forest_beam, csrc/assemblebeam.hip;
    forest_beam_rule is its numpy statement); beam = branch = 1 is the forest walk, a table without a restart gives the beam.
  * refine_assembly / refine_assembly_batch: the step after a walk.  The walk composes pair poses along a spanning tree, so a
    piece's pose carries the summed error of the edges between it and the root, and every accepted joint that is no tree edge
    is never asked.  The placed assembly is a pose graph - every ordered pair of placed pieces whose table score is no larger
    than the worst tree edge's is a joint - and all pieces but the root move so that the joints close together:
    block-coordinate descent that can only lower the summed score, one launch (ops.joint_refine, csrc/jointrefine.hip).
    refine_assembly chooses the joints on the host and gathers only their sets; the batch form reads them from the walk's
    output on the device.
  * evaluate / evaluate_batch: the score of an assembly against datapipe.fracture's ground truth.

The progressive walks do what the walks above leave out - those never look at a merged shape -: every round the pair of the
smallest score is merged on the device (ops.merge_resample: the moved part under its pose, the union resampled to N points by
farthest point sampling with the matched boundary points left out, the origin of every point kept), the merged part is
encoded alone - its sampling plan is read off its pick order, no FPS - and only its row and its column of the table are
computed again (two pair_block calls).  ProgressiveAssembler walks one puzzle with the choice and the ledger on the host
(MergeLedger) and compacts its state; ProgressiveBatch walks Z puzzles in lockstep, P - 1 rounds with nothing waiting for the
device: one ops.progressive_round launch chooses all Z merges and books them in a float64 ledger on the device
(csrc/progressive.hip; progressive_round_rule is its numpy statement; slots die instead of being compacted, so shapes never
change), one ops.merge_resample launch, one encode_pieces call and two pair_block_batch calls.  Not done there: dead slots
are still paired and stopped puzzles are still encoded.  refine_progressive / refine_progressive_batch are the step after
such a walk: the rows every merge left out say which pieces meet across it, one launch reads the pose graph off them
(ops.progressive_joints, csrc/progjoints.hip; progressive_joints_rule is its numpy statement) and one ops.joint_refine
launch closes it, every piece but its part's frame piece moving.

Inference only: eval mode, torch.no_grad(), fp32, one GPU.  Out of scope: any training on merged parts or on more than two
pieces, a beam or several merges per round of the progressive walk, undoing a merge, and more than one GPU.
"""
import collections
import math
import numbers

import numpy as np
import torch

from . import _lib, ops, se3
from .model5_b import draw_fps_starts, pick_order_plan, run_seq, run_seq_cat_global, sampling_plan, upload_starts

class PairTable(collections.namedtuple("PairTable", "twist T de_fpcb de_mrpcb top_f top_m score x2")):
    __slots__ = ()
    kept_f = kept_m = None      # (no field: a table that carries kept sets is a TrimmedPairTable, below)



Assembly = collections.namedtuple("Assembly", "root edges G placed")
PieceCodes = collections.namedtuple("PieceCodes", "U V local_f g_max de_mrpcb top_m x2")
class PairBlock(collections.namedtuple("PairBlock", "twist T de_fpcb top_f score")):
    __slots__ = ()
    kept_f = kept_m = None


class Refined(collections.namedtuple("Refined", "T score score0 iters_used")):
    __slots__ = ()
    kept_f = kept_m = None



JointRefined = collections.namedtuple("JointRefined", "G score score0 sweeps_used accepted joints")
Progressive = collections.namedtuple("Progressive", "G edges placed cloud piece_id row_id parts")
# refine_assembly(..., keep=) / refine_assembly_batch(..., keep=): JointRefined's fields, then per joint row kept_f [...,J,k] and
# kept_m [...,J,k] (int32: positions into top_f[i,j] / top_m[j] of the rows kept under the returned poses, ascending, -1 behind
# the count and throughout an unused row) and count_f, count_m [...,J] (int32: the counts the rows were given; an unused row's
# mean nothing)
TrimmedJointRefined = collections.namedtuple("TrimmedJointRefined", JointRefined._fields + ("kept_f", "kept_m", "count_f", "count_m"))
# refine_assembly(..., auto=) / refine_assembly_batch(..., auto=): TrimmedJointRefined's fields - count_f, count_m are the counts
# FOUND under the returned poses (0 on an unused row), score and score0 the trimmed energy at the counts found - then objective
# and objective0, the F the refinement lowered under G and under asm.G (objective <= objective0; score need not fall)
AutoJointRefined = collections.namedtuple("AutoJointRefined", TrimmedJointRefined._fields + ("objective", "objective0"))

# keep < 1 (partial contact): the same tuples with the trailing fields kept_f [...,Kf,Km,m_f] and kept_m [...,Kf,Km,m_m].  The
# untrimmed types answer kept_f / kept_m with None and keep their fields, so whatever walks over the fields of today's table
# meets tensors only; code that rebuilds a tuple field by field uses type(t)(...).
TrimmedPairTable = collections.namedtuple("TrimmedPairTable", PairTable._fields + ("kept_f", "kept_m"))
TrimmedPairBlock = collections.namedtuple("TrimmedPairBlock", PairBlock._fields + ("kept_f", "kept_m"))
TrimmedRefined = collections.namedtuple("TrimmedRefined", Refined._fields + ("kept_f", "kept_m"))

# keep = "auto" / AutoKeep(...): the share of every pair is found on the device, per pair and per evaluated pose (include/pzn.h,
# pzn_icp_refine_auto_f32).  The trimmed tuples' fields, then count_f, count_m [...,Kf,Km] (int32: the rows kept of each side
# under T[i,j]) and objective [...,Kf,Km] (the F the refinement lowered); kept_f [...,Kf,Km,k] and kept_m [...,Kf,Km,k] hold the
# kept positions ascending and -1 behind the count.  score stays the trimmed score at those counts: what max_score is held to.
_AUTO_FIELDS = ("count_f", "count_m", "objective")
AutoPairTable = collections.namedtuple("AutoPairTable", TrimmedPairTable._fields + _AUTO_FIELDS)
AutoPairBlock = collections.namedtuple("AutoPairBlock", TrimmedPairBlock._fields + _AUTO_FIELDS)
AutoRefined = collections.namedtuple("AutoRefined", TrimmedRefined._fields + _AUTO_FIELDS)


class AutoKeep(collections.namedtuple("AutoKeep", "least power", defaults=(0.25, 3))):
    """keep=AutoKeep(least, power) on the pair functions (keep="auto" is AutoKeep()): of each side no fewer than ceil(least k)
    rows are kept (least a fraction in (0, 1], or a pair (fixed side, moved side); the rule of a keep fraction), and the count
    m minimises (sum of the m smallest row minima) / m^(power + 1): power = 3 is Trimmed ICP's objective with its published
    lambda = 2, an integer in [1, 4]."""
    __slots__ = ()


_AutoCounts = collections.namedtuple("_AutoCounts", "lo_f lo_m power")      # what _keep_counts makes of an AutoKeep

# The three kinds of a refined pair, by what _keep_counts gives: None - no kept sets; counts (m_f, m_m) - kept sets; _AutoCounts -
# kept sets with counts.  The types of a kind share their extra fields, in one order, behind the base fields.
_Kind = collections.namedtuple("_Kind", "Refined PairBlock PairTable")
_KINDS = (_Kind(Refined, PairBlock, PairTable), _Kind(TrimmedRefined, TrimmedPairBlock, TrimmedPairTable),
          _Kind(AutoRefined, AutoPairBlock, AutoPairTable))


def _kind_of(counts):
    return _KINDS[0 if counts is None else 2 if isinstance(counts, _AutoCounts) else 1]

ENCODER_ROWS = 64      # pieces per encoder call (the fused per-point stem takes up to 64 clouds)


def _encode(enc, pieces, plan):
    """One encoder over all pieces, ENCODER_ROWS at a time -> (global feature [K,1024], per-point features [K,N,64])."""
    outs = []
    for a in range(0, pieces.shape[0], ENCODER_ROWS):
        b = a + ENCODER_ROWS
        sub = tuple((x[a:b], i[a:b]) for x, i in plan)
        r = enc(pieces[a:b], sub, None, False)      # need_out = False: only the maximum of the projection is used
        outs.append((r[0], r[4]))
    if len(outs) == 1:
        return outs[0]
    return tuple(torch.cat(ts, dim=0) for ts in zip(*outs))


def _pair_fixed_head(seq, local, g):
    """MLPFpcb over every (fixed i, moved j) pair of every puzzle: local [Z,Kf,N,64], g [Z,Km,64] -> [Z,Kf,Km,N,2] in one
    pair_head_blocks launch, or (shapes it does not take) one boundary-head call per puzzle and moved piece with its global
    vector expanded over the fixed pieces."""
    mods = list(seq)
    Z, Kf, N = local.shape[0], local.shape[1], local.shape[2]
    if len(mods) == 5 and ops.pair_head_blocks_supported(N, mods[2].out_features, mods[4].out_features):
        l1, l2, l3 = mods[0], mods[2], mods[4]
        return ops.pair_head_blocks(local, g, l1.weight, l1.bias, l2.weight, l2.bias, l3.weight, l3.bias)
    return torch.stack([torch.stack([run_seq_cat_global(seq, local[z], g[z, j:j + 1].expand(Kf, -1).reshape(Kf, 1, -1).contiguous())
                                     for j in range(g.shape[1])], dim=1) for z in range(Z)], dim=0)


def _on_gpu(who, **tensors):
    for name, t in tensors.items():
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise _lib.PznError(f"{who}: {name} must be a tensor on the GPU; puzzlenet_amd has no CPU fallback")


def _clouds(who, lead, **tensors):
    """Every tensor is float32 [*lead, N, 3] on the GPU (lead names the leading dimensions, "K" or "Z,P")."""
    _on_gpu(who, **tensors)
    for name, t in tensors.items():
        if t.dim() != lead.count(",") + 3 or t.shape[-1] != 3 or t.dtype != torch.float32:
            raise _lib.PznError(f"{who} expects float32 {name}[{lead},N,3]; got {t.dtype} {tuple(t.shape)}")


def _check_pieces(model, pieces, k, who, least=1):
    _clouds(who, "K", pieces=pieces)
    K, N, _ = pieces.shape
    if K < least or N != model.num_points:
        raise _lib.PznError(f"{who}: K = {K} pieces (>= {least}) of N = {N} points (the model takes {model.num_points})")
    k = int(k)
    if not 0 < k <= N:
        raise _lib.PznError(f"{who}: k = {k} of {N} points")
    return K, N, k


def encode_pieces(model, pieces, k=128, start=None, plan=None, _who="encode_pieces", _least=1):
    """Everything of the pair table that depends on ONE piece, for pieces [K,N,3] (float32, on the GPU) -> PieceCodes:

      U [K,H], V [K,H]    the fixed and the moved half of the pose head's first layer (V carries the bias)
      local_f [K,N,64]    MLPLocalPreFpc over Encoder's per-point features (the fixed-side boundary head's input)
      g_max [K,64]        the max over MLPLocalPreRpc of Encoder2's per-point features (TouchedRegraster.moved_branch)
      de_mrpcb [K,2,N]    moved-side boundary logits
      top_m [K,k]         their k points of largest class-1 probability
      x2 [K,256,3]        the second-level sample points

    start = (s1[K], s2[K]) as match_pairs takes it; plan = ((x1, idx1), (x2, idx2)) replaces both FPS levels and both
    neighbour searches by a plan the caller already has (start is ignored then).  Encoder2 runs on the model's side stream
    beside Encoder.  Nothing here waits for the device."""
    K, N, k = _check_pieces(model, pieces, k, _who, _least)
    pieces = pieces.contiguous()
    dev = pieces.device
    model.set_mode(False)
    with torch.no_grad():
        if plan is not None:
            pass
        elif start is None:
            plan = sampling_plan(pieces, *upload_starts(draw_fps_starts(1, K, N, getattr(model, "fps_generator", None)), dev), True)
        else:
            s1, s2 = (torch.as_tensor(s, dtype=torch.long).to(dev, non_blocking=True) for s in start)
            if s1.shape != (K,) or s2.shape != (K,):
                raise _lib.PznError(f"{_who}: start = (s1[{K}], s2[{K}]); got {tuple(s1.shape)}, {tuple(s2.shape)}")
            plan = sampling_plan(pieces, s1, s2, True)

        cur = torch.cuda.current_stream(dev)
        side = model.side_stream()
        side.wait_stream(cur)
        with torch.cuda.stream(side):
            # Encoder2 and everything that depends on the moved piece alone: its local chain, the global vector and
            # de_mrpcb (TouchedRegraster.moved_branch)
            fmrpc, local_m = _encode(model.Encoder2, pieces, plan)
            _, g_max, de_mrpcb = model.moved_branch(local_m)                              # [K,1,64], [K,N,2]
        ffpc, local_f = _encode(model.Encoder, pieces, plan)
        local_f = run_seq(model.MLPLocalPreFpc, local_f)
        cur.wait_stream(side)
        for t in (fmrpc, g_max, de_mrpcb):                     # made on the side stream, used on this one
            t.record_stream(cur)
        for t in (pieces,) + tuple(t for lvl in plan for t in lvl):      # made on this stream, read on the side stream
            t.record_stream(side)

        # pose head: the first layer splits into a fixed and a moved half (V carries the bias)
        w1, b1 = model.tfMLP[0].weight, model.tfMLP[0].bias
        ffpc, fmrpc = ffpc.contiguous(), fmrpc.contiguous()
        U = ops.linear_cols(ffpc, w1, 0)
        V = ops.linear_cols(fmrpc, w1, ffpc.shape[1], b1)
        p_m = torch.softmax(de_mrpcb, dim=-1)[..., 1]
        top_m = ops.topk_rows(p_m, k)
    return PieceCodes(U, V, local_f, g_max.squeeze(1), de_mrpcb.permute(0, 2, 1), top_m, plan[1][0])


def _keep_counts(keep, k_f, k_m, who):
    """keep as the pair functions take it - a fraction in (0, 1] of the picked rows, or a pair (fixed side, moved side) of
    such (Python or numpy real numbers) - -> None where every row is kept (today's path), otherwise the counts (m_f, m_m) =
    ceil(f k), at least 1, that ops.icp_refine takes as keep: known on the host, nothing waits for the device.  The product is
    formed in double arithmetic and one within 1e-9 above an integer counts as that integer (0.07 x 100 is 7.000000000000001
    in binary and means 7 rows, not 8).
    keep = "auto" or an AutoKeep -> _AutoCounts(lo_f, lo_m, power), the least counts by the same ceil rule (least = 1.0
    included: the auto launch with every row kept) and the power, an int in [1, 4]: what ops.icp_refine takes as auto."""
    power, shares = None, keep
    if isinstance(keep, str):
        if keep != "auto":
            raise _lib.PznError(f"{who}: keep = {keep!r} (the one word it takes is 'auto')")
        keep = AutoKeep()
    if isinstance(keep, AutoKeep):
        power, shares = keep.power, keep.least
        if not isinstance(power, numbers.Integral) or isinstance(power, (bool, np.bool_)) or not 1 <= power <= 4:
            raise _lib.PznError(f"{who}: keep = {keep!r} (power: an integer in [1, 4])")
    fs = tuple(shares) if isinstance(shares, (tuple, list)) else (shares, shares)
    if len(fs) != 2 or not all(isinstance(f, numbers.Real) and not isinstance(f, (bool, np.bool_)) and 0.0 < f <= 1.0 for f in fs):
        raise _lib.PznError(f"{who}: keep = {keep!r} (a fraction in (0, 1] of the picked rows, or a pair (fixed, moved) of such)")
    if power is None and fs[0] == 1.0 and fs[1] == 1.0:
        return None
    counts = tuple(min(k, max(1, math.ceil(float(f) * k - 1e-9))) for f, k in zip(fs, (int(k_f), int(k_m))))
    return counts if power is None else _AutoCounts(*counts, int(power))


def _refine_gathered(Bf, Bm, T, iters, keep=None):
    """refine_pairs on boundaries that are gathered already, for any leading puzzle dimensions of T [...,Kf,Km,4,4]: Bf
    [Z Kf Km,k,3] per pair, Bm [Z Km,k,3] per moved piece (served to every fixed piece of its puzzle: problem (z, i, j) reads
    Bm[z Km + j]) -> Refined with T's leading dimensions.  One launch.  keep = (m_f, m_m) counts (_keep_counts): the trimmed
    launch, iters = 0 included -> TrimmedRefined with kept_f [...,m_f] and kept_m [...,m_m]; None: the untrimmed launch;
    _AutoCounts: the auto launch -> AutoRefined with kept_f [...,k], kept_m [...,k] padded with -1."""
    Kf, Km = T.shape[-4], T.shape[-3]
    Z = T.numel() // (Kf * Km * 16)
    b_of = torch.arange(Z * Km, dtype=torch.long, device=T.device).view(Z, 1, Km).expand(Z, Kf, Km).reshape(-1)
    lead = T.shape[:-2]
    form = {} if keep is None else {"auto": tuple(keep)} if isinstance(keep, _AutoCounts) else {"keep": keep}
    out = ops.icp_refine(Bf, Bm, T.reshape(Z * Kf * Km, 4, 4), iters, b_of=b_of, return_kept=keep is not None, **form)
    # ops returns the counts and the objective before the kept sets, the tuples hold the kept sets first
    out = out[:4] + out[-2:] + out[4:-2] if keep is not None else out
    return _kind_of(keep).Refined(*(t.view(*lead, *t.shape[1:]) for t in out))


def refine_pairs(pieces_f, top_f, pieces_m, top_m, T, iters=30, keep=1.0):
    """Refine every pair pose on its matched boundaries: for pieces_f [Kf,N,3] with picked rows top_f [Kf,Km,k], pieces_m
    [Km,N,3] with top_m [Km,k] and poses T [Kf,Km,4,4] (T[i,j] maps moved piece j into fixed piece i's frame), symmetric
    point-to-point ICP between pieces_f[i][top_f[i,j]] and pieces_m[j][top_m[j]] from T[i,j], at most `iters` accepted steps
    -> Refined(T [Kf,Km,4,4], score [Kf,Km], score0 [Kf,Km], iters_used [Kf,Km] int32).  score is the table's quantity (mean
    + mean of the squared nearest-neighbour distances) under the returned pose and never above score0, the same under T.
    All Kf Km problems run in one launch (ops.icp_refine); nothing waits for the device.
    keep (a fraction in (0, 1] of the k picked rows, or a pair (fixed side, moved side)): partial contact - only the
    ceil(f k) rows of each side that lie closest to the other side under the pose at hand count, in the score and in every
    step (the trimmed launch; include/pzn.h states the rule), so the picked rows on faces towards other neighbours neither
    score nor pull.  The result is then a TrimmedRefined: Refined's fields, then kept_f [Kf,Km,m_f] and kept_m [Kf,Km,m_m]
    (int32, ascending), positions into top_f[i,j] and top_m[j] of the rows kept under the returned pose.  keep = 1.0 is the
    untrimmed launch and a Refined, whose kept_f and kept_m are None.
    keep = "auto" or an AutoKeep: the counts are found per pair and per evaluated pose on the device (the auto launch) ->
    AutoRefined: TrimmedRefined's fields with kept_f [Kf,Km,k], kept_m [Kf,Km,k] padded with -1 behind the count, then count_f,
    count_m [Kf,Km] (int32) and objective [Kf,Km], the F that fell; score is the trimmed score at the returned counts and may
    exceed score0."""
    _on_gpu("refine_pairs", pieces_f=pieces_f, pieces_m=pieces_m, T=T, top_f=top_f, top_m=top_m)
    if pieces_f.dim() != 3 or pieces_m.dim() != 3 or pieces_f.shape[2] != 3 or pieces_m.shape[2] != 3:
        raise _lib.PznError(f"refine_pairs expects pieces_f[Kf,N,3], pieces_m[Km,N,3]; got {tuple(pieces_f.shape)}, "
                            f"{tuple(pieces_m.shape)}")
    Kf, Km = pieces_f.shape[0], pieces_m.shape[0]
    if top_f.dim() != 3 or top_f.shape[:2] != (Kf, Km) or top_m.dim() != 2 or top_m.shape[0] != Km or T.shape != (Kf, Km, 4, 4):
        raise _lib.PznError(f"refine_pairs expects top_f[{Kf},{Km},k], top_m[{Km},k], T[{Kf},{Km},4,4]; got "
                            f"{tuple(top_f.shape)}, {tuple(top_m.shape)}, {tuple(T.shape)}")
    counts = _keep_counts(keep, top_f.shape[2], top_m.shape[1], "refine_pairs")
    with torch.no_grad():
        Bf = ops.index_points(pieces_f, top_f.reshape(Kf, -1)).view(Kf * Km, top_f.shape[2], 3)
        Bm = ops.index_points(pieces_m, top_m)
        return _refine_gathered(Bf, Bm, T.contiguous(), iters, counts)


def _check_refine(refine, who):
    refine = int(refine)
    if refine < 0:
        raise _lib.PznError(f"{who}: refine = {refine} (0: none, or the number of ICP steps at most)")
    return refine


def pair_block(model, pieces_f, codes_f, pieces_m, codes_m, k=128, refine=0, keep=1.0):
    """The rectangular block of the pair table with pieces_f [Kf,N,3] in the fixed role and pieces_m [Km,N,3] in the moved
    role, from their PieceCodes -> PairBlock(twist [Kf,Km,6], T [Kf,Km,4,4], de_fpcb [Kf,Km,2,N], top_f [Kf,Km,k],
    score [Kf,Km]); entries as match_pairs documents them (no diagonal is masked here).  refine > 0: T and score are those
    of refine_pairs(..., iters=refine) from the network's pose, one launch in place of the transform and the chamfer; twist
    stays the network's output.  keep as pair_block_batch takes it (kept_f [Kf,Km,m_f], kept_m [Kf,Km,m_m]).  It is
    pair_block_batch for one puzzle."""
    refine = _check_refine(refine, "pair_block")
    one = lambda codes: PieceCodes(*(f[None] for f in codes))
    blk = pair_block_batch(model, pieces_f[None], one(codes_f), pieces_m[None], one(codes_m), k, refine, keep)
    return type(blk)(*(f[0] for f in blk))


def _diagonal(pieces):
    """The [K,K] bool diagonal for pieces [...,K,N,3]."""
    return torch.eye(pieces.shape[-3], dtype=torch.bool, device=pieces.device)


def _table(codes, blk, mask=None):
    """The PairTable of pieces with the PieceCodes `codes` and their square PairBlock; score is +inf where mask (None: blk's
    score is masked already)."""
    score = blk.score if mask is None else blk.score.masked_fill(mask, float("inf"))
    fields = (blk.twist, blk.T, blk.de_fpcb, codes.de_mrpcb, blk.top_f, codes.top_m, score, codes.x2)
    kind = next(kind for kind in _KINDS if type(blk) is kind.PairBlock)
    return kind.PairTable(*fields, *blk[len(PairBlock._fields):])


def match_pairs(model, pieces, k=128, start=None, refine=0, keep=1.0):
    """All K (K - 1) ordered pairs of `pieces` [K,N,3] (float32, on the GPU, N = model.num_points, K >= 2) through
    predict5's eval path with every piece encoded once -> PairTable, index order [fixed i, moved j]:

      twist [K,K,6]       predict5's `out` for fpc = pieces[i], mrpc = pieces[j]
      T [K,K,4,4]         se3.exp(twist): maps piece j into piece i's frame
      de_fpcb [K,K,2,N]   fixed-side boundary logits (a permuted view of the kernel's [K,K,N,2])
      de_mrpcb [K,2,N]    moved-side boundary logits (they depend on j only)
      top_f [K,K,k], top_m [K,k]   the k points of largest class-1 probability
      score [K,K]         mean + mean of the chamfer distances between pieces[i][top_f[i,j]] and T[i,j] applied to
                          pieces[j][top_m[j]]; +inf on the diagonal
      x2 [K,256,3]        the second-level sample points of every piece (one plan, shared by both encoders)

    start = (s1[K], s2[K]): int64 FPS start indices of the two set-abstraction levels; None draws them with
    torch.randint(0, N, (K,)) then torch.randint(0, 512, (K,)) from model.fps_generator (the global generator when that
    is None).  Any K is taken: the encoders run on 64 pieces at a time.  Nothing here waits for the device.
    It is match_puzzles for the one puzzle pieces[None]: encode_pieces, the square pair block and the diagonal fill.

    refine = N > 0: T and score are refined on the picked rows (refine_pairs, at most N accepted ICP steps from se3.exp(twist),
    one launch for the table; the diagonal is refined like any pair and then masked); twist stays the network's output, so
    T is no longer se3.exp(twist); every other field is what refine = 0 gives, bit for bit.

    keep (a fraction in (0, 1] of the k picked rows, or a pair (fixed side, moved side); 1.0: every row, today's table): a
    piece has several fracture faces and only part of one mates with a given neighbour, while top_m[j] is picked for piece j
    alone.  With keep < 1 only the ceil(f k) rows of each side closest to the other side count (refine_pairs states it),
    always through the one trimmed launch - at refine = 0 it runs with no step, so T stays se3.exp(twist) and score is the
    trimmed score under it.  The table is then a TrimmedPairTable: PairTable's fields, then kept_f [K,K,m_f] and kept_m
    [K,K,m_m] (int32: positions into top_f[i,j] and top_m[j] of the rows kept under T[i,j]); at keep = 1.0 it is a PairTable,
    whose kept_f and kept_m are None.  Every other field but T and score is what keep = 1.0 gives.

    keep = "auto" or AutoKeep(least=0.25, power=3): a fracture has no one share - siblings mate along a whole face, pieces
    across an older cut along a corner - so the counts are found per pair and per evaluated pose on the device (AutoKeep and
    include/pzn.h state the rule), again through one launch, refine = 0 included.  The table is an AutoPairTable: the
    trimmed table's fields with kept_f, kept_m [K,K,k] padded with -1 behind the count, then count_f, count_m [K,K] (int32) and
    objective [K,K].  score is the trimmed score at each pair's own counts, so one max_score means the same for every pair;
    the walks and evaluate_* read score and T as ever.  refine_assembly takes such a table with kept="frozen"
    (a count per joint) and refuses it by default (PznUnsupported)."""
    refine = _check_refine(refine, "match_pairs")
    _check_pieces(model, pieces, k, "match_pairs", 2)
    if start is not None:
        start = tuple(torch.as_tensor(s, dtype=torch.long)[None] for s in start)
    pieces, codes, blk = _match_puzzles(model, pieces[None], k, start, refine, "match_pairs", keep)
    table = _table(codes, blk, _diagonal(pieces))
    return type(table)(*(f[0] for f in table))


def _host(a):
    if isinstance(a, torch.Tensor):
        return a.detach().to("cpu", torch.float64).numpy()
    return np.asarray(a, dtype=np.float64)


def _rigid_inv(T):
    R, t = T[:3, :3], T[:3, 3]
    out = np.eye(4)
    out[:3, :3] = R.T
    out[:3, 3] = -R.T @ t
    return out


def assemble(score, T, max_score=None):
    """Greedy assembly from a pair table, on the host in float64.  score[K,K] and T[K,K,4,4] (tensors or arrays; T[i,j]
    maps piece j into piece i's frame) -> Assembly:

      root     the fixed piece i0 of the smallest off-diagonal score (first row-major position)
      edges    (i, j, score, placed) in placement order
      G [K,4,4]    maps each piece into the root's frame; identity for pieces that were not placed
      placed [K]   bool

    Until every piece is placed, the ordered pair (i, j), i != j, with exactly one end placed and the smallest score is
    taken (ties: first row-major position); a fixed end that is placed gives G[j] = G[i] T[i,j], otherwise
    G[i] = G[j] inv(T[i,j]) with the rigid inverse.  With max_score, the walk stops at the first score above it."""
    S = _host(score)
    P = _host(T)
    K = S.shape[0]
    if S.shape != (K, K) or P.shape != (K, K, 4, 4) or K < 2:
        raise ValueError(f"assemble expects score[K,K], T[K,K,4,4] with K >= 2; got {S.shape}, {P.shape}")
    S = S.copy()
    S[np.arange(K), np.arange(K)] = np.inf
    S[np.isnan(S)] = np.inf
    root = int(np.argmin(S)) // K
    G = np.tile(np.eye(4), (K, 1, 1))
    placed = np.zeros(K, dtype=bool)
    placed[root] = True
    edges = []
    while not placed.all():
        one_end = placed[:, None] != placed[None, :]
        cand = np.where(one_end, S, np.inf)
        flat = int(np.argmin(cand))                     # the first row-major position of the minimum
        i, j = divmod(flat, K)
        s = cand[i, j]
        if not np.isfinite(s) or (max_score is not None and s > max_score):
            break
        if placed[i]:
            G[j] = G[i] @ P[i, j]
            new = j
        else:
            G[i] = G[j] @ _rigid_inv(P[i, j])
            new = i
        placed[new] = True
        edges.append((i, j, float(s), new))
    return Assembly(root, edges, G, placed)


AUTO_JOINT_MESSAGE = ("a table made with keep='auto' carries a kept count per pair, chosen under the pair's own pose: pass "
                      "kept='frozen' to refine it jointly over exactly those sets (the joint refinement does not trim again "
                      "under its own poses), or make the table with a keep fraction")


def _kept_mode(kept, table, who, keep=None):
    """The `kept` and `keep` keywords of the joint refinements, decided before any tensor is touched.
    kept: None or "frozen" (PznError for anything else).  Both refine over the kept sets the table carries, as they are; an
    AutoPairTable's were chosen per pair under the pair pose, and freezing them is a choice the caller has to name: None
    refuses such a table - unless keep is given, which names another choice.
    keep: None; a fraction in (0, 1] or a pair (fixed side, moved side) of such; or "table" (the table's own counts: a
    TrimmedPairTable's kept widths or an AutoPairTable's count per pair; a table without counts is a PznError).  keep together
    with kept="frozen" is a PznError: the kept rows are either frozen or chosen again.
    -> None (today's paths), the shares as keep gave them, or "table"."""
    if kept is not None and not (isinstance(kept, str) and kept == "frozen"):
        raise _lib.PznError(f"{who}: kept must be None or 'frozen'; got {kept!r}")
    if keep is None:
        if kept is None and isinstance(table, AutoPairTable):
            raise _lib.PznUnsupported(f"{who}: {AUTO_JOINT_MESSAGE}")
        return None
    if kept is not None:
        raise _lib.PznError(f"{who}: keep = {keep!r} chooses the kept rows again under the joint poses and kept = {kept!r} freezes "
                            "the table's: pass one of them")
    if isinstance(keep, str):
        if keep != "table":
            raise _lib.PznError(f"{who}: keep = {keep!r} (a fraction in (0, 1], a pair (fixed, moved) of such, or 'table')")
        if not isinstance(table, (TrimmedPairTable, AutoPairTable)):
            raise _lib.PznError(f"{who}: keep = 'table' needs a table that carries counts (match_pairs / match_puzzles with "
                                f"keep < 1 or keep = 'auto'); got a {type(table).__name__}")
        return "table"
    if isinstance(keep, AutoKeep):
        raise _lib.PznError(f"{who}: keep = {keep!r}: the joint refinement takes its counts, it does not find them (a fraction, "
                            "a pair of fractions, or 'table')")
    _keep_counts(keep, 1, 1, who)      # (the shares are checked here; the counts wait for k)
    return keep


def _auto_mode(auto, kept, keep, who):
    """The `auto` keyword of the joint refinements, decided before any tensor is touched: None, True (AutoKeep()) or an AutoKeep
    (PznError for anything else, a share or power out of range included).  It names a choice of its own - the counts of every
    joint are found under the joint poses - so together with keep or with kept it is a PznError, and an AutoPairTable is not
    refused.  -> None or the AutoKeep."""
    if auto is None:
        return None
    if auto is True:
        auto = AutoKeep()
    if not isinstance(auto, AutoKeep):
        raise _lib.PznError(f"{who}: auto must be None, True or an AutoKeep(least, power); got {auto!r}")
    if keep is not None or kept is not None:
        raise _lib.PznError(f"{who}: auto finds the counts of every joint under the joint poses; keep = {keep!r} gives them and "
                            f"kept = {kept!r} freezes the table's rows: pass one of the three")
    _keep_counts(auto, 1, 1, who)      # (least and power are checked here; the counts wait for k)
    return auto


def _auto_joint_refined(out, joints):
    """AutoJointRefined from ops.joint_refine(..., auto=, return_kept=True)'s tuple and the JointRefined `joints` field."""
    G, score, score0, _, used, accepted, kept_f, kept_m, count_f, count_m, objective, objective0 = out
    return AutoJointRefined(G, score, score0, used, accepted, joints, kept_f, kept_m, count_f, count_m, objective, objective0)


def _joint_keep_counts(mode, table, pick, shape, who):
    """The kept counts of the joint rows for a `keep` that _kept_mode let through -> (ma, mb, m_f, m_m): int32 tensors of `shape`
    on the GPU, or (None, None) where every row is kept (the untrimmed launch), and the two counts as ints where they are one
    for all rows (None for an AutoPairTable's).  pick(t) takes a per-pair tensor t [...,P,P] to the joint rows."""
    k = table.top_m.shape[-1]
    dev = table.top_m.device
    if mode == "table" and isinstance(table, AutoPairTable):
        return pick(table.count_f).to(torch.int32).reshape(shape), pick(table.count_m).to(torch.int32).reshape(shape), None, None
    if mode == "table":
        m_f, m_m = int(table.kept_f.shape[-1]), int(table.kept_m.shape[-1])
    else:
        m_f, m_m = _keep_counts(mode, k, k, who) or (k, k)
    if m_f == k and m_m == k:
        return None, None, k, k
    return (torch.full(shape, m_f, dtype=torch.int32, device=dev), torch.full(shape, m_m, dtype=torch.int32, device=dev), m_f, m_m)


def _trimmed_joint_refined(out, joints, rows, ma, mb, m_f, m_m, k):
    """TrimmedJointRefined from ops.joint_refine's tuple `out` (with its kept sets, or without them where every row was kept:
    then 0 .. k-1 on the used rows), the JointRefined `joints` field, the joint rows on the device `rows` [...,J,2] and
    _joint_keep_counts' answer; every tensor keeps its leading Z."""
    G, score, score0, _, used, accepted = out[:6]
    dev = G.device
    if len(out) > 6:
        kept_f, kept_m = out[6], out[7]
    else:
        live = (rows[..., 0] >= 0)[..., None]
        full = torch.arange(k, dtype=torch.int32, device=dev).expand(*rows.shape[:-1], k)
        kept_f = kept_m = torch.where(live, full, torch.full_like(full, -1))
    if ma is None:
        ma, mb = (torch.full(rows.shape[:-1], m, dtype=torch.int32, device=dev) for m in (m_f, m_m))
    return TrimmedJointRefined(G, score, score0, used, accepted, joints, kept_f, kept_m, ma, mb)


def _joint_sets(pieces, table, z, i, j, full=False):
    """The point sets of the ordered pairs (z[q], i[q], j[q]) (int64 [n], on the GPU; z may be one int for all of them) of
    pieces [Z,P,N,3] and their table (leading Z), by ONE gather over the Z P N rows of all pieces -> (a [n,ka,3], b [.,kb,3],
    b_of, na, nb) as ops.joint_refine takes them for rows that are those pairs in that order; b_of [n] (or None: b[q]) is
    where pair q finds its moved-side set.
      * no kept sets: a[q] = pieces[z,i][top_f[z,i,j]]; b holds one set per piece, top_m's, shared through b_of = z P + j;
      * kept sets: the kept rows of the pair on both sides, one set per ordered pair, b_of None;
      * an AutoPairTable: the same with stride k, the -1 padding clamped to 0 (it gathers row 0 of the set, never read) and
        count_f / count_m of the pairs as na / nb (None otherwise).
    full: the first form whatever the table carries (its kept fields are not read)."""
    Z, P, N, _ = pieces.shape
    n, k = i.numel(), table.top_m.shape[-1]
    fixed, moved = z * P + i, z * P + j      # the pieces of a pair among all Z P; piece p's rows begin at p N
    top_f = table.top_f[z, i, j]
    b_of = na = nb = None
    if full or table.kept_f is None:
        rows_a = (fixed * N)[:, None] + top_f
        rows_b = torch.arange(Z * P, dtype=torch.long, device=pieces.device)[:, None] * N + table.top_m.reshape(Z * P, k)
        b_of = moved
    else:
        kept_f, kept_m = table.kept_f[z, i, j].long(), table.kept_m[z, i, j].long()
        if isinstance(table, AutoPairTable):
            kept_f, kept_m = kept_f.clamp(min=0), kept_m.clamp(min=0)
            na, nb = table.count_f[z, i, j].to(torch.int32), table.count_m[z, i, j].to(torch.int32)
        rows_a = (fixed * N)[:, None] + top_f.gather(1, kept_f)
        rows_b = (moved * N)[:, None] + table.top_m[z, j].gather(1, kept_m)
    rows = torch.cat((rows_a.reshape(-1), rows_b.reshape(-1)))
    picked = ops.index_points(pieces.contiguous().view(1, Z * P * N, 3), rows.reshape(1, -1))[0]
    ka, kb = rows_a.shape[1], rows_b.shape[1]
    return picked[:n * ka].view(n, ka, 3), picked[n * ka:].view(-1, kb, 3), b_of, na, nb


def refine_assembly(pieces, table, asm, sweeps=30, joint_score=None, kept=None, keep=None, auto=None):
    """Refine all placed poses of a greedy assembly jointly over every joint: pieces [K,N,3] (float32, on the GPU), table =
    match_pairs' PairTable of them, asm = assemble's Assembly of that table -> JointRefined:

      G [K,4,4]       float32, on the GPU: each piece into the root's frame; the root's and every unplaced piece's pose is
                      asm.G's (rounded to float32), bit for bit
      score, score0   0-d tensors: the sum over the joints of the table's score with both sides in the root's frame, under G and
                      under asm.G; score <= score0
      sweeps_used     0-d int32, accepted [K] int32: ops.joint_refine's
      joints          the ordered pairs (i, j) used, a host list in row-major order

    The joints are every (i, j), i != j, both placed, with table.score[i,j] <= joint_score; the default joint_score is the
    largest score among asm.edges - a definition, not a measurement: the tree edges are then always joints and every placed
    piece has one.  Joint (i, j) pairs pieces[i][table.top_f[i,j]] with pieces[j][table.top_m[j]] (one set per moved piece,
    served to all its joints).  Every piece that is placed and not the root may move; sweeps = 0 returns asm.G.
    One download (the scores the joints are chosen from), one gather and one launch.

    A table that carries kept sets (match_pairs(..., keep < 1)): joint (i, j) pairs pieces[i][top_f[i,j][kept_f[i,j]]] with
    pieces[j][top_m[j][kept_m[i,j]]] - m_f and m_m rows, the moved-side set now one per ordered pair.  The kernel and its
    energy are the same, the untrimmed one over the rows the pair refinement kept: the joint refinement FREEZES the kept
    sets, it does not trim again under its own poses.

    kept: None or "frozen" (anything else is a PznError).  "frozen" names that freezing and changes nothing for the tables
    above.  An AutoPairTable (keep="auto") carries a count per pair, found under the pair's pose; it is refused by default
    (PznUnsupported, AUTO_JOINT_MESSAGE) and refined with kept="frozen": joint (i, j) pairs the count_f[i,j] rows
    pieces[i][top_f[i,j][kept_f[i,j][:count_f[i,j]]]] with the count_m[i,j] rows of pieces[j] likewise, J sets of stride k
    a side (the -1 padding gathers row 0 of the set, which the kernel never reads) and the counts as ops.joint_refine's
    na / nb: still one gather and one launch, with every 1 / ka and 1 / kb of the energy that joint's own count.

    keep (None: everything above, bit for bit): the kept rows of every joint are chosen AGAIN under the joint poses, at every
    evaluation (ops.joint_refine's ma / mb, pzn_joint_refine_trim_f32; include/pzn.h states the rule), so the picked rows on
    faces towards other neighbours neither score nor pull, and the rows that do are not tied to the pair's own pose.  The sets
    are the FULL ones of any table - pieces[i][top_f[i,j]] and pieces[j][top_m[j]], shared through b_of - and the table's kept
    fields are not read.  A fraction in (0, 1] or a pair (fixed side, moved side): ceil(f k) rows of each side, the pair
    functions' rule (1.0: the untrimmed launch over the full sets).  "table": the table's own counts - a TrimmedPairTable's kept
    widths for every joint, an AutoPairTable's count_f[i,j] and count_m[i,j] per joint; a table without counts is a PznError.
    keep together with kept="frozen" is a PznError; an AutoPairTable with keep is not refused.  -> TrimmedJointRefined:
    JointRefined's fields, then kept_f [J,k], kept_m [J,k] (int32: the positions into top_f[i,j] / top_m[j] kept under the
    returned poses, ascending, -1 behind the count) and count_f, count_m [J] (int32).  Still one gather and one launch.

    auto (None: everything above, bit for bit): True (AutoKeep()) or an AutoKeep(least, power) - the two counts of every joint
    are FOUND, at every evaluation of the joint under the poses being tried (ops.joint_refine's auto,
    pzn_joint_refine_auto_f32; include/pzn.h states the rule), no fewer than ceil(least k) rows a side by the rule of a keep
    fraction.  The sets are the full ones of any table, as for keep; an AutoPairTable is accepted.  auto together with keep or
    with kept is a PznError, raised before any tensor is touched.  -> AutoJointRefined: TrimmedJointRefined's fields with the
    counts found under the returned poses in count_f, count_m, then objective and objective0 (0-d: the F that fell; score is
    the trimmed energy at the counts found and need not fall).  Still one gather and one launch."""
    auto = _auto_mode(auto, kept, keep, "refine_assembly")
    mode = "auto" if auto is not None else _kept_mode(kept, table, "refine_assembly", keep)
    _clouds("refine_assembly", "K", pieces=pieces)
    K, N, _ = pieces.shape
    G0 = np.asarray(asm.G, dtype=np.float64)
    placed = np.asarray(asm.placed, dtype=bool)
    if table.score.shape != (K, K) or table.top_f.shape[:2] != (K, K) or table.top_m.shape[0] != K or G0.shape != (K, 4, 4) \
            or placed.shape != (K,):
        raise _lib.PznError(f"refine_assembly: the table and the assembly are not those of K = {K} pieces: score "
                            f"{tuple(table.score.shape)}, top_f {tuple(table.top_f.shape)}, G {G0.shape}")
    dev = pieces.device
    with torch.no_grad():
        S = table.score.detach().to("cpu", torch.float64).numpy()
        if joint_score is None:
            joint_score = max((float(e[2]) for e in asm.edges), default=-np.inf)
        ok = placed[:, None] & placed[None, :] & ~np.eye(K, dtype=bool) & (S <= float(joint_score))
        joints = [(int(i), int(j)) for i, j in zip(*np.nonzero(ok))]
        J = len(joints)
        g0 = torch.from_numpy(G0.astype(np.float32)).to(dev).reshape(1, K, 4, 4)
        movable = placed.copy()
        movable[int(asm.root)] = False
        mv = torch.from_numpy(movable.astype(np.uint8)).to(dev).reshape(1, K)
        jl = torch.tensor(joints, dtype=torch.int32).reshape(1, J, 2)
        if J > 0:      # exactly the J joints' sets, at Z = 1
            ji = torch.tensor([i for i, _ in joints], dtype=torch.long, device=dev)
            jj = torch.tensor([j for _, j in joints], dtype=torch.long, device=dev)
            one = type(table)(*(None if f is None else f[None] for f in table))      # (a caller's table may leave fields out)
            a, b, b_of, cnt_a, cnt_b = _joint_sets(pieces[None], one, 0, ji, jj, full=mode is not None)
            b_of = None if b_of is None else b_of.reshape(1, J)
        else:
            a = b = pieces[:0, :table.top_m.shape[1]]
            b_of = cnt_a = cnt_b = None
        if auto is not None:
            k = table.top_m.shape[1]
            out = ops.joint_refine(a, b, jl, g0, mv, sweeps, b_of=b_of, auto=tuple(_keep_counts(auto, k, k, "refine_assembly")),
                                   return_kept=True)
            return AutoJointRefined(*(f[0] if isinstance(f, torch.Tensor) else f for f in _auto_joint_refined(out, joints)))
        if mode is not None:
            ma, mb, m_f, m_m = _joint_keep_counts(mode, table, lambda t: t[ji, jj] if J > 0 else t[:0, 0], (1, J), "refine_assembly")
            out = ops.joint_refine(a, b, jl, g0, mv, sweeps, b_of=b_of, ma=ma, mb=mb, return_kept=ma is not None)
            out = _trimmed_joint_refined(out, joints, jl.to(dev) if ma is None else None, ma, mb, m_f, m_m, table.top_m.shape[1])
            return TrimmedJointRefined(*(f[0] if isinstance(f, torch.Tensor) else f for f in out))
        G, score, score0, _, used, accepted = ops.joint_refine(a, b, jl, g0, mv, sweeps, b_of=b_of, na=cnt_a, nb=cnt_b)
    return JointRefined(G[0], score[0], score0[0], used[0], accepted[0], joints)


def apply(pieces, G):
    """The pieces [K,N,3] (on the GPU) in the root's frame: G[k] applied to piece k."""
    _on_gpu("apply", pieces=pieces)
    g = torch.as_tensor(np.asarray(G) if not isinstance(G, torch.Tensor) else G).to(pieces.device, torch.float32)
    return se3.transform_points(g.contiguous(), pieces.contiguous())


# --------------------------------------------------------------------------- ground truth and the score of an assembly

Evaluation = collections.namedtuple("Evaluation", "rot_deg trans msd part_ok part_accuracy edge_precision")


def truth_table(pose, mates=None, cd=None):
    """The pair table a perfect matcher would return for pieces moved by `pose` [P,4,4] (datapipe.fracture's pose of one sample:
    moved piece = pose[p] applied to the piece where it belongs), on the host in float64 -> (T_gt [P,P,4,4], score_gt [P,P]):
    T_gt[i,j] = pose[i] inv(pose[j]) maps moved piece j into moved piece i's frame (PairTable.T's convention); score_gt = cd
    where mates, +inf elsewhere and on the diagonal (mates None: every pair; cd None: 0), so assemble(score_gt, T_gt) walks
    the pieces that touch."""
    X = _host(pose)
    P = X.shape[0]
    if X.shape != (P, 4, 4) or P < 2:
        raise ValueError(f"truth_table expects pose[P,4,4] with P >= 2; got {X.shape}")
    inv = np.stack([_rigid_inv(X[p]) for p in range(P)])
    T = np.einsum("iab,jbc->ijac", X, inv)
    S = np.zeros((P, P)) if cd is None else _host(cd).copy()
    keep = np.ones((P, P), dtype=bool) if mates is None else np.asarray(_host(mates) != 0)
    if S.shape != (P, P) or keep.shape != (P, P):
        raise ValueError(f"truth_table expects cd[P,P] and mates[P,P] with P = {P}; got {S.shape}, {keep.shape}")
    S[~keep] = np.inf
    S[np.arange(P), np.arange(P)] = np.inf
    return T, S


def evaluate(G, placed, pose, rest, root, edges=None, mates=None, tol=0.01):
    """The score of an assembly against the truth, on the host in float64.  G [P,4,4] maps moved piece p into the frame of moved
    piece `root`; placed [P] bool; pose [P,4,4] and rest [P,n,3] are datapipe.fracture's of one sample.  The truth for piece p
    is G*[p] = pose[root] inv(pose[p]).  -> Evaluation:
      rot_deg [P]      the geodesic angle between the rotations of G[p] and G*[p], degrees
      trans [P]        |t - t*|
      msd [P]          the mean over the piece's points x = pose[p] rest[p] of |G[p] x - G*[p] x|^2
      part_ok [P]      placed & (msd < tol); tol is a definition (a squared distance in the cloud's units), not a measurement
      part_accuracy    the share of the pieces other than root with part_ok
      edge_precision   the share of `edges` (tuples that begin with the two pieces joined) whose pair is in mates [P,P]; None
                       without both or without an edge
    It takes assemble's Assembly as evaluate(a.G, a.placed, pose, rest, a.root, a.edges, mates).  For a Progressive it takes
    one part: G and placed limited to that part's members, root the piece whose frame the part lives in (MergeLedger.frame)."""
    G, X, R = _host(G), _host(pose), _host(rest)
    P = X.shape[0]
    placed = np.asarray(placed.detach().cpu().numpy() if isinstance(placed, torch.Tensor) else placed).astype(bool)
    root = int(root)
    if G.shape != (P, 4, 4) or X.shape != (P, 4, 4) or R.ndim != 3 or R.shape[0] != P or R.shape[2] != 3 or placed.shape != (P,) \
            or not 0 <= root < P:
        raise ValueError(f"evaluate expects G[P,4,4], placed[P], pose[P,4,4], rest[P,n,3], 0 <= root < P; got {G.shape}, "
                         f"{placed.shape}, {X.shape}, {R.shape}, root = {root}")
    rot_deg, trans, msd = np.zeros(P), np.zeros(P), np.zeros(P)
    for p in range(P):
        Gt = X[root] @ _rigid_inv(X[p])
        D = G[p, :3, :3] @ Gt[:3, :3].T
        # the angle from both the trace and the skew part: atan2 keeps its precision at 0 and at 180 degrees
        skew = np.array([D[2, 1] - D[1, 2], D[0, 2] - D[2, 0], D[1, 0] - D[0, 1]])
        rot_deg[p] = np.degrees(np.arctan2(np.linalg.norm(skew), np.trace(D) - 1.0))
        trans[p] = np.linalg.norm(G[p, :3, 3] - Gt[:3, 3])
        x = R[p] @ X[p, :3, :3].T + X[p, :3, 3]
        d = x @ (G[p, :3, :3] - Gt[:3, :3]).T + (G[p, :3, 3] - Gt[:3, 3])
        msd[p] = (d * d).sum(1).mean()
    part_ok = placed & (msd < tol)
    others = np.arange(P) != root
    part_accuracy = float(part_ok[others].mean()) if others.any() else 1.0
    edge_precision = None
    if edges is not None and mates is not None and len(edges) > 0:
        m = np.asarray(_host(mates) != 0)
        edge_precision = float(np.mean([bool(m[int(e[0]), int(e[1])]) for e in edges]))
    return Evaluation(rot_deg, trans, msd, part_ok, part_accuracy, edge_precision)


# --------------------------------------------------------------------------- a batch of puzzles on the device

AssemblyBatch = collections.namedtuple("AssemblyBatch", "root edges edge_score n_edges G placed movable joints n_joints")
WalkRule = collections.namedtuple("WalkRule", "root edges edge_score n_edges G placed joints n_joints")


def _dot4(a0, b0, a1, b1, a2, b2, a3, b3):
    return ((a0 * b0 + a1 * b1) + a2 * b2) + a3 * b3


def _rule_product(A, B):
    """The 4x4 product of the walk rule on lists of Python floats (IEEE double): every entry ((a0 b0 + a1 b1) + a2 b2) + a3 b3."""
    return [[_dot4(A[u][0], B[0][v], A[u][1], B[1][v], A[u][2], B[2][v], A[u][3], B[3][v]) for v in range(4)] for u in range(4)]


def _rule_inverse(T):
    """[R^T, -(R^T t)] with the last row 0 0 0 1; an entry of R^T t is (r0 t0 + r1 t1) + r2 t2."""
    out = [[T[v][u] for v in range(3)] + [-((T[0][u] * T[0][3] + T[1][u] * T[1][3]) + T[2][u] * T[2][3])] for u in range(3)]
    out.append([0.0, 0.0, 0.0, 1.0])
    return out


def _as_np(a, dt):
    return (a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)).astype(dt)


def _rule_outputs(Z, K):
    """The walk's eight outputs as the kernels leave a puzzle that makes no edge -> WalkRule of numpy arrays."""
    return WalkRule(np.full(Z, -1, dtype=np.int32), np.full((Z, K - 1, 3), -1, dtype=np.int32),
                    np.full((Z, K - 1), np.inf, dtype=np.float32), np.zeros(Z, dtype=np.int32), np.tile(np.eye(4), (Z, K, 1, 1)),
                    np.zeros((Z, K), dtype=np.uint8), np.full((Z, K * (K - 1), 2), -1, dtype=np.int32), np.zeros(Z, dtype=np.int32))


def _rule_joints(comp, raw, limit, out):
    """The joints of a finished walk, row-major: every (i, j), i != j, inside and in one component (comp[p] = the component of
    piece p, -1 outside), with raw[i][j] <= limit, written to the first rows of out [K (K - 1),2] -> their number."""
    n = 0
    for i in range(len(comp)):
        for j in range(len(comp)):
            if i != j and comp[i] >= 0 and comp[i] == comp[j] and raw[i][j] <= limit:
                out[n] = (i, j)
                n += 1
    return n


def _rule_table(score, T, count, max_score, who, M=None):
    """What the rules read alike -> (S float32 [Z,K,K], P float32 [Z,K,K,4,4], counts [Z], the stop limit).  M: the beam rules'
    moment, already a float64 array, checked beside the other two."""
    S, P = _as_np(score, np.float32), _as_np(T, np.float32)
    Z, K = S.shape[0], S.shape[1]
    want, got = "score[Z,K,K], T[Z,K,K,4,4]", f"{S.shape}, {P.shape}"
    bad = S.shape != (Z, K, K) or P.shape != (Z, K, K, 4, 4) or K < 2
    if M is not None:
        want, got, bad = want + ", moment[Z,K,4,4]", got + f", {M.shape}", bad or M.shape != (Z, K, 4, 4)
    if bad:
        raise ValueError(f"{who} expects {want} with K >= 2; got {got}")
    counts = np.full(Z, K, dtype=np.int64) if count is None else _as_np(count, np.int64)
    return S, P, counts, float("inf") if max_score is None else float(max_score)


def _rule_keys(raw, c):
    """The keys of a puzzle's first c pieces from its scores (float32 values as Python floats): NaN and the diagonal are +inf."""
    inf = float("inf")
    return [[inf if (i == j or raw[i][j] != raw[i][j]) else raw[i][j] for j in range(c)] for i in range(c)]


def _rule_root(key, inside):
    """The row of the smallest key among the entries (i, j), i != j, with both ends outside, the first row-major position on ties
    (two or more pieces are outside)."""
    best, at = float("inf"), None
    for i in range(len(key)):
        for j in range(len(key)):
            if i != j and not inside[i] and not inside[j] and (at is None or key[i][j] < best):
                best, at = key[i][j], (i, j)
    return at[0]


def _rule_grow(key, raw, Pz, limit, r, inside, pose, made):
    """One tree of the walk: r goes inside with the identity, then rounds - the smallest key among the ordered pairs with exactly
    one end inside, the first row-major position on ties - until none is left or the key is not finite or above limit.  inside
    and pose {piece: 4x4 as lists} are updated, the edges (i, j, new) appended to made -> the pieces placed, r first."""
    inf = float("inf")
    inside[r] = True
    pose[r] = [[1.0 if u == v else 0.0 for v in range(4)] for u in range(4)]
    new_ones = [r]
    while True:
        best, at = inf, None
        for i in range(len(key)):
            for j in range(len(key)):
                if inside[i] != inside[j] and (at is None or key[i][j] < best):
                    best, at = key[i][j], (i, j)
        if at is None or not np.isfinite(best) or best > limit:
            return new_ones
        i, j = at
        Tij = Pz[i, j].astype(np.float64).tolist()
        if inside[i]:
            new = j
            pose[j] = _rule_product(pose[i], Tij)
        else:
            new = i
            pose[i] = _rule_product(pose[j], _rule_inverse(Tij))
        inside[new] = True
        new_ones.append(new)
        made.append((i, j, new))


def _rule_finish(z, out, S, raw, made, pose, comp, joint_score):
    """The outputs of puzzle z behind its root from its edges, poses and components (comp [c], -1 outside)."""
    _, edges, edge_score, n_edges, G, placed, joints, n_joints = out[:8]
    worst = -float("inf")
    for e, (i, j, new) in enumerate(made):
        edges[z, e] = (i, j, new)
        edge_score[z, e] = S[z, i, j]
        worst = max(worst, raw[i][j])
    n_edges[z] = len(made)
    for p, g in pose.items():
        G[z, p] = np.array(g, dtype=np.float64)
    placed[z, :len(comp)] = [q >= 0 for q in comp]
    js = worst if joint_score is None or joint_score != joint_score else float(joint_score)      # (NaN is the kernel's None)
    if made:
        n_joints[z] = _rule_joints(comp, raw, js, joints[z])


def walk_rule(score, T, count=None, max_score=None, joint_score=None):
    """The numpy statement of ops.assemble_walk (csrc/assemblewalk.hip, the rule in include/pzn.h), which is held to it bit for
    bit, G included: assemble() and the joint selection of refine_assembly() for Z puzzles, on the host.  score [Z,K,K] (read as
    float32), T [Z,K,K,4,4] (float32), count [Z] or None, tensors or arrays -> WalkRule of numpy arrays in the kernel's shapes
    and types: root [Z] int32, edges [Z,K-1,3] int32, edge_score [Z,K-1] float32, n_edges [Z] int32, G [Z,K,4,4] float64, placed
    [Z,K] uint8, joints [Z,K(K-1),2] int32, n_joints [Z] int32.

    Key of entry (i, j): its float32 score, NaN and the diagonal as +inf; compared as floats, ties to the lowest i K + j; only
    i, j < count[z] exist.  The root is the row of the smallest key; a round takes the smallest key among the ordered pairs with
    exactly one end placed and stops at a key that is not finite or above max_score.  Poses are composed in float64 with every
    operation rounded on its own (_rule_product, _rule_inverse).  joint_score None: the puzzle's largest edge score."""
    S, P, counts, limit = _rule_table(score, T, count, max_score, "walk_rule")
    Z, K = S.shape[0], S.shape[1]
    out = _rule_outputs(Z, K)
    for z in range(Z):
        c = int(counts[z])
        if not 2 <= c <= K:
            continue
        raw = S[z].tolist()                              # float32 values as Python floats (exact)
        key = _rule_keys(raw, c)
        inside, pose, made = [False] * c, {}, []
        out.root[z] = _rule_root(key, inside)
        _rule_grow(key, raw, P[z], limit, int(out.root[z]), inside, pose, made)
        _rule_finish(z, out, S, raw, made, pose, [0 if p else -1 for p in inside], joint_score)
    return out


ForestRule = collections.namedtuple("ForestRule", WalkRule._fields + ("component", "roots", "n_components"))


def forest_rule(score, T, count=None, max_score=None, joint_score=None):
    """The numpy statement of ops.assemble_forest (csrc/assemblewalk.hip, the rule in include/pzn.h), which is held to it bit
    for bit, G included: walk_rule for a pile that holds the pieces of several objects.  The arguments, the keys, their order and
    ties, the stop test, the pose arithmetic and count are walk_rule's (its helpers run here).  Where the walk stops with pieces
    < count still outside, a new component starts: its root is the row of the smallest key among the entries with both ends
    outside (_rule_root - with nothing inside, the walk's root), or the one piece left; the root is inside with the identity, and
    the rounds go on, over the ordered pairs with exactly one end inside whichever component that end is in, until no piece is
    outside.  -> ForestRule: WalkRule's fields - root = roots[:, 0], the edges of all components in placement order, G[p] into
    the frame of piece p's own root, placed 1 for every p < count, joints only inside a component (joint_score None: the pile's
    largest edge score; no joint in a pile without an edge) - then component [Z,K] int32 (in the order the components start, -1 at
    and beyond count), roots [Z,K] int32 (unused -1) and n_components [Z] int32.  A count outside [2, K]: the walk's empty answer
    and no component.

    On a table without -inf every entry between an older component and the outside has failed the stop test, so a round's end
    inside is in the growing component, and the components are the connected components of the graph whose edges are the entries
    with a finite key <= max_score.  The first component is walk_rule's result."""
    S, P, counts, limit = _rule_table(score, T, count, max_score, "forest_rule")
    Z, K = S.shape[0], S.shape[1]
    out = ForestRule(*_rule_outputs(Z, K), np.full((Z, K), -1, dtype=np.int32), np.full((Z, K), -1, dtype=np.int32),
                     np.zeros(Z, dtype=np.int32))
    for z in range(Z):
        c = int(counts[z])
        if not 2 <= c <= K:
            continue
        raw = S[z].tolist()                              # float32 values as Python floats (exact)
        key = _rule_keys(raw, c)
        inside, pose, made = [False] * c, {}, []
        q = 0
        while not all(inside):
            r = inside.index(False) if inside.count(False) == 1 else _rule_root(key, inside)
            out.roots[z, q] = r
            out.component[z, _rule_grow(key, raw, P[z], limit, r, inside, pose, made)] = q
            q += 1
        out.root[z], out.n_components[z] = out.roots[z, 0], q
        _rule_finish(z, out, S, raw, made, pose, out.component[z, :c].tolist(), joint_score)
    return out


def _placed_movable(placed, root):
    """The kernel's placed bytes [Z,K] as bool, and movable = placed and not the root."""
    with torch.no_grad():
        placed = placed.bool()
        index = torch.arange(placed.shape[1], dtype=torch.int32, device=placed.device)
        return placed, placed & (index[None, :] != root[:, None])


def _forest_movable(placed, roots):
    """The kernel's placed bytes [Z,K] as bool, and movable = placed and not the root of any component (roots [Z,K], unused -1)."""
    with torch.no_grad():
        placed = placed.bool()
        index = torch.arange(placed.shape[1], dtype=torch.int32, device=placed.device)
        return placed, placed & ~(roots[:, :, None] == index[None, None, :]).any(dim=1)


def assemble_batch(score, T, count=None, max_score=None, joint_score=None):
    """assemble() and the joint selection of refine_assembly() for Z puzzles in ONE launch (ops.assemble_walk), everything on
    the device: score [Z,K,K], T [Z,K,K,4,4] (float32, on the GPU; match_puzzles' fields), count [Z] int32 or None (the pieces of
    every puzzle), max_score and joint_score as assemble and refine_assembly take them -> AssemblyBatch:

      root [Z] int32            -1 for a puzzle whose count is outside [2, K]
      edges [Z,K-1,3] int32     (i, j, new) in placement order, unused rows -1;  edge_score [Z,K-1], unused +inf;  n_edges [Z]
      G [Z,K,4,4] float64       each piece into its root's frame, the identity where not placed
      placed, movable [Z,K] bool     movable = placed and not the root: what refine_assembly_batch lets move
      joints [Z,K(K-1),2] int32      the joints of refine_assembly in its order, unused rows (-1, -1);  n_joints [Z]

    Discrete outputs are assemble's bit for bit; G follows walk_rule bit for bit (assemble composes with numpy's matmul, a
    last-place matter).  Nothing waits for the device."""
    root, edges, edge_score, n_edges, G, placed, joints, n_joints = ops.assemble_walk(score, T, count, max_score, joint_score)
    placed, movable = _placed_movable(placed, root)
    return AssemblyBatch(root, edges, edge_score, n_edges, G, placed, movable, joints, n_joints)


# --------------------------------------------------------------------------- a pile of several objects: the forest walk

ForestBatch = collections.namedtuple("ForestBatch", AssemblyBatch._fields + ("component", "roots", "n_components"))
PileEvaluation = collections.namedtuple("PileEvaluation", "pair_precision pair_recall pair_pose_recall n_components exact msd")


def assemble_forest_batch(score, T, count=None, max_score=None, joint_score=None):
    """assemble_batch for piles that hold the pieces of several objects, ONE launch for Z piles (ops.assemble_forest; forest_rule
    is its numpy statement): where the greedy walk stops with pieces left over, the pieces outside start a new component from a
    new root, until every piece < count is in one - which pieces belong together, and how each group goes together.  With
    refine > 0 a table's score is the distance of the two picked boundaries where they meet, so max_score is a geometric
    threshold: the components are the connected components of the entries below it.  The arguments are assemble_batch's ->
    ForestBatch: AssemblyBatch's fields (root = roots[:, 0]; edges over all components in placement order; G [Z,K,4,4] float64,
    each piece into the frame of its own component's root; placed: every piece < count; movable = placed and not the root of any
    component; joints only inside a component), then component [Z,K] int32 (-1 at and beyond count), roots [Z,K] int32 (the root
    of component q, unused -1) and n_components [Z] int32.  refine_assembly_batch takes it as it takes an AssemblyBatch: no joint
    crosses components and no root moves, so its one launch refines every component of every pile.  Nothing waits for the
    device."""
    root, edges, edge_score, n_edges, G, placed, joints, n_joints, component, roots, n_components = ops.assemble_forest(
        score, T, count, max_score, joint_score)
    placed, movable = _forest_movable(placed, roots)
    return ForestBatch(root, edges, edge_score, n_edges, G, placed, movable, joints, n_joints, component, roots, n_components)


def _pile_msd(G, X, R):
    """msd [...,K,K] of evaluate_pile for G, X = pose [...,K,4,4] and R = rest [...,K,n,3], float64 numpy arrays or torch tensors
    alike: msd[p,q] = the mean over x = X[q] R[q] of |inv(G[p]) G[q] x - X[p] inv(X[q]) x|^2 with the rigid inverse.  Written
    with element-wise operations in one order (the walk rule's dot4 and inverse), so that the difference of the two relative
    poses - a difference of nearly equal matrices for a good assembly - has the same bits on the host and on the device."""
    xp = torch if isinstance(G, torch.Tensor) else np
    K = X.shape[-3]

    def inv_rows(T):            # rows 0..2 of [R^T, -(R^T t)], entries [...,K]
        return [[T[..., v, u] for v in range(3)]
                + [-((T[..., 0, u] * T[..., 0, 3] + T[..., 1, u] * T[..., 1, 3]) + T[..., 2, u] * T[..., 2, 3])] for u in range(3)]

    Gi, Xi = inv_rows(G), inv_rows(X)
    last = (0.0, 0.0, 0.0, 1.0)                                                    # the last row of a rigid motion
    x = [((X[..., c, 0, None] * R[..., 0] + X[..., c, 1, None] * R[..., 1]) + X[..., c, 2, None] * R[..., 2]) + X[..., c, 3, None]
         for c in range(3)]                                                        # the moved pieces' coordinates, [...,K,n] each
    rows = []
    for p in range(K):
        sq = None
        for u in range(3):
            # row u of inv(G[p]) G[q] - X[p] inv(X[q]) for every q: four entries [...,K]
            D = [_dot4(Gi[u][0][..., p, None], G[..., 0, v], Gi[u][1][..., p, None], G[..., 1, v], Gi[u][2][..., p, None], G[..., 2, v],
                       Gi[u][3][..., p, None], G[..., 3, v])
                 - _dot4(X[..., p, None, u, 0], Xi[0][v], X[..., p, None, u, 1], Xi[1][v], X[..., p, None, u, 2], Xi[2][v],
                         X[..., p, None, u, 3], last[v]) for v in range(4)]
            d = ((D[0][..., None] * x[0] + D[1][..., None] * x[1]) + D[2][..., None] * x[2]) + D[3][..., None]
            sq = d * d if sq is None else sq + d * d
        rows.append(sq.mean(-1))
    return xp.stack(rows, -2)


def _pile_masks(component, object_of, live, off):
    """-> (together, belong) [...,K,K] bool over the ordered pairs p != q (off: the [K,K] off-diagonal) of live pieces [...,K]: in
    one component, of one object.  numpy arrays or torch tensors."""
    pairs = live[..., :, None] & live[..., None, :] & off
    together = pairs & (component[..., :, None] == component[..., None, :]) & (component[..., :, None] >= 0)
    return together, pairs & (object_of[..., :, None] == object_of[..., None, :])


def evaluate_pile(G, component, pose, rest, object_of, count=None, tol=0.01):
    """The score of a sorted and assembled pile against the truth, on the host in float64.  G [K,4,4] maps piece p into the frame
    of its component's root, component [K] (assemble_forest_batch's of one pile; pieces with the same value >= 0 are together),
    pose [K,4,4], rest [K,n,3] and object_of [K] are datapipe.pile's of one pile; only pieces < count are counted (None: K).
    Over the ordered pairs (p, q), p != q: together = in one component, belong = of one object, and msd[p,q] = the mean over
    the points x = pose[q] rest[q] of moved piece q of |inv(G[p]) G[q] x - pose[p] inv(pose[q]) x|^2: how far the assembly puts
    q from where it belongs, seen from p.  -> PileEvaluation:
      pair_precision      together & belong over together
      pair_recall         together & belong over belong
      pair_pose_recall    together & belong & (msd < tol) over belong; tol is evaluate's definition, not a measurement
      n_components        the number of components among the pieces counted
      exact               the components are the objects
      msd [K,K]           float64
    An empty denominator gives NaN.  Pairs are counted and not pieces: a share of pieces in the right component is inflated by
    singletons, which are trivially right, and here a singleton only costs recall."""
    G, X, R = _host(G), _host(pose), _host(rest)
    comp, obj = _as_np(component, np.int64), _as_np(object_of, np.int64)
    K = X.shape[0]
    if G.shape != (K, 4, 4) or X.shape != (K, 4, 4) or R.ndim != 3 or R.shape[0] != K or R.shape[2] != 3 or comp.shape != (K,) \
            or obj.shape != (K,):
        raise ValueError(f"evaluate_pile expects G[K,4,4], component[K], pose[K,4,4], rest[K,n,3], object_of[K]; got {G.shape}, "
                         f"{comp.shape}, {X.shape}, {R.shape}, {obj.shape}")
    live = np.arange(K) < (K if count is None else int(count))
    together, belong = _pile_masks(comp, obj, live, ~np.eye(K, dtype=bool))
    msd = _pile_msd(G, X, R)
    both = together & belong
    with np.errstate(invalid="ignore"):
        ratios = [float(np.float64(a.sum()) / np.float64(b.sum())) for a, b in
                  ((both, together), (both, belong), (both & (msd < tol), belong))]
    return PileEvaluation(*ratios, len(set(comp[live & (comp >= 0)].tolist())), bool((together == belong).all()), msd)


def evaluate_pile_batch(G, component, pose, rest, object_of, count=None, tol=0.01):
    """evaluate_pile() for Z piles in float64 torch on the device, with its formulas in its order of operations: G [Z,K,4,4]
    (assemble_forest_batch's, or refine_assembly_batch's), component [Z,K], pose [Z,K,4,4], rest [Z,K,n,3], object_of [Z,K]
    (datapipe.pile's), count [Z] (integers on the device) or None -> PileEvaluation of tensors: the three ratios [Z] float64 (NaN
    for an empty denominator), n_components [Z] int64, exact [Z] bool, msd [Z,K,K] float64.  K passes of element-wise work on
    [Z,K,n] values, no [Z,K,K,n] intermediate.  Nothing waits for the device."""
    _on_gpu("evaluate_pile_batch", G=G, component=component, pose=pose, rest=rest, object_of=object_of)
    if pose.dim() != 4 or tuple(pose.shape[2:]) != (4, 4):
        raise _lib.PznError(f"evaluate_pile_batch expects pose[Z,K,4,4]; got {tuple(pose.shape)}")
    Z, K = pose.shape[0], pose.shape[1]
    if tuple(G.shape) != (Z, K, 4, 4) or tuple(component.shape) != (Z, K) or tuple(object_of.shape) != (Z, K) or rest.dim() != 4 \
            or tuple(rest.shape[:2]) != (Z, K) or rest.shape[3] != 3 or (count is not None and tuple(count.shape) != (Z,)):
        raise _lib.PznError(f"evaluate_pile_batch expects G[{Z},{K},4,4], component[{Z},{K}], rest[{Z},{K},n,3], object_of[{Z},{K}], "
                            f"count[{Z}]; got {tuple(G.shape)}, {tuple(component.shape)}, {tuple(rest.shape)}, "
                            f"{tuple(object_of.shape)}")
    with torch.no_grad():
        comp = component.long()
        index = torch.arange(K, device=comp.device)
        live = index[None, :] < count[:, None] if count is not None else torch.ones_like(comp, dtype=torch.bool)
        together, belong = _pile_masks(comp, object_of.long(), live, index[:, None] != index[None, :])
        msd = _pile_msd(G.double(), pose.double(), rest.double())
        both = together & belong
        n = lambda m: m.sum(dim=(1, 2)).double()
        # a piece opens its component when no counted piece before it is in the same one
        opens = live & (comp >= 0) & ~(together & (index[None, :] < index[:, None])).any(dim=2)
        return PileEvaluation(n(both) / n(together), n(both) / n(belong), n(both & (msd < tol)) / n(belong), opens.sum(dim=1),
                              (together == belong).all(dim=2).all(dim=1), msd)


# --------------------------------------------------------------------------- the beam walk scored by the placed pieces' votes

BeamBatch = collections.namedtuple("BeamBatch", AssemblyBatch._fields + ("cost", "n_hyp"))
BeamRule = collections.namedtuple("BeamRule", WalkRule._fields + ("cost", "n_hyp"))


def boundary_moments(pieces, top_m):
    """The second-moment matrix of every piece's picked boundary points in homogeneous form, the `moment` input of
    assemble_beam_batch: pieces [Z,P,N,3] (float32, on the GPU), top_m [Z,P,k] (match_puzzles' field) -> [Z,P,4,4] float64 on the
    device, moment[z,p] = the mean over x = pieces[z,p][top_m[z,p]] of (x, 1) (x, 1)^T.  With it mean_x |Q x - G x|^2 is
    sum_u D_u M D_u^T over the rows of D = Q - G: what two poses of piece p disagree by on its boundary, with no point read.
    Nothing waits for the device."""
    _on_gpu("boundary_moments", top_m=top_m)
    _clouds("boundary_moments", "Z,P", pieces=pieces)
    Z, P, N = pieces.shape[0], pieces.shape[1], pieces.shape[2]
    if top_m.dim() != 3 or tuple(top_m.shape[:2]) != (Z, P) or top_m.shape[2] < 1 or top_m.dtype != torch.long:
        raise _lib.PznError(f"boundary_moments expects int64 top_m[{Z},{P},k]; got {top_m.dtype} {tuple(top_m.shape)}")
    with torch.no_grad():
        x = ops.index_points(pieces.contiguous().view(Z * P, N, 3), top_m.reshape(Z * P, -1)).view(Z, P, -1, 3).double()
        xh = torch.cat((x, torch.ones_like(x[..., :1])), dim=-1)
        return (xh.unsqueeze(-1) * xh.unsqueeze(-2)).mean(dim=2)


def _rule_products(A, B):
    """_rule_product on stacks [n,4,4] of float64 matrices, element-wise (every numpy operation rounds on its own)."""
    out = np.empty_like(A)
    for u in range(4):
        for v in range(4):
            out[:, u, v] = _dot4(A[:, u, 0], B[:, 0, v], A[:, u, 1], B[:, 1, v], A[:, u, 2], B[:, 2, v], A[:, u, 3], B[:, 3, v])
    return out


def _rule_inverses(T):
    """_rule_inverse on a stack [n,4,4]."""
    out = np.zeros_like(T)
    for u in range(3):
        for v in range(3):
            out[:, u, v] = T[:, v, u]
        out[:, u, 3] = -((T[:, 0, u] * T[:, 0, 3] + T[:, 1, u] * T[:, 1, 3]) + T[:, 2, u] * T[:, 2, 3])
    out[:, 3, 3] = 1.0
    return out


def _restart_charge(restart_cost, limit):
    """restart_cost as the rule reads it: None or NaN is max_score (limit) where that is finite, 0 otherwise."""
    if restart_cost is None or restart_cost != restart_cost:
        return limit if np.isfinite(limit) else 0.0
    return float(restart_cost)


def _beam_rule_body(who, restarts, score, T, moment, count, beam, branch, weight, max_score, vote_score, joint_score, restart_cost):
    """beam_rule (restarts False) and forest_beam_rule (True): one statement of the candidates, the child's pose, the votes, the
    selection and the result -> the fields of BeamRule or of ForestBeamRule.  A hypothesis is (inside, poses, edges, cost,
    component, roots).  Without restarts a hypothesis without a candidate has no child, a round without any child ends the walk,
    there is one component (so its pieces, the voters, are all the placed ones) and the forest's three fields do not exist."""
    M = _as_np(moment, np.float64)
    B, C, weight = int(beam), int(branch), float(weight)
    S, P, counts, limit = _rule_table(score, T, count, max_score, who, M)
    Z, K = S.shape[0], S.shape[1]
    if B < 1 or C < 1 or weight != weight:
        raise ValueError(f"{who}: beam = {B}, branch = {C} (>= 1), weight = {weight} (not NaN)")
    inf = float("inf")
    vlimit = limit if vote_score is None or vote_score != vote_score else float(vote_score)
    charge = _restart_charge(restart_cost, limit)
    out = _rule_outputs(Z, K)
    if restarts:
        out = ForestRule(*out, np.full((Z, K), -1, dtype=np.int32), np.full((Z, K), -1, dtype=np.int32), np.zeros(Z, dtype=np.int32))
    cost = np.full((Z, B), np.inf, dtype=np.float64)
    n_hyp = np.zeros(Z, dtype=np.int32)
    with np.errstate(all="ignore"):
        for z in range(Z):
            c = int(counts[z])
            if not 2 <= c <= K:
                continue
            raw = S[z, :c, :c].astype(np.float64)
            key = np.where(np.isnan(raw) | np.eye(c, dtype=bool), inf, raw) + 0.0            # (-0 is +0)
            key_rows = key.tolist()
            flat_of = np.arange(c)[:, None] * K + np.arange(c)[None, :]
            r = int(np.flatnonzero(key.reshape(-1) == key.min())[0]) // c                    # the first row-major position
            Pz, Mz = P[z].astype(np.float64), M[z]
            first = np.zeros(c, dtype=bool)
            first[r] = True
            pose0 = np.zeros((c, 4, 4))
            pose0[r] = np.eye(4)
            comp0 = np.full(c, -1, dtype=np.int64)
            comp0[r] = 0
            hyps = [(first, pose0, [], 0.0, comp0, [r])]
            for _ in range(c - 1):
                kids = []                                                    # (slot, rank, i, j, new, key); i = -1: a restart
                for slot, (inside, _, _, _, _, _) in enumerate(hyps):
                    at = np.flatnonzero((inside[:, None] != inside[None, :]).reshape(-1))
                    kv, fv = key.reshape(-1)[at], flat_of.reshape(-1)[at]
                    grown = False
                    for rank, q in enumerate(np.lexsort((fv, kv))[:C]):
                        if not np.isfinite(kv[q]) or kv[q] > limit:      # (as the walk stops: a key of -inf ends the list too)
                            break
                        i, j = divmod(int(fv[q]), K)
                        kids.append((slot, rank, i, j, j if inside[i] else i, float(kv[q])))
                        grown = True
                    if restarts and not grown:
                        outside = np.flatnonzero(~inside)
                        new = int(outside[0]) if len(outside) == 1 else _rule_root(key_rows, inside.tolist())
                        kids.append((slot, 0, -1, -1, new, charge))
                if not kids:                                                 # (with restarts every hypothesis has a child)
                    break
                # the children's poses: G[new] = G[i] T[i,j], or G[j] inv(T[i,j]); a restart's root has the identity
                grow = [ci for ci, kid in enumerate(kids) if kid[2] >= 0]
                Gn = np.tile(np.eye(4), (len(kids), 1, 1))
                if grow:
                    Tij = np.stack([Pz[kids[ci][2], kids[ci][3]] for ci in grow])
                    fwd = np.array([kids[ci][4] == kids[ci][3] for ci in grow])
                    src = np.stack([hyps[kids[ci][0]][1][kids[ci][2] if kids[ci][4] == kids[ci][3] else kids[ci][3]] for ci in grow])
                    Gn[grow] = _rule_products(src, np.where(fwd[:, None, None], Tij, _rule_inverses(Tij)))
                costs = [hyps[slot][3] + k for slot, _, _, _, _, k in kids]
                if weight != 0.0:
                    votes = []                                                               # (child, p, a, b) in vote order
                    for ci in grow:
                        slot, _, i, j, new, _ = kids[ci]
                        comp = hyps[slot][4]
                        for p in np.flatnonzero(comp == comp[i if new == j else j]):         # the joined component's pieces
                            for a, b in ((int(p), new), (new, int(p))):
                                if (a, b) != (i, j) and np.isfinite(key[a, b]) and key[a, b] <= vlimit:
                                    votes.append((ci, int(p), a, b))
                    total, n_votes = [0.0] * len(kids), [0] * len(kids)
                    if votes:
                        Tab = np.stack([Pz[a, b] for _, _, a, b in votes])
                        vfwd = np.array([a == p for _, p, a, _ in votes])
                        Gp = np.stack([hyps[kids[ci][0]][1][p] for ci, p, _, _ in votes])
                        Q = _rule_products(Gp, np.where(vfwd[:, None, None], Tab, _rule_inverses(Tab)))
                        D = Q[:, :3, :] - np.stack([Gn[ci, :3, :] for ci, _, _, _ in votes])
                        Mn = np.stack([Mz[kids[ci][4]] for ci, _, _, _ in votes])
                        qs = []
                        for u in range(3):
                            m = [_dot4(Mn[:, v, 0], D[:, u, 0], Mn[:, v, 1], D[:, u, 1], Mn[:, v, 2], D[:, u, 2], Mn[:, v, 3], D[:, u, 3])
                                 for v in range(4)]
                            qs.append(_dot4(D[:, u, 0], m[0], D[:, u, 1], m[1], D[:, u, 2], m[2], D[:, u, 3], m[3]))
                        d = ((qs[0] + qs[1]) + qs[2]).tolist()
                        for (ci, _, _, _), dv in zip(votes, d):
                            total[ci] = total[ci] + dv
                            n_votes[ci] += 1
                    for ci in grow:                                                          # (a restart has no penalty term)
                        costs[ci] = costs[ci] + weight * (total[ci] / n_votes[ci] if n_votes[ci] else 0.0)
                costs = [inf if x != x else x for x in costs]
                nxt, seen = [], set()
                for ci in sorted(range(len(kids)), key=lambda ci: (costs[ci], kids[ci][0], kids[ci][1])):
                    slot, _, i, j, new, _ = kids[ci]
                    inside = hyps[slot][0].copy()
                    inside[new] = True
                    if inside.tobytes() in seen:
                        continue
                    seen.add(inside.tobytes())
                    poses, comp = hyps[slot][1].copy(), hyps[slot][4].copy()
                    poses[new] = Gn[ci]
                    if i >= 0:
                        comp[new] = comp[i if new == j else j]
                        nxt.append((inside, poses, hyps[slot][2] + [(i, j, new)], costs[ci], comp, hyps[slot][5]))
                    else:
                        comp[new] = len(hyps[slot][5])
                        nxt.append((inside, poses, hyps[slot][2], costs[ci], comp, hyps[slot][5] + [new]))
                    if len(nxt) == B:
                        break
                hyps = nxt
            inside, poses, es, _, comp, rts = hyps[0]
            n_hyp[z] = len(hyps)
            cost[z, :len(hyps)] = [h[3] for h in hyps]
            out.root[z] = rts[0]
            if restarts:
                out.n_components[z] = len(rts)
                out.roots[z, :len(rts)] = rts
                out.component[z, :c] = comp
            _rule_finish(z, out, S, raw, es, {int(p): poses[p] for p in np.flatnonzero(inside)}, comp.tolist(), joint_score)
    return (*out, cost, n_hyp)


def beam_rule(score, T, moment, count=None, beam=4, branch=4, weight=1.0, max_score=None, vote_score=None, joint_score=None):
    """The numpy statement of ops.assemble_beam (csrc/assemblebeam.hip, the rule in include/pzn.h), which is held to it bit for
    bit, G and cost included.  score [Z,K,K] (read as float32), T [Z,K,K,4,4] (float32), moment [Z,K,4,4] (float64), count [Z]
    or None, tensors or arrays -> BeamRule: walk_rule's fields in its shapes and types, cost [Z,beam] float64 and n_hyp [Z] int32.

    Keys, ties, the root, the pose arithmetic and count are walk_rule's.  A hypothesis is a placed set with its poses, edges and
    a float64 cost; its candidates are the first `branch` ordered pairs with one end placed in the order (key, i K + j), keys
    finite and <= max_score.  A child costs (parent + key) + weight * penalty, penalty = the mean, summed in vote order, of the
    disagreement d of every other entry between a placed piece p (ascending; (p, n) then (n, p); keys finite and <= vote_score)
    and the new piece n: D = G[p] T[p,n] - Gn or G[p] inv(T[n,p]) - Gn on rows 0..2, d = sum_u D_u M[n] D_u^T with the rule's
    dot4 order.  The round's children are ordered by (cost, parent slot, rank) and the first `beam` distinct placed sets live on.
    The result is slot 0.  Written with element-wise float64 only: no matmul, whose summation order is not fixed."""
    return BeamRule(*_beam_rule_body("beam_rule", False, score, T, moment, count, beam, branch, weight, max_score, vote_score,
                                     joint_score, None))


def assemble_beam_batch(score, T, moment, count=None, beam=4, branch=4, weight=1.0, max_score=None, vote_score=None,
                        joint_score=None):
    """assemble_batch with a beam in place of the greedy walk, ONE launch for Z puzzles (ops.assemble_beam; beam_rule is its
    numpy statement): `beam` hypotheses live side by side, each extended by its `branch` smallest entries, and a child is
    charged its entry's score plus `weight` times how far the entries of the OTHER placed pieces put the new piece's boundary
    from where this entry puts it (moment = boundary_moments(pieces, table.top_m)) - the cycles a spanning tree never asks.
    weight = 1 is a definition: both terms are mean squared distances of the moved piece's k boundary points.  vote_score
    (None: max_score) is the largest score an entry may have to vote.  -> BeamBatch: AssemblyBatch's fields for the cheapest
    hypothesis, cost [Z,beam] float64 of all that lived (unused +inf) and n_hyp [Z] int32.  refine_assembly_batch and
    evaluate_batch take it as they take an AssemblyBatch.  beam = branch = 1 is assemble_batch bit for bit.  Nothing waits for
    the device."""
    root, edges, edge_score, n_edges, G, placed, joints, n_joints, cost, n_hyp = ops.assemble_beam(
        score, T, moment, count, beam, branch, weight, max_score, vote_score, joint_score)
    placed, movable = _placed_movable(placed, root)
    return BeamBatch(root, edges, edge_score, n_edges, G, placed, movable, joints, n_joints, cost, n_hyp)


# --------------------------------------------------------------------------- the forest beam: the beam walk over a mixed pile

ForestBeamBatch = collections.namedtuple("ForestBeamBatch", ForestBatch._fields + ("cost", "n_hyp"))
ForestBeamRule = collections.namedtuple("ForestBeamRule", ForestRule._fields + ("cost", "n_hyp"))


def forest_beam_rule(score, T, moment, count=None, beam=4, branch=4, weight=1.0, max_score=None, vote_score=None, joint_score=None,
                     restart_cost=None):
    """The numpy statement of ops.assemble_forest_beam (csrc/assemblebeam.hip, the rule in include/pzn.h), which is held
    to it bit for bit, G and cost included: beam_rule with forest_rule's restarts.  The arguments are beam_rule's and restart_cost
    (float; None or NaN: max_score where that is finite, else 0) -> ForestBeamRule: forest_rule's fields in its shapes and types,
    cost [Z,beam] float64 and n_hyp [Z] int32.

    Keys, ties, count, the stop test, the pose arithmetic, the candidates, a growth child's cost and the selection are
    beam_rule's.  A hypothesis also holds the component of every placed piece and the roots of its components; the new piece of a
    growth child joins the component of the candidate's placed end, and only the placed pieces of that component vote - the
    others live in unrelated frames.  A hypothesis without a candidate has one child of rank 0, a restart: forest_rule's new root
    (_rule_root over its outside pieces, or the one piece left) with the identity opens the next component, adds no edge and
    costs parent + restart_cost.  So every hypothesis has a child, every child places one piece, and there are exactly count - 1
    rounds.  The result is slot 0.  Single linkage under a threshold t minimises the sum of the edge scores + t (the number of
    components): the default restart_cost extends the beam's cost to that objective.

    beam = branch = 1 is forest_rule on every shared field; on a table where no live hypothesis ever lacks a candidate every
    shared field, cost and n_hyp are beam_rule's.  Element-wise float64 only, no matmul."""
    return ForestBeamRule(*_beam_rule_body("forest_beam_rule", True, score, T, moment, count, beam, branch, weight, max_score,
                                           vote_score, joint_score, restart_cost))


def assemble_forest_beam_batch(score, T, moment, count=None, beam=4, branch=4, weight=1.0, max_score=None, vote_score=None,
                               joint_score=None, restart_cost=None):
    """assemble_forest_batch with a beam in place of the greedy walk inside every component, ONE launch for Z piles
    (ops.assemble_forest_beam; forest_beam_rule is its numpy statement): assemble_beam_batch's hypotheses, candidates and votes,
    where a hypothesis that finds no admissible entry restarts from a new root as the forest walk does, at the price restart_cost
    (None: max_score where that is finite, else 0 - the threshold is what single linkage charges a component).  A piece is
    charged by the votes of the component it joins alone.  So a planted false match inside an object no longer carries the pieces
    behind it away, and the pile is still sorted.  A false entry between two objects that scores under max_score still merges
    them: no admissible entry votes against it.  -> ForestBeamBatch: ForestBatch's fields for the cheapest hypothesis (movable =
    placed and not the root of any component), cost [Z,beam] float64 of all that lived (unused +inf) and n_hyp [Z] int32.
    refine_assembly_batch and evaluate_pile_batch take it as they take a ForestBatch.  beam = branch = 1 is
    assemble_forest_batch bit for bit.  Nothing waits for the device."""
    root, edges, edge_score, n_edges, G, placed, joints, n_joints, component, roots, n_components, cost, n_hyp = \
        ops.assemble_forest_beam(score, T, moment, count, beam, branch, weight, max_score, vote_score, joint_score, restart_cost)
    placed, movable = _forest_movable(placed, roots)
    return ForestBeamBatch(root, edges, edge_score, n_edges, G, placed, movable, joints, n_joints, component, roots, n_components,
                           cost, n_hyp)


def pair_block_batch(model, pieces_f, codes_f, pieces_m, codes_m, k=128, refine=0, keep=1.0):
    """pair_block for Z puzzles, block-diagonal: pieces_f [Z,Kf,N,3] in the fixed role meet only the pieces_m [Z,Km,N,3] of their
    own puzzle -> PairBlock whose every field carries a leading Z (twist [Z,Kf,Km,6], T [Z,Kf,Km,4,4], de_fpcb [Z,Kf,Km,2,N], top_f
    [Z,Kf,Km,k], score [Z,Kf,Km]).  codes_* are PieceCodes whose fields are [Z,K,...] views of one encode_pieces call over Z K pieces.
    Every stage runs ONCE for all puzzles: the pose head's four layers on the Z Kf Km rows relu(U + V), se3.exp, one
    ops.pair_head_blocks launch, softmax and one topk_rows, one gather per side, then the transform and ops.chamfer or
    (refine > 0) the one ops.icp_refine launch.  de_fpcb has the same bits whatever Z is (the blocked head does not know about
    z); the fields behind the few-row layers agree between batches as two calls on the same batch do.  Nothing waits for the
    device.  keep as match_pairs documents it: anything but 1.0 on both sides replaces the transform and the chamfer, or the
    untrimmed launch, by the one trimmed ops.icp_refine launch (iters = refine, 0 included) -> TrimmedPairBlock with kept_f
    [Z,Kf,Km,m_f], kept_m [Z,Kf,Km,m_m]; 1.0 is today's path untouched and a PairBlock, whose kept_* are None; "auto" or an
    AutoKeep: the one auto launch -> AutoPairBlock (kept_* [Z,Kf,Km,k] padded with -1, count_f, count_m, objective [Z,Kf,Km])."""
    refine = _check_refine(refine, "pair_block_batch")
    _clouds("pair_block_batch", "Z,K", pieces_f=pieces_f, pieces_m=pieces_m)
    Z, Kf, N = pieces_f.shape[0], pieces_f.shape[1], pieces_f.shape[2]
    Km = pieces_m.shape[1]
    if pieces_m.shape[0] != Z or pieces_m.shape[2] != N or Z < 1 or Kf < 1 or Km < 1:
        raise _lib.PznError(f"pair_block_batch: pieces_f {tuple(pieces_f.shape)} and pieces_m {tuple(pieces_m.shape)} are not the "
                            "pieces of the same Z >= 1 puzzles")
    if tuple(codes_f.U.shape[:2]) != (Z, Kf) or tuple(codes_f.local_f.shape[:3]) != (Z, Kf, N) or tuple(codes_m.V.shape[:2]) != (Z, Km) \
            or tuple(codes_m.g_max.shape[:2]) != (Z, Km) or tuple(codes_m.top_m.shape[:2]) != (Z, Km):
        raise _lib.PznError(f"pair_block_batch: the codes are not [Z,K,...] views of Z = {Z} puzzles of {Kf} and {Km} pieces")
    k = int(k)
    counts = _keep_counts(keep, k, codes_m.top_m.shape[-1], "pair_block_batch")
    with torch.no_grad():
        # pose head: the four layers after the split first one run on the Z Kf Km rows relu(U_i + V_j)
        hidden = torch.relu(codes_f.U[:, :, None] + codes_m.V[:, None]).reshape(Z * Kf * Km, -1)
        twist = run_seq(list(model.tfMLP)[2:], hidden).view(Z, Kf, Km, 6)
        T = se3.exp(twist)

        y_f = _pair_fixed_head(model.MLPFpcb, codes_f.local_f, codes_m.g_max)                 # [Z,Kf,Km,N,2]
        de_fpcb = y_f.permute(0, 1, 2, 4, 3)

        # the k points of largest class-1 probability (softmax over two logits) and the boundary-to-boundary distance
        p_f = torch.softmax(y_f, dim=-1)[..., 1].reshape(Z * Kf * Km, N)
        top_f = ops.topk_rows(p_f, k).view(Z, Kf, Km, k)
        # pieces_f[z,i][top_f[z,i,j]] per pair, pieces_m[z,j][top_m[z,j]] per moved piece
        Bf = ops.index_points(pieces_f.reshape(Z * Kf, N, 3), top_f.reshape(Z * Kf, Km * k)).view(Z * Kf * Km, k, 3)
        Bm = ops.index_points(pieces_m.reshape(Z * Km, N, 3), codes_m.top_m.reshape(Z * Km, -1))
        if counts is not None or refine > 0:      # one refinement launch of counts' kind (trimmed and auto: no step at refine = 0)
            r = _refine_gathered(Bf, Bm, T, refine, counts)
            return _kind_of(counts).PairBlock(twist, r.T, de_fpcb, top_f, r.score, *r[len(Refined._fields):])
        Bm = Bm.view(Z, 1, Km, -1, 3).expand(Z, Kf, Km, -1, 3).reshape(Z * Kf * Km, -1, 3)
        d1, d2 = ops.chamfer(Bf, se3.transform_points(T.reshape(Z * Kf * Km, 4, 4), Bm))
        score = (d1.mean(dim=1) + d2.mean(dim=1)).view(Z, Kf, Km)
    return PairBlock(twist, T, de_fpcb, top_f, score)


def _match_puzzles(model, pieces, k, start, refine, who, keep=1.0):
    """match_puzzles' body -> (pieces contiguous, PieceCodes of [Z,P,...] views, the square PairBlock, diagonal not masked)."""
    refine = _check_refine(refine, who)
    _clouds(who, "Z,P", pieces=pieces)
    Z, P, N, _ = pieces.shape
    if Z < 1 or P < 2:
        raise _lib.PznError(f"{who}: Z = {Z} puzzles (>= 1) of P = {P} pieces (>= 2)")
    pieces = pieces.contiguous()
    flat = pieces.view(Z * P, N, 3)
    if start is not None:
        s1, s2 = (torch.as_tensor(s, dtype=torch.long) for s in start)
        if tuple(s1.shape) != (Z, P) or tuple(s2.shape) != (Z, P):
            raise _lib.PznError(f"{who}: start = (s1[{Z},{P}], s2[{Z},{P}]); got {tuple(s1.shape)}, {tuple(s2.shape)}")
        start = (s1.reshape(Z * P), s2.reshape(Z * P))
    codes = encode_pieces(model, flat, k, start, _who=who, _least=2)
    codes = PieceCodes(*(f.view(Z, P, *f.shape[1:]) for f in codes))
    return pieces, codes, pair_block_batch(model, pieces, codes, pieces, codes, k, refine, keep)


def match_puzzles(model, pieces, k=128, start=None, refine=0, keep=1.0):
    """match_pairs for Z puzzles of P pieces: pieces [Z,P,N,3] (float32, on the GPU) -> PairTable whose every field carries a
    leading Z (twist [Z,P,P,6], T [Z,P,P,4,4], de_fpcb [Z,P,P,2,N], de_mrpcb [Z,P,2,N], top_f [Z,P,P,k], top_m [Z,P,k],
    score [Z,P,P] with +inf on the diagonals, x2 [Z,P,256,3]).  The Z P pieces go through ONE encode_pieces, so the encoders run
    on full 64-row batches however small a puzzle is, and ONE pair_block_batch: the number of library launches does not depend on Z.
    start = (s1[Z,P], s2[Z,P]) as match_pairs takes its starts; refine and keep as match_pairs takes them (kept_f [Z,P,P,m_f],
    kept_m [Z,P,P,m_m]).  x2 is match_pairs' of the
    same puzzle and starts bit for bit; the fields behind the few-row layers (twist, and with it T and score) are not equal
    bit for bit between two calls of match_pairs either, and agree with it as two such calls do.  Nothing waits for the device."""
    pieces, codes, blk = _match_puzzles(model, pieces, k, start, refine, "match_puzzles", keep)
    return _table(codes, blk, _diagonal(pieces))


def refine_assembly_batch(pieces, table, asm, sweeps=30, kept=None, keep=None, auto=None):
    """refine_assembly for Z puzzles with no download: pieces [Z,P,N,3] (float32, on the GPU), table = match_puzzles' PairTable
    of them, asm = assemble_batch's AssemblyBatch of that table -> JointRefined whose fields carry a leading Z: G [Z,P,4,4]
    float32, score, score0, sweeps_used [Z], accepted [Z,P], joints = asm.joints (the device tensor, unused rows (-1, -1)).

    Joint row e = (i, j) of puzzle z pairs pieces[z,i][table.top_f[z,i,j]] with pieces[z,j][table.top_m[z,j]]; which rows those
    are is known only on the device, so ONE gather picks the set of every ordered pair and of every moved piece - Z P^2 + Z P
    sets of k points, 12 k Z P (P + 1) bytes (7.1 MB at Z = 64, P = 8, k = 128) - and the rows find theirs through
    a_of = z P^2 + i P + j and b_of = z P + j, computed from asm.joints in torch (unused rows map to set 0 and are skipped by
    the kernel).  G0 = asm.G rounded to float32, movable = asm.movable, then the one launch of ops.joint_refine for all Z
    puzzles.  Per puzzle the result is refine_assembly's bit for bit.  Nothing waits for the device.

    A table that carries kept sets (match_puzzles(..., keep < 1)): the set of ordered pair (z, i, j) is its kept rows,
    pieces[z,i][top_f[z,i,j][kept_f[z,i,j]]] and pieces[z,j][top_m[z,j][kept_m[z,i,j]]] - 2 Z P^2 sets of m_f and m_m points,
    b_of = a_of per ordered pair; the counts are the table's shapes, known on the host.  The kernel and its energy are the same,
    the untrimmed one over the rows the pair refinement kept: the joint refinement freezes the kept sets, it does not trim
    again.

    kept: refine_assembly's keyword.  An AutoPairTable is refused by default (PznUnsupported, AUTO_JOINT_MESSAGE); with
    kept="frozen" its 2 Z P^2 sets have stride k, the -1 padding of kept_* gathers row 0 of the set, and the counts travel as
    ops.joint_refine's na = count_f and nb = count_m, one per ordered pair and found by the kernel through the same a_of:
    one gather, one launch, nothing waits for the device.

    keep: refine_assembly's keyword (None: everything above, bit for bit, with no new launch).  The sets are then the full
    Z P^2 + Z P ones of the first form whatever the table carries, a fraction gives every row the counts ceil(f k), and "table"
    a TrimmedPairTable's kept widths or, for an AutoPairTable, count_f[z,i,j] and count_m[z,i,j] gathered on the device through
    the same a_of (an unused row gets pair (0, 0, 0)'s and is skipped).  -> TrimmedJointRefined with a leading Z: kept_f, kept_m
    [Z,J,k] (all -1 on an unused row), count_f, count_m [Z,J].  One gather, one launch, nothing waits for the device.

    auto: refine_assembly's keyword (None: everything above, bit for bit, with no new launch).  The full Z P^2 + Z P sets, the
    least counts ceil(least k) known on the host, the counts of every joint found by the kernel -> AutoJointRefined with a
    leading Z (count_f, count_m [Z,J]: 0 on an unused row; objective, objective0 [Z]).  One gather, one launch, nothing waits
    for the device."""
    auto = _auto_mode(auto, kept, keep, "refine_assembly_batch")
    mode = "auto" if auto is not None else _kept_mode(kept, table, "refine_assembly_batch", keep)
    _clouds("refine_assembly_batch", "Z,P", pieces=pieces)
    Z, P, N, _ = pieces.shape
    J = P * (P - 1)
    if tuple(table.top_f.shape[:3]) != (Z, P, P) or tuple(table.top_m.shape[:2]) != (Z, P) or tuple(asm.G.shape) != (Z, P, 4, 4) \
            or tuple(asm.joints.shape) != (Z, J, 2) or tuple(asm.movable.shape) != (Z, P):
        raise _lib.PznError(f"refine_assembly_batch: the table and the assembly are not those of Z = {Z} puzzles of P = {P} "
                            f"pieces: top_f {tuple(table.top_f.shape)}, top_m {tuple(table.top_m.shape)}, G {tuple(asm.G.shape)}, "
                            f"joints {tuple(asm.joints.shape)}")
    dev = pieces.device
    with torch.no_grad():
        ji, jj = asm.joints[..., 0].long(), asm.joints[..., 1].long()
        first = torch.arange(Z, dtype=torch.long, device=dev)[:, None]
        a_of = torch.where(ji >= 0, (first * P + ji) * P + jj, torch.zeros_like(ji))
        # the sets of all Z P^2 ordered pairs in row-major order: a joint row finds its pair, and through it its sets, by a_of
        z, i, j = (t.reshape(-1) for t in torch.meshgrid(*(torch.arange(n, dtype=torch.long, device=dev) for n in (Z, P, P)),
                                                         indexing="ij"))
        a, b, b_of, cnt_a, cnt_b = _joint_sets(pieces, table, z, i, j, full=mode is not None)
        b_of = a_of if b_of is None else b_of[a_of]
        if auto is not None:
            k = table.top_m.shape[-1]
            out = ops.joint_refine(a, b, asm.joints, asm.G.to(torch.float32), asm.movable, sweeps, a_of=a_of, b_of=b_of,
                                   auto=tuple(_keep_counts(auto, k, k, "refine_assembly_batch")), return_kept=True)
            return _auto_joint_refined(out, asm.joints)
        if mode is not None:
            ma, mb, m_f, m_m = _joint_keep_counts(mode, table, lambda t: t.reshape(-1)[a_of], (Z, J), "refine_assembly_batch")
            out = ops.joint_refine(a, b, asm.joints, asm.G.to(torch.float32), asm.movable, sweeps, a_of=a_of, b_of=b_of, ma=ma, mb=mb,
                                   return_kept=ma is not None)
            return _trimmed_joint_refined(out, asm.joints, asm.joints, ma, mb, m_f, m_m, table.top_m.shape[-1])
        G, score, score0, _, used_sweeps, accepted = ops.joint_refine(a, b, asm.joints, asm.G.to(torch.float32), asm.movable, sweeps,
                                                                      a_of=a_of, b_of=b_of, na=cnt_a, nb=cnt_b)
    return JointRefined(G, score, score0, used_sweeps, accepted, asm.joints)


def _mm(A, B):
    """[...,a,b] x [...,b,c] in the tensors' own type by products and one sum: small float64 matrices need no GEMM library."""
    return (A.unsqueeze(-1) * B.unsqueeze(-3)).sum(dim=-2)


def evaluate_batch(G, placed, pose, rest, root, edges=None, n_edges=None, mates=None, tol=0.01):
    """evaluate() for Z puzzles in float64 torch on the device, with its formulas (the atan2 form of the angle included): G
    [Z,P,4,4] (assemble_batch's, or refine_assembly_batch's), placed [Z,P] bool, pose [Z,P,4,4] and rest [Z,P,n,3]
    (datapipe.fracture's), root [Z] (integers) -> Evaluation of tensors: rot_deg, trans, msd [Z,P] float64, part_ok [Z,P] bool,
    part_accuracy [Z] float64 (the share of the pieces other than the root with part_ok) and edge_precision [Z] float64: with
    edges [Z,P-1,3], n_edges [Z] and mates [Z,P,P], the share of the first n_edges rows whose pair (i, j) is in mates, NaN for a
    puzzle without an edge; None without all three.  A puzzle with root < 0 (assemble_batch gave it no root) is measured in
    piece 0's frame with every piece counted: nothing is placed there, so its part accuracy is 0.  Nothing waits for the device."""
    _on_gpu("evaluate_batch", G=G, placed=placed, pose=pose, rest=rest, root=root)
    if pose.dim() != 4 or tuple(pose.shape[2:]) != (4, 4):
        raise _lib.PznError(f"evaluate_batch expects pose[Z,P,4,4]; got {tuple(pose.shape)}")
    Z, P = pose.shape[0], pose.shape[1]
    if tuple(G.shape) != (Z, P, 4, 4) or tuple(placed.shape) != (Z, P) or rest.dim() != 4 or tuple(rest.shape[:2]) != (Z, P) \
            or rest.shape[3] != 3 or tuple(root.shape) != (Z,):
        raise _lib.PznError(f"evaluate_batch expects G[{Z},{P},4,4], placed[{Z},{P}], rest[{Z},{P},n,3], root[{Z}]; got "
                            f"{tuple(G.shape)}, {tuple(placed.shape)}, {tuple(rest.shape)}, {tuple(root.shape)}")
    with torch.no_grad():
        G, X, R = G.double(), pose.double(), rest.double()
        rt = root.long()
        frame = rt.clamp(min=0)
        Rx, tx = X[..., :3, :3], X[..., :3, 3]
        inv = torch.zeros_like(X)                                                  # the rigid inverse of every pose
        inv[..., :3, :3] = Rx.transpose(-1, -2)
        inv[..., :3, 3] = -_mm(Rx.transpose(-1, -2), tx.unsqueeze(-1)).squeeze(-1)
        inv[..., 3, 3] = 1.0
        Xr = X[torch.arange(Z, device=X.device), frame]                            # [Z,4,4]
        Gt = _mm(Xr[:, None], inv)                                                 # the truth: pose[root] inv(pose[p])
        dR, dt = G[..., :3, :3] - Gt[..., :3, :3], G[..., :3, 3] - Gt[..., :3, 3]
        D = _mm(G[..., :3, :3], Gt[..., :3, :3].transpose(-1, -2))
        skew = torch.stack((D[..., 2, 1] - D[..., 1, 2], D[..., 0, 2] - D[..., 2, 0], D[..., 1, 0] - D[..., 0, 1]), dim=-1)
        trace = D[..., 0, 0] + D[..., 1, 1] + D[..., 2, 2]
        rot_deg = torch.rad2deg(torch.atan2(skew.norm(dim=-1), trace - 1.0))
        trans = dt.norm(dim=-1)
        x = _mm(R, Rx.transpose(-1, -2)) + tx.unsqueeze(-2)                        # the moved pieces
        d = _mm(x, dR.transpose(-1, -2)) + dt.unsqueeze(-2)
        msd = (d * d).sum(dim=-1).mean(dim=-1)
        part_ok = placed.bool() & (msd < tol)
        others = torch.arange(P, device=X.device)[None, :] != rt[:, None]
        part_accuracy = (part_ok & others).sum(dim=1).double() / others.sum(dim=1).double()
        edge_precision = None
        if edges is not None and n_edges is not None and mates is not None:
            ei, ej = edges[..., 0].long().clamp(min=0), edges[..., 1].long().clamp(min=0)
            live = torch.arange(edges.shape[1], device=X.device)[None, :] < n_edges[:, None]
            hit = (mates != 0)[torch.arange(Z, device=X.device)[:, None], ei, ej] & live
            edge_precision = hit.sum(dim=1).double() / live.sum(dim=1).double()      # 0 / 0: NaN where no edge was made
    return Evaluation(rot_deg, trans, msd, part_ok, part_accuracy, edge_precision)


# --------------------------------------------------------------------------- progressive assembly

def _choose(score, max_score=None):
    """The first row-major minimum off the diagonal of score[K,K] (host) -> (i, j, s), or None when it is not finite or
    above max_score."""
    S = np.array(score, dtype=np.float64)
    K = S.shape[0]
    S[np.arange(K), np.arange(K)] = np.inf
    S[np.isnan(S)] = np.inf
    i, j = divmod(int(np.argmin(S)), K)
    s = float(S[i, j])
    if not np.isfinite(s) or (max_score is not None and s > max_score):
        return None
    return i, j, s


class MergeLedger:
    """The host side of progressive assembly, float64: which original pieces every current part holds and where they sit.

      members   one list of original piece indices per current part (a part's label is the lowest of them)
      frame     per current part, the original piece whose frame the part lives in
      G [K,4,4] maps original piece p into the frame of the part that holds it
      edges     (label_i, label_j, score, dropped_a, dropped_b) in merge order"""

    def __init__(self, K):
        self.members = [[p] for p in range(K)]
        self.frame = list(range(K))
        self.G = np.tile(np.eye(4), (K, 1, 1))
        self.edges = []

    def label(self, part):
        return min(self.members[part])

    def merge(self, i, j, T_ij, score, dropped_a=None, dropped_b=None):
        """Part j, moved by T_ij (which maps it into part i's frame), joins part i and is removed from the list: parts
        after j move down one place -> the new index of the merged part."""
        if i == j:
            raise ValueError("a part cannot be merged with itself")
        T_ij = np.asarray(T_ij, dtype=np.float64)
        edge = (self.label(i), self.label(j), float(score), dropped_a, dropped_b)
        for p in self.members[j]:
            self.G[p] = T_ij @ self.G[p]
        self.members[i].extend(self.members[j])
        del self.members[j], self.frame[j]
        self.edges.append(edge)
        return i if i < j else i - 1


def _check_merge(who, N, k, drop_matched):
    """What both progressive walks ask before they start: two N-point parts must merge into one."""
    if drop_matched and 2 * k > N:
        raise _lib.PznError(f"{who}: drop_matched needs k <= N / 2 (k = {k}, N = {N}): the rows kept of a union must fill "
                            "the merged part")
    if not ops.merge_resample_supported(N, N, N):
        raise _lib.PznUnsupported(f"{who}: two parts of N = {N} points are not a union merge_resample takes")


def _del1(x, j):
    return torch.cat((x[:j], x[j + 1:]), dim=0)


def _del2(x, j):
    x = _del1(x, j)
    return torch.cat((x[:, :j], x[:, j + 1:]), dim=1)


class ProgressiveAssembler:
    """Progressive assembly: after every placement the two joined parts are merged into ONE N-point part (ops.merge_resample:
    the union resampled by farthest point sampling, the matched boundary points left out with drop_matched), the merged part
    is encoded alone and only its row and its column of the pair table are computed again.

    State: parts [K',N,3] (device), codes (their PieceCodes), table (their PairTable), piece_id / row_id [K',N] int64
    (which original piece and row every point is), starts (the FPS starts (s1, s2) of every current part, host lists),
    and the MergeLedger fields members, G, edges.  pieces, k, start as match_pairs takes them; max_score stops the walk
    at the first minimum above it; generator draws the merges' start rows (torch.randint(0, N) on the host, K - 1 draws
    at construction).  refine = N > 0: every pose of the table is refined on its picked rows (refine_pairs; the whole table
    once, then only the new row and column of a round - kept entries stay bit for bit), so the merge moves the part by the
    refined pose and the ledger records it.  Inference only: eval mode, no_grad, fp32, one GPU."""

    def __init__(self, model, pieces, k=128, start=None, max_score=None, drop_matched=True, generator=None, refine=0):
        K, N, k = _check_pieces(model, pieces, k, "ProgressiveAssembler", 2)
        _check_merge("ProgressiveAssembler", N, k, drop_matched)
        self.model, self.k, self.max_score, self.drop_matched = model, k, max_score, bool(drop_matched)
        self.refine = _check_refine(refine, "ProgressiveAssembler")
        dev = pieces.device
        if start is None:
            s1, s2 = draw_fps_starts(1, K, N, getattr(model, "fps_generator", None))
        else:
            s1, s2 = (torch.as_tensor(s, dtype=torch.long).cpu() for s in start)
        self._s1, self._s2 = s1.tolist(), s2.tolist()
        self.parts = pieces.contiguous().clone()
        self.codes = encode_pieces(model, self.parts, k, (s1, s2), _who="ProgressiveAssembler", _least=2)
        blk = pair_block(model, self.parts, self.codes, self.parts, self.codes, k, self.refine)
        self.table = _table(self.codes, blk, _diagonal(self.parts))
        self.piece_id = torch.arange(K, dtype=torch.long, device=dev)[:, None].expand(K, N).contiguous()
        self.row_id = torch.arange(N, dtype=torch.long, device=dev)[None].expand(K, N).contiguous()
        self.ledger = MergeLedger(K)
        stage = torch.empty((K - 1,), dtype=torch.long, pin_memory=True)
        torch.randint(0, N, (K - 1,), dtype=torch.long, generator=generator, out=stage)
        self.merge_starts = stage.tolist()
        self._merge_starts = stage.to(dev, non_blocking=True)
        self._stage = stage      # (alive until the copy has run)
        self.rounds = 0

    members = property(lambda self: self.ledger.members)
    G = property(lambda self: self.ledger.G)
    edges = property(lambda self: self.ledger.edges)

    @property
    def starts(self):
        return torch.tensor(self._s1, dtype=torch.long), torch.tensor(self._s2, dtype=torch.long)

    def step(self):
        """One round -> the edge made, or None when one part is left, the smallest score is not finite or it is above
        max_score.  One wait for the device: the download of the scores and poses the choice is made from."""
        t = self.table
        Kp, N, k = self.parts.shape[0], self.parts.shape[1], self.k
        if Kp < 2:
            return None
        with torch.no_grad():
            # 1. choose the pair (scores and poses in one download)
            host = torch.cat((t.score.reshape(-1), t.T.reshape(-1))).cpu().double().numpy()
            pick = _choose(host[:Kp * Kp].reshape(Kp, Kp), self.max_score)
            if pick is None:
                return None
            i, j, s = pick
            T_ij = host[Kp * Kp:].reshape(Kp, Kp, 4, 4)[i, j]

            # 2. merge: part j moved into part i's frame, the union resampled to N points
            da = t.top_f[i, j].reshape(1, k) if self.drop_matched else None
            db = t.top_m[j].reshape(1, k) if self.drop_matched else None
            u = self._merge_starts[self.rounds:self.rounds + 1]
            merged, src = ops.merge_resample(self.parts[i:i + 1], self.parts[j:j + 1], t.T[i, j].reshape(1, 4, 4), u, N, da, db)
            pid = torch.cat((self.piece_id[i], self.piece_id[j]))
            rid = torch.cat((self.row_id[i], self.row_id[j]))
            dropped = (None, None)
            if self.drop_matched:
                dropped = (torch.stack((self.piece_id[i][da[0]], self.row_id[i][da[0]]), dim=1),
                           torch.stack((self.piece_id[j][db[0]], self.row_id[j][db[0]]), dim=1))
            pid, rid = pid[src[0]], rid[src[0]]

            # 3. host bookkeeping
            n = self.ledger.merge(i, j, T_ij, s, *dropped)
            del self._s1[j], self._s2[j]
            self._s1[n] = self._s2[n] = 0
            self.rounds += 1

            # 4. the merged part comes out in pick order: its sampling plan costs no FPS
            plan = pick_order_plan(merged)

            # 5. encode the merged part alone; its row and its column of the table; row and column j leave
            code = encode_pieces(self.model, merged, k, plan=plan, _who="ProgressiveAssembler")
            self.parts = _del1(self.parts, j)
            self.parts[n] = merged[0]
            self.piece_id, self.row_id = _del1(self.piece_id, j), _del1(self.row_id, j)
            self.piece_id[n], self.row_id[n] = pid, rid
            fields = []
            for old, new in zip(self.codes, code):
                old = _del1(old, j)
                old[n] = new[0]
                fields.append(old)
            self.codes = PieceCodes(*fields)
            row = pair_block(self.model, merged, code, self.parts, self.codes, k, self.refine)      # [1, K' - 1]
            col = pair_block(self.model, self.parts, self.codes, merged, code, k, self.refine)      # [K' - 1, 1]
            upd = []
            for name in PairBlock._fields:
                x = _del2(getattr(t, name), j)
                x[:, n] = getattr(col, name)[:, 0]
                x[n] = getattr(row, name)[0]
                upd.append(x)
            upd = PairBlock(*upd)
            upd.score[n, n] = float("inf")
            self.table = _table(self.codes, upd)
        return self.ledger.edges[-1]

    def run(self):
        while self.step() is not None:
            pass
        return self.result()

    def result(self):
        """-> Progressive(G, edges, placed [K] bool, cloud [N,3], piece_id [N], row_id [N], parts [K',N,3]): cloud and its two
        provenance rows are those of the part that holds the first edge's fixed piece (part 0 when no edge was made);
        placed marks the pieces in that part, and none without an edge."""
        K = self.ledger.G.shape[0]
        placed = np.zeros(K, dtype=bool)
        root = 0
        if self.ledger.edges:
            first = self.ledger.edges[0][0]
            root = next(q for q, mem in enumerate(self.ledger.members) if first in mem)
            placed[self.ledger.members[root]] = True
        return Progressive(self.ledger.G.copy(), list(self.ledger.edges), placed, self.parts[root], self.piece_id[root],
                           self.row_id[root], self.parts)


def assemble_progressive(model, pieces, k=128, start=None, max_score=None, drop_matched=True, generator=None, refine=0):
    """ProgressiveAssembler(...).step() until one part is left or the walk stops -> Progressive."""
    return ProgressiveAssembler(model, pieces, k, start, max_score, drop_matched, generator, refine).run()


# --------------------------------------------------------------------------- progressive assembly, a batch of puzzles in lockstep

ProgressiveState = ops.ProgressiveState
ProgressiveBatchResult = collections.namedtuple(
    "ProgressiveBatchResult", "G edges edge_score n_edges root placed part alive parts piece_id row_id dropped")


def progressive_start(Z, P, count=None):
    """The fresh state of Z progressive walks over P slots as numpy arrays, in the kernel's shapes and types (ops.progressive_state
    is the same on the device) -> ProgressiveState(alive [Z,P] uint8, part [Z,P] int32, G [Z,P,4,4] float64, done [Z] uint8,
    n_edges [Z] int32, edges [Z,P-1,4] int32, edge_score [Z,P-1] float32): slots at or beyond count[z] start dead."""
    alive = np.ones((Z, P), dtype=np.uint8)
    if count is not None:
        alive = (np.arange(P)[None, :] < np.asarray(count, dtype=np.int64).reshape(Z, 1)).astype(np.uint8)
    return ProgressiveState(alive, np.tile(np.arange(P, dtype=np.int32), (Z, 1)), np.tile(np.eye(4), (Z, P, 1, 1)),
                            np.zeros(Z, dtype=np.uint8), np.zeros(Z, dtype=np.int32), np.full((Z, P - 1, 4), -1, dtype=np.int32),
                            np.full((Z, P - 1), np.inf, dtype=np.float32))


def progressive_round_rule(score, T, state, max_score=None):
    """The numpy statement of ops.progressive_round (csrc/progressive.hip, the rule in include/pzn.h), which is held to it bit for
    bit, G included: one round of Z progressive walks on the host.  score [Z,P,P] (read as float32), T [Z,P,P,4,4] (float32),
    state = a ProgressiveState (tensors or arrays; it is not changed) -> (the new ProgressiveState of numpy arrays, took [Z] uint8,
    pick [Z,2] int64).

    Slots are not compacted: a merged part stays in the fixed part's slot i and slot j dies, so row-major order over the live
    slots is the compacted order of ProgressiveAssembler and "the first row-major minimum" is the same pair as _choose's.
    Key of (i, j): its float32 score; NaN, the diagonal and any pair with a dead end count as +inf; keys compare as floats, ties
    to the lowest i P + j.  Stop (done = 1, took = 0, pick = (0, 0), nothing else changes): done is set, fewer than two slots are
    alive, n_edges is outside [0, P - 2], the smallest key is not finite or it is above max_score.  Merge otherwise: for every p
    with part[p] == j, G[p] = T[i,j] G[p] (_rule_product: float64 from the float32 T, every operation rounded on its own) and
    part[p] = i; alive[j] = 0; the row (label_i, label_j, i, j) - a label is the part's lowest member piece, before the merge -
    and the score as stored are appended; took = 1, pick = (i, j)."""
    S, X = _as_np(score, np.float32), _as_np(T, np.float32)
    Z, P = S.shape[0], S.shape[1]
    if S.shape != (Z, P, P) or X.shape != (Z, P, P, 4, 4) or P < 2:
        raise ValueError(f"progressive_round_rule expects score[Z,P,P], T[Z,P,P,4,4] with P >= 2; got {S.shape}, {X.shape}")
    types = (np.uint8, np.int32, np.float64, np.uint8, np.int32, np.int32, np.float32)
    alive, part, G, done, n_edges, edges, edge_score = (_as_np(f, dt).copy() for f, dt in zip(state, types))
    took = np.zeros(Z, dtype=np.uint8)
    pick = np.zeros((Z, 2), dtype=np.int64)
    inf = float("inf")
    limit = inf if max_score is None else float(max_score)
    for z in range(Z):
        live = [s for s in range(P) if alive[z, s]]
        ne = int(n_edges[z])
        stop = bool(done[z]) or len(live) < 2 or not 0 <= ne < P - 1
        if not stop:
            raw = S[z].tolist()                          # float32 values as Python floats (exact)
            best, at = inf, None                         # the first row-major position of the smallest key
            for i in live:
                for j in live:
                    key = inf if (i == j or raw[i][j] != raw[i][j]) else raw[i][j]
                    if at is None or key < best:
                        best, at = key, (i, j)
            stop = not np.isfinite(best) or best > limit
        if stop:
            done[z] = 1
            continue
        i, j = at
        Tij = X[z, i, j].astype(np.float64).tolist()
        label = lambda s: min((p for p in range(P) if part[z, p] == s), default=s)
        row = (label(i), label(j), i, j)
        for p in range(P):
            if part[z, p] == j:
                G[z, p] = np.array(_rule_product(Tij, G[z, p].tolist()), dtype=np.float64)
                part[z, p] = i
        alive[z, j] = 0
        edges[z, ne] = row
        edge_score[z, ne] = S[z, i, j]
        n_edges[z] = ne + 1
        took[z] = 1
        pick[z] = (i, j)
    return ProgressiveState(alive, part, G, done, n_edges, edges, edge_score), took, pick


class ProgressiveBatch:
    """ProgressiveAssembler for Z puzzles of P pieces in lockstep, with no host in between: every round ALL puzzles choose their
    merge in one launch (ops.progressive_round; progressive_round_rule is its statement), merge in one launch
    (ops.merge_resample), encode the Z merged parts in ONE encode_pieces call - the encoders see batches of Z, not of 1 - and compute
    the new row [Z,1,P] and the new column [Z,P,1] of all Z tables by one pair_block_batch each.

    Slots are not compacted: a merged part stays in the fixed part's slot i, slot j dies; shapes never change and the part in slot s
    lives in original piece s's frame.  State, all on the device: parts [Z,P,N,3], codes (PieceCodes of [Z,P,...]), table (PairTable
    with a leading Z; rows and columns of dead slots and the diagonal have score +inf), piece_id / row_id [Z,P,N] int64 (which
    original piece and row every point is), ledger (ops.ProgressiveState: alive, part, G float64, done, n_edges, edges, edge_score),
    took / pick of the last round, dropped (per round, the (piece, row) pairs the merges left out).

    pieces [Z,P,N,3], k, refine as match_puzzles takes them; start = (s1[Z,P], s2[Z,P]); max_score stops a puzzle at its first
    minimum above it (the others go on); merge_starts [Z,P-1] int64 are the merges' start rows, drawn with torch.randint(0, N) from
    `generator` when None; count [Z]: the pieces of every puzzle, slots at or beyond it start dead.  A stopped puzzle keeps every bit
    of its state: what a round computed for it is discarded through torch.where(took, new, old).  Every table entry outside row i,
    column i and the dead slots is kept bit for bit.

    Not done here: dead slots are still paired every round (up to half of the block work is wasted) and stopped puzzles are
    still encoded.  The finished parts are refined jointly by refine_progressive_batch(pieces, result), from the dropped rows
    the result carries (drop_matched=True).  Inference only: eval mode, no_grad, fp32, one GPU."""

    def __init__(self, model, pieces, k=128, start=None, max_score=None, drop_matched=True, generator=None, merge_starts=None,
                 refine=0, count=None):
        who = "ProgressiveBatch"
        self.refine = _check_refine(refine, who)
        if isinstance(pieces, torch.Tensor) and pieces.dim() == 4:
            _check_pieces(model, pieces[0], k, who, 2)
        pieces, codes, blk = _match_puzzles(model, pieces, k, start, self.refine, who)
        Z, P, N, _ = pieces.shape
        k = int(k)
        _check_merge(who, N, k, drop_matched)
        if not ops.progressive_round_supported(P):
            raise _lib.PznUnsupported(f"{who}: P = {P} pieces a puzzle (2 <= P <= 64)")
        if max_score is not None and float(max_score) != float(max_score):
            raise _lib.PznError(f"{who}: max_score is NaN (None: no limit)")
        self.model, self.k, self.max_score, self.drop_matched = model, k, max_score, bool(drop_matched)
        dev = pieces.device
        with torch.no_grad():
            if count is not None:
                count = torch.as_tensor(count).to(dev)
                if tuple(count.shape) != (Z,) or count.dtype.is_floating_point:
                    raise _lib.PznError(f"{who}: count must be {Z} integers; got {count.dtype} {tuple(count.shape)}")
            self.ledger = ops.progressive_state(Z, P, dev, count)
            if merge_starts is None:
                stage = torch.empty((Z, P - 1), dtype=torch.long, pin_memory=True)
                torch.randint(0, N, (Z, P - 1), dtype=torch.long, generator=generator, out=stage)
                self._stage = stage      # (alive until the copy has run)
                merge_starts = stage.to(dev, non_blocking=True)
            else:
                merge_starts = torch.as_tensor(merge_starts)
                if tuple(merge_starts.shape) != (Z, P - 1) or merge_starts.dtype != torch.long:
                    raise _lib.PznError(f"{who}: merge_starts must be int64 [{Z},{P - 1}]; got {merge_starts.dtype} "
                                        f"{tuple(merge_starts.shape)}")
                merge_starts = merge_starts.to(dev)
            self.merge_starts = merge_starts
            self.parts = pieces.clone()
            self.codes = codes
            self._eye = _diagonal(pieces)
            self._z = torch.arange(Z, dtype=torch.long, device=dev)
            self._y_f = blk.de_fpcb.permute(0, 1, 2, 4, 3)      # the kernel's [Z,P,P,N,2]; de_fpcb is its permuted view
            self._twist, self._T, self._top_f = blk.twist, blk.T, blk.top_f
            self._score = blk.score.masked_fill(self._dead(), float("inf"))
            self.piece_id = torch.arange(P, dtype=torch.long, device=dev)[None, :, None].expand(Z, P, N).contiguous()
            self.row_id = torch.arange(N, dtype=torch.long, device=dev)[None, None, :].expand(Z, P, N).contiguous()
            self.took = torch.zeros((Z,), dtype=torch.uint8, device=dev)
            self.pick = torch.zeros((Z, 2), dtype=torch.long, device=dev)
        self.dropped = []
        self.rounds = 0

    def _dead(self):
        """[Z,P,P] bool: the diagonal and every pair with a dead end."""
        a = self.ledger.alive.bool()
        return ~(a[:, :, None] & a[:, None, :]) | self._eye

    @property
    def table(self):
        return _table(self.codes, PairBlock(self._twist, self._T, self._y_f.permute(0, 1, 2, 4, 3), self._top_f, self._score))

    def step(self):
        """One round of all Z puzzles.  Nothing here waits for the device: the picks stay there, every gather and every write-back
        is indexed by them, and whether a puzzle took its merge is a torch.where."""
        Z, P, N = self.parts.shape[0], self.parts.shape[1], self.parts.shape[2]
        if self.rounds >= P - 1:
            raise _lib.PznError(f"ProgressiveBatch: all {P - 1} rounds of P = {P} pieces are made")
        k, z = self.k, self._z
        with torch.no_grad():
            # 1. every puzzle chooses (and its ledger is updated) on the device
            took, pick = ops.progressive_round(self._score, self._T, self.ledger, self.max_score)
            i, j = pick[:, 0], pick[:, 1]
            tk = took.bool()
            wide = lambda t: tk.view(Z, *([1] * (t.dim() - 1)))

            # 2. merge: part j moved into part i's frame, the union resampled to N points; Z merges, one launch
            da = self._top_f[z, i, j] if self.drop_matched else None
            db = self.codes.top_m[z, j] if self.drop_matched else None
            merged, src = ops.merge_resample(self.parts[z, i], self.parts[z, j], self._T[z, i, j], self.merge_starts[:, self.rounds],
                                             N, da, db)
            pid = torch.cat((self.piece_id[z, i], self.piece_id[z, j]), dim=1).gather(1, src)
            rid = torch.cat((self.row_id[z, i], self.row_id[z, j]), dim=1).gather(1, src)
            if self.drop_matched:
                rows = torch.stack((torch.stack((self.piece_id[z, i].gather(1, da), self.row_id[z, i].gather(1, da)), dim=-1),
                                    torch.stack((self.piece_id[z, j].gather(1, db), self.row_id[z, j].gather(1, db)), dim=-1)), dim=1)
                self.dropped.append(torch.where(wide(rows), rows, torch.full_like(rows, -1)))          # [Z,2,k,2]
            self.rounds += 1

            # 3. the merged parts come out in pick order: their sampling plans cost no FPS; one encode_pieces over all Z
            code = encode_pieces(self.model, merged, k, plan=pick_order_plan(merged), _who="ProgressiveBatch")

            # 4. the state of a puzzle that took its merge moves on, slot i; a stopped one is written back as it was
            def put(old, new):
                old[z, i] = torch.where(wide(new), new, old[z, i])
            put(self.parts, merged)
            put(self.piece_id, pid)
            put(self.row_id, rid)
            for old, new in zip(self.codes, code):
                put(old, new)

            # 5. the new row and the new column of all Z tables, one blocked launch chain each
            one = PieceCodes(*(f.unsqueeze(1) for f in code))
            m1 = merged.unsqueeze(1)
            row = pair_block_batch(self.model, m1, one, self.parts, self.codes, k, self.refine)      # [Z,1,P]
            col = pair_block_batch(self.model, self.parts, self.codes, m1, one, k, self.refine)      # [Z,P,1]
            for old, r, c in ((self._twist, row.twist, col.twist), (self._T, row.T, col.T),
                              (self._y_f, row.de_fpcb.permute(0, 1, 2, 4, 3), col.de_fpcb.permute(0, 1, 2, 4, 3)),
                              (self._top_f, row.top_f, col.top_f), (self._score, row.score, col.score)):
                old[z, :, i] = torch.where(wide(c[:, :, 0]), c[:, :, 0], old[z, :, i])
                old[z, i] = torch.where(wide(r[:, 0]), r[:, 0], old[z, i])
            self._score.masked_fill_(self._dead(), float("inf"))
            self.took, self.pick = took, pick
        return took, pick

    def run(self):
        """The P - 1 rounds (a count the host knows: stopped puzzles idle) -> result()."""
        while self.rounds < self.parts.shape[1] - 1:
            self.step()
        return self.result()

    def result(self):
        """-> ProgressiveBatchResult of device tensors: G [Z,P,4,4] float64, edges [Z,P-1,4] int32 rows (label_i, label_j, i, j),
        edge_score [Z,P-1], n_edges [Z], root [Z] int32 (the slot - and so the frame piece - of the part that holds the first edge's
        fixed piece; -1 without an edge), placed [Z,P] bool (the members of that part; none without an edge), part, alive, parts,
        piece_id, row_id (the final state) and dropped [rounds,Z,2,k,2] int64 (per round and side - fixed, moved - the (piece, row)
        pairs left out; -1 where the puzzle made no merge; None without drop_matched).  It feeds evaluate_batch(r.G, r.placed,
        pose, rest, r.root, r.edges, r.n_edges, mates) as it is.  Nothing waits for the device."""
        s = self.ledger
        with torch.no_grad():
            has = s.n_edges > 0
            first = s.edges[:, 0, 0].long().clamp(min=0)
            root = torch.where(has, s.part.gather(1, first[:, None])[:, 0], torch.full_like(s.n_edges, -1))
            placed = (s.part == root[:, None]) & has[:, None]
            dropped = torch.stack(self.dropped, dim=0) if self.dropped else None
        return ProgressiveBatchResult(s.G, s.edges, s.edge_score, s.n_edges, root, placed, s.part, s.alive.bool(), self.parts,
                                      self.piece_id, self.row_id, dropped)


def assemble_progressive_batch(model, pieces, k=128, start=None, max_score=None, drop_matched=True, generator=None,
                               merge_starts=None, refine=0, count=None):
    """ProgressiveBatch(...).run(): the P - 1 lockstep rounds of Z puzzles -> ProgressiveBatchResult."""
    return ProgressiveBatch(model, pieces, k, start, max_score, drop_matched, generator, merge_starts, refine, count).run()


# --------------------------------------------------------------------------- progressive assembly, the joint refinement of a finished part

# refine_progressive / refine_progressive_batch: JointRefined's fields (G [...,P,4,4] float32, score, score0, sweeps_used [...],
# accepted [...,P], joints [...,J,2] int32 rows (fixed piece, moved piece), unused rows (-1, -1)), then joint_score [...,J], count_f,
# count_m [...,J] (int32: the points of either side of a joint, 0 on an unused row) and rows_f, rows_m [...,J,k] (int64: the rows
# of pieces[p] and pieces[q] they are, -1 behind the count); J = P (P - 1) / 2
ProgressiveJointRefined = collections.namedtuple(
    "ProgressiveJointRefined", JointRefined._fields + ("joint_score", "count_f", "count_m", "rows_f", "rows_m"))


def progressive_joints_rule(pieces, G, dropped, least=3):
    """The numpy statement of ops.progressive_joints (csrc/progjoints.hip, the rule in include/pzn.h), which is held to it bit for
    bit: the pose graph of Z progressive walks read off their ledgers.  pieces [Z,P,N,3] (read as float32), G [Z,P,4,4] (float64),
    dropped [R,Z,2,k,2] (int64: per round and side - fixed, moved - the (piece, row) pairs of a merge), least >= 1 -> (joints
    [Z,J,2] int32, a, b [Z,J,k,3] float32, na, nb [Z,J] int32, rows_a, rows_b [Z,J,k] int64), J = P (P - 1) / 2.

    Per round and puzzle: an entry with 0 <= piece < P and 0 <= row < N is valid, every other one is skipped, and a round with a
    side without a valid entry yields nothing.  A valid entry's point goes to its part's frame in float64, x' = ((g00 x + g01 y) +
    g02 z) + g03 with every operation rounded on its own; every valid entry takes the nearest valid entry of the other side by
    d2 = (dx dx + dy dy) + dz dz, ties to the lowest list position.  For a fixed piece p and a moved piece q != p, A = the fixed
    entries on p whose nearest lies on q, B = the moved entries on q whose nearest lies on p, both in list order; with |A| >= least
    and |B| >= least the joint (p, q) fills row hi (hi - 1) / 2 + lo of the pair {lo, hi}.  Unused rows: joints -1, points 0,
    rows -1, counts 0.  A row that two rounds emit keeps the later round's."""
    X, Gd, D = _as_np(pieces, np.float32), _as_np(G, np.float64), _as_np(dropped, np.int64)
    if X.ndim != 4 or X.shape[3] != 3 or X.shape[1] < 2 or Gd.shape != X.shape[:2] + (4, 4) or D.ndim != 5 \
            or (D.shape[1], D.shape[2], D.shape[4]) != (X.shape[0], 2, 2) or int(least) < 1:
        raise ValueError(f"progressive_joints_rule expects pieces[Z,P,N,3] with P >= 2, G[Z,P,4,4], dropped[R,Z,2,k,2] and "
                         f"least >= 1; got {X.shape}, {Gd.shape}, {D.shape}, {least}")
    Z, P, N = X.shape[:3]
    R, k = D.shape[0], D.shape[3]
    J = P * (P - 1) // 2
    joints = np.full((Z, J, 2), -1, dtype=np.int32)
    pts = [np.zeros((Z, J, k, 3), dtype=np.float32) for _ in range(2)]
    cnt = [np.zeros((Z, J), dtype=np.int32) for _ in range(2)]
    rows = [np.full((Z, J, k), -1, dtype=np.int64) for _ in range(2)]
    for r in range(R):
        for z in range(Z):
            ok, own, row, moved = [], [], [], []
            for s in range(2):
                pi, ro = D[r, z, s, :, 0], D[r, z, s, :, 1]
                v = (pi >= 0) & (pi < P) & (ro >= 0) & (ro < N)
                x = X[z, np.where(v, pi, 0), np.where(v, ro, 0)].astype(np.float64)      # [k,3]
                g = Gd[z, np.where(v, pi, 0)]                                                # [k,4,4]
                moved.append(np.stack([((g[:, u, 0] * x[:, 0] + g[:, u, 1] * x[:, 1]) + g[:, u, 2] * x[:, 2]) + g[:, u, 3]
                                       for u in range(3)], axis=1))
                ok.append(v), own.append(pi), row.append(ro)
            if not ok[0].any() or not ok[1].any():
                continue
            facing = []
            for s in range(2):
                there = np.flatnonzero(ok[1 - s])
                d = moved[s][:, None, :] - moved[1 - s][None, there, :]
                d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
                facing.append(own[1 - s][there[np.argmin(d2, axis=1)]])                      # (argmin: the first of equal minima)
            sets = [{}, {}]                                                                  # (p, q) -> list positions, ascending
            for s in range(2):
                for e in np.flatnonzero(ok[s] & (own[s] != facing[s])):
                    pq = (int(own[s][e]), int(facing[s][e])) if s == 0 else (int(facing[s][e]), int(own[s][e]))
                    sets[s].setdefault(pq, []).append(int(e))
            for (p, q), A in sets[0].items():
                B = sets[1].get((p, q), [])
                if len(A) < least or len(B) < least:
                    continue
                lo, hi = min(p, q), max(p, q)
                e = hi * (hi - 1) // 2 + lo
                joints[z, e] = (p, q)
                for s, piece, members in ((0, p, A), (1, q, B)):
                    pts[s][z, e], rows[s][z, e] = 0, -1
                    pts[s][z, e, :len(members)] = X[z, piece, row[s][members]]
                    rows[s][z, e, :len(members)] = row[s][members]
                    cnt[s][z, e] = len(members)
    return joints, pts[0], pts[1], cnt[0], cnt[1], rows[0], rows[1]


def _check_progressive_refine(who, P, k, least):
    """What both refine_progressive forms ask before they touch a tensor."""
    if isinstance(least, bool) or not isinstance(least, numbers.Integral) or least < 1:
        raise _lib.PznError(f"{who}: least must be an integer >= 1; got {least!r}")
    if not ops.progressive_joints_supported(P, k):
        raise _lib.PznUnsupported(f"{who}: P = {P} pieces, k = {k} dropped rows a side (2 <= P <= 64, 1 <= k <= 1024)")
    if not ops.joint_refine_supported(P, P * (P - 1) // 2, k, k):
        raise _lib.PznUnsupported(f"{who}: a pose graph of P = {P} pieces, {P * (P - 1) // 2} joints and sets of k = {k} points is "
                                  "not one ops.joint_refine takes")


_NO_DROPPED = ("{who}: the walk recorded no dropped rows (drop_matched=False): the joints of a progressive part are read off the "
               "(piece, row) pairs its merges left out, and there is nothing else to read them from")


def refine_progressive_batch(pieces, result, sweeps=30, least=3):
    """The joint refinement of what assemble_progressive_batch built, with no download: pieces [Z,P,N,3] (float32, on the GPU,
    the ORIGINAL pieces), result = the walk's ProgressiveBatchResult -> ProgressiveJointRefined with a leading Z.

    The ledger composes one pose per merge, so G[p] carries the summed error of every merge between piece p and its part's frame
    piece, and a merge of two parts knows every pair of pieces that meet across it at once: result.dropped holds the rows.  One
    ops.progressive_joints launch turns them into a pose graph (its rule: progressive_joints_rule; a joint needs `least` points
    on either side; the sets are chosen once, under result.G, and not trimmed again - the choice of kept="frozen"), one
    ops.joint_refine launch with a count per set closes it: G0 = result.G rounded to float32, movable[z,p] = part[z,p] != p - a
    part lives in its slot piece's frame, so frame pieces stay, as do dead slots and single pieces.  Every part of a puzzle is
    refined in its own frame in the same launch.  The result feeds evaluate_batch(r.G, result.placed, pose, rest, result.root,
    ...) as refine_assembly_batch's does.  Nothing waits for the device.

    A result without dropped rows (drop_matched=False) is a PznError; P or k outside 2 <= P <= 64, 1 <= k <= 1024 is
    PznUnsupported; both before any tensor is touched."""
    who = "refine_progressive_batch"
    if result.dropped is None:
        raise _lib.PznError(_NO_DROPPED.format(who=who))
    _clouds(who, "Z,P", pieces=pieces)
    Z, P, N, _ = pieces.shape
    if result.dropped.dim() != 5 or tuple(result.G.shape) != (Z, P, 4, 4) or tuple(result.part.shape) != (Z, P) \
            or result.dropped.shape[1] != Z:
        raise _lib.PznError(f"{who}: the result is not that of Z = {Z} puzzles of P = {P} pieces: G {tuple(result.G.shape)}, part "
                            f"{tuple(result.part.shape)}, dropped {tuple(result.dropped.shape)}")
    k = result.dropped.shape[3]
    _check_progressive_refine(who, P, k, least)
    J = P * (P - 1) // 2
    with torch.no_grad():
        slot = torch.arange(P, dtype=result.part.dtype, device=result.part.device)
        movable = result.part != slot[None, :]
        joints, a, b, na, nb, rows_a, rows_b = ops.progressive_joints(pieces, result.G, result.dropped, least)
        G, score, score0, joint_score, used, accepted = ops.joint_refine(
            a.view(Z * J, k, 3), b.view(Z * J, k, 3), joints, result.G.float(), movable, sweeps, na=na.view(Z * J), nb=nb.view(Z * J))
    return ProgressiveJointRefined(G, score, score0, used, accepted, joints, joint_score, na, nb, rows_a, rows_b)


def progressive_frames(K, edges):
    """The frame piece of every piece's part from a walk's edges (rows that start with (label_i, label_j): the labels of the fixed
    and of the moved part, a label being a member piece) -> [K] int64: a merged part stays in the fixed part's frame."""
    frame = list(range(K))
    for edge in edges:
        fi, fj = frame[int(edge[0])], frame[int(edge[1])]
        frame = [fi if f == fj else f for f in frame]
    return np.array(frame, dtype=np.int64)


def refine_progressive(pieces, prog, sweeps=30, least=3):
    """refine_progressive_batch for one puzzle: pieces [K,N,3] (float32, on the GPU), prog = assemble_progressive's Progressive ->
    ProgressiveJointRefined without the leading axis.  It IS the batched function at Z = 1, so it gives its bits: dropped is
    stacked from prog.edges, and the frame piece of every part is rebuilt on the host from the edge labels (progressive_frames)."""
    who = "refine_progressive"
    if any(e[3] is None or e[4] is None for e in prog.edges):
        raise _lib.PznError(_NO_DROPPED.format(who=who))
    _clouds(who, "K", pieces=pieces)
    K = pieces.shape[0]
    if not prog.edges:
        raise _lib.PznError(f"{who}: the walk made no merge, so there is no part to refine")
    _check_progressive_refine(who, K, prog.edges[0][3].shape[0], least)
    dev = pieces.device
    with torch.no_grad():
        dropped = torch.stack([torch.stack((e[3], e[4]), dim=0) for e in prog.edges], dim=0)[:, None].to(dev)      # [R,1,2,k,2]
        part = torch.from_numpy(progressive_frames(K, prog.edges)).to(torch.int32)[None].to(dev)
        result = ProgressiveBatchResult(torch.as_tensor(np.asarray(prog.G, dtype=np.float64))[None].to(dev), None, None, None,
                                        None, None, part, None, None, None, None, dropped)
    out = refine_progressive_batch(pieces[None], result, sweeps, least)
    return ProgressiveJointRefined(*(f[0] for f in out))
