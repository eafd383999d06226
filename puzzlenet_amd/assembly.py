"""Multi-piece assembly: match every ordered pair of K pieces with each piece encoded ONCE, then
put the pieces together greedily by the distance between the matched boundaries (the reference's README describes this
end use and ships no code for it).

In eval mode nothing in predict5 mixes batch rows (BatchNorm1d(num_points) uses its running statistics, everything else
is per row), so the all-pairs table factors exactly:

  * Encoder and Encoder2 run once per piece (2 K encoder rows instead of 2 K (K - 1)) on ONE sampling / neighbour plan per
    piece: FPS and kNN depend on coordinates only.
  * Pose head: the first tfMLP layer on cat([ffpc_i, fmrpc_j]) is U_i + V_j with U = ffpc W1[:, :1024]^T and
    V = fmrpc W1[:, 1024:]^T + b1; the other four layers run on the K^2 rows relu(U_i + V_j).
  * Moved-side boundary head: both "global" vectors are the max over the MOVED piece's local features (model5_b.py:440,
    the reference's line 741), so de_mrpcb depends on j only: K rows.
  * Fixed-side boundary head: de_fpcb[i, j] = MLPFpcb(cat([g_j, local_i])), the only per-point work that depends on the
    pair: one launch of ops.pair_head (csrc/pointmlp.hip, pair_head_fwd_kernel), which computes the first-layer product
    of a tile once and loops over the moved pieces in registers.

Inference only: eval mode, torch.no_grad(), fp32, one GPU.  Out of scope: re-encoding merged pieces after each placement
(resampling the union to N points and matching again), any training on more than two pieces, and more than one GPU.
"""
import collections

import numpy as np
import torch

from . import _lib, ops, se3
from .model5_b import _run_seq, _run_seq_cat_global

PairTable = collections.namedtuple("PairTable", "twist T de_fpcb de_mrpcb top_f top_m score x2")
Assembly = collections.namedtuple("Assembly", "root edges G placed")

ENCODER_ROWS = 64      # pieces per encoder call (the fused per-point stem takes up to 64 clouds)


def _plan(model, pieces, s1, s2):
    """FPS -> gather -> FPS -> gather and the two neighbour searches of every piece: coordinates only, so both encoders of
    a piece use the same plan (the form TouchedRegraster.prefetch_plans hands to predict5)."""
    f1 = ops.farthest_point_sample(pieces, 512, s1)
    x1 = ops.index_points(pieces, f1)
    f2 = ops.farthest_point_sample(x1, 256, s2)
    x2 = ops.index_points(x1, f2)
    return (x1, ops.knn(pieces, x1, 32)), (x2, ops.knn(x1, x2, 32))


def _encode(enc, pieces, plan):
    """One encoder over all pieces, ENCODER_ROWS at a time -> (global feature [K,1024], per-point features [K,N,64])."""
    outs = []
    for a in range(0, pieces.shape[0], ENCODER_ROWS):
        b = a + ENCODER_ROWS
        sub = tuple((x[a:b], i[a:b]) for x, i in plan)
        r = enc(pieces[a:b], sub)
        outs.append((r[0], r[4]))
    if len(outs) == 1:
        return outs[0]
    return tuple(torch.cat(ts, dim=0) for ts in zip(*outs))


def _pair_fixed_head(seq, local, g):
    """MLPFpcb over every (fixed i, moved j) pair -> [K,K,N,2]: one pair_head launch, or (shapes it does not take) one
    boundary-head call per moved piece with its global vector expanded over the fixed pieces."""
    mods = list(seq)
    K, N = local.shape[0], local.shape[1]
    if len(mods) == 5 and ops.pair_head_supported(N, mods[2].out_features, mods[4].out_features):
        l1, l2, l3 = mods[0], mods[2], mods[4]
        return ops.pair_head(local, g, l1.weight, l1.bias, l2.weight, l2.bias, l3.weight, l3.bias)
    cols = [_run_seq_cat_global(seq, local, g[j:j + 1].expand(K, -1).reshape(K, 1, -1).contiguous()) for j in range(g.shape[0])]
    return torch.stack(cols, dim=1)


def match_pairs(model, pieces, k=128, start=None):
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
    is None).  Any K is taken: the encoders run on 64 pieces at a time.  Nothing here waits for the device."""
    if not isinstance(pieces, torch.Tensor) or not pieces.is_cuda:
        raise _lib.PznError("match_pairs: pieces must be a tensor on the GPU; puzzlenet_amd has no CPU fallback")
    if pieces.dim() != 3 or pieces.shape[2] != 3 or pieces.dtype != torch.float32:
        raise _lib.PznError(f"match_pairs expects float32 pieces[K,N,3]; got {pieces.dtype} {tuple(pieces.shape)}")
    K, N, _ = pieces.shape
    if K < 2 or N != model.num_points:
        raise _lib.PznError(f"match_pairs: K = {K} pieces (>= 2) of N = {N} points (the model takes {model.num_points})")
    k = int(k)
    if not 0 < k <= N:
        raise _lib.PznError(f"match_pairs: k = {k} of {N} points")
    pieces = pieces.contiguous()
    dev = pieces.device
    for m in (model.Encoder, model.Encoder2, model.tfMLP, model.fpc_decoder, model.rpc_decoder):
        if any(sm.training for sm in m.modules()):
            m.train(False)
    with torch.no_grad():
        if start is None:
            gen = getattr(model, "fps_generator", None)
            s1 = torch.randint(0, N, (K,), dtype=torch.long, generator=gen)
            s2 = torch.randint(0, 512, (K,), dtype=torch.long, generator=gen)
            stage = torch.empty((2, K), dtype=torch.long, pin_memory=True)
            torch.stack((s1, s2), out=stage)
            s1, s2 = stage.to(dev, non_blocking=True).unbind(0)
        else:
            s1, s2 = (torch.as_tensor(s, dtype=torch.long).to(dev, non_blocking=True) for s in start)
            if s1.shape != (K,) or s2.shape != (K,):
                raise _lib.PznError(f"match_pairs: start = (s1[{K}], s2[{K}]); got {tuple(s1.shape)}, {tuple(s2.shape)}")
        plan = _plan(model, pieces, s1, s2)

        cur = torch.cuda.current_stream(dev)
        side = model.side_stream()
        model.Encoder.need_out = model.Encoder2.need_out = False
        try:
            side.wait_stream(cur)
            with torch.cuda.stream(side):
                # Encoder2 and everything that depends on the moved piece alone: its local chain, the global vector
                # (model5_b.py:440 - the max over the MOVED piece's local features serves both heads) and de_mrpcb
                fmrpc, local_m = _encode(model.Encoder2, pieces, plan)
                local_m = _run_seq(model.MLPLocalPreRpc, local_m)
                g_max = ops.max_over_points(local_m)                                          # [K,64]
                de_mrpcb = _run_seq_cat_global(model.MLPRpcb, local_m, g_max.unsqueeze(1))    # [K,N,2]
            ffpc, local_f = _encode(model.Encoder, pieces, plan)
            local_f = _run_seq(model.MLPLocalPreFpc, local_f)
        finally:
            model.Encoder.need_out = model.Encoder2.need_out = True
        cur.wait_stream(side)
        for t in (fmrpc, g_max, de_mrpcb):                     # made on the side stream, used on this one
            t.record_stream(cur)
        for t in (pieces,) + tuple(t for lvl in plan for t in lvl):      # made on this stream, read on the side stream
            t.record_stream(side)

        # pose head: the first layer splits into a fixed and a moved half, the other four run on the K^2 rows
        mods = list(model.tfMLP)
        w1, b1 = mods[0].weight, mods[0].bias
        D = ffpc.shape[1]
        U = torch.empty((K, w1.shape[0]), dtype=torch.float32, device=dev)
        V = torch.empty_like(U)
        ffpc, fmrpc = ffpc.contiguous(), fmrpc.contiguous()
        with ops._on(dev):
            st = ops._stream()
            ops._call("pzn_linear_slice_fwd_f32", ffpc.data_ptr(), w1.data_ptr(), w1.shape[1], None, K, D, w1.shape[0], 0,
                      U.data_ptr(), st, flops=2 * K * D * w1.shape[0])
            ops._call("pzn_linear_slice_fwd_f32", fmrpc.data_ptr(), w1.data_ptr() + 4 * D, w1.shape[1], b1.data_ptr(), K,
                      w1.shape[1] - D, w1.shape[0], 0, V.data_ptr(), st, flops=2 * K * (w1.shape[1] - D) * w1.shape[0])
        hidden = torch.relu(U[:, None] + V[None]).reshape(K * K, -1)
        twist = _run_seq(mods[2:], hidden).view(K, K, 6)
        T = se3.exp(twist)

        y_f = _pair_fixed_head(model.MLPFpcb, local_f, g_max)                                # [K,K,N,2]
        de_fpcb = y_f.permute(0, 1, 3, 2)

        # the k points of largest class-1 probability (softmax over two logits) and the boundary-to-boundary distance
        p_f = torch.softmax(y_f, dim=-1)[..., 1].reshape(K * K, N)
        p_m = torch.softmax(de_mrpcb, dim=-1)[..., 1]
        top_f = ops.topk_rows(p_f, k).view(K, K, k)
        top_m = ops.topk_rows(p_m, k)
        Bf = ops.index_points(pieces, top_f.reshape(K, K * k)).view(K * K, k, 3)             # pieces[i][top_f[i, j]]
        Bm = ops.index_points(pieces, top_m)                                                 # pieces[j][top_m[j]]
        Bm = se3.transform_points(T.reshape(K * K, 4, 4), Bm.unsqueeze(0).expand(K, -1, -1, -1).reshape(K * K, k, 3))
        d1, d2 = ops.chamfer(Bf, Bm)
        score = (d1.mean(dim=1) + d2.mean(dim=1)).view(K, K)
        score = score.masked_fill(torch.eye(K, dtype=torch.bool, device=dev), float("inf"))
    return PairTable(twist, T, de_fpcb, de_mrpcb.permute(0, 2, 1), top_f, top_m, score, plan[1][0])


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


def apply(pieces, G):
    """The pieces [K,N,3] (on the GPU) in the root's frame: G[k] applied to piece k."""
    if not isinstance(pieces, torch.Tensor) or not pieces.is_cuda:
        raise _lib.PznError("apply: pieces must be a tensor on the GPU; puzzlenet_amd has no CPU fallback")
    g = torch.as_tensor(np.asarray(G) if not isinstance(G, torch.Tensor) else G).to(pieces.device, torch.float32)
    return se3.transform_points(g.contiguous(), pieces.contiguous())
