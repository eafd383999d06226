"""Drop-in for the live path of the reference's ``model5_b`` (the model used in the
paper, model5_b.py): ``layerAttention``, ``PCTransformer_nonsort``,
``TouchedRegraster`` with ``predict5`` / ``training_step`` / ``chamfer_loss`` /
``comp`` / ``configure_optimizers`` — same class, attribute and parameter names,
so a reference ``state_dict`` loads unchanged (8,059,220 parameters).

What is different from the reference file
  * every hard-wired 1024 (BatchNorm1d(num_points), repeat(1,1024,1),
    zeros(B,1024)) follows ``num_points`` (``config.num_points``, default 1024);
  * the point ops, EMD, chamfer, shared-MLP and attention run as hand-written
    gfx950 kernels behind the C ABI (puzzlenet_amd.ops);
  * TensorBoard meshes / matplotlib figures of the reference's training_step
    (model5_b.py:975-982, 1130-1134) are host-side logging and are not produced;
  * dead code of the reference (Encoder, decoders other than BiDecoderNoneCross,
    predict2/3/4/6) is not restated; ``fpc_decoder`` / ``rpc_decoder`` exist because
    their parameters are part of the reference's state_dict.
Reference quirks that ARE reproduced: the model5_b.py:741 copy-paste (the fpc global
feature is the max of the *mrpc* local feature) and the ``x2[:, idx[:, 0]]`` indexing
at :940/:942 that yields a [B,B,3] tensor.
"""
import datetime
import math
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib, metrics, ops, se3
from . import pointnet_util as pu
from .PyTorchEMD.emd import earth_mover_distance

try:  # the reference subclasses pl.LightningModule; keep that when Lightning is installed
    import pytorch_lightning as pl
    _Base = pl.LightningModule
except ImportError:  # pragma: no cover - image without Lightning
    class _Base(nn.Module):
        current_epoch = 0
        global_step = 0
        logger = None

        def save_hyperparameters(self, *a, **k):
            pass

        def log(self, *a, **k):
            pass


def scaled_dot_production(q, k, v, mask=None):
    """model5_b.py:67-75 -> (values, attention)."""
    if mask is not None:
        raise NotImplementedError("mask is never passed on the live path (model5_b.py:96)")
    return ops.attention(q, k, v)


class layerAttention(nn.Module):
    """model5_b.py:83-101: offset-attention block, r = x + relu(W_o (x - attn(x)))."""

    def __init__(self, config, embed_dim):
        super().__init__()
        self.C = config
        self.mlpq = nn.Linear(embed_dim, embed_dim // 4)
        self.mlpk = nn.Linear(embed_dim, embed_dim // 4)
        self.mlpv = nn.Linear(embed_dim, embed_dim)
        self.out = nn.Linear(embed_dim, embed_dim)

    def forward(self, xyz):
        if ops.attention_block_supported(xyz, self.mlpq.weight.shape[0]):
            # the whole block behind one entry point each way: x - a and x + relu(.) ride in GEMM epilogues, the five
            # gradient contributions to x are summed by accumulate epilogues (csrc/gemm.hip pzn_attn_block_*)
            try:
                return ops.attention_block(xyz, self.mlpq.weight, self.mlpq.bias, self.mlpk.weight, self.mlpk.bias,
                                           self.mlpv.weight, self.mlpv.bias, self.out.weight, self.out.bias)
            except _lib.PznUnsupported:      # a shape / alignment the fused block does not take: compose it below
                pass
        q = ops.linear(xyz, self.mlpq.weight, self.mlpq.bias)
        k = ops.linear(xyz, self.mlpk.weight, self.mlpk.bias)
        v = ops.linear(xyz, self.mlpv.weight, self.mlpv.bias)
        r, attention = scaled_dot_production(q, k, v)
        r = xyz - r
        r = xyz + ops.linear(r, self.out.weight, self.out.bias, relu=True)
        return r, attention


class BiDecoderNoneCross(nn.Module):
    """model5_b.py:325-352.  Instantiated by the reference (:537-538), never called by
    predict5; kept for state_dict / parameter-count parity."""

    def __init__(self, config, num_points=1024):
        super().__init__()
        self.C = config
        self.mlp1 = nn.Linear(512, 512)
        self.mlp2 = nn.Linear(512, 256)
        self.mlp3 = nn.Linear(256, 2)

    def forward(self, f_local, f_global):
        f_global = f_global.unsqueeze(1) if len(f_global.shape) == 2 else f_global
        f = f_global.repeat(1, 256, 1)
        f = torch.cat([f_local, f], dim=1).permute(0, 2, 1)
        f = ops.linear(f, self.mlp1.weight, self.mlp1.bias, relu=True)
        f = ops.linear(f, self.mlp2.weight, self.mlp2.bias, relu=True)
        f = ops.linear(f, self.mlp3.weight, self.mlp3.bias)
        return f.permute(0, 2, 1)


class PCTransformer_nonsort(nn.Module):
    """model5_b.py:411-478: per-cloud encoder."""

    def __init__(self, config, num_points=1024):
        super().__init__()
        self.C = config
        feature_size = 64
        gs2_feature_size = 128
        self.mlp1 = nn.Linear(3, 64)
        self.mlp2 = nn.Linear(64, feature_size)
        self.mlp3 = nn.Linear(feature_size + 3, 128)
        self.mlp4 = nn.Linear(128, gs2_feature_size)
        self.mlp5 = nn.Linear(gs2_feature_size + 3, gs2_feature_size * 2)
        self.mlp6 = nn.Linear(gs2_feature_size * 2, gs2_feature_size * 2)
        self.bn1 = nn.BatchNorm1d(num_points)   # the channel axis of a [B,N,64] tensor is N (:424,:447)
        self.bn2 = nn.BatchNorm1d(num_points)
        self.sg1 = pu.sample_and_group
        self.fps = pu.farthest_point_sample
        self.sg2 = pu.sample_and_group
        self.atten1 = layerAttention(self.C, gs2_feature_size * 2)
        self.atten2 = layerAttention(self.C, gs2_feature_size * 2)
        self.atten3 = layerAttention(self.C, gs2_feature_size * 2)
        self.atten4 = layerAttention(self.C, gs2_feature_size * 2)
        self.out = nn.Linear(gs2_feature_size * 2 * 5, 1024)

    # (centroids, neighbours) of the two set-abstraction levels (:449, :456): the one statement of these sizes, read by the
    # sampling plan below, by its start-index draws and by assembly.py
    SA_LEVELS = ((512, 32), (256, 32))
    fused_sa = True     # False: literally sample_and_group -> [B,S,K,3+D] -> shared MLP, as the reference composes it
    grad_marker = None       # engine.TrainStep (N > 1): marker(tensor) registers "the backward has come this far" on it

    def _mark_f2f(self, f2f):
        """The input of the attention chain: when its gradient exists, the chain's and the out projection's backward of
        this encoder has been enqueued (data dependency)."""
        if self.grad_marker is not None and f2f.requires_grad:
            self.grad_marker(f2f)
        return f2f

    def _set_abstraction(self, xyz, feat, lin_a, lin_b, plan):
        """sample_and_group(npoint, 0, nsample, xyz, feat, knn=True) + relu(lin_a) + relu(lin_b) + max over K on one level
        of a sampling plan: plan = (new_xyz, idx), idx None = the search (:118-119) fused into the group launch."""
        new_xyz, idx = plan
        return new_xyz, ops.sa_mlp_max(xyz, feat, new_xyz, idx, lin_a.weight, lin_a.bias, lin_b.weight, lin_b.bias)

    def local_features(self, xyz):
        """:447-448, the per-point MLP in front of the set abstraction (does not need the sampling plan)."""
        if _STEM_FUSED and ops.stem_supported(xyz, self.mlp1, self.bn1, self.mlp2, self.bn2):
            # both lines in one launch each way (csrc/stem.hip).  The features have two consumers (the first set-abstraction
            # level here, the boundary branch of the heads through slot 4 of the encoder's tuple): each gets its own name
            # for them and the stem's backward adds their gradients while it loads them
            if not _STEM_TWO:
                return ops.stem(xyz, self.mlp1, self.bn1, self.mlp2, self.bn2)
            # -> (name for the set-abstraction level, name for the boundary branch): stem() below hands each on
            return ops.stem(xyz, self.mlp1, self.bn1, self.mlp2, self.bn2, two=True)
        # BatchNorm + ReLU as one launch each way (csrc/bnpoints.hip); ops.* raise on CPU tensors: there is no eager path
        x_feature = ops.bn_points_relu(ops.linear(xyz, self.mlp1.weight, self.mlp1.bias), self.bn1)   # :447
        return ops.bn_points_relu(ops.linear(x_feature, self.mlp2.weight, self.mlp2.bias), self.bn2)  # :448

    def _block_params(self):
        return [(a.mlpq.weight, a.mlpq.bias, a.mlpk.weight, a.mlpk.bias, a.mlpv.weight, a.mlpv.bias, a.out.weight, a.out.bias)
                for a in (self.atten1, self.atten2, self.atten3, self.atten4)]

    def stem(self, xyz, sa_plan=None, x_feature=None):
        """:447-461: per-point MLP and the two set-abstraction levels -> (x2, f2f, x_feature).  x_feature may be the pair of
        names local_features() returns for the fused stem: the first feeds the set abstraction, the second is what comes back
        (slot 4 of the encoder's tuple, the boundary branch's input)."""
        if x_feature is None:
            x_feature = self.local_features(xyz)
        second = x_feature
        if isinstance(x_feature, tuple):
            x_feature, second = x_feature
        if self.fused_sa and not xyz.requires_grad:
            if sa_plan is None:      # the encoder on its own: its two draws from the global generator (pointnet_util.py:65)
                sa_plan = sampling_plan(xyz, *upload_starts(draw_fps_starts(1, xyz.shape[0], xyz.shape[1]), xyz.device), False)
            x, f1f = self._set_abstraction(xyz, x_feature, self.mlp3, self.mlp4, sa_plan[0])
            x2, f2f = self._set_abstraction(x, f1f, self.mlp5, self.mlp6, sa_plan[1])
        else:
            (n1, k1), (n2, k2) = self.SA_LEVELS
            x, f1 = self.sg1(n1, 0, k1, xyz, x_feature, False, True)                              # :449
            f1f = ops.shared_mlp_max(f1, self.mlp3.weight, self.mlp3.bias, self.mlp4.weight, self.mlp4.bias)  # :452-454
            x2, f2 = self.sg2(n2, 0, k2, x, f1f, False, True)                                     # :456
            f2f = ops.shared_mlp_max(f2, self.mlp5.weight, self.mlp5.bias, self.mlp6.weight, self.mlp6.bias)  # :459-461
        return x2, self._mark_f2f(f2f), second

    def chain_fused_ok(self, f2f):
        return ops.attention_chain_fused_supported(f2f, self.atten1.mlpq.weight.shape[0], self.out.weight)

    def forward(self, xyz, sa_plan=None, x_feature=None, need_out=True, attn_strips=False):
        """-> (f_global, x2, attention, out, x_feature).  need_out = False: slot 3 (the [B,256,1024] projection) is None where
        the fused chain runs.  attn_strips = True: slot 2 is [B,16,256] strip column sums with the same mean over dim 1
        there (ops.attention_chain_fused)."""
        return self.tail(*self.stem(xyz, sa_plan, x_feature), need_out, attn_strips)

    def tail(self, x2, f2f, x_feature, need_out=True, attn_strips=False):
        """:462-475 behind stem(): the four attention blocks, the out projection, the max over the points."""
        if self.chain_fused_ok(f2f):
            # :462-475 through the chained matrix-core kernels (csrc/attnfused.hip), one encoder per launch here
            # need_out = False (passed by predict5, which uses only the maximum: :723): `out` is None, never written
            (out, attention, f_global), = ops.attention_chain_fused([f2f], [self._block_params()], [self.out.weight], [self.out.bias],
                                                                   need_out=need_out, map_strips=attn_strips)
            return f_global, x2, attention, out, x_feature
        # any other shape: the four blocks as modules, as the reference composes them
        att1, attention1 = self.atten1(f2f)
        att2, attention2 = self.atten2(att1)
        att3, attention3 = self.atten3(att2)
        att4, attention4 = self.atten4(att3)
        attention = ops.avg4(attention1, attention2, attention3, attention4)     # :468-469, one launch
        att = torch.cat([att1, att2, att3, att4, f2f], dim=-1)       # (:466, :470 as one copy instead of two)
        out = ops.linear(att, self.out.weight, self.out.bias)                                   # :474
        f_global = ops.max_over_points(out)                                                       # :475
        return f_global, x2, attention, out, x_feature


def draw_fps_starts(clouds, rows, n_points, generator=None):
    """The host draws of the FPS start indices for `clouds` clouds of `rows` samples with n_points points each -> 2 * clouds
    int64 CPU tensors [rows]: per cloud, in order, the level-1 starts in [0, n_points) and then the level-2 starts in
    [0, SA_LEVELS[0][0]) - the reference's order (sg1, sg2 of one encoder, then the next; pointnet_util.py:65).  The order of
    these calls is what a seed means.  generator None = torch's global one, as the reference."""
    n1 = PCTransformer_nonsort.SA_LEVELS[0][0]
    return [torch.randint(0, n_, (rows,), dtype=torch.long, generator=generator) for _ in range(clouds) for n_ in (n_points, n1)]


def upload_starts(draws, dev):
    """Host index vectors of one length -> their device copies, through ONE asynchronous upload from pinned memory: a
    pageable `.to(dev)` blocks the host until everything queued before it has run (4 of them per step drained the launch
    queue at every step start)."""
    stage = torch.empty((len(draws), draws[0].shape[0]), dtype=torch.long, pin_memory=True)
    torch.stack(tuple(draws), out=stage)
    return stage.to(dev, non_blocking=True).unbind(0)


def sampling_plan(xyz, s1, s2, with_knn):
    """FPS -> gather of both set-abstraction levels from the start indices s1, s2 (on the device) and, with_knn, the two
    neighbour searches -> ((x1, idx1 | None), (x2, idx2 | None)).  Coordinates only: no weight is read.  idx None = the
    search runs inside the encoder, fused with the group write."""
    (n1, k1), (n2, k2) = PCTransformer_nonsort.SA_LEVELS
    x1 = ops.index_points(xyz, ops.farthest_point_sample(xyz, n1, s1))
    x2 = ops.index_points(x1, ops.farthest_point_sample(x1, n2, s2))
    if with_knn:
        return (x1, ops.knn(xyz, x1, k1)), (x2, ops.knn(x1, x2, k2))
    return (x1, None), (x2, None)


def pick_order_plan(xyz):
    """sampling_plan(with_knn=True) of clouds that are in FPS pick order already (ops.merge_resample's output): the first n1
    points are the level-1 sample started at point 0, the first n2 of those the level-2 sample of that - no FPS."""
    (n1, k1), (n2, k2) = PCTransformer_nonsort.SA_LEVELS
    x1 = xyz[:, :n1].contiguous()
    x2 = xyz[:, :n2].contiguous()
    return (x1, ops.knn(xyz, x1, k1)), (x2, ops.knn(x1, x2, k2))


# training_step takes nothing but the row mean of the two attention maps (model5_b.py:937-942): on the fused attention path it
# asks for them as [B,16,256] strip column sums with that same row mean (tests compare both forms through this flag)
_ATTN_STRIPS = True
# the per-point stem (:447-448) as one launch each way (csrc/stem.hip, ops.stem) where its shape is supported (B <= 64); False =
# always the four launches (2 linear + 2 BatchNorm) it replaces, which larger batches use (tests compare the two through this flag)
_STEM_FUSED = True
_ROWS_CHAIN = True   # the pose head (:723-725) as the few-row chain of csrc/fewrows.hip; False = cat + one ops.linear per layer (tests compare the two)
_STEM_TWO = True     # the stem's output under two names (set abstraction / boundary branch): their gradients are added inside its backward launch


def _seq(*dims):
    layers = []
    for i in range(len(dims) - 1):
        layers.append(nn.Linear(dims[i], dims[i + 1]))
        if i < len(dims) - 2:
            layers.append(nn.ReLU())
    return nn.Sequential(*layers)


def _chain3(mods, x, cin):
    """(Linear, ReLU, Linear, ReLU, Linear) on [B, N, 64] rows that csrc/pointmlp.hip runs as one launch each way
    (the boundary heads' chains: 64 -> 64 -> 64 -> 64 and (64 |) 64 -> 64 -> 32 -> 2); None otherwise."""
    if not (len(mods) == 5 and isinstance(mods[1], nn.ReLU) and isinstance(mods[3], nn.ReLU)
            and all(isinstance(mods[i], nn.Linear) and mods[i].bias is not None for i in (0, 2, 4))
            and x.dim() == 3 and x.dtype == torch.float32 and x.shape[1] % 32 == 0):
        return None
    l1, l2, l3 = mods[0], mods[2], mods[4]
    if l1.in_features != cin or l2.in_features != l1.out_features or l3.in_features != l2.out_features:
        return None
    return (l1, l2, l3) if ops.point_mlp3_available(x.shape[2], l1.out_features, l2.out_features, l3.out_features) else None


def run_seq(seq, x):
    """nn.Sequential(Linear, ReLU, Linear, ...) (or a list of its modules) through the fused kernels: one launch for a
    three-layer chain on [B, N, 64] rows (_chain3), the linear(+ReLU) kernel per layer otherwise."""
    mods = list(seq)
    ch = _chain3(mods, x, x.shape[-1])
    if ch is not None:
        l1, l2, l3 = ch
        return ops.point_mlp3(x, l1.weight, l1.bias, l2.weight, l2.bias, l3.weight, l3.bias)
    i = 0
    while i < len(mods):
        lin = mods[i]
        relu = i + 1 < len(mods) and isinstance(mods[i + 1], nn.ReLU)
        x = ops.linear(x, lin.weight, lin.bias, relu=relu)
        i += 2 if relu else 1
    return x


def run_seq_parts(seq, parts):
    """run_seq on cat(parts, -1) for [M, k] row tensors: a Linear / ReLU stack on few rows runs as one chain of launches each
    way with every part read where it lies (ops.mlp_rows, csrc/fewrows.hip); the concatenation and run_seq otherwise."""
    mods = list(seq)
    lins = [m for m in mods if isinstance(m, nn.Linear)]
    if _ROWS_CHAIN and lins and isinstance(mods[0], nn.Linear) and all(isinstance(m, (nn.Linear, nn.ReLU)) for m in mods):
        relus = [i + 1 < len(mods) and isinstance(mods[i + 1], nn.ReLU) for i, m in enumerate(mods) if isinstance(m, nn.Linear)]
        plain = len(lins) + sum(relus) == len(mods)              # (no ReLU behind a ReLU)
        if plain and all(p.dim() == 2 for p in parts) and ops.mlp_rows_supported(parts, [m.weight for m in lins], [m.bias for m in lins]):
            return ops.mlp_rows(parts, [m.weight for m in lins], [m.bias for m in lins], relus)
    return run_seq(seq, parts[0] if len(parts) == 1 else torch.cat(list(parts), dim=-1))


def run_seq_cat_global(seq, x, g):
    """run_seq on cat([g.repeat(1, N, 1), x], -1) with the first Linear + ReLU split into a per-point and a per-cloud part."""
    mods = list(seq)
    if not (len(mods) >= 2 and isinstance(mods[1], nn.ReLU)):
        return run_seq(seq, torch.cat([g.expand(-1, x.shape[1], -1), x], dim=-1))
    ch = _chain3(mods, x, g.shape[-1] + x.shape[-1])
    if ch is not None:
        l1, l2, l3 = ch
        return ops.point_mlp3(x, l1.weight, l1.bias, l2.weight, l2.bias, l3.weight, l3.bias, g=g)
    y = ops.cat_global_linear_relu(x, g, mods[0].weight, mods[0].bias)
    return run_seq(mods[2:], y)


class TouchedRegraster(_Base):
    """model5_b.py:519-1519 (live path only)."""

    def __init__(self, config):
        super().__init__()
        self.save_hyperparameters()
        self.C = config
        self.num_points = int(getattr(config, "num_points", 1024))
        self.Encoder = PCTransformer_nonsort(config, self.num_points)
        self.Encoder2 = PCTransformer_nonsort(config, self.num_points)
        self.fpc_decoder = BiDecoderNoneCross(config)
        self.rpc_decoder = BiDecoderNoneCross(config)
        delta = 1.0e-2
        self.dt = nn.Parameter(torch.full((1, 6), delta), requires_grad=True)      # :541-543
        self.tfMLP = _seq(2048, 1024, 512, 512, 256, 6)                            # :559-569
        self.MLPLocalPreRpc = _seq(64, 64, 64, 64)                                 # :571-577
        self.MLPLocalPreFpc = _seq(64, 64, 64, 64)
        self.MLPRpcb = _seq(128, 64, 32, 2)                                        # :586-592
        self.MLPFpcb = _seq(128, 64, 32, 2)
        self.two_streams = True        # Encoder2 on a side stream; False = everything on the current stream
        self._side_stream = None
        self._plan_stream = None
        self._plan_cache = None        # (fpc, mrpc, plans, event, versions) from prefetch_plans, handed over by use_plans
        self.grad_marker = None        # engine.TrainStep (N > 1), see _heads
        self.fps_generator = None      # CPU generator of the FPS start indices (None = torch's global one, as the reference)
        self.defer_emd_loss = False    # see training_step: the EMD term as a separate backward root (engine.TrainStep)

    # ------------------------------------------------------------------ forward
    def predict5(self, batch, batch_indic, need=False, training=False, pose_hook=None, attn_strips=False):
        """model5_b.py:672-759.  pose_hook(out): called as soon as the pose head has produced `out`, before the boundary
        heads are enqueued (training_step starts the N x N EMD on the side stream from it).  attn_strips (training_step
        only, which takes nothing but the row mean of the two attention maps): on the fused attention path the maps come back
        as [B,16,256] strip column sums with that same row mean (ops.attention_chain_fused); every other path and every other
        caller gets the reference's [B,256,256] maps."""
        self.set_mode(training)
        fpc, mrpc = batch[0], batch[1]
        if len(fpc.shape) == 2:
            fpc = fpc.unsqueeze(0)
            mrpc = mrpc.unsqueeze(0)
        attn_strips = bool(attn_strips)
        # the encoders' [B,256,1024] projection itself (5-tuple slot 3) is not used by predict5, only its max over the
        # points (:723): every encoder call below passes need_out = False (the encoder called on its own still returns it)
        if self.two_streams:
            # FPS is a latency-bound chain on 128 workgroups: it runs on the side stream while this one computes the
            # per-point features of both clouds, which do not depend on it; then Encoder stays here, Encoder2 goes
            # to the side stream (the two are independent and most of their launches do not fill 256 CUs; autograd
            # replays each backward node on its forward stream, so the backward passes overlap as well).
            cur = torch.cuda.current_stream()
            side = self.side_stream()
            side.wait_stream(cur)
            taken = self._take_plans(fpc, mrpc, (cur, side))
            if taken is not None:          # sampling + searches were done ahead (prefetch_plans): both encoders start at once
                plan_f, plan_m = taken
                with torch.cuda.stream(side):
                    xf_m = self.Encoder2.local_features(mrpc)
                xf_f = self.Encoder.local_features(fpc)
            else:
                with torch.cuda.stream(side):
                    plan_f, plan_m = self._sa_plans(fpc, mrpc)
                xf_f = self.Encoder.local_features(fpc)
                xf_m = self.Encoder2.local_features(mrpc)
                cur.wait_stream(side)          # plans -> this stream
                side.wait_stream(cur)          # xf_m -> side stream
            if plan_f is not None:
                for lvl in plan_f:
                    lvl[0].record_stream(cur)
            for t_ in (xf_m if isinstance(xf_m, tuple) else (xf_m,)):
                t_.record_stream(side)
            if plan_f is None:
                # no hoisted sampling (fused_sa off, or clouds that carry gradients): each sample_and_group draws its own FPS
                # start indices, so the encoders are CALLED in the reference's order (:710 before :716) - the draws of a
                # seeded run are the reference's; the streams are the same either way
                ffpcs = self.Encoder(fpc, plan_f, xf_f, False, attn_strips)                         # :710
                with torch.cuda.stream(side):
                    fmrpcs = self.Encoder2(mrpc, plan_m, xf_m, False, attn_strips)                  # :716
            else:
                with torch.cuda.stream(side):
                    fmrpcs = self.Encoder2(mrpc, plan_m, xf_m, False, attn_strips)                  # :716
                ffpcs = self.Encoder(fpc, plan_f, xf_f, False, attn_strips)                         # :710
            # Encoder2's outputs are joined inside _heads: the second cloud's boundary head stays on the side stream
            return self._heads(ffpcs, fmrpcs, need, pose_hook, side)
        plan_f, plan_m = self._sa_plans(fpc, mrpc)
        ffpcs = self.Encoder(fpc, plan_f, None, False, attn_strips)                 # :710
        fmrpcs = self.Encoder2(mrpc, plan_m, None, False, attn_strips)              # :716
        return self._heads(ffpcs, fmrpcs, need, pose_hook)

    def set_mode(self, training):
        """:677-690: the five sub-modules predict5 moves to train or eval mode."""
        training = bool(training)
        for m in (self.Encoder, self.Encoder2, self.tfMLP, self.fpc_decoder, self.rpc_decoder):
            # (Module.train() re-assigns the flag of every submodule through Module.__setattr__: 0.3 ms of host time
            # per predict5 call when nothing changes; reading the flags is a tenth of that and leaves the behaviour as it is)
            if any(sm.training != training for sm in m.modules()):
                m.train(training)

    def side_stream(self):
        """The stream Encoder2 (and the N x N EMD) runs on, created on first use."""
        if self._side_stream is None:
            self._side_stream = torch.cuda.Stream()
            _quiet = getattr(torch.autograd.graph, "set_warn_on_accumulate_grad_stream_mismatch", None)
            if _quiet is not None:
                _quiet(False)
        return self._side_stream

    def pose_head(self, ffpc, fmrpc):
        """:723-725: tfMLP on the two global features side by side -> the twist [B,6]."""
        return run_seq_parts(self.tfMLP, (ffpc, fmrpc))

    def moved_branch(self, feat, ready=None, stream=None):
        """:739, :741, :749, :753-754: the moved cloud's per-point features [B,N,64] -> (local [B,N,64], g_max [B,1,64], logits
        [B,N,2]).  :741 - the reference takes the max over the MOVED cloud's local features for BOTH globals (its bug, kept):
        one reduction serves this branch and fixed_branch.  ready: an event recorded on `stream` (the one this runs on) once
        g_max is enqueued, for a consumer on another stream that needs no logits.
        :745-754 run without the repeat and the concatenation: the first layer of a head = a per-point product on the local
        features + a per-cloud bias from the global one (run_seq_cat_global)."""
        local = run_seq(self.MLPLocalPreRpc, feat)                                  # :739
        g_max = ops.max_over_points(local).unsqueeze(1)                             # :741
        if ready is not None:
            ready.record(stream)
        return local, g_max, run_seq_cat_global(self.MLPRpcb, local, g_max)         # :749, :753-754

    def fixed_branch(self, feat, g_max):
        """:738, :748, :751-752: the fixed cloud's per-point features [B,N,64] and moved_branch's g_max -> logits [B,N,2]."""
        return run_seq_cat_global(self.MLPFpcb, run_seq(self.MLPLocalPreFpc, feat), g_max)

    def _heads(self, ffpcs, fmrpcs, need, pose_hook=None, side=None):
        """:723-759: pose head on the two global features, boundary heads on the per-point features.
        side: the stream Encoder2 ran on (fmrpcs not yet joined).  The boundary head of the second cloud then stays on
        that stream - its inputs were produced there - beside the pose head and the first cloud's boundary head on this
        one: two chains of 131 072-row layers (25 us launches at a third of the HBM rate each) instead of one, forward and,
        since autograd replays a node on its forward stream, backward.  side None: the same launches in the same order on
        the current stream, no events."""
        ffpc, non_sg_ffpc = ffpcs[0], ffpcs[4]
        fmrpc, non_sg_fmrpc = fmrpcs[0], fmrpcs[4]
        if self.grad_marker is not None:
            # The boundary branch hangs off the encoders' per-point features, NOT off the attention chains: its backward
            # is no ancestor of the chains' input gradient.  An alias of each input carries its own marker: that alias's
            # gradient exists exactly when MLPLocalPre* / MLP*b of that cloud have been through their backward.
            if non_sg_ffpc.requires_grad:
                non_sg_ffpc = self.grad_marker(non_sg_ffpc.view_as(non_sg_ffpc))
            if non_sg_fmrpc.requires_grad:
                non_sg_fmrpc = self.grad_marker(non_sg_fmrpc.view_as(non_sg_fmrpc))
        if side is None:
            _, g_max, de_mrpcb = self.moved_branch(non_sg_fmrpc)
        else:
            cur = torch.cuda.current_stream()
            ready = torch.cuda.Event()
            with torch.cuda.stream(side):
                _, g_max, de_mrpcb = self.moved_branch(non_sg_fmrpc, ready, side)
            cur.wait_event(ready)                                                       # Encoder2's outputs and g_max
            for t in list(fmrpcs) + [g_max]:
                if isinstance(t, torch.Tensor):
                    t.record_stream(cur)
        out = self.pose_head(ffpc, fmrpc)
        if pose_hook is not None:
            pose_hook(out)
        de_fpcb = self.fixed_branch(non_sg_ffpc, g_max).permute(0, 2, 1)
        de_mrpcb = de_mrpcb.permute(0, 2, 1)
        if side is not None:
            cur.wait_stream(side)
            de_mrpcb.record_stream(cur)
        if not need:
            return out, out, de_fpcb, de_mrpcb
        return out, [0], ffpcs[1], ffpcs[2], fmrpcs[1], fmrpcs[2], de_fpcb, de_mrpcb

    def forward(self, batch, bat=None):
        return self.predict5(batch, bat)

    def prefetch_plans(self, fpc, mrpc):
        """The coordinate-only part of a LATER predict5(fpc, mrpc) call — the FPS chain, the centroid gathers and the two
        neighbour searches of both clouds, none of which depends on a weight — enqueued now on a background stream, so
        that it runs beside whatever the other streams are doing (engine.TrainStep calls it at the start of a step for
        the next step's batch: FPS is 0.5 ms of latency-bound launches on 128 workgroups that otherwise stand at the head
        of every step).  The start indices are drawn here, in the reference's order.  Returns the plan for use_plans();
        predict5 picks it up when it is called with the same two tensors and computes it in place otherwise."""
        if len(fpc.shape) == 2 or not self.two_streams:
            return None
        if self._plan_stream is None:
            self._plan_stream = torch.cuda.Stream()
        ps = self._plan_stream
        ps.wait_stream(torch.cuda.current_stream())       # the clouds exist
        with torch.cuda.stream(ps):
            plans = self._sa_plans(fpc, mrpc, with_knn=True)
            ready = torch.cuda.Event()
            ready.record(ps)
        # the plan belongs to these tensors AS THEY ARE NOW: an in-place refresh of a persistent batch buffer
        # (batch[0].copy_(...)) bumps the version counter and the plan is not taken (predict5 then computes its own)
        stamp = (fpc._version, mrpc._version, fpc.data_ptr(), mrpc.data_ptr())
        return (fpc, mrpc, plans, ready, stamp) if plans[0] is not None else None

    def use_plans(self, prefetched):
        """Hand a prefetch_plans() result to the next predict5 call (None: nothing prefetched)."""
        self._plan_cache = prefetched

    def _take_plans(self, fpc, mrpc, streams):
        """The prefetched plan of exactly these tensors (once), made visible to `streams`; None if there is none."""
        cached, self._plan_cache = self._plan_cache, None
        if cached is None or cached[0] is not fpc or cached[1] is not mrpc:
            return None
        if cached[4] != (fpc._version, mrpc._version, fpc.data_ptr(), mrpc.data_ptr()):
            return None                # same tensor objects, other contents: the prefetched samples are stale
        plans, ready = cached[2], cached[3]
        for st in streams:
            st.wait_event(ready)
            for plan in plans:
                for new_xyz, idx in plan:
                    new_xyz.record_stream(st)
                    if idx is not None:
                        idx.record_stream(st)
        return plans

    def _sa_plans(self, fpc, mrpc, with_knn=False):
        """FPS -> gather of BOTH set-abstraction levels for BOTH clouds, hoisted in front of the
        encoders: the sampling chain depends on coordinates only, so the two encoders' 64-workgroup,
        latency-bound FPS launches become one 128-workgroup launch per level (same wall time each).  The four start-index draws are made first, in the
        reference's order (Encoder sg1, sg2, Encoder2 sg1, sg2; pointnet_util.py:65), so a seeded run
        picks exactly the points the reference picks."""
        if not (self.Encoder.fused_sa and self.Encoder2.fused_sa) or fpc.requires_grad or mrpc.requires_grad \
                or fpc.shape != mrpc.shape:
            return None, None
        B, N, _ = fpc.shape
        # fps_generator (a CPU torch.Generator, default None = the global one the reference draws from): with the plan
        # prefetch the draws of step k+1 are made before step k runs, which shifts the global stream for any other
        # consumer between steps (a loader's augmentation); a private generator leaves the global one alone
        d1, d2, d3, d4 = upload_starts(draw_fps_starts(2, B, N, getattr(self, 'fps_generator', None)), fpc.device)
        # with_knn (prefetch_plans): the searches too; otherwise each runs inside its encoder, fused with the group write
        plan = sampling_plan(torch.cat([fpc, mrpc], dim=0), torch.cat([d1, d3]), torch.cat([d2, d4]), with_knn)
        return (tuple((x[:B], i if i is None else i[:B]) for x, i in plan),
                tuple((x[B:], i if i is None else i[B:]) for x, i in plan))

    # ------------------------------------------------------------------ losses
    def chamfer_loss(self, a, b):
        """model5_b.py:1495-1505 -> (min over a per b-point [B,m], min over b per a-point [B,n])."""
        return ops.chamfer(a, b)

    def comp(self, g, igt):
        """model5_b.py:1512-1519: |g igt - I|^2 mean * 16."""
        assert g.size(0) == igt.size(0)
        assert g.size(1) == igt.size(1) and g.size(1) == 4
        assert g.size(2) == igt.size(2) and g.size(2) == 4
        if g.is_cuda and g.dtype == torch.float32:
            return ops.comp_loss(g, igt.to(g))        # one launch each way (csrc/losstail.hip)
        A = g.matmul(igt)
        I = torch.eye(4, dtype=A.dtype, device=A.device).view(1, 4, 4).repeat(A.size(0), 1, 1)
        return F.mse_loss(A, I, reduction='mean') * 16

    def training_step(self, batch, batch_indic):
        """model5_b.py:912-1155 (non-pretrain branch), every loss term; logging calls kept as self.log."""
        fpc, mrpc, igt, rpc, fpcb, rpcb = batch[0], batch[1], batch[2], batch[3], batch[4], batch[5]
        batch_size = fpc.shape[0]
        fpc_idx, rpc_idx = batch[6], batch[7]
        N = fpc.shape[1]
        C = self.C

        # The N x N EMD (:1002) is ~1.7 ms of vector-ALU work that needs nothing but the pose, and nothing needs its
        # value until the loss terms are summed: on the GPU it is started on the side stream as soon as the pose head
        # is done (pose_hook), and the boundary heads, their losses and the other small launches run beside it.
        pose = {}

        def fork_emd(o):
            if self.two_streams and self._side_stream is not None:
                cur = torch.cuda.current_stream()
                side = self._side_stream
                side.wait_stream(cur)
                with torch.cuda.stream(side):
                    pose['emd'] = earth_mover_distance(pose['de_mrpc'], rpc, transpose=False)
                pose['de_mrpc'].record_stream(side)
                rpc.record_stream(side)
                pose['side'] = side

        def pose_hook(o):
            pose['mat'] = se3.exp(o).to(mrpc)                                       # :947
            pose['de_mrpc'] = se3.transform_points(pose['mat'], mrpc)               # :948-952 (transform of the transposed view)

        out, t, x2, attention, mrpc_x2, mrpc_attention, de_fpcb, de_mrpcb = self.predict5(
            batch, batch_size, training=True, need=True, pose_hook=pose_hook, attn_strips=_ATTN_STRIPS)      # :933
        fork_emd(out)      # forked after the heads were enqueued (right after the pose head measured slower)

        # :937-942: only the FIRST of the 32 top-k indices is used: mean over rows + arg-max, one launch
        x2att1 = x2[:, ops.colmean_argmax(attention)[1]]
        x2att2 = mrpc_x2[:, ops.colmean_argmax(mrpc_attention)[1]]

        mat, de_mrpc = pose['mat'], pose['de_mrpc']                                 # :947-952 (computed in pose_hook)
        R = mat[:, :3, :3]
        t = mat[:, :3, 3]

        dg_mrpc_dist1, dg_mrpc_dist2 = self.chamfer_loss(rpc, de_mrpc)              # :956-960
        if C.loss_sum:
            loss_recoversy = torch.sum(dg_mrpc_dist1) + torch.sum(dg_mrpc_dist2)
        else:
            loss_recoversy = torch.mean(dg_mrpc_dist1) + torch.mean(dg_mrpc_dist2)

        # :963-967 rebuild g from R and t: mat already IS [[R, t], [0 0 0 1]] (se3.exp), so comp takes it as it stands
        loss_g = self.comp(mat, igt)
        self.log('train/loss_re', loss_recoversy)
        self.log('train/loss_g', loss_g)

        dg_att1_dist1, dg_att1_dist2 = self.chamfer_loss(x2att1, x2att2)            # :1001
        # :1002 — the N x N EMD: already running on the side stream (pose_hook), else here.  The terms are added in the
        # reference's order further down (:1016-1151), so the loss value is the one of the sequential code.
        emd_side = pose.get('side')
        emd = pose['emd'] if emd_side is not None else earth_mover_distance(de_mrpc, rpc, transpose=False)
        if C.loss_sum:
            loss_cd2 = torch.sum(dg_att1_dist1) + torch.sum(dg_att1_dist2)
        else:
            loss_cd2 = torch.mean(dg_att1_dist1) + torch.mean(dg_att1_dist2)
        self.log('train/cd2', loss_cd2)
        # :1012 emd2 = earth_mover_distance(x2att1, x2att2) is evaluated further down, in one launch with the two other small
        # terms (:1123-1125); nothing in between reads it

        # :1063-1064 cross entropy and :1085-1090 class-1 probability in one launch per head, :1089-1091 top-128 as
        # one radix-select launch per head (csrc/losstail.hip)
        loss_fpcb_cel, de_fpcb_idx_sig = ops.boundary_ce(de_fpcb, fpc_idx.reshape(batch_size, N))
        loss_rpcb_cel, de_mrpcb_idx_sig = ops.boundary_ce(de_mrpcb, rpc_idx.reshape(batch_size, N))
        de_fpcb_idx = ops.topk_rows(de_fpcb_idx_sig, 128)
        de_mrpcb_idx = ops.topk_rows(de_mrpcb_idx_sig, 128)
        self.log('train/loss_fpcb_cel', loss_fpcb_cel)
        self.log('train/loss_rpcb_cel', loss_rpcb_cel)

        with torch.no_grad():                                                       # :1094-1105 (IoU, logged only)
            # |pred AND gt| = the labels gathered at the 128 picks; |pred OR gt| = 128 per cloud + |gt| - |pred AND gt|
            def _iou(idx, gt):
                inter = torch.gather(gt, 1, idx).sum()
                return inter / (float(idx.numel()) + gt.sum() - inter)
            fpc_iou = _iou(de_fpcb_idx, fpc_idx)
            mrpcb_iou = _iou(de_mrpcb_idx, rpc_idx)
        self.log('train/fpc_iou', fpc_iou)
        self.log('train/mrpcb_iou', mrpcb_iou)

        de_fpcb_pts = ops.index_points(fpc, de_fpcb_idx)                            # :1109-1110
        de_mrpcb_pts = ops.index_points(mrpc, de_mrpcb_idx)

        cd_fpcb1, cd_fpcb2 = self.chamfer_loss(de_fpcb_pts, fpcb)                   # :1112-1113
        loss_fpcb = torch.mean(cd_fpcb1) + torch.mean(cd_fpcb2)
        self.log('train/loss_fpcb', loss_fpcb)
        inverse_de_mrpcb = se3.transform_points(se3.exp(out).to(mrpc), de_mrpcb_pts)      # :1116
        cd_mrpcb1, cd_mrpcb2 = self.chamfer_loss(inverse_de_mrpcb, rpcb)            # :1119-1120
        loss_mrpcb = torch.mean(cd_mrpcb1) + torch.mean(cd_mrpcb2)
        self.log('train/loss_rpcb', loss_mrpcb)

        small = [(x2att1, x2att2), (de_fpcb_pts, fpcb), (inverse_de_mrpcb, rpcb)]      # :1012, :1123, :1125
        if all(t.dtype == torch.float32 and t.dim() == 3 and t.shape[1] <= ops.EMD_SMALL_MAX for pr in small for t in pr):
            # the three single-workgroup auctions as ONE launch (3 B workgroups instead of B three times; csrc/emd.hip)
            emd2, e_fpcb, e_mrpcb = ops.emd_fused_small_multi(small)
        else:
            emd2, e_fpcb, e_mrpcb = (earth_mover_distance(a_, b_, transpose=False) for a_, b_ in small)
        emd2 = torch.sum(emd2)                                                      # :1033
        self.log('train_emd2', emd2)
        emd_fpcb = torch.mean(e_fpcb)                                               # :1123-1126
        emd_mrpcb = torch.mean(e_mrpcb)
        self.log('train/loss_emd_fpcb', emd_fpcb)
        self.log('train/loss_emc_mrpcb', emd_mrpcb)

        # defer_emd_loss (set by engine.TrainStep in eager mode): the EMD term stays a separate backward root, so that the
        # backward of everything that does not hang off the pose (boundary terms, heads) is not queued behind the
        # join with the side stream; the caller adds the two parts after the backward has been enqueued.
        uses_emd = C.loss_mode in (1, 2, 3, 4)
        defer = emd_side is not None and uses_emd and getattr(self, 'defer_emd_loss', False)
        if emd_side is not None and not defer:     # join: from here on the N x N cost is used on this stream
            torch.cuda.current_stream().wait_stream(emd_side)
            emd.record_stream(torch.cuda.current_stream())
        if defer:
            with torch.cuda.stream(emd_side):
                loss_emd = torch.sum(emd) if C.loss_sum else torch.mean(emd)        # :1003-1010
        else:
            loss_emd = torch.sum(emd) if C.loss_sum else torch.mean(emd)            # :1003-1010
        self.log('train/loss_emd', loss_emd)

        mode = C.loss_mode                                                          # :1016-1029
        if mode == 0:
            loss = loss_recoversy + loss_g
        elif mode == 1:
            loss = loss_recoversy + loss_g if defer else loss_recoversy + loss_g + loss_emd
        elif mode == 2:
            loss = None if defer else loss_emd
        elif mode == 3:
            loss = loss_g if defer else loss_emd + loss_g
        elif mode == 4:
            loss = loss_recoversy if defer else loss_emd + loss_recoversy
        elif mode == 5:
            loss = loss_g
        elif mode == 6:
            loss = loss_recoversy
        else:
            raise ValueError(f"loss_mode {mode}")
        if C.use_emd2:                                                              # :1033-1036
            loss = emd2 if loss is None else loss + emd2
        if C.use_cd2:
            loss = loss_cd2 if loss is None else loss + loss_cd2
        loss = loss_fpcb_cel + loss_rpcb_cel if loss is None else loss + loss_fpcb_cel + loss_rpcb_cel   # :1065
        loss = loss + loss_mrpcb + loss_fpcb                                        # :1146-1151
        if C.use_emd3:
            loss = loss + emd_fpcb + emd_mrpcb
        if defer:
            return {'loss_terms': (loss, loss_emd), 'join_stream': emd_side}
        self.log('train_loss', loss)
        return {'loss': loss}

    # ------------------------------------------------------------------ eval path
    def compute_metrics(self, R, t, igt):
        """model5_b.py:1426-1440: errors of the predicted (R, t) against the INVERSE of the ground-truth motion
        igt[B,4,4] -> (r_mse, r_mae, t_mse, t_mae, r_isotropic, t_isotropic), one value per sample."""
        inv_R, inv_t = metrics.inv_R_t(igt[:, :3, :3], igt[:, :3, 3])
        r_mse, r_mae = metrics.anisotropic_R_error(R, inv_R)
        t_mse, t_mae = metrics.anisotropic_t_error(t, inv_t)
        return r_mse, r_mae, t_mse, t_mae, metrics.isotropic_R_error(R, inv_R), metrics.isotropic_t_error(t, inv_t, inv_R)

    METRIC_NAMES = ('r_mse', 'r_mae', 't_mse', 't_mae', 'r_iso', 't_iso', 'fpc_iou', 'mrpc_iou', 'cd_fpcb', 'cd_rpcb')

    def test_step(self, batch, batch_id):
        """model5_b.py:1279-1366 -> [1, 10] scores (METRIC_NAMES): registration errors of the predicted pose,
        IoU of the 128 predicted boundary points of both pieces, chamfer distance of the predicted boundaries.
        Un-batched samples ([N,3] clouds, [N] labels) are given a batch axis as the reference does; the width of the
        boundary masks follows the clouds (the reference hard-wires 1024)."""
        nb = [b.unsqueeze(0) if b.dim() == 2 else b for b in batch[:-2]]
        nb += [b.unsqueeze(0) if b.dim() == 1 else b for b in batch[-2:]]
        fpc, mrpc, igt, rpc, fpcb, rpcb, fpc_idx, rpc_idx = nb[:8]
        B, N = fpc.shape[0], fpc.shape[1]

        out, _, de_fpcb, de_mrpcb = self.predict5(nb, B, training=False, need=False)
        mat = se3.exp(out).to(fpc)
        R, t = mat[:, :3, :3], mat[:, :3, 3]
        scores = [torch.as_tensor(v, dtype=torch.float32).mean().to(fpc.device) for v in self.compute_metrics(R, t, igt)]

        fpc_top = torch.topk(torch.softmax(de_fpcb, dim=1)[:, 1, :], 128, 1)[1]         # [B,128]
        mrpc_top = torch.topk(torch.softmax(de_mrpcb, dim=1)[:, 1, :], 128, 1)[1]
        pred_f = torch.zeros((B, N), dtype=fpc_idx.dtype, device=fpc.device).scatter(1, fpc_top, 1)
        pred_m = torch.zeros((B, N), dtype=fpc_idx.dtype, device=fpc.device).scatter(1, mrpc_top, 1)
        for pred, gt in ((pred_f, fpc_idx), (pred_m, rpc_idx)):
            inter = torch.sum(torch.logical_and(pred, gt)).float()
            union = torch.sum(torch.logical_or(pred, gt)).float()
            scores.append(inter / union)

        cd1, cd2 = self.chamfer_loss(fpcb, ops.index_points(fpc, fpc_top))
        scores.append(torch.mean(cd1) + torch.mean(cd2))
        moved = se3.transform(mat, ops.index_points(rpc, mrpc_top).permute(0, 2, 1)).permute(0, 2, 1)
        cd1, cd2 = self.chamfer_loss(rpcb, moved)
        scores.append(torch.mean(cd1) + torch.mean(cd2))
        return torch.stack([s.float() for s in scores]).unsqueeze(0)

    def test_epoch_end(self, outputs):
        """model5_b.py:1368-1385: mean of the per-batch score rows, printed and written to
        <output_path>/<date>metrics.txt in the reference's format (header line, then the ten values)."""
        s = torch.mean(torch.cat(list(outputs), dim=0), dim=0)
        for name, v in zip(self.METRIC_NAMES, s):
            print(f"{name}   {float(v)}")
        path = os.path.join(self.C.output_path, datetime.datetime.now().strftime('%b%d_%H-%M-%S') + 'metrics.txt')
        os.makedirs(self.C.output_path, exist_ok=True)
        with open(path, 'w+') as fout:
            fout.write('r_mse,   r_mae,   t_mse,    t_mae,    r_iso,    t_iso,  fpc_iou,   mrpc_iou, cd_fpcb, cd_rpcb \n')
            fout.write(''.join(str(v.detach().cpu().numpy()) + '   ' for v in s) + '\n')
        return s

    def configure_optimizers(self):
        """model5_b.py:1453-1457: Adam + StepLR(50, 0.999) stepped per batch."""
        on_gpu = next(self.parameters()).is_cuda
        optimizer = torch.optim.Adam(self.parameters(), lr=self.C.lr, fused=on_gpu)   # fused: same rule, one kernel chain
        self.scheduler = torch.optim.lr_scheduler.StepLR(optimizer, 50, 0.999)
        return [optimizer], [{'scheduler': self.scheduler, 'interval': 'step'}]
