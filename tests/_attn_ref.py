"""The attention kernels' truth, stated once (no GPU): one layerAttention block with every intermediate the chained
kernels leave in memory, the four-block chain, the stand-alone softmax(q k^T / sqrt(dk)) v, the input regimes in which
the softmax is not flat, and the yardstick the GPU tests measure against - the same statement evaluated in float32 on
the CPU, err32 = max|T32 - T64| per tensor.

A fixed `1e-5 * max|T|` cannot hold for ANY fp32 evaluation once logits span tens of units or carry an offset of
hundreds (the logit's own rounding, 2^-24 |s|, is an error of that size in the exponent), so the bound of a tensor is
max(1e-5 * max|T64|, M * err32): the suite's own tolerance where the input is as well conditioned as the suite's, a
multiple of what fp32 itself loses where it is not."""
import math

import torch
import torch.nn.functional as F

L, E, DK = 256, 256, 64                  # the chained kernels' only shape (csrc/attnfused.hip)
REGIMES = ("soft", "peaked", "sharp", "offset", "mixed")
BLOCK_TENSORS = ("r", "t", "map", "lse", "dz", "delta", "dq", "u", "dk", "dv", "dx")
BLOCK_PARAM_GRADS = ("dwq", "dbq", "dwk", "dbk", "dwv", "dbv", "dwo", "dbo")


def attn_block_ref(x, wq, bq, wk, bk, wv, bv, wo, bo, dr, gate=None, dtype=torch.float64):
    """model5_b.py:67-101 and its backward, every intermediate the chained kernels leave in memory, in `dtype`.
    gate: the ReLU gates the backward uses (default: the pre-activation's own, z > 0).  Besides the kernels' tensors:
    z (the pre-activation), s (the logits) and the eight parameter gradients."""
    D = dtype
    X = x.to(D)
    q, k, v = X @ wq.to(D).T + bq.to(D), X @ wk.to(D).T + bk.to(D), X @ wv.to(D).T + bv.to(D)
    s = q @ k.transpose(1, 2) / 8
    P = torch.softmax(s, dim=-1)
    t = X - P @ v
    z = t @ wo.to(D).T + bo.to(D)
    r = X + torch.relu(z)
    DR = dr.to(D)
    dz = DR * ((z > 0) if gate is None else gate.reshape(z.shape))
    dt = dz @ wo.to(D)
    dP = (-dt) @ v.transpose(1, 2)
    delta = (P * dP).sum(-1)
    dS = P * (dP - delta[..., None]) / 8
    dq, dk, dv = dS @ k, dS.transpose(1, 2) @ q, P.transpose(1, 2) @ (-dt)
    u = DR + dt                                   # (what the query-side pass leaves for the key-side pass)
    dx = u + dq @ wq.to(D) + dk @ wk.to(D) + dv @ wv.to(D)
    rows = lambda a: a.reshape(-1, a.shape[-1])
    wg = lambda d, a: rows(d).T @ rows(a)
    return dict(r=r, t=t, map=P, lse=torch.logsumexp(s, dim=-1), dz=dz, delta=delta, dq=dq, u=u, dk=dk, dv=dv, dx=dx, z=z,
                s=s, dwq=wg(dq, X), dbq=rows(dq).sum(0), dwk=wg(dk, X), dbk=rows(dk).sum(0), dwv=wg(dv, X),
                dbv=rows(dv).sum(0), dwo=wg(dz, t), dbo=rows(dz).sum(0))


def attn_chain_ref(x, blocks, w, b, dtype=None, maps=None):
    """model5_b.py:462-475: four layerAttention blocks, the projection of [r1 r2 r3 r4 x] -> (y, mean map, max of y over
    the points).  dtype=None: in the leaves' own type (they carry the gradients); maps: a list that receives the four maps."""
    c = (lambda a: a) if dtype is None else (lambda a: a.to(dtype))
    x = c(x)
    cur, ms, outs = x, [], []
    for wq, bq, wk, bk, wv, bv, wo, bo in blocks:
        q, k, v = cur @ c(wq).T + c(bq), cur @ c(wk).T + c(bk), cur @ c(wv).T + c(bv)
        a = torch.softmax(q @ k.transpose(-2, -1) / math.sqrt(q.shape[-1]), dim=-1)
        cur = cur + torch.relu((cur - a @ v) @ c(wo).T + c(bo))
        ms.append(a)
        outs.append(cur)
    if maps is not None:
        maps.extend(m.detach() for m in ms)
    y = torch.cat(outs + [x], dim=-1) @ c(w).T + c(b)
    return y, sum(ms) / 4, y.max(dim=1)[0]


def regime(name, B, seed=3):
    """(x [B,L,E], wq, bq, wk, bk, wv, bv, wo, bo, dr [B,L,E]) on the CPU: the draws of test_attention_fused_block_intermediates
    (same generator, same order), then
      soft    unchanged: logits of a query span ~2, 240 of 256 keys effective
      peaked  wq, wk x 3: ~15 effective keys
      sharp   wq, wk x 8: spread ~90, nearly one-hot
      offset  bq, bk += 12 sign(randn(dk)): a common shift of ~200 on every logit of a query, which the softmax must not see
      mixed   wq, wk x 2 and row i of x scaled by [0.05, 1, 4, 12][i % 4]: the 16 queries of a wavefront, and the four
              row groups of a lane, carry maxima orders of magnitude apart."""
    assert name in REGIMES, name
    M = B * L
    g = torch.Generator().manual_seed(seed)
    x = 0.5 * torch.randn(M, E, generator=g)
    wq, wk = [torch.randn(DK, E, generator=g) / 16 for _ in range(2)]
    wv, wo = [torch.randn(E, E, generator=g) / 16 for _ in range(2)]
    bq, bk = [torch.randn(DK, generator=g) / 4 for _ in range(2)]
    bv, bo = [torch.randn(E, generator=g) / 4 for _ in range(2)]
    dr = torch.randn(M, E, generator=g)
    if name == "peaked":
        wq, wk = 3 * wq, 3 * wk
    elif name == "sharp":
        wq, wk = 8 * wq, 8 * wk
    elif name == "offset":
        bq = bq + 12 * torch.sign(torch.randn(DK, generator=g))
        bk = bk + 12 * torch.sign(torch.randn(DK, generator=g))
    elif name == "mixed":
        wq, wk = 2 * wq, 2 * wk
        x = x * torch.tensor([0.05, 1.0, 4.0, 12.0])[torch.arange(M) % 4][:, None]
    return x.view(B, L, E), wq, bq, wk, bk, wv, bv, wo, bo, dr.view(B, L, E)


def chain_regime(B, use, seed=11, sharpen=3.0):
    """(x, blocks, w, b, wg) on the CPU: the draws of test_attention_chain_fused_vs_float64 for one encoder, every block's
    wq, wk x `sharpen`; wg is the weight of the loss, on the maximum (use = "max") or on the projection (use = "out")."""
    Nout = 1024
    g = torch.Generator().manual_seed(seed)
    shapes = [(DK, E), (DK,), (DK, E), (DK,), (E, E), (E,), (E, E), (E,)]
    x = 0.5 * torch.randn(B, L, E, generator=g)
    blocks = [[torch.randn(*s, generator=g) / (math.sqrt(E) if len(s) == 2 else 4) for s in shapes] for _ in range(4)]
    w = torch.randn(Nout, 5 * E, generator=g) / math.sqrt(5 * E)
    b = 0.1 * torch.randn(Nout, generator=g)
    wg = torch.randn(B, Nout, generator=g) if use == "max" else torch.randn(B, L, Nout, generator=g) / 16
    for blk in blocks:
        blk[0], blk[2] = sharpen * blk[0], sharpen * blk[2]
    return x, blocks, w, b, wg


def chain_eval(prob, use, dtype):
    """The chain statement and its backward in `dtype` -> (dict of y, map, fg, colmean, strips), list of the 35 gradients
    (x, 4 x 8 block parameters, w, b), the four maps.  strips: the mean map's column means per strip of 16 query rows."""
    x0, blocks0, w0, b0, wg = prob
    leaf = lambda a: a.to(dtype).clone().requires_grad_(True)
    x, blocks, w, b = leaf(x0), [[leaf(p) for p in blk] for blk in blocks0], leaf(w0), leaf(b0)
    maps = []
    y, amap, fg = attn_chain_ref(x, blocks, w, b, maps=maps)
    ((fg if use == "max" else y) * wg.to(dtype)).sum().backward()
    amap = amap.detach()
    B = amap.shape[0]
    out = dict(y=y.detach(), map=amap, fg=fg.detach(), colmean=amap.mean(dim=1), strips=amap.view(B, L // 16, 16, L).mean(dim=2))
    return out, [x.grad] + [p.grad for blk in blocks for p in blk] + [w.grad, b.grad], maps


STANDALONE_REGIMES = ("peaked", "negative")


def standalone_regime(name, B, Lk, dk, dv, seed):
    """(q, k, v, go, ga) on the CPU for softmax(q k^T / sqrt(dk)) v with a gradient into both results.
      peaked    q, k = 3^(1/2) randn: logits of sigma ~ 3
      negative  along the unit vector e = 1/sqrt(dk), q carries +40 and k's component is -(20 + |randn|), strictly negative by
                construction: every logit is (40 + n)(-(20 + |n'|)) / sqrt(dk) + O(1) < -150.  A padded column that entered the
                maximum or the sum with logit 0 would underflow every real key."""
    assert name in STANDALONE_REGIMES, name
    g = torch.Generator().manual_seed(seed)
    q, k, v = torch.randn(B, Lk, dk, generator=g), torch.randn(B, Lk, dk, generator=g), torch.randn(B, Lk, dv, generator=g)
    go, ga = torch.randn(B, Lk, dv, generator=g), torch.randn(B, Lk, Lk, generator=g)
    if name == "peaked":
        q, k = math.sqrt(3.0) * q, math.sqrt(3.0) * k
    else:
        e = torch.full((dk,), 1.0 / math.sqrt(dk))
        q = q + 40.0 * e
        along = (k * e).sum(-1, keepdim=True)
        k = k - along * e - (20.0 + along.abs()) * e
    return q, k, v, go, ga


def standalone_eval(prob, dtype):
    """softmax(q k^T / sqrt(dk)) v and its backward in `dtype` -> dict(out, attn, dq, dk, dv, s)."""
    q, k, v, go, ga = prob
    ls = [t.to(dtype).clone().requires_grad_(True) for t in (q, k, v)]
    s = ls[0] @ ls[1].transpose(-2, -1) / math.sqrt(q.shape[-1])
    attn = F.softmax(s, dim=-1)
    out = attn @ ls[2]
    ((out * go.to(dtype)).sum() + (attn * ga.to(dtype)).sum()).backward()
    return dict(out=out.detach(), attn=attn.detach(), dq=ls[0].grad, dk=ls[1].grad, dv=ls[2].grad, s=s.detach())


def yardstick(name, ref32, ref64):
    """err32 of tensor `name`: max|T32 - T64|, both from the same statement (and, for a block, the same ReLU gates)."""
    return float((ref32[name].double() - ref64[name]).abs().max())


def block_refs(args, gate=None):
    """(float32 statement, float64 statement) of one block through the same ReLU gates: the ones given, else float64's own
    (a pre-activation within fp32 rounding of zero must not turn up in the yardstick as a whole element of dr)."""
    r64 = attn_block_ref(*args, gate=gate)
    gate = (r64["z"] > 0) if gate is None else gate
    return attn_block_ref(*args, gate=gate, dtype=torch.float32), r64


def bound(name, ref32, ref64, margin):
    """The bound of a tensor: max(1e-5 max|T64|, margin * err32) -> (bound, whether the err32 term is the binding one)."""
    floor, e = 1e-5 * float(ref64[name].abs().max()), margin * yardstick(name, ref32, ref64)
    return max(floor, e), e > floor


# ---- what a regime claims, measured on the logits (statistics over the B * L queries)

def logit_stats(s):
    """s: logits [B, L, L] (float64) -> dict of per-query tensors: spread, lse, effective keys 1 / sum P^2, max probability."""
    P = torch.softmax(s, dim=-1)
    return dict(spread=(s.max(-1)[0] - s.min(-1)[0]).flatten(), lse=torch.logsumexp(s, dim=-1).flatten(),
                eff=(1.0 / (P * P).sum(-1)).flatten(), pmax=P.max(-1)[0].flatten())


def tile_max_range(s):
    """Largest difference, over the 16-row tiles a wavefront owns, between the per-query maxima of the RAW products q.k
    (= 8 s: what softmax16 sees before it scales)."""
    m = (8 * s).max(-1)[0].reshape(-1, 16)
    return float((m.max(-1)[0] - m.min(-1)[0]).max())
