"""One layerAttention block through the chained kernels' entry points, launch by launch (csrc/attnfused.hip): what
test_attention_fused_block_intermediates and the regime tests both run."""
import torch


def fused_block(dev, x, wq, bq, wk, bk, wv, bv, wo, bo, dr):
    """pzn_attn_fused_prep_weights -> proj -> fwd -> bwd_q -> bwd_k for x [B,L,E] (tensors on the CPU or the device) ->
    dict of r, t, map, lse, dz, delta, dq, u, dk, dv, dx as rows [B*L, .] on the device (u untiled; dq is checked to hold
    the same values in its two layouts)."""
    from puzzlenet_amd import _lib, ops
    B, L, E = x.shape
    dk = wq.shape[0]
    M = B * L
    x, dr = x.to(dev).reshape(M, E).contiguous(), dr.to(dev).reshape(M, E).contiguous()
    wq, bq, wk, bk, wv, bv, wo, bo = [t.to(dev).contiguous() for t in (wq, bq, wk, bk, wv, bv, wo, bo)]
    lib = _lib.load()
    assert lib.pzn_attn_fused_supported(L, E, dk)
    P = ops._ptrs
    st = torch.cuda.current_stream().cuda_stream
    raw = lambda n: torch.zeros(n, dtype=torch.uint8, device=dev)
    mk = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)
    W = raw(lib.pzn_attn_fused_weight_bytes())
    _lib.call("pzn_attn_fused_prep_weights", wq.data_ptr(), wk.data_ptr(), wv.data_ptr(), wo.data_ptr(), W.data_ptr(), st)
    qkb, vb = lib.pzn_attn_fused_qk_image_bytes(B), lib.pzn_attn_fused_v_image_bytes(B)
    qrp, krp, vrp = raw(qkb), raw(qkb), raw(vb)
    _lib.call("pzn_attn_fused_proj", 1, P([x]), P([W]), P([bq]), P([bk]), P([bv]), B, P([qrp]), P([krp]), P([vrp]), st)
    r, t, lse, amap = mk(M, E), mk(M, E), mk(M), mk(B, L, L)
    mask = torch.zeros((M, 8), dtype=torch.int32, device=dev)
    _lib.call("pzn_attn_fused_fwd", 1, P([x]), P([qrp]), P([krp]), P([vrp]), P([W]), P([bo]), B, P([r]), P([t]), P([mask]),
              P([amap]), P([lse]), 0, 1.0, st)
    dz, u, dq, delta = mk(M, E), mk(M, E), mk(M, dk), mk(M)
    dqt = mk(M, dk)
    darp = raw(vb)
    _lib.call("pzn_attn_fused_bwd_q", 1, P([dr]), E, None, E, P([mask]), P([qrp]), P([krp]), P([vrp]), P([W]), B, P([dz]), P([u]),
              P([dq]), P([dqt]), P([darp]), P([delta]), st)
    dkk, dvv, dx = mk(M, dk), mk(M, E), mk(M, E)
    _lib.call("pzn_attn_fused_bwd_k", 1, P([qrp]), P([krp]), P([vrp]), P([darp]), P([W]), P([lse]),
              P([delta]), P([u]), P([dqt]), B, P([dkk]), P([dvv]), P([dx]), st)
    torch.cuda.synchronize()
    untile = ops.attention_tile_image_rows
    assert torch.equal(untile(dqt, dk), dq)                    # the same values in the two layouts
    return dict(r=r, t=t, map=amap, lse=lse, dz=dz, delta=delta, dq=dq, u=untile(u, E), dk=dkk, dv=dvv, dx=dx)
