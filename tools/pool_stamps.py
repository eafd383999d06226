#!/usr/bin/env python3
"""Where the cycles of the pooled layers' weight-gradient pass go: phase stamps (s_memtime) of wavefronts 0 and 15 of two
workgroups of pool_wgrad_regen_kernel (csrc/poolbwd.hip), at the encoder's two production shapes.

    python tools/pool_stamps.py build        # here (cross-compiles csrc/poolbwd.hip with -DPOOL_STAMPS into
                                             #  puzzlenet_amd/libpzn_diag.so; the other objects are the product's)
    python tools/pool_stamps.py run [B]      # on the GPU box: launch times per level, then per-phase ticks per group

Phases per batch of groups: DMA landed + gate (this wavefront's wait for its own LDS-DMA of the batch, then relu(. + Q) in
place), barrier (the wait for the other 15 wavefronts), issue (the next batch's DMA and loads), hit loops.  The tick rate of
s_memtime is not assumed: ticks are reported beside the launch's event time."""
import ctypes
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = os.path.join(ROOT, "puzzlenet_amd")
STAMP_LIB = os.path.join(PKG, "libpzn_diag.so")
PHASES = ("DMA landed + gate", "barrier", "DMA + load issue", "hit loops")
# (B, N, S, C1, C2): the encoder's first and second level at the benchmark's batch
LEVELS = ((2048, 512, 128, 128), (2048, 256, 256, 256))


def build():
    from puzzlenet_amd import build as pb
    pb.build()
    os.makedirs(os.path.join(PKG, "_obj_stamps"), exist_ok=True)
    src = "poolbwd.hip"
    objs = [os.path.join(pb.OBJ, s.replace(".hip", ".o")) for s, _ in pb.SOURCES if s != src]
    o = os.path.join(PKG, "_obj_stamps", "poolbwd.o")
    subprocess.check_call([pb.hipcc()] + pb.COMMON + dict(pb.SOURCES)[src] + ["-DPOOL_STAMPS", "-c", os.path.join(pb.CSRC, src), "-o", o])
    subprocess.check_call([pb.hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-o", STAMP_LIB] + objs + [o])
    print(STAMP_LIB)


def run(B):
    import torch
    from puzzlenet_amd import _lib
    _lib.LIB_PATH = os.environ.get("PZN_STAMP_LIB", STAMP_LIB)
    lib = _lib.load()
    rd = lib.pzn_pool_wgrad_read_stamps
    rd.restype = ctypes.c_int
    rd.argtypes = [ctypes.c_void_p, ctypes.c_int]
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    host = (ctypes.c_longlong * (2 * 2 * 2 * 8))()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    for N, S, C1, C2 in LEVELS:
        G = B * S
        g = torch.Generator(device=dev).manual_seed(C1 + S)
        P = torch.randn(B * N, C1, device=dev, generator=g)
        Q = 0.5 * torch.randn(G, C1, device=dev, generator=g)
        idx = torch.randint(0, N, (G, 32), device=dev, generator=g, dtype=torch.int64)
        dout = torch.randn(G, C2, device=dev, generator=g)
        argmax = torch.randint(0, 32, (G, C2), device=dev, generator=g, dtype=torch.int32)
        out = torch.randn(G, C2, device=dev, generator=g) + 0.12        # ~45 % of the channels dead, as trained
        dW, db = torch.zeros(C2, C1, device=dev), torch.zeros(C2, device=dev)
        ws = torch.empty(lib.pzn_pool_wgrad_workspace_bytes(G, C1, C2) // 4, device=dev)

        def call():
            rc = lib.pzn_pool_wgrad_f32(p(dout), p(argmax), p(out), None, p(P), p(Q), p(idx), N, S, G, C1, C2, p(dW), p(db),
                                        p(ws), ctypes.c_void_p(st))
            assert rc == 0, rc
        for _ in range(3):
            call()
        torch.cuda.synchronize()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        for _ in range(20):
            call()
        ev[1].record()
        torch.cuda.synchronize()
        us = ev[0].elapsed_time(ev[1]) / 20 * 1e3          # (the weight pass + its fixed-order reduction)
        rd(host, 1)
        call()
        torch.cuda.synchronize()
        rd(host, 0)
        k16 = 1 if C2 // 16 == 16 else 0
        print(f"pool_wgrad_regen_kernel<{C2 // 16}>  G={G} C1={C1} C2={C2}: {us:.1f} us per launch (+ reduction)")
        for wg in range(2):
            for wv in range(2):
                v = [host[((k16 * 2 + wg) * 2 + wv) * 8 + i] for i in range(8)]
                groups, tot = v[4], sum(v[:4])
                if groups == 0 or tot == 0:
                    continue
                print(f"  workgroup {0 if wg == 0 else 77:2d} wavefront {0 if wv == 0 else 15:2d}: {groups} groups, {tot} ticks in the walk")
                for k, name in enumerate(PHASES):
                    print(f"    {name:22s} {v[k]:9d} ticks  {100.0 * v[k] / tot:5.1f} %  {v[k] / groups:8.1f} ticks per group")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "build":
        build()
    else:
        run(int(sys.argv[2]) if len(sys.argv) > 2 else 64)
