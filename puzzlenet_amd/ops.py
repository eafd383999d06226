"""Host-side operators over the C ABI (include/pzn.h).

torch is used for device memory, the current HIP stream and autograd plumbing
only: every computation below is a call into libpzn.so with raw device
pointers.  Inputs must live on a HIP device; there is no CPU path.
"""
import collections
import ctypes
import numbers
import os
import weakref

import torch

from . import _lib


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_cur_device = getattr(torch._C, "_cuda_getDevice", None)


def _stream():
    """Raw handle of torch's current stream on the current device.  (torch.cuda.current_stream() builds a Stream object:
    9 us a call, 77 calls per training step; the raw getter is what torch's own C++ extensions use.)"""
    if _raw_stream is not None and _cur_device is not None:
        return _raw_stream(_cur_device())
    return torch.cuda.current_stream().cuda_stream


class _NoCtx:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


_NO_CTX = _NoCtx()


def _on(dev):
    """`with _on(dev):` = torch.cuda.device(dev), skipped when dev is already the current device (one process per GPU:
    always; the context manager cost 10 us per use, 70 uses per step)."""
    if _cur_device is not None and dev.index is not None and dev.index == _cur_device():
        return _NO_CTX
    return torch.cuda.device(dev)


class KernelTimer:
    """Optional per-entry-point device timing with HIP events recorded on the stream the
    kernels are launched on (torch's current stream).  Off by default; bench.py turns it on
    for the timed region to price individual kernels (roofline.achieved)."""
    enabled = False
    records = {}
    flops = {}
    shapes = None   # set to {} before start() to also collect {(entry point, int args): [ms, ...]} (tools/)
    variants = {}   # {(entry point, variant tag): (launches, ms, flops)} for calls that pass variant= (one kernel instantiation each)

    @classmethod
    def start(cls):
        cls.records = {}
        cls.enabled = True

    @classmethod
    def stop(cls):
        """-> {entry point: (launches, total milliseconds)}; synchronises the device."""
        cls.enabled = False
        torch.cuda.synchronize()
        out = {k: (len(v), sum(a.elapsed_time(b) for a, b, _ in v)) for k, v in cls.records.items()}
        cls.variants = {}
        for k, v in cls.records.items():
            for a, b, f in v:
                if isinstance(f, tuple) and isinstance(f[-1], str):
                    n_, ms_, fl_ = cls.variants.get((k, f[-1]), (0, 0.0, 0))
                    cls.variants[(k, f[-1])] = (n_ + 1, ms_ + a.elapsed_time(b), fl_ + f[0])
            v[:] = [(a, b, f[0] if (isinstance(f, tuple) and isinstance(f[-1], str)) else f) for a, b, f in v]
        if cls.shapes is not None:
            for k, v in cls.records.items():
                for a, b, f in v:
                    if isinstance(f, tuple):
                        cls.shapes.setdefault((k,) + f[1], []).append(a.elapsed_time(b))
            for v in cls.records.values():
                v[:] = [(a, b, f[0] if isinstance(f, tuple) else f) for a, b, f in v]
        cls.flops = {k: sum(f for _, _, f in v) for k, v in cls.records.items()}
        cls.records = {}
        return out


def ktimer_start():
    """Per-KERNEL device time from inside the library (pzn_ktimer_*, csrc/core.hip): from here on every kernel libpzn.so
    launches is bracketed by its own HIP event pair on its own stream.  Measurement only (bench.py)."""
    _lib.check(_lib.load().pzn_ktimer_collect() < 0, "pzn_ktimer_collect")      # (drop spans of an earlier window)
    _lib.check(_lib.load().pzn_ktimer_enable(1), "pzn_ktimer_enable")


def ktimer_stop():
    """-> {kernel name as in a rocprofv3 trace (template arguments included): (launches, summed milliseconds)}."""
    lib = _lib.load()
    _lib.check(lib.pzn_ktimer_enable(0), "pzn_ktimer_enable")
    n = lib.pzn_ktimer_collect()
    if n < 0:
        _lib.check(n, "pzn_ktimer_collect")
    out = {}
    buf = ctypes.create_string_buffer(512)
    cnt, ms = ctypes.c_int(0), ctypes.c_double(0.0)
    for i in range(n):
        _lib.check(lib.pzn_ktimer_row(i, buf, 512, ctypes.byref(cnt), ctypes.byref(ms)), "pzn_ktimer_row")
        out[buf.value.decode()] = (cnt.value, ms.value)
    return out


# tests set this to a list: every max-pool of the model path appends (kind, address of the layer's weight or None, arg-max
# tensor) - "sa": [B,S,C2] neighbour slots of a set-abstraction level (weight = its second layer's), "gmax": [B,Nout] rows of
# the out projection's max over the points (weight = the projection's), "maxpts": [B,C] rows of max_over_points
WINNER_CAPTURE = None


def _call(name, *args, flops=0, variant=None):
    """Invoke a C-ABI entry point; `flops` = algorithmic 2*M*N*K of the dense entry points (bench accounting); `variant` =
    the template arguments of the kernel this call launches, where one entry point has several instantiations."""
    if KernelTimer.enabled:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        _lib.call(name, *args)
        b.record()
        if variant is not None and KernelTimer.shapes is None:
            flops = (flops, variant)
        if KernelTimer.shapes is not None:
            flops = (flops, tuple(x for x in args if isinstance(x, int) and 0 <= x < (1 << 31)))
        KernelTimer.records.setdefault(name, []).append((a, b, flops))
    else:
        _lib.call(name, *args)


def _req(t, dtype, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise _lib.PznError(f"{name} must be a tensor on the GPU (got {type(t).__name__}"
                            f"{'' if not isinstance(t, torch.Tensor) else ' on ' + str(t.device)}); "
                            "puzzlenet_amd has no CPU fallback")
    if t.dtype != dtype:
        t = t.to(dtype)
    return t.contiguous()


def _f32(t, name):
    return _req(t, torch.float32, name)


def _i64(t, name):
    return _req(t, torch.int64, name)


def _p(t):
    return None if t is None else t.data_ptr()


# --------------------------------------------------------------------------- point ops

def square_distance(src, dst):
    src, dst = _f32(src, "src"), _f32(dst, "dst")
    B, S, C = src.shape
    if C != 3 or dst.shape[-1] != 3 or dst.shape[0] != B:
        raise _lib.PznError("square_distance: expected src[B,S,3], dst[B,N,3]")
    N = dst.shape[1]
    out = torch.empty((B, S, N), dtype=torch.float32, device=src.device)
    with _on(src.device):
        _call("pzn_square_distance_f32", _p(src), _p(dst), B, S, N, _p(out), _stream())
    return out


def farthest_point_sample(xyz, npoint, start_idx, background=False, counts=None, max_count=0):
    """background=True: the same picks from the small-footprint launch (no LDS image of the cloud; pzn_fps_background_f32):
    for sampling that runs on a side stream beside a training step (datapipe.PairFeeder); counts [B] int64: rows >= counts[b]
    of cloud b are padding copies of its row 0 and are skipped; max_count: the caller's promise counts <= max_count (0: none)."""
    xyz = _f32(xyz, "xyz")
    B, N, C = xyz.shape
    if C != 3:
        raise _lib.PznError("farthest_point_sample: expected xyz[B,N,3]")
    start_idx = _i64(start_idx, "start_idx")
    out = torch.empty((B, npoint), dtype=torch.int64, device=xyz.device)
    with _on(xyz.device):
        if background:
            counts = None if counts is None else _i64(counts, "counts")
            _call("pzn_fps_background_f32", _p(xyz), B, N, int(npoint), _p(start_idx), _p(out), _p(counts), int(max_count), _stream())
        else:
            _call("pzn_fps_f32", _p(xyz), B, N, int(npoint), _p(start_idx), _p(out), _stream())
    return out


def merge_resample_supported(Na, Nb, n_out):
    return bool(_lib.load().pzn_merge_resample_supported(int(Na), int(Nb), int(n_out)))


def merge_resample(a, b, T, start, n_out=None, drop_a=None, drop_b=None):
    """M merges in one launch (pzn_merge_resample_f32): the union of a[M,Na,3] and T[M,4,4] applied to b[M,Nb,3], resampled
    to n_out (default Na) points by farthest point sampling from the union index start[M] -> (points [M,n_out,3] in pick
    order, src [M,n_out] int64 union index of every pick: u < Na is row u of a, otherwise row u - Na of b).  drop_a[M,ka],
    drop_b[M,kb] (int64, optional): rows that start at running distance 0, i.e. are picked only when every kept row is at 0
    too; a start on a dropped row moves to the first kept row at or after it, wrapping round.  Na + Nb <= 4096
    (PznUnsupported beyond).  No autograd, nothing waits for the device."""
    a, b, T = _f32(a, "a"), _f32(b, "b"), _f32(T, "T")
    if a.dim() != 3 or b.dim() != 3 or a.shape[2] != 3 or b.shape[2] != 3 or b.shape[0] != a.shape[0]:
        raise _lib.PznError(f"merge_resample: expected a[M,Na,3], b[M,Nb,3]; got {tuple(a.shape)}, {tuple(b.shape)}")
    M, Na, Nb = a.shape[0], a.shape[1], b.shape[1]
    if T.shape != (M, 4, 4):
        raise _lib.PznError(f"merge_resample: expected T[{M},4,4]; got {tuple(T.shape)}")
    start = _i64(start, "start")
    if start.shape != (M,):
        raise _lib.PznError(f"merge_resample: expected start[{M}]; got {tuple(start.shape)}")
    n_out = Na if n_out is None else int(n_out)
    drops = []
    for name, d in (("drop_a", drop_a), ("drop_b", drop_b)):
        if d is not None:
            d = _i64(d, name)
            if d.dim() != 2 or d.shape[0] != M:
                raise _lib.PznError(f"merge_resample: expected {name}[{M},k]; got {tuple(d.shape)}")
            if d.shape[1] == 0:
                d = None
        drops.append(d)
    da, db = drops
    if M == 0 or not merge_resample_supported(Na, Nb, n_out):
        raise _lib.PznUnsupported(f"merge_resample: M = {M} merges of Na = {Na} and Nb = {Nb} rows to n_out = {n_out} "
                                  "(Na + Nb <= 4096, 1 <= n_out <= Na + Nb)")
    out = torch.empty((M, n_out, 3), dtype=torch.float32, device=a.device)
    src = torch.empty((M, n_out), dtype=torch.int64, device=a.device)
    with _on(a.device):
        _call("pzn_merge_resample_f32", _p(a), _p(b), _p(T), _p(start), _p(da), 0 if da is None else da.shape[1], _p(db),
              0 if db is None else db.shape[1], M, Na, Nb, n_out, _p(out), _p(src), _stream())
    return out, src


def _no_conversion(who, specs):
    """specs: (name, value, accepted dtypes).  A tensor of another dtype is refused, not converted: a pose refined in another
    precision, or an index read as another width, is not what the caller asked for."""
    for name, t, dts in specs:
        if isinstance(t, torch.Tensor) and t.dtype not in dts:
            raise _lib.PznError(f"{who}: {name} must be {' or '.join(str(d) for d in dts)}; got {t.dtype}")


def _set_maps(who, n_rows, shape, a_of, a, b_of, b):
    """The set maps of a refinement launch of n_rows rows (poses [P], or joint rows [Z,J]: `shape`): a map is int64 of that
    shape into a non-empty a / b; without one, a / b hold n_rows sets.  -> (a_of, b_of), contiguous or None."""
    what = f"P = {n_rows} poses" if len(shape) == 1 else f"Z J = {n_rows} joint rows"
    maps = []
    for name, m, x in (("a_of", a_of, a), ("b_of", b_of, b)):
        if m is None:
            if x.shape[0] != n_rows:
                raise _lib.PznError(f"{who}: {name[0]} holds {x.shape[0]} sets for {what} and no {name} is given")
        else:
            m = _i64(m, name)
            if m.shape != tuple(shape):
                raise _lib.PznError(f"{who}: expected {name}[{','.join(str(n) for n in shape)}]; got {tuple(m.shape)}")
            if x.shape[0] == 0 and n_rows > 0:
                raise _lib.PznError(f"{who}: {name} indexes an empty {name[0]}")
        maps.append(m)
    return maps


def icp_refine_supported(ka, kb):
    return bool(_lib.load().pzn_icp_refine_supported(int(ka), int(kb)))


def icp_refine_trim_supported(ka, kb, keep_a, keep_b):
    return bool(_lib.load().pzn_icp_refine_trim_supported(int(ka), int(kb), int(keep_a), int(keep_b)))


def icp_refine_auto_supported(ka, kb, lo_a, lo_b, power):
    return bool(_lib.load().pzn_icp_refine_auto_supported(int(ka), int(kb), int(lo_a), int(lo_b), int(power)))


def icp_refine(a, b, T0, iters, a_of=None, b_of=None, return_corr=False, keep=None, return_kept=False, auto=None):
    """P pose refinements in one launch (pzn_icp_refine_f32): symmetric point-to-point ICP of the moved set b[.,kb,3] onto the
    fixed set a[.,ka,3] from T0[P,4,4], at most `iters` accepted steps per problem -> (T [P,4,4], score [P], score0 [P],
    iters_used [P] int32), and with return_corr the correspondences the last candidate was built from, corr_a [P,ka] and
    corr_b [P,kb] (int32).  score = E(T) <= score0 = E(T0), E as include/pzn.h states it; iters = 0 returns T0.
    Problem p reads a[a_of[p]] and b[b_of[p]] (int64 [P]; the caller keeps them inside a / b - they are not checked, that
    would wait for the device); without a map, a / b hold P sets.  1 <= ka, kb <= 1024 and iters >= 0 (PznUnsupported
    beyond).  No autograd, nothing waits for the device.
    keep = (m_a, m_b), ints: the trimmed refinement for partial contact (pzn_icp_refine_trim_f32, one launch of its own
    kernel): of each direction's rows only the m with the smallest (minimum, index) count in E and as pairs of the step;
    1 <= m_a <= ka, 1 <= m_b <= kb (PznUnsupported beyond, before any launch).  return_kept appends kept_a [P,m_a] and kept_b
    [P,m_b] (int32, ascending): the rows kept under the returned T.  keep = None is the untrimmed launch, untouched; with it
    return_kept gives 0 .. k-1.
    auto = (lo_a, lo_b, power), ints, exclusive with keep: the counts are found per problem and per evaluated pose
    (pzn_icp_refine_auto_f32, one launch of its own kernel; include/pzn.h states the rule): the m in [lo, k] with the
    smallest (prefix sum of the sorted minima) / m^(power + 1), the step taken iff the objective F falls.  1 <= lo_a <= ka,
    1 <= lo_b <= kb, 1 <= power <= 4 (PznUnsupported beyond, before any launch).  The result is then (T, score, score0,
    iters_used[, corr_a, corr_b], count_a [P] int32, count_b [P] int32, objective [P]) and with return_kept kept_a [P,ka],
    kept_b [P,kb] (int32): the kept rows ascending, then -1.  score is the trimmed E at the returned pose's counts and may
    exceed score0; objective never exceeds the F of T0.  auto = (ka, kb, p) is keep = (ka, kb) bit for bit."""
    f32, i64 = (torch.float32,), (torch.int64,)
    _no_conversion("icp_refine", (("a", a, f32), ("b", b, f32), ("T0", T0, f32), ("a_of", a_of, i64), ("b_of", b_of, i64)))
    a, b, T0 = _f32(a, "a"), _f32(b, "b"), _f32(T0, "T0")
    if a.dim() != 3 or b.dim() != 3 or a.shape[2] != 3 or b.shape[2] != 3:
        raise _lib.PznError(f"icp_refine: expected a[.,ka,3], b[.,kb,3]; got {tuple(a.shape)}, {tuple(b.shape)}")
    if T0.dim() != 3 or T0.shape[1:] != (4, 4):
        raise _lib.PznError(f"icp_refine: expected T0[P,4,4]; got {tuple(T0.shape)}")
    P, ka, kb = T0.shape[0], a.shape[1], b.shape[1]
    maps = _set_maps("icp_refine", P, (P,), a_of, a, b_of, b)
    iters = int(iters)
    if iters < 0 or not icp_refine_supported(ka, kb):
        raise _lib.PznUnsupported(f"icp_refine: ka = {ka}, kb = {kb}, iters = {iters} (1 <= ka, kb <= 1024, iters >= 0)")
    if keep is not None:
        if not isinstance(keep, (tuple, list)) or len(keep) != 2 or not all(isinstance(m, int) and not isinstance(m, bool) for m in keep):
            raise _lib.PznError(f"icp_refine: keep = (m_a, m_b) as ints; got {keep!r}")
        if not icp_refine_trim_supported(ka, kb, keep[0], keep[1]):
            raise _lib.PznUnsupported(f"icp_refine: keep = {tuple(keep)} of ka = {ka}, kb = {kb} rows (1 <= m_a <= ka, 1 <= m_b <= kb)")
    if auto is not None:
        if keep is not None:
            raise _lib.PznError("icp_refine: keep and auto exclude each other (counts given, or counts found)")
        if not isinstance(auto, (tuple, list)) or len(auto) != 3 or not all(isinstance(m, int) and not isinstance(m, bool) for m in auto):
            raise _lib.PznError(f"icp_refine: auto = (lo_a, lo_b, power) as ints; got {auto!r}")
        if not icp_refine_auto_supported(ka, kb, *auto):
            raise _lib.PznUnsupported(f"icp_refine: auto = {tuple(auto)} of ka = {ka}, kb = {kb} rows (1 <= lo_a <= ka, 1 <= lo_b <= kb, "
                                      "1 <= power <= 4)")
    # the form, resolved once: the entry point, its integer arguments before iters and the widths of the kept sets it can
    # write (None: it writes none, and return_kept answers 0 .. k-1); the auto form alone finds counts and an objective
    if auto is not None:
        sym, ints, widths = "pzn_icp_refine_auto_f32", tuple(auto), (ka, kb)
    elif keep is not None:
        sym, ints, widths = "pzn_icp_refine_trim_f32", tuple(keep), tuple(keep)
    else:
        sym, ints, widths = "pzn_icp_refine_f32", (), None
    dev = a.device

    def out(shape, dtype=torch.int32):
        return torch.empty(shape, dtype=dtype, device=dev)

    T, score, score0, used = out((P, 4, 4), torch.float32), out((P,), torch.float32), out((P,), torch.float32), out((P,))
    ca, cb = (out((P, ka)), out((P, kb))) if return_corr else (None, None)
    found = (out((P,)), out((P,)), out((P,), torch.float32)) if auto is not None else ()
    kept = tuple(out((P, m)) for m in widths) if return_kept and widths else ()
    tail = () if widths is None else tuple(_p(t) for t in kept) or (None, None)
    if P > 0:
        with _on(dev):
            _call(sym, _p(a), _p(maps[0]), _p(b), _p(maps[1]), _p(T0), P, ka, kb, *ints, iters, _p(T), _p(score), _p(score0),
                  _p(used), _p(ca), _p(cb), *(_p(t) for t in found), *tail, _stream())
    if return_kept and widths is None:
        kept = tuple(torch.arange(k, dtype=torch.int32, device=dev).expand(P, k).contiguous() for k in (ka, kb))
    return ((T, score, score0, used, ca, cb) if return_corr else (T, score, score0, used)) + found + kept


def joint_refine_supported(K, J, ka, kb):
    return bool(_lib.load().pzn_joint_refine_supported(int(K), int(J), int(ka), int(kb)))


def joint_refine_trim_supported(K, J, ka, kb):
    return bool(_lib.load().pzn_joint_refine_trim_supported(int(K), int(J), int(ka), int(kb)))


def joint_refine_auto_supported(K, J, ka, kb, lo_a, lo_b, power):
    return bool(_lib.load().pzn_joint_refine_auto_supported(int(K), int(J), int(ka), int(kb), int(lo_a), int(lo_b), int(power)))


def joint_refine(a, b, joints, G0, movable, sweeps, a_of=None, b_of=None, na=None, nb=None, ma=None, mb=None, return_kept=False,
                 auto=None):
    """Z pose graphs refined in one launch (pzn_joint_refine_f32): puzzle z has the poses G0[z] [K,4,4], the mask movable[z]
    [K] (uint8 or bool) and the joint rows joints[z] [J,2] (int32 ordered pairs (i, j); a row with i < 0 is unused); row e has
    the set a[a_of[z,e]] [ka,3] in piece i's frame and b[b_of[z,e]] [kb,3] in piece j's (int64 [Z,J]; the caller keeps them
    inside a / b - they are not checked, that would wait for the device; without a map, a / b hold Z J sets).  Block-coordinate
    descent over the pieces as include/pzn.h states it, at most `sweeps` sweeps -> (G [Z,K,4,4], score [Z], score0 [Z],
    joint_score [Z,J], sweeps_used [Z] int32, accepted [Z,K] int32); score = E(G) <= score0 = E(G0); sweeps = 0 returns G0.
    joints may be a host tensor, the caller's own copy: then every used row is checked (0 <= i, j < K, i != j, no pair twice;
    PznError) and the list is uploaded; a device tensor is not checked, and the kernel skips such rows.
    na / nb (int32 [a.shape[0]] / [b.shape[0]]): a point count per SET of a / of b - set s holds na[s] points in its first
    rows, what lies behind them is never read (NaN is fine), and every ka / kb of the energy and of a visit is that row's count
    (pzn_joint_refine_counts_f32; ka, kb stay the strides).  Like joints: a host tensor is checked (1 <= n <= ka; PznError) and
    uploaded, a device tensor is not, and the kernel skips a row with a count out of range (joint_score 0).  With both None
    the launch is pzn_joint_refine_f32; one of them alone leaves the other side at its full size.
    ma / mb (int32 [Z,J]): partial contact - a kept count per joint ROW (pzn_joint_refine_trim_f32, one launch of its own
    kernel; include/pzn.h states the rule): of row e's ka rows of A only the ma[z,e] with the smallest (row minimum, row index)
    under the poses at hand count, in E_e and as pairs of a visit, of its kb rows of B the mb[z,e]; which rows those are is
    decided again at every evaluation.  A host tensor is checked (1 <= m <= k on the used rows - those with i >= 0 where
    joints is a host tensor too, every row otherwise; PznError) and uploaded; a device tensor is not, and the kernel skips a
    row with a count out of range.  One of them alone leaves the other side at its full size; counts together with na / nb
    are a PznError.  return_kept appends kept_a [Z,J,ka] and kept_b [Z,J,kb] (int32): the rows kept under the returned poses,
    ascending, -1 behind the count and throughout a skipped row (without counts: that launch with every row kept).  With ma,
    mb None and return_kept False nothing changes: the same launch and the same tuple.
    auto = (lo_a, lo_b, power), ints: the two counts of every joint are FOUND at every evaluation of the joint, under the poses
    being tried (pzn_joint_refine_auto_f32, one launch of its own kernel; include/pzn.h states the rule): per direction the m in
    [lo, k] with the smallest (prefix sum of the sorted row minima) / m^(power + 1); the joint is scored by the objective F of
    that rule and a candidate is taken iff F falls.  auto together with any of na, nb, ma, mb is a PznError; 1 <= lo_a <= ka,
    1 <= lo_b <= kb, 1 <= power <= 4 (PznUnsupported beyond, before any launch).  The result is then the six outputs above
    (score, score0 and joint_score in the trimmed E at the counts found: score may exceed score0), with return_kept kept_a
    [Z,J,ka], kept_b [Z,J,kb], and then count_a [Z,J], count_b [Z,J] (int32, 0 for a skipped row), objective [Z], objective0
    [Z] (the sums of F under G and G0; objective <= objective0 to the bit).  auto = (ka, kb, p) is the plain launch bit for bit.
    1 <= K <= 64, J <= K (K - 1), 1 <= ka, kb <= 1024 and sweeps >= 0 (PznUnsupported beyond).  Z = 0 or J = 0 launches
    nothing and returns G0 with scores of 0.  No autograd, nothing waits for the device."""
    f32, i32, i64 = (torch.float32,), (torch.int32,), (torch.int64,)
    _no_conversion("joint_refine", (("a", a, f32), ("b", b, f32), ("G0", G0, f32), ("joints", joints, i32),
                                    ("movable", movable, (torch.uint8, torch.bool)), ("a_of", a_of, i64), ("b_of", b_of, i64),
                                    ("na", na, i32), ("nb", nb, i32), ("ma", ma, i32), ("mb", mb, i32)))
    if auto is not None:
        if any(x is not None for x in (na, nb, ma, mb)):
            raise _lib.PznError("joint_refine: auto (counts found per joint) excludes na / nb / ma / mb (counts given)")
        if not isinstance(auto, (tuple, list)) or len(auto) != 3 or not all(isinstance(m, int) and not isinstance(m, bool) for m in auto):
            raise _lib.PznError(f"joint_refine: auto = (lo_a, lo_b, power) as ints; got {auto!r}")
    trim = auto is None and (ma is not None or mb is not None or bool(return_kept))
    if trim and (na is not None or nb is not None):
        raise _lib.PznError("joint_refine: kept counts per row (ma / mb, return_kept) and point counts per set (na / nb) exclude "
                            "each other")
    a, b, G0 = _f32(a, "a"), _f32(b, "b"), _f32(G0, "G0")
    if a.dim() != 3 or b.dim() != 3 or a.shape[2] != 3 or b.shape[2] != 3:
        raise _lib.PznError(f"joint_refine: expected a[.,ka,3], b[.,kb,3]; got {tuple(a.shape)}, {tuple(b.shape)}")
    if G0.dim() != 4 or G0.shape[2:] != (4, 4):
        raise _lib.PznError(f"joint_refine: expected G0[Z,K,4,4]; got {tuple(G0.shape)}")
    Z, K, ka, kb = G0.shape[0], G0.shape[1], a.shape[1], b.shape[1]
    if not isinstance(joints, torch.Tensor) or joints.dim() != 3 or joints.shape[0] != Z or joints.shape[2] != 2:
        raise _lib.PznError(f"joint_refine: expected joints[{Z},J,2]; got "
                            f"{tuple(joints.shape) if isinstance(joints, torch.Tensor) else type(joints).__name__}")
    J = joints.shape[1]
    used_rows = None      # the used rows as the caller's host copy of the list shows them
    if not joints.is_cuda:      # the caller's host copy: a check that waits for nothing
        i, j = joints[..., 0], joints[..., 1]
        used_rows = i >= 0
        bad = (i >= 0) & ((i >= K) | (j < 0) | (j >= K) | (i == j))
        if bool(bad.any()):
            z, e = (int(v) for v in bad.nonzero()[0])
            raise _lib.PznError(f"joint_refine: joints[{z},{e}] = ({int(i[z, e])}, {int(j[z, e])}) is no joint of K = {K} pieces")
        key = torch.where(i >= 0, i.long() * K + j.long(), -1 - torch.arange(J).expand(Z, J))      # unused rows: all different
        if J > 1 and bool((key.sort(dim=1).values.diff(dim=1) == 0).any()):
            raise _lib.PznError("joint_refine: a pair (i, j) is listed twice in one puzzle's joints")
        joints = joints.to(a.device)
    joints = _req(joints, torch.int32, "joints")
    movable = _req(movable, movable.dtype if isinstance(movable, torch.Tensor) else torch.uint8, "movable")
    if movable.shape != (Z, K):
        raise _lib.PznError(f"joint_refine: expected movable[{Z},{K}]; got {tuple(movable.shape)}")
    movable = movable.view(torch.uint8)
    maps = _set_maps("joint_refine", Z * J, (Z, J), a_of, a, b_of, b)
    counts = []
    for name, n, x, cap in (("na", na, a, ka), ("nb", nb, b, kb)):
        if n is not None:
            if not isinstance(n, torch.Tensor) or n.shape != (x.shape[0],):
                raise _lib.PznError(f"joint_refine: expected {name}[{x.shape[0]}] (one count per set of {name[1]}); got "
                                    f"{tuple(n.shape) if isinstance(n, torch.Tensor) else type(n).__name__}")
            if n.device.type not in ("cpu", "cuda"):
                raise _lib.PznError(f"joint_refine: {name} must be on the GPU or a host tensor; got one on {n.device}")
            if not n.is_cuda:      # the caller's host copy, as for joints
                bad = (n < 1) | (n > cap)
                if bool(bad.any()):
                    s = int(bad.nonzero()[0])
                    raise _lib.PznError(f"joint_refine: {name}[{s}] = {int(n[s])} is no count of a set of {cap} rows")
                n = n.to(a.device)
            n = _req(n, torch.int32, name)
        counts.append(n)
    kept_counts = []
    for name, m, cap in (("ma", ma, ka), ("mb", mb, kb)):
        if m is not None:
            if not isinstance(m, torch.Tensor) or m.shape != (Z, J):
                raise _lib.PznError(f"joint_refine: expected {name}[{Z},{J}] (one kept count per joint row); got "
                                    f"{tuple(m.shape) if isinstance(m, torch.Tensor) else type(m).__name__}")
            if m.device.type not in ("cpu", "cuda"):
                raise _lib.PznError(f"joint_refine: {name} must be on the GPU or a host tensor; got one on {m.device}")
            if not m.is_cuda:      # the caller's host copy, as for joints
                bad = (m < 1) | (m > cap)
                if used_rows is not None:
                    bad = bad & used_rows
                if bool(bad.any()):
                    z, e = (int(v) for v in bad.nonzero()[0])
                    raise _lib.PznError(f"joint_refine: {name}[{z},{e}] = {int(m[z, e])} is no kept count of a set of {cap} rows")
                m = m.to(a.device)
            m = _req(m, torch.int32, name)
        kept_counts.append(m)
    sweeps = int(sweeps)
    if sweeps < 0 or not (joint_refine_trim_supported if trim else joint_refine_supported)(K, J, ka, kb):
        raise _lib.PznUnsupported(f"joint_refine: K = {K}, J = {J}, ka = {ka}, kb = {kb}, sweeps = {sweeps} "
                                  "(1 <= K <= 64, J <= K (K - 1), 1 <= ka, kb <= 1024, sweeps >= 0)")
    if auto is not None and not joint_refine_auto_supported(K, J, ka, kb, *auto):
        raise _lib.PznUnsupported(f"joint_refine: auto = {tuple(auto)} of ka = {ka}, kb = {kb} rows (1 <= lo_a <= ka, 1 <= lo_b <= kb, "
                                  "1 <= power <= 4)")
    dev = a.device
    kept = tuple(torch.empty((Z, J, k), dtype=torch.int32, device=dev) for k in (ka, kb)) if return_kept else ()      # (empty if Z J = 0)
    # what the auto form alone gives: count_a, count_b, objective, objective0 (zeros where nothing is launched)
    new = torch.zeros if Z == 0 or J == 0 else torch.empty
    found = () if auto is None else (new((Z, J), dtype=torch.int32, device=dev), new((Z, J), dtype=torch.int32, device=dev),
                                     new((Z,), dtype=torch.float32, device=dev), new((Z,), dtype=torch.float32, device=dev))
    if Z == 0 or J == 0:
        return (G0.clone(), torch.zeros((Z,), dtype=torch.float32, device=dev), torch.zeros((Z,), dtype=torch.float32, device=dev),
                torch.zeros((Z, J), dtype=torch.float32, device=dev), torch.zeros((Z,), dtype=torch.int32, device=dev),
                torch.zeros((Z, K), dtype=torch.int32, device=dev)) + kept + found
    G = torch.empty((Z, K, 4, 4), dtype=torch.float32, device=dev)
    score = torch.empty((Z,), dtype=torch.float32, device=dev)
    score0 = torch.empty_like(score)
    joint_score = torch.empty((Z, J), dtype=torch.float32, device=dev)
    used = torch.empty((Z,), dtype=torch.int32, device=dev)
    accepted = torch.empty((Z, K), dtype=torch.int32, device=dev)
    kept_a, kept_b = kept or (None, None)
    with _on(dev):
        if auto is not None:
            _call("pzn_joint_refine_auto_f32", _p(a), _p(maps[0]), _p(b), _p(maps[1]), _p(joints), _p(G0), _p(movable), Z, K, J, ka, kb,
                  auto[0], auto[1], auto[2], sweeps, _p(G), _p(score), _p(score0), _p(joint_score), _p(used), _p(accepted),
                  _p(found[2]), _p(found[3]), _p(found[0]), _p(found[1]), _p(kept_a), _p(kept_b), _stream())
        elif trim:
            _call("pzn_joint_refine_trim_f32", _p(a), _p(maps[0]), _p(kept_counts[0]), _p(b), _p(maps[1]), _p(kept_counts[1]),
                  _p(joints), _p(G0), _p(movable), Z, K, J, ka, kb, sweeps, _p(G), _p(score), _p(score0), _p(joint_score), _p(used),
                  _p(accepted), _p(kept_a), _p(kept_b), _stream())
        elif counts[0] is None and counts[1] is None:
            _call("pzn_joint_refine_f32", _p(a), _p(maps[0]), _p(b), _p(maps[1]), _p(joints), _p(G0), _p(movable), Z, K, J, ka, kb,
                  sweeps, _p(G), _p(score), _p(score0), _p(joint_score), _p(used), _p(accepted), _stream())
        else:
            _call("pzn_joint_refine_counts_f32", _p(a), _p(maps[0]), _p(counts[0]), _p(b), _p(maps[1]), _p(counts[1]), _p(joints),
                  _p(G0), _p(movable), Z, K, J, ka, kb, sweeps, _p(G), _p(score), _p(score0), _p(joint_score), _p(used),
                  _p(accepted), _stream())
    return (G, score, score0, joint_score, used, accepted) + kept + found


def assemble_walk_supported(K):
    return bool(_lib.load().pzn_assemble_walk_supported(int(K)))


def _walk_args(who, score, T, count, max_score, joint_score):
    """What the assemble_* walks take alike, checked -> (score, T, count, max_score, joint_score, Z, K) as the
    library takes them: no limit is +inf, no joint_score NaN."""
    for name, t, dt in (("score", score, torch.float32), ("T", T, torch.float32), ("count", count, torch.int32)):
        if isinstance(t, torch.Tensor) and t.dtype != dt:      # (no silent conversion)
            raise _lib.PznError(f"{who}: {name} must be {dt}; got {t.dtype}")
    score, T = _f32(score, "score"), _f32(T, "T")
    if score.dim() != 3 or score.shape[1] != score.shape[2]:
        raise _lib.PznError(f"{who}: expected score[Z,K,K]; got {tuple(score.shape)}")
    Z, K = score.shape[0], score.shape[1]
    if tuple(T.shape) != (Z, K, K, 4, 4):
        raise _lib.PznError(f"{who}: expected T[{Z},{K},{K},4,4]; got {tuple(T.shape)}")
    if count is not None:
        count = _req(count, torch.int32, "count")
        if tuple(count.shape) != (Z,):
            raise _lib.PznError(f"{who}: expected count[{Z}]; got {tuple(count.shape)}")
    max_score = float("inf") if max_score is None else float(max_score)
    joint_score = float("nan") if joint_score is None else float(joint_score)
    if max_score != max_score:
        raise _lib.PznError(f"{who}: max_score is NaN (None: no limit)")
    return score, T, count, max_score, joint_score, Z, K


def _walk_outputs(Z, K, dev):
    """-> (root, edges, edge_score, n_edges, G, placed, joints, n_joints), not initialised."""
    i32 = dict(dtype=torch.int32, device=dev)
    root, n_edges, n_joints = (torch.empty((Z,), **i32) for _ in range(3))
    edges = torch.empty((Z, K - 1, 3), **i32)
    edge_score = torch.empty((Z, K - 1), dtype=torch.float32, device=dev)
    G = torch.empty((Z, K, 4, 4), dtype=torch.float64, device=dev)
    placed = torch.empty((Z, K), dtype=torch.uint8, device=dev)
    joints = torch.empty((Z, K * (K - 1), 2), **i32)
    return root, edges, edge_score, n_edges, G, placed, joints, n_joints


def assemble_walk(score, T, count=None, max_score=None, joint_score=None):
    """The greedy walk over Z pair tables and every walk's joint list in one launch (pzn_assemble_walk_f32; include/pzn.h states
    the rule, assembly.walk_rule is its numpy statement): score [Z,K,K] float32, T [Z,K,K,4,4] float32 (T[z,i,j] maps piece j into
    piece i's frame), count [Z] int32 (the pieces of every puzzle; None: K; a count outside [2, K] gives root -1 and nothing
    else), max_score (None: the walk stops only at a key that is not finite), joint_score (None: every puzzle's largest edge
    score) -> (root [Z] int32, edges [Z,K-1,3] int32 rows (i, j, new), edge_score [Z,K-1] float32, n_edges [Z] int32,
    G [Z,K,4,4] float64, placed [Z,K] uint8, joints [Z,K(K-1),2] int32, n_joints [Z] int32); unused edge rows are -1 with a score
    of +inf, unused joint rows (-1, -1).  2 <= K <= 64 (PznUnsupported beyond).  Z = 0 launches nothing.  No autograd, nothing
    waits for the device."""
    score, T, count, max_score, joint_score, Z, K = _walk_args("assemble_walk", score, T, count, max_score, joint_score)
    if not assemble_walk_supported(K):
        raise _lib.PznUnsupported(f"assemble_walk: K = {K} pieces (2 <= K <= 64)")
    out = root, edges, edge_score, n_edges, G, placed, joints, n_joints = _walk_outputs(Z, K, score.device)
    with _on(score.device):
        _call("pzn_assemble_walk_f32", _p(score), _p(T), _p(count), max_score, joint_score, Z, K, _p(root), _p(edges), _p(edge_score),
              _p(n_edges), _p(G), _p(placed), _p(joints), _p(n_joints), _stream())
    return out


def _forest_outputs(Z, K, dev):
    """What the forest walks add to _walk_outputs -> (component [Z,K], roots [Z,K], n_components [Z]) int32, not initialised."""
    component, roots = (torch.empty((Z, K), dtype=torch.int32, device=dev) for _ in range(2))
    return component, roots, torch.empty((Z,), dtype=torch.int32, device=dev)


def assemble_forest_supported(K):
    return bool(_lib.load().pzn_assemble_forest_supported(int(K)))


def assemble_forest(score, T, count=None, max_score=None, joint_score=None):
    """The forest walk over Z pair tables - a pile of pieces of several objects sorted into components, each assembled in its own
    root's frame - and every component's joints in one launch (pzn_assemble_forest_f32; include/pzn.h states the rule,
    assembly.forest_rule is its numpy statement): the arguments are assemble_walk's -> its eight outputs in its shapes and types
    (root = roots[:, 0]; edges over all components in placement order; placed is 1 for every piece < count; joints never cross
    components), then component [Z,K] int32 (-1 at and beyond count), roots [Z,K] int32 (the root of component q, unused -1) and
    n_components [Z] int32.  2 <= K <= 64 (PznUnsupported beyond).  Z = 0 launches nothing.  No autograd, nothing waits for the
    device."""
    score, T, count, max_score, joint_score, Z, K = _walk_args("assemble_forest", score, T, count, max_score, joint_score)
    if not assemble_forest_supported(K):
        raise _lib.PznUnsupported(f"assemble_forest: K = {K} pieces (2 <= K <= 64)")
    out = root, edges, edge_score, n_edges, G, placed, joints, n_joints, component, roots, n_components = \
        _walk_outputs(Z, K, score.device) + _forest_outputs(Z, K, score.device)
    with _on(score.device):
        _call("pzn_assemble_forest_f32", _p(score), _p(T), _p(count), max_score, joint_score, Z, K, _p(root), _p(edges),
              _p(edge_score), _p(n_edges), _p(G), _p(placed), _p(joints), _p(n_joints), _p(component), _p(roots), _p(n_components),
              _stream())
    return out


def _beam_args(who, supported, score, T, moment, count, beam, branch, weight, max_score, vote_score, joint_score):
    """What the beam walks take alike, checked (`supported`: the caller's own test) -> (score, T, moment, count, beam, branch,
    weight, max_score, vote_score, joint_score, Z, K) as the library takes them: no vote_score is NaN."""
    if isinstance(moment, torch.Tensor) and moment.dtype != torch.float64:      # (no silent conversion)
        raise _lib.PznError(f"{who}: moment must be {torch.float64}; got {moment.dtype}")
    score, T, count, max_score, joint_score, Z, K = _walk_args(who, score, T, count, max_score, joint_score)
    moment = _req(moment, torch.float64, "moment")
    if tuple(moment.shape) != (Z, K, 4, 4):
        raise _lib.PznError(f"{who}: expected moment[{Z},{K},4,4]; got {tuple(moment.shape)}")
    beam, branch, weight = int(beam), int(branch), float(weight)
    vote_score = float("nan") if vote_score is None else float(vote_score)
    if weight != weight:
        raise _lib.PznError(f"{who}: weight is NaN")
    if not supported(K, beam, branch):
        raise _lib.PznUnsupported(f"{who}: K = {K} pieces, beam = {beam}, branch = {branch} (2 <= K <= 64, 1 <= beam, branch <= 8)")
    return score, T, moment, count, beam, branch, weight, max_score, vote_score, joint_score, Z, K


def _beam_outputs(Z, beam, dev):
    """-> (cost [Z,beam] float64, n_hyp [Z] int32), not initialised."""
    return torch.empty((Z, beam), dtype=torch.float64, device=dev), torch.empty((Z,), dtype=torch.int32, device=dev)


def assemble_beam_supported(K, beam=4, branch=4):
    return bool(_lib.load().pzn_assemble_beam_supported(int(K), int(beam), int(branch)))


def assemble_beam(score, T, moment, count=None, beam=4, branch=4, weight=1.0, max_score=None, vote_score=None, joint_score=None):
    """The beam walk over Z pair tables, scored by the placed pieces' votes, in one launch (pzn_assemble_beam_f32; include/pzn.h
    states the rule, assembly.beam_rule is its numpy statement): score, T, count, max_score and joint_score as assemble_walk takes
    them, moment [Z,K,4,4] float64 (assembly.boundary_moments), beam and branch in 1 .. 8, weight (not NaN), vote_score (None:
    max_score) -> assemble_walk's eight outputs for the cheapest hypothesis, then cost [Z,beam] float64 (slot order, unused
    +inf) and n_hyp [Z] int32.  2 <= K <= 64 (PznUnsupported beyond).  Z = 0 launches nothing.  No autograd, nothing waits
    for the device."""
    score, T, moment, count, beam, branch, weight, max_score, vote_score, joint_score, Z, K = _beam_args(
        "assemble_beam", assemble_beam_supported, score, T, moment, count, beam, branch, weight, max_score, vote_score, joint_score)
    out = root, edges, edge_score, n_edges, G, placed, joints, n_joints, cost, n_hyp = \
        _walk_outputs(Z, K, score.device) + _beam_outputs(Z, beam, score.device)
    with _on(score.device):
        _call("pzn_assemble_beam_f32", _p(score), _p(T), _p(moment), _p(count), beam, branch, weight, max_score, vote_score,
              joint_score, Z, K, _p(root), _p(edges), _p(edge_score), _p(n_edges), _p(G), _p(placed), _p(joints), _p(n_joints),
              _p(cost), _p(n_hyp), _stream())
    return out


def assemble_forest_beam_supported(K, beam=4, branch=4):
    return bool(_lib.load().pzn_assemble_forest_beam_supported(int(K), int(beam), int(branch)))


def assemble_forest_beam(score, T, moment, count=None, beam=4, branch=4, weight=1.0, max_score=None, vote_score=None,
                         joint_score=None, restart_cost=None):
    """The forest beam over Z pair tables - the beam walk scored by the placed pieces' votes, with the forest walk's restarts - in
    one launch (pzn_assemble_forest_beam_f32; include/pzn.h states the rule, assembly.forest_beam_rule is its numpy statement): the
    arguments are assemble_beam's and restart_cost, what a new component costs (None or NaN: max_score where that is finite, else
    0) -> assemble_forest's eleven outputs for the cheapest hypothesis, then cost [Z,beam] float64 (slot order, unused +inf) and
    n_hyp [Z] int32.  2 <= K <= 64, beam and branch in 1 .. 8 (PznUnsupported beyond).  Z = 0 launches nothing.  No autograd,
    nothing waits for the device."""
    score, T, moment, count, beam, branch, weight, max_score, vote_score, joint_score, Z, K = _beam_args(
        "assemble_forest_beam", assemble_forest_beam_supported, score, T, moment, count, beam, branch, weight, max_score, vote_score,
        joint_score)
    restart_cost = float("nan") if restart_cost is None else float(restart_cost)
    dev = score.device
    out = root, edges, edge_score, n_edges, G, placed, joints, n_joints, component, roots, n_components, cost, n_hyp = \
        _walk_outputs(Z, K, dev) + _forest_outputs(Z, K, dev) + _beam_outputs(Z, beam, dev)
    with _on(dev):
        _call("pzn_assemble_forest_beam_f32", _p(score), _p(T), _p(moment), _p(count), beam, branch, weight, max_score, vote_score,
              joint_score, restart_cost, Z, K, _p(root), _p(edges), _p(edge_score), _p(n_edges), _p(G), _p(placed), _p(joints),
              _p(n_joints), _p(component), _p(roots), _p(n_components), _p(cost), _p(n_hyp), _stream())
    return out


ProgressiveState = collections.namedtuple("ProgressiveState", "alive part G done n_edges edges edge_score")
_PROGRESSIVE_TYPES = (torch.uint8, torch.int32, torch.float64, torch.uint8, torch.int32, torch.int32, torch.float32)


def progressive_round_supported(P):
    return bool(_lib.load().pzn_progressive_round_supported(int(P)))


def progressive_state(Z, P, device, count=None):
    """The fresh state of Z progressive walks over P slots (include/pzn.h, pzn_progressive_round_f32) -> ProgressiveState of
    device tensors: alive [Z,P] uint8 (1; 0 for the slots at or beyond count[z], count [Z] integers on the device or None), part
    [Z,P] int32 (part[p] = p), G [Z,P,4,4] float64 (identity), done [Z] uint8 (0), n_edges [Z] int32 (0), edges [Z,P-1,4] int32
    (-1), edge_score [Z,P-1] float32 (+inf).  Nothing waits for the device."""
    Z, P = int(Z), int(P)
    slot = torch.arange(P, dtype=torch.int32, device=device)
    if count is None:
        alive = torch.ones((Z, P), dtype=torch.uint8, device=device)
    else:
        if not isinstance(count, torch.Tensor) or not count.is_cuda or tuple(count.shape) != (Z,) or count.dtype.is_floating_point:
            raise _lib.PznError(f"progressive_state: count must be an integer tensor [{Z}] on the GPU")
        alive = (slot[None, :] < count[:, None]).to(torch.uint8)
    return ProgressiveState(alive, slot[None, :].repeat(Z, 1), torch.eye(4, dtype=torch.float64, device=device).repeat(Z, P, 1, 1),
                            torch.zeros((Z,), dtype=torch.uint8, device=device), torch.zeros((Z,), dtype=torch.int32, device=device),
                            torch.full((Z, max(P - 1, 0), 4), -1, dtype=torch.int32, device=device),
                            torch.full((Z, max(P - 1, 0)), float("inf"), dtype=torch.float32, device=device))


def progressive_round(score, T, state, max_score=None):
    """One round of Z progressive walks in one launch (pzn_progressive_round_f32; include/pzn.h states the rule,
    assembly.progressive_round_rule is its numpy statement): score [Z,P,P] float32, T [Z,P,P,4,4] float32 (T[z,i,j] maps the part
    in slot j into slot i's frame), state = a ProgressiveState of contiguous device tensors in its own types (progressive_state
    makes one), which is UPDATED IN PLACE, max_score (None: a walk stops only at a key that is not finite) -> (took [Z] uint8,
    pick [Z,2] int64): took = 1 and pick = (i, j) where puzzle z merged slot j into slot i, took = 0 and the safe pick (0, 0)
    where it stopped (its done is set and nothing else of its state has changed).  2 <= P <= 64 (PznUnsupported beyond).
    Z = 0 launches nothing.  No autograd, nothing waits for the device."""
    for name, t in (("score", score), ("T", T)):
        if isinstance(t, torch.Tensor) and t.dtype != torch.float32:      # (no silent conversion)
            raise _lib.PznError(f"progressive_round: {name} must be torch.float32; got {t.dtype}")
    score, T = _f32(score, "score"), _f32(T, "T")
    if score.dim() != 3 or score.shape[1] != score.shape[2]:
        raise _lib.PznError(f"progressive_round: expected score[Z,P,P]; got {tuple(score.shape)}")
    Z, P = score.shape[0], score.shape[1]
    if tuple(T.shape) != (Z, P, P, 4, 4):
        raise _lib.PznError(f"progressive_round: expected T[{Z},{P},{P},4,4]; got {tuple(T.shape)}")
    if not isinstance(state, ProgressiveState):
        raise _lib.PznError(f"progressive_round: state must be a ProgressiveState; got {type(state).__name__}")
    shapes = ((Z, P), (Z, P), (Z, P, 4, 4), (Z,), (Z,), (Z, max(P - 1, 0), 4), (Z, max(P - 1, 0)))
    for name, t, dt, shape in zip(ProgressiveState._fields, state, _PROGRESSIVE_TYPES, shapes):
        # the state is written in place: a converted or compacted copy would take the update with it
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.device != score.device or t.dtype != dt or tuple(t.shape) != shape \
                or not t.is_contiguous():
            raise _lib.PznError(f"progressive_round: state.{name} must be a contiguous {dt} tensor {list(shape)} on {score.device}; got "
                                f"{(t.dtype, tuple(t.shape), str(t.device)) if isinstance(t, torch.Tensor) else type(t).__name__}")
    max_score = float("inf") if max_score is None else float(max_score)
    if max_score != max_score:
        raise _lib.PznError("progressive_round: max_score is NaN (None: no limit)")
    if not progressive_round_supported(P):
        raise _lib.PznUnsupported(f"progressive_round: P = {P} slots (2 <= P <= 64)")
    dev = score.device
    took = torch.empty((Z,), dtype=torch.uint8, device=dev)
    pick = torch.empty((Z, 2), dtype=torch.int64, device=dev)
    if Z > 0:
        with _on(dev):
            s = state
            _call("pzn_progressive_round_f32", _p(score), _p(T), max_score, Z, P, _p(s.alive), _p(s.part), _p(s.G), _p(s.done),
                  _p(s.n_edges), _p(s.edges), _p(s.edge_score), _p(took), _p(pick), _stream())
    return took, pick


def progressive_joints_supported(P, k):
    return bool(_lib.load().pzn_progressive_joints_supported(int(P), int(k)))


def progressive_joints(pieces, G, dropped, least=3):
    """The pose graph of Z progressive walks read off their ledgers, one launch (pzn_progressive_joints_f32; include/pzn.h states
    the rule, assembly.progressive_joints_rule is its numpy statement): pieces [Z,P,N,3] float32 (the original pieces), G [Z,P,4,4]
    float64 (the ledger's poses), dropped [R,Z,2,k,2] int64 (per round and side - fixed, moved - the (piece, row) pairs a merge
    left out; entries outside the pieces and rows, such as -1, are skipped), least >= 1 (a joint needs that many points on either
    side) -> (joints [Z,J,2] int32 rows (p, q) with p the fixed piece, unused rows (-1, -1); a, b [Z,J,k,3] float32, the sets of a
    joint in their own piece's frame, zero behind the count; na, nb [Z,J] int32, 0 on an unused row; rows_a, rows_b [Z,J,k] int64,
    the rows in the piece, -1 behind the count), J = P (P - 1) / 2, row e of the pair {lo, hi} = hi (hi - 1) / 2 + lo.  With the
    sets viewed as [Z J,k,3] this is what joint_refine(..., na=, nb=) takes.  A tensor of another dtype is refused, not converted.
    2 <= P <= 64, 1 <= k <= 1024, R >= 1 (PznUnsupported beyond).  Z = 0 launches nothing.  No autograd, nothing waits for the
    device."""
    _no_conversion("progressive_joints", (("pieces", pieces, (torch.float32,)), ("G", G, (torch.float64,)),
                                          ("dropped", dropped, (torch.int64,))))
    pieces, G, dropped = _f32(pieces, "pieces"), _req(G, torch.float64, "G"), _i64(dropped, "dropped")
    if pieces.dim() != 4 or pieces.shape[3] != 3:
        raise _lib.PznError(f"progressive_joints: expected pieces[Z,P,N,3]; got {tuple(pieces.shape)}")
    Z, P, N, _ = pieces.shape
    if tuple(G.shape) != (Z, P, 4, 4):
        raise _lib.PznError(f"progressive_joints: expected G[{Z},{P},4,4]; got {tuple(G.shape)}")
    if dropped.dim() != 5 or dropped.shape[1] != Z or dropped.shape[2] != 2 or dropped.shape[4] != 2:
        raise _lib.PznError(f"progressive_joints: expected dropped[R,{Z},2,k,2]; got {tuple(dropped.shape)}")
    if isinstance(least, bool) or not isinstance(least, numbers.Integral) or least < 1:
        raise _lib.PznError(f"progressive_joints: least must be an integer >= 1; got {least!r}")
    R, k = dropped.shape[0], dropped.shape[3]
    if not progressive_joints_supported(P, k) or R < 1 or N < 1:
        raise _lib.PznUnsupported(f"progressive_joints: R = {R} rounds of P = {P} pieces of N = {N} rows, k = {k} entries a side "
                                  "(2 <= P <= 64, 1 <= k <= 1024, R >= 1, N >= 1)")
    dev = pieces.device
    J = P * (P - 1) // 2
    joints = torch.full((Z, J, 2), -1, dtype=torch.int32, device=dev)
    a = torch.zeros((Z, J, k, 3), dtype=torch.float32, device=dev)
    b = torch.zeros_like(a)
    na = torch.zeros((Z, J), dtype=torch.int32, device=dev)
    nb = torch.zeros_like(na)
    rows_a = torch.full((Z, J, k), -1, dtype=torch.int64, device=dev)
    rows_b = torch.full_like(rows_a, -1)
    if Z > 0:
        with _on(dev):
            _call("pzn_progressive_joints_f32", _p(pieces), _p(G), _p(dropped), R, Z, P, N, k, min(int(least), 1 << 30), _p(joints),
                  _p(a), _p(b), _p(na), _p(nb), _p(rows_a), _p(rows_b), _stream())
    return joints, a, b, na, nb, rows_a, rows_b


def knn(xyz, new_xyz, K):
    xyz, new_xyz = _f32(xyz, "xyz"), _f32(new_xyz, "new_xyz")
    B, N, _ = xyz.shape
    S = new_xyz.shape[1]
    out = torch.empty((B, S, K), dtype=torch.int64, device=xyz.device)
    with _on(xyz.device):
        _call("pzn_knn_f32", _p(xyz), _p(new_xyz), B, N, S, int(K), _p(out), _stream())
    return out


def ball_query(radius, nsample, xyz, new_xyz):
    xyz, new_xyz = _f32(xyz, "xyz"), _f32(new_xyz, "new_xyz")
    B, N, _ = xyz.shape
    S = new_xyz.shape[1]
    out = torch.empty((B, S, nsample), dtype=torch.int64, device=xyz.device)
    # `sqrdists > radius ** 2` is an fp32 comparison in the reference (pointnet_util.py:91)
    r2 = float(torch.tensor(float(radius) ** 2, dtype=torch.float32))
    with _on(xyz.device):
        _call("pzn_ball_query_f32", r2, int(nsample), _p(xyz), _p(new_xyz), B, N, S, _p(out), _stream())
    return out


class _Gather(torch.autograd.Function):
    """index_points (pointnet_util.py:39-50): forward gather, backward scatter-add."""

    @staticmethod
    def forward(ctx, points, idx):
        points = _f32(points, "points")
        idx = _i64(idx, "idx")
        B, N, C = points.shape
        flat = idx.reshape(B, -1)
        M = flat.shape[1]
        out = torch.empty((B, M, C), dtype=torch.float32, device=points.device)
        with _on(points.device):
            _call("pzn_gather_fwd_f32", _p(points), _p(flat), B, N, M, C, _p(out), _stream())
        ctx.save_for_backward(flat)
        ctx.dims = (B, N, M, C)
        return out.reshape(*idx.shape, C)

    @staticmethod
    def backward(ctx, grad_out):
        (flat,) = ctx.saved_tensors
        B, N, M, C = ctx.dims
        grad_out = _f32(grad_out, "grad_out")
        g = torch.zeros((B, N, C), dtype=torch.float32, device=grad_out.device)
        with _on(grad_out.device):
            _call("pzn_gather_bwd_f32", _p(grad_out), _p(flat), B, N, M, C, _p(g), _stream())
        return g, None


def index_points(points, idx):
    return _Gather.apply(points, idx)


class _MaxOverPoints(torch.autograd.Function):
    """torch.max(x, dim=1)[0] for x[B, L, C] (model5_b.py:475, :741): one pass forward (value + arg-max row), one
    streaming pass backward that writes every element of dx (no zero fill + scatter)."""

    @staticmethod
    def forward(ctx, x):
        x = _f32(x, "x")
        B, L, C = x.shape
        out = torch.empty((B, C), dtype=torch.float32, device=x.device)
        idx = torch.empty((B, C), dtype=torch.int32, device=x.device)
        with _on(x.device):
            _call("pzn_maxpool_points_fwd_f32", _p(x), B, L, C, _p(out), _p(idx), _stream())
        if WINNER_CAPTURE is not None:
            WINNER_CAPTURE.append(("maxpts", None, idx))
        ctx.save_for_backward(idx)
        ctx.dims = (B, L, C)
        return out

    @staticmethod
    def backward(ctx, dout):
        (idx,) = ctx.saved_tensors
        B, L, C = ctx.dims
        dout = _f32(dout, "dout")
        dx = torch.empty((B, L, C), dtype=torch.float32, device=dout.device)
        with _on(dout.device):
            _call("pzn_maxpool_points_bwd_f32", _p(dout), _p(idx), B, L, C, _p(dx), _stream())
        return dx


class _Se3Exp(torch.autograd.Function):
    """se3.exp (se_math/se3.py:57-80): twist [B,6] -> [B,4,4], one launch each way."""

    @staticmethod
    def forward(ctx, x):
        x = _f32(x, "twist")
        B = x.shape[0]
        g = torch.empty((B, 4, 4), dtype=torch.float32, device=x.device)
        with _on(x.device):
            _call("pzn_se3_exp_fwd_f32", _p(x), B, _p(g), _stream())
        ctx.save_for_backward(x)
        return g

    @staticmethod
    def backward(ctx, dg):
        (x,) = ctx.saved_tensors
        dg = _f32(dg, "dg")
        dx = torch.empty_like(x)
        with _on(x.device):
            _call("pzn_se3_exp_bwd_f32", _p(x), _p(dg), x.shape[0], _p(dx), _stream())
        return dx


class _Se3Transform(torch.autograd.Function):
    """se3.transform (se_math/se3.py:110-120) on points: out[b,n,:] = R_b p[b,n,:] + t_b, one launch each way."""

    @staticmethod
    def forward(ctx, g, p):
        g, p = _f32(g, "g"), _f32(p, "points")
        B, N, _ = p.shape
        out = torch.empty_like(p)
        with _on(p.device):
            _call("pzn_se3_transform_fwd_f32", _p(g), _p(p), B, N, _p(out), _stream())
        ctx.save_for_backward(g, p)
        return out

    @staticmethod
    def backward(ctx, dout):
        g, p = ctx.saved_tensors
        B, N, _ = p.shape
        dout = _f32(dout, "dout")
        dg = torch.empty_like(g) if ctx.needs_input_grad[0] else None
        dp = torch.empty_like(p) if ctx.needs_input_grad[1] else None
        if dg is None and dp is None:
            return None, None
        with _on(p.device):
            _call("pzn_se3_transform_bwd_f32", _p(g), _p(p), _p(dout), B, N, _p(dp), _p(dg), _stream())
        return dg, dp


def se3_transform_points(g, p):
    """g [B,4,4], p [B,N,3] on the GPU -> [B,N,3]"""
    if g.dim() != 3 or p.dim() != 3 or g.shape[0] != p.shape[0] or p.shape[2] != 3 or tuple(g.shape[1:]) != (4, 4):
        raise _lib.PznError(f"se3_transform_points expects g[B,4,4], p[B,N,3]; got {tuple(g.shape)}, {tuple(p.shape)}")
    return _Se3Transform.apply(g, p)


class _CompLoss(torch.autograd.Function):
    """TouchedRegraster.comp (model5_b.py:1512-1519): 16 * mean((g igt - I)^2), one launch each way."""

    @staticmethod
    def forward(ctx, g, igt):
        g, igt = _f32(g, "g"), _f32(igt, "igt")
        loss = torch.empty((1,), dtype=torch.float32, device=g.device)
        with _on(g.device):
            _call("pzn_comp_fwd_f32", _p(g), _p(igt), g.shape[0], _p(loss), _stream())
        ctx.save_for_backward(g, igt)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, dloss):
        g, igt = ctx.saved_tensors
        dl = _f32(dloss, "dloss").reshape(1)
        dg = torch.empty_like(g)
        with _on(g.device):
            _call("pzn_comp_bwd_f32", _p(g), _p(igt), _p(dl), g.shape[0], _p(dg), _stream())
        return dg, None


def comp_loss(g, igt):
    return _CompLoss.apply(g, igt)


class _BoundaryCE(torch.autograd.Function):
    """F.cross_entropy(logits[B,2,N], labels[B,N]) (model5_b.py:1063-1064) together with softmax(logits, 1)[:, 1, :]
    (:1085-1090) -> (loss, prob1); prob1 only feeds the (non-differentiable) top-128 selection."""

    @staticmethod
    def forward(ctx, logits, labels):
        labels = _f32(labels, "labels")
        if not isinstance(logits, torch.Tensor) or logits.dim() != 3:
            raise _lib.PznError("boundary_ce expects logits[B,2,N]")
        B, C, N = logits.shape
        # the heads' [B,N,2] output seen through permute(0,2,1) (model5_b.py:751-754) is read through its strides: no transposed
        # copy here, and the gradient goes back in the same layout (contiguous for the heads' backward)
        pm = logits.is_cuda and logits.dtype == torch.float32 and C == 2 and logits.stride() == (2 * N, 1, 2)
        if not pm:
            logits = _f32(logits, "logits")
        if C != 2 or tuple(labels.shape) != (B, N):
            raise _lib.PznError(f"boundary_ce expects logits[B,2,N], labels[B,N]; got {tuple(logits.shape)}, {tuple(labels.shape)}")
        prob1 = torch.empty((B, N), dtype=torch.float32, device=logits.device)
        loss = torch.empty((_lib.CONSTANTS["PZN_BOUNDARY_CE_LOSS_FLOATS"],), dtype=torch.float32,      # value + partials
                           device=logits.device)
        with _on(logits.device):
            _call("pzn_boundary_ce_fwd_f32", _p(logits), _p(labels), B, N, int(pm), _p(prob1), _p(loss), _stream())
        ctx.save_for_backward(logits, labels)
        ctx.points_major = pm
        ctx.mark_non_differentiable(prob1)
        ctx.set_materialize_grads(False)      # (prob1 carries no gradient: no zero-filled [B,N] stand-in for it)
        return loss[0], prob1

    @staticmethod
    def backward(ctx, dloss, _dprob):
        logits, labels = ctx.saved_tensors
        if dloss is None:
            return None, None
        B, _, N = logits.shape
        dl = _f32(dloss, "dloss").reshape(1)
        pm = ctx.points_major
        dlogits = torch.empty((B, N, 2), dtype=torch.float32, device=logits.device).permute(0, 2, 1) if pm else torch.empty_like(logits)
        with _on(logits.device):
            _call("pzn_boundary_ce_bwd_f32", _p(logits), _p(labels), _p(dl), B, N, int(pm), _p(dlogits), _stream())
        return dlogits, None


def boundary_ce(logits, labels):
    """-> (cross-entropy loss, class-1 probability [B,N])"""
    return _BoundaryCE.apply(logits, labels)


def topk_rows(x, k):
    """torch.topk(x, k, dim=1)[1] for x[R,N] on the GPU (value descending, ties by ascending index)."""
    x = _f32(x.detach(), "x")
    R, N = x.shape
    idx = torch.empty((R, int(k)), dtype=torch.int64, device=x.device)
    with _on(x.device):
        _call("pzn_topk_rows_f32", _p(x), R, N, int(k), _p(idx), _stream())
    return idx


def _cut_outputs(raw, P, cap):
    """What every cut launch writes for P pieces per sample: pieces [P B,cap,3] f32, counts [P B] and start [P B] int64, ok [B] uint8."""
    B, dev = raw.shape[0], raw.device
    return (torch.empty((P * B, int(cap), 3), dtype=torch.float32, device=dev), torch.empty((P * B,), dtype=torch.int64, device=dev),
            torch.empty((P * B,), dtype=torch.int64, device=dev), torch.empty((B,), dtype=torch.uint8, device=dev))


def cut_compact(raw, normals, zs, u, n_min, cap):
    """dataset.py:761-775 + 1176-1180 for a batch in one launch (pzn_cut_compact_f32): raw [B,M,3] f32, K candidate planes per
    sample (normals [B,K,3], zs [B,K], float64), start fractions u [B,2] float64
    -> (pieces [2B,cap,3]: up pieces then down pieces, counts [2B] int64, start [2B] int64, plane [B,4] float64, ok [B] bool)"""
    raw = _f32(raw, "raw")
    normals, zs, u = (_req(t, torch.float64, n_) for t, n_ in ((normals, "normals"), (zs, "zs"), (u, "u")))
    B, M, _ = raw.shape
    K = normals.shape[1]
    dev = raw.device
    pieces, counts, start, ok = _cut_outputs(raw, 2, cap)
    plane = torch.empty((B, 4), dtype=torch.float64, device=dev)
    with _on(dev):
        _call("pzn_cut_compact_f32", _p(raw), _p(normals), _p(zs), _p(u), B, M, K, int(n_min), int(cap), _p(pieces), _p(counts),
              _p(start), _p(plane), _p(ok), _stream())
    return pieces, counts, start, plane, ok.to(torch.bool)


SOLID_KINDS = ("sphere", "cylinder", "cone")      # the `kind` codes of pzn_cut_compact_solid_f32


def cut_compact_solid(raw, kind, params, u, n_min, cap):
    """dataset.py:715-759 + 1175-1179 for a batch in one launch (pzn_cut_compact_solid_f32): raw [B,M,3] f32, kind "sphere" |
    "cylinder" | "cone", K candidate solids per sample (params [B,K,6] float64: rot, shift), start fractions u [B,2] float64
    -> (pieces [2B,cap,3]: up (inside) pieces then down pieces, counts [2B] int64, start [2B] int64, chosen [B,6] float64,
        chosen_k [B] int32, ok [B] bool)"""
    if kind not in SOLID_KINDS:
        raise _lib.PznError(f"cut_compact_solid: unknown solid {kind!r} (one of {SOLID_KINDS})")
    raw = _f32(raw, "raw")
    params, u = _req(params, torch.float64, "params"), _req(u, torch.float64, "u")
    B, M, _ = raw.shape
    if params.dim() != 3 or params.shape[0] != B or params.shape[2] != 6 or tuple(u.shape) != (B, 2):
        raise _lib.PznError("cut_compact_solid: params as [B, K, 6] and u as [B, 2]")
    K = params.shape[1]
    dev = raw.device
    pieces, counts, start, ok = _cut_outputs(raw, 2, cap)
    chosen = torch.empty((B, 6), dtype=torch.float64, device=dev)
    chosen_k = torch.empty((B,), dtype=torch.int32, device=dev)
    with _on(dev):
        _call("pzn_cut_compact_solid_f32", _p(raw), SOLID_KINDS.index(kind), _p(params), _p(u), B, M, K, int(n_min), int(cap),
              _p(pieces), _p(counts), _p(start), _p(chosen), _p(chosen_k), _p(ok), _stream())
    return pieces, counts, start, chosen, chosen_k, ok.to(torch.bool)


DOUBLE_CUT_KINDS = ("single", "half_vs_rest", "half_vs_other", "halves")      # the `kind` codes of pzn_cut_compact_double_f32
DOUBLE_CUT_TRIES = 7      # plane-2 candidates per sample: the first draw + the re-draws of `while time <= 5` (dataset.py:1227)
DOUBLE_CUT_UNIFORMS = 7   # u_seed, u_se, u_choice, u_sU, u_sD, u_sFU, u_sFD


def cut_compact_double(raw, normals1, zs1, normals2, zs2, u, n_min, n_rich, cap):
    """dataset.py:1203-1355 (split_twice=True) up to the sampling for a batch in one launch (pzn_cut_compact_double_f32; the
    rule: datapipe.double_cut_rule): raw [B,M,3] f32; K candidates for plane 1 (normals1 [B,K,3], zs1 [B,K]), 7 for plane 2
    (normals2 [B,7,3], zs2 [B,7]), uniforms u [B,7], all float64
    -> (pieces [4B,cap,3]: U, D, fallback U, fallback D; counts [4B] int64, -1 where there is no fallback; start [4B] int64;
        kind [B] int32; planes [B,2,4] float64; tabs [B,4] int32; ok [B] bool)"""
    raw = _f32(raw, "raw")
    normals1, zs1, normals2, zs2, u = (_req(t, torch.float64, n_) for t, n_ in (
        (normals1, "normals1"), (zs1, "zs1"), (normals2, "normals2"), (zs2, "zs2"), (u, "u")))
    B, M, _ = raw.shape
    if normals1.dim() != 3 or normals1.shape[0] != B or normals1.shape[2] != 3 or tuple(zs1.shape) != (B, normals1.shape[1]):
        raise _lib.PznError("cut_compact_double: normals1 as [B, K, 3] and zs1 as [B, K]")
    if tuple(normals2.shape) != (B, DOUBLE_CUT_TRIES, 3) or tuple(zs2.shape) != (B, DOUBLE_CUT_TRIES) \
            or tuple(u.shape) != (B, DOUBLE_CUT_UNIFORMS):
        raise _lib.PznError(f"cut_compact_double: normals2 as [B, {DOUBLE_CUT_TRIES}, 3], zs2 as [B, {DOUBLE_CUT_TRIES}] and "
                            f"u as [B, {DOUBLE_CUT_UNIFORMS}]")
    K = normals1.shape[1]
    dev = raw.device
    pieces, counts, start, ok = _cut_outputs(raw, 4, cap)
    kind = torch.empty((B,), dtype=torch.int32, device=dev)
    planes = torch.empty((B, 2, 4), dtype=torch.float64, device=dev)
    tabs = torch.empty((B, 4), dtype=torch.int32, device=dev)
    with _on(dev):
        _call("pzn_cut_compact_double_f32", _p(raw), _p(normals1), _p(zs1), _p(normals2), _p(zs2), _p(u), B, M, K, int(n_min),
              int(n_rich), int(cap), _p(pieces), _p(counts), _p(start), _p(kind), _p(planes), _p(tabs), _p(ok), _stream())
    return pieces, counts, start, kind, planes, tabs, ok.to(torch.bool)


def fracture_supported(M, P, K):
    return bool(_lib.load().pzn_fracture_supported(int(M), int(P), int(K)))


def fracture(raw, normals, u_anchor, u_start, n_min, cap):
    """Every cloud of a batch cut into P pieces in one launch (pzn_fracture_f32; the rule: datapipe.fracture_rule): raw [B,M,3]
    f32; K candidate normals per cut (normals [B,P-1,K,3]), their anchor draws (u_anchor [B,P-1,K]) and the start fractions
    (u_start [B,P]), all float64 (no silent conversion: PznError)
    -> (pieces [P B,cap,3]: piece p of sample b at row p B + b; counts [P B] int64; start [P B] int64; label [B,M] uint8;
        order [B,M] int32; planes [B,P-1,4] float64; target [B,P-1] int32; cand [B,P-1] int32; ok [B] bool)
    2 <= P <= 16, K >= 1, M <= 65536 (PznUnsupported beyond).  Nothing waits for the device."""
    for name, t, dt in (("raw", raw, torch.float32), ("normals", normals, torch.float64), ("u_anchor", u_anchor, torch.float64),
                        ("u_start", u_start, torch.float64)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise _lib.PznError(f"fracture: {name} must be a tensor on the GPU; puzzlenet_amd has no CPU fallback")
        if t.dtype != dt:
            raise _lib.PznError(f"fracture: {name} must be {dt}; got {t.dtype}")
    if raw.dim() != 3 or raw.shape[2] != 3 or raw.shape[0] == 0 or raw.shape[1] == 0:
        raise _lib.PznError(f"fracture: raw as [B, M, 3]; got {tuple(raw.shape)}")
    B, M, _ = raw.shape
    if u_start.dim() != 2 or u_start.shape[0] != B:
        raise _lib.PznError(f"fracture: u_start as [B, P]; got {tuple(u_start.shape)}")
    P = u_start.shape[1]
    K = normals.shape[2] if normals.dim() == 4 else 0
    if not fracture_supported(M, P, max(K, 1)):
        raise _lib.PznUnsupported(f"fracture: M = {M} points into P = {P} pieces (2 <= P <= 16, M <= 65536)")
    if normals.dim() != 4 or tuple(normals.shape) != (B, P - 1, K, 3) or K < 1 or tuple(u_anchor.shape) != (B, P - 1, K):
        raise _lib.PznError(f"fracture: normals as [B, P - 1, K, 3] and u_anchor as [B, P - 1, K] with P = {P}, K >= 1; got "
                            f"{tuple(normals.shape)}, {tuple(u_anchor.shape)}")
    cap, n_min = int(cap), int(n_min)
    if cap < 1 or n_min < 0:
        raise _lib.PznError(f"fracture: cap = {cap}, n_min = {n_min}")
    raw, normals, u_anchor, u_start = raw.contiguous(), normals.contiguous(), u_anchor.contiguous(), u_start.contiguous()
    dev = raw.device
    pieces, counts, start, ok = _cut_outputs(raw, P, cap)
    label = torch.empty((B, M), dtype=torch.uint8, device=dev)
    order = torch.empty((B, M), dtype=torch.int32, device=dev)
    planes = torch.empty((B, P - 1, 4), dtype=torch.float64, device=dev)
    target = torch.empty((B, P - 1), dtype=torch.int32, device=dev)
    cand = torch.empty((B, P - 1), dtype=torch.int32, device=dev)
    with _on(dev):
        _call("pzn_fracture_f32", _p(raw), _p(normals), _p(u_anchor), _p(u_start), B, M, P, K, n_min, cap, _p(pieces),
              _p(counts), _p(start), _p(label), _p(order), _p(planes), _p(target), _p(cand), _p(ok), _stream())
    return pieces, counts, start, label, order, planes, target, cand, ok.to(torch.bool)


def fracture_curved_supported(M, P, K):
    return bool(_lib.load().pzn_fracture_curved_supported(int(M), int(P), int(K)))


def _curved_cut_args(who, supported, raw, frames, half_curv, u_anchor, last, cap, n_min):
    """The argument checks the two curved fracture forms share (those of fracture / fracture_pair): raw f32 [B,M,3]; frames
    [B,P-1,K,3,3], half_curv [B,P-1,K,2], u_anchor [B,P-1,K] and `last` = (name, tensor, columns or None: P) float64 [B,columns],
    all on the GPU.  -> (B, M, P, K)"""
    for name, t, dt in (("raw", raw, torch.float32), ("frames", frames, torch.float64), ("half_curv", half_curv, torch.float64),
                        ("u_anchor", u_anchor, torch.float64), (last[0], last[1], torch.float64)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise _lib.PznError(f"{who}: {name} must be a tensor on the GPU; puzzlenet_amd has no CPU fallback")
        if t.dtype != dt:
            raise _lib.PznError(f"{who}: {name} must be {dt}; got {t.dtype}")
    if raw.dim() != 3 or raw.shape[2] != 3 or raw.shape[0] == 0 or raw.shape[1] == 0:
        raise _lib.PznError(f"{who}: raw as [B, M, 3]; got {tuple(raw.shape)}")
    B, M, _ = raw.shape
    if frames.dim() != 5 or frames.shape[0] != B or tuple(frames.shape[3:]) != (3, 3):
        raise _lib.PznError(f"{who}: frames as [B, P - 1, K, 3, 3]; got {tuple(frames.shape)}")
    P, K = frames.shape[1] + 1, frames.shape[2]
    if not supported(M, P, max(K, 1)):
        raise _lib.PznUnsupported(f"{who}: M = {M} points into P = {P} pieces (2 <= P <= 16, M <= 65536)")
    name, t, cols = last
    cols = P if cols is None else cols
    if K < 1 or tuple(half_curv.shape) != (B, P - 1, K, 2) or tuple(u_anchor.shape) != (B, P - 1, K) or tuple(t.shape) != (B, cols):
        raise _lib.PznError(f"{who}: half_curv as [B, P - 1, K, 2], u_anchor as [B, P - 1, K] with P = {P}, K >= 1, and {name} as "
                            f"[B, {cols}]; got {tuple(half_curv.shape)}, {tuple(u_anchor.shape)}, {tuple(t.shape)}")
    if int(cap) < 1 or int(n_min) < 0:
        raise _lib.PznError(f"{who}: cap = {cap}, n_min = {n_min}")
    return B, M, P, K


def fracture_curved(raw, frames, half_curv, u_anchor, u_start, n_min, cap):
    """ops.fracture along curved surfaces, one launch (pzn_fracture_curved_f32; the rule: datapipe.fracture_curved_rule): candidate
    k of a cut is the paraboloid through the anchor in the frame frames[b,s-1,k] (rows e1, e2, n; [B,P-1,K,3,3]) with the half
    curvatures half_curv[b,s-1,k] ([B,P-1,K,2]), both float64 and taken as given (no silent conversion: PznError)
    -> (pieces, counts, start, label, order, planes, target, cand as ops.fracture returns them, planes [B,P-1,4] the TANGENT
        plane at the anchor; anchor [B,P-1] int32, the cloud row of the anchor taken; ok [B] bool)
    2 <= P <= 16, K >= 1, M <= 65536 (PznUnsupported beyond).  Nothing waits for the device."""
    B, M, P, K = _curved_cut_args("fracture_curved", fracture_curved_supported, raw, frames, half_curv, u_anchor,
                                  ("u_start", u_start, None), cap, n_min)
    cap, n_min = int(cap), int(n_min)
    raw, frames, half_curv, u_anchor, u_start = (t.contiguous() for t in (raw, frames, half_curv, u_anchor, u_start))
    dev = raw.device
    pieces, counts, start, ok = _cut_outputs(raw, P, cap)
    label = torch.empty((B, M), dtype=torch.uint8, device=dev)
    order = torch.empty((B, M), dtype=torch.int32, device=dev)
    planes = torch.empty((B, P - 1, 4), dtype=torch.float64, device=dev)
    target = torch.empty((B, P - 1), dtype=torch.int32, device=dev)
    cand = torch.empty((B, P - 1), dtype=torch.int32, device=dev)
    anchor = torch.empty((B, P - 1), dtype=torch.int32, device=dev)
    with _on(dev):
        _call("pzn_fracture_curved_f32", _p(raw), _p(frames), _p(half_curv), _p(u_anchor), _p(u_start), B, M, P, K, n_min, cap,
              _p(pieces), _p(counts), _p(start), _p(label), _p(order), _p(planes), _p(target), _p(cand), _p(anchor), _p(ok),
              _stream())
    return pieces, counts, start, label, order, planes, target, cand, anchor, ok.to(torch.bool)


FRACTURE_PAIR_KINDS = ("sibling", "neighbour")      # the `kind` codes of pzn_fracture_pair_f32
FRACTURE_PAIR_UNIFORMS = 7                          # u_kind, u_a, u_c, u_sU, u_sD, u_sFU, u_sFD


def fracture_pair_supported(M, P, K):
    return bool(_lib.load().pzn_fracture_pair_supported(int(M), int(P), int(K)))


def _pair_pieces(who, pieces, B, P, dev):
    """The number of pieces of every sample as the pair launches take it: an int32 tensor [B] on the GPU is passed on unread,
    anything else is checked on the host (2 <= P_b <= P) and uploaded."""
    if isinstance(pieces, torch.Tensor) and pieces.is_cuda:
        if pieces.dtype != torch.int32 or tuple(pieces.shape) != (B,):
            raise _lib.PznError(f"{who}: pieces on the GPU as int32 [B]; got {pieces.dtype} {tuple(pieces.shape)}")
        return pieces
    host = torch.as_tensor(pieces).reshape(-1)
    if host.numel() == 1:
        host = host.expand(B)
    if host.is_floating_point() or host.numel() != B or int(host.min()) < 2 or int(host.max()) > P:
        raise _lib.PznError(f"{who}: pieces as an integer or B = {B} integers in 2 .. P = {P}; got {pieces!r}")
    return host.to(torch.int32).to(dev)


def fracture_pair(raw, normals, u_anchor, pieces, u, n_min, neighbours, cap):
    """A training pair cut out of a fracture of every cloud of a batch in one launch (pzn_fracture_pair_f32; the rule:
    datapipe.fracture_pair_rule): raw [B,M,3] f32; normals [B,P-1,K,3], u_anchor [B,P-1,K], u [B,7], all float64 on the GPU (no
    silent conversion: PznError); pieces: the number of pieces P_b of every sample, 2 <= P_b <= P - an int, a sequence or a CPU
    tensor (checked here, PznError, before any launch) or an int32 tensor [B] on the GPU (nothing waits for the device: the
    launch itself refuses a sample out of range with kind -1, no pieces and ok = 0); neighbours in [0, 1]
    -> (pieces [4B,cap,3]: U, D, fallback U, fallback D; counts [4B] int64, -1 where there is no fallback; start [4B] int64;
        kind [B] int32; pair [B,4] int32; label [B,M] uint8; planes [B,P-1,4] float64; target, cand [B,P-1] int32; ok [B] bool)
    2 <= P <= 16, K >= 1, M <= 65536 (PznUnsupported beyond)."""
    for name, t, dt in (("raw", raw, torch.float32), ("normals", normals, torch.float64), ("u_anchor", u_anchor, torch.float64),
                        ("u", u, torch.float64)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise _lib.PznError(f"fracture_pair: {name} must be a tensor on the GPU; puzzlenet_amd has no CPU fallback")
        if t.dtype != dt:
            raise _lib.PznError(f"fracture_pair: {name} must be {dt}; got {t.dtype}")
    if raw.dim() != 3 or raw.shape[2] != 3 or raw.shape[0] == 0 or raw.shape[1] == 0:
        raise _lib.PznError(f"fracture_pair: raw as [B, M, 3]; got {tuple(raw.shape)}")
    B, M, _ = raw.shape
    if normals.dim() != 4 or normals.shape[0] != B or normals.shape[3] != 3:
        raise _lib.PznError(f"fracture_pair: normals as [B, P - 1, K, 3]; got {tuple(normals.shape)}")
    P, K = normals.shape[1] + 1, normals.shape[2]
    if not fracture_pair_supported(M, P, max(K, 1)):
        raise _lib.PznUnsupported(f"fracture_pair: M = {M} points into P = {P} pieces (2 <= P <= 16, M <= 65536)")
    if K < 1 or tuple(u_anchor.shape) != (B, P - 1, K) or tuple(u.shape) != (B, FRACTURE_PAIR_UNIFORMS):
        raise _lib.PznError(f"fracture_pair: u_anchor as [B, P - 1, K] with K >= 1 and u as [B, {FRACTURE_PAIR_UNIFORMS}]; got "
                            f"{tuple(u_anchor.shape)}, {tuple(u.shape)}")
    cap, n_min, neighbours = int(cap), int(n_min), float(neighbours)
    if cap < 1 or n_min < 0 or not 0.0 <= neighbours <= 1.0:
        raise _lib.PznError(f"fracture_pair: cap = {cap}, n_min = {n_min}, neighbours = {neighbours}")
    dev = raw.device
    pieces = _pair_pieces("fracture_pair", pieces, B, P, dev)
    raw, normals, u_anchor, pieces, u = (t.contiguous() for t in (raw, normals, u_anchor, pieces, u))
    out, counts, start, ok = _cut_outputs(raw, 4, cap)
    kind = torch.empty((B,), dtype=torch.int32, device=dev)
    pair = torch.empty((B, 4), dtype=torch.int32, device=dev)
    label = torch.empty((B, M), dtype=torch.uint8, device=dev)
    planes = torch.empty((B, P - 1, 4), dtype=torch.float64, device=dev)
    target = torch.empty((B, P - 1), dtype=torch.int32, device=dev)
    cand = torch.empty((B, P - 1), dtype=torch.int32, device=dev)
    with _on(dev):
        _call("pzn_fracture_pair_f32", _p(raw), _p(normals), _p(u_anchor), _p(pieces), _p(u), neighbours, B, M, P, K, n_min, cap,
              _p(out), _p(counts), _p(start), _p(kind), _p(pair), _p(label), _p(planes), _p(target), _p(cand), _p(ok), _stream())
    return out, counts, start, kind, pair, label, planes, target, cand, ok.to(torch.bool)


def fracture_pair_curved_supported(M, P, K):
    return bool(_lib.load().pzn_fracture_pair_curved_supported(int(M), int(P), int(K)))


def fracture_pair_curved(raw, frames, half_curv, u_anchor, pieces, u, n_min, neighbours, cap):
    """ops.fracture_pair along the curved surfaces of ops.fracture_curved, one launch (pzn_fracture_pair_curved_f32; the rule:
    datapipe.fracture_pair_curved_rule): frames [B,P-1,K,3,3] and half_curv [B,P-1,K,2] float64 in place of normals; pieces, u,
    neighbours as ops.fracture_pair takes them
    -> (pieces, counts, start, kind, pair, label, planes, target, cand as ops.fracture_pair returns them, planes the TANGENT
        planes; anchor [B,P-1] int32, zero where a step was not made; ok [B] bool)
    2 <= P <= 16, K >= 1, M <= 65536 (PznUnsupported beyond)."""
    B, M, P, K = _curved_cut_args("fracture_pair_curved", fracture_pair_curved_supported, raw, frames, half_curv, u_anchor,
                                  ("u", u, FRACTURE_PAIR_UNIFORMS), cap, n_min)
    cap, n_min, neighbours = int(cap), int(n_min), float(neighbours)
    if not 0.0 <= neighbours <= 1.0:
        raise _lib.PznError(f"fracture_pair_curved: neighbours = {neighbours}")
    dev = raw.device
    pieces = _pair_pieces("fracture_pair_curved", pieces, B, P, dev)
    raw, frames, half_curv, u_anchor, pieces, u = (t.contiguous() for t in (raw, frames, half_curv, u_anchor, pieces, u))
    out, counts, start, ok = _cut_outputs(raw, 4, cap)
    kind = torch.empty((B,), dtype=torch.int32, device=dev)
    pair = torch.empty((B, 4), dtype=torch.int32, device=dev)
    label = torch.empty((B, M), dtype=torch.uint8, device=dev)
    planes = torch.empty((B, P - 1, 4), dtype=torch.float64, device=dev)
    target = torch.empty((B, P - 1), dtype=torch.int32, device=dev)
    cand = torch.empty((B, P - 1), dtype=torch.int32, device=dev)
    anchor = torch.empty((B, P - 1), dtype=torch.int32, device=dev)
    with _on(dev):
        _call("pzn_fracture_pair_curved_f32", _p(raw), _p(frames), _p(half_curv), _p(u_anchor), _p(pieces), _p(u), neighbours, B, M,
              P, K, n_min, cap, _p(out), _p(counts), _p(start), _p(kind), _p(pair), _p(label), _p(planes), _p(target), _p(cand),
              _p(anchor), _p(ok), _stream())
    return out, counts, start, kind, pair, label, planes, target, cand, anchor, ok.to(torch.bool)


FRACTURE_LOST = 255                                 # the label of a point lost along an eroded cut (P <= 16 leaves it free)


def fracture_eroded_supported(M, P, K):
    return bool(_lib.load().pzn_fracture_eroded_supported(int(M), int(P), int(K)))


def fracture_pair_eroded_supported(M, P, K):
    return bool(_lib.load().pzn_fracture_pair_eroded_supported(int(M), int(P), int(K)))


def _eroded_cut_args(who, supported, raw, normals, frames, half_curv, u_anchor, last, erode, cap, n_min):
    """The argument checks of the two eroded fracture forms: those of their siblings without erosion - the plane forms' with
    normals [B,P-1,K,3], _curved_cut_args' with frames and half_curv and normals=None - and erode float64 [B,P-1,4] on the GPU.
    `last` as _curved_cut_args takes it.  -> (B, M, P, K, curved)"""
    if (frames is None) != (half_curv is None) or (normals is None) == (frames is None):
        raise _lib.PznError(f"{who}: normals (planes), or frames and half_curv with normals=None (surfaces)")
    if frames is not None:
        B, M, P, K = _curved_cut_args(who, supported, raw, frames, half_curv, u_anchor, last, cap, n_min)
    else:
        name, t, cols = last
        for nm, x, dt in (("raw", raw, torch.float32), ("normals", normals, torch.float64), ("u_anchor", u_anchor, torch.float64),
                          (name, t, torch.float64)):
            if not isinstance(x, torch.Tensor) or not x.is_cuda:
                raise _lib.PznError(f"{who}: {nm} must be a tensor on the GPU; puzzlenet_amd has no CPU fallback")
            if x.dtype != dt:
                raise _lib.PznError(f"{who}: {nm} must be {dt}; got {x.dtype}")
        if raw.dim() != 3 or raw.shape[2] != 3 or raw.shape[0] == 0 or raw.shape[1] == 0:
            raise _lib.PznError(f"{who}: raw as [B, M, 3]; got {tuple(raw.shape)}")
        B, M, _ = raw.shape
        if normals.dim() != 4 or normals.shape[0] != B or normals.shape[3] != 3:
            raise _lib.PznError(f"{who}: normals as [B, P - 1, K, 3]; got {tuple(normals.shape)}")
        P, K = normals.shape[1] + 1, normals.shape[2]
        if not supported(M, P, max(K, 1)):
            raise _lib.PznUnsupported(f"{who}: M = {M} points into P = {P} pieces (2 <= P <= 16, M <= 65536)")
        cols = P if cols is None else cols
        if K < 1 or tuple(u_anchor.shape) != (B, P - 1, K) or tuple(t.shape) != (B, cols):
            raise _lib.PznError(f"{who}: u_anchor as [B, P - 1, K] with P = {P}, K >= 1, and {name} as [B, {cols}]; got "
                                f"{tuple(u_anchor.shape)}, {tuple(t.shape)}")
        if int(cap) < 1 or int(n_min) < 0:
            raise _lib.PznError(f"{who}: cap = {cap}, n_min = {n_min}")
    if not isinstance(erode, torch.Tensor) or not erode.is_cuda:
        raise _lib.PznError(f"{who}: erode must be a tensor on the GPU; puzzlenet_amd has no CPU fallback")
    if erode.dtype != torch.float64 or tuple(erode.shape) != (B, P - 1, 4):
        raise _lib.PznError(f"{who}: erode as float64 [B, P - 1, 4] = (w_up, w_dn, depth, rho) per step; got {erode.dtype} "
                            f"{tuple(erode.shape)}")
    return B, M, P, K, frames is not None


def fracture_eroded(raw, normals, u_anchor, u_start, erode, n_min, cap, frames=None, half_curv=None):
    """ops.fracture (normals) or ops.fracture_curved (frames and half_curv, with normals=None) with EROSION, one launch
    (pzn_fracture_eroded_f32; the rule: datapipe.fracture_eroded_rule): at every cut the target's points close to the taken
    surface are lost - a band -w_dn < f < w_up and a chip -depth < f < depth within rho of the anchor, erode [B,P-1,4] float64 =
    (w_up, w_dn, depth, rho) per step, taken as given - and get label FRACTURE_LOST, in no piece
    -> (pieces, counts, start, label, order, planes, target, cand as the form without erosion returns them, counts without the
        lost points and their rows behind the last piece in order; anchor [B,P-1] int32, the cloud row of the anchor taken, for
        planes too; lost [B,P-1] int32, the points lost at every step; ok [B] bool)
    2 <= P <= 16, K >= 1, M <= 65536 (PznUnsupported beyond).  Nothing waits for the device."""
    B, M, P, K, curved = _eroded_cut_args("fracture_eroded", fracture_eroded_supported, raw, normals, frames, half_curv, u_anchor,
                                          ("u_start", u_start, None), erode, cap, n_min)
    cap, n_min = int(cap), int(n_min)
    raw, u_anchor, u_start, erode = (t.contiguous() for t in (raw, u_anchor, u_start, erode))
    cuts = (None, frames.contiguous(), half_curv.contiguous()) if curved else (normals.contiguous(), None, None)
    dev = raw.device
    pieces, counts, start, ok = _cut_outputs(raw, P, cap)
    label = torch.empty((B, M), dtype=torch.uint8, device=dev)
    order = torch.empty((B, M), dtype=torch.int32, device=dev)
    planes = torch.empty((B, P - 1, 4), dtype=torch.float64, device=dev)
    target, cand, anchor, lost = (torch.empty((B, P - 1), dtype=torch.int32, device=dev) for _ in range(4))
    with _on(dev):
        _call("pzn_fracture_eroded_f32", _p(raw), _p(cuts[0]), _p(cuts[1]), _p(cuts[2]), _p(u_anchor), _p(u_start), _p(erode), B, M,
              P, K, n_min, cap, _p(pieces), _p(counts), _p(start), _p(label), _p(order), _p(planes), _p(target), _p(cand),
              _p(anchor), _p(lost), _p(ok), _stream())
    return pieces, counts, start, label, order, planes, target, cand, anchor, lost, ok.to(torch.bool)


def fracture_pair_eroded(raw, normals, u_anchor, pieces, u, erode, n_min, neighbours, cap, frames=None, half_curv=None):
    """ops.fracture_pair (normals) or ops.fracture_pair_curved (frames and half_curv, with normals=None) with the erosion of
    ops.fracture_eroded, one launch (pzn_fracture_pair_eroded_f32; the rule: datapipe.fracture_pair_eroded_rule): erode [B,P-1,4]
    float64; pieces, u, neighbours as ops.fracture_pair takes them
    -> (pieces, counts, start, kind, pair, label, planes, target, cand as the form without erosion returns them, the pieces
        without the lost points; anchor, lost [B,P-1] int32, zero where a step was not made; ok [B] bool)
    2 <= P <= 16, K >= 1, M <= 65536 (PznUnsupported beyond)."""
    B, M, P, K, curved = _eroded_cut_args("fracture_pair_eroded", fracture_pair_eroded_supported, raw, normals, frames, half_curv,
                                          u_anchor, ("u", u, FRACTURE_PAIR_UNIFORMS), erode, cap, n_min)
    cap, n_min, neighbours = int(cap), int(n_min), float(neighbours)
    if not 0.0 <= neighbours <= 1.0:
        raise _lib.PznError(f"fracture_pair_eroded: neighbours = {neighbours}")
    dev = raw.device
    pieces = _pair_pieces("fracture_pair_eroded", pieces, B, P, dev)
    raw, u_anchor, pieces, u, erode = (t.contiguous() for t in (raw, u_anchor, pieces, u, erode))
    cuts = (None, frames.contiguous(), half_curv.contiguous()) if curved else (normals.contiguous(), None, None)
    out, counts, start, ok = _cut_outputs(raw, 4, cap)
    kind = torch.empty((B,), dtype=torch.int32, device=dev)
    pair = torch.empty((B, 4), dtype=torch.int32, device=dev)
    label = torch.empty((B, M), dtype=torch.uint8, device=dev)
    planes = torch.empty((B, P - 1, 4), dtype=torch.float64, device=dev)
    target, cand, anchor, lost = (torch.empty((B, P - 1), dtype=torch.int32, device=dev) for _ in range(4))
    with _on(dev):
        _call("pzn_fracture_pair_eroded_f32", _p(raw), _p(cuts[0]), _p(cuts[1]), _p(cuts[2]), _p(u_anchor), _p(pieces), _p(u),
              _p(erode), neighbours, B, M, P, K, n_min, cap, _p(out), _p(counts), _p(start), _p(kind), _p(pair), _p(label),
              _p(planes), _p(target), _p(cand), _p(anchor), _p(lost), _p(ok), _stream())
    return out, counts, start, kind, pair, label, planes, target, cand, anchor, lost, ok.to(torch.bool)


def pick_mask(idx, N):
    """0/1 float masks [R,N] with ones at idx [R,k] (dataset.py:1363-1366), one launch."""
    idx = _i64(idx, "idx")
    R, k = idx.shape
    mask = torch.empty((R, int(N)), dtype=torch.float32, device=idx.device)
    with _on(idx.device):
        _call("pzn_pick_mask_f32", _p(idx), R, k, int(N), _p(mask), _stream())
    return mask


class _Avg4(torch.autograd.Function):
    """(((a + b) + c) + d) / 4 (model5_b.py:468-469) in one launch."""

    @staticmethod
    def forward(ctx, a, b, c, d):
        a, b, c, d = (_f32(t, "map") for t in (a, b, c, d))
        out = torch.empty_like(a)
        with _on(a.device):
            _call("pzn_avg4_f32", _p(a), _p(b), _p(c), _p(d), a.numel(), _p(out), _stream())
        return out

    @staticmethod
    def backward(ctx, dout):
        g = dout / 4
        return g, g, g, g


def avg4(a, b, c, d):
    return _Avg4.apply(a, b, c, d)


def colmean_argmax(a):
    """a[B,R,C] on the GPU -> (a.mean(dim=1) [B,C], index of its largest entry [B] int64); no gradient (it feeds an index)."""
    a = _f32(a.detach(), "a")
    B, R, C = a.shape
    mean = torch.empty((B, C), dtype=torch.float32, device=a.device)
    arg = torch.empty((B,), dtype=torch.int64, device=a.device)
    ws = torch.empty((_lib.load().pzn_colmean_workspace_bytes(B, C) + 3) // 4, dtype=torch.float32, device=a.device)
    with _on(a.device):
        _call("pzn_colmean_argmax_f32", _p(a), B, R, C, _p(mean), _p(arg), _p(ws), _stream())
    return mean, arg


def se3_exp(x):
    """[B,6] on the GPU -> [B,4,4]"""
    return _Se3Exp.apply(x)


def max_over_points(x):
    """[B, L, C] -> [B, C]"""
    if x.shape[-1] % 4 != 0:
        raise _lib.PznError(f"max_over_points: channel count must be a multiple of 4, got {x.shape[-1]}")
    return _MaxOverPoints.apply(x)


class _Group(torch.autograd.Function):
    """pointnet_util.py:123-132: cat(xyz[idx] - new_xyz, feat[idx]) in one kernel.  idx=None: the K = 32 neighbour
    search of pointnet_util.py:118-119 runs in the same launch (pzn_knn_group_f32) and idx becomes an output."""

    @staticmethod
    def forward(ctx, xyz, feat, new_xyz, idx, want_grouped_xyz):
        xyz, new_xyz = _f32(xyz, "xyz"), _f32(new_xyz, "new_xyz")
        B, N, _ = xyz.shape
        S = new_xyz.shape[1]
        fuse_knn = idx is None
        if fuse_knn:
            K = 32
            idx = torch.empty((B, S, K), dtype=torch.int64, device=xyz.device)
        else:
            idx = _i64(idx, "idx")
            K = idx.shape[2]
        D = 0 if feat is None else feat.shape[-1]
        feat_c = None if feat is None else _f32(feat, "points")
        out = torch.empty((B, S, K, 3 + D), dtype=torch.float32, device=xyz.device)
        gx = torch.empty((B, S, K, 3), dtype=torch.float32, device=xyz.device) if want_grouped_xyz else None
        with _on(xyz.device):
            if fuse_knn:
                _call("pzn_knn_group_f32", _p(xyz), _p(feat_c), _p(new_xyz), B, N, S, D, _p(idx), _p(out), _p(gx), _stream())
            else:
                _call("pzn_group_fwd_f32", _p(xyz), _p(feat_c), _p(new_xyz), _p(idx), B, N, S, K, D,
                      _p(out), _p(gx), _stream())
        ctx.save_for_backward(idx)
        ctx.dims = (B, N, S, K, D)
        ctx.has_feat = feat is not None
        ctx.mark_non_differentiable(idx)
        if gx is not None:
            ctx.mark_non_differentiable(gx)
        return out, gx, idx

    @staticmethod
    def backward(ctx, grad_out, _grad_gx, _grad_idx):
        (idx,) = ctx.saved_tensors
        B, N, S, K, D = ctx.dims
        need_xyz, need_feat, need_new = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        need_feat = need_feat and ctx.has_feat
        if not (need_xyz or need_feat or need_new):
            return None, None, None, None, None
        grad_out = _f32(grad_out, "grad_out")
        dev = grad_out.device
        gxyz = torch.zeros((B, N, 3), dtype=torch.float32, device=dev) if need_xyz else None
        gfeat = torch.zeros((B, N, D), dtype=torch.float32, device=dev) if need_feat else None
        gnew = torch.empty((B, S, 3), dtype=torch.float32, device=dev) if need_new else None
        with _on(dev):
            _call("pzn_group_bwd_f32", _p(grad_out), _p(idx), B, N, S, K, D, _p(gxyz), _p(gfeat), _p(gnew),
                      _stream())
        return gxyz, gfeat, gnew, None, None


def group(xyz, feat, new_xyz, idx, want_grouped_xyz=False):
    out, gx, _ = _Group.apply(xyz, feat, new_xyz, idx, want_grouped_xyz)
    return (out, gx) if want_grouped_xyz else out


def knn_group_supported(xyz, feat, nsample):
    """Shapes pzn_knn_group_f32 takes (include/pzn.h): K = 32, 64 <= N <= 8192, a feature table with D % 4 == 0."""
    return nsample == 32 and feat is not None and feat.shape[-1] > 0 and feat.shape[-1] % 4 == 0 and \
        64 <= xyz.shape[1] <= 8192


def knn_group(xyz, feat, new_xyz, want_grouped_xyz=False):
    """Neighbour search (K = 32) + grouping in one launch -> (new_points[B,S,32,3+D], grouped_xyz or None, idx)."""
    return _Group.apply(xyz, feat, new_xyz, None, want_grouped_xyz)


# --------------------------------------------------------------------------- EMD

def _emd_ws(B, n, m, device):
    nbytes = _lib.load().pzn_emd_workspace_bytes(B, n, m)
    return torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=device)


def _emd_shapes(xyz1, xyz2):
    if xyz1.dim() != 3 or xyz2.dim() != 3 or xyz1.shape[2] != 3 or xyz2.shape[2] != 3 or xyz1.shape[0] != xyz2.shape[0]:
        # emd_kernel.cu:178-180 CHECK_EQ
        raise _lib.PznError(f"EMD expects xyz1[B,n,3], xyz2[B,m,3]; got {tuple(xyz1.shape)}, {tuple(xyz2.shape)}")
    return xyz1.shape[0], xyz1.shape[1], xyz2.shape[1]


def _emd_suffix(*ts):
    """emd_kernel.cu:187,273,391 dispatch on the floating type: fp32 (csrc/emd.hip) or double (csrc/emd64.hip)."""
    if all(t.dtype == torch.float64 for t in ts):
        return torch.float64, "f64"
    return torch.float32, "f32"


def emd_approxmatch(xyz1, xyz2):
    """emd_cuda.approxmatch_forward (emd.cpp:24, emd_kernel.cu:171-193) -> match[B,m,n]"""
    dt, suf = _emd_suffix(xyz1, xyz2)
    xyz1, xyz2 = _req(xyz1, dt, "xyz1"), _req(xyz2, dt, "xyz2")
    B, n, m = _emd_shapes(xyz1, xyz2)
    match = torch.empty((B, m, n), dtype=dt, device=xyz1.device)
    if suf == "f64":
        ws = torch.empty(_lib.load().pzn_emd_workspace_bytes_f64(B, n, m) // 8, dtype=torch.float64, device=xyz1.device)
    else:
        ws = _emd_ws(B, n, m, xyz1.device)
    with _on(xyz1.device):
        _call("pzn_emd_approxmatch_" + suf, _p(xyz1), _p(xyz2), B, n, m, _p(match), _p(ws), _stream())
    return match


def emd_matchcost(xyz1, xyz2, match):
    """emd_cuda.matchcost_forward (emd.cpp:25, emd_kernel.cu:257-279) -> cost[B]"""
    dt, suf = _emd_suffix(xyz1, xyz2, match)
    xyz1, xyz2, match = _req(xyz1, dt, "xyz1"), _req(xyz2, dt, "xyz2"), _req(match, dt, "match")
    B, n, m = _emd_shapes(xyz1, xyz2)
    cost = torch.empty((B,), dtype=dt, device=xyz1.device)
    with _on(xyz1.device):
        _call("pzn_emd_matchcost_" + suf, _p(xyz1), _p(xyz2), _p(match), B, n, m, _p(cost), _stream())
    return cost


def emd_matchcost_grad(grad_cost, xyz1, xyz2, match):
    """emd_cuda.matchcost_backward (emd.cpp:26, emd_kernel.cu:373-398) -> [grad1, grad2]"""
    dt, suf = _emd_suffix(grad_cost, xyz1, xyz2, match)
    grad_cost = _req(grad_cost, dt, "grad_cost")
    xyz1, xyz2, match = _req(xyz1, dt, "xyz1"), _req(xyz2, dt, "xyz2"), _req(match, dt, "match")
    B, n, m = _emd_shapes(xyz1, xyz2)
    g1 = torch.empty((B, n, 3), dtype=dt, device=xyz1.device)
    g2 = torch.empty((B, m, 3), dtype=dt, device=xyz1.device)
    with _on(xyz1.device):
        _call("pzn_emd_matchcost_grad_" + suf, _p(grad_cost), _p(xyz1), _p(xyz2), _p(match), B, n, m,
              _p(g1), _p(g2), _stream())
    return [g1, g2]


EMD_WALK_STATS = None      # bench.py sets this to a list: every fused call appends (walk counters int64 view or None, B, n, m)


class _EmdFused(torch.autograd.Function):
    """EarthMoverDistanceFunction (PyTorchEMD/emd.py:5-21) without the match tensor."""

    @staticmethod
    def forward(ctx, xyz1, xyz2):
        xyz1, xyz2 = _f32(xyz1, "xyz1"), _f32(xyz2, "xyz2")
        B, n, m = _emd_shapes(xyz1, xyz2)
        dev = xyz1.device
        cost = torch.empty((B,), dtype=torch.float32, device=dev)
        g1 = torch.empty((B, n, 3), dtype=torch.float32, device=dev)
        g2 = torch.empty((B, m, 3), dtype=torch.float32, device=dev)
        ws = _emd_ws(B, n, m, dev)
        with _on(dev):
            _call("pzn_emd_fused_f32", _p(xyz1), _p(xyz2), B, n, m, _p(cost), _p(g1), _p(g2), _p(ws), _stream())
        if EMD_WALK_STATS is not None:       # measurement only (bench.py): lengths of the active lists the passes walked
            off = _lib.load().pzn_emd_walk_counter_offset(B, n, m)
            ctr = None if off == 2 ** 64 - 1 else ws.view(torch.int64)[off // 8: off // 8 + _lib.load().pzn_emd_walk_counter_count()]
            EMD_WALK_STATS.append((ctr, B, n, m))
        ctx.save_for_backward(g1, g2)
        return cost

    @staticmethod
    def backward(ctx, grad_cost):
        g1, g2 = ctx.saved_tensors
        gc = grad_cost.contiguous().view(-1, 1, 1)
        return g1 * gc, g2 * gc


def emd_fused(xyz1, xyz2):
    return _EmdFused.apply(xyz1, xyz2)


EMD_SMALL_MAX = 256      # csrc/emd.hip: n, m up to here run as one workgroup per pair


class _EmdFusedSmallMulti(torch.autograd.Function):
    """Several small EarthMoverDistanceFunction calls (PyTorchEMD/emd.py:5-21; n, m <= 256 each) in one launch:
    apply(a1, b1, a2, b2, ...) -> (cost1, cost2, ...), each what _EmdFused gives for its pair, bit for bit."""

    @staticmethod
    def forward(ctx, *clouds):
        k = len(clouds) // 2
        a = [_f32(t, "xyz1") for t in clouds[0::2]]
        b = [_f32(t, "xyz2") for t in clouds[1::2]]
        shapes = [_emd_shapes(x, y) for x, y in zip(a, b)]
        dev = a[0].device
        cost = [torch.empty((B,), dtype=torch.float32, device=dev) for B, _, _ in shapes]
        g1 = [torch.empty((B, n, 3), dtype=torch.float32, device=dev) for B, n, _ in shapes]
        g2 = [torch.empty((B, m, 3), dtype=torch.float32, device=dev) for B, _, m in shapes]
        ints = lambda j: (ctypes.c_int * k)(*[int(sh[j]) for sh in shapes])
        with _on(dev):
            _call("pzn_emd_fused_small_multi_f32", k, _ptrs(a), _ptrs(b), ints(0), ints(1), ints(2), _ptrs(cost), _ptrs(g1),
                  _ptrs(g2), _stream())
        ctx.save_for_backward(*g1, *g2)
        ctx.k = k
        return tuple(cost)

    @staticmethod
    def backward(ctx, *grad_cost):
        k = ctx.k
        g1, g2 = ctx.saved_tensors[:k], ctx.saved_tensors[k:]
        out = []
        for i in range(k):
            if grad_cost[i] is None:
                out += [None, None]
            else:
                gc = grad_cost[i].contiguous().view(-1, 1, 1)
                out += [g1[i] * gc, g2[i] * gc]
        return tuple(out)


def emd_fused_small_multi(pairs):
    """[(xyz1, xyz2), ...] (1..4 pairs, every cloud of at most 256 points) -> [cost[B], ...] from one launch."""
    flat = [t for pr in pairs for t in pr]
    return list(_EmdFusedSmallMulti.apply(*flat))


# --------------------------------------------------------------------------- chamfer

CHAMFER_MAX_BATCH = 65535      # pzn_chamfer_*_f32 put the problem index on the grid's y axis


class _Chamfer(torch.autograd.Function):
    """TouchedRegraster.chamfer_loss (model5_b.py:1495-1505) without P[B,n,m]."""

    @staticmethod
    def forward(ctx, a, b):
        a, b = _f32(a, "a"), _f32(b, "b")
        if a.dim() != 3 or b.dim() != 3 or a.shape[2] != 3 or b.shape[2] != 3 or a.shape[0] != b.shape[0]:
            raise _lib.PznError(f"chamfer expects a[B,n,3], b[B,m,3]; got {tuple(a.shape)}, {tuple(b.shape)}")
        B, n, m = a.shape[0], a.shape[1], b.shape[1]
        if B > CHAMFER_MAX_BATCH:
            raise _lib.PznError(f"chamfer takes at most {CHAMFER_MAX_BATCH} problems in one call (got {B}); "
                                "ops.chamfer splits a larger batch")
        dev = a.device
        moa = torch.empty((B, m), dtype=torch.float32, device=dev)
        mob = torch.empty((B, n), dtype=torch.float32, device=dev)
        aoa = torch.empty((B, m), dtype=torch.int32, device=dev)
        aob = torch.empty((B, n), dtype=torch.int32, device=dev)
        ws = torch.empty((_lib.load().pzn_chamfer_workspace_bytes(B, n, m) + 3) // 4, dtype=torch.float32, device=dev)
        with _on(dev):
            _call("pzn_chamfer_fwd_f32", _p(a), _p(b), B, n, m, _p(moa), _p(aoa), _p(mob), _p(aob), _p(ws), _stream())
        ctx.save_for_backward(a, b, aoa, aob)
        ctx.mark_non_differentiable(aoa, aob)
        ctx.set_materialize_grads(False)      # (the arg-min outputs carry no gradient: no zero-filled stand-ins for them)
        return moa, mob, aoa, aob

    @staticmethod
    def backward(ctx, g_moa, g_mob, _ga, _gb):
        a, b, aoa, aob = ctx.saved_tensors
        B, n, m = a.shape[0], a.shape[1], b.shape[1]
        g_moa = None if g_moa is None else _f32(g_moa, "g_over_a")
        g_mob = None if g_mob is None else _f32(g_mob, "g_over_b")
        if g_moa is None and g_mob is None:
            return None, None
        both = torch.zeros((B * (n + m) * 3,), dtype=torch.float32, device=a.device)      # one fill for the two atomic targets
        ga, gb = both[:B * n * 3].view(B, n, 3), both[B * n * 3:].view(B, m, 3)
        with _on(a.device):
            _call("pzn_chamfer_bwd_f32", _p(a), _p(b), B, n, m, _p(g_moa), _p(aoa), _p(g_mob), _p(aob),
                  _p(ga), _p(gb), _stream())
        return ga, gb


def chamfer(a, b):
    """-> (min over a per b-point [B,m], min over b per a-point [B,n])  == torch.min(P,1)[0], torch.min(P,2)[0].
    More than CHAMFER_MAX_BATCH problems (assembly's K^2 pairs from K = 256 pieces on) go in several calls, each chunk with
    the bits of a call of its own."""
    if (isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor) and a.dim() == 3 and b.dim() == 3
            and a.shape[0] == b.shape[0] and a.shape[0] > CHAMFER_MAX_BATCH):
        parts = [_Chamfer.apply(a[s:s + CHAMFER_MAX_BATCH], b[s:s + CHAMFER_MAX_BATCH])
                 for s in range(0, a.shape[0], CHAMFER_MAX_BATCH)]
        return torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])
    moa, mob, _, _ = _Chamfer.apply(a, b)
    return moa, mob


# --------------------------------------------------------------------------- dense (MFMA fp32)

# Gradient sinks: parameter storage address -> its (pre-zeroed) gradient tensor.  When a parameter has a
# sink, the weight-gradient kernels ADD straight into it and the autograd Function returns None for that
# input: no zero-fill launch, no temporary dW, no separate AccumulateGrad "grad += dW" kernel
# (~280 small launches per training step).  distributed.FlatGradAllReduce registers the views of its flat
# bucket; without sinks the Functions return ordinary gradient tensors.
_GRAD_SINKS = {}      # parameter address -> (weak reference to the parameter, its gradient buffer)


def register_grad_sinks(params):
    for p_ in params:
        if p_.grad is not None:
            _GRAD_SINKS[p_.data_ptr()] = (weakref.ref(p_), p_.grad)


def clear_grad_sinks():
    _GRAD_SINKS.clear()


def _sink(t, needed):
    """The registered gradient buffer of parameter tensor `t`, or None.  An entry only counts while its parameter is
    alive, still sits at that address and has this shape (a freed parameter's address is re-used by the allocator:
    a stale entry must never capture the gradient of an unrelated tensor)."""
    if not needed or t is None:
        return None
    ent = _GRAD_SINKS.get(t.data_ptr())
    if ent is None:
        return None
    owner, grad = ent
    o = owner()
    if o is None or o.data_ptr() != t.data_ptr() or o.shape != t.shape or o.grad is not grad:
        _GRAD_SINKS.pop(t.data_ptr(), None)
        return None
    return grad

class _Linear(torch.autograd.Function):
    """nn.Linear (+ReLU) on the fp32 matrix-core engine: y = act(x W^T + b)."""

    @staticmethod
    def forward(ctx, x, weight, bias, relu):
        x = _f32(x, "x")
        weight = _f32(weight, "weight")
        bias_c = None if bias is None else _f32(bias, "bias")
        Kin = x.shape[-1]
        Nout = weight.shape[0]
        if weight.shape[1] != Kin:
            raise _lib.PznError(f"linear: x[..., {Kin}] vs weight{tuple(weight.shape)}")
        x2 = x.reshape(-1, Kin)
        M = x2.shape[0]
        y = torch.empty((M, Nout), dtype=torch.float32, device=x.device)
        with _on(x.device):
            _call("pzn_linear_fwd_f32", _p(x2), _p(weight), _p(bias_c), M, Kin, Nout, int(bool(relu)), _p(y), _stream(),
                  flops=2 * M * Kin * Nout)
        ctx.save_for_backward(x2, weight, y if relu else None)
        ctx.has_bias = bias is not None
        ctx.bias_ref = bias_c
        ctx.in_shape = x.shape
        return y.reshape(*x.shape[:-1], Nout)

    @staticmethod
    def backward(ctx, dy):
        x2, weight, y = ctx.saved_tensors
        M, Kin = x2.shape
        Nout = weight.shape[0]
        dy = _f32(dy, "dy").reshape(M, Nout)
        dev = dy.device
        dx = dW = db = None
        with _on(dev):
            if ctx.needs_input_grad[0]:
                dx = torch.empty((M, Kin), dtype=torch.float32, device=dev)
                _call("pzn_linear_dgrad_f32", _p(dy), _p(y), _p(weight), M, Kin, Nout, None, _p(dx), _stream(),
                      flops=2 * M * Kin * Nout)
                dx = dx.reshape(ctx.in_shape)
            if ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2]):
                sw = _sink(weight, ctx.needs_input_grad[1])
                sb = _sink(ctx.bias_ref, ctx.has_bias and ctx.needs_input_grad[2])
                if sw is not None and (sb is not None or not ctx.has_bias):
                    _call("pzn_linear_wgrad_f32", _p(dy), _p(y), _p(x2), M, Kin, Nout, _p(sw), _p(sb), 1, _stream(),
                          flops=2 * M * Kin * Nout)
                else:
                    dW = torch.empty((Nout, Kin), dtype=torch.float32, device=dev)
                    db = torch.empty((Nout,), dtype=torch.float32, device=dev) if ctx.has_bias else None
                    _call("pzn_linear_wgrad_f32", _p(dy), _p(y), _p(x2), M, Kin, Nout, _p(dW), _p(db), 0, _stream(),
                          flops=2 * M * Kin * Nout)
        return dx, dW, db, None


def linear(x, weight, bias=None, relu=False):
    return _Linear.apply(x, weight, bias, relu)


def _ptrs(ts):
    """Array of device pointers, one per problem, for the nprob entry points."""
    return (ctypes.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts])


_ROWS_PLANS = {}      # (M, widths) -> (widths as a C array, workspace bytes)


def _rows_plan(M, widths):
    pl = _ROWS_PLANS.get((M, widths))
    if pl is None:
        arr = (ctypes.c_int * len(widths))(*widths)
        pl = _ROWS_PLANS[(M, widths)] = (arr, _lib.load().pzn_fewrow_chain_workspace_bytes(M, len(widths) - 1, arr))
    return pl


def _rows_dense(t):
    return (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()
            and t.data_ptr() % 16 == 0)


def mlp_rows_supported(parts, weights, biases):
    """Whether the few-row chain (include/pzn.h, pzn_fewrow_chain_*) takes this stack: one or two [M, k] input parts side
    by side, M <= 128, dense float32 operands where they lie, the split-precision matrix-core modes."""
    if not (1 <= len(parts) <= 2 and len(weights) == len(biases) >= 1):
        return False
    if not all(_rows_dense(t) and t.dim() == 2 for t in tuple(parts) + tuple(weights)):
        return False
    if not all(b is None or (_rows_dense(b) and b.dim() == 1) for b in biases):
        return False
    M = parts[0].shape[0]
    widths = (sum(p_.shape[1] for p_ in parts),) + tuple(w.shape[0] for w in weights)
    if any(p_.shape[0] != M for p_ in parts) or any(w.shape[1] != k for w, k in zip(weights, widths)):
        return False
    if any(b is not None and b.shape[0] != n for b, n in zip(biases, widths[1:])):
        return False
    if not (1 <= M <= 128 and len(weights) <= 16):
        return False
    return bool(_lib.load().pzn_fewrow_chain_supported(M, len(weights), _rows_plan(M, widths)[0]))


class _MlpRows(torch.autograd.Function):
    """A stack of nn.Linear (+ReLU) on few rows as one chain of launches each way (csrc/fewrows.hip): the same tensors and
    gradients as the composed ops.linear calls on cat(parts, -1), summed in a fixed order."""

    @staticmethod
    def forward(ctx, n_parts, relus, *ts):
        L = len(relus)
        parts, weights, biases = ts[:n_parts], ts[n_parts:n_parts + L], ts[n_parts + L:]
        M, k0 = parts[0].shape
        x1 = parts[1] if n_parts == 2 else None
        k1 = x1.shape[1] if n_parts == 2 else 0
        widths = (k0 + k1,) + tuple(w.shape[0] for w in weights)
        arr, nbytes = _rows_plan(M, widths)
        dev = parts[0].device
        ys = [torch.empty((M, n), dtype=torch.float32, device=dev) for n in widths[1:]]
        ws = torch.empty((nbytes // 4,), dtype=torch.float32, device=dev)
        relu_arr = (ctypes.c_int * L)(*[int(bool(r)) for r in relus])
        flops = 2 * M * sum(a * b for a, b in zip(widths, widths[1:]))
        with _on(dev):
            _call("pzn_fewrow_chain_fwd_f32", _p(parts[0]), k0, _p(x1), k1, M, L, arr, _ptrs(weights), _ptrs(biases), relu_arr,
                  _ptrs(ys), ws.data_ptr(), nbytes, _stream(), flops=flops)
        ctx.save_for_backward(*parts, *weights, *ys)
        ctx.bias_refs = biases
        ctx.plan = (n_parts, L, M, k0, k1, arr, nbytes, relu_arr, flops)
        return ys[-1]

    @staticmethod
    def backward(ctx, dy):
        n_parts, L, M, k0, k1, arr, nbytes, relu_arr, flops = ctx.plan
        saved = ctx.saved_tensors
        parts, weights, ys = saved[:n_parts], saved[n_parts:n_parts + L], saved[n_parts + L:]
        biases = ctx.bias_refs
        needs = ctx.needs_input_grad
        dy = _f32(dy, "dy").reshape(M, weights[-1].shape[0])
        dev = dy.device
        dparts = [torch.empty_like(p_) if needs[2 + j] else None for j, p_ in enumerate(parts)]
        dWs, dbs, tw, tb, acc = [None] * L, [None] * L, [None] * L, [None] * L, [0] * L
        for i, (w, b) in enumerate(zip(weights, biases)):
            need_w, need_b = needs[2 + n_parts + i], b is not None and needs[2 + n_parts + L + i]
            if not (need_w or need_b):
                continue
            sw, sb = _sink(w, need_w), _sink(b, need_b)
            if sw is not None and (sb is not None or b is None):
                tw[i], tb[i], acc[i] = sw, sb, 1
            else:
                dWs[i] = tw[i] = torch.empty_like(w)
                dbs[i] = tb[i] = None if b is None else torch.empty_like(b)
        ws = torch.empty((nbytes // 4,), dtype=torch.float32, device=dev)
        with _on(dev):
            _call("pzn_fewrow_chain_bwd_f32", _p(dy), _p(parts[0]), k0, _p(parts[1]) if n_parts == 2 else None, k1, M, L, arr,
                  _ptrs(weights), relu_arr, _ptrs(ys), _p(dparts[0]), _p(dparts[1]) if n_parts == 2 else None, _ptrs(tw),
                  _ptrs(tb), (ctypes.c_int * L)(*acc), ws.data_ptr(), nbytes, _stream(), flops=2 * flops)
        return (None, None, *dparts, *dWs, *dbs)


def mlp_rows(parts, weights, biases, relus=None):
    """act(... act(cat(parts, -1) W_1^T + b_1) ...) for one or two [M, k] parts: nn.Linear layers with a ReLU behind each
    where relus[i] (default: behind every layer but the last, the nn.Sequential of model5_b._seq).  Few rows (M <= 128) run
    as the chain of csrc/fewrows.hip - one launch per layer each way, bit-identical from run to run; every other stack,
    and the exact-fp32 mode, as the ops.linear calls it stands for."""
    parts, weights, biases = tuple(parts), tuple(weights), tuple(biases)
    relus = tuple(i + 1 < len(weights) for i in range(len(weights))) if relus is None else tuple(bool(r) for r in relus)
    if len(relus) != len(weights):
        raise _lib.PznError(f"mlp_rows: {len(weights)} layers, {len(relus)} ReLU flags")
    if mlp_rows_supported(parts, weights, biases):
        return _MlpRows.apply(len(parts), relus, *parts, *weights, *biases)
    x = parts[0] if len(parts) == 1 else torch.cat(parts, dim=-1)
    for w, b, r in zip(weights, biases, relus):
        x = linear(x, w, b, relu=r)
    return x


def _f32_rows(t, name):
    """linear_cols takes its operands where they lie: on the GPU, float32, contiguous - no copy is made for it."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise _lib.PznError(f"linear_cols: {name} must be a tensor on the GPU; puzzlenet_amd has no CPU fallback")
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise _lib.PznError(f"linear_cols: {name} must be float32 with contiguous rows; got {t.dtype}, strides {t.stride()}")


def linear_cols(x, weight, col0, bias=None, accumulate=False, out=None):
    """x @ weight[:, col0:col0 + x.shape[-1]].T (+ bias) with the columns of the wider weight read in place: the product
    of one slice of a concatenated input (include/pzn.h, pzn_linear_slice_fwd_f32) -> [..., weight.shape[0]].  accumulate:
    the product is added to `out` instead (the bias is not read then).  Forward only: no autograd, nothing saved."""
    _f32_rows(x, "x")
    _f32_rows(weight, "weight")
    if bias is not None:
        _f32_rows(bias, "bias")
    if weight.dim() != 2 or x.dim() < 1 or x.shape[-1] == 0:
        raise _lib.PznError(f"linear_cols expects x[..., Kin], weight[Nout, >= Kin]; got {tuple(x.shape)}, {tuple(weight.shape)}")
    Kin = x.shape[-1]
    Nout, ldw = weight.shape
    if col0 < 0 or col0 + Kin > ldw:
        raise _lib.PznError(f"linear_cols: columns {col0}..{col0 + Kin} of weight{tuple(weight.shape)}")
    M = x.numel() // Kin
    if out is None:
        if accumulate:
            raise _lib.PznError("linear_cols: accumulate adds to `out`")
        out = torch.empty(x.shape[:-1] + (Nout,), dtype=torch.float32, device=x.device)
    else:
        _f32_rows(out, "out")
        if out.numel() != M * Nout:
            raise _lib.PznError(f"linear_cols: out{tuple(out.shape)} vs {M} rows of {Nout}")
    with _on(x.device):
        _call("pzn_linear_slice_fwd_f32", x.data_ptr(), weight.data_ptr() + 4 * col0, ldw, _p(bias), M, Kin, Nout,
              int(bool(accumulate)), out.data_ptr(), _stream(), flops=2 * M * Kin * Nout)
    return out


class _CatGlobalLinearRelu(torch.autograd.Function):
    """relu(Linear(cat([g.repeat(1, N, 1), x], -1))) without the concatenation (model5_b.py:745-752, first layer of the
    boundary heads): the product splits into x W[:, Cg:]^T per point and g W[:, :Cg]^T + b per CLOUD; the per-cloud part
    is a [B, Cout] bias added (with the ReLU) by pzn_cloud_bias_relu_f32.  Backward: the gated gradient goes through the
    point part's two products (the kernels take the ReLU mask), its per-cloud column sums (pzn_cloud_gated_colsum_f32)
    through the global part's.  x[B,N,C], g[B,Cg] (or [B,1,Cg]), weight[Cout, Cg + C], bias[Cout]."""

    @staticmethod
    def forward(ctx, x, g, weight, bias):
        x, g, weight, bias = _f32(x, "x"), _f32(g, "g"), _f32(weight, "weight"), _f32(bias, "bias")
        B, N, C = x.shape
        g2 = g.reshape(B, -1)
        Cg = g2.shape[1]
        Co = weight.shape[0]
        if weight.shape[1] != Cg + C:
            raise _lib.PznError(f"cat_global_linear_relu: weight{tuple(weight.shape)} vs {Cg} + {C} input columns")
        dev = x.device
        w_g, w_x = weight[:, :Cg].contiguous(), weight[:, Cg:].contiguous()
        x2 = x.reshape(B * N, C)
        y = torch.empty((B * N, Co), dtype=torch.float32, device=dev)
        cb = torch.empty((B, Co), dtype=torch.float32, device=dev)
        with _on(dev):
            st = _stream()
            _call("pzn_linear_fwd_f32", _p(g2), _p(w_g), _p(bias), B, Cg, Co, 0, _p(cb), st, flops=2 * B * Cg * Co)
            _call("pzn_linear_fwd_f32", _p(x2), _p(w_x), None, B * N, C, Co, 0, _p(y), st, flops=2 * B * N * C * Co)
            _call("pzn_cloud_bias_relu_f32", _p(y), _p(cb), B, N, Co, st)
        ctx.save_for_backward(x2, g2, w_g, w_x, y)
        ctx.dims = (B, N, C, Cg, Co)
        ctx.g_shape = g.shape
        return y.view(B, N, Co)

    @staticmethod
    def backward(ctx, dy):
        x2, g2, w_g, w_x, y = ctx.saved_tensors
        B, N, C, Cg, Co = ctx.dims
        dev = y.device
        dy = _f32(dy, "dy").reshape(B * N, Co)
        mk = lambda *sh: torch.empty(sh, dtype=torch.float32, device=dev)
        dx = dg = dW = db = None
        with _on(dev):
            st = _stream()
            dcb = mk(B, Co)
            _call("pzn_cloud_gated_colsum_f32", _p(dy), _p(y), B, N, Co, _p(dcb), st)
            if ctx.needs_input_grad[0]:
                dx = mk(B * N, C)
                _call("pzn_linear_dgrad_f32", _p(dy), _p(y), _p(w_x), B * N, C, Co, None, _p(dx), st, flops=2 * B * N * C * Co)
                dx = dx.view(B, N, C)
            if ctx.needs_input_grad[1]:
                dg = mk(B, Cg)
                _call("pzn_linear_dgrad_f32", _p(dcb), None, _p(w_g), B, Cg, Co, None, _p(dg), st, flops=2 * B * Cg * Co)
                dg = dg.view(ctx.g_shape)
            if ctx.needs_input_grad[2] or ctx.needs_input_grad[3]:
                dWx, dWg, db = mk(Co, C), mk(Co, Cg), mk(Co)
                _call("pzn_linear_wgrad_f32", _p(dy), _p(y), _p(x2), B * N, C, Co, _p(dWx), _p(db), 0, st,
                      flops=2 * B * N * C * Co)                                   # db = column sums of the gated gradient
                _call("pzn_linear_wgrad_f32", _p(dcb), None, _p(g2), B, Cg, Co, _p(dWg), None, 0, st, flops=2 * B * Cg * Co)
                dW = torch.cat([dWg, dWx], dim=1)
        return dx, dg, dW, db


def cat_global_linear_relu(x, g, weight, bias):
    return _CatGlobalLinearRelu.apply(x, g, weight, bias)


class _PointMlp3(torch.autograd.Function):
    """Three Linear layers with ReLU after the first two on [B, N, 64] rows, one launch each way (csrc/pointmlp.hip):
    nn.Sequential(Linear, ReLU, Linear, ReLU, Linear) of the boundary heads (model5_b.py:571-592, 738-739, 751-754).
    g is None: 64 -> 64 -> C2 -> C3 as it stands.  g[B, Cg] (or [B, 1, Cg]): the first layer acts on
    cat([g.repeat(1, N, 1), x], -1) (model5_b.py:745-749) — its global half becomes a per-cloud bias g W1[:, :Cg]^T + b1,
    whose gradient (the per-cloud column sums of the first gated gradient) the backward pass returns with the rest."""

    @staticmethod
    def forward(ctx, x, g, w1, b1, w2, b2, w3, b3):
        x = _f32(x, "x")
        w1, b1, w2, b2, w3, b3 = (_f32(t, n) for t, n in ((w1, "w1"), (b1, "b1"), (w2, "w2"), (b2, "b2"), (w3, "w3"), (b3, "b3")))
        B, N, C = x.shape
        M, C2, C3 = B * N, w2.shape[0], w3.shape[0]
        dev = x.device
        mk = lambda *sh: torch.empty(sh, dtype=torch.float32, device=dev)
        x2 = x.reshape(M, C)
        h1, h2, y = mk(M, 64), mk(M, C2), mk(M, C3)
        Cg = 0
        g2 = w_g = None
        with _on(dev):
            st = _stream()
            if g is not None:
                g2 = _f32(g, "g").reshape(B, -1)
                Cg = g2.shape[1]
                if w1.shape[1] != Cg + C:
                    raise _lib.PznError(f"point_mlp3: w1{tuple(w1.shape)} vs {Cg} + {C} input columns")
                bias1 = linear_cols(g2, w1, 0, b1)      # [B,64]: g W1[:, :Cg]^T + b1, the columns read in place
            else:
                bias1 = b1
            _call("pzn_point_mlp3_fwd_f32", _p(x2), M, N, _p(w1) + 4 * Cg, w1.shape[1], _p(bias1), 1 if g is not None else 0,
                  _p(w2), _p(b2), _p(w3), _p(b3), C2, C3, _p(h1), _p(h2), _p(y), st,
                  flops=2 * M * (64 * 64 + 64 * C2 + C2 * C3))
        ctx.save_for_backward(x2, g2, w_g, w1, w2, w3, h1, h2)
        ctx.bias_refs = (b1, b2, b3)      # (for their registered gradient buffers; parameters, alive anyway)
        ctx.dims = (B, N, C2, C3, Cg)
        ctx.g_shape = None if g is None else g.shape
        return y.view(B, N, C3)

    @staticmethod
    def backward(ctx, dy):
        x2, g2, w_g, w1, w2, w3, h1, h2 = ctx.saved_tensors
        B, N, C2, C3, Cg = ctx.dims
        M = B * N
        dev = x2.device
        dy = _f32(dy, "dy").reshape(M, C3)
        mk = lambda *sh: torch.empty(sh, dtype=torch.float32, device=dev)
        per_cloud = 1 if g2 is not None else 0
        nws = _lib.load().pzn_point_mlp3_bwd_workspace_bytes(M, N, per_cloud, C2, C3)
        ws = torch.empty((max(16, nws),), dtype=torch.uint8, device=dev)
        # the six parameter gradients straight into their registered buffers (ops.register_grad_sinks) when all six have one:
        # no six AccumulateGrad adds per head behind the node
        b1p, b2p, b3p = ctx.bias_refs
        sinks = [_sink(t, ctx.needs_input_grad[2 + i]) for i, t in enumerate((w1, b1p, w2, b2p, w3, b3p))]
        direct = all(s_ is not None for s_ in sinks)
        dx = mk(M, 64)
        if direct:
            dW1, db1_out, dW2, db2, dW3, db3 = sinks
        else:
            dW1, dW2, dW3, db2, db3, db1_out = mk(64, Cg + 64), mk(C2, 64), mk(C3, C2), mk(C2), mk(C3), mk(64)
        db1 = mk(B, 64) if per_cloud else db1_out
        dg = None
        with _on(dev):
            st = _stream()
            _call("pzn_point_mlp3_bwd_f32", _p(dy), _p(x2), _p(h1), _p(h2), M, N, _p(w1) + 4 * Cg, Cg + 64, per_cloud, _p(w2),
                  _p(w3), C2, C3, _p(dx), _p(dW1) + 4 * Cg, _p(db1), _p(dW2), _p(db2), _p(dW3), _p(db3), int(direct), _p(ws), st,
                  flops=4 * M * (64 * 64 + 64 * C2 + C2 * C3))
            if per_cloud:       # the global half of the first layer: [B, Cg] products on the per-cloud bias gradient
                dcb = db1
                if direct:      # += into the first Cg columns of the registered dW1 and into db1
                    _call("pzn_linear_slice_wgrad_f32", _p(dcb), _p(g2), B, Cg, 64, _p(dW1), Cg + 64, _p(db1_out), st,
                          flops=2 * B * Cg * 64)
                else:
                    dWg = mk(64, Cg)
                    _call("pzn_linear_wgrad_f32", _p(dcb), None, _p(g2), B, Cg, 64, _p(dWg), _p(db1_out), 0, st, flops=2 * B * Cg * 64)
                    dW1[:, :Cg] = dWg
                if ctx.needs_input_grad[1]:
                    dg = mk(B, Cg)
                    _call("pzn_linear_slice_dgrad_f32", _p(dcb), _p(w1), Cg + 64, B, Cg, 64, None, _p(dg), st, flops=2 * B * Cg * 64)
                    dg = dg.view(ctx.g_shape)
        if direct:
            return dx.view(B, N, 64), dg, None, None, None, None, None, None
        return dx.view(B, N, 64), dg, dW1, db1_out, dW2, db2, dW3, db3


def point_mlp3_available(C0, C1, C2, C3):
    return bool(_lib.load().pzn_point_mlp3_supported(int(C0), int(C1), int(C2), int(C3)))


def point_mlp3(x, w1, b1, w2, b2, w3, b3, g=None):
    """(relu(relu([g |] x) W1^T + b1) W2^T + b2) W3^T + b3 on [B, N, 64] rows; see _PointMlp3."""
    return _PointMlp3.apply(x, g, w1, b1, w2, b2, w3, b3)


def pair_head_supported(N, C2, C3):
    return bool(_lib.load().pzn_pair_head_supported(int(N), int(C2), int(C3)))


def pair_head(x, g, w1, b1, w2, b2, w3, b3):
    """MLPFpcb over every (fixed, moved) pair without the pair batch (csrc/pointmlp.hip, pair_head_fwd_kernel):
    y[i, j] = the 128 -> 64 -> 32 -> 2 chain on cat([g[j].repeat(N, 1), x[i]], -1).  x[Kf,N,64] local features of the
    fixed-role pieces, g[Km,64] (or [Km,1,64]) the moved pieces' global vectors, w1[64,128] -> [Kf,Km,N,2].  The global
    half of the first layer becomes the per-moved-piece bias c = g W1[:, :64]^T + b1 (as _PointMlp3.forward forms it), then
    one launch.  Forward only: no autograd, nothing saved."""
    x = _f32(x.detach(), "x")
    g = _f32(g.detach(), "g")
    w1, b1, w2, b2, w3, b3 = (_f32(t.detach(), n) for t, n in ((w1, "w1"), (b1, "b1"), (w2, "w2"), (b2, "b2"), (w3, "w3"), (b3, "b3")))
    if x.dim() != 3 or x.shape[2] != 64:
        raise _lib.PznError(f"pair_head expects x[Kf,N,64]; got {tuple(x.shape)}")
    Kf, N, C = x.shape
    g2 = g.reshape(-1, g.shape[-1])
    Km, Cg = g2.shape
    C2, C3 = w2.shape[0], w3.shape[0]
    if w1.shape != (64, Cg + C) or w2.shape[1] != 64 or w3.shape[1] != C2:
        raise _lib.PznError(f"pair_head: w1{tuple(w1.shape)}, w2{tuple(w2.shape)}, w3{tuple(w3.shape)} vs {Cg} + {C} input columns")
    if not pair_head_supported(N, C2, C3):
        raise _lib.PznUnsupported(f"pair_head: N = {N} (a multiple of 32) and a 64 -> {C2} -> {C3} tail (32 -> 2) are not "
                                  "a shape the kernel takes")
    dev = x.device
    y = torch.empty((Kf, Km, N, C3), dtype=torch.float32, device=dev)
    with _on(dev):
        st = _stream()
        c = linear_cols(g2, w1, 0, b1)      # [Km,64]
        _call("pzn_pair_head_fwd_f32", _p(x), Kf, N, _p(c), Km, _p(w1) + 4 * Cg, Cg + C, _p(w2), _p(b2), _p(w3), _p(b3),
              C2, C3, _p(y), st, flops=2 * Kf * N * (64 * 64 + Km * (64 * C2 + C2 * C3)))
    return y


def pair_head_blocks_supported(N, C2, C3):
    return bool(_lib.load().pzn_pair_head_blocks_supported(int(N), int(C2), int(C3)))


def pair_head_blocks(x, g, w1, b1, w2, b2, w3, b3):
    """pair_head for Z puzzles in one launch, block-diagonal (csrc/pointmlp.hip, pair_head_fwd_kernel behind
    pzn_pair_head_blocks_fwd_f32): x[Z,Kf,N,64] local features of the fixed-role pieces, g[Z,Km,64] the moved pieces' global
    vectors -> y[Z,Kf,Km,N,2] with y[z] = pair_head(x[z], g[z], ...) bit for bit: the fixed piece (z, i) meets only the moved
    pieces of its own puzzle.  One linear_cols over the Z Km global vectors, then one launch; Z = 0 launches nothing.
    Forward only: no autograd, nothing saved."""
    x = _f32(x.detach(), "x")
    g = _f32(g.detach(), "g")
    w1, b1, w2, b2, w3, b3 = (_f32(t.detach(), n) for t, n in ((w1, "w1"), (b1, "b1"), (w2, "w2"), (b2, "b2"), (w3, "w3"), (b3, "b3")))
    if x.dim() != 4 or x.shape[3] != 64:
        raise _lib.PznError(f"pair_head_blocks expects x[Z,Kf,N,64]; got {tuple(x.shape)}")
    Z, Kf, N, C = x.shape
    if g.dim() != 3 or g.shape[0] != Z:
        raise _lib.PznError(f"pair_head_blocks expects g[{Z},Km,Cg]; got {tuple(g.shape)}")
    Km, Cg = g.shape[1], g.shape[2]
    C2, C3 = w2.shape[0], w3.shape[0]
    if w1.shape != (64, Cg + C) or w2.shape[1] != 64 or w3.shape[1] != C2:
        raise _lib.PznError(f"pair_head_blocks: w1{tuple(w1.shape)}, w2{tuple(w2.shape)}, w3{tuple(w3.shape)} vs {Cg} + {C} input columns")
    if Kf < 1 or Km < 1:
        raise _lib.PznError(f"pair_head_blocks: Kf = {Kf}, Km = {Km} pieces a puzzle (>= 1)")
    if not pair_head_blocks_supported(N, C2, C3):
        raise _lib.PznUnsupported(f"pair_head_blocks: N = {N} (a multiple of 32) and a 64 -> {C2} -> {C3} tail (32 -> 2) are not "
                                  "a shape the kernel takes")
    dev = x.device
    y = torch.empty((Z, Kf, Km, N, C3), dtype=torch.float32, device=dev)
    if Z == 0:
        return y
    with _on(dev):
        st = _stream()
        c = linear_cols(g.reshape(Z * Km, Cg), w1, 0, b1)      # [Z Km,64]
        _call("pzn_pair_head_blocks_fwd_f32", _p(x), Z, Kf, N, _p(c), Km, _p(w1) + 4 * Cg, Cg + C, _p(w2), _p(b2), _p(w3), _p(b3),
              C2, C3, _p(y), st, flops=2 * Z * Kf * N * (64 * 64 + Km * (64 * C2 + C2 * C3)))
    return y


class _SharedMlpMax(torch.autograd.Function):
    """relu(x W1^T + b1) -> relu(. W2^T + b2) -> max over the K=32 axis (model5_b.py:452-454, 459-461)."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2):
        x = _f32(x, "x")
        w1, b1, w2, b2 = _f32(w1, "w1"), _f32(b1, "b1"), _f32(w2, "w2"), _f32(b2, "b2")
        Bq, S, K, C0 = x.shape
        if K != 32:
            raise _lib.PznError(f"shared_mlp_max: the fused epilogue pools over K=32 neighbours, got K={K}")
        C1, C2 = w1.shape[0], w2.shape[0]
        R = Bq * S
        dev = x.device
        h = torch.empty((R * 32, C1), dtype=torch.float32, device=dev)
        out = torch.empty((R, C2), dtype=torch.float32, device=dev)
        arg = torch.empty((R, C2), dtype=torch.int32, device=dev)
        with _on(dev):
            _call("pzn_sharedmlp_max_fwd_f32", _p(x), _p(w1), _p(b1), _p(w2), _p(b2), R, C0, C1, C2,
                  _p(h), _p(out), _p(arg), _stream())
        ctx.save_for_backward(x, w1, w2, h, out, arg)
        ctx.dims = (Bq, S, R, C0, C1, C2)
        return out.reshape(Bq, S, C2)

    @staticmethod
    def backward(ctx, dout):
        x, w1, w2, h, out, arg = ctx.saved_tensors
        Bq, S, R, C0, C1, C2 = ctx.dims
        dout = _f32(dout, "dout").reshape(R, C2)
        dev = dout.device
        dh = torch.empty((R * 32, C1), dtype=torch.float32, device=dev)
        dx = torch.empty((R * 32, C0), dtype=torch.float32, device=dev) if ctx.needs_input_grad[0] else None
        dW1 = torch.empty_like(w1)
        db1 = torch.empty((C1,), dtype=torch.float32, device=dev)
        dW2 = torch.empty_like(w2)
        db2 = torch.empty((C2,), dtype=torch.float32, device=dev)
        with _on(dev):
            _call("pzn_sharedmlp_max_bwd_f32", _p(x), _p(w1), _p(w2), _p(h), _p(out), _p(arg), _p(dout),
                  R, C0, C1, C2, _p(dh), _p(dx), _p(dW1), _p(db1), _p(dW2), _p(db2), 0, _stream())
        return (None if dx is None else dx.reshape(Bq, S, 32, C0)), dW1, db1, dW2, db2


def shared_mlp_max(x, w1, b1, w2, b2):
    return _SharedMlpMax.apply(x, w1, b1, w2, b2)


class _Attention(torch.autograd.Function):
    """scaled_dot_production (model5_b.py:67-75) -> (values, attention)."""

    @staticmethod
    def forward(ctx, q, k, v):
        q, k, v = _f32(q, "q"), _f32(k, "k"), _f32(v, "v")
        B, L, dk = q.shape
        dv = v.shape[-1]
        dev = q.device
        attn = torch.empty((B, L, L), dtype=torch.float32, device=dev)
        out = torch.empty((B, L, dv), dtype=torch.float32, device=dev)
        with _on(dev):
            _call("pzn_attn_fwd_f32", _p(q), _p(k), _p(v), B, L, dk, dv, _p(attn), _p(out), _stream(),
                  flops=2 * B * L * L * (dk + dv))
        ctx.save_for_backward(q, k, v, attn)
        ctx.set_materialize_grads(False)
        return out, attn

    @staticmethod
    def backward(ctx, d_out, d_attn):
        q, k, v, attn = ctx.saved_tensors
        B, L, dk = q.shape
        dv = v.shape[-1]
        dev = q.device
        d_out = torch.zeros((B, L, dv), dtype=torch.float32, device=dev) if d_out is None else _f32(d_out, "d_out")
        d_attn = None if d_attn is None else _f32(d_attn, "d_attn")
        dq, dk_, dv_ = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        ws = torch.empty((B, L, L), dtype=torch.float32, device=dev)
        with _on(dev):
            _call("pzn_attn_bwd_f32", _p(q), _p(k), _p(v), _p(attn), _p(d_out), _p(d_attn), B, L, dk, dv,
                  _p(dq), _p(dk_), _p(dv_), _p(ws), _stream(), flops=2 * B * L * L * (2 * dk + 2 * dv))
        return dq, dk_, dv_


def attention(q, k, v):
    return _Attention.apply(q, k, v)


class _AttentionBlock(torch.autograd.Function):
    """layerAttention as one unit (model5_b.py:83-101) -> (r, attention): the residual / offset lines ride in GEMM
    epilogues forward, and the five contributions to dx are summed by accumulate epilogues backward."""

    @staticmethod
    def forward(ctx, x, wq, bq, wk, bk, wv, bv, wo, bo):
        x = _f32(x, "x")
        ws_ = [_f32(t, "param") for t in (wq, bq, wk, bk, wv, bv, wo, bo)]
        wq, bq, wk, bk, wv, bv, wo, bo = ws_
        B, L, E = x.shape
        dk = wq.shape[0]
        dev = x.device
        M = B * L
        mk = lambda *sh: torch.empty(sh, dtype=torch.float32, device=dev)
        q, k, v = mk(M, dk), mk(M, dk), mk(M, E)
        attn, r, yo, out = mk(B, L, L), mk(M, E), mk(M, E), mk(M, E)
        with _on(dev):
            _call("pzn_attn_block_fwd_f32", _p(x), _p(wq), _p(bq), _p(wk), _p(bk), _p(wv), _p(bv), _p(wo), _p(bo),
                  B, L, E, dk, _p(q), _p(k), _p(v), _p(attn), _p(r), _p(yo), _p(out), _stream(),
                  flops=2 * M * E * (2 * dk + 2 * E) + 2 * B * L * L * (dk + E))
        ctx.save_for_backward(x, wq, wk, wv, wo, q, k, v, attn, r, yo)
        ctx.set_materialize_grads(False)       # an unused attention map must not cost a zero-filled [B,L,L] gradient
        ctx.dims = (B, L, E, dk)
        ctx.param_refs = (wq, bq, wk, bk, wv, bv, wo, bo)
        return out.view(B, L, E), attn

    @staticmethod
    def backward(ctx, dout, dattn):
        x, wq, wk, wv, wo, q, k, v, attn, r, yo = ctx.saved_tensors
        B, L, E, dk = ctx.dims
        dev = x.device
        M = B * L
        dout = torch.zeros((M, E), dtype=torch.float32, device=dev) if dout is None else _f32(dout, "dout").reshape(M, E)
        dattn = None if dattn is None else _f32(dattn, "dattn")
        sinks = [_sink(t, ctx.needs_input_grad[1 + i]) for i, t in enumerate(ctx.param_refs)]
        direct = all(s_ is not None for s_ in sinks)
        if direct:
            grads = sinks
        else:
            grads = [torch.empty_like(t) for t in ctx.param_refs]
        dx = torch.empty((M, E), dtype=torch.float32, device=dev)
        nbytes = _lib.load().pzn_attn_block_bwd_workspace_bytes(B, L, E, dk)
        ws = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=dev)
        gq, gbq, gk, gbk, gv, gbv, go, gbo = grads
        with _on(dev):
            _call("pzn_attn_block_bwd_f32", _p(x), _p(wq), _p(wk), _p(wv), _p(wo), _p(q), _p(k), _p(v), _p(attn), _p(r),
                  _p(yo), _p(dout), _p(dattn), B, L, E, dk, _p(ws), _p(dx), _p(gq), _p(gbq), _p(gk), _p(gbk), _p(gv),
                  _p(gbv), _p(go), _p(gbo), int(direct), _stream(),
                  flops=2 * (2 * M * E * (2 * dk + 2 * E)) + 2 * B * L * L * (2 * dk + 2 * E))
        if direct:
            return (dx.view(B, L, E),) + (None,) * 8
        return (dx.view(B, L, E),) + tuple(grads)


def attention_block_supported(x, dk):
    """Shapes the fused block takes (the weight-stationary kernel's domain): else compose it from linear + attention."""
    return x.is_cuda and x.dim() == 3 and x.shape[0] * x.shape[1] >= 4096 and x.shape[2] % 32 == 0 and dk % 32 == 0 \
        and x.shape[1] % 4 == 0 and _lib.load().pzn_gemm_get_precision() != 0


def attention_block(x, wq, bq, wk, bk, wv, bv, wo, bo):
    return _AttentionBlock.apply(x, wq, bq, wk, bk, wv, bv, wo, bo)


def attention_chain_fused_available():
    """The chained kernels run on the bf16 matrix pipe: three planes per operand (fp32 results, default) or, in the opt-in
    bf16 attention mode (pzn_attn_set_precision(1)), one plane (single bf16 MFMAs, fp32 accumulation and softmax) - not with
    the exact-fp32 engine selected."""
    return _lib.load().pzn_gemm_get_precision() != 0


def attention_tile_image_rows(img, F):
    """A register-order tile image the chained kernels pass to each other (u, dq), as rows [M, F] - for checks only:
    [16-row tile][feature tile][g][c][r], feature = 16 ft + 4 g + r (csrc/pzn_mfma16.h, store_tiles16)."""
    M = img.numel() // F
    return img.view(M // 16, F // 16, 4, 16, 4).permute(0, 3, 1, 2, 4).reshape(M, F)


def attention_chain_fused_supported(x, dk, w_out):
    """The chained-kernel path (csrc/attnfused.hip) takes the model's shape only: L = 256, E = 256, dk = 64."""
    return (x.is_cuda and x.dim() == 3 and w_out.shape[1] == 5 * x.shape[2]
            and bool(_lib.load().pzn_attn_fused_supported(x.shape[1], x.shape[2], dk))
            and attention_chain_fused_available())


class _AttnChainFused(torch.autograd.Function):
    """model5_b.py:462-475 for nprob = 1 or 2 encoders in the same launches: the four layerAttention blocks as chained
    matrix-core kernels (pzn_attn_fused_*: no q / k / v / score tensors in memory, one projection + one block launch
    per layer forward, two launches + the weight gradients per layer backward), the running mean of the four maps
    written by the block kernel, then — per encoder — the out projection over the five slices and the max over the
    points exactly as _AttnChainOut does them.
    inputs: nprob, flags (bit 0 clear: `out` is not materialised, an empty placeholder stands in the tuple; bit 1: the map as
    column sums per strip of 16 rows, [B,L/16,L], whose mean over dim 1 IS the mean attention's mean over its rows), then per
    problem x[B,L,E], 4 x (wq,bq,wk,bk,wv,bv,wo,bo), w_out, b_out
    -> per problem (out[B,L,Nout], attention[B,L,L], f_global[B,Nout])"""

    @staticmethod
    def forward(ctx, nprob, flags, *args):
        need_out, strips = bool(flags & 1), bool(flags & 2)
        per = 35
        xs = [_f32(args[per * i], "x") for i in range(nprob)]
        pss = [[_f32(t, "param") for t in args[per * i + 1: per * i + 35]] for i in range(nprob)]
        B, L, E = xs[0].shape
        dk = pss[0][0].shape[0]
        Nout = pss[0][32].shape[0]
        dev = xs[0].device
        M = B * L
        lib = _lib.load()
        wbytes, qkb, vb = lib.pzn_attn_fused_weight_bytes(), lib.pzn_attn_fused_qk_image_bytes(B), lib.pzn_attn_fused_v_image_bytes(B)
        mk = lambda *sh: torch.empty(sh, dtype=torch.float32, device=dev)
        raw = lambda n: torch.empty(n, dtype=torch.uint8, device=dev)
        R = range(nprob)
        with _on(dev):
            st = _stream()
            W = [[raw(wbytes) for _ in range(4)] for _ in R]
            for p in R:      # the four layers' weight planes in one launch per encoder
                _call("pzn_attn_fused_prep_weights_n", 4, *[_ptrs([pss[p][8 * i + j] for i in range(4)]) for j in (0, 2, 4, 6)],
                      _ptrs(W[p]), st)
            maps = [mk(B, L // 16, L) if strips else mk(B, L, L) for _ in R]
            cur = [x.reshape(M, E) for x in xs]
            saved = [[] for _ in R]
            for i in range(4):
                img = [[raw(qkb), raw(qkb), raw(vb)] for _ in R]   # Rp images of q, k, v
                _call("pzn_attn_fused_proj", nprob, _ptrs(cur), _ptrs([W[p][i] for p in R]),
                      _ptrs([pss[p][8 * i + 1] for p in R]), _ptrs([pss[p][8 * i + 3] for p in R]),
                      _ptrs([pss[p][8 * i + 5] for p in R]), B, *[_ptrs([img[p][j] for p in R]) for j in range(3)], st,
                      flops=nprob * 2 * M * E * (2 * dk + E))
                r = [mk(M, E) for _ in R]
                t = [mk(M, E) for _ in R]
                mask = [torch.empty((M, 8), dtype=torch.int32, device=dev) for _ in R]
                lse = [mk(M) for _ in R]
                _call("pzn_attn_fused_fwd", nprob, _ptrs(cur), _ptrs([img[p][0] for p in R]), _ptrs([img[p][1] for p in R]),
                      _ptrs([img[p][2] for p in R]), _ptrs([W[p][i] for p in R]), _ptrs([pss[p][8 * i + 7] for p in R]), B,
                      _ptrs(r), _ptrs(t), _ptrs(mask), _ptrs(maps), _ptrs(lse), int(i > 0) | (2 if strips else 0),
                      0.25 / 16 if strips else 0.25, st,
                      flops=nprob * (2 * M * E * E + 2 * B * L * L * (dk + E)))
                for p in R:
                    saved[p].append((cur[p], t[p], mask[p], lse[p], img[p][0], img[p][1], img[p][2], W[p][i]))
                cur = r
            outs, tosave, empties = [], [], []
            for p in R:
                w_out, b_out = pss[p][32], pss[p][33]
                xsl = [saved[p][1][0], saved[p][2][0], saved[p][3][0], cur[p], xs[p].reshape(M, E)]   # att1..att4, f2f (:466)
                f_global = mk(B, Nout)
                arg = torch.empty((B, Nout), dtype=torch.int32, device=dev)
                y = mk(M, Nout) if need_out else None
                ws_bytes = lib.pzn_outproj_maxpts_workspace_bytes(L, E, 5, Nout)
                fused = False
                if ws_bytes:
                    # :466-475 in one launch (csrc/outproj.hip); `out` only when the caller wants it
                    try:
                        _call("pzn_outproj_maxpts_fwd_f32", _ptrs(xsl), 5, _p(w_out), _p(b_out), B, L, E, Nout, _p(y), _p(f_global),
                              _p(arg), _p(raw(ws_bytes)), st, flops=2 * M * 5 * E * Nout)
                        fused = True
                    except _lib.PznUnsupported:
                        pass
                if not fused:
                    y = mk(M, Nout) if y is None else y
                    for i, xi in enumerate(xsl):
                        linear_cols(xi, w_out, E * i, b_out, i > 0, y)
                    _call("pzn_maxpool_points_fwd_f32", _p(y), B, L, Nout, _p(f_global), _p(arg), st)
                if y is None:         # (a placeholder keeps the output tuple's shape; it carries no data and no gradient)
                    y = f_global.new_empty((0,))
                    outs += [y, maps[p], f_global]
                    empties.append(y)
                else:
                    outs += [y.view(B, L, Nout), maps[p], f_global]
                tosave += [t_ for blk in saved[p] for t_ in blk] + [cur[p]] + pss[p] + [arg]
                if WINNER_CAPTURE is not None:
                    WINNER_CAPTURE.append(("gmax", args[per * p + 33].data_ptr(), arg))
        ctx.save_for_backward(*tosave)
        ctx.nprob = nprob
        ctx.dims = (B, L, E, dk, Nout)
        # the kernels pick the one- or three-plane instantiation from the process-wide precision mode at every launch, and the
        # single-plane projection leaves planes 1 and 2 of its images unwritten: the backward must run in the forward's mode
        ctx.attn_mode = _lib.load().pzn_attn_get_precision()
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(*maps, *empties)
        return tuple(outs)

    @staticmethod
    def backward(ctx, *gout):
        if _lib.load().pzn_attn_get_precision() != ctx.attn_mode:
            raise _lib.PznError("pzn_attn_set_precision() changed between the forward and the backward of an attention chain "
                                f"(forward: mode {ctx.attn_mode}): its bf16-plane images were written for the forward's mode")
        B, L, E, dk, Nout = ctx.dims
        nprob = ctx.nprob
        R = range(nprob)
        per_saved = 32 + 1 + 34 + 1
        T = ctx.saved_tensors
        M = B * L
        dev = T[0].device
        mk = lambda *sh: torch.empty(sh, dtype=torch.float32, device=dev)
        raw = lambda n: torch.empty(n, dtype=torch.uint8, device=dev)
        lib = _lib.load()
        vb = lib.pzn_attn_fused_v_image_bytes(B)
        grads = [None] * (2 + 35 * nprob)
        saved, ps, g, Gs, direct_blk = [], [], [], [], []
        with _on(dev):
            st = _stream()
            for p in R:
                t = T[per_saved * p: per_saved * (p + 1)]
                saved.append([t[8 * i: 8 * i + 8] for i in range(4)])
                att4 = t[32]
                ps.append(t[33:67])
                arg = t[67]
                dy, dfg = gout[3 * p], gout[3 * p + 2]
                w_out, b_out = ps[p][32], ps[p][33]
                base = 2 + 35 * p
                sparse = dy is None and dfg is not None and (5 * E) % 64 == 0 and L <= 600
                if sparse:
                    dfg = _f32(dfg, "df_global")
                else:
                    if dfg is not None:
                        dmax = mk(B, L, Nout)
                        _call("pzn_maxpool_points_bwd_f32", _p(_f32(dfg, "df_global")), _p(arg), B, L, Nout, _p(dmax), st)
                        dy = dmax if dy is None else dy + dmax
                    if dy is None:
                        dy = torch.zeros((M, Nout), dtype=torch.float32, device=dev)
                    dy = _f32(dy, "dy").reshape(M, Nout)
                xsl = [saved[p][1][0], saved[p][2][0], saved[p][3][0], att4, saved[p][0][0]]
                sink_w = _sink(w_out, ctx.needs_input_grad[base + 33])
                sink_b = _sink(b_out, ctx.needs_input_grad[base + 34])
                direct_out = sink_w is not None and sink_b is not None
                dW_out = sink_w if direct_out else torch.zeros_like(w_out)
                db_out = sink_b if direct_out else torch.zeros_like(b_out)
                G = mk(M, 5 * E)
                if sparse:
                    segs = (ctypes.c_void_p * 5)(*[_p(xi) for xi in xsl])
                    _call("pzn_linear_maxpts_wgrad_f32", _p(dfg), _p(arg), segs, 5, E, B, L, Nout, _p(dW_out), _p(db_out), st)
                    mws = torch.empty((lib.pzn_linear_maxpts_workspace_bytes(B, Nout) + 3) // 4, dtype=torch.int32, device=dev)
                    _call("pzn_linear_maxpts_dgrad_f32", _p(dfg), _p(arg), _p(w_out), B, L, 5 * E, Nout, _p(mws), _p(G), st)
                else:
                    for i, xi in enumerate(xsl):
                        _call("pzn_linear_slice_wgrad_f32", _p(dy), _p(xi), M, E, Nout, dW_out.data_ptr() + 4 * E * i, 5 * E,
                              _p(db_out) if i == 0 else None, st, flops=2 * M * E * Nout)
                    _call("pzn_linear_dgrad_f32", _p(dy), None, _p(w_out), M, 5 * E, Nout, None, _p(G), st,
                          flops=2 * M * 5 * E * Nout)
                if not direct_out:
                    grads[base + 33], grads[base + 34] = dW_out, db_out
                Gs.append(G)
                g.append(G[:, 3 * E: 4 * E])          # gradient of att4: its slice of the projection only (read in place)
            # scratch of the block backward, shared by the four layers
            dz, u, dx = [mk(M, E) for _ in R], [mk(M, E) for _ in R], [mk(M, E) for _ in R]
            dq, dkk, dvv = [mk(M, dk) for _ in R], [mk(M, dk) for _ in R], [mk(M, E) for _ in R]
            dqt = [mk(M, dk) for _ in R]          # dq once more in the kernels' tile order (query side -> key side)
            darp, delta = [raw(vb) for _ in R], [mk(M) for _ in R]
            g2 = None
            for i in (3, 2, 1, 0):
                blk = [saved[p][i] for p in R]        # (x, t, mask, lse, qrp, krp, vrp, W)
                col = lambda j: _ptrs([b[j] for b in blk])
                # the block's output gradient = its slice of the projection's input gradient (+ what the next block passed
                # back): both read in place by the kernel, no copy and no tensor add
                _call("pzn_attn_fused_bwd_q", nprob, _ptrs(g), 5 * E, _ptrs(g2) if g2 is not None else None, E,
                      col(2), col(4), col(5), col(6), col(7), B, _ptrs(dz),
                      _ptrs(u), _ptrs(dq), _ptrs(dqt), _ptrs(darp), _ptrs(delta), st,
                      flops=nprob * (2 * M * E * (E + dk) + 2 * B * L * L * (2 * dk + E)))
                _call("pzn_attn_fused_bwd_k", nprob, col(4), col(5), col(6), _ptrs(darp), col(7), col(3),
                      _ptrs(delta), _ptrs(u), _ptrs(dqt), B, _ptrs(dkk), _ptrs(dvv), _ptrs(dx), st,
                      flops=nprob * (2 * M * E * (E + dk) + 2 * B * L * L * (2 * dk + 2 * E)))
                for p in R:
                    base = 2 + 35 * p
                    prm = ps[p][8 * i: 8 * i + 8]
                    sinks = [_sink(p_, ctx.needs_input_grad[base + 1 + 8 * i + j]) for j, p_ in enumerate(prm)]
                    direct = all(s_ is not None for s_ in sinks)
                    gp = sinks if direct else [torch.empty_like(p_) for p_ in prm]
                    gq, gbq, gk, gbk, gv, gbv, go, gbo = gp
                    _call("pzn_attn_fused_wgrads", _p(dz[p]), _p(blk[p][1]), _p(dq[p]), _p(dkk[p]), _p(dvv[p]), _p(blk[p][0]),
                          M, E, dk, _p(gq), _p(gbq), _p(gk), _p(gbk), _p(gv), _p(gbv), _p(go), _p(gbo), int(direct), st,
                          flops=2 * M * E * (2 * dk + 2 * E))
                    if not direct:
                        grads[base + 1 + 8 * i: base + 9 + 8 * i] = gp
                sl = i - 1 if i > 0 else 4            # att_i sits in slice i-1 of the concatenation, f2f in slice 4
                g = [Gs[p][:, sl * E: (sl + 1) * E] for p in R]
                g2, dx = dx, [mk(M, E) for _ in R] if i > 0 else dx      # (dx of this block is the next one's second addend)
            for p in R:
                grads[2 + 35 * p] = torch.add(g[p], g2[p]).view(B, L, E)
        return tuple(grads)


class _AttnChainOne(torch.autograd.Function):
    """model5_b.py:462-475 of ONE encoder behind one C entry point each way (csrc/attnchain.hip: the kernels of
    _AttnChainFused, enqueued by the library on one caller-owned buffer per direction) for the case predict5 creates: `out` is
    not wanted and only f_global = max over the points carries a gradient.  inputs: strips flag, x[B,L,E], the 34 parameters
    -> (mean map [B,L,L] or its strip column sums [B,L/16,L], f_global[B,Nout])."""

    @staticmethod
    def forward(ctx, strips, x, *params):
        x = _f32(x, "x")
        ps = [_f32(t, "param") for t in params]
        B, L, E = x.shape
        Nout = ps[32].shape[0]
        dev = x.device
        lib = _lib.load()
        amap = torch.empty((B, L // 16, L) if strips else (B, L, L), dtype=torch.float32, device=dev)
        f_global = torch.empty((B, Nout), dtype=torch.float32, device=dev)
        arg = torch.empty((B, Nout), dtype=torch.int32, device=dev)
        saved = torch.empty((lib.pzn_attn_chain_saved_bytes(B),), dtype=torch.uint8, device=dev)
        with _on(dev):
            _call("pzn_attn_chain_fwd_f32", _p(x), _ptrs(ps), B, int(bool(strips)), _p(amap), None, _p(f_global), _p(arg),
                  _p(saved), _stream(),
                  flops=4 * (2 * B * L * E * (2 * (E // 4) + E) + 2 * B * L * E * E + 2 * B * L * L * (E // 4 + E)) + 2 * B * L * 5 * E * Nout)
        if WINNER_CAPTURE is not None:
            WINNER_CAPTURE.append(("gmax", params[32].data_ptr(), arg))
        ctx.save_for_backward(x, saved, arg, *ps)
        ctx.attn_mode = lib.pzn_attn_get_precision()
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(amap)
        return amap, f_global

    @staticmethod
    def backward(ctx, _dmap, dfg):
        lib = _lib.load()
        if lib.pzn_attn_get_precision() != ctx.attn_mode:
            raise _lib.PznError("pzn_attn_set_precision() changed between the forward and the backward of an attention chain "
                                f"(forward: mode {ctx.attn_mode}): its bf16-plane images were written for the forward's mode")
        x, saved, arg = ctx.saved_tensors[:3]
        ps = list(ctx.saved_tensors[3:])
        if dfg is None:
            return (None,) * 36
        B, L, E = x.shape
        dev = x.device
        dfg = _f32(dfg, "df_global")
        sinks = [_sink(p_, ctx.needs_input_grad[2 + j]) for j, p_ in enumerate(ps)]
        direct = all(s_ is not None for s_ in sinks)
        if direct:
            gp = sinks
        else:      # (the out projection's sparse backward ADDS: zero-initialised; the blocks' gradients are overwritten)
            gp = [torch.empty_like(p_) for p_ in ps[:32]] + [torch.zeros_like(ps[32]), torch.zeros_like(ps[33])]
        dx = torch.empty((B, L, E), dtype=torch.float32, device=dev)
        scratch = torch.empty((lib.pzn_attn_chain_scratch_bytes(B),), dtype=torch.uint8, device=dev)
        with _on(dev):
            _call("pzn_attn_chain_bwd_f32", _p(x), _ptrs(ps), _p(saved), _p(arg), _p(dfg), B, _ptrs(gp), int(direct), _p(dx),
                  _p(scratch), _stream())
        if direct:
            return (None, dx) + (None,) * 34
        return (None, dx) + tuple(gp)


def attention_chain_one_supported(x, dk, w_out):
    """The shape the one-call chain takes: the encoder's (256 points, E = 256, dk = 64, a 1280 -> 1024 out projection) on the
    split-precision matrix-core path, 16-byte aligned."""
    return (attention_chain_fused_supported(x, dk, w_out) and tuple(w_out.shape) == (1024, 1280) and
            _lib.load().pzn_outproj_maxpts_workspace_bytes(256, 256, 5, 1024) > 0 and _lib.load().pzn_gemm_get_precision() != 0)


def attention_chain_fused(xs, blocks_list, w_outs, b_outs, need_out=True, map_strips=False):
    """xs: list of nprob inputs [B,L,E]; blocks_list[p]: four 8-tuples; -> list of (out, mean map, f_global) per problem.
    need_out=False: only f_global = max over the points of the out projection is wanted (predict5, model5_b.py:723);
    `out` is then None and its 67 MB per encoder at B = 64 are never written.
    map_strips=True: the caller only takes the mean of the mean map over its rows (training_step, model5_b.py:937-942): the
    second result is [B,L/16,L], each row the scaled column sums of a strip of 16 query rows, with
    result.mean(dim=1) == mean_map.mean(dim=1); the [B,L,L] map (16.7 MB read + written per block and encoder) never exists."""
    if not need_out and not KernelTimer.enabled and all(
            attention_chain_one_supported(x, blocks[0][0].shape[0], w) for x, blocks, w in zip(xs, blocks_list, w_outs)):
        # what predict5 asks for (only the maximum of the projection): one C call per encoder and direction.  (With the
        # entry-point timer on - bench.py's `stages` - the chain is composed here, so that every kernel's entry point is timed.)
        res = []
        for x, blocks, w, b in zip(xs, blocks_list, w_outs, b_outs):
            amap, fg = _AttnChainOne.apply(bool(map_strips), x, *[p_ for blk in blocks for p_ in blk], w, b)
            res.append((None, amap, fg))
        return res
    flat = []
    for x, blocks, w, b in zip(xs, blocks_list, w_outs, b_outs):
        flat += [x] + [p_ for blk in blocks for p_ in blk] + [w, b]
    res = _AttnChainFused.apply(len(xs), int(bool(need_out)) | (2 if map_strips else 0), *flat)
    return [(res[3 * i] if res[3 * i].numel() else None, res[3 * i + 1], res[3 * i + 2]) for i in range(len(xs))]


class _BnPointsRelu(torch.autograd.Function):
    """relu(BatchNorm1d(num_points)(x)) for x[B, N, C] (model5_b.py:424, :447-448: the BN channel axis is the point
    index) as one launch each way (csrc/bnpoints.hip) instead of BN + clamp and their two backward kernels."""

    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var, training, momentum, eps):
        x = _f32(x, "x")
        B, N, C = x.shape
        dev = x.device
        y = torch.empty_like(x)
        mean = torch.empty((N,), dtype=torch.float32, device=dev)
        invstd = torch.empty((N,), dtype=torch.float32, device=dev)
        with _on(dev):
            _call("pzn_bn_points_relu_fwd_f32", _p(x), _p(weight), _p(bias), _p(running_mean), _p(running_var),
                  int(bool(training)), float(momentum), float(eps), B, N, C, _p(y), _p(mean), _p(invstd), _stream())
        ctx.save_for_backward(x, weight, bias, mean, invstd)
        ctx.training = bool(training)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight, bias, mean, invstd = ctx.saved_tensors
        B, N, C = x.shape
        dy = _f32(dy, "dy")
        dev = dy.device
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        need_w = weight is not None and ctx.needs_input_grad[1]
        need_b = bias is not None and ctx.needs_input_grad[2]
        sw, sb = _sink(weight, need_w), _sink(bias, need_b)
        direct = (sw is not None or not need_w) and (sb is not None or not need_b)
        if direct:
            dw, db = sw, sb
        else:
            dw = torch.zeros((N,), dtype=torch.float32, device=dev) if need_w else None
            db = torch.zeros((N,), dtype=torch.float32, device=dev) if need_b else None
        with _on(dev):
            _call("pzn_bn_points_relu_bwd_f32", _p(x), _p(dy), _p(weight), _p(bias), _p(mean), _p(invstd),
                  int(ctx.training), B, N, C, _p(dx), _p(dw), _p(db), _stream())
        if direct:
            return dx, None, None, None, None, None, None, None
        return dx, dw, db, None, None, None, None, None


def bn_points_relu(x, bn):
    """relu(bn(x)) for an nn.BatchNorm1d(num_points) applied to x[B, N, C] on the GPU: batch statistics and running
    buffers exactly as the module keeps them (momentum must be a number, as in the reference)."""
    if x.dim() != 3 or x.shape[1] != bn.num_features or bn.momentum is None:
        raise _lib.PznError(f"bn_points_relu: x{tuple(x.shape)} vs BatchNorm1d({bn.num_features}), momentum={bn.momentum}")
    use_batch = bn.training or not bn.track_running_stats
    rm = bn.running_mean if bn.track_running_stats else None
    rv = bn.running_var if bn.track_running_stats else None
    if bn.training and bn.track_running_stats and bn.num_batches_tracked is not None:
        bn.num_batches_tracked.add_(1)
    return _BnPointsRelu.apply(x, bn.weight, bn.bias, rm, rv, use_batch, bn.momentum, bn.eps)


class _StemFused(torch.autograd.Function):
    """model5_b.py:447-448 in one launch each way (csrc/stem.hip): relu(bn2(mlp2(relu(bn1(mlp1(xyz)))))) with both
    BatchNorm1d(num_points) over the point axis; the backward recomputes every activation from xyz and the saved statistics."""

    @staticmethod
    def forward(ctx, xyz, w1, b1, g1, o1, w2, b2, g2, o2, rm1, rv1, rm2, rv2, use_batch, mom1, eps1, mom2, eps2, two=False):
        xyz = _f32(xyz, "xyz")
        w1, b1, w2, b2 = _f32(w1, "w1"), _f32(b1, "b1"), _f32(w2, "w2"), _f32(b2, "b2")
        B, N, _ = xyz.shape
        dev = xyz.device
        out = torch.empty((B, N, 64), dtype=torch.float32, device=dev)
        stats = torch.empty((4, N), dtype=torch.float32, device=dev)
        with _on(dev):
            _call("pzn_stem_fwd_f32", _p(xyz), _p(w1), _p(b1), _p(g1), _p(o1), _p(rm1), _p(rv1), float(mom1), float(eps1),
                  _p(w2), _p(b2), _p(g2), _p(o2), _p(rm2), _p(rv2), float(mom2), float(eps2), int(bool(use_batch)), B, N,
                  _p(out), _p(stats[0]), _p(stats[1]), _p(stats[2]), _p(stats[3]), _stream(),
                  flops=2 * B * N * 64 * (3 + 64))
        ctx.save_for_backward(xyz, w1, b1, g1, o1, w2, b2, g2, o2, stats)
        ctx.param_refs = (w1, b1, g1, o1, w2, b2, g2, o2)
        ctx.use_batch = bool(use_batch)
        ctx.set_materialize_grads(False)
        if two:      # the same features under two names: each consumer's gradient arrives on its own and the kernel adds them
            return out, out.view_as(out)
        return out

    @staticmethod
    def backward(ctx, dout, dout2=None):
        xyz, w1, b1, g1, o1, w2, b2, g2, o2, stats = ctx.saved_tensors
        if ctx.needs_input_grad[0]:
            raise _lib.PznError("stem: gradients w.r.t. point coordinates are not provided on the fused stem; "
                                "use ops.linear + ops.bn_points_relu")
        if dout is None:
            dout, dout2 = dout2, None
        if dout is None:
            return (None,) * 19
        B, N, _ = xyz.shape
        dout = _f32(dout, "dout")
        dout2 = None if dout2 is None else _f32(dout2, "dout2")
        dev = dout.device
        params = (w1, b1, g1, o1, w2, b2, g2, o2)
        sinks = [None if t is None else _sink(t, ctx.needs_input_grad[1 + i]) for i, t in enumerate(params)]
        direct = all(s_ is not None or t is None for s_, t in zip(sinks, params))
        if direct:
            grads = sinks
        else:
            grads = [None if t is None else torch.zeros_like(t) for t in params]      # the kernel adds into these
        dw1, db1, dg1, do1, dw2, db2, dg2, do2 = grads
        ws = torch.empty((_lib.load().pzn_stem_bwd_workspace_bytes(N) + 3) // 4, dtype=torch.float32, device=dev)
        with _on(dev):
            _call("pzn_stem_bwd_f32", _p(xyz), _p(dout), _p(dout2), _p(w1), _p(b1), _p(w2), _p(b2), _p(g1), _p(o1), _p(g2), _p(o2),
                  _p(stats[0]), _p(stats[1]), _p(stats[2]), _p(stats[3]), int(ctx.use_batch), B, N, _p(dw1), _p(db1),
                  _p(dw2), _p(db2), _p(dg1), _p(do1), _p(dg2), _p(do2), _p(ws), _stream(), flops=2 * B * N * 64 * (3 + 3 * 64))
        if direct:
            return (None,) * 19
        return (None, dw1, db1, dg1, do1, dw2, db2, dg2, do2) + (None,) * 10


def stem_supported(xyz, lin1, bn1, lin2, bn2):
    return (xyz.is_cuda and xyz.dim() == 3 and xyz.shape[2] == 3 and xyz.shape[0] <= 64 and not xyz.requires_grad and
            tuple(lin1.weight.shape) == (64, 3) and tuple(lin2.weight.shape) == (64, 64) and lin1.bias is not None and
            lin2.bias is not None and bn1.num_features == xyz.shape[1] == bn2.num_features and bn1.momentum is not None and
            bn2.momentum is not None and bn1.training == bn2.training and bn1.track_running_stats == bn2.track_running_stats)


def stem(xyz, lin1, bn1, lin2, bn2, two=False):
    """relu(bn2(lin2(relu(bn1(lin1(xyz)))))) for the encoder's shapes (stem_supported); the modules' running buffers are kept
    exactly as the modules keep them.  two=True: -> (features, the same features under a second name): hand each of two consumers
    its own name and their gradients are added inside the backward launch instead of by autograd's pass over two 33.5 MB
    tensors."""
    use_batch = bn1.training or not bn1.track_running_stats
    track = bn1.track_running_stats
    for bn in (bn1, bn2):
        if bn.training and track and bn.num_batches_tracked is not None:
            bn.num_batches_tracked.add_(1)
    return _StemFused.apply(xyz, lin1.weight, lin1.bias, bn1.weight, bn1.bias, lin2.weight, lin2.bias, bn2.weight, bn2.bias,
                            bn1.running_mean if track else None, bn1.running_var if track else None,
                            bn2.running_mean if track else None, bn2.running_var if track else None,
                            use_batch, bn1.momentum, bn1.eps, bn2.momentum, bn2.eps, bool(two))


class _SaLevelFused(torch.autograd.Function):
    """The set-abstraction level (model5_b.py:449-454 / :456-461) with the first layer per point and its rows never in
    memory: W1[:,0:3] (xyz[j] - centre) is split into a per-point and a per-group part, so a grouped row is
    relu(Pp[idx] + Q[group]) with Pp = feat W1[:,3:]^T + W1[:,0:3] xyz and Q = b1 - W1[:,0:3] centre; the rows are generated
    inside the matrix-core kernel's operand loader forward and inside the backward passes (weight gradients of the pooled
    layer, walk by point).  Same result as group + shared_mlp_max up to the order of the fp32 sum; no h tensor (537 MB per
    level and cloud at B = 64).  One C entry point each way (csrc/sachain.hip) on one buffer per direction; with the
    entry-point timer on the same launches are made one by one from here."""

    @staticmethod
    def forward(ctx, xyz, feat, new_xyz, idx, w1, b1, w2, b2):
        xyz, feat, new_xyz = _f32(xyz, "xyz"), _f32(feat, "points"), _f32(new_xyz, "new_xyz")
        idx = None if idx is None else _i64(idx, "idx")
        w1, b1, w2, b2 = _f32(w1, "w1"), _f32(b1, "b1"), _f32(w2, "w2"), _f32(b2, "b2")
        B, N, _ = xyz.shape
        S = new_xyz.shape[1]
        D = feat.shape[-1]
        C1, C2 = w1.shape[0], w2.shape[0]
        dev = xyz.device
        R = B * S
        lib = _lib.load()
        out = torch.empty((R, C2), dtype=torch.float32, device=dev)
        arg = torch.empty((R, C2), dtype=torch.int32, device=dev)
        ctx.stepwise = KernelTimer.enabled
        if ctx.stepwise:
            saved = _SaLevelFused._forward_stepwise(xyz, feat, new_xyz, idx, w1, b1, w2, b2, out, arg)
        else:
            saved = (torch.empty((lib.pzn_sa_level_chain_saved_bytes(B, N, S, D, C1, C2),), dtype=torch.uint8, device=dev),)
            with _on(dev):
                _call("pzn_sa_level_chain_fwd_f32", _p(xyz), _p(feat), _p(new_xyz), _p(idx), _p(w1), _p(b1), _p(w2), _p(b2),
                      B, N, S, D, C1, C2, _p(out), _p(arg), _p(saved[0]), _stream())
        if WINNER_CAPTURE is not None:
            WINNER_CAPTURE.append(("sa", w2.data_ptr(), arg.view(B, S, C2)))
        ctx.have_idx = idx is not None
        ctx.save_for_backward(xyz, feat, new_xyz, idx if idx is not None else xyz.new_empty(0), w1, w2, out, arg, *saved)
        ctx.dims = (B, N, S, D, R, C1, C2)
        ctx.param_refs = (w1, b1, w2, b2)
        return out.reshape(B, S, C2)

    @staticmethod
    def _forward_stepwise(xyz, feat, new_xyz, idx, w1, b1, w2, b2, out, arg):
        """The forward's launches one entry point at a time (bench.py's `stages`) -> (idx, w_f, P, Q) for the backward."""
        B, N, _ = xyz.shape
        S, D, C1, C2 = new_xyz.shape[1], feat.shape[-1], w1.shape[0], w2.shape[0]
        dev, R = xyz.device, B * new_xyz.shape[1]
        w_f = w1[:, 3:].contiguous()
        P = torch.empty((B * N, C1), dtype=torch.float32, device=dev)
        Q = torch.empty((R, C1), dtype=torch.float32, device=dev)
        with _on(dev):
            _call("pzn_linear_fwd_f32", _p(feat), _p(w_f), None, B * N, D, C1, 0, _p(P), _stream(), flops=2 * B * N * D * C1)
            if idx is None:
                idx = torch.empty((B, S, 32), dtype=torch.int64, device=dev)
                _call("pzn_knn_f32", _p(xyz), _p(new_xyz), B, N, S, 32, _p(idx), _stream())
            _call("pzn_sa_prep_f32", _p(xyz), _p(new_xyz), _p(w1), _p(b1), B, N, S, D, C1, _p(P), _p(Q), _stream())
            ws_bytes = _lib.load().pzn_sa_level_fwd_workspace_bytes(C1, C2)
            ws = torch.empty((max(ws_bytes, 16),), dtype=torch.uint8, device=dev)
            done = False
            if ws_bytes:      # streamed-weights kernel: the weight split and the level as two entry points
                try:
                    _call("pzn_sa_level_prep_weights_f32", _p(w2), C1, C2, _p(ws), _stream())
                    _call("pzn_sa_level_fwd_packed_f32", _p(P), _p(Q), _p(idx), _p(b2), B, N, S, C1, C2, _p(out), _p(arg),
                          _p(ws), _stream(), flops=2 * R * 32 * C1 * C2, variant=f"<{C1}, {C2 // 32}>")
                    done = True
                except _lib.PznUnsupported:
                    pass
            if not done:
                _call("pzn_sa_level_fwd_ws_f32", _p(P), _p(Q), _p(idx), _p(w2), _p(b2), B, N, S, C1, C2, _p(out), _p(arg),
                      _p(ws), _stream(), flops=2 * R * 32 * C1 * C2)
        return idx, w_f, P, Q

    @staticmethod
    def backward(ctx, dout):
        xyz, feat, new_xyz, idx, w1, w2, out, arg = ctx.saved_tensors[:8]
        B, N, S, D, R, C1, C2 = ctx.dims
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[2]:
            raise _lib.PznError("sa_mlp_max: gradients w.r.t. point coordinates are not provided on the fused "
                                "encoder path; use pointnet_util.sample_and_group + ops.shared_mlp_max")
        dout = _f32(dout, "dout").reshape(R, C2)
        dev = dout.device
        need_feat = ctx.needs_input_grad[1]
        sinks = [_sink(t, ctx.needs_input_grad[4 + i]) for i, t in enumerate(ctx.param_refs)]
        direct = all(s_ is not None for s_ in sinks)
        if direct:
            dW1, db1, dW2, db2 = sinks
        else:      # (the stepwise kernels ADD into dW1 / db1: zero-filled here; the one-call form fills them itself)
            mk1 = torch.zeros if ctx.stepwise else torch.empty
            dW1 = mk1((C1, 3 + D), dtype=torch.float32, device=dev)
            db1 = mk1((C1,), dtype=torch.float32, device=dev)
            dW2 = torch.empty_like(w2)
            db2 = torch.empty((C2,), dtype=torch.float32, device=dev)
        dfeat = torch.empty((B, N, D), dtype=torch.float32, device=dev) if need_feat else None
        lib = _lib.load()
        if not ctx.stepwise:
            saved = ctx.saved_tensors[8]
            scratch = torch.empty((lib.pzn_sa_level_chain_scratch_bytes(B, N, S, C1, C2),), dtype=torch.uint8, device=dev)
            with _on(dev):
                _call("pzn_sa_level_chain_bwd_f32", _p(dout), _p(arg), _p(out), _p(xyz), _p(feat), _p(new_xyz),
                      _p(idx) if ctx.have_idx else None, _p(w1), _p(w2), _p(saved), B, N, S, D, C1, C2, _p(dfeat), _p(dW1),
                      _p(db1), _p(dW2), _p(db2), int(direct), _p(scratch), _stream())
        else:
            idx_s, w_f, P, Q = ctx.saved_tensors[8:12]
            off = torch.empty((B * (N + 1),), dtype=torch.int32, device=dev)
            rows = torch.empty((B * S * 32,), dtype=torch.int32, device=dev)
            pts = torch.empty((B * S * 32,), dtype=torch.int32, device=dev)
            dP = torch.empty((B * N, C1), dtype=torch.float32, device=dev)
            with _on(dev):
                _call("pzn_knn_inverse_lists", _p(idx_s), B, N, S, 32, _p(off), _p(rows), _p(pts), _stream())
                ws = torch.empty((lib.pzn_sa_level_bwd_pt_workspace_bytes(B, S, C2) + 3) // 4, dtype=torch.float32, device=dev)
                _call("pzn_sa_level_bwd_pt_f32", _p(dout), _p(arg), _p(out), _p(w2), _p(P), _p(Q), _p(idx_s), _p(xyz), _p(new_xyz),
                      _p(off), _p(rows), _p(pts), B, N, S, D, C1, C2, _p(dP), _p(dW2), _p(db2), _p(dW1), _p(db1), int(direct),
                      _p(ws), _stream(), flops=2 * R * (2 * C1 * C2))
                if need_feat:
                    _call("pzn_linear_dgrad_f32", _p(dP), None, _p(w_f), B * N, D, C1, None, _p(dfeat), _stream(),
                          flops=2 * B * N * D * C1)
                _call("pzn_linear_slice_wgrad_f32", _p(dP), _p(feat), B * N, D, C1, dW1.data_ptr() + 12, 3 + D, None, _stream(),
                      flops=2 * B * N * D * C1)
        if direct:
            return None, dfeat, None, None, None, None, None, None
        return None, dfeat, None, None, dW1, db1, dW2, db2


def sa_level_fused_supported(feat, idx, w1, w2):
    """The shapes the per-point set-abstraction kernels take, decided BEFORE anything is launched (forward: pzn_sa_prep_f32 +
    pzn_sa_level_fwd_*; backward: pzn_sa_level_bwd_pt_f32): 32 neighbours, a first layer of 128 or 256 channels over
    [xyz | features], a second layer of 64 / 128 / 256 channels, the split-precision matrix-core path."""
    K = 32 if idx is None else idx.shape[2]
    return (K == 32 and w1.shape[0] in (128, 256) and w1.shape[1] == 3 + feat.shape[-1] and w2.shape[0] in (64, 128, 256)
            and w2.shape[1] == w1.shape[0] and _lib.load().pzn_gemm_get_precision() != 0)


def sa_mlp_max(xyz, feat, new_xyz, idx, w1, b1, w2, b2):
    """sample_and_group(.., knn=True)'s grouping (pointnet_util.py:117-132) + relu(lin_a) + relu(lin_b) + max over the
    neighbours (model5_b.py:449-454 / :456-461) for given centroids.  The encoder's shapes run per point with no grouped tensor
    in memory (_SaLevelFused); anything else is composed as the reference composes it: the [B,S,K,3+D] group tensor (search
    fused with the group write when idx is None) and the shared MLP + max on its rows."""
    if sa_level_fused_supported(feat, idx, w1, w2):
        try:
            return _SaLevelFused.apply(xyz, feat, new_xyz, idx, w1, b1, w2, b2)
        except _lib.PznUnsupported:
            pass        # a table beyond the 32-bit buffer offsets: the composed form below
    if idx is None and knn_group_supported(xyz, feat, 32):
        grouped = knn_group(xyz, feat, new_xyz)[0]
    else:
        grouped = group(xyz, feat, new_xyz, knn(xyz, new_xyz, 32) if idx is None else idx)
    return shared_mlp_max(grouped, w1, b1, w2, b2)
