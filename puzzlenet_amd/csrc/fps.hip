// fps.hip — farthest point sampling for gfx950.
//
// Replaces pointnet_util.farthest_point_sample (pointnet_util.py:53-73): a
// Python loop of npoint iterations x 5 torch ops.  Here one workgroup owns one
// cloud for the whole loop:
//   * the cloud is read from HBM exactly once and each thread keeps PPT points
//     + their running min-distance in registers for all iterations;
//   * per iteration (pzn_fps_round.h, the definition mergefps.hip shares):
//     distance update in registers, arg-max of key = (dist_bits << 32) | ~index
//     within the wavefront, one LDS slot per wave, one barrier, every wave
//     re-reduces the <=16 slots redundantly; the pick goes to a buffer in LDS
//     that leaves in chunks;
//   * slots are double-buffered on the iteration parity, so one barrier per
//     iteration is enough.
// Two forms.  IMAGE (use_lds): a coalesced flat copy of the (N,3) AoS rows
// into an SoA image in LDS, from which the registers are filled and every
// round's centroid is fetched; the round is pzn_fps_round.h's as it stands.
// PUBLISHED (no image; PPT >= 8): the registers are filled from memory, held
// as packed pairs, and every wavefront publishes its best point's coordinates
// beside its key, so the next round's centroid comes out of LDS as well; its
// packed-pair arg-max is this file's own, the cross-wavefront step and the
// pick buffer are the shared ones.
// The loop is latency-bound by construction (npoint dependent rounds); the
// launch is B workgroups, i.e. parallel over clouds only.
#include <stdlib.h>

#include <type_traits>

#include "pzn_common.h"

namespace {

#include "pzn_fps_round.h"

typedef float v2f __attribute__((ext_vector_type(2)));

// f(0), f(1), ... while q < n, q < Q1, as NESTED ifs on compile-time q: the first failing guard jumps past all the rest (an
// unrolled loop with one guard per body jumps over every unused body in turn; with `break` the loop is not unrolled at all and
// the register arrays are indexed dynamically)
template <int Q, int Q1, typename F>
__device__ __forceinline__ void nested_while_below(int n, F&& f) {
  if constexpr (Q < Q1) {
    if (Q < n) {
      f(std::integral_constant<int, Q>{});
      nested_while_below<Q + 1, Q1>(n, f);
    }
  }
}

// f(q) for the one compile-time q in [Q, Q1) that equals the (wavefront-uniform) n
template <int Q, int Q1, typename F>
__device__ __forceinline__ void uniform_pick(int n, F&& f) {
  if constexpr (Q < Q1) {
    if (n == Q)
      f(std::integral_constant<int, Q>{});
    else
      uniform_pick<Q + 1, Q1>(n, f);
  }
}

constexpr size_t FPS_IMAGE_MAX_LDS = 150 * 1024;      // the most LDS a workgroup takes for head + image

// use_lds: the cloud's SoA image is in LDS, else published coordinates (compile-time: with a run-time choice the centroid
// fetch became three flat_load instructions waited for with vmcnt(0) lgkmcnt(0) in the middle of every round's dependent chain)
// G clouds per workgroup (T threads each; cloud blockIdx.x + g gridDim.x): the background form packs the two pieces of a cut
// into one workgroup - they share nothing but the barrier of a round -, so that the loader holds half as many CUs beside a
// training step (two or four such 4-wavefront groups on a CU run as fast as one: the round is a latency chain).
// counts: published form only (the image form serves pzn_fps_f32, which has none, and takes N <= T PPT points, all real).
template <int T, int PPT, bool use_lds, int G = 1>
__global__ __launch_bounds__(T * G) void fps_kernel(const float* __restrict__ xyz, int N, int npoint,
                                                    const int64_t* __restrict__ start,
                                                    int64_t* __restrict__ out, const int64_t* __restrict__ counts, int lds_per_cloud) {
  static_assert(use_lds ? G == 1 : PPT > 4 && PPT % 2 == 0, "the published form holds its points as register pairs");
  constexpr int W = T / PZN_WAVE;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_all[];
  const int grp = G > 1 ? __builtin_amdgcn_readfirstlane((int)threadIdx.x / T) : 0;
  unsigned char* smem_raw = smem_all + (size_t)grp * lds_per_cloud;
  uint64_t* slots = reinterpret_cast<uint64_t*>(smem_raw);             // [2][W]
  int* sout = reinterpret_cast<int*>(smem_raw + 2 * W * sizeof(uint64_t));      // [FPS_OUT_CHUNK] picks not yet written out

  const int b = blockIdx.x + grp * gridDim.x;
  const int tid = G > 1 ? (int)threadIdx.x - grp * T : (int)threadIdx.x;
  const int lane = tid & (PZN_WAVE - 1);
  const int wave = tid / PZN_WAVE;
  const float* g = xyz + (size_t)b * N * 3;
  int64_t* o = out + (size_t)b * npoint;
  auto flush = [&](int base, int cnt) {
    for (int t = tid; t < cnt; t += T) o[base + t] = (int64_t)sout[t];
  };

  if constexpr (use_lds) {
    float* sx = reinterpret_cast<float*>(smem_raw + fps_lds_head(W));
    float* sy = sx + N;
    float* sz = sy + N;
    fps_load_soa<T>(g, N, sx, sy, sz, 0, tid);
    __syncthreads();
    float px[PPT], py[PPT], pz[PPT], dist[PPT];
#pragma unroll
    for (int p = 0; p < PPT; ++p) {
      const int j = tid + p * T;
      const bool ok = j < N;
      px[p] = ok ? sx[j] : 0.f;
      py[p] = ok ? sy[j] : 0.f;
      pz[p] = ok ? sz[j] : 0.f;
      dist[p] = 1e10f;  // pointnet_util.py:64
    }
    const int pmax = (N + T - 1) / T;
    const bool full = N == T * PPT;      // every thread's every point exists: no bounds tests in the rounds
    int far = (int)start[b];  // pointnet_util.py:65 (the caller's randint draw)
    far = far < 0 ? 0 : (far >= N ? N - 1 : far);
    for (int i = 0; i < npoint; ++i) {
      fps_buffer_pick(sout, i, npoint, far, tid, flush);      // :68
      const float cx = sx[far], cy = sy[far], cz = sz[far];  // :69
      const uint64_t best = fps_wave_argmax<T, PPT>(px, py, pz, dist, cx, cy, cz, tid, N, pmax, full);
      far = (int)(~(uint32_t)fps_cross_wave<W>(slots, i, lane, wave, best));  // :72
    }
  } else {
    // every wavefront publishes its best point's coordinates beside its key, [2][W] x 16 bytes (the pick's owner has them in
    // registers: no fetch from memory in the round's dependent chain)
    float4* scoord = reinterpret_cast<float4*>(smem_raw + fps_lds_head(W));

    // counts < 0 = a piece that does not exist (the fallback rows of pzn_cut_compact_double_f32): when that holds for every
    // piece of the workgroup it writes index 0 everywhere and leaves before the first barrier, so it holds no CU for npoint rounds
    if (counts) {
      bool skip = true;
#pragma unroll
      for (int q = 0; q < G; ++q) skip = skip && counts[blockIdx.x + q * gridDim.x] < 0;
      if (skip) {      // (workgroup-uniform)
        for (int t = tid; t < npoint; t += T) o[t] = 0;
        return;
      }
    }

    // the points as PAIRS of register slots (2q, 2q + 1): the distance update is packed fp32 - two points per instruction,
    // every operation individually rounded as in sqdist3 (this file is built with -ffp-contract=off) -: with up to 16 slots
    // per thread and 8 wavefronts the round is bound by vector issue, not by its dependent latencies
    constexpr int PQ = PPT / 2;
    v2f qx[PQ], qy[PQ], qz[PQ], qd[PQ];
#pragma unroll
    for (int p = 0; p < PPT; ++p) {
      const int j = tid + p * T;
      const bool ok = j < N;
      // (a slot without a point: distance 0 for ever - it can only tie at 0, and ties go to the lower, i.e. a real, index)
      qx[p >> 1][p & 1] = ok ? g[(size_t)j * 3 + 0] : 0.f;
      qy[p >> 1][p & 1] = ok ? g[(size_t)j * 3 + 1] : 0.f;
      qz[p >> 1][p & 1] = ok ? g[(size_t)j * 3 + 2] : 0.f;
      qd[p >> 1][p & 1] = ok ? 1e10f : 0.f;  // pointnet_util.py:64
    }

    // counts (the data pipeline's padded pieces): only the first counts[b] rows of the cloud are real, the rest are copies of
    // row 0, which can never be picked (distance 0 after the first round at the latest, and any tie goes to the lower index);
    // the rounds then leave out every register slot that holds padding only (a workgroup-uniform bound)
    constexpr int CAP = T * PPT;      // (the background form may hold fewer slots than the buffer has rows: max_count)
    const int nmax = N < CAP ? N : CAP;
    const int nreal = counts ? (int)(counts[b] < 1 ? 1 : (counts[b] > nmax ? nmax : counts[b])) : nmax;
    const int pmax = (nreal + T - 1) / T;
    int far = (int)start[b];  // pointnet_util.py:65 (the caller's randint draw)
    far = far < 0 ? 0 : (far >= N ? N - 1 : far);
    float ncx = 0.f, ncy = 0.f, ncz = 0.f;      // the next round's centroid

    for (int i = 0; i < npoint; ++i) {
      fps_buffer_pick(sout, i, npoint, far, tid, flush);      // :68
      float cx, cy, cz;          // :69
      if (i > 0) {
        cx = ncx, cy = ncy, cz = ncz;      // published by the owner's wavefront in the round before
      } else {
        cx = g[(size_t)far * 3 + 0];
        cy = g[(size_t)far * 3 + 1];
        cz = g[(size_t)far * 3 + 2];
      }
      // packed distances, 32-bit keys with the slot number deferred (as fps_wave_argmax's form for few points): 8 vector
      // instructions per point instead of 13
      // the centroid as three real register pairs (the asm is empty: it only keeps the compiler from broadcasting one half of a
      // pair with op_sel on src1 - the packed form that returns wrong results beside AGPR-accumulator MFMAs, DESIGN.md section 4,
      // tests/test_isa_forms.py)
      v2f c2x = v2f{cx, cx}, c2y = v2f{cy, cy}, c2z = v2f{cz, cz};
      asm volatile("" : "+v"(c2x), "+v"(c2y), "+v"(c2z));
      const int qmax = (pmax + 1) >> 1;      // (workgroup-uniform; an odd pmax evaluates one slot of padding: harmless, see above)
      uint32_t bd = 0, bp = 0;
      nested_while_below<0, PQ>(qmax, [&](auto qc) {
        constexpr int q = decltype(qc)::value;
        const v2f dx = qx[q] - c2x, dy = qy[q] - c2y, dz = qz[q] - c2z;      // :70
        const v2f d = (dx * dx + dy * dy) + dz * dz;
        v2f nd;                                                             // :71
        nd.x = d.x < qd[q].x ? d.x : qd[q].x;
        nd.y = d.y < qd[q].y ? d.y : qd[q].y;
        qd[q] = nd;
        const uint32_t n0 = __float_as_uint(nd.x), n1 = __float_as_uint(nd.y);
        // strict >: the lower slot (= lower index) of equal distances stays; the thread's first slot is always taken
        const bool t0 = q == 0 ? true : n0 > bd;
        bd = t0 ? n0 : bd;
        bp = t0 ? (uint32_t)(2 * q) : bp;
        const bool t1 = n1 > bd;
        bd = t1 ? n1 : bd;
        bp = t1 ? (uint32_t)(2 * q + 1) : bp;
      });
      const uint32_t bj = (uint32_t)tid + bp * (uint32_t)T;
      const uint32_t wm = pzn::wave_max_u32_dpp(bd);
      const bool tied = bd == wm;
      const unsigned long long tmask = __ballot(tied);
      uint32_t wj;
      if (__popcll(tmask) == 1)
        wj = (uint32_t)__builtin_amdgcn_readlane((int)bj, __builtin_ctzll(tmask));
      else
        wj = pzn::wave_min_u32_dpp(tied ? bj : 0xffffffffu);
      const uint64_t best = ((uint64_t)wm << 32) | (uint32_t)(~wj);

      // the wavefront's best point j = tid' + ps T sits in register slot ps (wavefront-uniform) of lane j & 63
      const int ps = __builtin_amdgcn_readfirstlane((int)(wj / T));
      const int qs = ps >> 1;
      // slot pair qs is wavefront-uniform: a chain of scalar compares with ONE taken body instead of six selects per pair on
      // every lane (the empty asm keeps the compiler from turning the bodies back into selects)
      v2f sx2 = qx[0], sy2 = qy[0], sz2 = qz[0];
      uniform_pick<1, PQ>(qs, [&](auto qc) {
        constexpr int q = decltype(qc)::value;
        sx2 = qx[q], sy2 = qy[q], sz2 = qz[q];
        asm volatile("" : "+v"(sx2), "+v"(sy2), "+v"(sz2));
      });
      const bool hi = (ps & 1) != 0;
      const float bx = hi ? sx2.y : sx2.x, by = hi ? sy2.y : sy2.x, bz = hi ? sz2.y : sz2.x;
      const int ol = (int)(wj & (PZN_WAVE - 1));
      const float ox = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, bx), ol));
      const float oy = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, by), ol));
      const float oz = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, bz), ol));
      int mw;
      far = (int)(~(uint32_t)fps_cross_wave<W>(slots, i, lane, wave, best, mw, scoord, make_float4(ox, oy, oz, 0.f)));  // :72
      const float4 c = scoord[(i & 1) * W + mw];
      ncx = c.x, ncy = c.y, ncz = c.z;
    }
  }
}

// the image form: the main entry's, for every cloud whose image fits
template <int T, int PPT>
int launch_image(const float* xyz, int B, int N, int npoint, const int64_t* start, int64_t* out, hipStream_t st) {
  const size_t lds = fps_lds_head(T / PZN_WAVE) + (size_t)3 * N * sizeof(float);
  if (lds > 64 * 1024 &&
      hipFuncSetAttribute(reinterpret_cast<const void*>(&fps_kernel<T, PPT, true>),
                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return PZN_ELAUNCH;
  PZN_LAUNCH((fps_kernel<T, PPT, true>), dim3(B), dim3(T), lds, st, xyz, N, npoint, start, out, nullptr, (int)lds);
  PZN_RETURN_LAUNCH_STATUS();
}

// the published form; with four wavefronts per cloud, clouds b and b + B / 2 (the two pieces of a cut) share a workgroup
template <int T, int PPT>
int launch_published(const float* xyz, int B, int N, int npoint, const int64_t* start, int64_t* out, hipStream_t st,
                     const int64_t* counts) {
  constexpr int W = T / PZN_WAVE;
  const size_t lds = fps_lds_head(W) + 2 * W * sizeof(float4);
  if constexpr (T == 256) {
    if (B % 2 == 0) {
      PZN_LAUNCH((fps_kernel<T, PPT, false, 2>), dim3(B / 2), dim3(2 * T), 2 * lds, st, xyz, N, npoint, start, out, counts, (int)lds);
      PZN_RETURN_LAUNCH_STATUS();
    }
  }
  PZN_LAUNCH((fps_kernel<T, PPT, false>), dim3(B), dim3(T), lds, st, xyz, N, npoint, start, out, counts, (int)lds);
  PZN_RETURN_LAUNCH_STATUS();
}

}  // namespace

// The same sampling as a BACKGROUND job (datapipe.PairFeeder: pieces of up to 32768 raw points sampled on a side stream while
// a training step owns the chip): no LDS image of the cloud - every wavefront publishes its best point's coordinates beside its
// key, so the next round's centroid comes from the owner's registers through 16 bytes of LDS, not from memory -, so
// a workgroup holds 1.5 KB of LDS instead of up to 150 KB and the step's LDS-tiled kernels keep their CUs; 512 threads for
// N <= 16384.  counts (may be NULL): int64 [B], the number of REAL rows of each cloud when the rest is padding with copies of
// row 0 (datapipe._compact): the rounds skip the padding.  Same picks bit for bit (sqdist3's operations in its order,
// each rounded on its own, two points at a time; the tie rule and the cross-wavefront step are the image form's).
PZN_EXPORT int pzn_fps_background_f32(const float* xyz, int B, int N, int npoint, const int64_t* start_idx,
                                      int64_t* out_idx, const int64_t* counts, int max_count, pzn_stream_t stream) {
  PZN_CHECK_ARG(xyz && start_idx && out_idx && B > 0 && N > 0 && npoint > 0 && max_count >= 0);
  hipStream_t st = pzn_hip_stream(stream);
  // Threads x register slots by the number of rows that can be REAL (max_count: the caller's promise counts[b] <= max_count;
  // 0 or no counts: N): four wavefronts wherever the points fit 32 slots - the round's fixed part (wave reductions, barrier,
  // re-reduction of the per-wave slots) grows with the wavefront count: per round on 2048 real points 1.16 us with eight
  // wavefronts against 0.77 with four, and 0.07 us per 512 points either way (tools/bench_fps.py).  Rows at and beyond
  // threads x slots are never looked at (padding by the promise).
  const int cap = (counts && max_count > 0 && max_count < N) ? max_count : N;
  if (cap <= 2048) return launch_published<256, 8>(xyz, B, N, npoint, start_idx, out_idx, st, counts);
  if (cap <= 4096) return launch_published<256, 16>(xyz, B, N, npoint, start_idx, out_idx, st, counts);
  if (cap <= 8192) return launch_published<256, 32>(xyz, B, N, npoint, start_idx, out_idx, st, counts);
  if (cap <= 16384) return launch_published<512, 32>(xyz, B, N, npoint, start_idx, out_idx, st, counts);
  if (cap <= 32768) return launch_published<1024, 32>(xyz, B, N, npoint, start_idx, out_idx, st, counts);
  return PZN_EUNSUPPORTED;
}

PZN_EXPORT int pzn_fps_f32(const float* xyz, int B, int N, int npoint, const int64_t* start_idx,
                           int64_t* out_idx, pzn_stream_t stream) {
  PZN_CHECK_ARG(xyz && start_idx && out_idx && B > 0 && N > 0 && npoint > 0);
  hipStream_t st = pzn_hip_stream(stream);
  // Fewer, fatter wavefronts: the round is a dependent chain (fetch the pick, update, wave reduction, barrier, re-reduce
  // the per-wave slots), and the cross-wave part grows with the wave count while the per-thread update is cheap.  Measured
  // per round at N = 2048: 1024 threads 1.35 us, 512 0.75, 256 0.62 (tools/bench_fps.py)
  if (N <= 64) return launch_image<64, 1>(xyz, B, N, npoint, start_idx, out_idx, st);
  if (N <= 128) return launch_image<128, 1>(xyz, B, N, npoint, start_idx, out_idx, st);
  if (N <= 256) return launch_image<256, 1>(xyz, B, N, npoint, start_idx, out_idx, st);
  if (N <= 512) return launch_image<256, 2>(xyz, B, N, npoint, start_idx, out_idx, st);
  if (N <= 1024) return launch_image<256, 4>(xyz, B, N, npoint, start_idx, out_idx, st);
  if (N <= 2048) return launch_image<256, 8>(xyz, B, N, npoint, start_idx, out_idx, st);
  if (N <= 4096) return launch_image<256, 16>(xyz, B, N, npoint, start_idx, out_idx, st);
  if (N <= 8192) return launch_image<512, 16>(xyz, B, N, npoint, start_idx, out_idx, st);
  if (N <= 16384) {      // the one shape whose image may or may not fit (it does up to N = 12693)
    if (fps_lds_head(1024 / PZN_WAVE) + (size_t)3 * N * sizeof(float) <= FPS_IMAGE_MAX_LDS)
      return launch_image<1024, 16>(xyz, B, N, npoint, start_idx, out_idx, st);
    return launch_published<1024, 16>(xyz, B, N, npoint, start_idx, out_idx, st, nullptr);
  }
  if (N <= 32768) return launch_published<1024, 32>(xyz, B, N, npoint, start_idx, out_idx, st, nullptr);      // never fits
  return PZN_EUNSUPPORTED;
}
