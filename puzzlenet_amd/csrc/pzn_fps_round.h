// pzn_fps_round.h — the one definition of a farthest-point-sampling round, shared by fps.hip (fps_kernel) and mergefps.hip
// (merge_resample_kernel): the SoA load of a cloud, the per-wavefront arg-max over register-held points, the
// cross-wavefront step and the chunked pick buffer.  Tests pin the picks of both kernels bit for bit (and against each
// other), so each of these has this one definition.  Included inside the translation unit's anonymous namespace, after
// pzn_common.h; both translation units are built with -ffp-contract=off -fno-slp-vectorize.
#pragma once

constexpr int FPS_OUT_CHUNK = 256;      // picks buffered in LDS between write-outs (power of two)

// A cloud's LDS starts with the slots [2][W] (uint64) and the pick buffer [FPS_OUT_CHUNK] (int); this many bytes, then
// what the kernel keeps there (an image, published coordinates)
constexpr size_t fps_lds_head(int W) { return 2 * W * sizeof(uint64_t) + FPS_OUT_CHUNK * sizeof(int); }

// Rows 0 .. n-1 of g ((n,3) AoS in memory) into rows at .. at+n-1 of the SoA image, as a flat coalesced copy by T threads.
template <int T>
__device__ __forceinline__ void fps_load_soa(const float* g, int n, float* sx, float* sy, float* sz, int at, int tid) {
  for (int i = tid; i < 3 * n; i += T) {
    const float v = g[i];
    const int p = i / 3, c = i - 3 * p;
    (c == 0 ? sx : (c == 1 ? sy : sz))[at + p] = v;
  }
}

// One round on the points a thread holds in registers (point tid + p T in slot p; n points in all): the running distance
// becomes min(dist, |point - centroid|^2) (pointnet_util.py:70-71) and the wavefront's arg-max comes back as
// (dist_bits << 32) | ~index - dist >= 0, so its bit pattern is monotonic as an integer, and ~index makes the LOWEST
// index win ties, as torch.max does on CPU.  pmax: the register slots that hold a point at all, full: every thread's
// every slot does (both workgroup-uniform).
template <int T, int PPT>
__device__ __forceinline__ uint64_t fps_wave_argmax(const float (&px)[PPT], const float (&py)[PPT], const float (&pz)[PPT],
                                                    float (&dist)[PPT], float cx, float cy, float cz, int tid, int n, int pmax,
                                                    bool full) {
  if constexpr (PPT <= 4) {
    // arg-max in two parts: the 32-bit distance pattern goes through the wave reduction alone — six v_max_u32 with DPP
    // operands instead of six 64-bit compare-and-select steps — and the index is resolved afterwards: one lane holds the
    // maximum almost always (ballot + readlane); on a tie the lowest index wins, found by a second reduction only then.
    uint32_t bd = 0, bj = 0x7fffffffu;      // (a thread without a valid point keeps the sentinel and never ties)
#pragma unroll
    for (int p = 0; p < PPT; ++p) {
      const int j = tid + p * T;
      const float d = pzn::sqdist3(px[p], py[p], pz[p], cx, cy, cz);  // :70
      const float nd = d < dist[p] ? d : dist[p];                     // :71
      dist[p] = nd;
      const uint32_t nb = __float_as_uint(nd);
      // strict >: the lower index of equal distances stays (j ascends with p); the thread's first point is always taken
      const bool take = p == 0 ? (full || j < n) : ((full || j < n) && nb > bd);
      bd = take ? nb : bd;
      bj = take ? (uint32_t)j : bj;
    }
    const uint32_t wm = pzn::wave_max_u32_dpp(bd);
    const bool tied = bd == wm && (full || bj != 0x7fffffffu);
    const unsigned long long tmask = __ballot(tied);
    uint32_t wj;
    if (__popcll(tmask) == 1)
      wj = (uint32_t)__builtin_amdgcn_readlane((int)bj, __builtin_ctzll(tmask));
    else
      wj = pzn::wave_min_u32_dpp(tied ? bj : 0xffffffffu);
    return ((uint64_t)wm << 32) | (uint32_t)(~wj);
  } else {      // many points per thread: the 64-bit key (distance, ~index) per point measured faster there
    uint64_t best = 0;  // below every real key: real keys have ~j >= 1
#pragma unroll
    for (int p = 0; p < PPT; ++p) {
      if (p < pmax) {      // (workgroup-uniform: slots at and beyond pmax hold no point, or padding only)
        const int j = tid + p * T;
        const float d = pzn::sqdist3(px[p], py[p], pz[p], cx, cy, cz);  // :70
        const float nd = d < dist[p] ? d : dist[p];                     // :71
        dist[p] = nd;
        uint64_t key = ((uint64_t)__float_as_uint(nd) << 32) | (uint32_t)(~(uint32_t)j);
        key = j < n ? key : 0ull;
        best = key > best ? key : best;
      }
    }
    return pzn::wave_max_u64_dpp(best);
  }
}

// The cross-wavefront step: lane 0 of every wavefront writes its key to the slot row of the round's parity (so one
// barrier per round is enough), then every wavefront re-reduces the W slots redundantly.  Returns the workgroup's key -
// the pick is ~(uint32_t)key, the first (lowest-index) maximum (:72) - and in mw the wavefront that held it.  COORD (the
// published-coordinates form of fps.hip): lane 0 also writes c, the coordinates of its wavefront's best point, to
// scoord [2][W] beside the key, in the same exec-masked block (as a separate `if` of the caller the two stores are not merged).
template <int W, bool COORD = true>
__device__ __forceinline__ uint64_t fps_cross_wave(uint64_t* slots, int i, int lane, int wave, uint64_t best, int& mw,
                                                   float4* scoord, float4 c) {
  uint64_t* sl = slots + (i & 1) * W;
  if (lane == 0) {
    sl[wave] = best;
    if constexpr (COORD) scoord[(i & 1) * W + wave] = c;
  }
  __syncthreads();
  uint64_t m = sl[0];
  mw = 0;
#pragma unroll
  for (int w = 1; w < W; ++w) {
    const uint64_t v = sl[w];
    mw = v > m ? w : mw;
    m = v > m ? v : m;
  }
  return m;
}

// the same step with the key alone (the image form, merge_resample_kernel)
template <int W>
__device__ __forceinline__ uint64_t fps_cross_wave(uint64_t* slots, int i, int lane, int wave, uint64_t best) {
  int mw;
  return fps_cross_wave<W, false>(slots, i, lane, wave, best, mw, nullptr, float4{});
}

// Pick i of npicks (:68) goes to LDS and leaves in chunks: a global store inside the loop keeps a vector-memory operation
// outstanding at every barrier (__syncthreads waits for it: several hundred cycles per round on wave 0).  Every
// FPS_OUT_CHUNK picks, and at the last one, flush(base, cnt) writes out picks base .. base+cnt-1 = sout[0 .. cnt-1],
// between two barriers (sout is rewritten next round).
template <class Flush>
__device__ __forceinline__ void fps_buffer_pick(int* sout, int i, int npicks, int far, int tid, Flush&& flush) {
  if (tid == 0) sout[i & (FPS_OUT_CHUNK - 1)] = far;
  if ((i & (FPS_OUT_CHUNK - 1)) == FPS_OUT_CHUNK - 1 || i == npicks - 1) {
    __syncthreads();
    const int base = i & ~(FPS_OUT_CHUNK - 1);
    flush(base, i - base + 1);
    __syncthreads();
  }
}
