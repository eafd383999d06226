// pzn_walk.h — what the walks over pair tables share (assemblewalk.hip, assemblebeam.hip, progressive.hip): the key of a table
// entry, the 64-lane lexicographic arg-min over (key, i K + j), the stop test on a round's winning key, the order-fixed float64
// dot product the poses are composed with, the greedy walks' sixteen-lane pose product, the beam walks' ordered cost bits, lane
// reads and right factor, and the tail of a walk's result (assemblewalk.hip, assemblebeam.hip): the placed bytes and the joint
// list.  One statement of each, so "the smallest key, the lowest i K + j on ties", "the walk stops here" and "every operation
// rounded on its own" mean the same in every kernel.  Files that include it are built with -ffp-contract=off and say so again
// with the pragma.
#ifndef PZN_WALK_H_
#define PZN_WALK_H_

#include "pzn_common.h"

#pragma clang fp contract(off)

namespace {

// fp32 -> dword with the floats' order (no NaN reaches it)
__device__ __forceinline__ uint32_t ordered(float x) {
  const uint32_t u = __float_as_uint(x);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ float unordered(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// the key of entry (i, j) with score s: NaN and the diagonal are +inf, -0 is +0
__device__ __forceinline__ uint64_t entry(float s, int i, int j, int K) {
  float k = (i == j || s != s) ? __builtin_inff() : s;
  k = k == 0.f ? 0.f : k;
  return ((uint64_t)ordered(k) << 32) | (uint32_t)(i * K + j);
}

__device__ __forceinline__ uint64_t wave_min_u64_dpp(uint64_t v) {
  uint64_t o;
  o = pzn::xor_lane_u64<1>(v), v = o < v ? o : v;
  o = pzn::xor_lane_u64<2>(v), v = o < v ? o : v;
  o = pzn::xor_lane_u64<4>(v), v = o < v ? o : v;
  o = pzn::xor_lane_u64<8>(v), v = o < v ? o : v;
  o = pzn::xor_lane_u64<16>(v), v = o < v ? o : v;
  o = pzn::xor_lane_u64<32>(v), v = o < v ? o : v;
  return v;
}

// a round ends the walk at a winning key (the high dword of the 64-lane minimum) that is not finite or above max_score
__device__ __forceinline__ bool stops(uint32_t w_key, double max_score) {
  const float key = unordered(w_key);
  return !(fabsf(key) < __builtin_inff()) || (double)key > max_score;
}

__device__ __forceinline__ double dot4(double a0, double b0, double a1, double b1, double a2, double b2, double a3, double b3) {
  return ((a0 * b0 + a1 * b1) + a2 * b2) + a3 * b3;
}

// ---- what the beam walks share (assemblebeam.hip)

// doubles -> qword with the doubles' order (no NaN reaches it), -0 as +0
__device__ __forceinline__ uint64_t ordered64(double x) {
  x = x == 0.0 ? 0.0 : x;
  const uint64_t u = (uint64_t)__double_as_longlong(x);
  return (u >> 63) ? ~u : (u | ((uint64_t)1 << 63));
}

__device__ __forceinline__ uint64_t lane_u64(uint64_t v, int l) {
  const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, l, PZN_WAVE), hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), l, PZN_WAVE);
  return ((uint64_t)hi << 32) | lo;
}

// the right factor of a pose product, b[4 k + v] = B[k][v]: T[i,j] as stored, or its rigid inverse [R^T, -(R^T t)] with the
// last row 0 0 0 1 (the walk's arithmetic, entry for entry)
__device__ __forceinline__ void right_factor(const float* __restrict__ t, bool fwd, double* b) {
  double d[16];
#pragma unroll
  for (int e = 0; e < 16; ++e) d[e] = (double)t[e];
  const double i0 = -((d[0] * d[3] + d[4] * d[7]) + d[8] * d[11]);
  const double i1 = -((d[1] * d[3] + d[5] * d[7]) + d[9] * d[11]);
  const double i2 = -((d[2] * d[3] + d[6] * d[7]) + d[10] * d[11]);
  const double inv[16] = {d[0], d[4], d[8], i0, d[1], d[5], d[9], i1, d[2], d[6], d[10], i2, 0.0, 0.0, 0.0, 1.0};
#pragma unroll
  for (int e = 0; e < 16; ++e) b[e] = fwd ? d[e] : inv[e];
}

// The greedy walks' pose product g[nw] = g[src] B over the [K][16] float64 poses g in LDS, B = T[i,j] as t stores it (fwd) or
// its rigid inverse: the wavefront's first sixteen lanes, one entry each - lane 4 u + v takes column v of B and row u of
// g[src] (right_factor's arithmetic entry for entry, but a column a lane and not the whole factor).  nw != src: no lane reads
// what another writes.
__device__ __forceinline__ void compose_pose16(double* g, int src, int nw, const float* __restrict__ t, bool fwd, int lane) {
  if (lane < 16) {
    const int u = lane >> 2, v = lane & 3;
    double b0, b1, b2, b3;
    if (fwd) {
      b0 = (double)t[v], b1 = (double)t[4 + v], b2 = (double)t[8 + v], b3 = (double)t[12 + v];
    } else if (v < 3) {
      b0 = (double)t[4 * v], b1 = (double)t[4 * v + 1], b2 = (double)t[4 * v + 2], b3 = 0.0;
    } else {
      const double t0 = (double)t[3], t1 = (double)t[7], t2 = (double)t[11];
      b0 = -(((double)t[0] * t0 + (double)t[4] * t1) + (double)t[8] * t2);
      b1 = -(((double)t[1] * t0 + (double)t[5] * t1) + (double)t[9] * t2);
      b2 = -(((double)t[2] * t0 + (double)t[6] * t1) + (double)t[10] * t2);
      b3 = 1.0;
    }
    const double* a = g + 16 * src + 4 * u;
    g[16 * nw + lane] = dot4(a[0], b0, a[1], b1, a[2], b2, a[3], b3);
  }
}

// The tail of a walk's result for one puzzle, by its wavefront: `in` is the placed set (bit p = piece p), c the puzzle's
// pieces, ne its edges, worst its largest edge score, S its [K,K] scores, my_comp the component of piece `lane` (read for placed
// pieces only; the one-tree walks pass 0); placed [K] and joints [K (K - 1), 2] are the puzzle's rows of the outputs -> the
// number of joints.  The joints are the placed i != j of one component with (double)score[i,j] <= limit on the raw score,
// limit = joint_score or (NaN) worst: for every placed row i in turn, lane j tests entry (i, j) (a coalesced row) and the
// ballot's prefix count is the place of (i, j) after the joints of the rows before - row-major order with no scan through
// memory.  Unused rows are (-1, -1).  (`in`, c, ne and the count are the same in every lane.)
__device__ __forceinline__ int walk_tail(uint64_t in, int c, int K, int ne, double worst, double joint_score,
                                         const float* __restrict__ S, int lane, int my_comp, uint8_t* __restrict__ placed,
                                         int32_t* __restrict__ joints) {
  if (lane < K) placed[lane] = (uint8_t)((in >> lane) & 1);
  const double limit = joint_score != joint_score ? worst : joint_score;
  int nj = 0;
  if (ne > 0) {
    for (int i = 0; i < c; ++i) {
      if (!((in >> i) & 1)) continue;
      const int comp_i = __builtin_amdgcn_readlane(my_comp, i);
      bool ok = false;
      if (lane < c && lane != i && ((in >> lane) & 1) && my_comp == comp_i) ok = (double)S[i * K + lane] <= limit;
      const uint64_t m = __ballot(ok);
      if (ok) {
        const int at = nj + __popcll(m & (((uint64_t)1 << lane) - 1));
        joints[2 * at] = i, joints[2 * at + 1] = lane;
      }
      nj += __popcll(m);
    }
  }
  for (int e = nj + lane; e < K * (K - 1); e += PZN_WAVE) joints[2 * e] = -1, joints[2 * e + 1] = -1;
  return nj;
}

}  // namespace

#endif  // PZN_WALK_H_
