// pzn_walk.h — what the walks over pair tables share (assemblewalk.hip, progressive.hip): the key of a table entry, the
// 64-lane lexicographic arg-min over (key, i K + j) and the order-fixed float64 dot product the poses are composed with.  One
// statement of each, so "the smallest key, the lowest i K + j on ties" and "every operation rounded on its own" mean the same
// in both kernels.  Files that include it are built with -ffp-contract=off and say so again with the pragma.
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

__device__ __forceinline__ double dot4(double a0, double b0, double a1, double b1, double a2, double b2, double a3, double b3) {
  return ((a0 * b0 + a1 * b1) + a2 * b2) + a3 * b3;
}

}  // namespace

#endif  // PZN_WALK_H_
