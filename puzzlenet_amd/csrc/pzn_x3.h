// pzn_x3.h — "bf16x3" split precision, the numeric recipe of every matrix-core kernel (gfx950): the vector types, the split
// of fp32 values into bf16 planes, the products of split operands.  Tests compare kernels' results bit for bit, so this is
// the only definition.  Included inside the translation unit's anonymous namespace, after pzn_common.h (pzn_mfma.h
// includes it for the chained kernels).
//
// x = x1 + x2 + x3 exactly, each xi a bf16 (8 significant bits, fp32's exponent range - as long as x3, up to 2^-16 of x,
// is still a normal number; tests/test_gpu_x3_exact.py probes operands scaled by 2^-40 .. 2^40 with every plane at or
// above 2^-40 and every product within 2^-80 .. 2^104, and says nothing about where a plane would underflow): x1 = bf16(x),
// x2 = bf16(x - x1), x3 = bf16(x - x1 - x2).  a*b is then summed from the six products whose magnitude is
// >= 2^-16 of the leading one: (1,1) (1,2) (2,1) (1,3) (2,2) (3,1); the three dropped ones are <= 2^-24
// relative, i.e. below fp32 rounding.  Each product of two bf16 is exact in fp32 and the MFMA accumulates
// in fp32, so the result has fp32-GEMM accuracy — at 6 v_mfma_f32_32x32x16_bf16 (32 cycles for 16 k) against
// 8 v_mfma_f32_32x32x2_f32 (64 cycles for 2 k): 2.67x the matrix-pipe throughput.
#pragma once

typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef float floatx4 __attribute__((ext_vector_type(4)));
typedef float v2f __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ uint32_t f2bf(float x) {
  __bf16 b = (__bf16)x;  // v_cvt_pk_bf16_f32, round to nearest even
  return (uint32_t)__builtin_bit_cast(unsigned short, b);
}
__device__ __forceinline__ float bf2f(uint32_t b) { return __uint_as_float(b << 16); }
// one value -> its three planes (the general tile engine, gemm.hip)
__device__ __forceinline__ void split3(float x, uint32_t& a, uint32_t& b, uint32_t& c) {
  a = f2bf(x);
  float r = x - bf2f(a);
  b = f2bf(r);
  float r2 = r - bf2f(b);
  c = f2bf(r2);
}

// Two values -> three dwords of two bf16 each (plane 1, 2, 3; lo = x0), in two instruction forms that give the same bits:
// every remainder is the same exact fp32 subtraction (x and bf16(x) are within a factor of two), issued either as
// v_sub_f32 or as a lane of v_pk_add_f32.  Both stay because the form is part of the kernels' instruction streams: the
// chained kernels (pzn_mfma.h, built with -fno-slp-vectorize) issue the scalar one, wsgemm / dfgemm / attnwgrad the packed
// one; moving a kernel to the other form is a performance change to be measured.
// scalar: 3 v_cvt_pk_bf16_f32 + 4 unpack + 4 v_sub_f32
__device__ __forceinline__ void split_pair_scalar(float x0, float x1, uint32_t& p1, uint32_t& p2, uint32_t& p3) {
  const v2f x = {x0, x1};
  p1 = __builtin_bit_cast(uint32_t, __builtin_convertvector(x, bf16x2));
  const v2f r = {x0 - __uint_as_float(p1 << 16), x1 - __uint_as_float(p1 & 0xffff0000u)};
  p2 = __builtin_bit_cast(uint32_t, __builtin_convertvector(r, bf16x2));
  const v2f t = {r[0] - __uint_as_float(p2 << 16), r[1] - __uint_as_float(p2 & 0xffff0000u)};
  p3 = __builtin_bit_cast(uint32_t, __builtin_convertvector(t, bf16x2));
}
// packed: 3 v_cvt_pk_bf16_f32 + 4 unpack + 2 v_pk_add_f32
__device__ __forceinline__ void split_pair_packed(float x0, float x1, uint32_t& p1, uint32_t& p2, uint32_t& p3) {
  const v2f x = {x0, x1};
  p1 = __builtin_bit_cast(uint32_t, __builtin_convertvector(x, bf16x2));
  const v2f r = x - v2f{__uint_as_float(p1 << 16), __uint_as_float(p1 & 0xffff0000u)};
  p2 = __builtin_bit_cast(uint32_t, __builtin_convertvector(r, bf16x2));
  const v2f t = r - v2f{__uint_as_float(p2 << 16), __uint_as_float(p2 & 0xffff0000u)};
  p3 = __builtin_bit_cast(uint32_t, __builtin_convertvector(t, bf16x2));
}

typedef void (*PairSplit)(float, float, uint32_t&, uint32_t&, uint32_t&);

// eight values (one lane's MFMA operand) -> the dwords of its three planes, w[plane][pair], a pair at a time in the form
// PAIR.  The packing is left to the caller: attnwgrad.hip packs and stores behind its MFMAs (packed here, the compiler
// schedules that kernel's split differently).
template <PairSplit PAIR>
__device__ __forceinline__ void split8(const float (&v)[8], uint32_t (&w)[3][4]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) PAIR(v[2 * j], v[2 * j + 1], w[0][j], w[1][j], w[2][j]);
}
// the same as three bf16x8 fragments
template <PairSplit PAIR>
__device__ __forceinline__ void split8(const float (&v)[8], bf16x8 (&b)[3]) {
  uint32_t w[3][4];
  split8<PAIR>(v, w);
#pragma unroll
  for (int p = 0; p < 3; ++p) b[p] = __builtin_bit_cast(bf16x8, u32x4{w[p][0], w[p][1], w[p][2], w[p][3]});
}

// one product of bf16 fragments, the shape chosen by the accumulator: 32x32x16 (16 registers) or 16x16x32 (4)
__device__ __forceinline__ floatx16 mfma_bf16(bf16x8 a, bf16x8 b, floatx16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ floatx4 mfma_bf16(bf16x8 a, bf16x8 b, floatx4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

// acc += A B with A, B in NPL planes each.  NPL = 3: the six products >= 2^-16, small terms first; NPL = 1: plane 0 only,
// one product (the opt-in bf16 modes).  TRANSPOSED: acc += (A B)^T, each product with its operands exchanged and the
// terms in the same order (exchanging the arguments instead would reorder the terms, and change the bits).
template <int NPL = 3, bool TRANSPOSED = false, class Acc>
__device__ __forceinline__ Acc mma_x3(const bf16x8* a, const bf16x8* b, Acc c) {
  const auto mma = [&](int i, int j) { c = TRANSPOSED ? mfma_bf16(b[j], a[i], c) : mfma_bf16(a[i], b[j], c); };
  if constexpr (NPL == 3) {
    mma(2, 0);
    mma(1, 1);
    mma(0, 2);
    mma(1, 0);
    mma(0, 1);
  }
  mma(0, 0);
  return c;
}

// the gate of a generated row, relu(x + q): P' row + the group's Q row (the per-point first layer); the forward and the
// backward regenerate the same rows and must produce the same bits
__device__ __forceinline__ float4 add_relu(float4 x, float4 q) {
  return make_float4(fmaxf(x.x + q.x, 0.f), fmaxf(x.y + q.y, 0.f), fmaxf(x.z + q.z, 0.f), fmaxf(x.w + q.w, 0.f));
}
