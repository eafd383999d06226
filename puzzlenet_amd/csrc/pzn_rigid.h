// pzn_rigid.h — the arithmetic the pose refinement kernels share (icprefine.hip, jointrefine.hip): a pose as fp32 values
// and how it moves a point, the two order-fixed wave sums, the workgroup sum of the two objective halves, Horn's closed-form
// rotation in float64 and the one lane's solve with its degenerate rule.  One statement of each, so a pose refined by one
// kernel moves points to the same bits in the other (and in mergefps.hip).
#ifndef PZN_RIGID_H_
#define PZN_RIGID_H_

#include "pzn_common.h"

namespace {

constexpr int ICP_SWEEPS = 12;             // cyclic Jacobi sweeps at most (a 4x4 converges in 5 to 7)
constexpr double ICP_DEGENERATE = 1e-10;   // degenerate iff m2 <= ICP_DEGENERATE * tr * tr (solve_pose states the rule)

__device__ __forceinline__ double wave_sum_f64(double v) {
  uint64_t u;
  u = pzn::xor_lane_u64<1>((uint64_t)__double_as_longlong(v)), v += __longlong_as_double((long long)u);
  u = pzn::xor_lane_u64<2>((uint64_t)__double_as_longlong(v)), v += __longlong_as_double((long long)u);
  u = pzn::xor_lane_u64<4>((uint64_t)__double_as_longlong(v)), v += __longlong_as_double((long long)u);
  u = pzn::xor_lane_u64<8>((uint64_t)__double_as_longlong(v)), v += __longlong_as_double((long long)u);
  u = pzn::xor_lane_u64<16>((uint64_t)__double_as_longlong(v)), v += __longlong_as_double((long long)u);
  u = pzn::xor_lane_u64<32>((uint64_t)__double_as_longlong(v)), v += __longlong_as_double((long long)u);
  return v;
}

__device__ __forceinline__ float wave_sum_f32_dpp(float v) {
  v = __fadd_rn(v, __uint_as_float(pzn::xor_lane<1>(__float_as_uint(v))));
  v = __fadd_rn(v, __uint_as_float(pzn::xor_lane<2>(__float_as_uint(v))));
  v = __fadd_rn(v, __uint_as_float(pzn::xor_lane<4>(__float_as_uint(v))));
  v = __fadd_rn(v, __uint_as_float(pzn::xor_lane<8>(__float_as_uint(v))));
  v = __fadd_rn(v, __uint_as_float(pzn::xor_lane<16>(__float_as_uint(v))));
  v = __fadd_rn(v, __uint_as_float(pzn::xor_lane<32>(__float_as_uint(v))));
  return v;
}

// The workgroup sum of the two objective halves, the same bits in every thread: the wave adds its lanes by the xor butterfly
// (both partners form the same sum), lane 0 leaves the wave's two sums in rede [W][2], a barrier, the W wave sums are added
// in wave order -> e1, e2.  The caller's next barrier frees rede.
template <int W>
__device__ __forceinline__ void block_sum2_f32(float* rede, int tid, float s1, float s2, float& e1, float& e2) {
  s1 = wave_sum_f32_dpp(s1);
  s2 = wave_sum_f32_dpp(s2);
  if ((tid & (PZN_WAVE - 1)) == 0) rede[2 * (tid / PZN_WAVE)] = s1, rede[2 * (tid / PZN_WAVE) + 1] = s2;
  __syncthreads();
  e1 = rede[0], e2 = rede[1];
#pragma unroll
  for (int w = 1; w < W; ++w) e1 = __fadd_rn(e1, rede[2 * w]), e2 = __fadd_rn(e2, rede[2 * w + 1]);
}

// One Jacobi rotation of the symmetric 4x4 A in the (P, Q) plane, accumulated into V (columns = eigenvectors).
template <int P, int Q>
__device__ __forceinline__ void jacobi_rot(double (&A)[4][4], double (&V)[4][4]) {
  const double apq = A[P][Q];
  if (apq == 0.0) return;
  const double theta = (A[Q][Q] - A[P][P]) / (2.0 * apq);
  const double tt = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
  const double c = 1.0 / sqrt(tt * tt + 1.0), s = tt * c;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double x = A[k][P], y = A[k][Q];
    A[k][P] = c * x - s * y;
    A[k][Q] = s * x + c * y;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double x = A[P][k], y = A[Q][k];
    A[P][k] = c * x - s * y;
    A[Q][k] = s * x + c * y;
  }
  A[P][Q] = A[Q][P] = 0.0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double x = V[k][P], y = V[k][Q];
    V[k][P] = c * x - s * y;
    V[k][Q] = s * x + c * y;
  }
}

// Horn's closed form: the rotation R (row-major) that maximises sum p . R q for S[u][v] = sum q_u p_v.
__device__ void horn_rotation(const double (&S)[3][3], double (&R)[9]) {
  double A[4][4], V[4][4];
  A[0][0] = S[0][0] + S[1][1] + S[2][2];
  A[1][1] = S[0][0] - S[1][1] - S[2][2];
  A[2][2] = -S[0][0] + S[1][1] - S[2][2];
  A[3][3] = -S[0][0] - S[1][1] + S[2][2];
  A[0][1] = A[1][0] = S[1][2] - S[2][1];
  A[0][2] = A[2][0] = S[2][0] - S[0][2];
  A[0][3] = A[3][0] = S[0][1] - S[1][0];
  A[1][2] = A[2][1] = S[0][1] + S[1][0];
  A[1][3] = A[3][1] = S[2][0] + S[0][2];
  A[2][3] = A[3][2] = S[1][2] + S[2][1];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) V[i][j] = i == j ? 1.0 : 0.0;
  for (int sweep = 0; sweep < ICP_SWEEPS; ++sweep) {
    const double off = A[0][1] * A[0][1] + A[0][2] * A[0][2] + A[0][3] * A[0][3] + A[1][2] * A[1][2] + A[1][3] * A[1][3] +
                       A[2][3] * A[2][3];
    const double dia = A[0][0] * A[0][0] + A[1][1] * A[1][1] + A[2][2] * A[2][2] + A[3][3] * A[3][3];
    if (off <= 1e-34 * dia) break;
    jacobi_rot<0, 1>(A, V);
    jacobi_rot<0, 2>(A, V);
    jacobi_rot<0, 3>(A, V);
    jacobi_rot<1, 2>(A, V);
    jacobi_rot<1, 3>(A, V);
    jacobi_rot<2, 3>(A, V);
  }
  // the column of the largest eigenvalue (first of equals), by selects: no dynamically indexed array
  double l = A[0][0], w = V[0][0], x = V[1][0], y = V[2][0], z = V[3][0];
#pragma unroll
  for (int c = 1; c < 4; ++c) {
    const bool take = A[c][c] > l;
    l = take ? A[c][c] : l;
    w = take ? V[0][c] : w, x = take ? V[1][c] : x, y = take ? V[2][c] : y, z = take ? V[3][c] : z;
  }
  const double inv = 1.0 / sqrt(w * w + x * x + y * y + z * z);
  w *= inv, x *= inv, y *= inv, z *= inv;
  R[0] = 1.0 - 2.0 * (y * y + z * z), R[1] = 2.0 * (x * y - w * z), R[2] = 2.0 * (x * z + w * y);
  R[3] = 2.0 * (x * y + w * z), R[4] = 1.0 - 2.0 * (x * x + z * z), R[5] = 2.0 * (y * z - w * x);
  R[6] = 2.0 * (x * z - w * y), R[7] = 2.0 * (y * z + w * x), R[8] = 1.0 - 2.0 * (x * x + y * y);
}

struct Pose {
  float r[9], t[3];
};

// x' = ((r00 x + r01 y) + r02 z) + t0 and likewise y', z': every product and sum rounded on its own (mergefps.hip's arithmetic).
__device__ __forceinline__ void pose_move(const Pose& g, float x, float y, float z, float& ox, float& oy, float& oz) {
  ox = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(g.r[0], x), __fmul_rn(g.r[1], y)), __fmul_rn(g.r[2], z)), g.t[0]);
  oy = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(g.r[3], x), __fmul_rn(g.r[4], y)), __fmul_rn(g.r[5], z)), g.t[1]);
  oz = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(g.r[6], x), __fmul_rn(g.r[7], y)), __fmul_rn(g.r[8], z)), g.t[2]);
}

// One lane's solve in float64, from the centred cross-covariance S[u][v] = sum q_u p_v (fixed p, moved q), the scatter
// sum q q^T of the moved side as c = its entries 00 11 22 01 02 12, the centroids pc, qc and the current pose -> the
// candidate in cand [12]: R (Horn) and t = pc - R qc, each rounded to fp32.
// DEGENERATE pairs (a single point, all moved-side points q coincident or collinear) keep the current R and update t only.
// The rule, stated once: with the scatter's trace tr and the sum of its three principal 2x2 minors m2 (= l1 l2 + l1 l3 +
// l2 l3 for eigenvalues l), degenerate iff m2 <= ICP_DEGENERATE * tr * tr, ICP_DEGENERATE = 1e-10 (m2 / tr^2 is about
// l2 / l1 for a thin set; points exactly on a line, rounded to fp32, sit near 1e-14).
__device__ __forceinline__ void solve_pose(const double (&S)[3][3], const double (&c)[6], const Pose& cur, const double (&pc)[3],
                                           const double (&qc)[3], float* cand) {
  const double tr = c[0] + c[1] + c[2];
  const double m2 = (c[0] * c[1] - c[3] * c[3]) + (c[0] * c[2] - c[4] * c[4]) + (c[1] * c[2] - c[5] * c[5]);
  double R[9];
  if (m2 <= ICP_DEGENERATE * tr * tr) {
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = (double)cur.r[k];
  } else {
    horn_rotation(S, R);
  }
#pragma unroll
  for (int k = 0; k < 9; ++k) cand[k] = (float)R[k];
#pragma unroll
  for (int u = 0; u < 3; ++u) cand[9 + u] = (float)(pc[u] - ((R[3 * u] * qc[0] + R[3 * u + 1] * qc[1]) + R[3 * u + 2] * qc[2]));
}

}  // namespace

#endif  // PZN_RIGID_H_
