// jointauto.hip — the joint refinement of jointtrim.hip with the two kept counts of every joint FOUND at every evaluation of the
// joint, under the poses being tried, for gfx950 (ops.joint_refine(..., auto=), assembly.refine_assembly(..., auto=)).  The
// contract is in include/pzn.h (pzn_joint_refine_auto_f32); the count rule is the one stated there above
// pzn_icp_refine_auto_f32, Trimmed ICP's search for the overlap carried into the pose graph.
//
// joint_auto_kernel is the AUTO = true instantiation of the body in pzn_jointtrim.h; everything of jointtrim.hip stands.  What
// an evaluation of a joint gains:
//   * after the row minima stand in LDS every row counts the rows of its direction before it in (minimum, row index) order, as
//     the sibling does, but keeps that rank in a register (a thread owns at most 8 rows) and writes its minimum to sorted[rank]
//     of its direction - the ranks are a permutation, so this is the sort; a barrier;
//   * find_counts: thread t adds the four sorted values 4t .. 4t+3 of each direction one after the other, the wave scans the
//     thread totals (Hillis-Steele, lane l adds lane l - d for d = 1 .. 32), the four wave totals go through LDS and are added
//     in wave order - float32 prefix sums S_m in one fixed order; phi(m) = (double)S_m / m^(p+1) for the thread's own four m in
//     [lo, n], one float64 division a row; the lexicographic arg-min of (phi, larger m) is a butterfly and four LDS slots per
//     direction.  Two barriers; the counts m_a, m_b are then the same bits in all 256 threads;
//   * the kept rows (rank < m) are summed from the ranks in the sibling's order, so E_e = e_a + e_b is the sibling's at these
//     counts; the joint is scored by F_e = e_a r_a + e_b r_b, r = (float)(k / m)^p, and it is F_e that L.js and L.jn hold and the
//     two acceptance guards compare: objective <= objective0 to the bit, score (the sum of E_e) need not fall;
//   * a visit: the kept pairs weigh r_a / m_a and r_b / m_b in float64 (the candidate then minimises F_p for the sets and
//     counts at hand); at lo = k that is 1 / k, the sibling's weight, and every sum has its bits;
//   * after the loop every joint is evaluated once more under the returned poses, always: that pass writes joint_score (E_e),
//     count_a, count_b and, where asked for, kept_a / kept_b, and its sum of E_e is score; score0 is the first pass's sum.
// LDS, in bytes: jointtrim.hip's image plus 4 * (ka + kb) of sorted minima.  At K = 64, J = 4032, ka = kb = 1024 that is
// 69 904 + 8 192 = 78 096 B (76.3 KB): the launch raises the kernel's dynamic limit as jointtrim.hip does, and two workgroups
// still fit a CU's 160 KB.
// Every loop bound and every branch around a barrier depends only on the joint list, `movable`, kernel arguments and values
// that are the same bits in all 256 threads (the counts come out of a butterfly plus LDS slots read by every thread).
// Duplicated from icprefine.hip (DESIGN section 3 lists it for a later fold): the count search, find_counts in pzn_jointtrim.h.
#include "pzn_jointtrim.h"

namespace {

__global__ __launch_bounds__(JT_T) void joint_auto_kernel(
    const float* __restrict__ a, const int64_t* __restrict__ a_of, const float* __restrict__ b, const int64_t* __restrict__ b_of,
    const int32_t* __restrict__ joints, const float* __restrict__ G0, const uint8_t* __restrict__ movable, int Z, int K, int J,
    int ka, int kb, int lo_a, int lo_b, int power, int sweeps, float* __restrict__ G, float* __restrict__ score,
    float* __restrict__ score0, float* __restrict__ joint_score, int32_t* __restrict__ sweeps_used,
    int32_t* __restrict__ accepted, float* __restrict__ objective, float* __restrict__ objective0,
    int32_t* __restrict__ count_a, int32_t* __restrict__ count_b, int32_t* __restrict__ kept_a, int32_t* __restrict__ kept_b) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const Sets S = {a, a_of, b, b_of, ka, kb, nullptr, nullptr, kept_a, kept_b, lo_a, lo_b, power, count_a, count_b, joint_score};
  joint_trim_body<true>(S, joints, G0, movable, Z, K, J, sweeps, G, score, score0, joint_score, sweeps_used, accepted,
                        AutoOut{objective, objective0}, smem_raw);
}

}  // namespace

PZN_EXPORT int pzn_joint_refine_auto_supported(int K, int J, int ka, int kb, int lo_a, int lo_b, int power) {
  return joint_trim_range(K, J, ka, kb) && lo_a >= 1 && lo_a <= ka && lo_b >= 1 && lo_b <= kb && power >= 1 && power <= 4;
}

PZN_EXPORT int pzn_joint_refine_auto_f32(const float* a, const int64_t* a_of, const float* b, const int64_t* b_of,
                                         const int32_t* joints, const float* G0, const uint8_t* movable, int Z, int K, int J,
                                         int ka, int kb, int lo_a, int lo_b, int power, int sweeps, float* G, float* score,
                                         float* score0, float* joint_score, int32_t* sweeps_used, int32_t* accepted,
                                         float* objective, float* objective0, int32_t* count_a, int32_t* count_b,
                                         int32_t* kept_a, int32_t* kept_b, pzn_stream_t stream) {
  if (!pzn_joint_refine_auto_supported(K, J, ka, kb, lo_a, lo_b, power) || sweeps < 0) return PZN_EUNSUPPORTED;
  PZN_CHECK_ARG(Z >= 0);
  if (Z == 0 || J == 0) return PZN_OK;
  PZN_CHECK_ARG(a && b && joints && G0 && movable && G && score && score0 && joint_score && sweeps_used && accepted && objective &&
                objective0 && count_a && count_b);
  hipStream_t st = pzn_hip_stream(stream);
  const size_t lds = joint_trim_lds(K, J, ka, kb, true);
  if (lds > 64 * 1024 && hipFuncSetAttribute(reinterpret_cast<const void*>(joint_auto_kernel),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return PZN_ELAUNCH;
  const int grid = Z < JT_MAX_GRID ? Z : JT_MAX_GRID;
  PZN_LAUNCH(joint_auto_kernel, dim3(grid), dim3(JT_T), lds, st, a, a_of, b, b_of, joints, G0, movable, Z, K, J, ka, kb, lo_a, lo_b,
             power, sweeps, G, score, score0, joint_score, sweeps_used, accepted, objective, objective0, count_a, count_b, kept_a,
             kept_b);
  PZN_RETURN_LAUNCH_STATUS();
}
