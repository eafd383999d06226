// jointtrim.hip — the joint refinement of jointrefine.hip with the kept rows of every joint chosen again under the joint poses,
// for gfx950 (ops.joint_refine(..., ma=, mb=), assembly.refine_assembly(..., keep=)).  The contract is in include/pzn.h.
//
// Everything of jointrefine.hip stands: one workgroup of 256 threads per puzzle (more puzzles share a workgroup in turn), the
// poses G[K] in LDS, block-coordinate descent over the pieces, the fp32 images, pzn::sqdist3, the lowest-index arg-min, row
// r < ka = G_i a_r scanning G_j B and row ka + c = G_j b_c scanning G_i A, a thread owning rows tid, tid + 256, ..., the two
// acceptance guards and the outputs.  What is new is a pair of counts per joint ROW, ma in [1, ka] and mb in [1, kb]:
//   * every evaluation of a joint leaves each row's minimum and arg-min in LDS (rmin, arg); after one more barrier every row
//     counts the rows of its direction that come before it in (minimum, row index) order - a broadcast read, O(k) per row,
//     like the scan - and is KEPT iff fewer than ma (mb) do: icp_trim_kernel's rule, exactly m rows whatever the ties;
//   * E_e = (sum of kept A-row minima) / ma + (sum of kept B-row minima) / mb: the thread adds its kept rows' minima in row
//     order, then the butterfly, then the wave order (block_sum2_f32), the divisors (float)ma and (float)mb;
//   * a visit: in that same second pass over its own rows a thread adds the pair of every KEPT row to the 22 float64 sums, with
//     weight 1 / ma or 1 / mb (today's kernel adds them inside the scan loop; the arithmetic of a pair and their order are
//     the same, so with ma = ka and mb = kb every sum has the sibling's bits); solve_pose is unchanged;
//   * the candidate is evaluated with ITS OWN kept sets and taken iff E_p' < E_p and the fp32 total does not round above the
//     current one: score <= score0 to the bit;
//   * kept_a [Z,J,ka] / kept_b [Z,J,kb]: after the loop, when either is asked for, every joint is evaluated once more under
//     the returned poses with the kept flags written over `arg`; a kept row's place is the number of kept rows before it.
//     Positions ascending, -1 behind the count, all -1 for a skipped row;
//   * a row with a count outside [1, ka] / [1, kb] is skipped like a bad (i, j); ma / mb NULL mean ka / kb for every row.
// LDS, in bytes: the sibling's image - 704 of float64 partials, 80 of wave sums and the candidate, 48 * K of poses, 9 images
// of 4 * kmax (kmax = max(ka, kb) rounded up to a multiple of four), 4 * K of visit counts, 4 * (J + 2 * K) of joint energies -
// plus 4 * (ka + kb) of row minima and 2 * (ka + kb) of arg-mins (unsigned short: k <= 1024).  At K = 64, J = 4032, ka = kb = 1024 that is 57 616 + 8 192 + 4 096 =
// 69 904 B (68.3 KB): above the 64 KB a kernel may ask for by default, so the launch raises the kernel's dynamic limit
// (hipFuncAttributeMaxDynamicSharedMemorySize, as sapool.hip and wsgemm.hip do) when it needs more; two workgroups still fit
// a CU's 160 KB.  pzn_joint_refine_trim_supported is therefore the sibling's range.
// Every loop bound and every branch around a barrier depends only on the joint list, `movable`, the counts of a row (read by
// every thread from one address), the two kept pointers and E values that are the same bits in all 256 threads.
// Duplicated from jointrefine.hip, which stays as it is (DESIGN section 3 lists these for a later fold): Lds and Sets, load_pose,
// eval_joint's staging and scan, candidate, joint_ok, row_ok, eval_joints, total_with and the body's sweep loop.
// All of it stands in pzn_jointtrim.h, as one body with an AUTO template flag that jointauto.hip instantiates too; this file
// holds the AUTO = false kernel and its entry point.
#include "pzn_jointtrim.h"      // the body, shared with jointauto.hip (AUTO = false here: every addition of that form is compiled out)

namespace {

__global__ __launch_bounds__(JT_T) void joint_trim_kernel(
    const float* __restrict__ a, const int64_t* __restrict__ a_of, const int32_t* __restrict__ ma, const float* __restrict__ b,
    const int64_t* __restrict__ b_of, const int32_t* __restrict__ mb, const int32_t* __restrict__ joints,
    const float* __restrict__ G0, const uint8_t* __restrict__ movable, int Z, int K, int J, int ka, int kb, int sweeps,
    float* __restrict__ G, float* __restrict__ score, float* __restrict__ score0, float* __restrict__ joint_score,
    int32_t* __restrict__ sweeps_used, int32_t* __restrict__ accepted, int32_t* __restrict__ kept_a,
    int32_t* __restrict__ kept_b) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const Sets S = {a, a_of, b, b_of, ka, kb, ma, mb, kept_a, kept_b, 0, 0, 0, nullptr, nullptr, nullptr};
  joint_trim_body<false>(S, joints, G0, movable, Z, K, J, sweeps, G, score, score0, joint_score, sweeps_used, accepted,
                         AutoOut{nullptr, nullptr}, smem_raw);
}

}  // namespace

// The sibling's range: the 68.3 KB of LDS at its upper end are allowed by attribute at the launch.
PZN_EXPORT int pzn_joint_refine_trim_supported(int K, int J, int ka, int kb) { return joint_trim_range(K, J, ka, kb); }

PZN_EXPORT int pzn_joint_refine_trim_f32(const float* a, const int64_t* a_of, const int32_t* ma, const float* b,
                                         const int64_t* b_of, const int32_t* mb, const int32_t* joints, const float* G0,
                                         const uint8_t* movable, int Z, int K, int J, int ka, int kb, int sweeps, float* G,
                                         float* score, float* score0, float* joint_score, int32_t* sweeps_used,
                                         int32_t* accepted, int32_t* kept_a, int32_t* kept_b, pzn_stream_t stream) {
  if (!pzn_joint_refine_trim_supported(K, J, ka, kb) || sweeps < 0) return PZN_EUNSUPPORTED;
  PZN_CHECK_ARG(Z >= 0);
  if (Z == 0 || J == 0) return PZN_OK;
  PZN_CHECK_ARG(a && b && joints && G0 && movable && G && score && score0 && joint_score && sweeps_used && accepted);
  hipStream_t st = pzn_hip_stream(stream);
  const size_t lds = joint_trim_lds(K, J, ka, kb, false);
  if (lds > 64 * 1024 && hipFuncSetAttribute(reinterpret_cast<const void*>(joint_trim_kernel),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return PZN_ELAUNCH;
  const int grid = Z < JT_MAX_GRID ? Z : JT_MAX_GRID;
  PZN_LAUNCH(joint_trim_kernel, dim3(grid), dim3(JT_T), lds, st, a, a_of, ma, b, b_of, mb, joints, G0, movable, Z, K, J, ka, kb,
             sweeps, G, score, score0, joint_score, sweeps_used, accepted, kept_a, kept_b);
  PZN_RETURN_LAUNCH_STATUS();
}
