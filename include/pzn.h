/*
 * pzn.h — C ABI of libpzn.so, the MI355X (gfx950) hot path of PuzzleNet's
 * pairwise point-cloud forward/backward.
 *
 * Everything below is `extern "C"`, takes raw DEVICE pointers, sizes and a HIP
 * stream, and returns an int status (0 = PZN_OK, negative = error).  No torch
 * types, no exceptions across the boundary, no hidden allocation: the caller
 * owns every buffer (workspace sizes are queried with the *_workspace_bytes
 * helpers).  All kernels are enqueued on `stream` and return immediately.
 *
 * Each entry point cites the reference interface it replaces
 * (paths relative to the reference checkout, Gibbs-liu/PuzzleNet @ 2024_10_08).
 *
 * Conventions
 *   - float tensors are fp32, contiguous, row-major; index tensors are int64.
 *   - `B` batch (clouds), `N` points per cloud, `S` centroids/queries per
 *     cloud, `K` neighbours per query, `D` feature channels.
 *   - distances are ((dx*dx + dy*dy) + dz*dz) in fp32 WITHOUT fma contraction,
 *     which is bit-identical to pointnet_util.square_distance on CPU.
 */
#ifndef PZN_H_
#define PZN_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* pzn_stream_t; /* hipStream_t, passed opaquely (0 = null stream) */

enum {
  PZN_OK = 0,
  PZN_EINVAL = -1,       /* bad shape / null pointer / unsupported size */
  PZN_ELAUNCH = -2,      /* hipGetLastError() != hipSuccess after a launch */
  PZN_EUNSUPPORTED = -3, /* valid request this build cannot serve */
  PZN_ENODEVICE = -4     /* no HIP device / device is not gfx950 */
};

/* Library identification and error text. */
int pzn_version(void);
const char* pzn_strerror(int status);
/* 0 when a gfx950 device is usable by this process, PZN_ENODEVICE otherwise. */
int pzn_device_check(void);

/* Measurement only (bench.py; no counterpart in the reference): per-KERNEL device time.  pzn_ktimer_enable(1): every kernel
 * the library launches from now on is bracketed by a HIP event pair on its own stream, under the name a rocprofv3 kernel
 * trace shows (template arguments included).  pzn_ktimer_collect() waits for the recorded launches and folds them into
 * rows -> number of rows; pzn_ktimer_row(i, ...) reads one (name, launches, summed milliseconds).  Off by default. */
int pzn_ktimer_enable(int on);
int pzn_ktimer_collect(void);
int pzn_ktimer_row(int i, char* name, int cap, int* launches, double* ms);

/* ------------------------------------------------------------------------ */
/* Point ops: pointnet_util.py                                              */
/* ------------------------------------------------------------------------ */

/* pointnet_util.py:22-36  square_distance(src[B,S,3], dst[B,N,3]) -> [B,S,N]
 * Materialising form kept for API parity; the kNN / ball-query kernels never
 * build this tensor. */
int pzn_square_distance_f32(const float* src, const float* dst, int B, int S,
                            int N, float* out, pzn_stream_t stream);

/* pointnet_util.py:53-73  farthest_point_sample(xyz[B,N,3], npoint)
 * `start_idx[B]` carries the reference's torch.randint draw (line 65) so the
 * kernel itself is deterministic.  out_idx is int64 [B,npoint]. Ties in the
 * arg-max resolve to the LOWEST index (torch.max on CPU). */
int pzn_fps_f32(const float* xyz, int B, int N, int npoint,
                const int64_t* start_idx, int64_t* out_idx,
                pzn_stream_t stream);
/* dataset.py:1147-1163 (`fps` of a raw piece in the loader processes) as a background job beside a training step: the same
 * picks bit for bit, but no LDS image of the cloud (1.2 KB of LDS per workgroup instead of up to 150 KB), so the step's
 * LDS-tiled kernels keep their CUs.  N <= 32768.  counts (NULL or int64 [B]): rows >= counts[b] of cloud b are padding
 * (copies of row 0, which never win) and are left out of the rounds.  max_count (0: unknown): the caller's promise that
 * counts[b] <= max_count for every cloud - a cut piece holds at most M - n of the raw cloud's M points - which lets the
 * launch hold only that many rows in registers (fewer, faster wavefronts); rows beyond it are never read.  counts[b] < 0 =
 * a piece that does not exist (pzn_cut_compact_double_f32): a workgroup all of whose pieces are such writes index 0 to every
 * output slot of them and returns without a round; beside a real piece in the same workgroup (B even: pieces b and b + B / 2
 * share one) it counts as 1 row, as counts[b] = 0 does. */
int pzn_fps_background_f32(const float* xyz, int B, int N, int npoint,
                           const int64_t* start_idx, int64_t* out_idx,
                           const int64_t* counts, int max_count, pzn_stream_t stream);

/* Merge two placed pieces and resample the union (no counterpart in the reference, which ships no assembly code; the rounds
 * are pointnet_util.py:53-73): M merges in one launch, one workgroup each.  The union of merge m has Na + Nb rows: rows
 * 0..Na-1 are a[m] [Na,3] as read, rows Na.. are b[m] [Nb,3] moved by T[m] ([4,4] row-major, as pzn_se3_exp_fwd_f32 writes
 * it): x' = ((R00 x + R01 y) + R02 z) + t0 and likewise y', z', every product and sum rounded to fp32 on its own.
 * Farthest point sampling of the union for n_out rounds, the arithmetic and the tie rule of pzn_fps_f32 (lowest union index),
 * gives out[M,n_out,3] (the picked coordinates in pick order) and src[M,n_out] (int64 union index of every pick).
 * drop_a[M,ka], drop_b[M,kb] (int64 rows of a / b; NULL or a count of 0: none; repeats allowed; an index outside its cloud
 * is ignored): listed rows start with running distance 0 instead of 1e10 and are otherwise rows like any other, so one
 * is picked only when every kept row is at distance 0 too.  start[M]: the union index sampling begins at (clamped to the
 * union); if that row is dropped, the first kept row at or after it, wrapping round to 0.
 * Na + Nb <= 4096 and 1 <= n_out <= Na + Nb (pzn_merge_resample_supported: 1 / 0); PZN_EUNSUPPORTED otherwise. */
int pzn_merge_resample_supported(int Na, int Nb, int n_out);
int pzn_merge_resample_f32(const float* a, const float* b, const float* T, const int64_t* start,
                           const int64_t* drop_a, int ka, const int64_t* drop_b, int kb, int M, int Na, int Nb,
                           int n_out, float* out, int64_t* src, pzn_stream_t stream);

/* Refine P poses on their matched point sets by symmetric point-to-point ICP (no counterpart in the reference): one launch,
 * one workgroup per problem, no workspace, no atomics, nothing waits for the device.  Problem p has the fixed set
 * a[a_of ? a_of[p] : p] [ka,3], the moved set b[b_of ? b_of[p] : p] [kb,3] (a_of / b_of: NULL or int64 [P] rows of a / b,
 * so one set can serve many problems) and the start pose T0[p] ([4,4] row-major, as pzn_se3_exp_fwd_f32 writes it).
 * A pose moves a point as pzn_merge_resample_f32 does: x' = ((R00 x + R01 y) + R02 z) + t0, each operation rounded to fp32.
 * Objective E(T) = mean_i min_j |a_i - T b_j|^2 + mean_j min_i |a_i - T b_j|^2 (fp32 differences, lowest index on ties,
 * sums in a fixed order).  One iteration: the arg-mins c1(i), c2(j) under T give ka + kb pairs; the candidate T' is their
 * least-squares rigid motion (centred float64 sums, Horn's quaternion in float64 = Kabsch with the reflection fix), rounded to
 * fp32; E(T') < E(T) takes it, anything else stops.  Pairs whose moved-side points are one point, coincident or collinear
 * (sum of the principal 2x2 minors of their scatter <= 1e-10 trace^2) keep the rotation and update the translation only.
 * Out: T[P,4,4] (last row exactly 0 0 0 1), score[P] = E(T) <= score0[P] = E(T0), iters_used[P] (int32, accepted
 * candidates), and, when non-NULL, corr_a[P,ka] / corr_b[P,kb] (int32): the c1 / c2 the last candidate was built from
 * (those under T0 when iters = 0).  iters = 0 returns T0.  1 <= ka, kb <= 1024 (pzn_icp_refine_supported: 1 / 0) and
 * iters >= 0, PZN_EUNSUPPORTED otherwise, before any launch; P = 0 is a success that launches nothing. */
int pzn_icp_refine_supported(int ka, int kb);
int pzn_icp_refine_f32(const float* a, const int64_t* a_of, const float* b, const int64_t* b_of,
                       const float* T0, int P, int ka, int kb, int iters,
                       float* T, float* score, float* score0, int32_t* iters_used,
                       int32_t* corr_a, int32_t* corr_b, pzn_stream_t stream);
/* pzn_icp_refine_f32 for partial contact: of each direction's rows only a fixed number counts, keep_a of the ka rows of a and
 * keep_b of the kb rows of b, so the faces of a piece that belong to other neighbours neither score nor pull.  Inputs, the
 * arithmetic of a pose and of a distance, the row minima and their arg-mins are pzn_icp_refine_f32's.
 * Kept set of a direction under a pose: its m rows with the smallest (row minimum, row index) in lexicographic order - among
 * equal minima the lowest row index is kept; exactly m rows whatever the ties.
 * Objective E(T) = (sum of the kept a-row minima) / keep_a + (sum of the kept b-row minima) / keep_b, the kept minima added
 * in pzn_icp_refine_f32's order with the other rows skipped.  One iteration: the keep_a + keep_b pairs of the kept rows
 * alone, each of one weight, give the candidate (centroids, cross-covariance, the degenerate rule and Horn's solve as there,
 * the divisor keep_a + keep_b); E(T') < E(T), each with its own pose's kept sets, takes it, anything else (NaN included)
 * stops.  So score <= score0 holds to the bit.
 * Out: T, score, score0, iters_used, corr_a / corr_b with pzn_icp_refine_f32's meaning (corr_* hold the arg-min of EVERY
 * row, kept or not), and, when non-NULL, kept_a[P,keep_a] / kept_b[P,keep_b] (int32, ascending): the rows kept under the
 * RETURNED T, whether or not the last candidate was rejected (the kernel holds the current pose's mask and the candidate's
 * side by side); with iters = 0 the rows kept under T0.  The same bits on every run.
 * keep_a = ka and keep_b = kb is pzn_icp_refine_f32 bit for bit on every shared output, with kept_* = 0 .. k-1.
 * 1 <= ka, kb <= 1024, 1 <= keep_a <= ka, 1 <= keep_b <= kb (pzn_icp_refine_trim_supported: 1 / 0) and iters >= 0,
 * PZN_EUNSUPPORTED otherwise, before any launch; P = 0 is a success that launches nothing. */
int pzn_icp_refine_trim_supported(int ka, int kb, int keep_a, int keep_b);
int pzn_icp_refine_trim_f32(const float* a, const int64_t* a_of, const float* b, const int64_t* b_of,
                            const float* T0, int P, int ka, int kb, int keep_a, int keep_b, int iters,
                            float* T, float* score, float* score0, int32_t* iters_used,
                            int32_t* corr_a, int32_t* corr_b, int32_t* kept_a, int32_t* kept_b,
                            pzn_stream_t stream);
/* pzn_icp_refine_trim_f32 with the two counts found per problem and per EVALUATION of a pose instead of given per launch
 * (Trimmed ICP's search for the overlap, its objective e(xi) / xi^(1 + lambda) with 1 + lambda = power): a sibling pair mates
 * along a whole face, two pieces across an older cut along a corner, and one launch serves both.  In place of keep_a, keep_b
 * the launch takes the least counts 1 <= lo_a <= ka, 1 <= lo_b <= kb and an integer power p in [1, 4].  The rule:
 *  1. row minima, arg-mins and the (value, row index) order of each direction: the trimmed kernel's, ranked by counting;
 *  2. one direction with n rows: its minima in that order, w_1 <= ... <= w_n, their float32 prefix sums S_m, and
 *     phi(m) = (double)S_m / m^(p+1), the power by repeated multiplication in float64 (exact: m <= 1024, p + 1 <= 5), the
 *     division in float64.  Order of the prefix sums (the same on every run): thread t of 256 adds w_(4t+1) .. w_(4t+4) one
 *     after the other from 0 (values past n count as 0); each wavefront scans its 64 thread totals inclusively, lane l adding
 *     lane l - d's running value for d = 1, 2, 4, 8, 16, 32 in turn; the totals of the wavefronts before a thread's are added
 *     in wavefront order from 0; S_(4t+i) = ((that offset + the scan's value of the lane before, 0 for lane 0) + the thread's
 *     own running sum up to i), every addition rounded to float32;
 *  3. count: m* = the m in [lo, n] with the smallest phi, among equal phi the LARGEST m (all minima zero keeps every row);
 *  4. kept set: rank < m*, as in the trimmed kernel;
 *  5. e_a, e_b: what the trimmed kernel computes for those counts (kept minima in row-ownership order, butterfly, wave order,
 *     one correctly rounded division by m*), not taken from the prefix sums;
 *  6. objective F = e_a r_a + e_b r_b, each product and the sum rounded to float32, r = (float)(q^p) with q = (double)n /
 *     (double)m* and the power by repeated multiplication in float64 (F = n^p phi(m*) per direction, up to rounding);
 *  7. score = e_a + e_b, the trimmed kernel's E at these counts: the quantity, in the units, a trimmed table compares;
 *  8. step: the trimmed step over the m_a + m_b kept pairs of the current pose; the candidate is taken iff F' < F, each with
 *     its own pose's counts and kept sets; anything else (NaN included) stops.  F falls along a run; score need not;
 *  9. the counts, like the kept masks, belong to a pose and swap on acceptance: every output is the RETURNED pose's.
 * Out beside the trimmed launch's T, score, score0 (E under T0 at T0's counts), iters_used, corr_a, corr_b: count_a[P],
 * count_b[P] (int32), objective[P] (float32, F), and when non-NULL kept_a[P,ka] / kept_b[P,kb] (int32): the count kept rows
 * ascending, then -1 up to the row's end.  lo_a = ka and lo_b = kb gives r = 1, F = E and pzn_icp_refine_trim_f32 with
 * keep = (ka, kb) bit for bit, hence pzn_icp_refine_f32.  60.5 KB of LDS at ka = kb = 1024.
 * Supported (pzn_icp_refine_auto_supported: 1 / 0) for 1 <= ka, kb <= 1024, 1 <= lo_a <= ka, 1 <= lo_b <= kb, 1 <= power <= 4;
 * otherwise, and for iters < 0, PZN_EUNSUPPORTED before any launch; P = 0 is a success that launches nothing. */
int pzn_icp_refine_auto_supported(int ka, int kb, int lo_a, int lo_b, int power);
int pzn_icp_refine_auto_f32(const float* a, const int64_t* a_of, const float* b, const int64_t* b_of,
                            const float* T0, int P, int ka, int kb, int lo_a, int lo_b, int power, int iters,
                            float* T, float* score, float* score0, int32_t* iters_used,
                            int32_t* corr_a, int32_t* corr_b, int32_t* count_a, int32_t* count_b, float* objective,
                            int32_t* kept_a, int32_t* kept_b, pzn_stream_t stream);

/* Refine all piece poses of Z placed assemblies jointly over every joint (no counterpart in the reference): one launch, one
 * workgroup per puzzle, no workspace, no atomics, no grid-wide synchronisation, nothing waits for the device.  Puzzle z has
 * K poses G0[z] ([K,4,4] row-major, piece frame to root frame), the mask movable[z] ([K] bytes, non-zero = may move) and J
 * joint rows joints[z] ([J,2] int32: the ordered pair (i, j)).  Row e has the set A_e = a[a_of ? a_of[z J + e] : z J + e]
 * [ka,3] in piece i's frame and B_e = b[b_of ? b_of[z J + e] : z J + e] [kb,3] in piece j's frame (a_of / b_of: NULL or int64
 * [Z,J] rows of a / b, so one set can serve many joints).  A row with i < 0 is unused; a row with i or j outside [0, K) or
 * i == j is skipped in the same way (the device does not report it; callers check their own host copy).  A pair listed twice
 * counts twice, and a piece that is an end of more than 2 K rows - possible only that way - is never visited.
 * Energy of a joint: E_e(G) = mean_r min_c |G_i a_r - G_j b_c|^2 + mean_c min_r |G_i a_r - G_j b_c|^2, points moved and
 * distances formed as pzn_icp_refine_f32 does (fp32, lowest index on ties, sums in a fixed order); E_p = the fp32 sum in row
 * order of E_e over the rows with i = p or j = p; E = that sum over all rows.
 * A visit of piece p: the arg-mins of p's joints under G give, per joint, ka pairs of weight 1 / ka and kb pairs of weight
 * 1 / kb, each (x = the point of p's side in p's frame, y = its partner's fp32 root-frame image); the candidate G_p' is their
 * weighted least-squares rigid motion (float64 sums, Horn's quaternion in float64, rounded to fp32; a degenerate scatter of
 * x by pzn_icp_refine_f32's rule keeps R_p and updates t); it is taken iff E_p' < E_p, anything else (NaN included) keeps
 * G_p.  Only p's joints depend on G_p, so E falls with E_p; the fp32 sum E is held to that too: a candidate under which E
 * would round above its current value (a matter of the last place) is left, so score <= score0 holds to the bit.  A sweep visits p = 0 .. K-1 in order, skipping pieces that are not movable or have no joint; later pieces see the
 * earlier pieces' new poses.  The loop ends after `sweeps` sweeps or after a sweep that took nothing.
 * Out: G[Z,K,4,4] (last rows exactly 0 0 0 1), score[Z] = E(G), score0[Z] = E(G0), joint_score[Z,J] = E_e(G) (0 for a
 * skipped row), sweeps_used[Z] (int32: sweeps that took at least one candidate), accepted[Z,K] (int32: candidates taken per
 * piece).  sweeps = 0 returns G0.  The same bits on every run.
 * 1 <= K <= 64, 0 <= J <= K (K - 1), 1 <= ka, kb <= 1024 (pzn_joint_refine_supported: 1 / 0) and sweeps >= 0,
 * PZN_EUNSUPPORTED otherwise, before any launch; Z = 0 or J = 0 is a success that launches nothing and writes nothing (the
 * answer is G0 with scores of 0; ops.joint_refine fills it in). */
int pzn_joint_refine_supported(int K, int J, int ka, int kb);
int pzn_joint_refine_f32(const float* a, const int64_t* a_of, const float* b, const int64_t* b_of,
                         const int32_t* joints, const float* G0, const uint8_t* movable,
                         int Z, int K, int J, int ka, int kb, int sweeps,
                         float* G, float* score, float* score0, float* joint_score,
                         int32_t* sweeps_used, int32_t* accepted, pzn_stream_t stream);
/* pzn_joint_refine_f32 with a point count per set instead of one per launch (the joints of a table whose kept counts differ
 * per pair, pzn_icp_refine_auto_f32's): the same kernel body, the same limits (pzn_joint_refine_supported), the same outputs.
 * na: NULL or int32 with one entry per SET of a, indexed by the set and not by the row - row z J + e reads
 * na[a_of ? a_of[z J + e] : z J + e] - so one array serves every joint that uses the set; nb likewise for b.  NULL means ka /
 * kb for every set.  Set s of a holds na[s] points in its FIRST rows; the rows behind them are never read and may hold
 * anything, NaN included.  ka, kb stay the strides of a and b and size the LDS, whose footprint does not change.
 * Wherever pzn_joint_refine_f32's contract says ka / kb for row e, this one reads that row's na / nb:
 * E_e = (sum of the na row minima) / na + (sum of the nb row minima) / nb, the divisors (float)na and (float)nb; row r < na is
 * a row of A and row na + c one of B, a thread owning rows tid, tid + 256, ... of these na + nb; the pairs of a visit weigh
 * 1 / na and 1 / nb (float64).  The reference point, Horn's solve, the degenerate rule, the acceptance E_p' < E_p and the held
 * fp32 total are unchanged.  The sets are frozen: nothing is trimmed again under the joint poses.
 * A row whose na is outside [1, ka] or whose nb is outside [1, kb] is skipped exactly like a row with a bad (i, j):
 * joint_score 0, no part in any E_p or visit (the device does not report it; callers check their own host copy).  The counts
 * of a row with a bad (i, j) are not read, and neither are its a_of / b_of.
 * na = nb = NULL: every output is pzn_joint_refine_f32's, bit for bit (it is that launch); so is every output with all
 * counts equal to ka / kb, and with all sets at one (m_a, m_b) the outputs are those of pzn_joint_refine_f32 on the sets cut
 * to [m_a,3] / [m_b,3]. */
int pzn_joint_refine_counts_f32(const float* a, const int64_t* a_of, const int32_t* na,
                                const float* b, const int64_t* b_of, const int32_t* nb,
                                const int32_t* joints, const float* G0, const uint8_t* movable,
                                int Z, int K, int J, int ka, int kb, int sweeps,
                                float* G, float* score, float* score0, float* joint_score,
                                int32_t* sweeps_used, int32_t* accepted, pzn_stream_t stream);
/* pzn_joint_refine_f32 for partial contact: of each joint's rows only a given number counts, and WHICH rows is decided again
 * at every evaluation, under the poses at hand (pzn_icp_refine_trim_f32's rule carried to the pose graph; a kernel of its own,
 * joint_trim_kernel).  Everything of pzn_joint_refine_f32 stands: the joint list, movable, the sets a[a_of] with ka rows and
 * b[b_of] with kb rows, the fp32 images, the distances, the row minima and their lowest-index arg-mins, the visit order, the
 * two acceptance guards, the outputs, and a skipped row scoring 0.  New are two counts per joint ROW, ma[z,e] in [1, ka] and
 * mb[z,e] in [1, kb] (int32 [Z,J]; per row and not per set, because a set is shared by all joints of its piece while a count
 * belongs to an ordered pair; NULL means ka / kb for every row).
 * Kept set: of the ka rows of A under the poses at hand the ma rows with the smallest (row minimum, row index) in
 * lexicographic order are kept, of the kb rows of B the mb - ranked by counting, exactly m rows whatever the ties.
 * Energy: E_e = (sum of the kept A-row minima) / ma + (sum of the kept B-row minima) / mb, the kept minima added in
 * pzn_joint_refine_f32's order with the other rows left out (a thread's rows in order, the butterfly, the wave order), the
 * divisors (float)ma and (float)mb.
 * Visit of piece p: only the pairs of the kept rows of p's joints enter the 22 float64 sums, with weights 1 / ma and 1 / mb; the
 * reference point, Horn's solve and the degenerate rule are unchanged.
 * Acceptance: the candidate is evaluated with ITS OWN kept sets and taken iff E_p' < E_p and the fp32 total does not round
 * above the current one; score <= score0 holds to the bit.
 * Out beside pzn_joint_refine_f32's: when non-NULL, kept_a[Z,J,ka] / kept_b[Z,J,kb] (int32): the rows kept under the RETURNED
 * poses, positions ascending, -1 behind the count, all -1 for a skipped row.  The same bits on every run.
 * A row whose ma is outside [1, ka] or whose mb is outside [1, kb] is skipped like a row with a bad (i, j); the counts of a row
 * with a bad (i, j) are not read.  ma = ka and mb = kb on every row (or both NULL) is pzn_joint_refine_f32 bit for bit on all
 * six shared outputs, with kept_* = 0 .. k-1.
 * The range is pzn_joint_refine_f32's (pzn_joint_refine_trim_supported: 1 / 0): the row minima and arg-mins take the LDS image
 * from 56.3 KB to 68.3 KB at K = 64, J = 4032, ka = kb = 1024, and the launch RAISES the kernel's dynamic LDS limit for such
 * shapes rather than narrowing the range.  sweeps < 0 or a shape outside it: PZN_EUNSUPPORTED before any launch; Z = 0 or
 * J = 0 is a success that launches nothing and writes nothing. */
int pzn_joint_refine_trim_supported(int K, int J, int ka, int kb);
int pzn_joint_refine_trim_f32(const float* a, const int64_t* a_of, const int32_t* ma,
                              const float* b, const int64_t* b_of, const int32_t* mb,
                              const int32_t* joints, const float* G0, const uint8_t* movable,
                              int Z, int K, int J, int ka, int kb, int sweeps,
                              float* G, float* score, float* score0, float* joint_score,
                              int32_t* sweeps_used, int32_t* accepted, int32_t* kept_a, int32_t* kept_b,
                              pzn_stream_t stream);
/* pzn_joint_refine_trim_f32 with the two counts of every joint FOUND at every evaluation of the joint, under whatever poses
 * are being tried, instead of given per row (pzn_icp_refine_auto_f32's count search carried to the pose graph; a kernel of its
 * own, joint_auto_kernel, one launch for Z puzzles).  Inputs: everything of pzn_joint_refine_trim_f32 except ma and mb; in
 * their place, per launch, the least counts 1 <= lo_a <= ka, 1 <= lo_b <= kb and the integer power p in [1, 4], with
 * pzn_icp_refine_auto_f32's meaning.
 * Evaluation of joint row e under poses G: the images, distances, row minima and lowest-index arg-mins are
 * pzn_joint_refine_trim_f32's.  Steps 1 to 7 of the rule above pzn_icp_refine_auto_f32 then apply to the ka row minima of A and
 * the kb row minima of B, the order of the float32 prefix sums (thread by thread, as stated there) and the tie rules (the larger
 * m among equal phi, the lower row index among equal minima) included.  It yields m_a, m_b, the kept rows, E_e = e_a + e_b (the
 * trimmed energy at these counts, summed as pzn_joint_refine_trim_f32 sums it) and F_e = e_a r_a + e_b r_b, each product and
 * the sum rounded to float32, r = (float)(q^p), q = (double)k / (double)m, the power by repeated multiplication in float64.
 * F_p = the fp32 sum in row order of F_e over the rows with i = p or j = p; F = that sum over all rows (formed exactly as E_p
 * and E are formed by pzn_joint_refine_f32).
 * Visit of piece p: only the kept pairs of p's joints enter the 22 float64 sums, with weights r_a / m_a and r_b / m_b in
 * float64 (r = q^p as above, before its cast to float, then one division by (double)m): the candidate then minimises F_p for the
 * sets and counts at hand; the joints of one piece are summed, so their relative weight matters.  At lo = k the weight is
 * 1 / k, pzn_joint_refine_trim_f32's.  The reference point, Horn's solve and the degenerate rule are unchanged.
 * Acceptance: the candidate is evaluated with ITS OWN counts and kept sets and taken iff F_p' < F_p and the fp32 total F does
 * not round above its current value; anything else (NaN included) keeps G_p.  So objective <= objective0 holds to the bit.
 * F falls along a run; score, the sum of E_e at counts that move with the poses, need not.
 * Out: the six of pzn_joint_refine_f32, in the units a trimmed table compares - score[Z] and score0[Z] are the sums of E_e under
 * G and under G0, joint_score[Z,J] is E_e(G) (0 for a skipped row) - and objective[Z], objective0[Z]: the sums of F_e under G
 * and under G0; count_a[Z,J], count_b[Z,J] (int32; 0 for a skipped row); and, when non-NULL, kept_a[Z,J,ka] / kept_b[Z,J,kb]
 * (int32): the kept rows ascending, -1 behind the count, all -1 for a skipped row.  Every output is that of the RETURNED poses:
 * joint_score, the counts and the kept rows are written in one last evaluation of every joint after the loop.  The same bits
 * on every run.
 * lo_a = ka and lo_b = kb is pzn_joint_refine_f32 bit for bit on the six shared outputs, with objective == score, every count
 * k and kept_* = 0 .. k-1.
 * The range is pzn_joint_refine_trim_supported's plus the three new arguments (pzn_joint_refine_auto_supported: 1 / 0).  The
 * sorted minima add 4 (ka + kb) bytes of LDS, 76.3 KB at K = 64, J = 4032, ka = kb = 1024; the launch raises the kernel's
 * dynamic LDS limit for such shapes.  sweeps < 0 or anything outside the range: PZN_EUNSUPPORTED before any launch; Z = 0 or
 * J = 0 is a success that launches nothing and writes nothing. */
int pzn_joint_refine_auto_supported(int K, int J, int ka, int kb, int lo_a, int lo_b, int power);
int pzn_joint_refine_auto_f32(const float* a, const int64_t* a_of, const float* b, const int64_t* b_of,
                              const int32_t* joints, const float* G0, const uint8_t* movable,
                              int Z, int K, int J, int ka, int kb, int lo_a, int lo_b, int power, int sweeps,
                              float* G, float* score, float* score0, float* joint_score,
                              int32_t* sweeps_used, int32_t* accepted, float* objective, float* objective0,
                              int32_t* count_a, int32_t* count_b, int32_t* kept_a, int32_t* kept_b,
                              pzn_stream_t stream);

/* The greedy walk over Z pair tables and the joint list of every walk (no counterpart in the reference; assembly.assemble and
 * the joint selection of assembly.refine_assembly for Z puzzles): one launch, one wavefront per puzzle, no workspace, no
 * atomics, nothing waits for the device.  Puzzle z has score[z] ([K,K] fp32) and T[z] ([K,K,4,4] fp32, T[i,j] maps piece j
 * into piece i's frame) and count[z] pieces (int32 [Z]; NULL: K for every puzzle): only entries with i, j < count[z] exist, and
 * nothing else of score or T is read.  A count outside [2, K] gives root -1, nothing placed, no edge and no joint.
 * Key of entry (i, j): its fp32 score; NaN and the diagonal count as +inf.  Keys compare as floats (-0 equals 0); of equal
 * keys the lowest i K + j is the smaller.
 * Walk: root[z] = the row of the smallest key; placed = {root}.  A round takes the smallest key among the ordered pairs
 * with exactly one end placed; the walk stops at a key that is not finite or at (double)key > max_score (+inf: never; NaN is
 * PZN_EINVAL).  A placed fixed end i gives G[j] = G[i] T[i,j], otherwise G[i] = G[j] inv(T[i,j]) with inv = [R^T, -(R^T t)]
 * and the last row 0 0 0 1.  Poses are float64 from the fp32 T, every operation rounded on its own: an entry of a 4x4 product
 * is ((a0 b0 + a1 b1) + a2 b2) + a3 b3 over all four terms, an entry of R^T t is (r0 t0 + r1 t1) + r2 t2.  Unplaced pieces
 * keep the identity.
 * Joints: every (i, j), i != j, both placed, with (double)score[i,j] <= joint_score on the score as stored (NaN is never a
 * joint; +inf is one under joint_score = +inf); joint_score = NaN means the largest edge score of that puzzle, and no joint
 * where the walk made no edge.
 * Out: root[Z] int32; edges[Z,K-1,3] int32 rows (i, j, new) in placement order and edge_score[Z,K-1] (the score as stored),
 * unused rows -1 and +inf; n_edges[Z] int32; G[Z,K,4,4] float64; placed[Z,K] bytes 0 / 1; joints[Z,K(K-1),2] int32 in
 * row-major order of (i, j), unused rows (-1, -1); n_joints[Z] int32.  The same bits on every run.
 * 2 <= K <= 64 (pzn_assemble_walk_supported: 1 / 0), PZN_EUNSUPPORTED otherwise, before any launch; Z = 0 is a success that
 * launches nothing. */
int pzn_assemble_walk_supported(int K);
int pzn_assemble_walk_f32(const float* score, const float* T, const int32_t* count,
                          double max_score, double joint_score, int Z, int K,
                          int32_t* root, int32_t* edges, float* edge_score, int32_t* n_edges,
                          double* G, uint8_t* placed, int32_t* joints, int32_t* n_joints,
                          pzn_stream_t stream);

/* The beam walk over Z pair tables, scored by the placed pieces' votes (no counterpart in the reference; assembly.beam_rule is
 * the numpy statement): one launch, one wavefront per puzzle, no workspace, no atomics, nothing waits for the device.
 * score, T, count, max_score and joint_score are pzn_assemble_walk_f32's; keys, their order and ties, the root, the pose
 * arithmetic (an entry of a product is dot4(a0,b0,a1,b1,a2,b2,a3,b3) = ((a0 b0 + a1 b1) + a2 b2) + a3 b3, the rigid inverse) and
 * the meaning of count are its own, word for word.  moment[z] ([K,4,4] float64): moment[n] = the mean over piece n's picked
 * boundary points x of (x, 1) (x, 1)^T.  beam B, branch C; weight (double; NaN is PZN_EINVAL); vote_score (double; NaN means
 * max_score).
 * Hypothesis: a placed set, a float64 pose for every placed piece, its edges in placement order and a float64 cost.  Round 0
 * has one: {root}, cost 0.
 * Candidates of a hypothesis: the ordered pairs (i, j), i, j < count, with exactly one end placed, a finite key and
 * (double)key <= max_score; the first C of them in the order (key, i K + j), rank = the position 0 .. C-1.  (The list ends at
 * the first key that fails, as the walk stops there: a key of -inf ends it as well.)  Several candidates may place the same
 * piece through different entries.
 * Child of candidate (i, j): its new piece n and pose Gn follow the walk's rule.  Its votes: over the hypothesis' placed pieces
 * p in ascending order, entry (p, n) and then entry (n, p), without the candidate's own entry and without an entry whose key
 * is not finite or has (double)key > vote_score.  A vote predicts Q = G[p] T[p,n] or Q = G[p] inv(T[n,p]) and disagrees by d:
 * D = Q - Gn on rows 0..2; for row u, m_v = dot4(M[v][0], D[u][0], M[v][1], D[u][1], M[v][2], D[u][2], M[v][3], D[u][3]) with
 * M = moment[n] and q_u = dot4(D[u][0], m_0, D[u][1], m_1, D[u][2], m_2, D[u][3], m_3); d = (q_0 + q_1) + q_2 - the mean over
 * n's boundary points of |Q x - Gn x|^2, in the unit of score.  penalty = (0 + d_1 + d_2 + ...) summed in vote order, divided by
 * the number of votes; 0 with no vote.  Child cost = (parent cost + (double)key) + weight * penalty, every operation rounded on
 * its own; with weight == 0 the last term is neither computed nor added; a NaN cost becomes +inf.
 * Selection: all children of the round in the order (cost, parent slot, rank) - costs compare as doubles, -0 equals 0 -, each
 * kept unless a kept child has the same placed set, until B are kept; the kept order is the next round's slot order.  A
 * hypothesis without a candidate has no child; a round without any child ends the walk.  All live hypotheses hold the same
 * number of pieces.
 * Out: the result is slot 0, in pzn_assemble_walk_f32's outputs (root, edges, edge_score, n_edges, G, placed, and joints /
 * n_joints by the walk's joint rule from the result's own edges); cost[Z,B] float64 in slot order, unused slots +inf;
 * n_hyp[Z] int32, the live hypotheses.  A count outside [2, K] gives the walk's empty answer and n_hyp 0.  With B = C = 1
 * every walk output is pzn_assemble_walk_f32's bit for bit, whatever weight is.  The same bits on every run.
 * 2 <= K <= 64, 1 <= B, C <= 8 (pzn_assemble_beam_supported: 1 / 0; each of a round's B C children has a lane, two generations of
 * hypotheses are 2 B (128 K + 4 (K - 1) + 16) bytes of LDS), PZN_EUNSUPPORTED otherwise, before any launch; Z = 0 is a success
 * that launches nothing. */
int pzn_assemble_beam_supported(int K, int B, int C);
int pzn_assemble_beam_f32(const float* score, const float* T, const double* moment, const int32_t* count,
                          int beam, int branch, double weight, double max_score, double vote_score,
                          double joint_score, int Z, int K,
                          int32_t* root, int32_t* edges, float* edge_score, int32_t* n_edges,
                          double* G, uint8_t* placed, int32_t* joints, int32_t* n_joints,
                          double* cost, int32_t* n_hyp, pzn_stream_t stream);

/* The forest walk over Z pair tables: a pile of pieces of several objects, sorted and assembled (no counterpart in the
 * reference; assembly.forest_rule is the numpy statement): one launch, one wavefront per pile, no workspace, no atomics, nothing
 * waits for the device.  score, T, count, max_score and joint_score are pzn_assemble_walk_f32's; keys, their order and ties, the
 * stop test, the pose arithmetic and the meaning of count are its own, word for word.  A piece is inside once it has a pose,
 * outside until then; only pieces < count[z] are either.
 * Walk: while a piece is outside, a component starts and grows.
 *   Start: with two or more pieces outside, the root of the new component is the row i of the smallest key among the entries
 *   (i, j), i != j, with both ends outside (of equal keys the lowest i K + j) - with nothing inside yet, the walk's root -; with
 *   one piece outside, that piece.  The root's pose is the identity, and it is inside.
 *   Rounds: the walk's.  A round takes the smallest key among the ordered pairs with exactly one end inside, whichever component
 *   that end is in, and stops the component at a key that is not finite or at (double)key > max_score.  The new piece's pose is
 *   G[j] = G[i] T[i,j] or G[i] = G[j] inv(T[i,j]) from the pose of the end inside, and it belongs to the component that is
 *   growing.  (On a table without -inf every entry between an older component and the outside has failed the stop test already,
 *   so the end inside is in the growing component and the pose in its root's frame.)
 * The components are numbered in the order they start; every start places a piece, so there are at most count of them, and a
 * component may be a single piece.  On a table without -inf they are the connected components of the graph whose edges are the
 * entries with a finite key <= max_score (single linkage).
 * Joints: every (i, j), i != j, in the same component, with (double)score[i,j] <= joint_score on the score as stored;
 * joint_score = NaN means the largest edge score of the pile, and no joint in a pile without an edge.
 * Out: pzn_assemble_walk_f32's eight outputs - root[Z] = roots[z,0]; edges[Z,K-1,3], edge_score[Z,K-1] and n_edges[Z] over all
 * components in placement order (at most count - 1 edges); G[Z,K,4,4], piece p into the frame of its own component's root;
 * placed[Z,K], 1 for every p < count; joints[Z,K(K-1),2] row-major, n_joints[Z] - then component[Z,K] int32 (the component of
 * every piece, -1 at and beyond count), roots[Z,K] int32 (the root of component q, unused -1) and n_components[Z] int32.  A count
 * outside [2, K] gives the walk's empty answer, all components -1 and n_components 0.  The first component is the walk's
 * result: its root, its edges as the first edges, its poses bit for bit; where the walk places every piece, all eight shared
 * outputs are the walk's.  The same bits on every run.
 * 2 <= K <= 64 (pzn_assemble_forest_supported: 1 / 0), PZN_EUNSUPPORTED otherwise, before any launch; Z = 0 is a success that
 * launches nothing. */
int pzn_assemble_forest_supported(int K);
int pzn_assemble_forest_f32(const float* score, const float* T, const int32_t* count,
                            double max_score, double joint_score, int Z, int K,
                            int32_t* root, int32_t* edges, float* edge_score, int32_t* n_edges,
                            double* G, uint8_t* placed, int32_t* joints, int32_t* n_joints,
                            int32_t* component, int32_t* roots, int32_t* n_components,
                            pzn_stream_t stream);

/* The forest beam over Z pair tables: pzn_assemble_beam_f32 with pzn_assemble_forest_f32's restarts (no counterpart in the
 * reference; assembly.forest_beam_rule is the numpy statement): one launch, one wavefront per pile, no workspace, no atomics,
 * nothing waits for the device.  score, T, moment, count, beam B, branch C, weight, max_score, vote_score and joint_score are
 * pzn_assemble_beam_f32's; keys, their order and ties, count, the stop test, the pose arithmetic (dot4, the rigid inverse,
 * float64, every operation rounded on its own) and the joint rule are the walk's, word for word.  restart_cost (double): NaN
 * means max_score where that is finite, else 0 - single linkage under a threshold t is what minimises the sum of the edge scores
 * + t (the number of components), and the beam's cost extends that objective by the votes; without a threshold a restart only
 * happens at a wall of non-finite keys, where nothing was refused.
 * Hypothesis: a placed set, a float64 pose and a component for every placed piece, the roots of its components in the order
 * they started, its edges in placement order and a float64 cost.  Round 0 has one: the beam's root (the row of the smallest key)
 * as component 0 with the identity, cost 0.  There are exactly count - 1 rounds; every child places exactly one piece, so all live
 * hypotheses hold the same number of pieces, and a hypothesis always has a child.
 * Candidates of a hypothesis: the beam's - the first C ordered pairs with exactly one end placed in the order (key, i K + j), keys
 * finite and (double)key <= max_score; the placed end may be in any component, and the new piece joins the component of the
 * placed end.
 * Growth child of candidate (i, j): cost = (parent + (double)key) + weight * penalty as in the beam, the voters being the placed
 * pieces p of the component the new piece joins: p ascending, entry (p, n) then (n, p), not the candidate's own entry, keys
 * finite and (double)key <= vote_score.  Pieces of other components live in unrelated frames and do not vote.
 * Restart: a hypothesis with no candidate has one child of rank 0.  Its new root is the forest walk's: with two or more pieces
 * outside, the row i of the smallest key among the entries (i, j), i != j, with both ends outside (of equal keys the lowest
 * i K + j); with one piece outside, that piece.  The root gets the identity and opens the next component; the restart adds no
 * edge and costs parent + restart_cost (no penalty term).
 * Selection: the beam's - a NaN cost is +inf, the order is (cost, parent slot, rank), each child kept unless a kept child has the
 * same placed set, until B are kept.
 * Out: the result is slot 0, in pzn_assemble_forest_f32's eleven outputs - root[Z] = roots[z,0]; edges, edge_score, n_edges over
 * all components in placement order (n_edges + n_components = count); G[p] in the frame of p's own root; placed 1 for every
 * p < count; joints only inside a component, from the result's own edges; component[Z,K], roots[Z,K], n_components[Z] - then
 * cost[Z,B] float64 in slot order (unused +inf) and n_hyp[Z] int32.  A count outside [2, K] gives the walk's empty answer, no
 * component and n_hyp 0.  With B = C = 1 the eleven outputs are pzn_assemble_forest_f32's bit for bit, whatever weight is; on a
 * table where no live hypothesis ever lacks a candidate the ten shared outputs are pzn_assemble_beam_f32's bit for bit and
 * n_components is 1.  The same bits on every run.
 * 2 <= K <= 64, 1 <= B, C <= 8 (pzn_assemble_forest_beam_supported: 1 / 0; two generations of hypotheses are
 * 2 B (128 K + 16 + 4 (K - 1) + 4 + 2 K) bytes of LDS - poses, cost and placed set, edges, the two counts, a component byte and a
 * root byte per piece: 137472 of 163840 bytes at K = 64, B = 8), PZN_EUNSUPPORTED otherwise, before any launch; Z = 0 is a
 * success that launches nothing. */
int pzn_assemble_forest_beam_supported(int K, int B, int C);
int pzn_assemble_forest_beam_f32(const float* score, const float* T, const double* moment, const int32_t* count,
                                 int beam, int branch, double weight, double max_score, double vote_score,
                                 double joint_score, double restart_cost, int Z, int K,
                                 int32_t* root, int32_t* edges, float* edge_score, int32_t* n_edges,
                                 double* G, uint8_t* placed, int32_t* joints, int32_t* n_joints,
                                 int32_t* component, int32_t* roots, int32_t* n_components,
                                 double* cost, int32_t* n_hyp, pzn_stream_t stream);

/* One round of Z progressive walks (no counterpart in the reference; the choice and the ledger of assembly.ProgressiveAssembler
 * for Z puzzles in lockstep): one launch, one wavefront per puzzle, no workspace, no atomics, nothing waits for the device.
 * Slots are not compacted: puzzle z has P slots, a merged part stays in the fixed part's slot i and slot j dies, so a part in
 * slot s lives in original piece s's frame.  State of puzzle z, updated in place: alive[P] (bytes 0 / 1: the slot holds a part),
 * part[P] (int32: the slot of the part that holds original piece p), G[P,4,4] (float64: piece p into its part's frame), done
 * (byte), n_edges (int32), edges[P-1,4] (int32 rows (label_i, label_j, i, j), a part's label = its lowest member piece; unused
 * rows -1), edge_score[P-1] (fp32, the score as stored; unused rows +inf).  A fresh state: alive 1 (0 at or beyond a puzzle's
 * piece count), part[p] = p, G the identity, done 0, n_edges 0.
 * Key of entry (i, j) of score[z] ([P,P] fp32): its score; NaN, the diagonal and any pair with a dead end count as +inf.  Keys
 * compare as floats (-0 equals 0); of equal keys the lowest i P + j is the smaller.
 * Stop: done set, fewer than two slots alive, n_edges outside [0, P - 2], the smallest key not finite, or (double)key >
 * max_score (+inf: never; NaN is PZN_EINVAL): done = 1, took = 0, pick = (0, 0), and nothing else of the state changes.
 * Merge otherwise: for every p with part[p] == j, G[p] = T[z,i,j] G[p] (T fp32 widened to float64, an entry of the product is
 * ((a0 b0 + a1 b1) + a2 b2) + a3 b3 with every operation rounded on its own) and part[p] = i; alive[j] = 0; the row
 * (label_i, label_j, i, j) with the labels from before the merge and its score are appended; took = 1, pick = (i, j).
 * Out: took[Z] bytes, pick[Z,2] int64.  The same bits on every run.
 * 2 <= P <= 64 (pzn_progressive_round_supported: 1 / 0), PZN_EUNSUPPORTED otherwise, before any launch; Z = 0 is a success
 * that launches nothing. */
int pzn_progressive_round_supported(int P);
int pzn_progressive_round_f32(const float* score, const float* T, double max_score, int Z, int P,
                              uint8_t* alive, int32_t* part, double* G, uint8_t* done, int32_t* n_edges,
                              int32_t* edges, float* edge_score, uint8_t* took, int64_t* pick,
                              pzn_stream_t stream);

/* The pose graph of Z progressive walks, read off their ledgers (no counterpart in the reference; the step between
 * assembly.ProgressiveBatch and pzn_joint_refine_counts_f32; assembly.progressive_joints_rule is the numpy statement): one launch,
 * one workgroup per (round, puzzle), no workspace, no atomics, nothing waits for the device.
 * pieces[Z,P,N,3] fp32: the original pieces, each in its own frame.  G[Z,P,4,4] float64: the ledger's poses, piece p into the
 * frame of its part.  dropped[R,Z,2,k,2] int64: per round and puzzle the two lists of a merge, side 0 the fixed side and side 1
 * the moved side, k entries (piece, row) each in original pieces and rows.  least >= 1.
 * Per round r and puzzle z:
 * 1. An entry is valid iff 0 <= piece < P and 0 <= row < N; every other entry is skipped (the -1 rows of a puzzle that made no
 *    merge, -1 padding inside a list).  A round with a side that holds no valid entry yields nothing.
 * 2. The root-frame point of a valid entry, float64: the fp32 point widened, x' = ((g00 x + g01 y) + g02 z) + g03 with every
 *    product and sum rounded on its own, rows 1 and 2 likewise, g = G[z,piece].
 * 3. Every valid fixed entry takes its nearest valid moved entry and every valid moved entry its nearest valid fixed entry, by
 *    d2 = (dx dx + dy dy) + dz dz in float64, every operation rounded on its own; of equal distances the lowest position in the
 *    list.  (Coordinates are finite: a NaN distance is never the smaller one.)
 * 4. For a fixed piece p and a moved piece q != p: A(p,q) = the fixed entries on piece p whose nearest moved entry lies on q,
 *    B(p,q) = the moved entries on piece q whose nearest fixed entry lies on p, both in ascending list position.  Every valid
 *    entry is in at most one set, and the two sets of a joint face each other; they are chosen once, under G, and not trimmed.
 * 5. The joint (p, q) is emitted iff |A| >= least and |B| >= least, into row e = hi (hi - 1) / 2 + lo of the unordered pair
 *    (lo = min(p,q), hi = max(p,q)): J = P (P - 1) / 2 rows a puzzle.
 * A walk's own ledger puts every unordered pair of pieces on opposite sides in exactly one round, the one that merges their two
 * parts, so no row is written twice.  A caller's own `dropped` that breaks this is NOT checked: the numpy statement keeps the
 * later round, here the row's contents are then those of either round, element by element.
 * Out, all initialised by the caller (joints and rows_* to -1, the others to 0) and written only where a joint is emitted:
 * joints[Z,J,2] int32 rows (p, q), p the fixed piece; a[Z,J,k,3], b[Z,J,k,3] fp32, the points of A and B as read from pieces, in
 * their own piece's frame; rows_a[Z,J,k], rows_b[Z,J,k] int64, the row in the piece; na[Z,J], nb[Z,J] int32, |A| and |B|.  With
 * the sets of stride k and the counts na / nb this is the input of pzn_joint_refine_counts_f32.  The same bits on every run.
 * 2 <= P <= 64, 1 <= k <= 1024 (pzn_progressive_joints_supported: 1 / 0; 64 k bytes of LDS), R >= 1: PZN_EUNSUPPORTED otherwise,
 * before any launch; Z = 0 is a success that launches nothing. */
int pzn_progressive_joints_supported(int P, int k);
int pzn_progressive_joints_f32(const float* pieces, const double* G, const int64_t* dropped,
                               int R, int Z, int P, int N, int k, int least,
                               int32_t* joints, float* a, float* b, int32_t* na, int32_t* nb,
                               int64_t* rows_a, int64_t* rows_b, pzn_stream_t stream);

/* pointnet_util.py:118-119  dists.argsort()[:, :, :K] fused with the distance:
 * idx[B,S,K] = the K nearest points of xyz[B,N,3] to each new_xyz[B,S,3],
 * ascending by (distance, index) == a stable ascending sort.  K <= N. */
int pzn_knn_f32(const float* xyz, const float* new_xyz, int B, int N, int S,
                int K, int64_t* idx, pzn_stream_t stream);

/* pointnet_util.py:117-132 (knn=True, nsample = 32) in ONE launch and in the reference's layout: the
 * neighbour search of pzn_knn_f32 followed, per query and in the same wavefront, by the grouping of
 * pzn_group_fwd_f32: idx[B,S,32] and out[B,S,32,3+D] = cat(xyz[idx] - new_xyz, feat[idx]); grouped_xyz
 * [B,S,32,3] is written when non-NULL (returnfps=True).  64 <= N <= 8192, D > 0, D % 4 == 0, feat and out
 * 16-byte aligned; PZN_EUNSUPPORTED otherwise (compose the two single entry points then). */
int pzn_knn_group_f32(const float* xyz, const float* feat, const float* new_xyz, int B, int N,
                      int S, int D, int64_t* idx, float* out, float* grouped_xyz,
                      pzn_stream_t stream);

/* pointnet_util.py:76-96  query_ball_point(radius, nsample, xyz, new_xyz):
 * first `nsample` indices (ascending) with d <= radius^2, slots beyond the hit
 * count are filled with the first hit; a row with no hit is filled with N
 * (what the reference's sort/pad produces). radius2 = (float)(radius*radius). */
int pzn_ball_query_f32(float radius2, int nsample, const float* xyz,
                       const float* new_xyz, int B, int N, int S, int64_t* idx,
                       pzn_stream_t stream);

/* pointnet_util.py:39-50  index_points(points[B,N,C], idx[B,M]) -> [B,M,C]
 * (M = S or S*K; the rank-3 form is the same gather on a flattened idx). */
int pzn_gather_fwd_f32(const float* points, const int64_t* idx, int B, int N,
                       int M, int C, float* out, pzn_stream_t stream);
/* autograd of the gather: grad_points[B,N,C] += scatter(grad_out[B,M,C]).
 * grad_points must be zero-initialised by the caller. */
int pzn_gather_bwd_f32(const float* grad_out, const int64_t* idx, int B, int N,
                       int M, int C, float* grad_points, pzn_stream_t stream);

/* pointnet_util.py:123-132  the grouping tail of sample_and_group:
 * out[B,S,K,3+D] = cat(xyz[idx] - new_xyz[:, :, None], feat[idx]).
 * feat may be NULL with D = 0 (points=None, pointnet_util.py:131-132).
 * grouped_xyz[B,S,K,3] (un-normalised, returnfps=True) is written when
 * non-NULL. */
int pzn_group_fwd_f32(const float* xyz, const float* feat, const float* new_xyz,
                      const int64_t* idx, int B, int N, int S, int K, int D,
                      float* out, float* grouped_xyz, pzn_stream_t stream);
/* Backward of the above.  Any of the three gradient outputs may be NULL.
 * grad_xyz[B,N,3] and grad_feat[B,N,D] must be zero-initialised;
 * grad_new_xyz[B,S,3] is overwritten (= -sum_k grad_out[...,0:3]). */
int pzn_group_bwd_f32(const float* grad_out, const int64_t* idx, int B, int N,
                      int S, int K, int D, float* grad_xyz, float* grad_feat,
                      float* grad_new_xyz, pzn_stream_t stream);

/* ------------------------------------------------------------------------ */
/* Earth Mover's Distance: PyTorchEMD/cuda/emd.cpp:23-27, emd_kernel.cu     */
/* ------------------------------------------------------------------------ */

/* Bytes of scratch the EMD entry points need for (B,n,m). */
size_t pzn_emd_workspace_bytes(int B, int n, int m);

/* emd_kernel.cu:171-193  ApproxMatchForward(xyz1[B,n,3], xyz2[B,m,3])
 *   -> match[B,m,n]   (kernel emd_kernel.cu:25-158).  */
int pzn_emd_approxmatch_f32(const float* xyz1, const float* xyz2, int B, int n,
                            int m, float* match, void* workspace,
                            pzn_stream_t stream);
/* emd_kernel.cu:257-279  MatchCostForward -> cost[B] (kernel :200-243). */
int pzn_emd_matchcost_f32(const float* xyz1, const float* xyz2,
                          const float* match, int B, int n, int m, float* cost,
                          pzn_stream_t stream);
/* emd_kernel.cu:373-398  MatchCostBackward -> grad1[B,n,3], grad2[B,m,3]
 * (kernels :333-355 and :286-327). */
int pzn_emd_matchcost_grad_f32(const float* grad_cost, const float* xyz1,
                               const float* xyz2, const float* match, int B,
                               int n, int m, float* grad1, float* grad2,
                               pzn_stream_t stream);
/* Fused replacement of the three calls above for PyTorchEMD/emd.py:5-21:
 * runs the 10-level auction and accumulates cost[B] and the UNSCALED
 * gradients g1[B,n,3] = d cost/d xyz1, g2[B,m,3] = d cost/d xyz2 on the fly,
 * so match[B,m,n] is never written to HBM.  backward = grad_cost[b] * g{1,2}. */
int pzn_emd_fused_f32(const float* xyz1, const float* xyz2, int B, int n, int m,
                      float* cost, float* g1, float* g2, void* workspace,
                      pzn_stream_t stream);
/* 1..4 SMALL calls of the function above (n, m <= 256 each: model5_b.py:1012 and :1123-1125, the three small terms of the loss) as
 * ONE launch of single-workgroup auctions; HOST arrays of device pointers / sizes, one entry per call; results bit-identical to
 * the separate calls.  PZN_EUNSUPPORTED when one of them is larger. */
int pzn_emd_fused_small_multi_f32(int count, const float* const* xyz1, const float* const* xyz2,
                                  const int* B, const int* n, const int* m, float* const* cost,
                                  float* const* g1, float* const* g2, pzn_stream_t stream);

/* The double instantiation of the three calls (emd_kernel.cu:187, :273, :391 dispatch on the floating type;
 * csrc/emd64.hip): same layouts in double, workspace of pzn_emd_workspace_bytes_f64(B,n,m) bytes.  model5_b never
 * calls EMD in double; PyTorchEMD.emd.earth_mover_distance routes double clouds here. */
size_t pzn_emd_workspace_bytes_f64(int B, int n, int m);
int pzn_emd_approxmatch_f64(const double* xyz1, const double* xyz2, int B, int n, int m, double* match,
                            void* workspace, pzn_stream_t stream);
int pzn_emd_matchcost_f64(const double* xyz1, const double* xyz2, const double* match, int B, int n, int m,
                          double* cost, pzn_stream_t stream);
int pzn_emd_matchcost_grad_f64(const double* grad_cost, const double* xyz1, const double* xyz2, const double* match,
                               int B, int n, int m, double* grad1, double* grad2, pzn_stream_t stream);

/* Measurement aid (bench.py's EMD roofline): byte offset inside the workspace of pzn_emd_walk_counter_count() uint64
 * counters the fused entry point leaves behind; their sum x 64 = (row, point) evaluations executed (points of exhausted mass
 * and points outside a level's x window are not walked); counters (16 i + s) * 16, s = 0..15, belong to launch i of the call
 * (0 = first pass A, 1 + 2 k = pass B and 2 + 2 k = pass C of the k-th level); (size_t)-1 on the single-workgroup path
 * (n, m <= 256: 30 n m). */
size_t pzn_emd_walk_counter_offset(int B, int n, int m);
int pzn_emd_walk_counter_count(void);

/* ------------------------------------------------------------------------ */
/* Loss tail: model5_b.py:1495-1505 chamfer_loss                            */
/* ------------------------------------------------------------------------ */

size_t pzn_chamfer_workspace_bytes(int B, int n, int m);
/* chamfer_loss(a[B,n,3], b[B,m,3]) -> (torch.min(P,1): min over a for each b
 * point [B,m],  torch.min(P,2): min over b for each a point [B,n]) with the
 * reference's expansion P = |a|^2 + |b|^2 - 2 a.b, never materialising
 * P[B,n,m].  arg-min indices (int32) are written for the backward. */
int pzn_chamfer_fwd_f32(const float* a, const float* b, int B, int n, int m,
                        float* min_over_a, int32_t* arg_over_a,
                        float* min_over_b, int32_t* arg_over_b, void* workspace,
                        pzn_stream_t stream);
/* grad_a[B,n,3], grad_b[B,m,3] (zero-initialised by the caller) from the
 * upstream gradients g_over_a[B,m], g_over_b[B,n] (either may be NULL). */
int pzn_chamfer_bwd_f32(const float* a, const float* b, int B, int n, int m,
                        const float* g_over_a, const int32_t* arg_over_a,
                        const float* g_over_b, const int32_t* arg_over_b,
                        float* grad_a, float* grad_b, pzn_stream_t stream);

/* ------------------------------------------------------------------------ */
/* Dense path on the matrix cores (fp32 results; default operand path = bf16x3 */
/* split precision, exact-fp32 MFMA on request: pzn_gemm_set_precision)       */
/* ------------------------------------------------------------------------ */

/* nn.Linear as used throughout model5_b.py (e.g. :417-422, :559-599):
 * y[M,Nout] = act(x[M,Kin] W[Nout,Kin]^T + bias[Nout]); act = ReLU if relu.
 * bias may be NULL. */
int pzn_linear_fwd_f32(const float* x, const float* W, const float* bias, int M,
                       int Kin, int Nout, int relu, float* y,
                       pzn_stream_t stream);
/* Same product with the epilogue of model5_b.py:453-454 / :460-461: ReLU then
 * max over each group of 32 consecutive rows (the K=32 neighbours of one
 * centroid): out[R,Nout], argmax[R,Nout] (row 0..31 of the maximum). */
int pzn_linear_maxpool_fwd_f32(const float* x, const float* W, const float* bias,
                               int R, int Kin, int Nout, float* out,
                               int32_t* argmax, pzn_stream_t stream);
/* dx[M,Kin] = (dy * [y_relu > 0]) W, then * [x_relu > 0].  y_relu / x_relu are
 * the forward outputs of this / the previous layer when they ended in a ReLU,
 * NULL otherwise. */
int pzn_linear_dgrad_f32(const float* dy, const float* y_relu, const float* W,
                         int M, int Kin, int Nout, const float* x_relu,
                         float* dx, pzn_stream_t stream);
/* dW[Nout,Kin] = (dy * [y_relu > 0])^T x,  db[Nout] = its column sums (db may
 * be NULL).  Split over the row range, accumulated with fp32 atomics: results are
 * reproducible to rounding, not bitwise.  accumulate == 0: both outputs are overwritten;
 * accumulate != 0: added to (e.g. directly into a zeroed flat gradient bucket, which
 * saves the zero-fill launches and autograd's separate "grad += dW" pass). */
int pzn_linear_wgrad_f32(const float* dy, const float* y_relu, const float* x,
                         int M, int Kin, int Nout, float* dW, float* db,
                         int accumulate, pzn_stream_t stream);
/* The three products of nn.Linear on a COLUMN SLICE of a wider weight matrix: W points at column k0 of
 * W_full[Nout, ldw] and is Kin columns wide.  cat(x_1 .. x_n) W_full^T (model5_b.py:466-474) then is sum_i x_i W_i^T + b
 * without the concatenation ever being built, and a weight gradient can be added straight into a slice of a parameter.
 *   fwd:   y[M,Nout] = x[M,Kin] W^T + bias   (accumulate == 0)   or   y += x W^T   (accumulate != 0, bias ignored)
 *   dgrad: dx[M,Kin] = dy[M,Nout] W (+ addend[M,Kin] when non-NULL)
 *   wgrad: dW[Nout, ldw-strided, Kin columns] += dy^T x,  db[Nout] += column sums of dy (db may be NULL) */
int pzn_linear_slice_fwd_f32(const float* x, const float* W, int ldw, const float* bias, int M, int Kin,
                             int Nout, int accumulate, float* y, pzn_stream_t stream);
int pzn_linear_slice_dgrad_f32(const float* dy, const float* W, int ldw, int M, int Kin, int Nout,
                               const float* addend, float* dx, pzn_stream_t stream);
int pzn_linear_slice_wgrad_f32(const float* dy, const float* x, int M, int Kin, int Nout, float* dW, int ldw,
                               float* db, pzn_stream_t stream);
/* Backward through the max-pool epilogue: the [R*32,Nout] gradient
 * dy[g*32+k, c] = (argmax[g,c]==k && out[g,c]>0) ? dout[g,c] : 0 is generated
 * inside the operand loader, never materialised. */
int pzn_linear_maxpool_dgrad_f32(const float* dout, const int32_t* argmax,
                                 const float* out, const float* W, int R, int Kin,
                                 int Nout, const float* x_relu, float* dx,
                                 pzn_stream_t stream);
int pzn_linear_maxpool_wgrad_f32(const float* dout, const int32_t* argmax,
                                 const float* out, const float* x, int R, int Kin,
                                 int Nout, float* dW, float* db, int accumulate,
                                 pzn_stream_t stream);
/* A chain of L nn.Linear layers (each + ReLU where relu[i] != 0) on FEW rows, one launch per layer each way and one small
 * reduce launch at the end (csrc/fewrows.hip): the pose head, model5_b.py:559-569 on cat([ffpc, fmrpc]).
 *   widths[L + 1] = input width, then every layer's output width; W[i] = [widths[i + 1], widths[i]] dense, bias[i] or NULL.
 *   The input rows are x0[M, k0] and, when k1 > 0, x1[M, k1] beside them (k0 + k1 = widths[0]): the concatenation is
 *   never built.  y[i] = [M, widths[i + 1]], i < L: every layer's output, the last one the result (the backward reads all).
 *   bwd: dy[M, widths[L]] -> dx0[M, k0], dx1[M, k1] (both NULL: no input gradient), dW[i] / db[i] (dW[i] NULL: none for
 *   layer i; db[i] may be NULL), overwritten, or added to where accumulate[i] != 0.
 * No atomics: a layer's workgroups store partial sums over chunks of the reduction range, the next launch adds them in a
 * fixed order while it loads its operand; results are bit-identical from run to run.
 * widths, W, bias, relu, y, dW, db, accumulate are HOST arrays.  workspace: pzn_fewrow_chain_workspace_bytes bytes.
 * Limits: 1 <= M <= 128, 1 <= L <= 16, widths[0] >= 256, inner widths > 64, split-precision modes only
 * (pzn_fewrow_chain_supported: 1 / 0), every device pointer 16-byte aligned: PZN_EUNSUPPORTED otherwise, before any
 * launch (compose pzn_linear_* then). */
int pzn_fewrow_chain_supported(int M, int L, const int* widths);
size_t pzn_fewrow_chain_workspace_bytes(int M, int L, const int* widths);
int pzn_fewrow_chain_fwd_f32(const float* x0, int k0, const float* x1, int k1, int M, int L, const int* widths,
                             const float* const* W, const float* const* bias, const int* relu, float* const* y,
                             void* workspace, size_t workspace_bytes, pzn_stream_t stream);
int pzn_fewrow_chain_bwd_f32(const float* dy, const float* x0, int k0, const float* x1, int k1, int M, int L,
                             const int* widths, const float* const* W, const int* relu, const float* const* y,
                             float* dx0, float* dx1, float* const* dW, float* const* db, const int* accumulate,
                             void* workspace, size_t workspace_bytes, pzn_stream_t stream);
/* Matrix-core path of every dense entry point below: 0 = exact fp32 (v_mfma_f32_32x32x2_f32),
 * 1 = bf16x3 split precision (x = x1+x2+x3 in bf16, six v_mfma_f32_32x32x16_bf16 products,
 * fp32 accumulate: fp32-GEMM accuracy at up to 2.67x the matrix-pipe rate), 2 = auto (default;
 * currently bf16x3 for every product).
 * Process-wide; also PZN_GEMM_PRECISION=f32|x3|auto in the environment. */
int pzn_gemm_set_precision(int mode);
int pzn_gemm_get_precision(void);
/* Precision of the attention contractions (model5_b.py:67-75: q k^T, attn v, and their four backward products) inside
 * pzn_attn_* / pzn_attn_block_*: 0 (default) = the matrix-core path selected above (fp32 results), 1 = operands rounded
 * to bf16 once and ONE v_mfma_f32_32x32x16_bf16 per product, fp32 accumulation, fp32 softmax (BASELINE configs[4] "bf16
 * attn with MFMA").  The q / k / v / out projections keep the fp32-accurate path.  Also PZN_ATTN_PRECISION=bf16. */
int pzn_attn_set_precision(int mode);
int pzn_attn_get_precision(void);

/* Shared MLP + max over the K=32 neighbours, model5_b.py:452-454 / :459-461:
 *   h = relu(x[R*32,C0] W1^T + b1)  (kept: the backward reads it);
 *   out[R,C2] = max_k relu(h W2^T + b2),  argmax[R,C2]. */
int pzn_sharedmlp_max_fwd_f32(const float* x, const float* W1, const float* b1,
                              const float* W2, const float* b2, int R, int C0,
                              int C1, int C2, float* h, float* out,
                              int32_t* argmax, pzn_stream_t stream);
/* dh_ws: [R*32,C1] scratch.  dx[R*32,C0] may be NULL.  dW1,db1,dW2,db2 are
 * overwritten. */
int pzn_sharedmlp_max_bwd_f32(const float* x, const float* W1, const float* W2,
                              const float* h, const float* out,
                              const int32_t* argmax, const float* dout, int R,
                              int C0, int C1, int C2, float* dh_ws, float* dx,
                              float* dW1, float* db1, float* dW2, float* db2,
                              int accumulate, pzn_stream_t stream);

/* The same set-abstraction level with its first layer computed PER POINT (csrc/sapoint.hip): a grouped row is
 * {xyz[j] - centre, feat[j]} (pointnet_util.py:123-132), so its product with W1[C1,3+D] (model5_b.py:452 / :459)
 * is a per-point term plus a per-group term (below); the grouped tensor is never materialised.
 *   pzn_knn_inverse_lists: the B*S*K (row, point) pairs of idx sorted by point, per cloud: rows[B, S*K] = in-cloud
 *         row numbers (s*K + k), ascending within a point, pts[B, S*K] = the point each gathered (may be NULL),
 *         off[B, N+1] = where every point's rows start (index_points backward without atomics on rows). */
int pzn_knn_inverse_lists(const int64_t* idx, int B, int N, int S, int K, int32_t* off,
                          int32_t* rows, int32_t* pts, pzn_stream_t stream);

/* The same level with the first layer's rows NEVER in memory (what model5_b's encoder runs by default).  The coordinate
 * term is split:  W1[:,0:3] (xyz[j] - centre) = W1[:,0:3] xyz[j] - W1[:,0:3] centre,  so with
 *   Pp[B*N, C1] = feat W1[:,3:]^T + W1[:,0:3] xyz      (pzn_linear_fwd_f32, then pzn_sa_prep_f32 adds the xyz term in place)
 *   Q [B*S, C1] = b1 - W1[:,0:3] new_xyz                (pzn_sa_prep_f32)
 * a grouped row of the first layer is relu(Pp[idx] + Q[group]) — generated inside the operand loader of the
 * weight-stationary matrix-core kernel (fwd) and inside the backward passes; same result as the grouped-row form above up to
 * the order of the fp32 sum.  K = 32, C1 % 128 == 0 backward (C1 % 32 == 0 forward), C2 in {64,128,256}.
 *   fwd:  out[B*S, C2] = max_k relu(relu(Pp[idx[.,k]] + Q) W2^T + b2), argmax[B*S, C2]
 *   bwd:  pzn_sa_level_bwd_pt_f32 below (the rows' gradient dh[B*S*32, C1] is summed per point where it is computed and
 *         never written; rounds 2-4 wrote it: pzn_sa_level_bwd_f32 + pzn_sa_point_l1_bwd_f32, removed in round 6). */
int pzn_sa_prep_f32(const float* xyz, const float* new_xyz, const float* W1, const float* b1, int B, int N, int S,
                    int D, int C1, float* P, float* Q, pzn_stream_t stream);
int pzn_sa_level_fwd_f32(const float* Pp, const float* Q, const int64_t* idx, const float* W2, const float* b2,
                         int B, int N, int S, int C1, int C2, float* out, int32_t* argmax, pzn_stream_t stream);
/* same, with a caller-owned 16-byte aligned workspace of pzn_sa_level_fwd_workspace_bytes(C1, C2) bytes (0 = no streamed
 * form for this shape; workspace may then be NULL): C1 = C2 in {128, 256} run the streamed-weights kernel, which
 * generates each grouped row once and streams the split planes of W2 through LDS; identical results (same products,
 * same tie rule of the arg-max). */
size_t pzn_sa_level_fwd_workspace_bytes(int C1, int C2);
int pzn_sa_level_fwd_ws_f32(const float* Pp, const float* Q, const int64_t* idx, const float* W2, const float* b2,
                            int B, int N, int S, int C1, int C2, float* out, int32_t* argmax, void* workspace,
                            pzn_stream_t stream);
/* The same in two launches that a caller times (or schedules) separately, as pzn_attn_fused_prep_weights is for the
 * attention blocks: the split of W2 into the streamed kernel's plane image (workspace of
 * pzn_sa_level_fwd_workspace_bytes() bytes), and the level on a workspace that holds it.  PZN_EUNSUPPORTED where the
 * shape has no streamed form (pzn_sa_level_fwd_ws_f32 serves every shape). */
int pzn_sa_level_prep_weights_f32(const float* W2, int C1, int C2, void* workspace, pzn_stream_t stream);
int pzn_sa_level_fwd_packed_f32(const float* Pp, const float* Q, const int64_t* idx, const float* b2, int B, int N,
                                int S, int C1, int C2, float* out, int32_t* argmax, const void* workspace,
                                pzn_stream_t stream);

/* The level's backward BY POINT (csrc/sapool.hip): dW2[C2,C1] / db2[C2] (overwritten, or added to when accumulate), the
 * per-point sums dP[B*N, C1] of the rows' gradient dh (overwritten), dW1[:, 0:3] += dh^T (xyz[idx] - centre) and db1 += column
 * sums of dh (both ADDED to, db1 may be NULL).  dh itself is computed by point (hit lists per group, sorted by arg-max row;
 * W2 slice in LDS; gate from Pp and Q) and never written.  off / rows / pts: pzn_knn_inverse_lists of idx.  A wavefront owns
 * whole points: every row of dP is written exactly once by plain stores and the rows of a point are summed in ascending row
 * order, so dP is the same bit for bit in every run.  workspace: pzn_sa_level_bwd_pt_workspace_bytes(B, S, C2) bytes,
 * 16-byte aligned.  PZN_EUNSUPPORTED for C1 % 128 != 0 or C2 not in {64, 128, 256}. */
size_t pzn_sa_level_bwd_pt_workspace_bytes(int B, int S, int C2);
/* The weight-gradient pass of pzn_sa_level_bwd_pt_f32 on its own (csrc/poolbwd.hip): dW2[C2, C1] += the sparse dy^T h,
 * db2[C2] += its column sums (both ADDED to), with the workgroups' partial tiles summed in a fixed order.  The rows are
 * h[G*32, C1] (Pp, Q, idx NULL), or h == NULL and they are regenerated as relu(Pp[(g / S) * N + idx[g*32+k], :] + Q[g, :]).
 * workspace: pzn_pool_wgrad_workspace_bytes(G, C1, C2) bytes, 16-byte aligned.  PZN_EUNSUPPORTED for C1 % 128 != 0 or C2 not
 * in {64, 128, 256}. */
size_t pzn_pool_wgrad_workspace_bytes(int G, int C1, int C2);
int pzn_pool_wgrad_f32(const float* dout, const int32_t* argmax, const float* out, const float* h, const float* Pp,
                       const float* Q, const int64_t* idx, int N, int S, int G, int C1, int C2, float* dW2, float* db2,
                       void* workspace, pzn_stream_t stream);
int pzn_sa_level_bwd_pt_f32(const float* dout, const int32_t* argmax, const float* out, const float* W2,
                            const float* Pp, const float* Q, const int64_t* idx, const float* xyz, const float* new_xyz,
                            const int32_t* off, const int32_t* rows, const int32_t* pts, int B, int N, int S, int D, int C1,
                            int C2, float* dP, float* dW2, float* db2, float* dW1, float* db1, int accumulate, void* workspace,
                            pzn_stream_t stream);

/* One set-abstraction level of the encoder behind one entry point each way (csrc/sachain.hip): the sequences
 *   fwd:  P' = feat W1[:,3:]^T (pzn_linear_fwd_f32) -> neighbour search when idx == NULL (pzn_knn_f32) -> pzn_sa_prep_f32 ->
 *         pzn_sa_level_prep_weights_f32 -> pzn_sa_level_fwd_packed_f32
 *   bwd:  pzn_knn_inverse_lists -> pzn_sa_level_bwd_pt_f32 -> dfeat = dP W1[:,3:] (pzn_linear_dgrad_f32) ->
 *         dW1[:,3:] += dP^T feat (pzn_linear_slice_wgrad_f32)
 * enqueued by the library on one caller-owned buffer per direction (same kernels, order and operands as the caller-composed
 * form: 2 calls and 2 allocations per level instead of 9 and ~13).  xyz[B,N,3], feat[B,N,D], new_xyz[B,S,3], idx[B,S,32] or NULL,
 * W1[C1,3+D], b1[C1], W2[C2,C1], b2[C2]; out[B*S,C2], argmax[B*S,C2]; saved / scratch: pzn_sa_level_chain_saved_bytes /
 * _scratch_bytes, 256-byte aligned; the backward gets the idx the forward got (NULL: the searched indices live in `saved`).
 * accumulate != 0: the four parameter gradients are ADDED to; 0: overwritten.  dfeat[B,N,D] overwritten, may be NULL.
 * C1 % 128 == 0, C2 in {64,128,256}: PZN_EUNSUPPORTED otherwise, before anything is launched. */
size_t pzn_sa_level_chain_saved_bytes(int B, int N, int S, int D, int C1, int C2);
size_t pzn_sa_level_chain_scratch_bytes(int B, int N, int S, int C1, int C2);
int pzn_sa_level_chain_fwd_f32(const float* xyz, const float* feat, const float* new_xyz, const int64_t* idx,
                               const float* W1, const float* b1, const float* W2, const float* b2, int B, int N, int S,
                               int D, int C1, int C2, float* out, int32_t* argmax, void* saved, pzn_stream_t stream);
int pzn_sa_level_chain_bwd_f32(const float* dout, const int32_t* argmax, const float* out, const float* xyz,
                               const float* feat, const float* new_xyz, const int64_t* idx, const float* W1,
                               const float* W2, const void* saved, int B, int N, int S, int D, int C1, int C2,
                               float* dfeat, float* dW1, float* db1, float* dW2, float* db2, int accumulate,
                               void* scratch, pzn_stream_t stream);

/* The per-point stem of the encoder in one launch each way (csrc/stem.hip, model5_b.py:447-448):
 *   out = relu(bn2(mlp2(relu(bn1(mlp1(xyz))))))   xyz[B,N,3], mlp1 = (W1[64,3], b1[64]), mlp2 = (W2[64,64], b2[64]),
 * bn1 / bn2 = BatchNorm1d(N) over the POINT axis of [B,N,64] (weight / bias / running buffers [N]; any may be NULL as the module
 * has them; training != 0: batch statistics, running buffers updated in place as torch does).  out[B,N,64]; mean1 / invstd1 /
 * mean2 / invstd2 [N] (written) feed the backward, which recomputes every activation from xyz.  bwd: dW1[64,3], db1[64],
 * dW2[64,64], db2[64] and the BatchNorm weight / bias gradients [N] (these may be NULL) are ADDED to; no gradient for xyz;
 * workspace = pzn_stem_bwd_workspace_bytes(N) bytes, 16-byte aligned, need not be cleared (the workgroups' partial sums);
 * dout2 (may be NULL): a second gradient of the same output, added to dout while loading (two consumers of the features).
 * PZN_EUNSUPPORTED for B > 64 or W2 not 16-byte aligned (compose pzn_linear_* + pzn_bn_points_relu_* then). */
int pzn_stem_fwd_f32(const float* xyz, const float* W1, const float* b1, const float* bn1_weight, const float* bn1_bias,
                     float* bn1_running_mean, float* bn1_running_var, float bn1_momentum, float bn1_eps, const float* W2,
                     const float* b2, const float* bn2_weight, const float* bn2_bias, float* bn2_running_mean,
                     float* bn2_running_var, float bn2_momentum, float bn2_eps, int training, int B, int N, float* out,
                     float* mean1, float* invstd1, float* mean2, float* invstd2, pzn_stream_t stream);
size_t pzn_stem_bwd_workspace_bytes(int N);
int pzn_stem_bwd_f32(const float* xyz, const float* dout, const float* dout2, const float* W1, const float* b1, const float* W2, const float* b2,
                     const float* bn1_weight, const float* bn1_bias, const float* bn2_weight, const float* bn2_bias,
                     const float* mean1, const float* invstd1, const float* mean2, const float* invstd2, int training, int B,
                     int N, float* dW1, float* db1, float* dW2, float* db2, float* dbn1_weight, float* dbn1_bias,
                     float* dbn2_weight, float* dbn2_bias, void* workspace, pzn_stream_t stream);

/* relu(BatchNorm1d(num_points)(x)) of the per-point feature MLP (model5_b.py:424, :447-448): x[B,N,C], the BN
 * "channel" axis is the POINT index, statistics over the B*C values of a point.  training != 0: batch statistics
 * (biased variance), running_mean / running_var updated in place as torch does (momentum, unbiased variance; may be
 * NULL); else the running statistics normalise.  save_mean / save_invstd [N] feed the backward.
 * bwd: dx[B,N,C] (may be NULL), dweight[N] / dbias[N] ADDED to (may be NULL); the ReLU gate is recomputed from x. */
int pzn_bn_points_relu_fwd_f32(const float* x, const float* weight, const float* bias,
                               float* running_mean, float* running_var, int training,
                               float momentum, float eps, int B, int N, int C, float* y,
                               float* save_mean, float* save_invstd, pzn_stream_t stream);
int pzn_bn_points_relu_bwd_f32(const float* x, const float* dy, const float* weight,
                               const float* bias, const float* save_mean,
                               const float* save_invstd, int training, int B, int N, int C,
                               float* dx, float* dweight, float* dbias, pzn_stream_t stream);

/* scaled_dot_production of layerAttention, model5_b.py:67-75:
 * attn[B,L,L] = softmax(q[B,L,dk] k[B,L,dk]^T / sqrt(dk)), out[B,L,dv] = attn v.
 * attn is an output because the reference returns it (model5_b.py:97,101). */
int pzn_attn_fwd_f32(const float* q, const float* k, const float* v, int B,
                     int L, int dk, int dv, float* attn, float* out,
                     pzn_stream_t stream);
size_t pzn_attn_bwd_workspace_bytes(int B, int L, int dk, int dv);
/* dq, dk_out, dv_out from d_out[B,L,dv] and d_attn[B,L,L] (may be NULL). */
int pzn_attn_bwd_f32(const float* q, const float* k, const float* v,
                     const float* attn, const float* d_out, const float* d_attn,
                     int B, int L, int dk, int dv, float* dq, float* dk_out,
                     float* dv_out, void* workspace, pzn_stream_t stream);

/* layerAttention as one unit (model5_b.py:83-101): q,k,v = Linear(x[B*L,E]); attn = softmax(q k^T /
 * sqrt(dk)); r = x - attn v; yo = relu(r Wo^T + bo); out = x + yo.  q[B*L,dk], k, v[B*L,E], attn
 * [B,L,L], r, yo are outputs the backward needs (attn is also the block's second result).  The
 * backward takes dout (and d_attn or NULL), returns dx and the eight parameter gradients
 * (overwritten, or added to when accumulate != 0).  Returns PZN_EUNSUPPORTED for shapes the
 * weight-stationary kernel does not take: compose the block from the single entry points then. */
int pzn_attn_block_fwd_f32(const float* x, const float* Wq, const float* bq, const float* Wk,
                           const float* bk, const float* Wv, const float* bv, const float* Wo,
                           const float* bo, int B, int L, int E, int dk, float* q, float* k,
                           float* v, float* attn, float* r, float* yo, float* out,
                           pzn_stream_t stream);
size_t pzn_attn_block_bwd_workspace_bytes(int B, int L, int E, int dk);
int pzn_attn_block_bwd_f32(const float* x, const float* Wq, const float* Wk, const float* Wv,
                           const float* Wo, const float* q, const float* k, const float* v,
                           const float* attn, const float* r, const float* yo, const float* dout,
                           const float* d_attn, int B, int L, int E, int dk, void* workspace,
                           float* dx, float* dWq, float* dbq, float* dWk, float* dbk, float* dWv,
                           float* dbv, float* dWo, float* dbo, int accumulate,
                           pzn_stream_t stream);

/* layerAttention (model5_b.py:67-75, 83-101) as CHAINED matrix-core kernels (csrc/attnfused.hip) for the model's shape
 * L = 256 points, E = 256 channels, dk = 64 (pzn_attn_fused_supported).  The point sits on the MFMA lane, so every
 * product's accumulator is the next product's operand in registers: no score matrix and no q / k / v tensors in
 * memory.  Shared operands live as bf16x3 "plane images" in MFMA-fragment order, written by their producer:
 *   weights:  pzn_attn_fused_prep_weights -> one buffer of pzn_attn_fused_weight_bytes() per block;
 *   q, k, v:  pzn_attn_fused_proj -> three images per problem (q, k: *_qk_image_bytes(B); v: *_v_image_bytes(B)); one
 *             image serves the products that sum over its columns (plain slabs) and those that sum over its rows
 *             (the same bytes fetched in a transposed-read cut by the LDS-DMA: no second copy since round 4).
 * Every entry point takes nprob = 1 or 2 independent problems as arrays of nprob pointers (the two encoders of
 * predict5, model5_b.py:700-707, in one launch); B clouds each; all buffers 16-byte aligned.
 *   fwd:    r = x + relu(Wo (x - softmax(q k^T / 8) v) + bo) [B*L,E];  t = x - attn v [B*L,E];  mask [B*L,8] u32 = gate
 *           bits of the ReLU;  lse [B*L];  map[i] (may be NULL): map_mode 0: [B,L,L] = scale P; 1: += scale P (the mean of the
 *           four blocks' maps, model5_b.py:468-469); 2 / 3: the same for [B,L/16,L] = the column sums of P over each strip
 *           of 16 query rows - all that a consumer of the map's mean over its rows needs (model5_b.py:937-942: 1/16 of the
 *           bytes, no [B,L,L] tensor).
 *   bwd_q:  query side of the backward from dr (+ dr2 when non-NULL: rows of ld_dr / ld_dr2 floats, so a column slice of
 *           a wider gradient needs no copy and the sum of two gradients no add): dz = dr . gate, dq [B*L,dk], delta [B*L],
 *           the image of da = -dz Wo, and for bwd_k only: u = dr + dz Wo [B*L,E] and dq_tiles [B*L,dk] in the kernels'
 *           own register-tile order (same sizes as the row tensors; not meant to be read by anything else).
 *   bwd_k:  key side (u, dq = the two tile tensors of bwd_q): dk [B*L,dk], dv [B*L,E],
 *           dx = u + dq Wq + dk Wk + dv Wv [B*L,E] = the block's input gradient.
 *   wgrads: the eight parameter gradients from dz, t, dq, dk, dv and the block input x (one problem per call). */
int pzn_attn_fused_supported(int L, int E, int dk);
size_t pzn_attn_fused_weight_bytes(void);
size_t pzn_attn_fused_qk_image_bytes(int B);
size_t pzn_attn_fused_v_image_bytes(int B);
int pzn_attn_fused_prep_weights(const float* Wq, const float* Wk, const float* Wv, const float* Wo,
                                void* planes, pzn_stream_t stream);
/* the same for n <= 4 blocks in one launch (an encoder's four layers): arrays of n pointers */
int pzn_attn_fused_prep_weights_n(int n, const float* const* Wq, const float* const* Wk,
                                  const float* const* Wv, const float* const* Wo,
                                  void* const* planes, pzn_stream_t stream);
int pzn_attn_fused_proj(int nprob, const float* const* x, const void* const* w,
                        const float* const* bq, const float* const* bk, const float* const* bv, int B,
                        void* const* qrp, void* const* krp, void* const* vrp, pzn_stream_t stream);
int pzn_attn_fused_fwd(int nprob, const float* const* x, const void* const* qrp,
                       const void* const* krp, const void* const* vrp, const void* const* w,
                       const float* const* bo, int B, float* const* r, float* const* t,
                       void* const* mask, float* const* map, float* const* lse, int map_mode,
                       float map_scale, pzn_stream_t stream);
int pzn_attn_fused_bwd_q(int nprob, const float* const* dr, int ld_dr, const float* const* dr2,
                         int ld_dr2, const void* const* mask,
                         const void* const* qrp, const void* const* krp, const void* const* vrp,
                         const void* const* w, int B, float* const* dz, float* const* u,
                         float* const* dq, float* const* dq_tiles, void* const* darp,
                         float* const* delta, pzn_stream_t stream);
int pzn_attn_fused_bwd_k(int nprob, const void* const* qrp, const void* const* krp,
                         const void* const* vrp, const void* const* darp, const void* const* w,
                         const float* const* lse, const float* const* delta, const float* const* u,
                         const float* const* dq, int B, float* const* dk, float* const* dv,
                         float* const* dx, pzn_stream_t stream);
/* The four weight gradients and four bias gradients of one block from what the chained kernels leave in memory: dWo (+)= dz^T t,
 * dWq/k/v (+)= dq/dk/dv^T x, the biases' = column sums (accumulate == 0: overwritten).  E = 256, dk = 64, M % 64 == 0: one launch
 * of LDS-shared 128 x 128 tiles over 24 row ranges (csrc/attnwgrad.hip), which meet in fp32 atomics here and in a fixed-order sum
 * inside pzn_attn_chain_bwd_f32 (its scratch holds their partial tiles); other shapes: the general weight-gradient kernels. */
int pzn_attn_fused_wgrads(const float* dz, const float* t, const float* dq, const float* dk,
                          const float* dv, const float* x, int M, int E, int dk_dim, float* dWq,
                          float* dbq, float* dWk, float* dbk, float* dWv, float* dbv, float* dWo,
                          float* dbo, int accumulate, pzn_stream_t stream);

/* model5_b.py:462-475 of ONE encoder behind one entry point each way (csrc/attnchain.hip): the four layerAttention blocks, the
 * mean of their maps, the out projection over the five un-concatenated slices and the max over the points, enqueued by the
 * library on one caller-owned buffer per direction (the same kernels, in the same order, on the same operands as the entry
 * points above composed by the caller: 2 calls and 2 allocations per encoder and training step instead of 24 and ~100).
 *   params: HOST array of 34 device pointers in the module's order: per block (Wq, bq, Wk, bk, Wv, bv, Wo, bo) x 4, then the out
 *           projection's W[1024, 1280] and bias[1024].   x[B*256, 256].
 *   fwd:  map = the mean map, [B,256,256] (strips == 0) or its strip column sums [B,16,256] (strips != 0, see pzn_attn_fused_fwd);
 *         out[B*256, 1024] or NULL; fmax[B,1024], arg[B,1024]; saved: pzn_attn_chain_saved_bytes(B) bytes, 256-byte aligned,
 *         kept for the backward.
 *   bwd:  the case predict5 creates - only the maximum carries a gradient, dfg[B,1024]; grads: HOST array of 34 device pointers
 *         (accumulate != 0: all ADDED to; 0: the blocks' overwritten, the out projection's two zero-initialised by the caller);
 *         dx[B*256, 256] overwritten; scratch: pzn_attn_chain_scratch_bytes(B) bytes, 256-byte aligned.
 * The precision mode (pzn_attn_set_precision) must be the same for both calls. */
size_t pzn_attn_chain_saved_bytes(int B);
size_t pzn_attn_chain_scratch_bytes(int B);
int pzn_attn_chain_fwd_f32(const float* x, const float* const* params, int B, int strips, float* map, float* out,
                           float* fmax, int32_t* arg, void* saved, pzn_stream_t stream);
int pzn_attn_chain_bwd_f32(const float* x, const float* const* params, const void* saved, const int32_t* arg,
                           const float* dfg, int B, float* const* grads, int accumulate, float* dx, void* scratch,
                           pzn_stream_t stream);

/* First layer of the boundary heads without the concatenation (model5_b.py:745-752: Linear(cat([g.repeat(1,N,1), x], -1))
 * = x W[:,Cg:]^T per point + (g W[:,:Cg]^T + b) per cloud):
 *   pzn_cloud_bias_relu_f32:     y[b,n,:] = relu(y[b,n,:] + cb[b,:])  in place       (C % 4 == 0, 16-byte aligned)
 *   pzn_cloud_gated_colsum_f32:  dcb[b,c] = sum_n (y[b,n,c] > 0 ? dy[b,n,c] : 0)    (overwritten; fixed summation order) */
int pzn_cloud_bias_relu_f32(float* y, const float* cb, int B, int N, int C, pzn_stream_t stream);
int pzn_cloud_gated_colsum_f32(const float* dy, const float* y, int B, int N, int C, float* dcb, pzn_stream_t stream);

/* The per-point MLP chains of the boundary heads as ONE launch each way (csrc/pointmlp.hip; replaces the three
 * nn.Linear (+ ReLU) launches of nn.Sequential at model5_b.py:571-592 as called at :738-739, :751-754):
 *   y = (relu(relu(x W1^T + b1) W2^T + b2)) W3^T + b3  on M rows of 64 floats, h1 / h2 = the hidden activations.
 * Chains: 64 -> 64 -> 64 -> 64 (C2 = C3 = 64) and 64 -> 64 -> 32 -> 2 (C2 = 32, C3 = 2); W1[64, ldw1] may be a column
 * slice of a wider matrix (ldw1 >= 64); b1 is [64], or with b1_per_cloud != 0 one row of 64 per cloud of rows_per_cloud
 * rows (the folded global half of a head's first layer, see pzn_cloud_bias_relu_f32).  M % 32 == 0, 16-byte aligned
 * operands; PZN_EUNSUPPORTED for other chains (compose pzn_linear_* then). */
int pzn_point_mlp3_supported(int C0, int C1, int C2, int C3);
int pzn_point_mlp3_fwd_f32(const float* x, long long M, int rows_per_cloud, const float* W1, int ldw1,
                           const float* b1, int b1_per_cloud, const float* W2, const float* b2,
                           const float* W3, const float* b3, int C2, int C3, float* h1, float* h2,
                           float* y, pzn_stream_t stream);
/* Backward of the chain in one pass + a fixed-order sum of its partial results (timing-independent output):
 * dx[M, 64], dW1[64, ldw1] (columns 0..63 written), dW2[C2, 64], dW3[C3, C2], db2[C2], db3[C3] and db1 — [64], or with
 * b1_per_cloud != 0 one row of 64 per cloud (the gradient of the per-cloud bias) —: OVERWRITTEN (accumulate == 0) or, the
 * parameter gradients, ADDED to (accumulate != 0: one owner per element, no atomics - e.g. straight into a flat gradient
 * bucket; dx and a per-cloud db1 are overwritten either way); x, h1, h2 as the forward left them; workspace of
 * pzn_point_mlp3_bwd_workspace_bytes() bytes (0 = unsupported shape). */
size_t pzn_point_mlp3_bwd_workspace_bytes(long long M, int rows_per_cloud, int b1_per_cloud, int C2, int C3);
int pzn_point_mlp3_bwd_f32(const float* dy, const float* x, const float* h1, const float* h2, long long M,
                           int rows_per_cloud, const float* W1, int ldw1, int b1_per_cloud, const float* W2,
                           const float* W3, int C2, int C3, float* dx, float* dW1, float* db1, float* dW2,
                           float* db2, float* dW3, float* db3, int accumulate, void* workspace, pzn_stream_t stream);
/* The fixed-side boundary head of an all-pairs table (assembly.py), forward only, one launch (csrc/pointmlp.hip):
 *   y[i, j, p, :] = (relu(relu(x[i, p, :] W1^T + c[j, :]) W2^T + b2)) W3^T + b3     for i < Kf, j < Km, p < N,
 * x[Kf, N, 64] the local features of the fixed-role pieces, c[Km, 64] the first-layer bias of every moved piece (the
 * folded global half g_j W1[:, :64]^T + b1), W1[64, ldw1] the LOCAL half of the first layer (a column slice, ldw1 >= 64).
 * The first-layer product is computed once per 32-row tile and reused for every j; no hidden activation is written, no
 * workspace, no atomics (the same bits on every run).  The bias is added behind the products, so the result equals
 * pzn_point_mlp3_fwd_f32 on the materialised pair batch to rounding, not bitwise.  N % 32 == 0 and (C2, C3) = (32, 2)
 * (pzn_pair_head_supported); PZN_EUNSUPPORTED otherwise, before anything is launched.  16-byte aligned x, c, b2, y. */
int pzn_pair_head_supported(int N, int C2, int C3);
int pzn_pair_head_fwd_f32(const float* x, int Kf, int N, const float* c, int Km, const float* W1, int ldw1,
                          const float* W2, const float* b2, const float* W3, const float* b3, int C2, int C3,
                          float* y, pzn_stream_t stream);
/* The same head for Z puzzles in one launch, block-diagonal: the fixed piece (z, i) meets only the moved pieces (z, 0 .. Km-1)
 * of its own puzzle,
 *   y[z, i, j, p, :] = (relu(relu(x[z, i, p, :] W1^T + c[z, j, :]) W2^T + b2)) W3^T + b3     for z < Z, i < Kf, j < Km, p < N,
 * x[Z, Kf, N, 64], c[Z, Km, 64], y[Z, Kf, Km, N, 2].  The work item is a (32-row tile, chunk of moved pieces) pair over the tiles
 * of ALL puzzles (the j range is split until the launch fills the chip, counting every puzzle's tiles); the tile's piece gives z,
 * which offsets c and y and nothing else, so y[z] has the bits of pzn_pair_head_fwd_f32 on x[z], c[z] - that entry is the
 * Z = 1 case.  Shapes, alignment and PZN_EUNSUPPORTED as above, checked before any launch; Z = 0 is a success that launches
 * nothing. */
int pzn_pair_head_blocks_supported(int N, int C2, int C3);
int pzn_pair_head_blocks_fwd_f32(const float* x, int Z, int Kf, int N, const float* c, int Km, const float* W1,
                                 int ldw1, const float* W2, const float* b2, const float* W3, const float* b3,
                                 int C2, int C3, float* y, pzn_stream_t stream);

/* The encoder's out projection and the max over the points in ONE launch (model5_b.py:466-475):
 *   out[b,l,:] = cat(x[0] .. x[nslice-1])[b,l,:] W^T + bias   (W[Nout, nslice*E]; the concatenation is never built),
 *   fmax[b,:] = max_l out[b,l,:],  arg[b,:] = its point (the lowest one on ties, as torch.max).
 * out may be NULL: predict5 uses only the maximum (model5_b.py:723).  Shape taken: L = 256, E = 256, nslice = 5,
 * Nout = 1024 (pzn_outproj_maxpts_workspace_bytes > 0; the workspace, 16-byte aligned, holds the split planes of W);
 * everything else, and the exact-fp32 engine, returns PZN_EUNSUPPORTED (compose pzn_linear_slice_fwd_f32 +
 * pzn_maxpool_points_fwd_f32 then).  arg feeds pzn_linear_maxpts_dgrad/wgrad_f32. */
size_t pzn_outproj_maxpts_workspace_bytes(int L, int E, int nslice, int Nout);
int pzn_outproj_maxpts_fwd_f32(const float* const* x, int nslice, const float* W, const float* bias, int B, int L, int E,
                               int Nout, float* out, float* fmax, int32_t* arg, void* workspace, pzn_stream_t stream);

/* torch.max(x, dim=1) over the point axis (model5_b.py:475 global feature, :741): out[b,c] =
 * max_l x[b,l,c], idx[b,c] = its row (the lowest one on ties); backward dx[b,l,c] =
 * (l == idx[b,c]) ? dout[b,c] : 0, every element of dx written (any C; C % 4 == 0 with 16-byte aligned
 * pointers takes the vector kernels). */
int pzn_maxpool_points_fwd_f32(const float* x, int B, int L, int C, float* out, int32_t* idx,
                               pzn_stream_t stream);
int pzn_maxpool_points_bwd_f32(const float* dout, const int32_t* idx, int B, int L, int C,
                               float* dx, pzn_stream_t stream);

/* Backward of "linear, then max over the points" (model5_b.py:474-475: out = self.out(att); f_global = max over
 * dim 1) when only the maximum is used downstream (predict5, model5_b.py:723): the gradient of the [B*L, Nout]
 * product has one non-zero per (cloud, channel), at row arg[b,c] (pzn_maxpool_points_fwd_f32's idx), so both
 * products are B*Nout row operations instead of B*L*Nout*Kin multiply-adds:
 *   dgrad:  dx[b,l,:] = sum over {c: arg[b,c]==l} dg[b,c] W[c,:]        (every element of dx written; Kin % 64 == 0,
 *           L <= 600, Nout <= 16384, W[Nout,Kin] dense; workspace of pzn_linear_maxpts_workspace_bytes(B, Nout)
 *           bytes, 16-byte aligned: the channels of each cloud sorted by selected row; summation order is fixed,
 *           results are reproducible)
 *   wgrad:  dW[c, s*seg_cols + k] += sum_b dg[b,c] x_s[b, arg[b,c], k],  db[c] += sum_b dg[b,c]  (db may be NULL);
 *           x is given as nseg <= 8 separate [B*L, seg_cols] tensors — the column blocks of a concatenation that
 *           need not exist (x_segs: HOST array of nseg device pointers; seg_cols % 4 == 0; dW[Nout, nseg*seg_cols]).
 * PZN_EUNSUPPORTED outside these shapes (callers then take pzn_maxpool_points_bwd_f32 + the dense products). */
size_t pzn_linear_maxpts_workspace_bytes(int B, int Nout);
int pzn_linear_maxpts_dgrad_f32(const float* dg, const int32_t* arg, const float* W, int B, int L, int Kin,
                                int Nout, void* workspace, float* dx, pzn_stream_t stream);
int pzn_linear_maxpts_wgrad_f32(const float* dg, const int32_t* arg, const float* const* x_segs, int nseg,
                                int seg_cols, int B, int L, int Nout, float* dW, float* db, pzn_stream_t stream);

/* SE(3) exponential of the pose head (se_math/se3.py:57-80 with so3.mat and the Taylor-guarded
 * sinc1/2/3 of se_math/sinc.py): twist[B,6] = (w, v) -> g[B,4,4]; backward dg[B,4,4] ->
 * dtwist[B,6] (the last row of dg is ignored: it is constant). */
int pzn_se3_exp_fwd_f32(const float* twist, int B, float* g, pzn_stream_t stream);
int pzn_se3_exp_bwd_f32(const float* twist, const float* dg, int B, float* dtwist,
                        pzn_stream_t stream);

/* se3.transform on points (se_math/se3.py:110-120 as model5_b.py:948-952, :1116 use it): out[b,n,:] = R_b p[b,n,:] + t_b
 * with g[B,4,4] = [[R, t], [0 0 0 1]] and p[B,N,3].  bwd: dp[B,N,3] = R^T dout (may be NULL), dg[B,4,4] (may be NULL;
 * overwritten: dR = sum_n dout p^T, dt = sum_n dout, last row 0). */
int pzn_se3_transform_fwd_f32(const float* g, const float* p, int B, int N, float* out, pzn_stream_t stream);
int pzn_se3_transform_bwd_f32(const float* g, const float* p, const float* dout, int B, int N, float* dp,
                              float* dg, pzn_stream_t stream);
/* TouchedRegraster.comp (model5_b.py:1512-1519): loss[0] = 16 * mean((g igt - I)^2) over [B,4,4];
 * bwd: dg[B,4,4] = dloss[0] * d loss / d g (igt is data). */
int pzn_comp_fwd_f32(const float* g, const float* igt, int B, float* loss, pzn_stream_t stream);
int pzn_comp_bwd_f32(const float* g, const float* igt, const float* dloss, int B, float* dg, pzn_stream_t stream);
/* Boundary head losses (model5_b.py:1063-1064 F.cross_entropy(logits[B,2,N], labels) with mean reduction, and :1085-1090
 * softmax(logits, dim=1)[:, 1, :]): labels[B,N] hold 0 / 1 as floats (dataset.py:1363-1366).  fwd: prob1[B,N] (class-1
 * probability, what the top-128 selection ranks by), loss[0] (overwritten); loss points at PZN_BOUNDARY_CE_LOSS_FLOATS floats:
 * the value and the per-workgroup partial sums it is reduced from in a fixed order (bit-reproducible).
 * bwd: dlogits[B,2,N] = dloss[0] * d loss / d logits.
 * points_major != 0: logits (and dlogits) are the heads' [B,N,2] output as it lies in memory - the [B,2,N] tensor the reference
 * builds with permute(0,2,1) (model5_b.py:751-754) read through its strides, no transposed copy either way. */
#define PZN_BOUNDARY_CE_LOSS_FLOATS 513
int pzn_boundary_ce_fwd_f32(const float* logits, const float* labels, int B, int N, int points_major, float* prob1,
                            float* loss, pzn_stream_t stream);
int pzn_boundary_ce_bwd_f32(const float* logits, const float* labels, const float* dloss, int B, int N,
                            int points_major, float* dlogits, pzn_stream_t stream);
/* torch.topk(x[R,N], K, dim=1)[1] (model5_b.py:1089-1091): indices of the K largest entries of every row, value
 * descending, equal values by ascending index.  K <= 256, N <= 16384 (PZN_EUNSUPPORTED beyond). */
int pzn_topk_rows_f32(const float* x, int R, int N, int K, int64_t* idx, pzn_stream_t stream);
/* (((a + b) + c) + d) / 4 elementwise (model5_b.py:468-469: the mean of the four attention maps); n % 4 == 0, 16-byte
 * aligned pointers (PZN_EUNSUPPORTED otherwise). */
int pzn_avg4_f32(const float* a, const float* b, const float* c, const float* d, size_t n, float* out,
                 pzn_stream_t stream);
/* a[B,R,C] -> mean[B,C] = a.mean(dim=1) and arg[B] = index of its largest entry (the lowest on ties): model5_b.py:937-942,
 * `x2[:, topk(attention.mean(dim=1), 32)[1][:, 0]]` needs only the first of the 32.  C <= 1024; workspace of
 * pzn_colmean_workspace_bytes(B, C) bytes (partial column sums, fixed summation order). */
size_t pzn_colmean_workspace_bytes(int B, int C);
int pzn_colmean_argmax_f32(const float* a, int B, int R, int C, float* mean, int64_t* arg, void* workspace,
                           pzn_stream_t stream);

/* torch.optim.Adam step (model5_b.py:1453-1457: Adam(lr), no weight decay, no amsgrad) over flat
 * buffers of n floats: param, exp_avg, exp_avg_sq updated in place from grad; step = 1, 2, ...
 * (bias corrections 1 - beta^step).  All four buffers 16-byte aligned. */
int pzn_adam_step_f32(float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                      size_t n, float lr, float beta1, float beta2, float eps, int step,
                      pzn_stream_t stream);

/* ------------------------------------------------------------------------ */
/* Data pipeline on the GPU: dataset.py                        */
/* ------------------------------------------------------------------------ */

/* dataset.py:761-775 + 1176-1180 (CADDataset.slice with its re-draw loop) for a batch, one launch: K candidate planes per sample
 * (normals float64 [B,K,3] = np.random.rand(3,1), zs float64 [B,K] = np.random.rand(1)/3), the FIRST that leaves >= n_min points
 * on both sides is taken (none: the most balanced one, ok = 0).  pieces [2B,cap,3]: rows 0..B-1 the `up` pieces
 * (points . normal + z >= 0, float64, no fma), rows B..2B-1 the `down` pieces, each in the cloud's point order and padded with
 * copies of its first row; counts int64 [2B]; start int64 [2B] = floor(u * count) (u float64 [B,2]: uniform draws standing in for
 * np.random.randint(0, n_piece), dataset.py:1153); plane float64 [B,4] = (normal, z) taken; ok uint8 [B]. */
int pzn_cut_compact_f32(const float* raw, const double* normals, const double* zs, const double* u, int B, int M,
                        int K, int n_min, int cap, float* pieces, int64_t* counts, int64_t* start, double* plane,
                        uint8_t* ok, pzn_stream_t stream);
/* dataset.py:715-759 (sphere_split / cylinder_split / cone_split) + 1175-1179 (the re-draw loop) for a batch, one launch; the
 * contract of pzn_cut_compact_f32 with a solid in place of the plane.  kind 0 sphere, 1 cylinder, 2 cone (uniform per launch);
 * params float64 [B,K,6] = (rot[3] = np.random.rand(3,1), shift[3] = np.random.rand(3,1)/3) per candidate: the sphere ignores
 * rot, the cone ignores shift.  `up` (rows 0..B-1 of pieces) = strictly INSIDE the polyhedron open3d 0.15.2 builds at
 * resolution 50 (create_sphere(0.5, 50) translated by shift; create_cylinder(0.6, 1, 50) rotated by the axis-angle vector rot
 * about the origin, then translated by shift; create_cone(1, 2, 50) translated by (0,0,-1), then rotated by rot), `down` (rows
 * B..2B-1) = the rest; float64, no fma.  The FIRST candidate with n_min <= n_up and n_min <= M - n_up is taken (none: the most
 * balanced one, the first among equals, ok = 0; ok = 0 also when a piece exceeds cap).  pieces, counts, start as in
 * pzn_cut_compact_f32; chosen float64 [B,6] = the parameters taken, chosen_k int32 [B] their candidate index; ok uint8 [B]. */
int pzn_cut_compact_solid_f32(const float* raw, int kind, const double* params, const double* u, int B, int M, int K,
                              int n_min, int cap, float* pieces, int64_t* counts, int64_t* start, double* chosen,
                              int32_t* chosen_k, uint8_t* ok, pzn_stream_t stream);
/* dataset.py:1203-1355 (CADDataset.__getitem__ with split_twice=True, `train.py --random_slice`) up to the sampling, for a
 * batch, one launch: steps 1-7 of datapipe.double_cut_rule, which is the statement of this entry point.  Draws per sample:
 * normals1 float64 [B,K,3], zs1 float64 [B,K] = K candidates for plane 1; normals2 float64 [B,7,3], zs2 float64 [B,7] = the
 * first draw of plane 2 and the six re-draws of `while time <= 5`; u float64 [B,7] = u_seed, u_se, u_choice, u_sU, u_sD, u_sFU,
 * u_sFD.  side = (points . normal + z >= 0), float64, no fma, as in pzn_cut_compact_f32.  n_min: the points a piece must hold
 * (the reference's 1024); n_rich: the points a piece must hold to be cut again (the reference's 3000, dataset.py:1214-1217).
 * pieces [4B,cap,3]: rows 0..B-1 U, B..2B-1 D, 2B..3B-1 / 3B..4B-1 the pair of plane 1 alone that replaces a HALF_VS_OTHER
 * pair whose boundaries do not touch; each piece = rows of its first region table, then of its second, in the cloud's point
 * order, padded with copies of its first row.  counts int64 [4B] (-1 in the fallback rows of samples that are not
 * HALF_VS_OTHER: their rows are copies of the cloud's first point); start int64 [4B] = clamp(floor(u * count), 0, count - 1);
 * kind int32 [B] (0 SINGLE, 1 HALF_VS_REST, 2 HALF_VS_OTHER, 3 HALVES); planes float64 [B,2,4] = (normal, z) of the two planes
 * taken (plane 2 zero for SINGLE); tabs int32 [B,4] = the region tables u_tab[2], d_tab[2] (bit 2 s1 + s2); ok uint8 [B]: 0 when
 * SINGLE found no valid candidate among the K (the most balanced one is taken, the first among equals) or a piece exceeds cap. */
int pzn_cut_compact_double_f32(const float* raw, const double* normals1, const double* zs1, const double* normals2,
                               const double* zs2, const double* u, int B, int M, int K, int n_min, int n_rich, int cap,
                               float* pieces, int64_t* counts, int64_t* start, int32_t* kind, double* planes, int32_t* tabs,
                               uint8_t* ok, pzn_stream_t stream);
/* Fracture (no counterpart in the reference, which ships pairs only): every cloud of a batch cut into P pieces by P - 1 planes,
 * one launch, one workgroup per sample; datapipe.fracture_rule is the statement of this entry point.  All points start with
 * label 0.  Step s = 1 .. P-1: the target t is the label with the most points among 0 .. s-1 (ties: the lowest); candidate k
 * (k < K) is the plane with normal normals[b,s-1,k] (float64 [B,P-1,K,3]) through the ANCHOR, the target's r-th point in the
 * cloud's order, r = clamp(floor(u_anchor[b,s-1,k] count[t]), 0, count[t] - 1) (u_anchor float64 [B,P-1,K]); its offset is
 * -((x n0 + y n1) + z n2) of the anchor and its side test that of pzn_cut_compact_f32 (float64, no fma), so the anchor is at
 * exactly 0, on the up side.  The FIRST candidate that leaves >= n_min target points on both sides is taken (none: the most
 * balanced one, the first among equals, ok = 0); the up side keeps t, the down side becomes s.
 * pieces [P B,cap,3]: piece p of sample b at row p B + b, the rows of label p in the cloud's order, padded with copies of its
 * first row (of the cloud's first row when it is empty); rows beyond cap are not written (ok = 0).  counts int64 [P B];
 * start int64 [P B] = clamp(floor(u_start[b,p] count), 0, count - 1) (u_start float64 [B,P]); label uint8 [B,M]; order int32
 * [B,M]: the cloud row of every position of the concatenated pieces (the stable argsort of label); planes float64 [B,P-1,4]
 * (normal, offset); target, cand int32 [B,P-1]: the label cut and the candidate taken at every step; ok uint8 [B].
 * 2 <= P <= 16, K >= 1, 1 <= M <= 65536 (pzn_fracture_supported: 1 / 0), PZN_EUNSUPPORTED otherwise, before any launch. */
int pzn_fracture_supported(int M, int P, int K);
int pzn_fracture_f32(const float* raw, const double* normals, const double* u_anchor, const double* u_start, int B, int M,
                     int P, int K, int n_min, int cap, float* pieces, int64_t* counts, int64_t* start, uint8_t* label,
                     int32_t* order, double* planes, int32_t* target, int32_t* cand, uint8_t* ok, pzn_stream_t stream);
/* A training pair cut out of a fracture, one launch, one workgroup per sample; datapipe.fracture_pair_rule is the statement of
 * this entry point.  raw, normals, u_anchor, n_min, cap and the steps as in pzn_fracture_f32, made for s = 1 .. P_b - 1 with
 * P_b = n_pieces[b] (int32 [B], 2 <= P_b <= P; the draws of later steps are not read; planes, target and cand rows from
 * P_b - 1 on are zero).  u float64 [B,7] = u_kind, u_a, u_c, u_sU, u_sD, u_sFU, u_sFD.  The SIBLING pair is U = target[P_b-2]
 * (the up side of the last cut), D = P_b - 1 (its down side).  kind int32 [B]: 1 NEIGHBOUR iff P_b >= 3, u_kind < neighbours
 * (0 <= neighbours <= 1) and the drawn pair a = min(P_b - 1, floor(u_a P_b)), c = c' + (c' >= a) with c' = min(P_b - 2,
 * floor(u_c (P_b - 1))) is not the sibling pair in either order: then (U, D) = (a, c) and the sibling pair is the fallback;
 * else 0 SIBLING, without a fallback.  pieces [4B,cap,3]: rows 0..B-1 U, B..2B-1 D, 2B..3B-1 / 3B..4B-1 the fallback pair, each
 * the rows of its label in the cloud's order, padded as in pzn_fracture_f32; counts int64 [4B] (-1 where there is no fallback:
 * those rows are copies of the cloud's first point, start 0); start int64 [4B] = clamp(floor(u_s* count), 0, count - 1);
 * pair int32 [B,4]: the four labels (-1: none); label uint8 [B,M]; planes float64 [B,P-1,4]; target, cand int32 [B,P-1];
 * ok uint8 [B]: every step made had a valid candidate and every written piece fits in cap.  n_pieces lives on the device, so a
 * value outside 2 .. P is refused by the launch itself: that sample gets kind -1, no piece (counts -1), label 0 and ok = 0.
 * Limits: those of pzn_fracture_f32 (pzn_fracture_pair_supported: 1 / 0), PZN_EUNSUPPORTED otherwise, before any launch. */
int pzn_fracture_pair_supported(int M, int P, int K);
int pzn_fracture_pair_f32(const float* raw, const double* normals, const double* u_anchor, const int32_t* n_pieces,
                          const double* u, double neighbours, int B, int M, int P, int K, int n_min, int cap, float* pieces,
                          int64_t* counts, int64_t* start, int32_t* kind, int32_t* pair, uint8_t* label, double* planes,
                          int32_t* target, int32_t* cand, uint8_t* ok, pzn_stream_t stream);
/* pzn_fracture_f32 with curved break surfaces, one launch; datapipe.fracture_curved_rule is the statement of this entry point.
 * Candidate k of step s is a second-order patch through the anchor a (chosen as in pzn_fracture_f32): a paraboloid in the frame
 * frames[b,s-1,k] (float64 [B,P-1,K,3,3], rows e1, e2, n) with the half curvatures half_curv[b,s-1,k] = (c1, c2) = (kappa1 / 2,
 * kappa2 / 2) (float64 [B,P-1,K,2]); both are taken as given, neither normalised nor checked.  A point x is on the up side iff
 * f >= 0, in float64 with every operation rounded on its own (no fma): d = x - a (the float32 coordinates widened, three
 * subtractions); s1 = (d0 e1[0] + d1 e1[1]) + d2 e1[2], s2 and h likewise with e2 and n; f = (h + (c1 s1) s1) + (c2 s2) s2.
 * The anchor has d = 0, so it is at exactly 0, on the up side; (0, 0) is the plane with normal n.  Everything else - the target,
 * the anchor's rank, the first valid candidate else the first most balanced one, the labels, and every output - is as in
 * pzn_fracture_f32, except: planes float64 [B,P-1,4] is the TANGENT plane at the anchor, (n, -((ax n0 + ay n1) + az n2)), and
 * anchor int32 [B,P-1] is the cloud row of the anchor taken at every step.
 * Limits: those of pzn_fracture_f32 (pzn_fracture_curved_supported: 1 / 0), PZN_EUNSUPPORTED otherwise, before any launch. */
int pzn_fracture_curved_supported(int M, int P, int K);
int pzn_fracture_curved_f32(const float* raw, const double* frames, const double* half_curv, const double* u_anchor,
                            const double* u_start, int B, int M, int P, int K, int n_min, int cap, float* pieces,
                            int64_t* counts, int64_t* start, uint8_t* label, int32_t* order, double* planes, int32_t* target,
                            int32_t* cand, int32_t* anchor, uint8_t* ok, pzn_stream_t stream);
/* pzn_fracture_pair_f32 with the curved break surfaces of pzn_fracture_curved_f32 (frames, half_curv in place of normals), one
 * launch; datapipe.fracture_pair_curved_rule is the statement of this entry point.  The pair, the pieces and every output are as
 * in pzn_fracture_pair_f32, except: planes holds the tangent planes, and anchor int32 [B,P-1] the cloud row of the anchor taken
 * at every step (rows from P_b - 1 on, and every row of a sample whose n_pieces is out of range, are zero, like target and cand).
 * Limits: those of pzn_fracture_f32 (pzn_fracture_pair_curved_supported: 1 / 0), PZN_EUNSUPPORTED otherwise, before any launch. */
int pzn_fracture_pair_curved_supported(int M, int P, int K);
int pzn_fracture_pair_curved_f32(const float* raw, const double* frames, const double* half_curv, const double* u_anchor,
                                 const int32_t* n_pieces, const double* u, double neighbours, int B, int M, int P, int K,
                                 int n_min, int cap, float* pieces, int64_t* counts, int64_t* start, int32_t* kind,
                                 int32_t* pair, uint8_t* label, double* planes, int32_t* target, int32_t* cand, int32_t* anchor,
                                 uint8_t* ok, pzn_stream_t stream);
/* pzn_fracture_f32 / pzn_fracture_curved_f32 with EROSION, one launch: at every cut the target's points close to the taken
 * surface are lost and belong to no piece; datapipe.fracture_eroded_rule is the statement of this entry point.  The cuts are
 * planes (normals, with frames = half_curv = NULL) or surfaces (frames and half_curv, with normals = NULL); anything else is
 * PZN_EINVAL, before any launch.  erode float64 [B,P-1,4] = (w_up, w_dn, depth, rho) per step, taken as given: neither clamped
 * nor checked.  For candidate k of step s through the anchor a let f(x) be the value whose sign the side test takes - the plane's
 * ((x n0 + y n1) + z n2) + off, the surface's f of pzn_fracture_curved_f32 - in float64, every operation rounded on its own.  A
 * member x of the target is LOST under that candidate iff -w_dn < f < w_up (the band), or -depth < f < depth and r2 < rho rho
 * (the chip) with d = x - a (the float32 coordinates widened, three subtractions) and r2 = (d0 d0 + d1 d1) + d2 d2.  All
 * comparisons are strict: zeros lose nothing, and neither does a NaN; with w_up > 0 and w_dn > 0 the anchor itself (f = 0) is lost.  Up is the members
 * with f >= 0 that are not lost, down those with f < 0 that are not lost; a candidate is valid iff both hold >= n_min points and
 * its balance is the smaller of the two; the first valid candidate is taken, else the first most balanced one; up keeps t, down
 * becomes s, and the lost points get label 255: they are never counted or targeted again.  A step whose target holds no point
 * (everything has been lost) is not made: its rows of planes, cand, anchor and lost are zero, target is t, and ok = 0.  f is the
 * offset along n to the surface, so across a cut the kept points of the two sides are >= w_up + w_dn apart along n.
 * Outputs as in pzn_fracture_f32 (planes: the tangent planes for surfaces), except: counts exclude the lost points; order is
 * still the stable argsort of label, so the lost rows stand behind the last piece, in the cloud's order; anchor int32 [B,P-1] is
 * the cloud row of the anchor taken (the chip's centre), for planes too; lost int32 [B,P-1] is the number of points lost at
 * every step, so the counts of a sample and its lost sum to M.
 * Limits: those of pzn_fracture_f32 (pzn_fracture_eroded_supported: 1 / 0), PZN_EUNSUPPORTED otherwise, before any launch. */
int pzn_fracture_eroded_supported(int M, int P, int K);
int pzn_fracture_eroded_f32(const float* raw, const double* normals, const double* frames, const double* half_curv,
                            const double* u_anchor, const double* u_start, const double* erode, int B, int M, int P, int K,
                            int n_min, int cap, float* pieces, int64_t* counts, int64_t* start, uint8_t* label, int32_t* order,
                            double* planes, int32_t* target, int32_t* cand, int32_t* anchor, int32_t* lost, uint8_t* ok,
                            pzn_stream_t stream);
/* pzn_fracture_pair_f32 / pzn_fracture_pair_curved_f32 with the erosion of pzn_fracture_eroded_f32 (normals, or frames and
 * half_curv, as there; erode float64 [B,P-1,4], rows from P_b - 1 on are not read), one launch;
 * datapipe.fracture_pair_eroded_rule is the statement of this entry point.  The pair and every output are as in
 * pzn_fracture_pair_f32, on the eroded pieces: a lost point (label 255) is in no piece; anchor and lost int32 [B,P-1] as in
 * pzn_fracture_eroded_f32, their rows from P_b - 1 on zero like those of target and cand.
 * Limits: those of pzn_fracture_f32 (pzn_fracture_pair_eroded_supported: 1 / 0), PZN_EUNSUPPORTED otherwise, before any launch. */
int pzn_fracture_pair_eroded_supported(int M, int P, int K);
int pzn_fracture_pair_eroded_f32(const float* raw, const double* normals, const double* frames, const double* half_curv,
                                 const double* u_anchor, const int32_t* n_pieces, const double* u, const double* erode,
                                 double neighbours, int B, int M, int P, int K, int n_min, int cap, float* pieces,
                                 int64_t* counts, int64_t* start, int32_t* kind, int32_t* pair, uint8_t* label, double* planes,
                                 int32_t* target, int32_t* cand, int32_t* anchor, int32_t* lost, uint8_t* ok,
                                 pzn_stream_t stream);
/* dataset.py:1363-1366: 0/1 masks [R,N] with ones at the k picked rows idx int64 [R,k] of each cloud. */
int pzn_pick_mask_f32(const int64_t* idx, int R, int k, int N, float* mask, pzn_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* PZN_H_ */
