// jointrefine.hip — refine all piece poses of a placed assembly jointly over every joint, for gfx950 (assembly.refine_assembly).
//
// One workgroup per puzzle z does block-coordinate descent on the pose graph, with the poses G[K] in LDS and the arithmetic of
// icprefine.hip (pzn_rigid.h): what would otherwise be transform -> chamfer -> two gathers -> centring -> 3x3 solve -> compose
// per piece per sweep from the host.
//   * joint e = (i, j) has the set A_e (ka points, piece i's frame) and B_e (kb points, piece j's frame); its energy is the
//     pair table's score with both sides in the root frame, E_e = mean_r min_c |G_i a_r - G_j b_c|^2 + mean_c min_r (same),
//     fp32 differences (pzn::sqdist3), arg-min = the lowest index.  Row r < ka is G_i a_r scanning G_j B, row ka + c is
//     G_j b_c scanning G_i A; a thread owns rows tid, tid + 256, ..., adds their minima in that order, the wave adds its lanes
//     by the xor butterfly, the four wave sums are added in wave order (icprefine.hip's evaluate);
//   * a visit of piece p: E_p = the fp32 sum, in list order, of E_e over the joints with i = p or j = p.  While they are
//     evaluated every row adds its pair (x = the point of p's side in p's frame, y = its partner's fp32 root-frame image,
//     weight 1 / ka for a row of A and 1 / kb for a row of B) to 22 float64 sums: w, w x, w y, w x y^T and the upper triangle
//     of w x x^T, of x - x0 and y - y0 (x0 = point 0 of p's side of its first joint, y0 = its image: a shift the centred
//     sums do not depend on, which keeps them well conditioned far from the origin); thread, butterfly, wave order.  Thread 0
//     centres them and solves in float64: Horn's quaternion on S = sum w (x - xc)(y - yc)^T, t = yc - R xc, rounded to fp32;
//     a degenerate scatter of x keeps R_p (solve_pose in pzn_rigid.h).  The candidate is evaluated on the same joints and taken
//     iff E_p' < E_p (NaN rejects); only p's joints depend on G_p, so no visit raises the total - and the fp32 total, the
//     sum over all rows in list order of the current E_e (kept in LDS), is held to that as well: a candidate under which it
//     would round above the current total is left.  score and joint_score are that total and those E_e;
//   * a sweep visits p = 0 .. K-1 in order (movable pieces with a joint), later pieces see earlier pieces' new poses; the
//     loop ends after `sweeps` sweeps or after one that took nothing.
// LDS holds, for the joint being evaluated, the far side's root-frame image, p's side as given and p's side under the pose
// being tried; the sets are read again from global memory (L2) for every evaluation, the joint list is scanned there.  Every
// loop bound and every branch around a barrier depends on the joint list, `movable` and E values that are the same bits in
// all 256 threads.  A joint row with i or j outside [0, K) or i == j is skipped everywhere (joint_score 0).  A pair listed
// twice counts twice; a piece that is an end of more than 2 K rows (only possible that way) is never visited.
// The same body with a count per set (joint_refine_counts_kernel behind pzn_joint_refine_counts_f32; the body's template
// argument COUNTS): the ka and kb of a row above are then na / nb of that row's sets, read by all threads from one address,
// and a row with a count outside [1, ka] / [1, kb] is skipped like a bad (i, j); ka and kb remain the strides of the sets
// and the size of the LDS images.
#include "pzn_rigid.h"

namespace {

constexpr int JR_T = 256;                  // four wavefronts
constexpr int JR_W = JR_T / PZN_WAVE;
constexpr int JR_MAX_K = 1024;             // points per side: 9 x 4 KB of images
constexpr int JR_MAX_PIECES = 64;          // 3 KB of poses, at most 16 KB of joint energies: 57 KB of LDS with 1024 points a side
constexpr int JR_MAX_GRID = 512;           // two workgroups per CU of a 256-CU part; more puzzles share a workgroup in turn
constexpr int JR_SUMS = 22;                // w, wx[3], wy[3], wxy[9], wxx[6]

struct Lds {
  float *fx, *fy, *fz;      // far side's root-frame image, [kmax] (kmax = max(ka, kb) rounded up to a multiple of 4)
  float *ox, *oy, *oz;      // own side as given, [kmax]
  float *tx, *ty, *tz;      // own side under the pose being tried, [kmax]
  float* G;                 // [K][12] the poses: r[9], t[3]
  double* redd;             // [JR_W][JR_SUMS] wave partials of the float64 sums
  float* rede;              // [JR_W][2] wave partials of the two objective sums
  float* cand;              // [12] the candidate pose, thread 0 -> everyone
  int* taken;               // [K] accepted visits
  float* js;                // [J] E_e of every row under the current poses (0 for a skipped row)
  float* jn;                // [2 K] E_e of the visited piece's joints under the candidate
};

struct Sets {
  const float* a;
  const int64_t* a_of;
  const float* b;
  const int64_t* b_of;
  int ka, kb;                   // the strides of a and b, and what sizes the LDS
  const int32_t *na, *nb;       // points per set of a / of b, indexed by the set (COUNTS launches; NULL: ka / kb everywhere)
};

__device__ __forceinline__ Pose load_pose(const float* g) {
  Pose p;
#pragma unroll
  for (int k = 0; k < 9; ++k) p.r[k] = g[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) p.t[k] = g[9 + k];
  return p;
}

// E_e of joint row `row` (global index z * J + e) with `own_is_b ? B : A` as the own side under `own` and the other side
// under `far`.  SUMS: every row adds its pair to acc (shifted by ref, which the first call of a visit sets: have_ref).
// The sets hold ka and kb points (the row's counts: S.ka / S.kb without counts, 1 <= ka <= S.ka and 1 <= kb <= S.kb with them,
// the same value in every thread); rows of a set behind its count are never read, and the LDS behind it holds whatever an
// earlier joint left.  Three barriers; on entry no thread may still be reading the images or rede (every caller comes from a
// barrier).
template <bool SUMS>
__device__ float eval_joint(const Lds& L, const Sets& S, size_t row, int ka, int kb, bool own_is_b, const Pose& own,
                            const Pose& far, int tid, double (&acc)[JR_SUMS], float (&ref)[6], bool& have_ref) {
  const float* ga = S.a + (size_t)(S.a_of ? S.a_of[row] : (int64_t)row) * S.ka * 3;
  const float* gb = S.b + (size_t)(S.b_of ? S.b_of[row] : (int64_t)row) * S.kb * 3;
  const float* gown = own_is_b ? gb : ga;
  const float* gfar = own_is_b ? ga : gb;
  const int kown = own_is_b ? kb : ka, kfar = own_is_b ? ka : kb;
  for (int q = tid; q < kown; q += JR_T) {
    const float x = gown[3 * q], y = gown[3 * q + 1], z = gown[3 * q + 2];
    L.ox[q] = x, L.oy[q] = y, L.oz[q] = z;
    pose_move(own, x, y, z, L.tx[q], L.ty[q], L.tz[q]);
  }
  for (int q = tid; q < kfar; q += JR_T) pose_move(far, gfar[3 * q], gfar[3 * q + 1], gfar[3 * q + 2], L.fx[q], L.fy[q], L.fz[q]);
  __syncthreads();
  if (SUMS && !have_ref) {
    ref[0] = L.ox[0], ref[1] = L.oy[0], ref[2] = L.oz[0];
    ref[3] = L.tx[0], ref[4] = L.ty[0], ref[5] = L.tz[0];
    have_ref = true;
  }
  // the images of A and of B, whichever side is the own one
  const float* Ax = own_is_b ? L.fx : L.tx;
  const float* Ay = own_is_b ? L.fy : L.ty;
  const float* Az = own_is_b ? L.fz : L.tz;
  const float* Bx = own_is_b ? L.tx : L.fx;
  const float* By = own_is_b ? L.ty : L.fy;
  const float* Bz = own_is_b ? L.tz : L.fz;
  const double wa = 1.0 / (double)ka, wb = 1.0 / (double)kb;
  float s1 = 0.f, s2 = 0.f;
  const int rows = ka + kb;
  for (int r = tid; r < rows; r += JR_T) {
    const bool a_row = r < ka;
    const int me = a_row ? r : r - ka;
    const float qx = a_row ? Ax[me] : Bx[me];
    const float qy = a_row ? Ay[me] : By[me];
    const float qz = a_row ? Az[me] : Bz[me];
    const float* sx = a_row ? Bx : Ax;
    const float* sy = a_row ? By : Ay;
    const float* sz = a_row ? Bz : Az;
    const int n = a_row ? kb : ka;
    float best = __builtin_inff();
    int arg = 0;
    // (G_i a - G_j b)^2 and (G_j b - G_i a)^2 are the same bits (the difference only changes its sign), so one form serves
    // both directions; candidates in index order with a strict <: the lowest index of equal distances stays.  Four
    // candidates per 16-byte LDS read (the images start on 16-byte boundaries), the rest one by one.
    int c = 0;
    for (; c + 4 <= n; c += 4) {
      const float4 X = *reinterpret_cast<const float4*>(sx + c);
      const float4 Y = *reinterpret_cast<const float4*>(sy + c);
      const float4 Z = *reinterpret_cast<const float4*>(sz + c);
      const float d0 = pzn::sqdist3(qx, qy, qz, X.x, Y.x, Z.x), d1 = pzn::sqdist3(qx, qy, qz, X.y, Y.y, Z.y);
      const float d2 = pzn::sqdist3(qx, qy, qz, X.z, Y.z, Z.z), d3 = pzn::sqdist3(qx, qy, qz, X.w, Y.w, Z.w);
      bool take = d0 < best;
      best = take ? d0 : best, arg = take ? c : arg;
      take = d1 < best;
      best = take ? d1 : best, arg = take ? c + 1 : arg;
      take = d2 < best;
      best = take ? d2 : best, arg = take ? c + 2 : arg;
      take = d3 < best;
      best = take ? d3 : best, arg = take ? c + 3 : arg;
    }
    for (; c < n; ++c) {
      const float d = pzn::sqdist3(qx, qy, qz, sx[c], sy[c], sz[c]);
      const bool take = d < best;
      best = take ? d : best;
      arg = take ? c : arg;
    }
    if (a_row)
      s1 = __fadd_rn(s1, best);
    else
      s2 = __fadd_rn(s2, best);
    if (SUMS) {
      const int ia = a_row ? me : arg, ib = a_row ? arg : me;      // the pair (a_ia, b_ib)
      const int io = own_is_b ? ib : ia, ifar = own_is_b ? ia : ib;
      const double w = a_row ? wa : wb;
      const double x0 = (double)L.ox[io] - (double)ref[0], x1 = (double)L.oy[io] - (double)ref[1], x2 = (double)L.oz[io] - (double)ref[2];
      const double y0 = (double)L.fx[ifar] - (double)ref[3], y1 = (double)L.fy[ifar] - (double)ref[4], y2 = (double)L.fz[ifar] - (double)ref[5];
      const double wx0 = w * x0, wx1 = w * x1, wx2 = w * x2;
      acc[0] += w;
      acc[1] += wx0, acc[2] += wx1, acc[3] += wx2;
      acc[4] += w * y0, acc[5] += w * y1, acc[6] += w * y2;
      acc[7] += wx0 * y0, acc[8] += wx0 * y1, acc[9] += wx0 * y2;
      acc[10] += wx1 * y0, acc[11] += wx1 * y1, acc[12] += wx1 * y2;
      acc[13] += wx2 * y0, acc[14] += wx2 * y1, acc[15] += wx2 * y2;
      acc[16] += wx0 * x0, acc[17] += wx1 * x1, acc[18] += wx2 * x2;
      acc[19] += wx0 * x1, acc[20] += wx0 * x2, acc[21] += wx1 * x2;
    }
  }
  float e1, e2;
  block_sum2_f32<JR_W>(L.rede, tid, s1, s2, e1, e2);
  const float e = __fadd_rn(__fdiv_rn(e1, (float)ka), __fdiv_rn(e2, (float)kb));
  __syncthreads();      // rede and the images are free again
  return e;
}

// The candidate pose of a visit from its 22 sums (every thread's acc) and the current pose (its rotation is kept when the
// scatter of x is degenerate).  Two barriers; the result is in L.cand and in every thread's registers.
__device__ Pose candidate(const Lds& L, const Pose& cur, double (&acc)[JR_SUMS], const float (&ref)[6], int tid) {
  const int lane = tid & (PZN_WAVE - 1), wave = tid / PZN_WAVE;
#pragma unroll
  for (int k = 0; k < JR_SUMS; ++k) acc[k] = wave_sum_f64(acc[k]);
  if (lane == 0)
#pragma unroll
    for (int k = 0; k < JR_SUMS; ++k) L.redd[JR_SUMS * wave + k] = acc[k];
  __syncthreads();
  if (tid == 0) {
    double m[JR_SUMS];
#pragma unroll
    for (int k = 0; k < JR_SUMS; ++k) {
      double v = L.redd[k];
#pragma unroll
      for (int w = 1; w < JR_W; ++w) v += L.redd[JR_SUMS * w + k];
      m[k] = v;
    }
    const double iw = 1.0 / m[0];
    const double xc[3] = {m[1] * iw, m[2] * iw, m[3] * iw}, yc[3] = {m[4] * iw, m[5] * iw, m[6] * iw};
    // centred: sum w (x - xc)(y - yc)^T = sum w x y^T - (sum w x)(sum w y)^T / sum w, and likewise the scatter of x
    const double S[3][3] = {{m[7] - m[1] * yc[0], m[8] - m[1] * yc[1], m[9] - m[1] * yc[2]},
                            {m[10] - m[2] * yc[0], m[11] - m[2] * yc[1], m[12] - m[2] * yc[2]},
                            {m[13] - m[3] * yc[0], m[14] - m[3] * yc[1], m[15] - m[3] * yc[2]}};
    const double C[6] = {m[16] - m[1] * xc[0], m[17] - m[2] * xc[1], m[18] - m[3] * xc[2],
                         m[19] - m[1] * xc[1], m[20] - m[1] * xc[2], m[21] - m[2] * xc[2]};
    const double px[3] = {(double)ref[0] + xc[0], (double)ref[1] + xc[1], (double)ref[2] + xc[2]};
    const double py[3] = {(double)ref[3] + yc[0], (double)ref[4] + yc[1], (double)ref[5] + yc[2]};
    solve_pose(S, C, cur, py, px, L.cand);
  }
  __syncthreads();
  return load_pose(L.cand);      // (cand is written next after the barriers of the evaluations that follow)
}

__device__ __forceinline__ bool joint_ok(int i, int j, int K) { return i >= 0 && j >= 0 && i < K && j < K && i != j; }

// Whether joint row `row` = (i, j) counts, and the sizes of its two sets.  COUNTS: na / nb of the row's sets (read by every
// thread from the same address: workgroup-uniform, and only for a row whose (i, j) is a joint, so the set maps of unused rows
// are never followed); a count outside [1, ka] or [1, kb] skips the row like a bad (i, j).
template <bool COUNTS>
__device__ __forceinline__ bool row_ok(const Sets& S, size_t row, int i, int j, int K, int& na, int& nb) {
  na = S.ka, nb = S.kb;
  if (!joint_ok(i, j, K)) return false;
  if (COUNTS) {
    if (S.na) na = S.na[S.a_of ? S.a_of[row] : (int64_t)row];
    if (S.nb) nb = S.nb[S.b_of ? S.b_of[row] : (int64_t)row];
    return na >= 1 && na <= S.ka && nb >= 1 && nb <= S.kb;
  }
  return true;
}

// The fp32 sum, in list order, of E_e over the joints of piece p (all joints: p < 0) with piece p under `gp`.  Thread 0 leaves
// every E_e in `out` (LDS): out[e] for a p < 0 pass (0 for a skipped row), out[t] for the t-th joint of piece p otherwise (NULL:
// nowhere); readers come after a barrier.  -> the number of joints met in `met`.
template <bool SUMS, bool COUNTS>
__device__ float eval_joints(const Lds& L, const Sets& S, const int32_t* __restrict__ jl, size_t row0, int J, int K, int p,
                             const Pose& gp, int tid, double (&acc)[JR_SUMS], float (&ref)[6], bool& have_ref, int& met,
                             float* out) {
  float E = 0.f;
  met = 0;
  for (int e = 0; e < J; ++e) {      // (workgroup-uniform: the list is the same for every thread)
    const int i = jl[2 * e], j = jl[2 * e + 1];
    int na, nb;
    const bool ok = row_ok<COUNTS>(S, row0 + e, i, j, K, na, nb);
    if (p < 0 && out && tid == 0 && !ok) out[e] = 0.f;
    if (!ok || (p >= 0 && i != p && j != p)) continue;
    const bool own_is_b = p < 0 || j == p;
    const Pose own = p < 0 ? load_pose(L.G + 12 * j) : gp;
    const Pose far = load_pose(L.G + 12 * (own_is_b ? i : j));
    const float ee = eval_joint<SUMS>(L, S, row0 + e, na, nb, own_is_b, own, far, tid, acc, ref, have_ref);
    if (out && tid == 0) out[p < 0 ? e : met] = ee;
    E = __fadd_rn(E, ee);
    ++met;
  }
  return E;
}

// The fp32 sum of L.js over all rows in list order (a skipped row holds 0, which changes no bit of a sum of energies), with
// the joints of piece p taken from L.jn instead (p < 0: none; the rows eval_joints met, by the same rule: row_ok and an end
// at p); commit: thread 0 moves those into L.js.
template <bool COUNTS>
__device__ float total_with(const Lds& L, const Sets& S, const int32_t* __restrict__ jl, size_t row0, int J, int K, int p,
                            bool commit, int tid) {
  float tot = 0.f;
  int t = 0;
  for (int e = 0; e < J; ++e) {
    const int i = jl[2 * e], j = jl[2 * e + 1];
    int na, nb;
    const bool mine = p >= 0 && (i == p || j == p) && row_ok<COUNTS>(S, row0 + e, i, j, K, na, nb);
    const float v = mine ? L.jn[t] : L.js[e];
    if (commit && mine && tid == 0) L.js[e] = v;
    t += mine ? 1 : 0;
    tot = __fadd_rn(tot, v);
  }
  return tot;
}

// The one body of both kernels below: COUNTS = false is joint_refine_kernel (na, nb are not looked at), true is
// joint_refine_counts_kernel.
template <bool COUNTS>
__device__ __forceinline__ void joint_refine_body(unsigned char* smem_raw, const float* __restrict__ a,
                                                  const int64_t* __restrict__ a_of, const int32_t* __restrict__ na,
                                                  const float* __restrict__ b, const int64_t* __restrict__ b_of,
                                                  const int32_t* __restrict__ nb, const int32_t* __restrict__ joints,
                                                  const float* __restrict__ G0, const uint8_t* __restrict__ movable, int Z, int K,
                                                  int J, int ka, int kb, int sweeps, float* __restrict__ G,
                                                  float* __restrict__ score, float* __restrict__ score0,
                                                  float* __restrict__ joint_score, int32_t* __restrict__ sweeps_used,
                                                  int32_t* __restrict__ accepted) {
  const int kmax = ((ka > kb ? ka : kb) + 3) & ~3;      // the stride of the images: a multiple of four floats
  Lds L;
  L.redd = reinterpret_cast<double*>(smem_raw);                       // [JR_W][JR_SUMS]
  L.rede = reinterpret_cast<float*>(L.redd + JR_W * JR_SUMS);         // [JR_W][2]
  L.cand = L.rede + JR_W * 2;                                         // [12]
  L.G = L.cand + 12;                                                  // [K][12]
  L.fx = L.G + 12 * K, L.fy = L.fx + kmax, L.fz = L.fy + kmax;
  L.ox = L.fz + kmax, L.oy = L.ox + kmax, L.oz = L.oy + kmax;
  L.tx = L.oz + kmax, L.ty = L.tx + kmax, L.tz = L.ty + kmax;
  L.taken = reinterpret_cast<int*>(L.tz + kmax);                      // [K]
  L.js = reinterpret_cast<float*>(L.taken + K);                       // [J]
  L.jn = L.js + J;                                                    // [2 K]
  const int tid = (int)threadIdx.x;
  const Sets S = {a, a_of, b, b_of, ka, kb, na, nb};

  for (int z = (int)blockIdx.x; z < Z; z += (int)gridDim.x) {      // (workgroup-uniform)
    const int32_t* jl = joints + (size_t)z * J * 2;
    const uint8_t* mv = movable + (size_t)z * K;
    const size_t row0 = (size_t)z * J;
    for (int i = tid; i < 12 * K; i += JR_T) {
      const int p = i / 12, k = i - 12 * p;
      const float* g0 = G0 + ((size_t)z * K + p) * 16;
      L.G[i] = k < 9 ? g0[4 * (k / 3) + (k % 3)] : g0[4 * (k - 9) + 3];
    }
    for (int i = tid; i < K; i += JR_T) L.taken[i] = 0;
    __syncthreads();

    double acc[JR_SUMS];
    float ref[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    bool have_ref = true;
    int met;
    const Pose none = load_pose(L.G);
    eval_joints<false, COUNTS>(L, S, jl, row0, J, K, -1, none, tid, acc, ref, have_ref, met, L.js);
    __syncthreads();
    const float e0 = total_with<COUNTS>(L, S, jl, row0, J, K, -1, false, tid);
    float e = e0;      // E under the current poses: the sum of L.js, the same bits in every thread
    int used = 0;
    for (int sw = 0; sw < sweeps; ++sw) {
      bool any = false;
      for (int p = 0; p < K; ++p) {
        if (!mv[p]) continue;
        const Pose cur = load_pose(L.G + 12 * p);
#pragma unroll
        for (int k = 0; k < JR_SUMS; ++k) acc[k] = 0.0;
        have_ref = false;
        const float ep = eval_joints<true, COUNTS>(L, S, jl, row0, J, K, p, cur, tid, acc, ref, have_ref, met, nullptr);
        if (met == 0 || met > 2 * K) continue;      // (more than 2 (K - 1) rows only where the list repeats a pair: L.jn holds 2 K)
        const Pose nxt = candidate(L, cur, acc, ref, tid);
        const float en = eval_joints<false, COUNTS>(L, S, jl, row0, J, K, p, nxt, tid, acc, ref, have_ref, met, L.jn);
        if (!(en < ep)) continue;      // (the same bits in every thread)
        __syncthreads();               // L.jn is written
        // E_p fell, so E falls - in exact arithmetic.  The fp32 sum over all rows is held to it too: a candidate whose
        // total would round ABOVE the current one is left (a last-place matter: score <= score0 holds to the bit)
        const float et = total_with<COUNTS>(L, S, jl, row0, J, K, p, false, tid);
        if (!(et <= e)) continue;
        __syncthreads();               // every thread has read L.js
        total_with<COUNTS>(L, S, jl, row0, J, K, p, true, tid);
        if (tid < 12) L.G[12 * p + tid] = L.cand[tid];
        if (tid == 0) L.taken[p] += 1;
        e = et;
        any = true;
        __syncthreads();
      }
      if (!any) break;
      ++used;
    }
    for (int i = tid; i < J; i += JR_T) joint_score[row0 + i] = L.js[i];
    for (int i = tid; i < 16 * K; i += JR_T) {
      const int p = i >> 4, u = (i >> 2) & 3, v = i & 3;
      const float val = u < 3 ? (v < 3 ? L.G[12 * p + 3 * u + v] : L.G[12 * p + 9 + u]) : (v == 3 ? 1.f : 0.f);
      G[((size_t)z * K + p) * 16 + (i & 15)] = val;
    }
    for (int i = tid; i < K; i += JR_T) accepted[(size_t)z * K + i] = L.taken[i];
    if (tid == 0) score[z] = e, score0[z] = e0, sweeps_used[z] = used;
    __syncthreads();      // the LDS image is replaced by the next puzzle's
  }
}

__global__ __launch_bounds__(JR_T) void joint_refine_kernel(const float* __restrict__ a, const int64_t* __restrict__ a_of,
                                                            const float* __restrict__ b, const int64_t* __restrict__ b_of,
                                                            const int32_t* __restrict__ joints, const float* __restrict__ G0,
                                                            const uint8_t* __restrict__ movable, int Z, int K, int J, int ka,
                                                            int kb, int sweeps, float* __restrict__ G, float* __restrict__ score,
                                                            float* __restrict__ score0, float* __restrict__ joint_score,
                                                            int32_t* __restrict__ sweeps_used, int32_t* __restrict__ accepted) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  joint_refine_body<false>(smem_raw, a, a_of, nullptr, b, b_of, nullptr, joints, G0, movable, Z, K, J, ka, kb, sweeps, G, score,
                           score0, joint_score, sweeps_used, accepted);
}

__global__ __launch_bounds__(JR_T) void joint_refine_counts_kernel(
    const float* __restrict__ a, const int64_t* __restrict__ a_of, const int32_t* __restrict__ na, const float* __restrict__ b,
    const int64_t* __restrict__ b_of, const int32_t* __restrict__ nb, const int32_t* __restrict__ joints,
    const float* __restrict__ G0, const uint8_t* __restrict__ movable, int Z, int K, int J, int ka, int kb, int sweeps,
    float* __restrict__ G, float* __restrict__ score, float* __restrict__ score0, float* __restrict__ joint_score,
    int32_t* __restrict__ sweeps_used, int32_t* __restrict__ accepted) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  joint_refine_body<true>(smem_raw, a, a_of, na, b, b_of, nb, joints, G0, movable, Z, K, J, ka, kb, sweeps, G, score, score0,
                          joint_score, sweeps_used, accepted);
}

}  // namespace

PZN_EXPORT int pzn_joint_refine_supported(int K, int J, int ka, int kb) {
  return K >= 1 && K <= JR_MAX_PIECES && J >= 0 && J <= K * (K - 1) && ka >= 1 && kb >= 1 && ka <= JR_MAX_K && kb <= JR_MAX_K;
}

namespace {

// na = nb = NULL launches joint_refine_kernel, anything else joint_refine_counts_kernel.
int joint_refine_launch(const float* a, const int64_t* a_of, const int32_t* na, const float* b, const int64_t* b_of,
                        const int32_t* nb, const int32_t* joints, const float* G0, const uint8_t* movable, int Z, int K, int J,
                        int ka, int kb, int sweeps, float* G, float* score, float* score0, float* joint_score,
                        int32_t* sweeps_used, int32_t* accepted, pzn_stream_t stream) {
  if (!pzn_joint_refine_supported(K, J, ka, kb) || sweeps < 0) return PZN_EUNSUPPORTED;
  PZN_CHECK_ARG(Z >= 0);
  if (Z == 0 || J == 0) return PZN_OK;
  PZN_CHECK_ARG(a && b && joints && G0 && movable && G && score && score0 && joint_score && sweeps_used && accepted);
  hipStream_t st = pzn_hip_stream(stream);
  const size_t kmax = ((size_t)(ka > kb ? ka : kb) + 3) & ~(size_t)3;
  const size_t lds = JR_W * JR_SUMS * sizeof(double) + (JR_W * 2 + 12 + 12 * (size_t)K + 9 * kmax) * sizeof(float) +
                     (size_t)K * sizeof(int) + ((size_t)J + 2 * (size_t)K) * sizeof(float);
  const int grid = Z < JR_MAX_GRID ? Z : JR_MAX_GRID;
  if (!na && !nb)
    PZN_LAUNCH(joint_refine_kernel, dim3(grid), dim3(JR_T), lds, st, a, a_of, b, b_of, joints, G0, movable, Z, K, J, ka, kb,
               sweeps, G, score, score0, joint_score, sweeps_used, accepted);
  else
    PZN_LAUNCH(joint_refine_counts_kernel, dim3(grid), dim3(JR_T), lds, st, a, a_of, na, b, b_of, nb, joints, G0, movable, Z, K,
               J, ka, kb, sweeps, G, score, score0, joint_score, sweeps_used, accepted);
  PZN_RETURN_LAUNCH_STATUS();
}

}  // namespace

PZN_EXPORT int pzn_joint_refine_f32(const float* a, const int64_t* a_of, const float* b, const int64_t* b_of,
                                    const int32_t* joints, const float* G0, const uint8_t* movable, int Z, int K, int J, int ka,
                                    int kb, int sweeps, float* G, float* score, float* score0, float* joint_score,
                                    int32_t* sweeps_used, int32_t* accepted, pzn_stream_t stream) {
  return joint_refine_launch(a, a_of, nullptr, b, b_of, nullptr, joints, G0, movable, Z, K, J, ka, kb, sweeps, G, score, score0,
                             joint_score, sweeps_used, accepted, stream);
}

// With both counts NULL this is the launch above: the same kernel, so the same bits.
PZN_EXPORT int pzn_joint_refine_counts_f32(const float* a, const int64_t* a_of, const int32_t* na, const float* b,
                                           const int64_t* b_of, const int32_t* nb, const int32_t* joints, const float* G0,
                                           const uint8_t* movable, int Z, int K, int J, int ka, int kb, int sweeps, float* G,
                                           float* score, float* score0, float* joint_score, int32_t* sweeps_used,
                                           int32_t* accepted, pzn_stream_t stream) {
  return joint_refine_launch(a, a_of, na, b, b_of, nb, joints, G0, movable, Z, K, J, ka, kb, sweeps, G, score, score0,
                             joint_score, sweeps_used, accepted, stream);
}
