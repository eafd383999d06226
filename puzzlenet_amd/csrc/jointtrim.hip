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
#include "pzn_rigid.h"

namespace {

constexpr int JT_T = 256;                  // four wavefronts
constexpr int JT_W = JT_T / PZN_WAVE;
constexpr int JT_MAX_K = 1024;             // points per side
constexpr int JT_MAX_PIECES = 64;
constexpr int JT_MAX_GRID = 512;           // two workgroups per CU of a 256-CU part; more puzzles share a workgroup in turn
constexpr int JT_SUMS = 22;                // w, wx[3], wy[3], wxy[9], wxx[6]

struct Lds {
  float *fx, *fy, *fz;      // far side's root-frame image, [kmax]
  float *ox, *oy, *oz;      // own side as given, [kmax]
  float *tx, *ty, *tz;      // own side under the pose being tried, [kmax]
  float* G;                 // [K][12] the poses: r[9], t[3]
  double* redd;             // [JT_W][JT_SUMS] wave partials of the float64 sums
  float* rede;              // [JT_W][2] wave partials of the two objective sums
  float* cand;              // [12] the candidate pose, thread 0 -> everyone
  int* taken;               // [K] accepted visits
  float* js;                // [J] E_e of every row under the current poses (0 for a skipped row)
  float* jn;                // [2 K] E_e of the visited piece's joints under the candidate
  float* rmin;              // [ka + kb] every row's minimum of the joint being evaluated
  unsigned short* arg;      // [ka + kb] every row's arg-min (the last pass: 1 = kept)
};

struct Sets {
  const float* a;
  const int64_t* a_of;
  const float* b;
  const int64_t* b_of;
  int ka, kb;
  const int32_t *ma, *mb;       // rows kept of A / of B, indexed by the joint ROW (NULL: ka / kb everywhere)
  int32_t *kept_a, *kept_b;     // [Z J, ka], [Z J, kb] or NULL
};

__device__ __forceinline__ Pose load_pose(const float* g) {
  Pose p;
#pragma unroll
  for (int k = 0; k < 9; ++k) p.r[k] = g[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) p.t[k] = g[9 + k];
  return p;
}

// E_e of joint row `row` with `own_is_b ? B : A` as the own side under `own` and the other side under `far`, of which ma of the
// ka rows of A and mb of the kb rows of B are kept (1 <= ma <= ka, 1 <= mb <= kb, the same values in every thread).  SUMS: every
// kept row adds its pair to acc (shifted by ref, which the first call of a visit sets: have_ref).  KEPT: the kept rows leave
// in S.kept_a / S.kept_b.  Four barriers; on entry no thread may still be reading the images, rmin, arg or rede (every caller
// comes from a barrier).
template <bool SUMS, bool KEPT>
__device__ float eval_joint(const Lds& L, const Sets& S, size_t row, int ma, int mb, bool own_is_b, const Pose& own,
                            const Pose& far, int tid, double (&acc)[JT_SUMS], float (&ref)[6], bool& have_ref) {
  const int ka = S.ka, kb = S.kb;
  const float* ga = S.a + (size_t)(S.a_of ? S.a_of[row] : (int64_t)row) * ka * 3;
  const float* gb = S.b + (size_t)(S.b_of ? S.b_of[row] : (int64_t)row) * kb * 3;
  const float* gown = own_is_b ? gb : ga;
  const float* gfar = own_is_b ? ga : gb;
  const int kown = own_is_b ? kb : ka, kfar = own_is_b ? ka : kb;
  for (int q = tid; q < kown; q += JT_T) {
    const float x = gown[3 * q], y = gown[3 * q + 1], z = gown[3 * q + 2];
    L.ox[q] = x, L.oy[q] = y, L.oz[q] = z;
    pose_move(own, x, y, z, L.tx[q], L.ty[q], L.tz[q]);
  }
  for (int q = tid; q < kfar; q += JT_T) pose_move(far, gfar[3 * q], gfar[3 * q + 1], gfar[3 * q + 2], L.fx[q], L.fy[q], L.fz[q]);
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
  const int rows = ka + kb;
  for (int r = tid; r < rows; r += JT_T) {
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
    // one form of the distance serves both directions; candidates in index order with a strict <: the lowest index of equal
    // distances stays.  Four candidates per 16-byte LDS read (the images start on 16-byte boundaries), the rest one by one.
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
    L.rmin[r] = best;
    L.arg[r] = (unsigned short)arg;
  }
  __syncthreads();      // every row's minimum and arg-min stand in LDS
  const double wa = 1.0 / (double)ma, wb = 1.0 / (double)mb;
  float s1 = 0.f, s2 = 0.f;
  for (int r = tid; r < rows; r += JT_T) {      // the second pass over the thread's own rows: rank, then sum what is kept
    const bool a_row = r < ka;
    const int me = a_row ? r : r - ka;
    const float* v = a_row ? L.rmin : L.rmin + ka;
    const int n = a_row ? ka : kb;
    const float mine = v[me];      // (never NaN: a NaN distance never passes d < best)
    int before = 0;
    for (int c = 0; c < n; ++c) {      // one address for the whole wave: a broadcast read
      const float o = v[c];
      before += (o < mine || (o == mine && c < me)) ? 1 : 0;
    }
    const bool kept = before < (a_row ? ma : mb);
    if (kept) {
      if (a_row)
        s1 = __fadd_rn(s1, mine);
      else
        s2 = __fadd_rn(s2, mine);
      if (SUMS) {
        const int arg = (int)L.arg[r];
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
    if (KEPT) L.arg[r] = kept ? 1 : 0;      // (a row writes its own slot only, and no pass with KEPT reads the arg-mins)
  }
  float e1, e2;
  block_sum2_f32<JT_W>(L.rede, tid, s1, s2, e1, e2);      // (its barrier: every kept flag is written)
  const float e = __fadd_rn(__fdiv_rn(e1, (float)ma), __fdiv_rn(e2, (float)mb));
  if (KEPT) {
    for (int r = tid; r < rows; r += JT_T) {
      const bool a_row = r < ka;
      const int me = a_row ? r : r - ka;
      int32_t* out = a_row ? S.kept_a : S.kept_b;
      if (!out) continue;
      out += row * (size_t)(a_row ? ka : kb);
      const int m = a_row ? ma : mb;
      const unsigned short* f = a_row ? L.arg : L.arg + ka;
      if (f[me]) {
        int pos = 0;
        for (int c = 0; c < me; ++c) pos += f[c];
        out[pos] = me;      // pos < m: exactly m rows of a direction are kept
      }
      if (me >= m) out[me] = -1;      // the k - m slots behind the count, one per row
    }
  }
  __syncthreads();      // rede, rmin, arg and the images are free again
  return e;
}

// The candidate pose of a visit from its 22 sums (every thread's acc) and the current pose (its rotation is kept when the
// scatter of x is degenerate).  Two barriers; the result is in L.cand and in every thread's registers.
__device__ Pose candidate(const Lds& L, const Pose& cur, double (&acc)[JT_SUMS], const float (&ref)[6], int tid) {
  const int lane = tid & (PZN_WAVE - 1), wave = tid / PZN_WAVE;
#pragma unroll
  for (int k = 0; k < JT_SUMS; ++k) acc[k] = wave_sum_f64(acc[k]);
  if (lane == 0)
#pragma unroll
    for (int k = 0; k < JT_SUMS; ++k) L.redd[JT_SUMS * wave + k] = acc[k];
  __syncthreads();
  if (tid == 0) {
    double m[JT_SUMS];
#pragma unroll
    for (int k = 0; k < JT_SUMS; ++k) {
      double v = L.redd[k];
#pragma unroll
      for (int w = 1; w < JT_W; ++w) v += L.redd[JT_SUMS * w + k];
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

// Whether joint row `row` = (i, j) counts, and how many rows of its two sets are kept: ma / mb of the row (read by every thread
// from the same address: workgroup-uniform, and only for a row whose (i, j) is a joint); a count outside [1, ka] or [1, kb]
// skips the row like a bad (i, j).
__device__ __forceinline__ bool row_ok(const Sets& S, size_t row, int i, int j, int K, int& ma, int& mb) {
  ma = S.ka, mb = S.kb;
  if (!joint_ok(i, j, K)) return false;
  if (S.ma) ma = S.ma[row];
  if (S.mb) mb = S.mb[row];
  return ma >= 1 && ma <= S.ka && mb >= 1 && mb <= S.kb;
}

// The fp32 sum, in list order, of E_e over the joints of piece p (all joints: p < 0) with piece p under `gp`.  Thread 0 leaves
// every E_e in `out` (LDS): out[e] for a p < 0 pass (0 for a skipped row), out[t] for the t-th joint of piece p otherwise (NULL:
// nowhere); readers come after a barrier.  -> the number of joints met in `met`.  KEPT (a p < 0 pass): the kept rows of every
// row leave in S.kept_a / S.kept_b, -1 throughout for a skipped row.
template <bool SUMS, bool KEPT>
__device__ float eval_joints(const Lds& L, const Sets& S, const int32_t* __restrict__ jl, size_t row0, int J, int K, int p,
                             const Pose& gp, int tid, double (&acc)[JT_SUMS], float (&ref)[6], bool& have_ref, int& met,
                             float* out) {
  float E = 0.f;
  met = 0;
  for (int e = 0; e < J; ++e) {      // (workgroup-uniform: the list is the same for every thread)
    const int i = jl[2 * e], j = jl[2 * e + 1];
    int ma, mb;
    const bool ok = row_ok(S, row0 + e, i, j, K, ma, mb);
    if (p < 0 && out && tid == 0 && !ok) out[e] = 0.f;
    if (KEPT && !ok) {
      if (S.kept_a)
        for (int q = tid; q < S.ka; q += JT_T) S.kept_a[(row0 + e) * (size_t)S.ka + q] = -1;
      if (S.kept_b)
        for (int q = tid; q < S.kb; q += JT_T) S.kept_b[(row0 + e) * (size_t)S.kb + q] = -1;
    }
    if (!ok || (p >= 0 && i != p && j != p)) continue;
    const bool own_is_b = p < 0 || j == p;
    const Pose own = p < 0 ? load_pose(L.G + 12 * j) : gp;
    const Pose far = load_pose(L.G + 12 * (own_is_b ? i : j));
    const float ee = eval_joint<SUMS, KEPT>(L, S, row0 + e, ma, mb, own_is_b, own, far, tid, acc, ref, have_ref);
    if (out && tid == 0) out[p < 0 ? e : met] = ee;
    E = __fadd_rn(E, ee);
    ++met;
  }
  return E;
}

// The fp32 sum of L.js over all rows in list order (a skipped row holds 0, which changes no bit of a sum of energies), with
// the joints of piece p taken from L.jn instead (p < 0: none; the rows eval_joints met, by the same rule: row_ok and an end
// at p); commit: thread 0 moves those into L.js.
__device__ float total_with(const Lds& L, const Sets& S, const int32_t* __restrict__ jl, size_t row0, int J, int K, int p,
                            bool commit, int tid) {
  float tot = 0.f;
  int t = 0;
  for (int e = 0; e < J; ++e) {
    const int i = jl[2 * e], j = jl[2 * e + 1];
    int ma, mb;
    const bool mine = p >= 0 && (i == p || j == p) && row_ok(S, row0 + e, i, j, K, ma, mb);
    const float v = mine ? L.jn[t] : L.js[e];
    if (commit && mine && tid == 0) L.js[e] = v;
    t += mine ? 1 : 0;
    tot = __fadd_rn(tot, v);
  }
  return tot;
}

__global__ __launch_bounds__(JT_T) void joint_trim_kernel(
    const float* __restrict__ a, const int64_t* __restrict__ a_of, const int32_t* __restrict__ ma, const float* __restrict__ b,
    const int64_t* __restrict__ b_of, const int32_t* __restrict__ mb, const int32_t* __restrict__ joints,
    const float* __restrict__ G0, const uint8_t* __restrict__ movable, int Z, int K, int J, int ka, int kb, int sweeps,
    float* __restrict__ G, float* __restrict__ score, float* __restrict__ score0, float* __restrict__ joint_score,
    int32_t* __restrict__ sweeps_used, int32_t* __restrict__ accepted, int32_t* __restrict__ kept_a,
    int32_t* __restrict__ kept_b) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int kmax = ((ka > kb ? ka : kb) + 3) & ~3;      // the stride of the images: a multiple of four floats
  Lds L;
  L.redd = reinterpret_cast<double*>(smem_raw);                       // [JT_W][JT_SUMS]
  L.rede = reinterpret_cast<float*>(L.redd + JT_W * JT_SUMS);         // [JT_W][2]
  L.cand = L.rede + JT_W * 2;                                         // [12]
  L.G = L.cand + 12;                                                  // [K][12]
  L.fx = L.G + 12 * K, L.fy = L.fx + kmax, L.fz = L.fy + kmax;
  L.ox = L.fz + kmax, L.oy = L.ox + kmax, L.oz = L.oy + kmax;
  L.tx = L.oz + kmax, L.ty = L.tx + kmax, L.tz = L.ty + kmax;
  L.taken = reinterpret_cast<int*>(L.tz + kmax);                      // [K]
  L.js = reinterpret_cast<float*>(L.taken + K);                       // [J]
  L.jn = L.js + J;                                                    // [2 K]
  L.rmin = L.jn + 2 * K;                                              // [ka + kb]
  L.arg = reinterpret_cast<unsigned short*>(L.rmin + ka + kb);        // [ka + kb]
  const int tid = (int)threadIdx.x;
  const Sets S = {a, a_of, b, b_of, ka, kb, ma, mb, kept_a, kept_b};

  for (int z = (int)blockIdx.x; z < Z; z += (int)gridDim.x) {      // (workgroup-uniform)
    const int32_t* jl = joints + (size_t)z * J * 2;
    const uint8_t* mv = movable + (size_t)z * K;
    const size_t row0 = (size_t)z * J;
    for (int i = tid; i < 12 * K; i += JT_T) {
      const int p = i / 12, k = i - 12 * p;
      const float* g0 = G0 + ((size_t)z * K + p) * 16;
      L.G[i] = k < 9 ? g0[4 * (k / 3) + (k % 3)] : g0[4 * (k - 9) + 3];
    }
    for (int i = tid; i < K; i += JT_T) L.taken[i] = 0;
    __syncthreads();

    double acc[JT_SUMS];
    float ref[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    bool have_ref = true;
    int met;
    const Pose none = load_pose(L.G);
    eval_joints<false, false>(L, S, jl, row0, J, K, -1, none, tid, acc, ref, have_ref, met, L.js);
    __syncthreads();
    const float e0 = total_with(L, S, jl, row0, J, K, -1, false, tid);
    float e = e0;      // E under the current poses: the sum of L.js, the same bits in every thread
    int used = 0;
    for (int sw = 0; sw < sweeps; ++sw) {
      bool any = false;
      for (int p = 0; p < K; ++p) {
        if (!mv[p]) continue;
        const Pose cur = load_pose(L.G + 12 * p);
#pragma unroll
        for (int k = 0; k < JT_SUMS; ++k) acc[k] = 0.0;
        have_ref = false;
        const float ep = eval_joints<true, false>(L, S, jl, row0, J, K, p, cur, tid, acc, ref, have_ref, met, nullptr);
        if (met == 0 || met > 2 * K) continue;      // (more than 2 (K - 1) rows only where the list repeats a pair: L.jn holds 2 K)
        const Pose nxt = candidate(L, cur, acc, ref, tid);
        const float en = eval_joints<false, false>(L, S, jl, row0, J, K, p, nxt, tid, acc, ref, have_ref, met, L.jn);
        if (!(en < ep)) continue;      // (the same bits in every thread)
        __syncthreads();               // L.jn is written
        // the fp32 sum over all rows is held to the fall of E_p too: a candidate whose total would round ABOVE the current one
        // is left (a last-place matter: score <= score0 holds to the bit)
        const float et = total_with(L, S, jl, row0, J, K, p, false, tid);
        if (!(et <= e)) continue;
        __syncthreads();               // every thread has read L.js
        total_with(L, S, jl, row0, J, K, p, true, tid);
        if (tid < 12) L.G[12 * p + tid] = L.cand[tid];
        if (tid == 0) L.taken[p] += 1;
        e = et;
        any = true;
        __syncthreads();
      }
      if (!any) break;
      ++used;
    }
    for (int i = tid; i < J; i += JT_T) joint_score[row0 + i] = L.js[i];
    for (int i = tid; i < 16 * K; i += JT_T) {
      const int p = i >> 4, u = (i >> 2) & 3, v = i & 3;
      const float val = u < 3 ? (v < 3 ? L.G[12 * p + 3 * u + v] : L.G[12 * p + 9 + u]) : (v == 3 ? 1.f : 0.f);
      G[((size_t)z * K + p) * 16 + (i & 15)] = val;
    }
    for (int i = tid; i < K; i += JT_T) accepted[(size_t)z * K + i] = L.taken[i];
    if (tid == 0) score[z] = e, score0[z] = e0, sweeps_used[z] = used;
    // the rows kept under the returned poses (a kernel argument: workgroup-uniform); the energies it finds are those in L.js
    if (kept_a || kept_b) eval_joints<false, true>(L, S, jl, row0, J, K, -1, none, tid, acc, ref, have_ref, met, nullptr);
    __syncthreads();      // the LDS image is replaced by the next puzzle's
  }
}

size_t joint_trim_lds(int K, int J, int ka, int kb) {
  const size_t kmax = ((size_t)(ka > kb ? ka : kb) + 3) & ~(size_t)3;
  return JT_W * JT_SUMS * sizeof(double) + (JT_W * 2 + 12 + 12 * (size_t)K + 9 * kmax) * sizeof(float) + (size_t)K * sizeof(int) +
         ((size_t)J + 2 * (size_t)K) * sizeof(float) + ((size_t)ka + (size_t)kb) * (sizeof(float) + sizeof(unsigned short));
}

}  // namespace

// The sibling's range: the 68.3 KB of LDS at its upper end are allowed by attribute at the launch.
PZN_EXPORT int pzn_joint_refine_trim_supported(int K, int J, int ka, int kb) {
  return K >= 1 && K <= JT_MAX_PIECES && J >= 0 && J <= K * (K - 1) && ka >= 1 && kb >= 1 && ka <= JT_MAX_K && kb <= JT_MAX_K;
}

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
  const size_t lds = joint_trim_lds(K, J, ka, kb);
  if (lds > 64 * 1024 && hipFuncSetAttribute(reinterpret_cast<const void*>(joint_trim_kernel),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return PZN_ELAUNCH;
  const int grid = Z < JT_MAX_GRID ? Z : JT_MAX_GRID;
  PZN_LAUNCH(joint_trim_kernel, dim3(grid), dim3(JT_T), lds, st, a, a_of, ma, b, b_of, mb, joints, G0, movable, Z, K, J, ka, kb,
             sweeps, G, score, score0, joint_score, sweeps_used, accepted, kept_a, kept_b);
  PZN_RETURN_LAUNCH_STATUS();
}
