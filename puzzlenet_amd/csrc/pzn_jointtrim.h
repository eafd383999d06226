// pzn_jointtrim.h — the one body of the joint refinements that choose the kept rows of every joint again under the joint poses:
// joint_trim_kernel (jointtrim.hip: two counts per joint row, given) is the AUTO = false instantiation and joint_auto_kernel
// (jointauto.hip: the counts found at every evaluation of a joint) the AUTO = true one.  What the body does, its LDS image and
// what it duplicates from jointrefine.hip are stated at the head of jointtrim.hip; what AUTO adds, at the head of jointauto.hip.
// Every addition of the auto form stands under `if constexpr (AUTO)`, so joint_trim_kernel computes what it computed before.
#ifndef PZN_JOINTTRIM_H_
#define PZN_JOINTTRIM_H_

#include "pzn_rigid.h"

namespace {

constexpr int JT_T = 256;                  // four wavefronts
constexpr int JT_W = JT_T / PZN_WAVE;
constexpr int JT_MAX_K = 1024;             // points per side
constexpr int JT_SLOTS = 2 * JT_MAX_K / JT_T;      // rows a thread owns at most (auto: their ranks stay in registers)
constexpr int JT_MAX_PIECES = 64;
constexpr int JT_MAX_GRID = 512;           // two workgroups per CU of a 256-CU part; more puzzles share a workgroup in turn
constexpr int JT_SUMS = 22;                // w, wx[3], wy[3], wxy[9], wxx[6]

struct Lds {
  float *fx, *fy, *fz;      // far side's root-frame image, [kmax]
  float *ox, *oy, *oz;      // own side as given, [kmax]
  float *tx, *ty, *tz;      // own side under the pose being tried, [kmax]
  float* G;                 // [K][12] the poses: r[9], t[3]
  double* redd;             // [JT_W][JT_SUMS] wave partials of the float64 sums (auto: the waves' best (phi, m) too)
  float* rede;              // [JT_W][2] wave partials of the two objective sums (auto: the waves' totals of the scan too)
  float* cand;              // [12] the candidate pose, thread 0 -> everyone
  int* taken;               // [K] accepted visits
  float* js;                // [J] E_e (auto: F_e) of every row under the current poses (0 for a skipped row)
  float* jn;                // [2 K] E_e (auto: F_e) of the visited piece's joints under the candidate
  float* rmin;              // [ka + kb] every row's minimum of the joint being evaluated
  float* sorted;            // auto only: [ka + kb] every direction's row minima in (value, index) order
  unsigned short* arg;      // [ka + kb] every row's arg-min (the last pass: 1 = kept)
};

struct Sets {
  const float* a;
  const int64_t* a_of;
  const float* b;
  const int64_t* b_of;
  int ka, kb;
  const int32_t *ma, *mb;       // rows kept of A / of B, indexed by the joint ROW (NULL: ka / kb everywhere); not read by the auto form
  int32_t *kept_a, *kept_b;     // [Z J, ka], [Z J, kb] or NULL
  // the auto form only
  int lo_a, lo_b, power;        // the least counts and p of phi(m) = S_m / m^(p+1)
  int32_t *count_a, *count_b;   // [Z J] the counts under the returned poses
  float* joint_score;           // [Z J] E_e under the returned poses (the last pass writes it: L.js holds F_e)
};

__device__ __forceinline__ Pose load_pose(const float* g) {
  Pose p;
#pragma unroll
  for (int k = 0; k < 9; ++k) p.r[k] = g[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) p.t[k] = g[9 + k];
  return p;
}

// (phi, m) before (ophi, om) in the arg-min's order: the smaller phi, among equal phi the larger m
__device__ __forceinline__ bool jt_phi_before(double phi, int m, double ophi, int om) { return phi < ophi || (phi == ophi && m > om); }

// Steps 2 and 3 of the auto rule (include/pzn.h, above pzn_icp_refine_auto_f32) for both directions at once: L.sorted holds the
// ka minima of A and behind them the kb minima of B, each in (value, index) order (the caller's barrier stands behind the
// scatter); ma, mb come in as the least counts and leave as the counts, the same values in every thread.  Thread t adds the
// sorted values 4t .. 4t+3 one after the other, the wave scans the thread totals (Hillis-Steele), the wave totals go through
// L.rede and are added in wave order; phi(m) = (double)S_m / m^(p+1) for the thread's own four m; the lexicographic arg-min of
// (phi, larger m) is a butterfly and one slot pair of L.redd per wave and direction.  Two barriers; the caller's next barrier
// frees rede and redd.  Duplicated from icprefine.hip's evaluate<TRIM, AUTO> (DESIGN section 3 lists it for the later fold).
__device__ __forceinline__ void find_counts(const Lds& L, int ka, int kb, int power, int tid, int& ma, int& mb) {
  const int lane = tid & (PZN_WAVE - 1), wave = tid / PZN_WAVE;
  float c[2][4], exc[2];
#pragma unroll
  for (int d = 0; d < 2; ++d) {
    const float* w = d ? L.sorted + ka : L.sorted;
    const int n = d ? kb : ka;
    float run = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int at = 4 * tid + i;
      run = __fadd_rn(run, at < n ? w[at] : 0.f);
      c[d][i] = run;
    }
    float inc = run;
#pragma unroll
    for (int step = 1; step < PZN_WAVE; step *= 2) {
      const float o = __shfl_up(inc, step, PZN_WAVE);
      inc = lane >= step ? __fadd_rn(inc, o) : inc;
    }
    const float up = __shfl_up(inc, 1, PZN_WAVE);
    exc[d] = lane == 0 ? 0.f : up;
    if (lane == PZN_WAVE - 1) L.rede[2 * wave + d] = inc;
  }
  __syncthreads();      // the wave totals
  double bphi[2];
  int bm[2];
#pragma unroll
  for (int d = 0; d < 2; ++d) {
    const int n = d ? kb : ka, lo = d ? mb : ma;
    float off = 0.f;
#pragma unroll
    for (int w = 0; w < JT_W - 1; ++w) off = w < wave ? __fadd_rn(off, L.rede[2 * w + d]) : off;
    const float base = __fadd_rn(off, exc[d]);
    bphi[d] = (double)__builtin_inff(), bm[d] = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int m = 4 * tid + i + 1;
      const double dm = (double)m;
      double q = dm;
      for (int j = 0; j < power; ++j) q *= dm;      // m^(p+1), exact: m <= 1024, p + 1 <= 5
      const double phi = (double)__fadd_rn(base, c[d][i]) / q;
      const bool take = m >= lo && m <= n && jt_phi_before(phi, m, bphi[d], bm[d]);
      bphi[d] = take ? phi : bphi[d], bm[d] = take ? m : bm[d];
    }
#define JT_PHI_STEP(J)                                                                                          \
  {                                                                                                             \
    const double ophi = __longlong_as_double((long long)pzn::xor_lane_u64<J>((uint64_t)__double_as_longlong(bphi[d]))); \
    const int om = (int)pzn::xor_lane<J>((uint32_t)bm[d]);                                                      \
    const bool take = jt_phi_before(ophi, om, bphi[d], bm[d]);                                                  \
    bphi[d] = take ? ophi : bphi[d], bm[d] = take ? om : bm[d];                                                 \
  }
    JT_PHI_STEP(1) JT_PHI_STEP(2) JT_PHI_STEP(4) JT_PHI_STEP(8) JT_PHI_STEP(16) JT_PHI_STEP(32)
#undef JT_PHI_STEP
    if (lane == 0) L.redd[JT_SUMS * wave + 2 * d] = bphi[d], L.redd[JT_SUMS * wave + 2 * d + 1] = (double)bm[d];
  }
  __syncthreads();      // the four waves' best (phi, m) of both directions
#pragma unroll
  for (int d = 0; d < 2; ++d) {
    double phi = L.redd[2 * d];
    int m = (int)L.redd[2 * d + 1];
#pragma unroll
    for (int w = 1; w < JT_W; ++w) {
      const double ophi = L.redd[JT_SUMS * w + 2 * d];
      const int om = (int)L.redd[JT_SUMS * w + 2 * d + 1];
      const bool take = jt_phi_before(ophi, om, phi, m);
      phi = take ? ophi : phi, m = take ? om : m;
    }
    (d ? mb : ma) = m;      // in [lo, n]: the same value in every thread
  }
}

// The pair of a kept row enters the 22 float64 sums of a visit with weight w.
__device__ __forceinline__ void add_pair(const Lds& L, int r, bool a_row, int me, bool own_is_b, double w, const float (&ref)[6],
                                         double (&acc)[JT_SUMS]) {
  const int arg = (int)L.arg[r];
  const int ia = a_row ? me : arg, ib = a_row ? arg : me;      // the pair (a_ia, b_ib)
  const int io = own_is_b ? ib : ia, ifar = own_is_b ? ia : ib;
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

// What an evaluation of a joint by the auto form leaves beside its return value F_e.
struct AutoJoint {
  float E;        // e_a + e_b at the counts found
  int ma, mb;     // the counts found
};

// E_e of joint row `row` with `own_is_b ? B : A` as the own side under `own` and the other side under `far`, of which ma of the
// ka rows of A and mb of the kb rows of B are kept (1 <= ma <= ka, 1 <= mb <= kb, the same values in every thread).  SUMS: every
// kept row adds its pair to acc (shifted by ref, which the first call of a visit sets: have_ref).  KEPT: the kept rows leave
// in S.kept_a / S.kept_b.  Four barriers; on entry no thread may still be reading the images, rmin, arg or rede (every caller
// comes from a barrier).
// AUTO: ma, mb come in as the least counts; every row keeps its rank in a register and writes its minimum to sorted[rank] of
// its direction (the ranks are a permutation, so this is the sort), a barrier, find_counts (two more), then the kept rows are
// summed from the ranks exactly as the other form sums them; the pairs weigh r_a / m_a and r_b / m_b (r = q^p, q = k / m, in
// float64); -> F_e = e_a r_a + e_b r_b, with E_e and the counts in `au`.  Seven barriers; sorted and redd are free on entry too.
template <bool SUMS, bool KEPT, bool AUTO>
__device__ float eval_joint(const Lds& L, const Sets& S, size_t row, int ma, int mb, bool own_is_b, const Pose& own,
                            const Pose& far, int tid, double (&acc)[JT_SUMS], float (&ref)[6], bool& have_ref, AutoJoint& au) {
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
  float s1 = 0.f, s2 = 0.f;
  [[maybe_unused]] double ra = 1.0, rb = 1.0;      // auto only: (ka / ma)^p and (kb / mb)^p
  if constexpr (AUTO) {
    int rank[JT_SLOTS];
#pragma unroll
    for (int s = 0; s < JT_SLOTS; ++s) {      // (constant slot indices: the ranks stay in registers)
      const int r = tid + s * JT_T;
      rank[s] = 0;
      if (r < rows) {
        const bool a_row = r < ka;
        const int me = a_row ? r : r - ka;
        const float* v = a_row ? L.rmin : L.rmin + ka;
        const int n = a_row ? ka : kb;
        const float mine = v[me];
        int before = 0;
        for (int c = 0; c < n; ++c) {      // one address for the whole wave: a broadcast read
          const float o = v[c];
          before += (o < mine || (o == mine && c < me)) ? 1 : 0;
        }
        rank[s] = before;
        (a_row ? L.sorted : L.sorted + ka)[before] = mine;      // before < n: the ranks of a direction are a permutation
      }
    }
    __syncthreads();      // both directions' minima stand sorted
    find_counts(L, ka, kb, S.power, tid, ma, mb);
    const double qa = (double)ka / (double)ma, qb = (double)kb / (double)mb;
    ra = qa, rb = qb;
    for (int j = 1; j < S.power; ++j) ra *= qa, rb *= qb;
    const double wa = ra / (double)ma, wb = rb / (double)mb;
#pragma unroll
    for (int s = 0; s < JT_SLOTS; ++s) {      // the thread's rows in the other form's order
      const int r = tid + s * JT_T;
      if (r < rows) {
        const bool a_row = r < ka;
        const int me = a_row ? r : r - ka;
        const bool kept = rank[s] < (a_row ? ma : mb);
        if (kept) {
          const float mine = L.rmin[r];
          if (a_row)
            s1 = __fadd_rn(s1, mine);
          else
            s2 = __fadd_rn(s2, mine);
          if (SUMS) add_pair(L, r, a_row, me, own_is_b, a_row ? wa : wb, ref, acc);
        }
        if (KEPT) L.arg[r] = kept ? 1 : 0;
      }
    }
  } else {
    const double wa = 1.0 / (double)ma, wb = 1.0 / (double)mb;
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
        if (SUMS) add_pair(L, r, a_row, me, own_is_b, a_row ? wa : wb, ref, acc);
      }
      if (KEPT) L.arg[r] = kept ? 1 : 0;      // (a row writes its own slot only, and no pass with KEPT reads the arg-mins)
    }
  }
  float e1, e2;
  block_sum2_f32<JT_W>(L.rede, tid, s1, s2, e1, e2);      // (its barrier: every kept flag is written)
  const float ea = __fdiv_rn(e1, (float)ma), eb = __fdiv_rn(e2, (float)mb);
  float e = __fadd_rn(ea, eb);
  if constexpr (AUTO) {
    au.E = e, au.ma = ma, au.mb = mb;
    e = __fadd_rn(__fmul_rn(ea, (float)ra), __fmul_rn(eb, (float)rb));      // F_e: what the loop compares
  }
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
  __syncthreads();      // rede, rmin, arg and the images are free again (auto: sorted and redd too)
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
// skips the row like a bad (i, j).  AUTO: the launch's least counts (in range by pzn_joint_refine_auto_supported), from which
// the evaluation finds the row's own.
template <bool AUTO>
__device__ __forceinline__ bool row_ok(const Sets& S, size_t row, int i, int j, int K, int& ma, int& mb) {
  if constexpr (AUTO) {
    ma = S.lo_a, mb = S.lo_b;
    return joint_ok(i, j, K);
  } else {
    ma = S.ka, mb = S.kb;
    if (!joint_ok(i, j, K)) return false;
    if (S.ma) ma = S.ma[row];
    if (S.mb) mb = S.mb[row];
    return ma >= 1 && ma <= S.ka && mb >= 1 && mb <= S.kb;
  }
}

// The fp32 sum, in list order, of E_e over the joints of piece p (all joints: p < 0) with piece p under `gp`.  Thread 0 leaves
// every E_e in `out` (LDS): out[e] for a p < 0 pass (0 for a skipped row), out[t] for the t-th joint of piece p otherwise (NULL:
// nowhere); readers come after a barrier.  -> the number of joints met in `met`.  KEPT (a p < 0 pass): the kept rows of every
// row leave in S.kept_a / S.kept_b, -1 throughout for a skipped row.
// AUTO: the sum and `out` hold F_e; the fp32 sum of E_e in the same order leaves in `esum`, and a KEPT pass writes every row's
// E_e and counts to S.joint_score, S.count_a, S.count_b (zeros for a skipped row).
template <bool SUMS, bool KEPT, bool AUTO>
__device__ float eval_joints(const Lds& L, const Sets& S, const int32_t* __restrict__ jl, size_t row0, int J, int K, int p,
                             const Pose& gp, int tid, double (&acc)[JT_SUMS], float (&ref)[6], bool& have_ref, int& met,
                             float* out, float& esum) {
  float E = 0.f;
  met = 0;
  if constexpr (AUTO) esum = 0.f;
  for (int e = 0; e < J; ++e) {      // (workgroup-uniform: the list is the same for every thread)
    const int i = jl[2 * e], j = jl[2 * e + 1];
    int ma, mb;
    const bool ok = row_ok<AUTO>(S, row0 + e, i, j, K, ma, mb);
    if (p < 0 && out && tid == 0 && !ok) out[e] = 0.f;
    if (KEPT && !ok) {
      if (S.kept_a)
        for (int q = tid; q < S.ka; q += JT_T) S.kept_a[(row0 + e) * (size_t)S.ka + q] = -1;
      if (S.kept_b)
        for (int q = tid; q < S.kb; q += JT_T) S.kept_b[(row0 + e) * (size_t)S.kb + q] = -1;
      if constexpr (AUTO)
        if (tid == 0) S.joint_score[row0 + e] = 0.f, S.count_a[row0 + e] = 0, S.count_b[row0 + e] = 0;
    }
    if (!ok || (p >= 0 && i != p && j != p)) continue;
    const bool own_is_b = p < 0 || j == p;
    const Pose own = p < 0 ? load_pose(L.G + 12 * j) : gp;
    const Pose far = load_pose(L.G + 12 * (own_is_b ? i : j));
    AutoJoint au;
    const float ee = eval_joint<SUMS, KEPT, AUTO>(L, S, row0 + e, ma, mb, own_is_b, own, far, tid, acc, ref, have_ref, au);
    if (out && tid == 0) out[p < 0 ? e : met] = ee;
    E = __fadd_rn(E, ee);
    if constexpr (AUTO) {
      esum = __fadd_rn(esum, au.E);
      if (KEPT && tid == 0) S.joint_score[row0 + e] = au.E, S.count_a[row0 + e] = au.ma, S.count_b[row0 + e] = au.mb;
    }
    ++met;
  }
  return E;
}

// The fp32 sum of L.js over all rows in list order (a skipped row holds 0, which changes no bit of a sum of energies), with
// the joints of piece p taken from L.jn instead (p < 0: none; the rows eval_joints met, by the same rule: row_ok and an end
// at p); commit: thread 0 moves those into L.js.
template <bool AUTO>
__device__ float total_with(const Lds& L, const Sets& S, const int32_t* __restrict__ jl, size_t row0, int J, int K, int p,
                            bool commit, int tid) {
  float tot = 0.f;
  int t = 0;
  for (int e = 0; e < J; ++e) {
    const int i = jl[2 * e], j = jl[2 * e + 1];
    int ma, mb;
    const bool mine = p >= 0 && (i == p || j == p) && row_ok<AUTO>(S, row0 + e, i, j, K, ma, mb);
    const float v = mine ? L.jn[t] : L.js[e];
    if (commit && mine && tid == 0) L.js[e] = v;
    t += mine ? 1 : 0;
    tot = __fadd_rn(tot, v);
  }
  return tot;
}

// What only joint_auto_kernel writes (the counts and E_e of every row go out through Sets).
struct AutoOut {
  float *objective, *objective0;      // [Z] the sums of F_e under G and under G0
};

// The one body of the two kernels.  The LDS image: the sibling's (jointtrim.hip states it), and for AUTO the sorted minima
// between the row minima and the arg-mins.
template <bool AUTO>
__device__ __forceinline__ void joint_trim_body(const Sets& S, const int32_t* __restrict__ joints, const float* __restrict__ G0,
                                                const uint8_t* __restrict__ movable, int Z, int K, int J, int sweeps,
                                                float* __restrict__ G, float* __restrict__ score, float* __restrict__ score0,
                                                float* __restrict__ joint_score, int32_t* __restrict__ sweeps_used,
                                                int32_t* __restrict__ accepted, const AutoOut& ao, unsigned char* smem_raw) {
  const int ka = S.ka, kb = S.kb;
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
  L.sorted = AUTO ? L.rmin + ka + kb : nullptr;                       // [ka + kb], auto only
  L.arg = reinterpret_cast<unsigned short*>(L.rmin + (AUTO ? 2 : 1) * (ka + kb));      // [ka + kb]
  const int tid = (int)threadIdx.x;

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
    [[maybe_unused]] float es0 = 0.f, es = 0.f;      // auto only: the sums of E_e under G0 and under the returned poses
    const Pose none = load_pose(L.G);
    eval_joints<false, false, AUTO>(L, S, jl, row0, J, K, -1, none, tid, acc, ref, have_ref, met, L.js, es0);
    __syncthreads();
    const float e0 = total_with<AUTO>(L, S, jl, row0, J, K, -1, false, tid);
    float e = e0;      // E (auto: F) under the current poses: the sum of L.js, the same bits in every thread
    int used = 0;
    for (int sw = 0; sw < sweeps; ++sw) {
      bool any = false;
      for (int p = 0; p < K; ++p) {
        if (!mv[p]) continue;
        const Pose cur = load_pose(L.G + 12 * p);
#pragma unroll
        for (int k = 0; k < JT_SUMS; ++k) acc[k] = 0.0;
        have_ref = false;
        const float ep = eval_joints<true, false, AUTO>(L, S, jl, row0, J, K, p, cur, tid, acc, ref, have_ref, met, nullptr, es);
        if (met == 0 || met > 2 * K) continue;      // (more than 2 (K - 1) rows only where the list repeats a pair: L.jn holds 2 K)
        const Pose nxt = candidate(L, cur, acc, ref, tid);
        const float en = eval_joints<false, false, AUTO>(L, S, jl, row0, J, K, p, nxt, tid, acc, ref, have_ref, met, L.jn, es);
        if (!(en < ep)) continue;      // (the same bits in every thread)
        __syncthreads();               // L.jn is written
        // the fp32 sum over all rows is held to the fall of E_p too: a candidate whose total would round ABOVE the current one
        // is left (a last-place matter: score <= score0 holds to the bit; auto: objective <= objective0)
        const float et = total_with<AUTO>(L, S, jl, row0, J, K, p, false, tid);
        if (!(et <= e)) continue;
        __syncthreads();               // every thread has read L.js
        total_with<AUTO>(L, S, jl, row0, J, K, p, true, tid);
        if (tid < 12) L.G[12 * p + tid] = L.cand[tid];
        if (tid == 0) L.taken[p] += 1;
        e = et;
        any = true;
        __syncthreads();
      }
      if (!any) break;
      ++used;
    }
    if constexpr (!AUTO)
      for (int i = tid; i < J; i += JT_T) joint_score[row0 + i] = L.js[i];
    for (int i = tid; i < 16 * K; i += JT_T) {
      const int p = i >> 4, u = (i >> 2) & 3, v = i & 3;
      const float val = u < 3 ? (v < 3 ? L.G[12 * p + 3 * u + v] : L.G[12 * p + 9 + u]) : (v == 3 ? 1.f : 0.f);
      G[((size_t)z * K + p) * 16 + (i & 15)] = val;
    }
    for (int i = tid; i < K; i += JT_T) accepted[(size_t)z * K + i] = L.taken[i];
    if constexpr (AUTO) {
      // one last evaluation of every joint under the returned poses: its E_e, counts and kept rows (the F_e it finds are L.js's)
      eval_joints<false, true, true>(L, S, jl, row0, J, K, -1, none, tid, acc, ref, have_ref, met, nullptr, es);
      if (tid == 0) score[z] = es, score0[z] = es0, ao.objective[z] = e, ao.objective0[z] = e0, sweeps_used[z] = used;
    } else {
      if (tid == 0) score[z] = e, score0[z] = e0, sweeps_used[z] = used;
      // the rows kept under the returned poses (a kernel argument: workgroup-uniform); the energies it finds are those in L.js
      if (S.kept_a || S.kept_b) eval_joints<false, true, false>(L, S, jl, row0, J, K, -1, none, tid, acc, ref, have_ref, met, nullptr, es);
    }
    __syncthreads();      // the LDS image is replaced by the next puzzle's
  }
}

// Bytes of LDS of a launch: jointtrim.hip's image, and for the auto form 4 (ka + kb) more of sorted minima.
inline size_t joint_trim_lds(int K, int J, int ka, int kb, bool automatic) {
  const size_t kmax = ((size_t)(ka > kb ? ka : kb) + 3) & ~(size_t)3;
  return JT_W * JT_SUMS * sizeof(double) + (JT_W * 2 + 12 + 12 * (size_t)K + 9 * kmax) * sizeof(float) + (size_t)K * sizeof(int) +
         ((size_t)J + 2 * (size_t)K) * sizeof(float) + ((size_t)ka + (size_t)kb) * (sizeof(float) + sizeof(unsigned short)) +
         (automatic ? ((size_t)ka + (size_t)kb) * sizeof(float) : 0);
}

// The range of both forms (jointrefine.hip's).
inline bool joint_trim_range(int K, int J, int ka, int kb) {
  return K >= 1 && K <= JT_MAX_PIECES && J >= 0 && J <= K * (K - 1) && ka >= 1 && kb >= 1 && ka <= JT_MAX_K && kb <= JT_MAX_K;
}

}  // namespace

#endif  // PZN_JOINTTRIM_H_
