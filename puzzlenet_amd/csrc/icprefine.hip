// icprefine.hip — refine every pair pose on its matched boundaries, for gfx950 (assembly.refine_pairs).
//
// One workgroup per problem p does symmetric point-to-point ICP between the fixed set a (ka rows) and the moved set b (kb
// rows), from the pose T0[p], with everything in LDS: what would otherwise be transform -> chamfer -> two gathers -> centring
// -> bmm -> batched 3x3 SVD -> compose -> chamfer again, about a dozen launches per iteration.
//   * state: ONE pose (R, t) as fp32 values, in every thread's registers.  A pose is always evaluated on the original moved
//     points: x' = ((R00 x + R01 y) + R02 z) + t0, every product and sum rounded on its own (__fmul_rn / __fadd_rn: the
//     arithmetic of mergefps.hip, so a refined pose moves points to the same bits there as here);
//   * objective: E(T) = mean_i min_j |a_i - T b_j|^2 + mean_j min_i |a_i - T b_j|^2, direct differences
//     (pzn::sqdist3), arg-min = the lowest index of the minimum.  Row r < ka of the ka + kb rows is a_r scanning T b, row
//     ka + j is T b_j scanning a; a thread owns rows tid, tid + 256, ... and adds their minima in that order, the wave adds
//     its 64 lanes by the xor butterfly (both partners form the same sum), the four wave sums are added in wave order:
//     the same bits on every run;
//   * one iteration from T: the correspondences c1(i), c2(j) of the evaluation of T give ka + kb pairs (fixed p, moved q):
//     (a_i, b_c1(i)) and (a_c2(j), b_j), q always the ORIGINAL point.  Centroids, then the centred cross-covariance
//     S = sum (q - qc)(p - pc)^T and the moved side's scatter C = sum (q - qc)(q - qc)^T, all accumulated in float64 (thread,
//     butterfly, wave order).  Thread 0 solves in float64: Horn's quaternion - the eigenvector of the largest eigenvalue of
//     the symmetric 4x4 N(S), cyclic Jacobi sweeps - which is Kabsch with the reflection fix; t' = pc - R' qc; both rounded
//     to fp32.  E(T') < E(T) takes the candidate, anything else (NaN included) stops and keeps T: the only stop rule besides
//     iters;
//   * DEGENERATE correspondences (a single point, all moved-side points q coincident or collinear) keep the current R and
//     update t only: the rule is stated, with the solve, at solve_pose in pzn_rigid.h.
// Latency-bound: per iteration a serial chain of six barriers, a (ka | kb)-step scan and one lane's float64 solve; the
// launch is parallel over problems only, and the grid walks when P exceeds ICP_MAX_GRID.
//
// TRIMMED form (icp_trim_kernel, pzn_icp_refine_trim_f32): the same body with TRIM = true, for pieces of which only a part
// mates.  Of each direction's rows only the m_a (m_b) with the smallest (row minimum, row index) count, in E - the kept
// minima summed in today's order, divided by m_a and m_b - and as pairs of the step (divisor m_a + m_b).  What it adds per
// evaluation: every row's minimum goes to LDS, one more barrier, and every row RANKS itself by counting the rows of its
// direction that precede it in (value, index) order - all lanes read the same address, a broadcast, O(k) per row like the
// scan - kept iff rank < m: exactly m rows whatever the ties, the same on every run.  The kept rows live in a byte mask; there
// are TWO masks, the current pose's and the one the candidate's evaluation writes, swapped when the candidate is taken, so
// the kept set of the returned pose survives a rejected candidate and kept_a / kept_b are written once, at the end.
// icp_refine_kernel is the TRIM = false instantiation: no minima in LDS, no ranking, no mask, the instructions it had before.
//
// AUTO form (icp_auto_kernel, pzn_icp_refine_auto_f32): the trimmed body with AUTO = true, the counts no longer the caller's
// but found per problem and per evaluation of a pose (the rule is stated in include/pzn.h).  What an evaluation gains: after
// the ranking every row writes its minimum to sorted[rank] of its direction (ranks are a permutation, so this IS the sort)
// and keeps its rank in a register; a barrier; thread t adds the four sorted values 4t .. 4t+3 of each direction one after
// the other, the wave scans the thread totals (Hillis-Steele, lane l adds lane l - d for d = 1 .. 32), the four wave totals
// go through LDS and are added in wave order: float32 prefix sums S_m in one fixed order; each thread forms
// phi(m) = (double)S_m / m^(p+1) for its own four m in [lo, n] (one float64 division a row), and the lexicographic arg-min of
// (phi, larger m) is a butterfly and four LDS slots per direction.  The two counts are then workgroup-uniform, the kept
// masks are written from the ranks in registers and the kept minima summed exactly as the trimmed form sums them.  The loop
// compares F = e_a (ka / m_a)^p + e_b (kb / m_b)^p where the other two compare E; counts, like masks, belong to a pose.
// The other two instantiations compile to the instructions they had (every addition stands under if constexpr (AUTO)).
#include "pzn_rigid.h"      // the wave and workgroup sums, solve_pose, Pose / pose_move: shared with jointrefine.hip

namespace {

constexpr int ICP_T = 256;                 // four wavefronts
constexpr int ICP_W = ICP_T / PZN_WAVE;
constexpr int ICP_MAX_K = 1024;            // 36 KB of point images + 4 KB of arg-mins + 0.5 KB of reduction slots: 40.5 KB of LDS at most;
                                           // trimmed: + 8 KB of row minima + 2 x 2 KB of kept masks = 52.5 KB at most;
                                           // auto: + 8 KB of sorted minima = 60.5 KB at most, under the 64 KB of a plain launch
constexpr int ICP_SLOTS = 2 * ICP_MAX_K / ICP_T;      // rows a thread owns at most (auto: their ranks stay in registers)
constexpr int ICP_MAX_GRID = 512;          // two workgroups per CU of a 256-CU part; more problems share a workgroup in turn

struct Lds {
  float *ax, *ay, *az;      // fixed set, [ka]
  float *bx, *by, *bz;      // moved set as given, [kb]
  float *tx, *ty, *tz;      // moved set under the pose being evaluated, [kb]
  unsigned short* corr;     // [ka + kb] arg-min of every row under the pose evaluated last (a row's owner alone touches it)
  float* rmin;              // trimmed only: [ka + kb] the minimum of every row under the pose evaluated last
  unsigned char* keep;      // trimmed only: [2][ka + kb] kept masks (1 = kept); which is the current pose's is the caller's flip
  float* sorted;            // auto only: [ka + kb] every direction's row minima in (value, index) order
  double* redd;             // [ICP_W][15] wave partials of the float64 sums
  float* rede;              // [ICP_W][2] wave partials of the two objective sums
  float* cand;              // [12] the candidate pose, thread 0 -> everyone
};

// What an evaluation of the auto form takes and leaves beside E.
struct AutoEval {
  int power;      // in: p of phi(m) = S_m / m^(p+1)
  int ma, mb;     // out: the counts of the pose evaluated
  float F;        // out: e_a (ka / ma)^p + e_b (kb / mb)^p
};

// (phi, m) before (ophi, om) in the arg-min's order: the smaller phi, among equal phi the larger m
__device__ __forceinline__ bool phi_before(double phi, int m, double ophi, int om) { return phi < ophi || (phi == ophi && m > om); }

// E(pose): moves b into (tx, ty, tz), scans, leaves every row's arg-min in L.corr -> the objective, the same bits in every
// thread.  Three barriers; on entry no thread may still be reading tx / rede (every caller comes from a barrier).
// TRIM: every row's minimum goes to L.rmin, a fourth barrier, then every row counts the rows of its direction before it in
// (minimum, index) order - kept iff fewer than ma (mb) - marks itself in `keep` [ka + kb] and only kept minima are summed.
// AUTO: ma, mb come in as the least counts lo_a, lo_b; the counts of this pose are found (header comment; two barriers for the
// sort and the prefix sums, one for the arg-min) and leave in `au` with the objective F; the value returned stays E at them.
template <bool TRIM, bool AUTO = false>
__device__ float evaluate(const Lds& L, const Pose& g, int ka, int kb, int ma, int mb, unsigned char* keep, int tid,
                          AutoEval* au = nullptr) {
  for (int j = tid; j < kb; j += ICP_T) {
    const float x = L.bx[j], y = L.by[j], z = L.bz[j];
    pose_move(g, x, y, z, L.tx[j], L.ty[j], L.tz[j]);
  }
  __syncthreads();
  float s1 = 0.f, s2 = 0.f;
  const int rows = ka + kb;
  for (int r = tid; r < rows; r += ICP_T) {
    const bool fixed_row = r < ka;
    const int own = fixed_row ? r : r - ka;
    const float qx = fixed_row ? L.ax[own] : L.tx[own];
    const float qy = fixed_row ? L.ay[own] : L.ty[own];
    const float qz = fixed_row ? L.az[own] : L.tz[own];
    const float* sx = fixed_row ? L.tx : L.ax;
    const float* sy = fixed_row ? L.ty : L.ay;
    const float* sz = fixed_row ? L.tz : L.az;
    const int n = fixed_row ? kb : ka;
    float best = __builtin_inff();
    int arg = 0;
    for (int c = 0; c < n; ++c) {
      // (a - T b) in both directions; strict <: the lowest index of equal distances stays
      const float d = fixed_row ? pzn::sqdist3(qx, qy, qz, sx[c], sy[c], sz[c]) : pzn::sqdist3(sx[c], sy[c], sz[c], qx, qy, qz);
      const bool take = d < best;
      best = take ? d : best;
      arg = take ? c : arg;
    }
    L.corr[r] = (unsigned short)arg;
    if constexpr (TRIM) {
      L.rmin[r] = best;
    } else {
      if (fixed_row)
        s1 = __fadd_rn(s1, best);
      else
        s2 = __fadd_rn(s2, best);
    }
  }
  if constexpr (AUTO) {
    __syncthreads();      // every row's minimum is in rmin
    int rank[ICP_SLOTS];
#pragma unroll
    for (int s = 0; s < ICP_SLOTS; ++s) {      // (constant slot indices: the ranks stay in registers)
      const int r = tid + s * ICP_T;
      rank[s] = 0;
      if (r < rows) {
        const bool fixed_row = r < ka;
        const int own = fixed_row ? r : r - ka;
        const float* v = fixed_row ? L.rmin : L.rmin + ka;
        const int n = fixed_row ? ka : kb;
        const float mine = v[own];
        int before = 0;
        for (int c = 0; c < n; ++c) {
          const float o = v[c];
          before += (o < mine || (o == mine && c < own)) ? 1 : 0;
        }
        rank[s] = before;
        (fixed_row ? L.sorted : L.sorted + ka)[before] = mine;      // before < n: the ranks of a direction are a permutation
      }
    }
    __syncthreads();      // both directions' minima stand sorted
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
      for (int w = 0; w < ICP_W - 1; ++w) off = w < wave ? __fadd_rn(off, L.rede[2 * w + d]) : off;
      const float base = __fadd_rn(off, exc[d]);
      bphi[d] = (double)__builtin_inff(), bm[d] = 0;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int m = 4 * tid + i + 1;
        const double dm = (double)m;
        double q = dm;
        for (int j = 0; j < au->power; ++j) q *= dm;      // m^(p+1), exact: m <= 1024, p + 1 <= 5
        const double phi = (double)__fadd_rn(base, c[d][i]) / q;
        const bool take = m >= lo && m <= n && phi_before(phi, m, bphi[d], bm[d]);
        bphi[d] = take ? phi : bphi[d], bm[d] = take ? m : bm[d];
      }
#define ICP_PHI_STEP(J)                                                                                         \
  {                                                                                                             \
    const double ophi = __longlong_as_double((long long)pzn::xor_lane_u64<J>((uint64_t)__double_as_longlong(bphi[d]))); \
    const int om = (int)pzn::xor_lane<J>((uint32_t)bm[d]);                                                      \
    const bool take = phi_before(ophi, om, bphi[d], bm[d]);                                                     \
    bphi[d] = take ? ophi : bphi[d], bm[d] = take ? om : bm[d];                                                 \
  }
      ICP_PHI_STEP(1) ICP_PHI_STEP(2) ICP_PHI_STEP(4) ICP_PHI_STEP(8) ICP_PHI_STEP(16) ICP_PHI_STEP(32)
#undef ICP_PHI_STEP
      if (lane == 0) L.redd[15 * wave + 2 * d] = bphi[d], L.redd[15 * wave + 2 * d + 1] = (double)bm[d];
    }
    __syncthreads();      // the four waves' best (phi, m) of both directions
#pragma unroll
    for (int d = 0; d < 2; ++d) {
      double phi = L.redd[2 * d];
      int m = (int)L.redd[2 * d + 1];
#pragma unroll
      for (int w = 1; w < ICP_W; ++w) {
        const double ophi = L.redd[15 * w + 2 * d];
        const int om = (int)L.redd[15 * w + 2 * d + 1];
        const bool take = phi_before(ophi, om, phi, m);
        phi = take ? ophi : phi, m = take ? om : m;
      }
      (d ? mb : ma) = m;      // in [lo, n]: the same value in every thread
    }
#pragma unroll
    for (int s = 0; s < ICP_SLOTS; ++s) {
      const int r = tid + s * ICP_T;
      if (r < rows) {
        const bool fixed_row = r < ka;
        const bool kept = rank[s] < (fixed_row ? ma : mb);
        keep[r] = kept ? 1 : 0;
        if (kept) {
          if (fixed_row)
            s1 = __fadd_rn(s1, L.rmin[r]);
          else
            s2 = __fadd_rn(s2, L.rmin[r]);
        }
      }
    }
  } else if constexpr (TRIM) {
    __syncthreads();      // every row's minimum is in rmin
    for (int r = tid; r < rows; r += ICP_T) {
      const bool fixed_row = r < ka;
      const int own = fixed_row ? r : r - ka;
      const float* v = fixed_row ? L.rmin : L.rmin + ka;
      const int n = fixed_row ? ka : kb;
      const float mine = v[own];      // (never NaN: a NaN distance never passes d < best)
      int before = 0;
      for (int c = 0; c < n; ++c) {      // one address for the whole wave: a broadcast read
        const float o = v[c];
        before += (o < mine || (o == mine && c < own)) ? 1 : 0;
      }
      const bool kept = before < (fixed_row ? ma : mb);
      keep[r] = kept ? 1 : 0;
      if (kept) {
        if (fixed_row)
          s1 = __fadd_rn(s1, mine);
        else
          s2 = __fadd_rn(s2, mine);
      }
    }
  }
  float e1, e2;
  block_sum2_f32<ICP_W>(L.rede, tid, s1, s2, e1, e2);
  const float ea = __fdiv_rn(e1, (float)(TRIM ? ma : ka)), eb = __fdiv_rn(e2, (float)(TRIM ? mb : kb));
  const float e = __fadd_rn(ea, eb);
  if constexpr (AUTO) {
    const double qa = (double)ka / (double)ma, qb = (double)kb / (double)mb;
    double ra = qa, rb = qb;
    for (int j = 1; j < au->power; ++j) ra *= qa, rb *= qb;
    au->ma = ma, au->mb = mb;
    au->F = __fadd_rn(__fmul_rn(ea, (float)ra), __fmul_rn(eb, (float)rb));
  }
  __syncthreads();      // rede and tx are free again (auto: redd too)
  return e;
}

// The candidate from the correspondences in L.corr and the current pose (kept when the pairs are degenerate).  Three barriers.
// TRIM: the pairs of the rows marked in `keep` alone, npairs = ma + mb of them (otherwise all ka + kb rows; npairs is not read).
template <bool TRIM>
__device__ Pose candidate(const Lds& L, const Pose& cur, int ka, int kb, int npairs, const unsigned char* keep, int tid) {
  const int rows = ka + kb;
  const int lane = tid & (PZN_WAVE - 1), wave = tid / PZN_WAVE;
  // pass 1: centroids of the fixed-side points p and the moved-side points q of the ka + kb pairs
  double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int r = tid; r < rows; r += ICP_T) {
    if (TRIM && !keep[r]) continue;
    const int c = L.corr[r];
    const int ia = r < ka ? r : c, ib = r < ka ? c : r - ka;
    s[0] += (double)L.ax[ia], s[1] += (double)L.ay[ia], s[2] += (double)L.az[ia];
    s[3] += (double)L.bx[ib], s[4] += (double)L.by[ib], s[5] += (double)L.bz[ib];
  }
#pragma unroll
  for (int k = 0; k < 6; ++k) s[k] = wave_sum_f64(s[k]);
  if (lane == 0)
#pragma unroll
    for (int k = 0; k < 6; ++k) L.redd[15 * wave + k] = s[k];
  __syncthreads();
  double cen[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    double v = L.redd[k];
#pragma unroll
    for (int w = 1; w < ICP_W; ++w) v += L.redd[15 * w + k];
    cen[k] = v / (double)(TRIM ? npairs : rows);
  }
  __syncthreads();      // redd is written again below
  // pass 2: S[u][v] = sum qd_u pd_v (9) and the upper triangle of C = sum qd qd^T (6)
  double m[15];
#pragma unroll
  for (int k = 0; k < 15; ++k) m[k] = 0.0;
  for (int r = tid; r < rows; r += ICP_T) {
    if (TRIM && !keep[r]) continue;
    const int c = L.corr[r];
    const int ia = r < ka ? r : c, ib = r < ka ? c : r - ka;
    const double px = (double)L.ax[ia] - cen[0], py = (double)L.ay[ia] - cen[1], pz = (double)L.az[ia] - cen[2];
    const double qx = (double)L.bx[ib] - cen[3], qy = (double)L.by[ib] - cen[4], qz = (double)L.bz[ib] - cen[5];
    m[0] += qx * px, m[1] += qx * py, m[2] += qx * pz;
    m[3] += qy * px, m[4] += qy * py, m[5] += qy * pz;
    m[6] += qz * px, m[7] += qz * py, m[8] += qz * pz;
    m[9] += qx * qx, m[10] += qy * qy, m[11] += qz * qz;
    m[12] += qx * qy, m[13] += qx * qz, m[14] += qy * qz;
  }
#pragma unroll
  for (int k = 0; k < 15; ++k) m[k] = wave_sum_f64(m[k]);
  if (lane == 0)
#pragma unroll
    for (int k = 0; k < 15; ++k) L.redd[15 * wave + k] = m[k];
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int k = 0; k < 15; ++k) {
      double v = L.redd[k];
#pragma unroll
      for (int w = 1; w < ICP_W; ++w) v += L.redd[15 * w + k];
      m[k] = v;
    }
    const double S[3][3] = {{m[0], m[1], m[2]}, {m[3], m[4], m[5]}, {m[6], m[7], m[8]}};
    const double C[6] = {m[9], m[10], m[11], m[12], m[13], m[14]};
    const double pc[3] = {cen[0], cen[1], cen[2]}, qc[3] = {cen[3], cen[4], cen[5]};
    solve_pose(S, C, cur, pc, qc, L.cand);
  }
  __syncthreads();
  Pose out;
#pragma unroll
  for (int k = 0; k < 9; ++k) out.r[k] = L.cand[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) out.t[k] = L.cand[9 + k];
  return out;      // (cand is written next after the three barriers of an evaluation)
}

// The arg-mins of the pose evaluated last leave as corr_a[p] / corr_b[p] (either may be NULL); every row by its owner.
__device__ __forceinline__ void store_corr(const Lds& L, int p, int ka, int kb, int tid, int32_t* __restrict__ corr_a,
                                           int32_t* __restrict__ corr_b) {
  for (int r = tid; r < ka + kb; r += ICP_T) {
    if (r < ka) {
      if (corr_a) corr_a[(size_t)p * ka + r] = (int32_t)L.corr[r];
    } else {
      if (corr_b) corr_b[(size_t)p * kb + (r - ka)] = (int32_t)L.corr[r];
    }
  }
}

// The arguments both kernels take.
#define ICP_PARAMS                                                                                                          \
  const float *__restrict__ a, const int64_t *__restrict__ a_of, const float *__restrict__ b,                               \
      const int64_t *__restrict__ b_of, const float *__restrict__ T0, int P, int ka, int kb, int iters,                     \
      float *__restrict__ T, float *__restrict__ score, float *__restrict__ score0, int32_t *__restrict__ iters_used,       \
      int32_t *__restrict__ corr_a, int32_t *__restrict__ corr_b

// What only the trimmed kernel takes, as the kernel's last argument.  The untrimmed form is empty, so icp_refine_kernel keeps
// the arguments it had, and the names of the two argument types are what tells the two instantiations apart in a trace.
struct icp_trim_kernel_args {
  static constexpr bool TRIM = true, AUTO = false;
  int ma, mb;                   // rows kept of a and of b
  int32_t *kept_a, *kept_b;     // [P,ma], [P,mb] or NULL
};
struct icp_refine_kernel_args {
  static constexpr bool TRIM = false, AUTO = false;
  static constexpr int ma = 0, mb = 0;
  static constexpr int32_t *kept_a = nullptr, *kept_b = nullptr;
};

// The auto form: ma, mb are the least counts lo_a, lo_b; kept_a [P,ka], kept_b [P,kb] are padded with -1 behind the count.
struct icp_auto_kernel_args {
  static constexpr bool TRIM = true, AUTO = true;
  int ma, mb;
  int32_t *kept_a, *kept_b;     // [P,ka], [P,kb] or NULL
  int power;
  int32_t *count_a, *count_b;   // [P]
  float* objective;             // [P]
};

// The one body of the kernels (icp_auto_kernel = icp_kernel<icp_auto_kernel_args>): icp_refine_kernel = icp_kernel<icp_refine_kernel_args>, icp_trim_kernel =
// icp_kernel<icp_trim_kernel_args>.  The body stands in the kernel itself and the untrimmed form sets up its LDS exactly as
// it did before there was a second form: its instructions are then the earlier kernel's, one for one (an inlined body
// function between the two cost the untrimmed launch 3 % through another register allocation).
template <typename Args>
__global__ __launch_bounds__(ICP_T) void icp_kernel(ICP_PARAMS, Args trim) {
  constexpr bool TRIM = Args::TRIM, AUTO = Args::AUTO;
  const int ma = trim.ma, mb = trim.mb;
  int32_t* const kept_a = trim.kept_a;
  int32_t* const kept_b = trim.kept_b;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  Lds L;
  L.redd = reinterpret_cast<double*>(smem_raw);                       // [ICP_W][15]
  L.rede = reinterpret_cast<float*>(L.redd + ICP_W * 15);             // [ICP_W][2]
  L.cand = L.rede + ICP_W * 2;                                        // [12]
  L.ax = L.cand + 12, L.ay = L.ax + ka, L.az = L.ay + ka;
  L.bx = L.az + ka, L.by = L.bx + kb, L.bz = L.by + kb;
  L.tx = L.bz + kb, L.ty = L.tx + kb, L.tz = L.ty + kb;
  L.rmin = TRIM ? L.tz + kb : nullptr;                                                 // [ka + kb], trimmed only
  L.sorted = AUTO ? L.rmin + ka + kb : nullptr;                                        // [ka + kb], auto only
  L.corr = reinterpret_cast<unsigned short*>(L.tz + kb + (TRIM ? ka + kb : 0) + (AUTO ? ka + kb : 0));      // [ka + kb]
  L.keep = TRIM ? reinterpret_cast<unsigned char*>(L.corr + ka + kb) : nullptr;         // [2][ka + kb], trimmed only
  const int npairs = TRIM ? ma + mb : 0;      // (the untrimmed candidate divides by its own ka + kb)
  const int tid = (int)threadIdx.x;

  for (int p = (int)blockIdx.x; p < P; p += (int)gridDim.x) {      // (workgroup-uniform)
    const float* ga = a + (size_t)(a_of ? a_of[p] : (int64_t)p) * ka * 3;
    const float* gb = b + (size_t)(b_of ? b_of[p] : (int64_t)p) * kb * 3;
    for (int i = tid; i < 3 * ka; i += ICP_T) {
      const float v = ga[i];
      const int q = i / 3, c = i - 3 * q;
      (c == 0 ? L.ax : (c == 1 ? L.ay : L.az))[q] = v;
    }
    for (int i = tid; i < 3 * kb; i += ICP_T) {
      const float v = gb[i];
      const int q = i / 3, c = i - 3 * q;
      (c == 0 ? L.bx : (c == 1 ? L.by : L.bz))[q] = v;
    }
    const float* g0 = T0 + (size_t)p * 16;
    Pose cur;
#pragma unroll
    for (int u = 0; u < 3; ++u) {
      cur.r[3 * u] = g0[4 * u], cur.r[3 * u + 1] = g0[4 * u + 1], cur.r[3 * u + 2] = g0[4 * u + 2];
      cur.t[u] = g0[4 * u + 3];
    }
    __syncthreads();

    int flip = 0;      // which kept mask is the current pose's (workgroup-uniform; trimmed only)
    [[maybe_unused]] AutoEval ac, an;      // auto only: the counts and F of the current pose and of the candidate
    if constexpr (AUTO) ac.power = an.power = trim.power;
    float e = evaluate<TRIM, AUTO>(L, cur, ka, kb, ma, mb, L.keep, tid, &ac);
    const float e0 = e;
    int used = 0;
    for (int it = 0; it < iters; ++it) {      // (e, and with it the exit, is the same in every thread)
      // the correspondences this candidate is built from (L.corr is overwritten by its evaluation)
      store_corr(L, p, ka, kb, tid, corr_a, corr_b);
      const Pose nxt = candidate<TRIM>(L, cur, ka, kb, AUTO ? ac.ma + ac.mb : npairs, L.keep + flip * (ka + kb), tid);
      const float en = evaluate<TRIM, AUTO>(L, nxt, ka, kb, ma, mb, L.keep + (flip ^ 1) * (ka + kb), tid, &an);      // (the other mask)
      if constexpr (AUTO) {
        if (!(an.F < ac.F)) break;      // F is what falls; the score follows the counts
        ac = an;
      } else {
        if (!(en < e)) break;
      }
      cur = nxt, e = en, ++used, flip ^= 1;
    }
    if (iters == 0) store_corr(L, p, ka, kb, tid, corr_a, corr_b);      // the correspondences under T0
    if constexpr (TRIM) {
      // the rows kept under the returned pose, ascending: a kept row's place is the number of kept rows before it (the mask
      // was complete at the last barrier of the evaluation that wrote it)
      const unsigned char* kp = L.keep + flip * (ka + kb);
      for (int r = tid; r < ka + kb; r += ICP_T) {
        const bool fixed_row = r < ka;
        int32_t* out = fixed_row ? kept_a : kept_b;
        if (!kp[r] || !out) continue;
        const int own = fixed_row ? r : r - ka, m = AUTO ? (fixed_row ? ac.ma : ac.mb) : (fixed_row ? ma : mb);
        const int stride = AUTO ? (fixed_row ? ka : kb) : m;
        const unsigned char* side = fixed_row ? kp : kp + ka;
        int pos = 0;
        for (int c = 0; c < own; ++c) pos += side[c];
        if (pos < m) out[(size_t)p * stride + pos] = own;      // (always: exactly m rows of a direction are kept)
      }
    }
    if constexpr (AUTO) {
      for (int r = tid; r < ka + kb; r += ICP_T) {      // -1 behind the count
        const bool fixed_row = r < ka;
        int32_t* out = fixed_row ? kept_a : kept_b;
        const int own = fixed_row ? r : r - ka;
        if (out && own >= (fixed_row ? ac.ma : ac.mb)) out[(size_t)p * (fixed_row ? ka : kb) + own] = -1;
      }
      if (tid == 0) trim.count_a[p] = ac.ma, trim.count_b[p] = ac.mb, trim.objective[p] = ac.F;
    }
    if (tid < 16) {
      const int u = tid >> 2, v = tid & 3;
      float val = 0.f;
#pragma unroll
      for (int k = 0; k < 9; ++k) val = (u < 3 && v < 3 && 3 * u + v == k) ? cur.r[k] : val;
#pragma unroll
      for (int k = 0; k < 3; ++k) val = (u == k && v == 3) ? cur.t[k] : val;
      val = tid == 15 ? 1.f : val;
      T[(size_t)p * 16 + tid] = val;
    }
    if (tid == 0) score[p] = e, score0[p] = e0, iters_used[p] = used;
    __syncthreads();      // the LDS image is replaced by the next problem's
  }
}

// Bytes of LDS of a launch: reduction slots, the three point images, the arg-mins; trimmed: the row minima and two masks;
// automatic: the sorted minima too.
size_t icp_lds_bytes(int ka, int kb, bool trim, bool automatic) {
  const size_t rows = (size_t)ka + (size_t)kb;
  return ICP_W * 15 * sizeof(double) + (ICP_W * 2 + 12) * sizeof(float) + 3 * ((size_t)ka + 2 * (size_t)kb) * sizeof(float) +
         rows * sizeof(unsigned short) + (trim ? rows * sizeof(float) + 2 * rows : 0) + (automatic ? rows * sizeof(float) : 0);
}

// The one launch of the three forms: `supported` is the form's own pzn_*_supported answer, `extra` what the form must have
// beside the common outputs.
template <typename Args>
int icp_launch(bool supported, bool extra, const float* a, const int64_t* a_of, const float* b, const int64_t* b_of,
               const float* T0, int P, int ka, int kb, int iters, float* T, float* score, float* score0, int32_t* iters_used,
               int32_t* corr_a, int32_t* corr_b, const Args& args, pzn_stream_t stream) {
  if (!supported || iters < 0) return PZN_EUNSUPPORTED;
  PZN_CHECK_ARG(P >= 0);
  if (P == 0) return PZN_OK;
  PZN_CHECK_ARG(a && b && T0 && T && score && score0 && iters_used && extra);
  hipStream_t st = pzn_hip_stream(stream);
  const int grid = P < ICP_MAX_GRID ? P : ICP_MAX_GRID;
  PZN_LAUNCH(icp_kernel<Args>, dim3(grid), dim3(ICP_T), icp_lds_bytes(ka, kb, Args::TRIM, Args::AUTO), st, a, a_of, b, b_of, T0,
             P, ka, kb, iters, T, score, score0, iters_used, corr_a, corr_b, args);
  PZN_RETURN_LAUNCH_STATUS();
}

}  // namespace

PZN_EXPORT int pzn_icp_refine_supported(int ka, int kb) { return ka >= 1 && kb >= 1 && ka <= ICP_MAX_K && kb <= ICP_MAX_K; }

PZN_EXPORT int pzn_icp_refine_f32(const float* a, const int64_t* a_of, const float* b, const int64_t* b_of, const float* T0,
                                  int P, int ka, int kb, int iters, float* T, float* score, float* score0,
                                  int32_t* iters_used, int32_t* corr_a, int32_t* corr_b, pzn_stream_t stream) {
  return icp_launch(pzn_icp_refine_supported(ka, kb), true, a, a_of, b, b_of, T0, P, ka, kb, iters, T, score, score0, iters_used,
                    corr_a, corr_b, icp_refine_kernel_args{}, stream);
}

PZN_EXPORT int pzn_icp_refine_trim_supported(int ka, int kb, int keep_a, int keep_b) {
  return pzn_icp_refine_supported(ka, kb) && keep_a >= 1 && keep_a <= ka && keep_b >= 1 && keep_b <= kb;
}

PZN_EXPORT int pzn_icp_refine_trim_f32(const float* a, const int64_t* a_of, const float* b, const int64_t* b_of, const float* T0,
                                       int P, int ka, int kb, int keep_a, int keep_b, int iters, float* T, float* score,
                                       float* score0, int32_t* iters_used, int32_t* corr_a, int32_t* corr_b, int32_t* kept_a,
                                       int32_t* kept_b, pzn_stream_t stream) {
  return icp_launch(pzn_icp_refine_trim_supported(ka, kb, keep_a, keep_b), true, a, a_of, b, b_of, T0, P, ka, kb, iters, T, score,
                    score0, iters_used, corr_a, corr_b, icp_trim_kernel_args{keep_a, keep_b, kept_a, kept_b}, stream);
}

PZN_EXPORT int pzn_icp_refine_auto_supported(int ka, int kb, int lo_a, int lo_b, int power) {
  return pzn_icp_refine_trim_supported(ka, kb, lo_a, lo_b) && power >= 1 && power <= 4;
}

PZN_EXPORT int pzn_icp_refine_auto_f32(const float* a, const int64_t* a_of, const float* b, const int64_t* b_of, const float* T0,
                                       int P, int ka, int kb, int lo_a, int lo_b, int power, int iters, float* T, float* score,
                                       float* score0, int32_t* iters_used, int32_t* corr_a, int32_t* corr_b, int32_t* count_a,
                                       int32_t* count_b, float* objective, int32_t* kept_a, int32_t* kept_b, pzn_stream_t stream) {
  return icp_launch(pzn_icp_refine_auto_supported(ka, kb, lo_a, lo_b, power), count_a && count_b && objective, a, a_of, b, b_of,
                    T0, P, ka, kb, iters, T, score, score0, iters_used, corr_a, corr_b,
                    icp_auto_kernel_args{lo_a, lo_b, kept_a, kept_b, power, count_a, count_b, objective}, stream);
}
