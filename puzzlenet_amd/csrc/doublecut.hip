// doublecut.hip — the double cut of the reference's loader (dataset.py:1203-1355, `split_twice=True`) as one launch per batch.
//
// `CADDataset.__getitem__` cuts the cloud by a plane, cuts one of the two pieces again and returns the two halves, a half
// against the rest, or a half against the other piece; with nothing valid it falls back to the single cut.  Which branch is
// taken depends on piece sizes, so the host form (datapipe.plan_double_cut_like_reference) needs the counts on the host.  Here
// every draw of a sample is made up front - K candidates for plane 1, 7 for plane 2 (the first draw and the six re-draws of
// `while time <= 5`), seven uniforms - and one workgroup per sample walks the decision tree of datapipe.double_cut_rule (the
// numpy statement of this kernel) on counts it takes itself:
//   1. sides of plane-1 candidate 0: a = |up|;  2. seed with its two flips by n_rich;  4. the first plane-2 candidate that
//   leaves >= n_min points on both sides INSIDE the inner piece;  5. the kind and its region tables;  6. SINGLE: the first valid
//   plane-1 candidate, else the most balanced one (ok = 0);  7. the start indices.
// A point's cell is code = 2 s1 + s2 (s = side of the plane taken, 1: distance >= 0); a piece is an ordered pair of region
// tables (bit `code` set = the cell belongs to it: datapipe.UP, UP_UPPC, ...): rows of the first table, then rows of the second,
// each in the cloud's point order (np.vstack, dataset.py:1239) - a two-segment stable partition written from ONE scan of the
// packed per-thread counts.  The signed distance is the plane cut's: float64, every operation individually rounded (no fma);
// it, the block sum, the exclusive scan, the padding and the start index come from pzn_cut.h.  The decision tree and the two-segment partition are
// this file's own (the single cuts' two-way body is a different algorithm).
//
// Replaces, per batch: a device-to-host round trip per decision, two float64 einsums, two stable sorts of [B, M] keys per piece.
#include "pzn_common.h"

namespace {

#include "pzn_cut.h"

constexpr int DC_TRIES = 7;          // plane-2 candidates: the first draw + the re-draws of `while time <= 5` (dataset.py:1227)
constexpr int DC_UNIFORMS = 7;       // u_seed, u_se, u_choice, u_sU, u_sD, u_sFU, u_sFD

enum Kind { SINGLE = 0, HALF_VS_REST = 1, HALF_VS_OTHER = 2, HALVES = 3 };
// region tables (datapipe.py): bit 2 s1 + s2
constexpr int R_UP = 0xC, R_DOWN = 0x3, R_UP_UPPC = 0x8, R_UP_DOWNPC = 0x4, R_DOWN_UPPC = 0x2, R_DOWN_DOWNPC = 0x1;

struct DoubleCutArgs {
  const float* raw;         // [B, M, 3]
  const double* normals1;   // [B, K, 3]
  const double* zs1;        // [B, K]
  const double* normals2;   // [B, 7, 3]
  const double* zs2;        // [B, 7]
  const double* u;          // [B, 7]
  int B, M, K, n_min, n_rich, cap;
  float* pieces;            // [4B, cap, 3]: U, D, fallback U, fallback D
  int64_t* counts;          // [4B]: -1 = no such piece (the fallback rows of samples that are not HALF_VS_OTHER)
  int64_t* start;           // [4B]
  int32_t* kind;            // [B]
  double* planes;           // [B, 2, 4]
  int32_t* tabs;            // [B, 4]: u_tab, d_tab
  uint8_t* ok;              // [B]
};

// 0 / 1: the segment of the piece (t0, t1) a cell belongs to; 2: left out (datapipe._segments)
__device__ __forceinline__ int segment(int code, int t0, int t1) { return ((t0 >> code) & 1) ? 0 : (((t1 >> code) & 1) ? 1 : 2); }

__global__ __launch_bounds__(CUT_T) void cut_compact_double_kernel(DoubleCutArgs a) {
  __shared__ int slots[CUT_W];
  __shared__ long long seg_slots[CUT_W], seg_base[CUT_W];      // the scan's tables: two counts per word
  const int b = blockIdx.x, tid = threadIdx.x;
  const int M = a.M, n = a.n_min;
  const float* g = a.raw + (size_t)b * M * 3;
  // a thread owns a CONTIGUOUS run of points, so that a partition keeps the original order with one scan over threads
  const int chunk = (M + CUT_T - 1) / CUT_T;
  const int lo = tid * chunk < M ? tid * chunk : M, hi = lo + chunk < M ? lo + chunk : M;

  auto plane1 = [&](int k) {
    const double* nk = a.normals1 + ((size_t)b * a.K + k) * 3;
    return Plane{nk[0], nk[1], nk[2], a.zs1[(size_t)b * a.K + k]};
  };
  auto plane2 = [&](int t) {
    const double* nk = a.normals2 + ((size_t)b * DC_TRIES + t) * 3;
    return Plane{nk[0], nk[1], nk[2], a.zs2[(size_t)b * DC_TRIES + t]};
  };
  // points on side 1 of q; within > = 0: only among the points on side `within` of p
  auto count_up = [&](const Plane& q, int within, const Plane& p) {
    int c = 0;
    for (int j = lo; j < hi; ++j) {
      const float x = g[3 * j], y = g[3 * j + 1], z = g[3 * j + 2];
      const bool in = within < 0 || (int)is_up(x, y, z, p) == within;
      c += (in && is_up(x, y, z, q)) ? 1 : 0;
    }
    return block_sum(c, slots);
  };
  const double* u = a.u + (size_t)b * DC_UNIFORMS;
  const Plane none{0.0, 0.0, 0.0, 0.0};

  // 1-2: the first split and the piece that is cut again (every thread holds the same sums: the branches are uniform)
  Plane p1 = plane1(0), p2 = none;
  const int n_up = count_up(p1, -1, none), n_down = M - n_up;
  int seed = (int)floor(3.0 * u[0]);
  seed = seed > 2 ? 2 : seed;
  if (seed == 1 && n_up < a.n_rich) seed = 2;       // dataset.py:1214-1217, in this order: the second may undo the first
  if (seed == 2 && n_down < a.n_rich) seed = 1;
  // 4-5: the second cut and the kind
  int kind = SINGLE;
  int ut0 = R_UP, ut1 = 0, dt0 = R_DOWN, dt1 = 0;
  if (seed != 0) {
    const int inner = seed == 1 ? 1 : 0;
    const int n_in = inner ? n_up : n_down, n_other = M - n_in;
    int t2 = -1;
    for (int t = 0; t < DC_TRIES; ++t) {
      const Plane q = plane2(t);
      const int na = count_up(q, inner, p1), nb = n_in - na;
      if (na >= n && nb >= n) {
        t2 = t, p2 = q;
        break;
      }
    }
    if (t2 >= 0) {
      int se = (int)floor(3.0 * u[1]);
      se = se > 2 ? 2 : se;
      int choice = (int)floor(2.0 * u[2]);
      choice = choice > 1 ? 1 : choice;
      const int A = inner ? R_UP_UPPC : R_DOWN_UPPC, Bt = inner ? R_UP_DOWNPC : R_DOWN_DOWNPC, other = inner ? R_DOWN : R_UP;
      const int first = choice == 0 ? A : Bt, second = choice == 0 ? Bt : A;
      if (se == 0 || n_other < n)
        kind = HALF_VS_REST, ut0 = first, dt0 = second, dt1 = other;
      else if (se == 1)
        kind = HALF_VS_OTHER, ut0 = first, dt0 = other;
      else
        kind = HALVES, ut0 = A, dt0 = Bt;
    }
  }
  // 6: the single cut, `self.slice` starting from the split already made
  bool valid = true;
  if (kind == SINGLE) {
    valid = n_up >= n && n_down >= n;
    int best_k = 0, best_bal = n_up < n_down ? n_up : n_down;
    for (int k = 1; k < a.K && !valid; ++k) {
      const Plane q = plane1(k);
      const int up = count_up(q, -1, none);
      const int bal = up < M - up ? up : M - up;
      if (bal > best_bal) best_bal = bal, best_k = k;
      if (up >= n && M - up >= n) valid = true, best_k = k;
    }
    p1 = plane1(best_k);
  }

  // the pieces: U, D and - HALF_VS_OTHER only - the pair of plane 1 alone that replaces them when the boundaries do not touch
  const int n_pieces = kind == HALF_VS_OTHER ? 4 : 2;
  bool fits = true;
  for (int p = 0; p < 4; ++p) {
    float* dst = a.pieces + ((size_t)p * a.B + b) * a.cap * 3;
    if (p >= n_pieces) {      // no such piece: rows of the cloud's first point, count -1 (the sampling skips it)
      pad_piece(dst, 0, a.cap, g);
      if (tid == 0) a.counts[(size_t)p * a.B + b] = -1, a.start[(size_t)p * a.B + b] = 0;
      continue;
    }
    const int t0 = p == 0 ? ut0 : (p == 1 ? dt0 : (p == 2 ? R_UP : R_DOWN));
    const int t1 = p == 0 ? ut1 : (p == 1 ? dt1 : 0);
    // rows of either segment in this thread's run, and their exclusive scan over the workgroup (both counts in one word)
    int c0 = 0, c1 = 0;
    for (int j = lo; j < hi; ++j) {
      const float x = g[3 * j], y = g[3 * j + 1], z = g[3 * j + 2];
      const int s = segment(2 * (int)is_up(x, y, z, p1) + (int)is_up(x, y, z, p2), t0, t1);
      c0 += s == 0, c1 += s == 1;
    }
    // (each half counts at most M < 2^31 points, so no carry crosses from the low count into the high one)
    const long long excl = block_excl_scan((long long)c0 | ((long long)c1 << 32), seg_slots, seg_base);
    const long long tot = seg_slots[0];
    const int n0 = (int)(tot & 0xffffffffll), cnt = n0 + (int)(tot >> 32);
    int at0 = (int)(excl & 0xffffffffll);            // rows of the first region in front of this run
    int at1 = n0 + (int)(excl >> 32);                // the second region follows the whole first one
    for (int j = lo; j < hi; ++j) {
      const float x = g[3 * j], y = g[3 * j + 1], z = g[3 * j + 2];
      const int s = segment(2 * (int)is_up(x, y, z, p1) + (int)is_up(x, y, z, p2), t0, t1);
      const int at = s == 0 ? at0 : at1;
      if (s < 2 && at < a.cap) dst[(size_t)at * 3] = x, dst[(size_t)at * 3 + 1] = y, dst[(size_t)at * 3 + 2] = z;
      at0 += s == 0, at1 += s == 1;
    }
    __syncthreads();      // the piece's first row is in memory for this workgroup
    pad_piece(dst, cnt, a.cap, g);
    fits = fits && cnt <= a.cap;
    if (tid == 0) {
      a.counts[(size_t)p * a.B + b] = cnt;
      a.start[(size_t)p * a.B + b] = start_index(u[3 + p], cnt);
    }
  }
  if (tid == 0) {
    a.kind[b] = kind;
    double* pl = a.planes + (size_t)b * 8;
    pl[0] = p1.n0, pl[1] = p1.n1, pl[2] = p1.n2, pl[3] = p1.off;
    pl[4] = p2.n0, pl[5] = p2.n1, pl[6] = p2.n2, pl[7] = p2.off;
    int32_t* tb = a.tabs + (size_t)b * 4;
    tb[0] = ut0, tb[1] = ut1, tb[2] = dt0, tb[3] = dt1;
    a.ok[b] = (valid && fits) ? 1 : 0;
  }
}

}  // namespace

PZN_EXPORT int pzn_cut_compact_double_f32(const float* raw, const double* normals1, const double* zs1, const double* normals2,
                                          const double* zs2, const double* u, int B, int M, int K, int n_min, int n_rich, int cap,
                                          float* pieces, int64_t* counts, int64_t* start, int32_t* kind, double* planes,
                                          int32_t* tabs, uint8_t* ok, pzn_stream_t stream) {
  PZN_CHECK_ARG(raw && normals1 && zs1 && normals2 && zs2 && u && pieces && counts && start && kind && planes && tabs && ok);
  PZN_CHECK_ARG(B > 0 && M > 0 && K > 0 && cap > 0 && n_min >= 0 && n_rich >= 0);
  DoubleCutArgs a{raw, normals1, zs1, normals2, zs2, u, B, M, K, n_min, n_rich, cap, pieces, counts, start, kind, planes, tabs, ok};
  PZN_LAUNCH(cut_compact_double_kernel, dim3(B), dim3(CUT_T), 0, pzn_hip_stream(stream), a);
  PZN_RETURN_LAUNCH_STATUS();
}
