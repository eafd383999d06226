// pzn_cut.h — what the loader's three cut kernels share (datapipe.hip: plane, solidcut.hip: sphere / cylinder / cone,
// doublecut.hip: two planes) and fracture.hip (P pieces, along planes or paraboloids): the workgroup shape, the float64 side
// tests of a plane and of a paraboloid, the workgroup sum, the workgroup exclusive scan behind every stable partition, the FPS
// start index, the padding of a piece, and the whole single-cut body - the first valid of K candidates, else the most balanced
// one, written as a stable two-way partition.  Tests pin pieces, counts and start indices bit for bit, so each of these has this one
// definition.  Included inside the translation unit's anonymous namespace, after pzn_common.h; the translation units are
// built with -ffp-contract=off (float64, every operation individually rounded, like numpy).
#pragma once

constexpr int CUT_T = 1024;                  // threads of a cut kernel: one workgroup per sample
constexpr int CUT_W = CUT_T / PZN_WAVE;

struct Plane {
  double n0, n1, n2, off;
};

// points . normal + z as numpy evaluates it for float32 points times float64 draws: ((x n0 + y n1) + z n2) + offset - the signed
// offset of the point along the normal to the plane
__device__ __forceinline__ double value(float x, float y, float z, const Plane& p) {
  return __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn((double)x, p.n0), __dmul_rn((double)y, p.n1)), __dmul_rn((double)z, p.n2)), p.off);
}

// A second-order surface patch through the point a: the paraboloid h + c1 s1^2 + c2 s2^2 = 0 in the frame (e1, e2, n) at a,
// (s1, s2, h) the coordinates of x - a in that frame and c1, c2 HALF the two curvatures - a bowl (c1 c2 > 0), a cylinder
// (c2 = 0), a saddle (c1 c2 < 0) or the plane with normal n (0, 0).  The frame is taken as given.
struct Quadric {
  double a0, a1, a2;
  double e1[3], e2[3], n[3];
  double c1, c2;
};

// f(x) with d = x - a (the float32 coordinates widened, three subtractions), s1 = (d0 e1[0] + d1 e1[1]) + d2 e1[2], s2 and
// h likewise with e2 and n, f = (h + (c1 s1) s1) + (c2 s2) s2: float64, every operation individually rounded, as numpy
// evaluates it.  d = 0 at a, so a itself evaluates to exactly 0.
__device__ __forceinline__ double value(float x, float y, float z, const Quadric& q) {
  const double d0 = __dsub_rn((double)x, q.a0), d1 = __dsub_rn((double)y, q.a1), d2 = __dsub_rn((double)z, q.a2);
  const double s1 = __dadd_rn(__dadd_rn(__dmul_rn(d0, q.e1[0]), __dmul_rn(d1, q.e1[1])), __dmul_rn(d2, q.e1[2]));
  const double s2 = __dadd_rn(__dadd_rn(__dmul_rn(d0, q.e2[0]), __dmul_rn(d1, q.e2[1])), __dmul_rn(d2, q.e2[2]));
  const double h = __dadd_rn(__dadd_rn(__dmul_rn(d0, q.n[0]), __dmul_rn(d1, q.n[1])), __dmul_rn(d2, q.n[2]));
  return __dadd_rn(__dadd_rn(h, __dmul_rn(__dmul_rn(q.c1, s1), s1)), __dmul_rn(__dmul_rn(q.c2, s2), s2));
}

// the side test of either surface: value >= 0, so a point at exactly 0 (the anchor of a fracture's cut) is on the up side
template <class Surface>
__device__ __forceinline__ bool is_up(float x, float y, float z, const Surface& s) {
  return value(x, y, z, s) >= 0.0;
}

// sum of one count per thread over the workgroup, the same value returned to every thread (two barriers); slots: CUT_W counts of
// LDS.  Count: int, or long long holding two counts, one per 32-bit half, as block_excl_scan takes them.
template <class Count>
__device__ __forceinline__ Count block_sum(Count v, Count* slots) {
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, PZN_WAVE);
  __syncthreads();          // (slots may still be read from the previous call)
  if ((threadIdx.x & (PZN_WAVE - 1)) == 0) slots[threadIdx.x / PZN_WAVE] = v;
  __syncthreads();
  Count t = 0;
#pragma unroll
  for (int w = 0; w < CUT_W; ++w) t += slots[w];
  return t;
}

// exclusive scan of one count per thread over the workgroup in thread order (three barriers, the first for tables that may
// still be read from the call before); the total in slots[0].  slots, wave_base: CUT_W counts of LDS each.  Count: int, or
// long long holding two counts, one per 32-bit half, each of which stays below 2^31 (no carry crosses).
template <class Count>
__device__ __forceinline__ Count block_excl_scan(Count c, Count* slots, Count* wave_base) {
  const int lane = threadIdx.x & (PZN_WAVE - 1), wave = threadIdx.x / PZN_WAVE;
  Count incl = c;
  for (int d = 1; d < PZN_WAVE; d <<= 1) {
    const Count o = __shfl_up(incl, d, PZN_WAVE);
    if (lane >= d) incl += o;
  }
  __syncthreads();
  if (lane == PZN_WAVE - 1) slots[wave] = incl;
  __syncthreads();
  if (threadIdx.x == 0) {
    Count run = 0;
    for (int w = 0; w < CUT_W; ++w) wave_base[w] = run, run += slots[w];
    slots[0] = run;
  }
  __syncthreads();
  return wave_base[wave] + incl - c;
}

// np.random.randint(0, n_piece) from a uniform draw: floor(u n_piece) held to [0, n_piece - 1] (0 for an empty piece)
__device__ __forceinline__ long start_index(double u, int cnt) {
  long s = (long)floor(u * (double)cnt);
  s = s > cnt - 1 ? cnt - 1 : s;
  return s < 0 ? 0 : s;
}

// rows cnt .. cap - 1 of piece p: copies of its first row (which can never win farthest point sampling), of the cloud's first
// row g when the piece is empty.  By the whole workgroup, behind a barrier that follows the write of p's first row.
__device__ __forceinline__ void pad_piece(float* p, int cnt, int cap, const float* g) {
  const float* first = cnt > 0 ? p : g;
  const float fx = first[0], fy = first[1], fz = first[2];
  for (int r = (cnt < cap ? cnt : cap) + threadIdx.x; r < cap; r += CUT_T) p[3 * r] = fx, p[3 * r + 1] = fy, p[3 * r + 2] = fz;
}

// the part of a single cut's arguments that does not depend on what cuts
struct CutIO {
  const float* raw;        // [B, M, 3]
  const double* u;         // [B, 2]: start fractions (up, down)
  int B, M, K, n_min, cap;
  float* pieces;           // [2B, cap, 3]: rows 0..B-1 the up pieces, rows B..2B-1 the down pieces
  int64_t* counts;         // [2B]
  int64_t* start;          // [2B]
  uint8_t* ok;             // [B]: a candidate was valid (else: the most balanced candidate was taken)
};

// The single cut of sample blockIdx.x by a workgroup of CUT_T threads: the FIRST of the K candidates that leaves >= n_min
// points on both sides, else the most balanced one (the first among equals); both pieces in the cloud's point order, padded
// to `cap` rows; their sizes, start indices and `ok`.  `cut` says what cuts:
//   cut.load(k)             candidate k, in registers; called by every thread with the same k, may contain barriers
//   cut.test(cd, x, y, z)   the point is on the up side of candidate cd
//   cut.record(k)           thread 0 only: write what the kernel reports about the candidate that was taken
// A thread evaluates the predicate ONCE per point and candidate and keeps the bits of its run (<= 64 points, i.e. M <= 65536;
// beyond that the candidate taken is evaluated again for the scan and the write).  slots, wave_base: CUT_W ints of LDS each.
template <class Cut>
__device__ __forceinline__ void cut_compact_body(const CutIO& a, const Cut& cut, int* slots, int* wave_base) {
  const int b = blockIdx.x, tid = threadIdx.x;
  const int M = a.M;
  const float* g = a.raw + (size_t)b * M * 3;
  // a thread owns a CONTIGUOUS run of points, so that the partition keeps the original order with one scan over threads
  const int chunk = (M + CUT_T - 1) / CUT_T;
  const int lo = tid * chunk < M ? tid * chunk : M, hi = lo + chunk < M ? lo + chunk : M;
  const bool keep = chunk <= 64;      // the run's membership bits fit one register pair (uniform)

  int chosen = -1, best_k = 0, best_bal = -1;
  uint64_t sel = 0;                   // membership of this thread's run under the candidate that is taken
  for (int k = 0; k < a.K; ++k) {
    const auto cd = cut.load(k);
    int c = 0;
    uint64_t bits = 0;
    for (int j = lo; j < hi; ++j) {
      const bool in = cut.test(cd, g[3 * j], g[3 * j + 1], g[3 * j + 2]);
      c += in ? 1 : 0;
      bits |= (uint64_t)(in ? 1 : 0) << ((j - lo) & 63);
    }
    const int up = block_sum(c, slots);
    const int bal = up < M - up ? up : M - up;
    const bool valid = up >= a.n_min && M - up >= a.n_min;      // (uniform: every thread holds the same sum)
    if (bal > best_bal || valid) sel = bits;
    if (bal > best_bal) best_bal = bal, best_k = k;
    if (valid) {
      chosen = k;
      break;
    }
  }
  const bool valid = chosen >= 0;
  if (!valid) chosen = best_k;
  decltype(cut.load(0)) cd = {};
  if (!keep) cd = cut.load(chosen);      // (uniform)
  auto member = [&](int j) -> bool {
    return keep ? ((sel >> (j - lo)) & 1) != 0 : cut.test(cd, g[3 * j], g[3 * j + 1], g[3 * j + 2]);
  };

  // stable partition: exclusive scan of the per-thread up counts over the workgroup
  int c = 0;
  if (keep) c = __popcll(sel);
  else
    for (int j = lo; j < hi; ++j) c += member(j) ? 1 : 0;
  int up_at = block_excl_scan(c, slots, wave_base);      // ups in front of this thread's run
  const int n_up = slots[0], n_down = M - n_up;
  int down_at = lo - up_at;                    // downs in front of it
  float* pu = a.pieces + (size_t)b * a.cap * 3;
  float* pd = a.pieces + (size_t)(a.B + b) * a.cap * 3;
  for (int j = lo; j < hi; ++j) {
    const float x = g[3 * j], y = g[3 * j + 1], z = g[3 * j + 2];
    const bool up = member(j);
    const int at = up ? up_at : down_at;
    float* dst = (up ? pu : pd) + (size_t)at * 3;
    if (at < a.cap) dst[0] = x, dst[1] = y, dst[2] = z;
    up_at += up ? 1 : 0;
    down_at += up ? 0 : 1;
  }
  __syncthreads();      // the pieces' first rows are in memory for this workgroup
  pad_piece(pu, n_up, a.cap, g);
  pad_piece(pd, n_down, a.cap, g);
  if (tid == 0) {
    a.counts[b] = n_up;
    a.counts[a.B + b] = n_down;
    a.start[b] = start_index(a.u[2 * b], n_up);
    a.start[a.B + b] = start_index(a.u[2 * b + 1], n_down);
    cut.record(chosen);
    a.ok[b] = (valid && n_up <= a.cap && n_down <= a.cap) ? 1 : 0;
  }
}
