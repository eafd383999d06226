// fracture.hip — a cloud cut into P pieces with ground truth, one launch per batch (no counterpart in the reference, which
// ships pairs only; the multi-piece assembly of assembly.py is what consumes it).
//
// One workgroup per sample runs datapipe.fracture_rule (the numpy statement of this kernel): all points start with label 0;
// step s = 1 .. P-1 cuts the TARGET, the label with the most points so far (ties: the lowest), by the first of K candidate
// planes that leaves >= n_min target points on both sides (none: the most balanced one, the first among equals, ok = 0); the
// up side keeps the target's label, the down side becomes s.  A candidate plane goes through an ANCHOR, the target's r-th
// point in the cloud's order (r from a uniform draw): a plane drawn around the origin need not meet a sub-piece, one through
// a point of it always does, and the offset -((x n0 + y n1) + z n2) of one point is reproducible to the bit where a centroid
// would depend on the order of a sum.  The side test is the plane cut's (float64, every operation individually rounded, no
// fma), so the anchor evaluates to exactly 0 and is on the up side.
//
// A thread owns a contiguous run of <= 64 points (M <= 65536) as the other cut kernels do and is the only one that reads or
// writes its run's labels, which live in LDS, one byte per point (a register array indexed by a run-time j would go to
// scratch); the per-label counts are registers that every thread holds alike (the sums come from block_sum), so every branch
// on them is uniform.  Per step: the run's target members as one bit mask, ONE exclusive scan of their counts for all K anchor
// ranks (the thread whose run holds rank r_k writes that point to a small LDS table, FR_KC candidates at a time), then one
// pass over the members and a block_sum per candidate.  The P-way stable partition at the end is the same exclusive scan, once
// per label; the same pass writes `order`, the first one `label`.  Side test, workgroup sum, exclusive scan, start index and
// padding come from pzn_cut.h.
//
// fracture_pair_kernel (datapipe.fracture_pair_rule; the loader's PairFeeder(pieces=...)) runs the same steps, one
// __device__ function for both kernels, for a per-sample number of pieces, chooses a training pair on the device - the two
// sides of the last cut, or a drawn pair of final pieces with those two as its fallback - and partitions the <= 4 chosen
// labels only: no `order`, no other piece.
//
// fracture_curved_kernel / fracture_pair_curved_kernel (datapipe.fracture_curved_rule / fracture_pair_curved_rule) are the same
// two bodies with a curved candidate in the plane's place: a paraboloid through the anchor (Quadric, pzn_cut.h) in a frame and
// with two half curvatures that the host draws per candidate.  The steps and both bodies are templates over what cuts
// (PlaneCuts, QuadricCuts).  Frame and curvatures are uniform reads per candidate, as the normal is; the anchor table's fourth
// column, which the planes leave unused, carries the anchor's cloud row; the LDS layout and the launch geometry are those of
// the plane kernels.
//
// The four *_eroded kernels (datapipe.fracture_eroded_rule / fracture_pair_eroded_rule) are the same two bodies again, with cuts
// along which material is lost (Eroded<PlaneRowCuts>, Eroded<QuadricCuts>): per candidate a member of the target is up, down or
// lost - a band around the surface and a chip around the anchor, from the value whose sign the side test takes - and a candidate
// is judged by what it leaves on both sides, two counts that one workgroup sum carries in the halves of a 64-bit word.  The lost
// points get label 255, are counted for no piece and are never targeted again; a step that finds its target empty is not made.
// `order` takes one more scan, for the lost rows behind the last piece.  Every erosion branch is an `if constexpr` on the cuts'
// type, so the kernels without erosion are the code they were.
#include "pzn_common.h"

namespace {

#include "pzn_cut.h"

constexpr int FR_MAX_P = 16;         // pieces per sample
constexpr int FR_MAX_M = 65536;      // points per sample: runs of <= 64 points, one membership mask per thread
constexpr int FR_KC = 16;            // anchors held in LDS at a time
constexpr int FR_LOST = 255;         // the label of a point lost along a cut (P <= 16 leaves it free)
// the dynamic LDS region: every table at a multiple of 16 bytes, the labels last
constexpr int FR_SLOTS = 0, FR_WBASE = FR_SLOTS + CUT_W * 4, FR_ANCHOR = FR_WBASE + CUT_W * 4, FR_LABELS = FR_ANCHOR + FR_KC * 4 * 4;

// What cuts: the candidates' draws as the host lays them out, [B, P-1, K, ...].
//   at(step, c)                the same tables from row `step` on, which is candidate c = K step (a sample's first step, or a
//                              step of a sample)
//   ROWS                       the anchor table's fourth column holds the anchor's cloud row
//   through(k, anchor)         candidate k of the step as a surface through the anchor, a row of the LDS table
//   keep(surface)              what is held of a candidate that may be the one taken (uniform)
//   record(taken, k, g, pl)    thread 0 only, on the step's tables: the step's row of `planes` (and of `anchor`)
//   zero_from(i, n)            the whole workgroup, on the sample's tables: rows i .. n-1 of what record writes beside `planes`
//   ERODED                     material is lost along the cut (Eroded<...> below)
struct PlaneCuts {
  const double* normals;     // [B, P-1, K, 3]
  static constexpr bool ROWS = false;
  static constexpr bool ERODED = false;
  using Taken = Plane;
  __device__ __forceinline__ PlaneCuts at(size_t, size_t c) const { return PlaneCuts{normals + c * 3}; }
  // the plane through the anchor: the anchor itself evaluates to d + (-d) = 0
  __device__ __forceinline__ Plane through(int k, const float* anchor) const {
    const double n0 = normals[3 * k], n1 = normals[3 * k + 1], n2 = normals[3 * k + 2];
    const double ax = (double)anchor[0], ay = (double)anchor[1], az = (double)anchor[2];
    return Plane{n0, n1, n2, -__dadd_rn(__dadd_rn(__dmul_rn(ax, n0), __dmul_rn(ay, n1)), __dmul_rn(az, n2))};
  }
  static __device__ __forceinline__ const Plane& side(const Plane& q) { return q; }
  static __device__ __forceinline__ Plane keep(const Plane& q) { return q; }
  __device__ __forceinline__ void record(const Plane& taken, int, const float*, double* pl) const {
    pl[0] = taken.n0, pl[1] = taken.n1, pl[2] = taken.n2, pl[3] = taken.off;
  }
  __device__ __forceinline__ void zero_from(int, int) const {}
};

struct QuadricCuts {
  const double* frames;      // [B, P-1, K, 3, 3]: rows e1, e2, n
  const double* half_curv;   // [B, P-1, K, 2]
  int32_t* anchor;           // [B, P-1]: the cloud row of the anchor taken
  static constexpr bool ROWS = true;
  static constexpr bool ERODED = false;
  struct Through {
    Quadric q;
    int row;                 // the anchor's cloud row
  };
  static __device__ __forceinline__ void centre(const Through& t, double (&a)[3]) { a[0] = t.q.a0, a[1] = t.q.a1, a[2] = t.q.a2; }
  using Taken = int;         // the anchor's row is all that is held: thread 0 makes the tangent plane from it once per step
  __device__ __forceinline__ QuadricCuts at(size_t step, size_t c) const {
    return QuadricCuts{frames + c * 9, half_curv + c * 2, anchor + step};
  }
  __device__ __forceinline__ Through through(int k, const float* anchor_row) const {
    const double* f = frames + 9 * k;
    return Through{Quadric{(double)anchor_row[0], (double)anchor_row[1], (double)anchor_row[2], {f[0], f[1], f[2]},
                           {f[3], f[4], f[5]}, {f[6], f[7], f[8]}, half_curv[2 * k], half_curv[2 * k + 1]},
                   __float_as_int(anchor_row[3])};
  }
  static __device__ __forceinline__ const Quadric& side(const Through& t) { return t.q; }
  static __device__ __forceinline__ int keep(const Through& t) { return t.row; }
  // the tangent plane at the anchor: (n, -((ax n0 + ay n1) + az n2))
  __device__ __forceinline__ void record(int row, int k, const float* g, double* pl) const {
    const double n0 = frames[9 * k + 6], n1 = frames[9 * k + 7], n2 = frames[9 * k + 8];
    const double ax = (double)g[3 * row], ay = (double)g[3 * row + 1], az = (double)g[3 * row + 2];
    pl[0] = n0, pl[1] = n1, pl[2] = n2, pl[3] = -__dadd_rn(__dadd_rn(__dmul_rn(ax, n0), __dmul_rn(ay, n1)), __dmul_rn(az, n2));
    anchor[0] = row;
  }
  __device__ __forceinline__ void zero_from(int i, int n) const {
    for (i += threadIdx.x; i < n; i += CUT_T) anchor[i] = 0;
  }
};

// PlaneCuts that hold on to the anchor, as an eroded cut needs it: its coordinates are the chip's centre, its cloud row is reported.
struct PlaneRowCuts {
  const double* normals;     // [B, P-1, K, 3]
  int32_t* anchor;           // [B, P-1]: the cloud row of the anchor taken
  static constexpr bool ROWS = true;
  struct Through {
    Plane p;
    double a0, a1, a2;       // the anchor
    int row;                 // its cloud row
  };
  struct Taken {
    Plane p;
    int row;
  };
  __device__ __forceinline__ PlaneRowCuts at(size_t step, size_t c) const { return PlaneRowCuts{normals + c * 3, anchor + step}; }
  __device__ __forceinline__ Through through(int k, const float* anchor_row) const {
    const double n0 = normals[3 * k], n1 = normals[3 * k + 1], n2 = normals[3 * k + 2];
    const double ax = (double)anchor_row[0], ay = (double)anchor_row[1], az = (double)anchor_row[2];
    return Through{Plane{n0, n1, n2, -__dadd_rn(__dadd_rn(__dmul_rn(ax, n0), __dmul_rn(ay, n1)), __dmul_rn(az, n2))}, ax, ay, az,
                   __float_as_int(anchor_row[3])};
  }
  static __device__ __forceinline__ const Plane& side(const Through& t) { return t.p; }
  static __device__ __forceinline__ void centre(const Through& t, double (&a)[3]) { a[0] = t.a0, a[1] = t.a1, a[2] = t.a2; }
  static __device__ __forceinline__ Taken keep(const Through& t) { return Taken{t.p, t.row}; }
  __device__ __forceinline__ void record(const Taken& taken, int, const float*, double* pl) const {
    pl[0] = taken.p.n0, pl[1] = taken.p.n1, pl[2] = taken.p.n2, pl[3] = taken.p.off;
    anchor[0] = taken.row;
  }
  __device__ __forceinline__ void zero_from(int i, int n) const {
    for (i += threadIdx.x; i < n; i += CUT_T) anchor[i] = 0;
  }
};

// Cuts along which material is lost (datapipe.fracture_eroded_rule): Base's candidates, and per step (w_up, w_dn, depth, rho).  With
// f the value whose sign the side test takes, a member of the target is LOST under a candidate iff -w_dn < f < w_up (the band) or
// -depth < f < depth and |x - anchor|^2 < rho rho (the chip), all comparisons strict, so zeros and NaNs lose nothing.  Base holds
// the anchor (ROWS, centre, `anchor`): PlaneRowCuts or QuadricCuts.
//   lost_to(q, f, x, y, z)     the member with value f is lost under the surface q
//   skip()                     thread 0 only, on the step's tables: a step that is not made (zero rows)
template <class Base>
struct Eroded : Base {
  const double* erode;       // [B, P-1, 4]
  int32_t* lost;             // [B, P-1]: the points lost at every step
  static constexpr bool ERODED = true;
  __device__ __forceinline__ Eroded at(size_t step, size_t c) const { return Eroded{Base::at(step, c), erode + step * 4, lost + step}; }
  __device__ __forceinline__ bool lost_to(const typename Base::Through& q, double f, float x, float y, float z) const {
    const double w_up = erode[0], w_dn = erode[1], depth = erode[2], rho = erode[3];
    double a[3];
    Base::centre(q, a);
    const double d0 = __dsub_rn((double)x, a[0]), d1 = __dsub_rn((double)y, a[1]), d2 = __dsub_rn((double)z, a[2]);
    const double r2 = __dadd_rn(__dadd_rn(__dmul_rn(d0, d0), __dmul_rn(d1, d1)), __dmul_rn(d2, d2));
    return (f < w_up && f > -w_dn) || (f < depth && f > -depth && r2 < __dmul_rn(rho, rho));
  }
  __device__ __forceinline__ void skip() const { this->anchor[0] = 0, lost[0] = 0; }
  __device__ __forceinline__ void zero_from(int i, int n) const {
    Base::zero_from(i, n);
    for (i += threadIdx.x; i < n; i += CUT_T) lost[i] = 0;
  }
};

template <class Cuts>
struct FractureArgs {
  const float* raw;          // [B, M, 3]
  Cuts cuts;                 // [B, P-1, K, ...]
  const double* u_anchor;    // [B, P-1, K]
  const double* u_start;     // [B, P]
  int B, M, P, K, n_min, cap;
  float* pieces;             // [P B, cap, 3]: piece p of sample b at row p B + b
  int64_t* counts;           // [P B]
  int64_t* start;            // [P B]
  uint8_t* label;            // [B, M]
  int32_t* order;            // [B, M]
  double* planes;            // [B, P-1, 4]
  int32_t* target;           // [B, P-1]
  int32_t* cand;             // [B, P-1]
  uint8_t* ok;               // [B]
};

// What a workgroup of either kernel holds about its sample: the dynamic LDS region cut into its tables, and the run of points
// this thread owns.
struct FractureBlock {
  int* slots;
  int* wave_base;
  float* anchor;             // [FR_KC][4]
  uint8_t* lab;              // [M]
  const float* g;            // the sample's cloud
  int lo, hi;                // this thread's run of points
};

__device__ __forceinline__ FractureBlock fracture_block(unsigned char* smem, const float* raw, int M) {
  FractureBlock w;
  w.slots = reinterpret_cast<int*>(smem + FR_SLOTS);
  w.wave_base = reinterpret_cast<int*>(smem + FR_WBASE);
  w.anchor = reinterpret_cast<float*>(smem + FR_ANCHOR);
  w.lab = smem + FR_LABELS;
  w.g = raw + (size_t)blockIdx.x * M * 3;
  // a thread owns a CONTIGUOUS run of points, so that a partition keeps the original order with one scan over threads
  const int tid = threadIdx.x, chunk = (M + CUT_T - 1) / CUT_T;      // <= 64
  w.lo = tid * chunk < M ? tid * chunk : M;
  w.hi = w.lo + chunk < M ? w.lo + chunk : M;
  return w;
}

// Steps s = 1 .. steps of the rule on sample blockIdx.x (every kernel; steps <= P - 1, uniform over the workgroup): the labels in
// w.lab, the counts per label in cnt (the same in every thread), planes / target / cand rows 0 .. steps - 1 written by thread 0.
// cuts0, ua0: the sample's candidates [P-1,K,...] and anchor draws [P-1,K]; planes, target, cand: the sample's rows.  last_t: the
// target of the last step.  -> every step had a valid candidate
template <class Cuts>
__device__ __forceinline__ bool fracture_cuts(const FractureBlock& w, const Cuts& cuts0, const double* ua0, int K, int n_min,
                                              int steps, int (&cnt)[FR_MAX_P], double* planes, int32_t* target, int32_t* cand,
                                              int& last_t) {
  int* slots = w.slots;
  int* wave_base = w.wave_base;
  float* anchor = w.anchor;
  uint8_t* lab = w.lab;
  const float* g = w.g;
  const int lo = w.lo, hi = w.hi, tid = threadIdx.x;
  bool all_valid = true;

  for (int s = 1; s <= steps; ++s) {
    // 1. the target: the first largest label among 0 .. s-1
    int t = 0, n_t = cnt[0];
#pragma unroll
    for (int p = 1; p < FR_MAX_P; ++p)
      if (p < s && cnt[p] > n_t) t = p, n_t = cnt[p];
    if constexpr (Cuts::ERODED) {
      // everything has been lost: the step is not made (uniform: every thread holds the same counts)
      if (n_t == 0) {
        if (tid == 0) {
          double* pl = planes + (size_t)(s - 1) * 4;
          pl[0] = pl[1] = pl[2] = pl[3] = 0.0;
          target[s - 1] = t, cand[s - 1] = 0;
          cuts0.at((size_t)(s - 1), (size_t)(s - 1) * K).skip();
        }
        all_valid = false;
        last_t = t;
        continue;
      }
    }
    uint64_t tbits = 0;      // the run's members of the target
    for (int j = lo; j < hi; ++j) tbits |= (uint64_t)(lab[j] == t ? 1 : 0) << (j - lo);
    const int c_t = __popcll(tbits);
    const int before = block_excl_scan(c_t, slots, wave_base);      // target members in front of this run

    const Cuts cuts = cuts0.at((size_t)(s - 1), (size_t)(s - 1) * K);
    const double* ua = ua0 + (size_t)(s - 1) * K;
    int chosen = -1, best_k = 0, best_bal = -1, best_up = 0;
    uint64_t sel = 0;        // the run's target members on the DOWN side of the candidate that is taken
    [[maybe_unused]] int best_dn = 0;              // eroded cuts: what is kept of the down side is no longer n_t - best_up,
    [[maybe_unused]] uint64_t sel_lost = 0;        // and the run's target members that are lost to the candidate taken
    typename Cuts::Taken taken{};
    for (int k0 = 0; k0 < K && chosen < 0; k0 += FR_KC) {
      // 2. the anchors of candidates k0 .. k0 + FR_KC - 1 (the table's readers of the chunk before are behind block_sum's barriers)
      const int kn = K - k0 < FR_KC ? K - k0 : FR_KC;
      for (int kk = 0; kk < kn; ++kk) {
        const int r = (int)start_index(ua[k0 + kk], n_t) - before;      // (n_t >= 1: the target is a largest label)
        if (r >= 0 && r < c_t) {
          uint64_t m = tbits;
          for (int i = 0; i < r; ++i) m &= m - 1;
          const int j = lo + __ffsll((unsigned long long)m) - 1;
          anchor[4 * kk] = g[3 * j], anchor[4 * kk + 1] = g[3 * j + 1], anchor[4 * kk + 2] = g[3 * j + 2];
          if constexpr (Cuts::ROWS) anchor[4 * kk + 3] = __int_as_float(j);
        }
      }
      __syncthreads();
      for (int kk = 0; kk < kn; ++kk) {
        const int k = k0 + kk;
        // 3. the surface through the anchor (the table is read here, in front of block_sum's barriers)
        const auto q = cuts.through(k, anchor + 4 * kk);
        int bal;
        bool valid;
        if constexpr (Cuts::ERODED) {
          // every member is up, down or lost; the kept members of both sides in one sum, one count per 32-bit half (<= 65536
          // each): slots and wave_base are adjacent and together hold CUT_W such words
          long long c = 0;
          uint64_t down = 0, gone = 0;
          for (uint64_t m = tbits; m != 0; m &= m - 1) {
            const int i = __ffsll((unsigned long long)m) - 1, j = lo + i;
            const float x = g[3 * j], y = g[3 * j + 1], z = g[3 * j + 2];
            const double f = value(x, y, z, Cuts::side(q));
            const bool lost = cuts.lost_to(q, f, x, y, z), above = f >= 0.0;
            c += lost ? 0ll : (above ? 1ll : 1ll << 32);
            down |= (uint64_t)(!lost && !above ? 1 : 0) << i;
            gone |= (uint64_t)(lost ? 1 : 0) << i;
          }
          // 4. as below, on what the candidate leaves on its two sides
          const long long both = block_sum(c, reinterpret_cast<long long*>(slots));
          const int up = (int)(both & 0xffffffffll), dn = (int)(both >> 32);
          bal = up < dn ? up : dn;
          valid = up >= n_min && dn >= n_min;
          if (bal > best_bal || valid) sel = down, sel_lost = gone, taken = Cuts::keep(q), best_up = up, best_dn = dn;
        } else {
          int c = 0;
          uint64_t down = 0;
          for (uint64_t m = tbits; m != 0; m &= m - 1) {
            const int i = __ffsll((unsigned long long)m) - 1, j = lo + i;
            const bool up = is_up(g[3 * j], g[3 * j + 1], g[3 * j + 2], Cuts::side(q));
            c += up ? 1 : 0;
            down |= (uint64_t)(up ? 0 : 1) << i;
          }
          // 4. the first valid candidate, else the most balanced one (uniform: every thread holds the same sum)
          const int up = block_sum(c, slots);
          bal = up < n_t - up ? up : n_t - up;
          valid = up >= n_min && n_t - up >= n_min;
          if (bal > best_bal || valid) sel = down, taken = Cuts::keep(q), best_up = up;
        }
        if (bal > best_bal) best_bal = bal, best_k = k;
        if (valid) {
          chosen = k;
          break;
        }
      }
    }
    all_valid = all_valid && chosen >= 0;
    if (chosen < 0) chosen = best_k;
    // 5. the down side becomes label s; what is lost belongs to no piece and is never counted or targeted again
    for (uint64_t m = sel; m != 0; m &= m - 1) lab[lo + __ffsll((unsigned long long)m) - 1] = (uint8_t)s;
    if constexpr (Cuts::ERODED)
      for (uint64_t m = sel_lost; m != 0; m &= m - 1) lab[lo + __ffsll((unsigned long long)m) - 1] = (uint8_t)FR_LOST;
#pragma unroll
    for (int p = 0; p < FR_MAX_P; ++p) {
      if (p == t) cnt[p] = best_up;
      if constexpr (Cuts::ERODED) {
        if (p == s) cnt[p] = best_dn;
      } else {
        if (p == s) cnt[p] = n_t - best_up;
      }
    }
    if (tid == 0) {
      cuts.record(taken, chosen, g, planes + (size_t)(s - 1) * 4);
      if constexpr (Cuts::ERODED) cuts.lost[0] = n_t - best_up - best_dn;
      target[s - 1] = t;
      cand[s - 1] = chosen;
    }
    last_t = t;
  }
  return all_valid;
}

template <class Cuts>
__device__ __forceinline__ void fracture_body(const FractureArgs<Cuts>& a, unsigned char* smem) {
  const int b = blockIdx.x, tid = threadIdx.x;
  const int M = a.M, P = a.P, K = a.K;
  const FractureBlock w = fracture_block(smem, a.raw, M);
  int* slots = w.slots;
  int* wave_base = w.wave_base;
  uint8_t* lab = w.lab;
  const float* g = w.g;
  const int lo = w.lo, hi = w.hi;
  for (int j = lo; j < hi; ++j) lab[j] = 0;

  int cnt[FR_MAX_P];          // points per label: the same in every thread; only ever indexed by unrolled loops (registers)
#pragma unroll
  for (int p = 0; p < FR_MAX_P; ++p) cnt[p] = p == 0 ? M : 0;
  int last_t = 0;
  const bool all_valid = fracture_cuts(w, a.cuts.at((size_t)b * (P - 1), (size_t)b * (P - 1) * K), a.u_anchor + (size_t)b * (P - 1) * K, K, a.n_min,
                                       P - 1, cnt, a.planes + (size_t)b * (P - 1) * 4, a.target + (size_t)b * (P - 1),
                                       a.cand + (size_t)b * (P - 1), last_t);

  // the pieces: a stable P-way partition, one scan per label; `order` is the same partition without the cap
  for (int j = lo; j < hi; ++j) a.label[(size_t)b * M + j] = lab[j];
  int32_t* ord = a.order + (size_t)b * M;
  const double* us = a.u_start + (size_t)b * P;
  bool fits = true;
  int off = 0;               // rows of the labels in front
  for (int p = 0; p < P; ++p) {
    float* dst = a.pieces + ((size_t)p * a.B + b) * a.cap * 3;
    int c = 0;
    for (int j = lo; j < hi; ++j) c += lab[j] == p ? 1 : 0;
    int at = block_excl_scan(c, slots, wave_base);      // rows of label p in front of this run
    const int n_p = slots[0];                           // == cnt[p]
    for (int j = lo; j < hi; ++j) {
      if (lab[j] != p) continue;
      if (at < a.cap) dst[(size_t)at * 3] = g[3 * j], dst[(size_t)at * 3 + 1] = g[3 * j + 1], dst[(size_t)at * 3 + 2] = g[3 * j + 2];
      ord[off + at] = j;
      ++at;
    }
    __syncthreads();         // the piece's first row is in memory for this workgroup
    pad_piece(dst, n_p, a.cap, g);
    fits = fits && n_p <= a.cap;
    if (tid == 0) {
      a.counts[(size_t)p * a.B + b] = n_p;
      a.start[(size_t)p * a.B + b] = start_index(us[p], n_p);
    }
    off += n_p;
  }
  if constexpr (Cuts::ERODED) {
    // `order` stays the stable argsort of the labels: the lost rows behind the last piece, in the cloud's order
    int c = 0;
    for (int j = lo; j < hi; ++j) c += lab[j] == FR_LOST ? 1 : 0;
    int at = block_excl_scan(c, slots, wave_base);
    for (int j = lo; j < hi; ++j)
      if (lab[j] == FR_LOST) ord[off + at++] = j;
  }
  if (tid == 0) a.ok[b] = (all_valid && fits) ? 1 : 0;
}

__global__ __launch_bounds__(CUT_T) void fracture_kernel(FractureArgs<PlaneCuts> a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  fracture_body(a, smem);
}

__global__ __launch_bounds__(CUT_T) void fracture_curved_kernel(FractureArgs<QuadricCuts> a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  fracture_body(a, smem);
}

// The training pair of a fractured sample (datapipe.fracture_pair_rule): the cuts of a P_b-piece fracture, the pair chosen on
// the device, and only the chosen pieces written - what a loader beside the training step needs of a fracture.
constexpr int FP_UNIFORMS = 7;       // u_kind, u_a, u_c, u_sU, u_sD, u_sFU, u_sFD
enum PairKind { SIBLING = 0, NEIGHBOUR = 1 };

template <class Cuts>
struct FracturePairArgs {
  const float* raw;          // [B, M, 3]
  Cuts cuts;                 // [B, P-1, K, ...]
  const double* u_anchor;    // [B, P-1, K]
  const int32_t* n_pieces;   // [B]: P_b, 2 .. P
  const double* u;           // [B, 7]
  double neighbours;
  int B, M, P, K, n_min, cap;
  float* pieces;             // [4B, cap, 3]: U, D, fallback U, fallback D
  int64_t* counts;           // [4B]: -1 = no such piece
  int64_t* start;            // [4B]
  int32_t* kind;             // [B]
  int32_t* pair;             // [B, 4]: the labels of the four pieces, -1 = none
  uint8_t* label;            // [B, M]
  double* planes;            // [B, P-1, 4]
  int32_t* target;           // [B, P-1]
  int32_t* cand;             // [B, P-1]
  uint8_t* ok;               // [B]
};

template <class Cuts>
__device__ __forceinline__ void fracture_pair_body(const FracturePairArgs<Cuts>& a, unsigned char* smem) {
  const int b = blockIdx.x, tid = threadIdx.x;
  const int M = a.M, P = a.P, K = a.K;
  const FractureBlock w = fracture_block(smem, a.raw, M);
  int* slots = w.slots;
  int* wave_base = w.wave_base;
  uint8_t* lab = w.lab;
  const float* g = w.g;
  const int lo = w.lo, hi = w.hi;
  for (int j = lo; j < hi; ++j) lab[j] = 0;

  // a count outside 2 .. P (the host refuses the ones it can see): no cut, no piece, ok = 0
  const int asked = a.n_pieces[b];
  const bool in_range = asked >= 2 && asked <= P;
  const int Pb = in_range ? asked : 1;
  int cnt[FR_MAX_P];          // points per label: the same in every thread; only ever indexed by unrolled loops (registers)
#pragma unroll
  for (int p = 0; p < FR_MAX_P; ++p) cnt[p] = p == 0 ? M : 0;
  double* planes = a.planes + (size_t)b * (P - 1) * 4;
  int32_t* target = a.target + (size_t)b * (P - 1);
  int32_t* cand = a.cand + (size_t)b * (P - 1);
  const Cuts cuts = a.cuts.at((size_t)b * (P - 1), (size_t)b * (P - 1) * K);
  int last_t = 0;
  const bool all_valid = fracture_cuts(w, cuts, a.u_anchor + (size_t)b * (P - 1) * K, K, a.n_min, Pb - 1, cnt, planes, target,
                                       cand, last_t);
  // the steps that were not made: zero rows
  for (int i = (Pb - 1) * 4 + tid; i < (P - 1) * 4; i += CUT_T) planes[i] = 0.0;
  for (int i = Pb - 1 + tid; i < P - 1; i += CUT_T) target[i] = 0, cand[i] = 0;
  cuts.zero_from(Pb - 1, P - 1);
  for (int j = lo; j < hi; ++j) a.label[(size_t)b * M + j] = lab[j];

  // the pair (uniform: every thread reads the same draws and holds the same last target)
  const double* u = a.u + (size_t)b * FP_UNIFORMS;
  int kind = SIBLING;
  int lab4[4] = {last_t, Pb - 1, -1, -1};      // U, D, fallback U, fallback D; the sibling pair: the two sides of the last cut
  if (Pb >= 3 && u[0] < a.neighbours) {
    int pa = (int)floor(u[1] * (double)Pb);
    pa = pa > Pb - 1 ? Pb - 1 : pa;
    int pc = (int)floor(u[2] * (double)(Pb - 1));
    pc = pc > Pb - 2 ? Pb - 2 : pc;
    pc += pc >= pa ? 1 : 0;
    const bool sibling = (pa == lab4[0] && pc == lab4[1]) || (pa == lab4[1] && pc == lab4[0]);
    if (!sibling) kind = NEIGHBOUR, lab4[2] = lab4[0], lab4[3] = lab4[1], lab4[0] = pa, lab4[1] = pc;
  }
  if (!in_range) lab4[0] = lab4[1] = -1;

  // the pieces: a stable partition of the chosen labels only, one scan each
  bool fits = true;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    float* dst = a.pieces + ((size_t)q * a.B + b) * a.cap * 3;
    const int lq = lab4[q];
    if (lq < 0) {            // no such piece: rows of the cloud's first point, count -1 (the sampling skips it)
      pad_piece(dst, 0, a.cap, g);
      if (tid == 0) a.counts[(size_t)q * a.B + b] = -1, a.start[(size_t)q * a.B + b] = 0;
      continue;
    }
    int c = 0;
    for (int j = lo; j < hi; ++j) c += lab[j] == lq ? 1 : 0;
    int at = block_excl_scan(c, slots, wave_base);      // rows of the label in front of this run
    const int n_p = slots[0];
    for (int j = lo; j < hi; ++j) {
      if (lab[j] != lq) continue;
      if (at < a.cap) dst[(size_t)at * 3] = g[3 * j], dst[(size_t)at * 3 + 1] = g[3 * j + 1], dst[(size_t)at * 3 + 2] = g[3 * j + 2];
      ++at;
    }
    __syncthreads();         // the piece's first row is in memory for this workgroup
    pad_piece(dst, n_p, a.cap, g);
    fits = fits && n_p <= a.cap;
    if (tid == 0) {
      a.counts[(size_t)q * a.B + b] = n_p;
      a.start[(size_t)q * a.B + b] = start_index(u[3 + q], n_p);
    }
  }
  if (tid == 0) {
    a.kind[b] = in_range ? kind : -1;
    int32_t* pr = a.pair + (size_t)b * 4;
    pr[0] = lab4[0], pr[1] = lab4[1], pr[2] = lab4[2], pr[3] = lab4[3];
    a.ok[b] = (in_range && all_valid && fits) ? 1 : 0;
  }
}

__global__ __launch_bounds__(CUT_T) void fracture_pair_kernel(FracturePairArgs<PlaneCuts> a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  fracture_pair_body(a, smem);
}

__global__ __launch_bounds__(CUT_T) void fracture_pair_curved_kernel(FracturePairArgs<QuadricCuts> a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  fracture_pair_body(a, smem);
}

__global__ __launch_bounds__(CUT_T) void fracture_eroded_kernel(FractureArgs<Eroded<PlaneRowCuts>> a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  fracture_body(a, smem);
}

__global__ __launch_bounds__(CUT_T) void fracture_curved_eroded_kernel(FractureArgs<Eroded<QuadricCuts>> a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  fracture_body(a, smem);
}

__global__ __launch_bounds__(CUT_T) void fracture_pair_eroded_kernel(FracturePairArgs<Eroded<PlaneRowCuts>> a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  fracture_pair_body(a, smem);
}

__global__ __launch_bounds__(CUT_T) void fracture_pair_curved_eroded_kernel(FracturePairArgs<Eroded<QuadricCuts>> a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  fracture_pair_body(a, smem);
}

// the dynamic LDS of every kernel here: <= 64.4 KiB
int fracture_lds(const void* kernel, int M, size_t* lds) {
  *lds = (size_t)FR_LABELS + ((size_t)M + 15) / 16 * 16;
  if (*lds > 64 * 1024 && hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)*lds) != hipSuccess)
    return PZN_ELAUNCH;
  return PZN_OK;
}

}  // namespace

PZN_EXPORT int pzn_fracture_supported(int M, int P, int K) {
  return (M >= 1 && M <= FR_MAX_M && P >= 2 && P <= FR_MAX_P && K >= 1) ? 1 : 0;
}

PZN_EXPORT int pzn_fracture_f32(const float* raw, const double* normals, const double* u_anchor, const double* u_start, int B,
                                int M, int P, int K, int n_min, int cap, float* pieces, int64_t* counts, int64_t* start,
                                uint8_t* label, int32_t* order, double* planes, int32_t* target, int32_t* cand, uint8_t* ok,
                                pzn_stream_t stream) {
  PZN_CHECK_ARG(raw && normals && u_anchor && u_start && pieces && counts && start && label && order && planes && target && cand && ok);
  PZN_CHECK_ARG(B > 0 && cap > 0 && n_min >= 0);
  if (!pzn_fracture_supported(M, P, K)) return PZN_EUNSUPPORTED;
  FractureArgs<PlaneCuts> a{raw, {normals}, u_anchor, u_start, B, M, P, K, n_min, cap, pieces, counts, start, label, order, planes,
                            target, cand, ok};
  size_t lds;
  if (fracture_lds(reinterpret_cast<const void*>(fracture_kernel), M, &lds) != PZN_OK) return PZN_ELAUNCH;
  PZN_LAUNCH(fracture_kernel, dim3(B), dim3(CUT_T), lds, pzn_hip_stream(stream), a);
  PZN_RETURN_LAUNCH_STATUS();
}

PZN_EXPORT int pzn_fracture_curved_supported(int M, int P, int K) { return pzn_fracture_supported(M, P, K); }

PZN_EXPORT int pzn_fracture_curved_f32(const float* raw, const double* frames, const double* half_curv, const double* u_anchor,
                                       const double* u_start, int B, int M, int P, int K, int n_min, int cap, float* pieces,
                                       int64_t* counts, int64_t* start, uint8_t* label, int32_t* order, double* planes,
                                       int32_t* target, int32_t* cand, int32_t* anchor, uint8_t* ok, pzn_stream_t stream) {
  PZN_CHECK_ARG(raw && frames && half_curv && u_anchor && u_start && pieces && counts && start && label && order && planes &&
                target && cand && anchor && ok);
  PZN_CHECK_ARG(B > 0 && cap > 0 && n_min >= 0);
  if (!pzn_fracture_curved_supported(M, P, K)) return PZN_EUNSUPPORTED;
  FractureArgs<QuadricCuts> a{raw, {frames, half_curv, anchor}, u_anchor, u_start, B, M, P, K, n_min, cap, pieces, counts, start,
                              label, order, planes, target, cand, ok};
  size_t lds;
  if (fracture_lds(reinterpret_cast<const void*>(fracture_curved_kernel), M, &lds) != PZN_OK) return PZN_ELAUNCH;
  PZN_LAUNCH(fracture_curved_kernel, dim3(B), dim3(CUT_T), lds, pzn_hip_stream(stream), a);
  PZN_RETURN_LAUNCH_STATUS();
}

PZN_EXPORT int pzn_fracture_pair_supported(int M, int P, int K) { return pzn_fracture_supported(M, P, K); }

PZN_EXPORT int pzn_fracture_pair_f32(const float* raw, const double* normals, const double* u_anchor, const int32_t* n_pieces,
                                     const double* u, double neighbours, int B, int M, int P, int K, int n_min, int cap,
                                     float* pieces, int64_t* counts, int64_t* start, int32_t* kind, int32_t* pair, uint8_t* label,
                                     double* planes, int32_t* target, int32_t* cand, uint8_t* ok, pzn_stream_t stream) {
  PZN_CHECK_ARG(raw && normals && u_anchor && n_pieces && u && pieces && counts && start && kind && pair && label && planes &&
                target && cand && ok);
  PZN_CHECK_ARG(B > 0 && cap > 0 && n_min >= 0 && neighbours >= 0.0 && neighbours <= 1.0);
  if (!pzn_fracture_pair_supported(M, P, K)) return PZN_EUNSUPPORTED;
  FracturePairArgs<PlaneCuts> a{raw, {normals}, u_anchor, n_pieces, u, neighbours, B, M, P, K, n_min, cap, pieces, counts, start,
                                kind, pair, label, planes, target, cand, ok};
  size_t lds;
  if (fracture_lds(reinterpret_cast<const void*>(fracture_pair_kernel), M, &lds) != PZN_OK) return PZN_ELAUNCH;
  PZN_LAUNCH(fracture_pair_kernel, dim3(B), dim3(CUT_T), lds, pzn_hip_stream(stream), a);
  PZN_RETURN_LAUNCH_STATUS();
}

PZN_EXPORT int pzn_fracture_pair_curved_supported(int M, int P, int K) { return pzn_fracture_supported(M, P, K); }

PZN_EXPORT int pzn_fracture_pair_curved_f32(const float* raw, const double* frames, const double* half_curv, const double* u_anchor,
                                            const int32_t* n_pieces, const double* u, double neighbours, int B, int M, int P, int K,
                                            int n_min, int cap, float* pieces, int64_t* counts, int64_t* start, int32_t* kind,
                                            int32_t* pair, uint8_t* label, double* planes, int32_t* target, int32_t* cand,
                                            int32_t* anchor, uint8_t* ok, pzn_stream_t stream) {
  PZN_CHECK_ARG(raw && frames && half_curv && u_anchor && n_pieces && u && pieces && counts && start && kind && pair && label &&
                planes && target && cand && anchor && ok);
  PZN_CHECK_ARG(B > 0 && cap > 0 && n_min >= 0 && neighbours >= 0.0 && neighbours <= 1.0);
  if (!pzn_fracture_pair_curved_supported(M, P, K)) return PZN_EUNSUPPORTED;
  FracturePairArgs<QuadricCuts> a{raw, {frames, half_curv, anchor}, u_anchor, n_pieces, u, neighbours, B, M, P, K, n_min, cap,
                                  pieces, counts, start, kind, pair, label, planes, target, cand, ok};
  size_t lds;
  if (fracture_lds(reinterpret_cast<const void*>(fracture_pair_curved_kernel), M, &lds) != PZN_OK) return PZN_ELAUNCH;
  PZN_LAUNCH(fracture_pair_curved_kernel, dim3(B), dim3(CUT_T), lds, pzn_hip_stream(stream), a);
  PZN_RETURN_LAUNCH_STATUS();
}

PZN_EXPORT int pzn_fracture_eroded_supported(int M, int P, int K) { return pzn_fracture_supported(M, P, K); }

PZN_EXPORT int pzn_fracture_eroded_f32(const float* raw, const double* normals, const double* frames, const double* half_curv,
                                       const double* u_anchor, const double* u_start, const double* erode, int B, int M, int P,
                                       int K, int n_min, int cap, float* pieces, int64_t* counts, int64_t* start, uint8_t* label,
                                       int32_t* order, double* planes, int32_t* target, int32_t* cand, int32_t* anchor,
                                       int32_t* lost, uint8_t* ok, pzn_stream_t stream) {
  PZN_CHECK_ARG(raw && u_anchor && u_start && erode && pieces && counts && start && label && order && planes && target && cand &&
                anchor && lost && ok);
  // planes (normals) or surfaces (frames and half_curv), never both and never half of one
  PZN_CHECK_ARG(normals ? (!frames && !half_curv) : (frames && half_curv));
  PZN_CHECK_ARG(B > 0 && cap > 0 && n_min >= 0);
  if (!pzn_fracture_eroded_supported(M, P, K)) return PZN_EUNSUPPORTED;
  size_t lds;
  if (normals) {
    FractureArgs<Eroded<PlaneRowCuts>> a{raw, {{normals, anchor}, erode, lost}, u_anchor, u_start, B, M, P, K, n_min, cap, pieces,
                                         counts, start, label, order, planes, target, cand, ok};
    if (fracture_lds(reinterpret_cast<const void*>(fracture_eroded_kernel), M, &lds) != PZN_OK) return PZN_ELAUNCH;
    PZN_LAUNCH(fracture_eroded_kernel, dim3(B), dim3(CUT_T), lds, pzn_hip_stream(stream), a);
  } else {
    FractureArgs<Eroded<QuadricCuts>> a{raw, {{frames, half_curv, anchor}, erode, lost}, u_anchor, u_start, B, M, P, K, n_min, cap,
                                        pieces, counts, start, label, order, planes, target, cand, ok};
    if (fracture_lds(reinterpret_cast<const void*>(fracture_curved_eroded_kernel), M, &lds) != PZN_OK) return PZN_ELAUNCH;
    PZN_LAUNCH(fracture_curved_eroded_kernel, dim3(B), dim3(CUT_T), lds, pzn_hip_stream(stream), a);
  }
  PZN_RETURN_LAUNCH_STATUS();
}

PZN_EXPORT int pzn_fracture_pair_eroded_supported(int M, int P, int K) { return pzn_fracture_supported(M, P, K); }

PZN_EXPORT int pzn_fracture_pair_eroded_f32(const float* raw, const double* normals, const double* frames, const double* half_curv,
                                            const double* u_anchor, const int32_t* n_pieces, const double* u, const double* erode,
                                            double neighbours, int B, int M, int P, int K, int n_min, int cap, float* pieces,
                                            int64_t* counts, int64_t* start, int32_t* kind, int32_t* pair, uint8_t* label,
                                            double* planes, int32_t* target, int32_t* cand, int32_t* anchor, int32_t* lost,
                                            uint8_t* ok, pzn_stream_t stream) {
  PZN_CHECK_ARG(raw && u_anchor && n_pieces && u && erode && pieces && counts && start && kind && pair && label && planes && target &&
                cand && anchor && lost && ok);
  PZN_CHECK_ARG(normals ? (!frames && !half_curv) : (frames && half_curv));
  PZN_CHECK_ARG(B > 0 && cap > 0 && n_min >= 0 && neighbours >= 0.0 && neighbours <= 1.0);
  if (!pzn_fracture_pair_eroded_supported(M, P, K)) return PZN_EUNSUPPORTED;
  size_t lds;
  if (normals) {
    FracturePairArgs<Eroded<PlaneRowCuts>> a{raw, {{normals, anchor}, erode, lost}, u_anchor, n_pieces, u, neighbours, B, M, P, K,
                                             n_min, cap, pieces, counts, start, kind, pair, label, planes, target, cand, ok};
    if (fracture_lds(reinterpret_cast<const void*>(fracture_pair_eroded_kernel), M, &lds) != PZN_OK) return PZN_ELAUNCH;
    PZN_LAUNCH(fracture_pair_eroded_kernel, dim3(B), dim3(CUT_T), lds, pzn_hip_stream(stream), a);
  } else {
    FracturePairArgs<Eroded<QuadricCuts>> a{raw, {{frames, half_curv, anchor}, erode, lost}, u_anchor, n_pieces, u, neighbours, B, M,
                                            P, K, n_min, cap, pieces, counts, start, kind, pair, label, planes, target, cand, ok};
    if (fracture_lds(reinterpret_cast<const void*>(fracture_pair_curved_eroded_kernel), M, &lds) != PZN_OK) return PZN_ELAUNCH;
    PZN_LAUNCH(fracture_pair_curved_eroded_kernel, dim3(B), dim3(CUT_T), lds, pzn_hip_stream(stream), a);
  }
  PZN_RETURN_LAUNCH_STATUS();
}
