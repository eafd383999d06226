// solidcut.hip — the sphere / cylinder / cone cuts of the reference's loader (dataset.py:715-759, re-draw :1175-1179) as one
// launch per batch: the contract of cut_compact_kernel (datapipe.hip) with a solid in place of the plane.
//
// The reference keeps the points whose signed distance to a tessellated open3d mesh is negative, i.e. the points strictly
// inside a CONVEX polyhedron (oracle/solids.py: a UV sphere of 50 bands x 100 sectors, a 50-gon prism, a 50-gon pyramid):
// strictly on the inner side of every face plane.  The faces come in rotation families about the solid's axis, which
// leaves few planes to test (datapipe.solid_cut_mask states the same geometry through atan2 / acos; here no
// transcendental is evaluated per point):
//   * every side face of the prism / pyramid, and every face of band i of the sphere, has the outward normal
//     (a cos phi_j, a sin phi_j, c) with a > 0 and phi_j = (j + 1/2) step the mid-angle of sector j, so over the sectors the
//     binding face is the one with the largest t_j = x cos phi_j + y sin phi_j;
//   * the set of phi_j is symmetric under phi -> -phi and phi -> pi - phi, so max_j t_j = max over the phi_j in [0, pi/2] of
//     |x| cos phi_j + |y| sin phi_j: 13 of the 50-gon's normals, 25 of the sphere's 100;
//   * the sphere's bands mirror in z and a band of the other hemisphere never binds (its c has the other sign), so the 25
//     bands of one hemisphere are tested against |z|.
// That is the brute-force test over ALL faces with the equal and the implied ones left out.  Per workgroup the tables
// (sector cosines / sines, band normals and offsets) are computed once into LDS; per candidate one thread computes the
// rotation matrix.  A thread evaluates the predicate ONCE per point and candidate and keeps the bits of its run (<= 64 points,
// i.e. M <= 65536; beyond that the chosen candidate is evaluated again for the scan and the write).
// float64 throughout, every operation individually rounded (-ffp-contract=off), like the plane cut.
#include "pzn_common.h"

namespace {

constexpr int SC_T = 1024;
constexpr int SC_W = SC_T / PZN_WAVE;
constexpr int SC_RES = 50;                    // resolution of the three meshes (dataset.py:717, :733, :750)
constexpr int SC_SEC_MAX = SC_RES / 2;        // sphere: 25 of the 100 sector mid-angles lie in [0, pi/2]
constexpr int SC_BANDS = SC_RES / 2;          // sphere: 25 latitude bands per hemisphere
constexpr double SC_PI = 3.14159265358979323846;

enum { SOLID_SPHERE = 0, SOLID_CYLINDER = 1, SOLID_CONE = 2 };

struct SolidArgs {
  const float* raw;        // [B, M, 3]
  const double* params;    // [B, K, 6]: rot, shift
  const double* u;         // [B, 2]: start fractions (up, down)
  int B, M, K, n_min, cap;
  float* pieces;           // [2B, cap, 3]: rows 0..B-1 the up pieces (inside), rows B..2B-1 the down pieces
  int64_t* counts;         // [2B]
  int64_t* start;          // [2B]
  double* chosen;          // [B, 6]: rot, shift of the candidate that was taken
  int32_t* chosen_k;       // [B]: its index
  uint8_t* ok;             // [B]: a candidate was valid (else: the most balanced candidate was taken)
};

struct Tables {
  double sec_c[SC_SEC_MAX], sec_s[SC_SEC_MAX];                    // cos / sin of the sector mid-angles in [0, pi/2]
  double band_a[SC_BANDS], band_c[SC_BANDS], band_d[SC_BANDS];    // sphere: a m + c |z| < d, band i between rings i and i + 1
  double half_c;                                                  // cos(step / 2) of the 50-gon
  double cand[12];                                                // rotation (row-major) and shift of the current candidate
};

struct Cand {
  double r[9], s[3];
};

template <int KIND>
__device__ __forceinline__ constexpr int n_sectors() { return KIND == SOLID_SPHERE ? SC_RES / 2 : SC_RES / 4 + 1; }

template <int KIND>
__device__ void fill_tables(Tables& t) {
  const int tid = threadIdx.x;
  // sphere: 2 res meridians, sector step pi / res; prism and pyramid: a res-gon, step 2 pi / res
  const double step = KIND == SOLID_SPHERE ? SC_PI / SC_RES : 2.0 * SC_PI / SC_RES;
  if (tid < n_sectors<KIND>()) {
    const double phi = ((double)tid + 0.5) * step;
    t.sec_c[tid] = cos(phi), t.sec_s[tid] = sin(phi);
  }
  if (KIND == SOLID_SPHERE && tid < SC_BANDS) {
    // the face of band i in the sector centred at phi = 0 is the planar trapezoid (a triangle at the pole) with the corners
    // r (sin a_i cos(step/2), +- sin a_i sin(step/2), cos a_i) and the same on ring i + 1: its normal lies in the xz-plane,
    // perpendicular to the line through the two chord midpoints P_i = r (sin a_i cos(step/2), 0, cos a_i)
    const double r = 0.5, ch = cos(0.5 * step);
    const double a0 = (double)tid * step, a1 = (double)(tid + 1) * step;
    const double px = r * sin(a0) * ch, pz = r * cos(a0);
    double na = r * (cos(a0) - cos(a1)), nc = r * (sin(a1) - sin(a0)) * ch;
    const double len = sqrt(na * na + nc * nc);
    na /= len, nc /= len;
    t.band_a[tid] = na, t.band_c[tid] = nc, t.band_d[tid] = na * px + nc * pz;
  }
  if (tid == 0) t.half_c = cos(0.5 * step);
}

// open3d's get_rotation_matrix_from_axis_angle (Rodrigues: I + sin(th) K + (1 - cos(th)) K^2, K^2 = k k^T - I) and the shift of
// candidate p[6] -> t.cand, by ONE thread; then every thread's copy in registers.  Two barriers: the second also publishes
// the tables on first use.
template <int KIND>
__device__ Cand load_candidate(Tables& t, const double* p) {
  __syncthreads();      // (t.cand may still be read for the previous candidate)
  if (threadIdx.x == 0) {
    double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    if (KIND != SOLID_SPHERE) {
      const double wx = p[0], wy = p[1], wz = p[2];
      const double th = sqrt(wx * wx + wy * wy + wz * wz);
      if (th > 0.0) {
        const double kx = wx / th, ky = wy / th, kz = wz / th, s = sin(th), v = 1.0 - cos(th);
        R[0] = 1.0 + v * (kx * kx - 1.0), R[1] = -s * kz + v * (kx * ky), R[2] = s * ky + v * (kx * kz);
        R[3] = s * kz + v * (ky * kx), R[4] = 1.0 + v * (ky * ky - 1.0), R[5] = -s * kx + v * (ky * kz);
        R[6] = -s * ky + v * (kz * kx), R[7] = s * kx + v * (kz * ky), R[8] = 1.0 + v * (kz * kz - 1.0);
      }
    }
    for (int i = 0; i < 9; ++i) t.cand[i] = R[i];
    for (int i = 0; i < 3; ++i) t.cand[9 + i] = KIND == SOLID_CONE ? 0.0 : p[3 + i];      // (the cone is not translated by a draw)
  }
  __syncthreads();
  Cand c;
  for (int i = 0; i < 9; ++i) c.r[i] = t.cand[i];
  for (int i = 0; i < 3; ++i) c.s[i] = t.cand[9 + i];
  return c;
}

// strictly inside the moved polyhedron
template <int KIND>
__device__ __forceinline__ bool inside(const Tables& t, const Cand& c, float fx, float fy, float fz) {
  const double dx = (double)fx - c.s[0], dy = (double)fy - c.s[1], dz = (double)fz - c.s[2];
  double x = dx, y = dy, z = dz;
  if (KIND != SOLID_SPHERE) {      // mesh point = R x (+ shift): x = R^T (p - shift)
    x = (c.r[0] * dx + c.r[3] * dy) + c.r[6] * dz;
    y = (c.r[1] * dx + c.r[4] * dy) + c.r[7] * dz;
    z = (c.r[2] * dx + c.r[5] * dy) + c.r[8] * dz;
  }
  const double ax = fabs(x), ay = fabs(y);
  double m = 0.0;
  // (not unrolled in full: the tables would be hoisted into registers, 250 of them for the sphere, and spill)
#pragma unroll 4
  for (int j = 0; j < n_sectors<KIND>(); ++j) {
    const double tj = ax * t.sec_c[j] + ay * t.sec_s[j];
    m = tj > m ? tj : m;
  }
  if (KIND == SOLID_SPHERE) {
    const double az = fabs(z);
    bool in = true;
#pragma unroll 5
    for (int i = 0; i < SC_BANDS; ++i) in &= t.band_a[i] * m + t.band_c[i] * az < t.band_d[i];
    return in;
  }
  if (KIND == SOLID_CYLINDER) return m < 0.6 * t.half_c && fabs(z) < 0.5;      // create_cylinder(0.6, 1, 50)
  const double h = z + 1.0;      // create_cone(1, 2, 50) - (0,0,1): height above the base plane, apex at h = 2; the side plane
  return h > 0.0 && 2.0 * m + t.half_c * h < 2.0 * t.half_c;      // of a sector has the normal (2 cos phi, 2 sin phi, cos(step/2))
}

// sum of one int per thread over the workgroup, the same value returned to every thread (two barriers)
__device__ __forceinline__ int block_sum(int v, int* slots) {
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, PZN_WAVE);
  __syncthreads();          // (slots may still be read from the previous call)
  if ((threadIdx.x & (PZN_WAVE - 1)) == 0) slots[threadIdx.x / PZN_WAVE] = v;
  __syncthreads();
  int t = 0;
#pragma unroll
  for (int w = 0; w < SC_W; ++w) t += slots[w];
  return t;
}

template <int KIND>
__global__ __launch_bounds__(SC_T) void cut_compact_solid_kernel(SolidArgs a) {
  __shared__ Tables tab;
  __shared__ int slots[SC_W];
  __shared__ int wave_base[SC_W];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & (PZN_WAVE - 1), wave = tid / PZN_WAVE;
  const int M = a.M;
  const float* g = a.raw + (size_t)b * M * 3;
  // a thread owns a CONTIGUOUS run of points, so that the partition keeps the original order with one scan over threads
  const int chunk = (M + SC_T - 1) / SC_T;
  const int lo = tid * chunk < M ? tid * chunk : M, hi = lo + chunk < M ? lo + chunk : M;
  const bool keep = chunk <= 64;      // the run's membership bits fit one register pair (uniform)
  fill_tables<KIND>(tab);

  int chosen = -1, best_k = 0, best_bal = -1;
  uint64_t sel = 0;                   // membership of this thread's run under the candidate that is taken
  for (int k = 0; k < a.K; ++k) {
    const Cand cd = load_candidate<KIND>(tab, a.params + ((size_t)b * a.K + k) * 6);
    int c = 0;
    uint64_t bits = 0;
    for (int j = lo; j < hi; ++j) {
      const bool in = inside<KIND>(tab, cd, g[3 * j], g[3 * j + 1], g[3 * j + 2]);
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
  const double* pk = a.params + ((size_t)b * a.K + chosen) * 6;
  Cand cd = {};
  if (!keep) cd = load_candidate<KIND>(tab, pk);
  auto member = [&](int j) -> bool {
    return keep ? ((sel >> (j - lo)) & 1) != 0 : inside<KIND>(tab, cd, g[3 * j], g[3 * j + 1], g[3 * j + 2]);
  };

  // stable partition: exclusive scan of the per-thread up counts over the workgroup
  int c = 0;
  if (keep) c = __popcll(sel);
  else
    for (int j = lo; j < hi; ++j) c += member(j) ? 1 : 0;
  int incl = c;
  for (int d = 1; d < PZN_WAVE; d <<= 1) {
    const int o = __shfl_up(incl, d, PZN_WAVE);
    if (lane >= d) incl += o;
  }
  __syncthreads();
  if (lane == PZN_WAVE - 1) slots[wave] = incl;
  __syncthreads();
  if (tid == 0) {
    int run = 0;
    for (int w = 0; w < SC_W; ++w) wave_base[w] = run, run += slots[w];
    slots[0] = run;      // total
  }
  __syncthreads();
  const int n_up = slots[0], n_down = M - n_up;
  int up_at = wave_base[wave] + incl - c;      // ups in front of this thread's run
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
  // padding: copies of the piece's first row (of the cloud's first row when the piece is empty)
  for (int half = 0; half < 2; ++half) {
    float* p = half ? pd : pu;
    const int cnt = half ? n_down : n_up;
    const float* first = cnt > 0 ? p : g;
    const float fx = first[0], fy = first[1], fz = first[2];
    for (int r = (cnt < a.cap ? cnt : a.cap) + tid; r < a.cap; r += SC_T) p[3 * r] = fx, p[3 * r + 1] = fy, p[3 * r + 2] = fz;
  }
  if (tid == 0) {
    a.counts[b] = n_up;
    a.counts[a.B + b] = n_down;
    for (int half = 0; half < 2; ++half) {
      const int cnt = half ? n_down : n_up;
      long s = (long)floor(a.u[2 * b + half] * (double)cnt);      // np.random.randint(0, n_piece) from a uniform draw
      s = s < 0 ? 0 : (s > cnt - 1 ? cnt - 1 : s);
      a.start[half * a.B + b] = s < 0 ? 0 : s;
    }
    for (int i = 0; i < 6; ++i) a.chosen[6 * b + i] = pk[i];
    a.chosen_k[b] = chosen;
    a.ok[b] = (valid && n_up <= a.cap && n_down <= a.cap) ? 1 : 0;
  }
}

}  // namespace

PZN_EXPORT int pzn_cut_compact_solid_f32(const float* raw, int kind, const double* params, const double* u, int B, int M, int K,
                                         int n_min, int cap, float* pieces, int64_t* counts, int64_t* start, double* chosen,
                                         int32_t* chosen_k, uint8_t* ok, pzn_stream_t stream) {
  PZN_CHECK_ARG(raw && params && u && pieces && counts && start && chosen && chosen_k && ok);
  PZN_CHECK_ARG(B > 0 && M > 0 && K > 0 && cap > 0 && n_min >= 0);
  PZN_CHECK_ARG(kind == SOLID_SPHERE || kind == SOLID_CYLINDER || kind == SOLID_CONE);
  SolidArgs a{raw, params, u, B, M, K, n_min, cap, pieces, counts, start, chosen, chosen_k, ok};
  hipStream_t st = pzn_hip_stream(stream);
  if (kind == SOLID_SPHERE) PZN_LAUNCH(cut_compact_solid_kernel<SOLID_SPHERE>, dim3(B), dim3(SC_T), 0, st, a);
  else if (kind == SOLID_CYLINDER) PZN_LAUNCH(cut_compact_solid_kernel<SOLID_CYLINDER>, dim3(B), dim3(SC_T), 0, st, a);
  else PZN_LAUNCH(cut_compact_solid_kernel<SOLID_CONE>, dim3(B), dim3(SC_T), 0, st, a);
  PZN_RETURN_LAUNCH_STATUS();
}
