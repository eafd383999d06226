// solidcut.hip — the sphere / cylinder / cone cuts of the reference's loader (dataset.py:715-759, re-draw :1175-1179) as one
// launch per batch: the single-cut body of pzn_cut.h (the plane cut's, datapipe.hip) with a solid in place of the plane.  This
// file holds the predicate, its tables and the solids' cut object.
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
// rotation matrix.  The body evaluates the predicate ONCE per point and candidate (it keeps the bits of a thread's run).
// float64 throughout, every operation individually rounded (-ffp-contract=off), like the plane cut.
#include "pzn_common.h"

namespace {

#include "pzn_cut.h"

constexpr int SC_RES = 50;                    // resolution of the three meshes (dataset.py:717, :733, :750)
constexpr int SC_SEC_MAX = SC_RES / 2;        // sphere: 25 of the 100 sector mid-angles lie in [0, pi/2]
constexpr int SC_BANDS = SC_RES / 2;          // sphere: 25 latitude bands per hemisphere
constexpr double SC_PI = 3.14159265358979323846;

enum { SOLID_SPHERE = 0, SOLID_CYLINDER = 1, SOLID_CONE = 2 };

struct SolidArgs {
  CutIO io;                // pieces: the up side is the solid's inside
  const double* params;    // [B, K, 6]: rot, shift
  double* chosen;          // [B, 6]: rot, shift of the candidate that was taken
  int32_t* chosen_k;       // [B]: its index
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

template <int KIND>
struct SolidCut {
  const SolidArgs& a;
  Tables& t;
  __device__ const double* candidate(int k) const { return a.params + ((size_t)blockIdx.x * a.io.K + k) * 6; }
  __device__ Cand load(int k) const { return load_candidate<KIND>(t, candidate(k)); }
  __device__ bool test(const Cand& c, float x, float y, float z) const { return inside<KIND>(t, c, x, y, z); }
  __device__ void record(int k) const {
    const double* pk = candidate(k);
    for (int i = 0; i < 6; ++i) a.chosen[6 * blockIdx.x + i] = pk[i];
    a.chosen_k[blockIdx.x] = k;
  }
};

template <int KIND>
__global__ __launch_bounds__(CUT_T) void cut_compact_solid_kernel(SolidArgs a) {
  __shared__ Tables tab;
  __shared__ int slots[CUT_W];
  __shared__ int wave_base[CUT_W];
  fill_tables<KIND>(tab);      // (published by the barriers of the first load)
  cut_compact_body(a.io, SolidCut<KIND>{a, tab}, slots, wave_base);
}

}  // namespace

PZN_EXPORT int pzn_cut_compact_solid_f32(const float* raw, int kind, const double* params, const double* u, int B, int M, int K,
                                         int n_min, int cap, float* pieces, int64_t* counts, int64_t* start, double* chosen,
                                         int32_t* chosen_k, uint8_t* ok, pzn_stream_t stream) {
  PZN_CHECK_ARG(raw && params && u && pieces && counts && start && chosen && chosen_k && ok);
  PZN_CHECK_ARG(B > 0 && M > 0 && K > 0 && cap > 0 && n_min >= 0);
  PZN_CHECK_ARG(kind == SOLID_SPHERE || kind == SOLID_CYLINDER || kind == SOLID_CONE);
  SolidArgs a{{raw, u, B, M, K, n_min, cap, pieces, counts, start, ok}, params, chosen, chosen_k};
  hipStream_t st = pzn_hip_stream(stream);
  if (kind == SOLID_SPHERE) PZN_LAUNCH(cut_compact_solid_kernel<SOLID_SPHERE>, dim3(B), dim3(CUT_T), 0, st, a);
  else if (kind == SOLID_CYLINDER) PZN_LAUNCH(cut_compact_solid_kernel<SOLID_CYLINDER>, dim3(B), dim3(CUT_T), 0, st, a);
  else PZN_LAUNCH(cut_compact_solid_kernel<SOLID_CONE>, dim3(B), dim3(CUT_T), 0, st, a);
  PZN_RETURN_LAUNCH_STATUS();
}
