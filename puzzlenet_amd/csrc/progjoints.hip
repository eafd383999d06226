// progjoints.hip — the pose graph of Z progressive walks read off their ledgers, for gfx950 (assembly.refine_progressive_batch):
// which pieces face each other across every merge, and on which rows.  include/pzn.h states the rule;
// assembly.progressive_joints_rule is its numpy statement, and every output here is held to that bit for bit.
//
// One workgroup of 256 threads per (round, puzzle), all rounds of all puzzles in one launch.  Per side of the merge the LDS holds
// the k root-frame points in float64 (24 bytes an entry), the piece of every entry and its key (own piece, facing piece): 32 bytes
// per entry and side, 64 KB at k = 1024.  A thread owns the entries tid, tid + 256, ... of either side; what it compares them with
// is read from the LDS at one address per instruction (a broadcast).  Five phases, a barrier where a phase reads what another
// thread wrote:
//   1. load and transform: the (piece, row) pair, the point widened to float64 and moved by G[piece];   (barrier; a workgroup
//      with a side that holds no valid entry ends here)
//   2. the nearest valid entry of the other side, both ways, and with it the key own * 64 + facing;           (barrier)
//   3. the rank of every entry inside its set - the earlier entries of its side with the same key - and the size of the set;
//   4. the size of the set that faces it - the other side's entries with the mirrored key - and the `least` test;
//   5. the scatter: the point as read, its row, and from the first entry of a set the count and, on the fixed side, the joint row.
// Phases 3 to 5 need nothing another thread writes after the second barrier.  No workspace, no atomics: every output element has
// one writer, so the same bits on every run.
// Every index is formed from a piece in [0, P), a row in [0, N), a slot below P (P - 1) / 2 and a rank below k.
#include "pzn_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int PJ_T = 256;
constexpr int PJ_MAX_P = 64;                    // a key is own * 64 + facing
constexpr int PJ_MAX_K = 1024;                  // 32 bytes per entry and side: 64 KB of LDS

// the points, pieces and keys of both sides, then the two "this side holds a valid entry" words (all LDS is dynamic: a static
// word would sit in front of the 16-byte aligned base)
size_t pj_lds_bytes(int k) { return (size_t)2 * k * (3 * sizeof(double) + 2 * sizeof(int32_t)) + 16; }

__global__ __launch_bounds__(PJ_T) void progressive_joints_kernel(
    const float* __restrict__ pieces, const double* __restrict__ G, const int64_t* __restrict__ dropped, int Z, int P, int N, int k,
    int least, int32_t* __restrict__ joints, float* __restrict__ a, float* __restrict__ b, int32_t* __restrict__ na,
    int32_t* __restrict__ nb, int64_t* __restrict__ rows_a, int64_t* __restrict__ rows_b) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  double* xyz = reinterpret_cast<double*>(smem_raw);                            // [2][3][k], in the root frame
  int32_t* piece = reinterpret_cast<int32_t*>(xyz + (size_t)6 * k);             // [2][k], -1: no valid entry
  int32_t* key = piece + 2 * k;                                                 // [2][k], own * 64 + facing, -1: none
  int32_t* holds = key + 2 * k;                                                 // [2]: the side holds a valid entry
  const int tid = (int)threadIdx.x;
  const int z = (int)(blockIdx.x % (unsigned)Z);                                // blockIdx.x = r Z + z
  const int64_t* list = dropped + (size_t)blockIdx.x * 4 * k;                   // [2][k][2] (piece, row)
  const int J = P * (P - 1) / 2;

  // 1. load and transform
  if (tid < 2) holds[tid] = 0;
  __syncthreads();
  for (int s = 0; s < 2; ++s)
    for (int e = tid; e < k; e += PJ_T) {
      const int64_t pi = list[2 * ((size_t)s * k + e)], ro = list[2 * ((size_t)s * k + e) + 1];
      const bool ok = pi >= 0 && pi < P && ro >= 0 && ro < N;
      piece[s * k + e] = ok ? (int32_t)pi : -1;
      key[s * k + e] = -1;
      if (ok) {
        const float* x = pieces + (((size_t)z * P + (size_t)pi) * N + (size_t)ro) * 3;
        const double* g = G + ((size_t)z * P + (size_t)pi) * 16;
        const double x0 = (double)x[0], x1 = (double)x[1], x2 = (double)x[2];
        for (int u = 0; u < 3; ++u)
          xyz[(size_t)(3 * s + u) * k + e] = __dadd_rn(
              __dadd_rn(__dadd_rn(__dmul_rn(g[4 * u], x0), __dmul_rn(g[4 * u + 1], x1)), __dmul_rn(g[4 * u + 2], x2)), g[4 * u + 3]);
        holds[s] = 1;                                                           // (every writer stores the same word)
      }
    }
  __syncthreads();
  if (!holds[0] || !holds[1]) return;                                           // (the same in every thread)

  // 2. the nearest valid entry of the other side; ties to the lowest position
  for (int s = 0; s < 2; ++s) {
    const int o = 1 - s;
    const double *ox = xyz + (size_t)(3 * o) * k, *oy = ox + k, *oz = oy + k;
    for (int e = tid; e < k; e += PJ_T) {
      const int own = piece[s * k + e];
      if (own < 0) continue;
      const double x0 = xyz[(size_t)(3 * s) * k + e], x1 = xyz[(size_t)(3 * s + 1) * k + e], x2 = xyz[(size_t)(3 * s + 2) * k + e];
      double best = 0.0;
      int at = -1;
      for (int t = 0; t < k; ++t) {
        if (piece[o * k + t] < 0) continue;                                     // (the same in every thread)
        const double dx = __dsub_rn(x0, ox[t]), dy = __dsub_rn(x1, oy[t]), dz = __dsub_rn(x2, oz[t]);
        const double d2 = __dadd_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz));
        if (at < 0 || d2 < best) best = d2, at = t;
      }
      key[s * k + e] = own * 64 + piece[o * k + at];                            // (the other side has a valid entry: at >= 0)
    }
  }
  __syncthreads();

  // 3. - 5. rank and size of the entry's set, size of the facing set, the scatter
  for (int s = 0; s < 2; ++s) {
    const int o = 1 - s;
    for (int e = tid; e < k; e += PJ_T) {
      const int mine = key[s * k + e];
      if (mine < 0) continue;
      const int own = mine >> 6, facing = mine & 63;
      if (own == facing) continue;                                              // (a piece on both sides: no joint with itself)
      const int mirrored = facing * 64 + own;
      int rank = 0, size = 0, size_facing = 0;
      for (int t = 0; t < k; ++t) {
        const int same = key[s * k + t] == mine;
        size += same;
        rank += same & (int)(t < e);
        size_facing += key[o * k + t] == mirrored;
      }
      if (size < least || size_facing < least) continue;
      const int p = s == 0 ? own : facing, q = s == 0 ? facing : own;          // p fixed, q moved
      const int lo = p < q ? p : q, hi = p < q ? q : p;
      const size_t slot = (size_t)z * J + (size_t)(hi * (hi - 1) / 2 + lo);
      const int64_t ro = list[2 * ((size_t)s * k + e) + 1];
      const float* x = pieces + (((size_t)z * P + own) * N + (size_t)ro) * 3;
      float* dst = (s == 0 ? a : b) + (slot * k + rank) * 3;
      dst[0] = x[0], dst[1] = x[1], dst[2] = x[2];
      (s == 0 ? rows_a : rows_b)[slot * k + rank] = ro;
      if (rank == 0) {
        (s == 0 ? na : nb)[slot] = size;
        if (s == 0) joints[2 * slot] = p, joints[2 * slot + 1] = q;
      }
    }
  }
}

}  // namespace

PZN_EXPORT int pzn_progressive_joints_supported(int P, int k) { return P >= 2 && P <= PJ_MAX_P && k >= 1 && k <= PJ_MAX_K; }

PZN_EXPORT int pzn_progressive_joints_f32(const float* pieces, const double* G, const int64_t* dropped, int R, int Z, int P, int N,
                                          int k, int least, int32_t* joints, float* a, float* b, int32_t* na, int32_t* nb,
                                          int64_t* rows_a, int64_t* rows_b, pzn_stream_t stream) {
  if (!pzn_progressive_joints_supported(P, k) || R < 1) return PZN_EUNSUPPORTED;
  PZN_CHECK_ARG(Z >= 0 && N >= 1 && least >= 1);
  if (Z == 0) return PZN_OK;
  PZN_CHECK_ARG((long long)R * Z <= 0x7fffffffLL);
  PZN_CHECK_ARG(pieces && G && dropped && joints && a && b && na && nb && rows_a && rows_b);
  const size_t lds = pj_lds_bytes(k);
  if (lds > 64 * 1024 &&
      hipFuncSetAttribute(reinterpret_cast<const void*>(progressive_joints_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)lds) != hipSuccess)
    return PZN_ELAUNCH;
  PZN_LAUNCH(progressive_joints_kernel, dim3((unsigned)(R * Z)), dim3(PJ_T), lds, pzn_hip_stream(stream), pieces, G, dropped, Z, P, N,
             k, least, joints, a, b, na, nb, rows_a, rows_b);
  PZN_RETURN_LAUNCH_STATUS();
}
