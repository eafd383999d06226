// assemblewalk.hip — the greedy walk over Z pair tables and the joint list of every walk, for gfx950 (assembly.assemble_batch):
// assembly.assemble plus the joint selection of assembly.refine_assembly with no host in between.  include/pzn.h states the
// rule; assembly.walk_rule is its numpy statement, and every output here is held to that bit for bit.
//
// One wavefront per puzzle, four puzzles per workgroup, a capped grid with a loop over puzzles.  Nothing is shared between
// the wavefronts of a workgroup, so there is no barrier: a wavefront's own LDS accesses execute in order (pzn::wave_lds_sync
// tells the compiler).
//   * a key is the entry's fp32 score with NaN and the diagonal as +inf and -0 as +0, mapped to a dword whose unsigned order
//     is the float order (after the -0 fold equal floats are equal dwords); (key << 32 | i K + j) makes the rule's "smallest
//     key, lowest i K + j on ties" one unsigned 64-bit minimum, which does not depend on the order candidates are met in;
//   * the root: every lane folds the entries f = lane, lane + 64, ... of the table (coalesced), one 64-lane minimum;
//   * a round: lane p holds the best (key, i K + j) that joins unplaced piece p to the placed set; one 64-lane minimum ends
//     the round, and after the placement of piece `new` every lane folds its two new entries (new, p) and (p, new);
//   * the poses G [K,4,4] float64 live in LDS (8 KB a puzzle at K = 64); sixteen lanes compose a placed pose, one entry
//     each, ((a0 b0 + a1 b1) + a2 b2) + a3 b3 with every operation rounded on its own (the file is built with
//     -ffp-contract=off, and the pragma below says it again);
//   * edge e stays in lane e's registers until the end (K - 1 <= 63 edges);
//   * the placed bytes and the joints are pzn_walk.h's walk_tail, shared with assemblebeam.hip.
// Every index into score and T is formed from an i, j < count[z] <= K.  No atomics: the same bits on every run.
#include "pzn_common.h"
#include "pzn_walk.h"      // the key, the 64-lane arg-min, the stop test, the float64 dot product and the result tail

#pragma clang fp contract(off)

namespace {

constexpr int AW_T = 256;                       // four wavefronts = four puzzles in flight per workgroup
constexpr int AW_W = AW_T / PZN_WAVE;
constexpr int AW_MAX_K = 64;                    // a piece per lane
constexpr int AW_MAX_GRID = 256;                // 1024 puzzles in flight; more take their turn in the same wavefronts

__global__ __launch_bounds__(AW_T) void assemble_walk_kernel(const float* __restrict__ score, const float* __restrict__ T,
                                                             const int32_t* __restrict__ count, double max_score,
                                                             double joint_score, int Z, int K, int32_t* __restrict__ root,
                                                             int32_t* __restrict__ edges, float* __restrict__ edge_score,
                                                             int32_t* __restrict__ n_edges, double* __restrict__ G,
                                                             uint8_t* __restrict__ placed, int32_t* __restrict__ joints,
                                                             int32_t* __restrict__ n_joints) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int lane = (int)threadIdx.x & (PZN_WAVE - 1);
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x / PZN_WAVE);      // (the same in the wavefront: say so)
  double* g = reinterpret_cast<double*>(smem_raw) + (size_t)wave * K * 16;      // this wavefront's [K][16] poses
  const uint64_t NONE = ~(uint64_t)0;
  const int KK = K * K, JR = K * (K - 1);

  for (int z = (int)blockIdx.x * AW_W + wave; z < Z; z += (int)gridDim.x * AW_W) {      // (wavefront-uniform)
    const float* S = score + (size_t)z * KK;
    const float* Tz = T + (size_t)z * KK * 16;
    const int c = count ? count[z] : K;
    const bool live = c >= 2 && c <= K;

    for (int e = lane; e < 16 * K; e += PZN_WAVE) g[e] = ((e >> 2) & 3) == (e & 3) ? 1.0 : 0.0;
    pzn::wave_lds_sync();

    uint64_t in = 0;            // the placed set, bit p = piece p (the same in every lane)
    int r = -1, ne = 0;
    int my_i = -1, my_j = -1, my_new = -1;      // edge `lane`
    float my_s = __builtin_inff();
    double worst = -__builtin_inf();            // the largest edge score
    if (live) {
      uint64_t best = NONE;
      for (int f = lane; f < KK; f += PZN_WAVE) {
        const int i = f / K, j = f - i * K;
        if (i < c && j < c) {
          const uint64_t k = entry(S[f], i, j, K);
          best = k < best ? k : best;
        }
      }
      best = wave_min_u64_dpp(best);
      r = __builtin_amdgcn_readfirstlane((int)((uint32_t)best / (uint32_t)K));
      in = (uint64_t)1 << r;
      // what joins piece `lane` to the root
      uint64_t mine = NONE;
      if (lane < c && lane != r) {
        const uint64_t a = entry(S[r * K + lane], r, lane, K), b = entry(S[lane * K + r], lane, r, K);
        mine = a < b ? a : b;
      }
      for (int round = 0; round + 1 < c; ++round) {
        const uint64_t w = wave_min_u64_dpp(mine);
        const uint32_t w_key = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(w >> 32));
        const int flat = __builtin_amdgcn_readfirstlane((int)(uint32_t)w);
        if ((w_key & (uint32_t)flat) == 0xffffffffu) break;      // no candidate left
        if (stops(w_key, max_score)) break;
        const int i = flat / K, j = flat - i * K;
        const bool fwd = (in >> i) & 1;           // the fixed end is placed: G[j] = G[i] T[i,j]
        const int nw = fwd ? j : i, src = fwd ? i : j;
        const float* t = Tz + (size_t)flat * 16;
        if (lane < 16) {
          const int u = lane >> 2, v = lane & 3;
          double b0, b1, b2, b3;                  // column v of T[i,j], or of its rigid inverse [R^T, -(R^T t)]
          if (fwd) {
            b0 = (double)t[v], b1 = (double)t[4 + v], b2 = (double)t[8 + v], b3 = (double)t[12 + v];
          } else if (v < 3) {
            b0 = (double)t[4 * v], b1 = (double)t[4 * v + 1], b2 = (double)t[4 * v + 2], b3 = 0.0;
          } else {
            const double t0 = (double)t[3], t1 = (double)t[7], t2 = (double)t[11];
            b0 = -(((double)t[0] * t0 + (double)t[4] * t1) + (double)t[8] * t2);
            b1 = -(((double)t[1] * t0 + (double)t[5] * t1) + (double)t[9] * t2);
            b2 = -(((double)t[2] * t0 + (double)t[6] * t1) + (double)t[10] * t2);
            b3 = 1.0;
          }
          const double* a = g + 16 * src + 4 * u;
          const double val = dot4(a[0], b0, a[1], b1, a[2], b2, a[3], b3);
          g[16 * nw + lane] = val;                // (nw != src: no lane reads what another writes here)
        }
        pzn::wave_lds_sync();
        const float raw = S[flat];
        if (lane == round) my_i = i, my_j = j, my_new = nw, my_s = raw;
        worst = (double)raw > worst ? (double)raw : worst;
        in |= (uint64_t)1 << nw;
        ++ne;
        if (lane == nw) mine = NONE;
        if (lane < c && !((in >> lane) & 1)) {
          const uint64_t a = entry(S[nw * K + lane], nw, lane, K), b = entry(S[lane * K + nw], lane, nw, K);
          const uint64_t m = a < b ? a : b;
          mine = m < mine ? m : mine;
        }
      }
    }

    // the walk's outputs
    if (lane < K - 1) {
      int32_t* e = edges + ((size_t)z * (K - 1) + lane) * 3;
      e[0] = my_i, e[1] = my_j, e[2] = my_new;
      edge_score[(size_t)z * (K - 1) + lane] = my_s;
    }
    for (int e = lane; e < 16 * K; e += PZN_WAVE) G[(size_t)z * K * 16 + e] = g[e];

    const int nj = walk_tail(in, c, K, ne, worst, joint_score, S, lane, 0, placed + (size_t)z * K, joints + (size_t)z * JR * 2);
    if (lane == 0) root[z] = r, n_edges[z] = ne, n_joints[z] = nj;
    pzn::wave_lds_sync();      // the poses are replaced by the next puzzle's
  }
}

}  // namespace

PZN_EXPORT int pzn_assemble_walk_supported(int K) { return K >= 2 && K <= AW_MAX_K; }

PZN_EXPORT int pzn_assemble_walk_f32(const float* score, const float* T, const int32_t* count, double max_score, double joint_score,
                                     int Z, int K, int32_t* root, int32_t* edges, float* edge_score, int32_t* n_edges, double* G,
                                     uint8_t* placed, int32_t* joints, int32_t* n_joints, pzn_stream_t stream) {
  if (!pzn_assemble_walk_supported(K)) return PZN_EUNSUPPORTED;
  PZN_CHECK_ARG(Z >= 0);
  PZN_CHECK_ARG(max_score == max_score);
  if (Z == 0) return PZN_OK;
  PZN_CHECK_ARG(score && T && root && edges && edge_score && n_edges && G && placed && joints && n_joints);
  hipStream_t st = pzn_hip_stream(stream);
  const size_t lds = (size_t)AW_W * K * 16 * sizeof(double);
  const int blocks = (Z + AW_W - 1) / AW_W;
  const int grid = blocks < AW_MAX_GRID ? blocks : AW_MAX_GRID;
  PZN_LAUNCH(assemble_walk_kernel, dim3(grid), dim3(AW_T), lds, st, score, T, count, max_score, joint_score, Z, K, root, edges,
             edge_score, n_edges, G, placed, joints, n_joints);
  PZN_RETURN_LAUNCH_STATUS();
}
