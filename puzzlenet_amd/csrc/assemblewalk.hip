// assemblewalk.hip — the greedy walks over Z pair tables and the joint list of every walk, for gfx950: one body, two kernels.
//   * assemble_walk_kernel (assembly.assemble_batch): assembly.assemble plus the joint selection of assembly.refine_assembly
//     with no host in between - one tree from the table's best entry, grown until a round's best key stops it;
//   * assemble_forest_kernel (assembly.assemble_forest_batch): the same walk that does not end where its tree stops growing -
//     the pieces still outside start a new component from a new root, until every piece of the pile is inside - and the joint
//     list of every component.
// include/pzn.h states the rules; assembly.walk_rule and assembly.forest_rule are their numpy statements, and every output
// here is held to those bit for bit.
//
// One wavefront per puzzle, four puzzles per workgroup, a capped grid with a loop over puzzles.  Nothing is shared between
// the wavefronts of a workgroup, so there is no barrier: a wavefront's own LDS accesses execute in order (pzn::wave_lds_sync
// tells the compiler).
//   * a key is the entry's fp32 score with NaN and the diagonal as +inf and -0 as +0, mapped to a dword whose unsigned order
//     is the float order (after the -0 fold equal floats are equal dwords); (key << 32 | i K + j) makes the rule's "smallest
//     key, lowest i K + j on ties" one unsigned 64-bit minimum, which does not depend on the order candidates are met in;
//   * a root: every lane folds the entries f = lane, lane + 64, ... of the table (coalesced), one 64-lane minimum;
//   * a round: lane p holds the best (key, i K + j) that joins piece p, outside, to a piece inside; one 64-lane minimum ends
//     the round, and after the placement of piece `new` (a root is one) every lane outside folds its two new entries
//     (new, p) and (p, new) into the key it holds;
//   * the poses G [K,4,4] float64 live in LDS (8 KB a puzzle at K = 64); sixteen lanes compose a placed pose, one entry
//     each (pzn_walk.h's compose_pose16), ((a0 b0 + a1 b1) + a2 b2) + a3 b3 with every operation rounded on its own (the file
//     is built with -ffp-contract=off, and the pragma below says it again);
//   * edge e stays in lane e's registers until the end (K - 1 <= 63 edges);
//   * the placed bytes and the joints are pzn_walk.h's walk_tail, shared with assemblebeam.hip.
// What FOREST adds to the body: the loop goes on to the next component while a piece is outside; a later root comes from the
// same fold masked to entries with both ends outside (K^2 / 64 loads a lane; the keys are not kept in LDS), or is the one
// piece left; the key a lane holds still covers the older components, as the rule's rounds do; lane p holds the component of
// piece p (walk_tail reads it) and lane q the root of component q; three more outputs.  A restart places a piece and so does
// a round: at most count restarts and count - 1 rounds, whatever the table holds.
// Every index into score and T is formed from an i, j < count[z] <= K.  No atomics: the same bits on every run.
#include "pzn_common.h"
#include "pzn_walk.h"      // the key, the 64-lane arg-min, the stop test, the sixteen-lane pose product and the result tail

#pragma clang fp contract(off)

namespace {

constexpr int AW_T = 256;                       // four wavefronts = four puzzles in flight per workgroup
constexpr int AW_W = AW_T / PZN_WAVE;
constexpr int AW_MAX_K = 64;                    // a piece per lane
constexpr int AW_MAX_GRID = 256;                // 1024 puzzles in flight; more take their turn in the same wavefronts

template <bool FOREST>
__device__ __forceinline__ void greedy_walk_body(const float* __restrict__ score, const float* __restrict__ T,
                                                 const int32_t* __restrict__ count, double max_score, double joint_score, int Z,
                                                 int K, int32_t* __restrict__ root, int32_t* __restrict__ edges,
                                                 float* __restrict__ edge_score, int32_t* __restrict__ n_edges,
                                                 double* __restrict__ G, uint8_t* __restrict__ placed,
                                                 int32_t* __restrict__ joints, int32_t* __restrict__ n_joints,
                                                 int32_t* __restrict__ component, int32_t* __restrict__ roots,
                                                 int32_t* __restrict__ n_components) {
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

    uint64_t in = 0;            // the pieces inside, bit p = piece p (the same in every lane)
    int ne = 0, nc = 0, r0 = -1;                // edges, components, the first root
    int my_comp = -1, my_root = -1;             // FOREST: the component of piece `lane`, the root of component `lane`
    int my_i = -1, my_j = -1, my_new = -1;      // edge `lane`
    float my_s = __builtin_inff();
    double worst = -__builtin_inf();            // the largest edge score
    if (live) {
      const uint64_t all = c == 64 ? NONE : (((uint64_t)1 << c) - 1);
      uint64_t mine = NONE;                     // the best (key, i K + j) that joins piece `lane`, outside, to a piece inside
      while (in != all) {
        // a component starts
        const uint64_t out = all & ~in;
        int r = -1;
        if constexpr (FOREST) {
          if ((out & (out - 1)) == 0) r = (int)__builtin_ctzll(out);      // one piece left
        }
        if (r < 0) {
          uint64_t best = NONE;
          for (int f = lane; f < KK; f += PZN_WAVE) {
            const int i = f / K, j = f - i * K;
            bool ok = i < c && j < c;
            if constexpr (FOREST) ok = ok && ((out >> i) & (out >> j) & 1);
            if (ok) {
              const uint64_t k = entry(S[f], i, j, K);
              best = k < best ? k : best;
            }
          }
          best = wave_min_u64_dpp(best);
          r = __builtin_amdgcn_readfirstlane((int)((uint32_t)best / (uint32_t)K));
        }
        in |= (uint64_t)1 << r;
        if (nc == 0) r0 = r;
        if constexpr (FOREST) {
          if (lane == nc) my_root = r;
          if (lane == r) my_comp = nc, mine = NONE;
        }
        if (lane < c && !((in >> lane) & 1)) {      // what joins piece `lane` to the new root
          const uint64_t a = entry(S[r * K + lane], r, lane, K), b = entry(S[lane * K + r], lane, r, K);
          const uint64_t m = a < b ? a : b;
          mine = m < mine ? m : mine;
        }
        // its rounds
        while (in != all) {
          const uint64_t w = wave_min_u64_dpp(mine);
          const uint32_t w_key = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(w >> 32));
          const int flat = __builtin_amdgcn_readfirstlane((int)(uint32_t)w);
          if ((w_key & (uint32_t)flat) == 0xffffffffu) break;      // no candidate left
          if (stops(w_key, max_score)) break;
          const int i = flat / K, j = flat - i * K;
          const bool fwd = (in >> i) & 1;           // the fixed end is inside: G[j] = G[i] T[i,j]
          const int nw = fwd ? j : i, src = fwd ? i : j;
          compose_pose16(g, src, nw, Tz + (size_t)flat * 16, fwd, lane);
          pzn::wave_lds_sync();
          const float raw = S[flat];
          if (lane == ne) my_i = i, my_j = j, my_new = nw, my_s = raw;
          worst = (double)raw > worst ? (double)raw : worst;
          in |= (uint64_t)1 << nw;
          ++ne;
          if (lane == nw) mine = NONE;
          if constexpr (FOREST) {
            if (lane == nw) my_comp = nc;
          }
          if (lane < c && !((in >> lane) & 1)) {
            const uint64_t a = entry(S[nw * K + lane], nw, lane, K), b = entry(S[lane * K + nw], lane, nw, K);
            const uint64_t m = a < b ? a : b;
            mine = m < mine ? m : mine;
          }
        }
        ++nc;
        if constexpr (!FOREST) break;               // one tree
      }
    }

    // the walk's outputs (ne <= c - 1 <= K - 1: every edge has its row)
    if (lane < K - 1) {
      int32_t* e = edges + ((size_t)z * (K - 1) + lane) * 3;
      e[0] = my_i, e[1] = my_j, e[2] = my_new;
      edge_score[(size_t)z * (K - 1) + lane] = my_s;
    }
    for (int e = lane; e < 16 * K; e += PZN_WAVE) G[(size_t)z * K * 16 + e] = g[e];
    if constexpr (FOREST) {
      if (lane < K) component[(size_t)z * K + lane] = my_comp, roots[(size_t)z * K + lane] = my_root;
    }

    const int nj = walk_tail(in, c, K, ne, worst, joint_score, S, lane, FOREST ? my_comp : 0, placed + (size_t)z * K,
                             joints + (size_t)z * JR * 2);
    if (lane == 0) {
      root[z] = r0, n_edges[z] = ne, n_joints[z] = nj;
      if constexpr (FOREST) n_components[z] = nc;
    }
    pzn::wave_lds_sync();      // the poses are replaced by the next puzzle's
  }
}

__global__ __launch_bounds__(AW_T) void assemble_walk_kernel(const float* __restrict__ score, const float* __restrict__ T,
                                                             const int32_t* __restrict__ count, double max_score,
                                                             double joint_score, int Z, int K, int32_t* __restrict__ root,
                                                             int32_t* __restrict__ edges, float* __restrict__ edge_score,
                                                             int32_t* __restrict__ n_edges, double* __restrict__ G,
                                                             uint8_t* __restrict__ placed, int32_t* __restrict__ joints,
                                                             int32_t* __restrict__ n_joints) {
  greedy_walk_body<false>(score, T, count, max_score, joint_score, Z, K, root, edges, edge_score, n_edges, G, placed, joints,
                          n_joints, nullptr, nullptr, nullptr);
}

__global__ __launch_bounds__(AW_T) void assemble_forest_kernel(const float* __restrict__ score, const float* __restrict__ T,
                                                               const int32_t* __restrict__ count, double max_score,
                                                               double joint_score, int Z, int K, int32_t* __restrict__ root,
                                                               int32_t* __restrict__ edges, float* __restrict__ edge_score,
                                                               int32_t* __restrict__ n_edges, double* __restrict__ G,
                                                               uint8_t* __restrict__ placed, int32_t* __restrict__ joints,
                                                               int32_t* __restrict__ n_joints, int32_t* __restrict__ component,
                                                               int32_t* __restrict__ roots, int32_t* __restrict__ n_components) {
  greedy_walk_body<true>(score, T, count, max_score, joint_score, Z, K, root, edges, edge_score, n_edges, G, placed, joints,
                         n_joints, component, roots, n_components);
}

// what both launches share: the LDS of four wavefronts' poses and the capped grid
size_t aw_lds_bytes(int K) { return (size_t)AW_W * K * 16 * sizeof(double); }
int aw_grid(int Z) {
  const int blocks = (Z + AW_W - 1) / AW_W;
  return blocks < AW_MAX_GRID ? blocks : AW_MAX_GRID;
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
  PZN_LAUNCH(assemble_walk_kernel, dim3(aw_grid(Z)), dim3(AW_T), aw_lds_bytes(K), st, score, T, count, max_score, joint_score, Z, K,
             root, edges, edge_score, n_edges, G, placed, joints, n_joints);
  PZN_RETURN_LAUNCH_STATUS();
}

PZN_EXPORT int pzn_assemble_forest_supported(int K) { return pzn_assemble_walk_supported(K); }

PZN_EXPORT int pzn_assemble_forest_f32(const float* score, const float* T, const int32_t* count, double max_score,
                                       double joint_score, int Z, int K, int32_t* root, int32_t* edges, float* edge_score,
                                       int32_t* n_edges, double* G, uint8_t* placed, int32_t* joints, int32_t* n_joints,
                                       int32_t* component, int32_t* roots, int32_t* n_components, pzn_stream_t stream) {
  if (!pzn_assemble_forest_supported(K)) return PZN_EUNSUPPORTED;
  PZN_CHECK_ARG(Z >= 0);
  PZN_CHECK_ARG(max_score == max_score);
  if (Z == 0) return PZN_OK;
  PZN_CHECK_ARG(score && T && root && edges && edge_score && n_edges && G && placed && joints && n_joints && component && roots &&
                n_components);
  hipStream_t st = pzn_hip_stream(stream);
  PZN_LAUNCH(assemble_forest_kernel, dim3(aw_grid(Z)), dim3(AW_T), aw_lds_bytes(K), st, score, T, count, max_score, joint_score, Z, K,
             root, edges, edge_score, n_edges, G, placed, joints, n_joints, component, roots, n_components);
  PZN_RETURN_LAUNCH_STATUS();
}
