// assembleforest.hip — the forest walk over Z pair tables, for gfx950 (assembly.assemble_forest_batch): the greedy walk of
// assemblewalk.hip that does not end where its tree stops growing - the pieces still outside start a new component from a new
// root, until every piece of the pile is inside - and the joint list of every component.  include/pzn.h states the rule;
// assembly.forest_rule is its numpy statement, and every output here is held to that bit for bit.
//
// The form is assemblewalk.hip's: one wavefront per pile, four piles per workgroup, a capped grid with a loop over piles, no
// barrier (pzn::wave_lds_sync), a piece per lane, the poses G [K,4,4] float64 in LDS, edge e in lane e's registers, the keys
// and the 64-lane arg-min of pzn_walk.h.  What a restart adds:
//   * the new root: with two or more pieces outside, the coalesced fold over the table that finds the walk's root, masked to
//     entries with both ends outside, and one 64-lane minimum (K^2 / 64 loads a lane; the keys are not kept in LDS); with one
//     piece outside, that piece;
//   * every lane outside folds its two entries with the new root into the best key it holds - the fold every placement does.
//     That key still covers the older components, as the rule's rounds do;
//   * lane p holds the component of piece p, lane q the root of component q; pzn_walk.h's walk_tail reads the former.
// A restart places a piece and so does a round: at most count restarts and count - 1 rounds, whatever the table holds.
// Every index into score and T is formed from an i, j < count[z] <= K.  No atomics: the same bits on every run.
#include "pzn_common.h"
#include "pzn_walk.h"      // the key, the 64-lane arg-min, the stop test, the float64 dot product and the result tail

#pragma clang fp contract(off)

namespace {

constexpr int AF_T = 256;                       // four wavefronts = four piles in flight per workgroup
constexpr int AF_W = AF_T / PZN_WAVE;
constexpr int AF_MAX_K = 64;                    // a piece per lane
constexpr int AF_MAX_GRID = 256;                // 1024 piles in flight; more take their turn in the same wavefronts

__global__ __launch_bounds__(AF_T) void assemble_forest_kernel(const float* __restrict__ score, const float* __restrict__ T,
                                                               const int32_t* __restrict__ count, double max_score,
                                                               double joint_score, int Z, int K, int32_t* __restrict__ root,
                                                               int32_t* __restrict__ edges, float* __restrict__ edge_score,
                                                               int32_t* __restrict__ n_edges, double* __restrict__ G,
                                                               uint8_t* __restrict__ placed, int32_t* __restrict__ joints,
                                                               int32_t* __restrict__ n_joints, int32_t* __restrict__ component,
                                                               int32_t* __restrict__ roots, int32_t* __restrict__ n_components) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int lane = (int)threadIdx.x & (PZN_WAVE - 1);
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x / PZN_WAVE);      // (the same in the wavefront: say so)
  double* g = reinterpret_cast<double*>(smem_raw) + (size_t)wave * K * 16;      // this wavefront's [K][16] poses
  const uint64_t NONE = ~(uint64_t)0;
  const int KK = K * K, JR = K * (K - 1);

  for (int z = (int)blockIdx.x * AF_W + wave; z < Z; z += (int)gridDim.x * AF_W) {      // (wavefront-uniform)
    const float* S = score + (size_t)z * KK;
    const float* Tz = T + (size_t)z * KK * 16;
    const int c = count ? count[z] : K;
    const bool live = c >= 2 && c <= K;

    for (int e = lane; e < 16 * K; e += PZN_WAVE) g[e] = ((e >> 2) & 3) == (e & 3) ? 1.0 : 0.0;
    pzn::wave_lds_sync();

    uint64_t in = 0;            // the pieces inside, bit p = piece p (the same in every lane)
    int ne = 0, nc = 0;
    int my_comp = -1, my_root = -1;             // the component of piece `lane`, the root of component `lane`
    int my_i = -1, my_j = -1, my_new = -1;      // edge `lane`
    float my_s = __builtin_inff();
    double worst = -__builtin_inf();            // the largest edge score
    if (live) {
      const uint64_t all = c == 64 ? NONE : (((uint64_t)1 << c) - 1);
      uint64_t mine = NONE;                     // the best (key, i K + j) that joins piece `lane`, outside, to a piece inside
      while (in != all) {
        // a component starts
        const uint64_t out = all & ~in;
        int r;
        if ((out & (out - 1)) == 0) {
          r = (int)__builtin_ctzll(out);
        } else {
          uint64_t best = NONE;
          for (int f = lane; f < KK; f += PZN_WAVE) {
            const int i = f / K, j = f - i * K;
            if (i < c && j < c && ((out >> i) & (out >> j) & 1)) {
              const uint64_t k = entry(S[f], i, j, K);
              best = k < best ? k : best;
            }
          }
          best = wave_min_u64_dpp(best);
          r = __builtin_amdgcn_readfirstlane((int)((uint32_t)best / (uint32_t)K));
        }
        in |= (uint64_t)1 << r;
        if (lane == nc) my_root = r;
        if (lane == r) my_comp = nc, mine = NONE;
        if (lane < c && !((in >> lane) & 1)) {      // what joins piece `lane` to the new root
          const uint64_t a = entry(S[r * K + lane], r, lane, K), b = entry(S[lane * K + r], lane, r, K);
          const uint64_t m = a < b ? a : b;
          mine = m < mine ? m : mine;
        }
        // its rounds: the walk's
        while (in != all) {
          const uint64_t w = wave_min_u64_dpp(mine);
          const uint32_t w_key = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(w >> 32));
          const int flat = __builtin_amdgcn_readfirstlane((int)(uint32_t)w);
          if ((w_key & (uint32_t)flat) == 0xffffffffu) break;      // no candidate left
          if (stops(w_key, max_score)) break;
          const int i = flat / K, j = flat - i * K;
          const bool fwd = (in >> i) & 1;           // the fixed end is inside: G[j] = G[i] T[i,j]
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
          if (lane == ne) my_i = i, my_j = j, my_new = nw, my_s = raw;
          worst = (double)raw > worst ? (double)raw : worst;
          in |= (uint64_t)1 << nw;
          ++ne;
          if (lane == nw) my_comp = nc, mine = NONE;
          if (lane < c && !((in >> lane) & 1)) {
            const uint64_t a = entry(S[nw * K + lane], nw, lane, K), b = entry(S[lane * K + nw], lane, nw, K);
            const uint64_t m = a < b ? a : b;
            mine = m < mine ? m : mine;
          }
        }
        ++nc;
      }
    }

    // the walk's outputs (ne <= c - 1 <= K - 1: every edge has its row)
    if (lane < K - 1) {
      int32_t* e = edges + ((size_t)z * (K - 1) + lane) * 3;
      e[0] = my_i, e[1] = my_j, e[2] = my_new;
      edge_score[(size_t)z * (K - 1) + lane] = my_s;
    }
    for (int e = lane; e < 16 * K; e += PZN_WAVE) G[(size_t)z * K * 16 + e] = g[e];
    if (lane < K) component[(size_t)z * K + lane] = my_comp, roots[(size_t)z * K + lane] = my_root;

    const int nj = walk_tail(in, c, K, ne, worst, joint_score, S, lane, my_comp, placed + (size_t)z * K,
                             joints + (size_t)z * JR * 2);
    const int r0 = __builtin_amdgcn_readfirstlane(my_root);      // (lane 0: the first component's)
    if (lane == 0) root[z] = r0, n_edges[z] = ne, n_joints[z] = nj, n_components[z] = nc;
    pzn::wave_lds_sync();      // the poses are replaced by the next pile's
  }
}

}  // namespace

PZN_EXPORT int pzn_assemble_forest_supported(int K) { return K >= 2 && K <= AF_MAX_K; }

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
  const size_t lds = (size_t)AF_W * K * 16 * sizeof(double);
  const int blocks = (Z + AF_W - 1) / AF_W;
  const int grid = blocks < AF_MAX_GRID ? blocks : AF_MAX_GRID;
  PZN_LAUNCH(assemble_forest_kernel, dim3(grid), dim3(AF_T), lds, st, score, T, count, max_score, joint_score, Z, K, root, edges,
             edge_score, n_edges, G, placed, joints, n_joints, component, roots, n_components);
  PZN_RETURN_LAUNCH_STATUS();
}
