// assemblebeam.hip — the beam walks over Z pair tables, scored by the placed pieces' votes, for gfx950: one body, two kernels.
//   * assemble_beam_kernel (assembly.assemble_beam_batch): B hypotheses of one tree each, C children of each per round;
//   * assemble_forest_beam_kernel (assembly.assemble_forest_beam_batch): the same beam with the forest walk's restarts - a
//     hypothesis that finds no admissible entry opens a new component from a new root, so the beam sorts and assembles a pile
//     that holds several objects.
// include/pzn.h states the rules; assembly.beam_rule and assembly.forest_beam_rule are their numpy statements, and every
// output here is held to those bit for bit, the float64 poses and costs included.
//
// One wavefront per puzzle, one puzzle per workgroup, a capped grid with a loop over puzzles; no barrier (a wavefront's own LDS
// accesses execute in order, pzn::wave_lds_sync tells the compiler).  A hypothesis lives in LDS: its K float64 poses, its cost,
// its placed set as a 64-bit mask and its edges as (i K + j) | fwd << 16.  Two generations, 2 B (128 K + 4 (K - 1) + 16) bytes.
//   * candidates: for every live hypothesis in turn, the first C keys of (key << 32 | i K + j) over the pairs with one end
//     placed, by C passes "the smallest key above the last one" - the walk's 64-lane minimum (pzn_walk.h), so the order and the
//     ties are the walk's; a round has B C <= 64 children, and child (slot, rank) has the L lanes from (slot C + rank) L on,
//     L the largest power of two with B C L <= 64 (64 lanes at B = C = 1, 4 at the defaults, 1 at B = C = 8);
//   * a child: every one of its lanes composes the new pose as the walk does (the same bits); vote v = 2 p + dir - placed
//     piece p ascending, entry (p, n) before (n, p) - is worked out by lane v mod L, and after every L votes the disagreements
//     are added, through lane reads in vote order, to ONE running sum that all the child's lanes hold alike: the rule's
//     sequential order, with the float64 work of L votes side by side;
//   * selection: a child's first lane stands for it, and lane order is (parent slot, rank) order, so the order (cost, slot,
//     rank) is a 64-lane minimum of the cost's ordered bits and the lowest lane of the ballot of its ties; a winner whose
//     placed set equals a kept child's is dropped; B winners at most;
//   * the next generation: the wavefront copies each winner's parent poses and edges, the winner's lane adds its own.
// Without FOREST a hypothesis without a candidate has no child, and a round without any child ends the walk (on a table without
// -inf that is every live hypothesis in the same round: they fill the root's component together).
// What FOREST adds to the body: a hypothesis holds the component of every piece and the roots of its components as bytes, and
// the numbers of its components and edges in one dword (2 B (4 + 2 K) bytes more; the plain beam does not carve them out) - an
// edge has the place of its number and not of the round, since a restart makes none;
//   * a hypothesis whose first candidate pass finds nothing admissible gets the lanes of its rank 0 for the restart child; the
//     new root is the forest walk's: the fold over the table masked to entries with both ends outside and one 64-lane minimum,
//     or the one piece left; the child has the identity, no edge, no vote, and costs parent + restart_cost;
//   * a vote is valid only from a piece of the component the new piece joins (the component of the candidate's placed end);
//   * three more outputs.  Every hypothesis has a child in every round: count - 1 rounds, each placing one piece.
// Every index into score, T and moment is formed from i, j < count[z] <= K.  No atomics: the same bits on every run.
#include "pzn_common.h"
#include "pzn_walk.h"      // the key, the 64-lane arg-min, the stop test, the float64 dot product, the beam's helpers, the result tail

#pragma clang fp contract(off)

namespace {

constexpr int AB_T = PZN_WAVE;                  // one wavefront = one puzzle per workgroup
constexpr int AB_MAX_K = 64;                    // a piece per bit of the placed set
constexpr int AB_MAX_B = 8, AB_MAX_C = 8;       // B C <= 64: every child has a lane
constexpr int AB_MAX_GRID = 2048;
constexpr size_t AB_MAX_LDS = 160 * 1024;       // a CU's LDS on gfx950

// per hypothesis: K poses, cost and placed set, K - 1 edges; the forest adds (components | edges << 16), K component bytes,
// K root bytes
size_t ab_lds_bytes(int K, int B, bool forest) {
  return (size_t)2 * B * ((size_t)K * 16 * sizeof(double) + 16 + (size_t)(K - 1) * 4 + (forest ? 4 + (size_t)2 * K : 0));
}

template <bool FOREST>
__device__ __forceinline__ void beam_walk_body(
    const float* __restrict__ score, const float* __restrict__ T, const double* __restrict__ moment,
    const int32_t* __restrict__ count, double max_score, double vote_score, double joint_score, double weight, double restart_cost,
    int Z, int K, int B, int C, int L, int32_t* __restrict__ root, int32_t* __restrict__ edges, float* __restrict__ edge_score,
    int32_t* __restrict__ n_edges, double* __restrict__ G, uint8_t* __restrict__ placed, int32_t* __restrict__ joints,
    int32_t* __restrict__ n_joints, int32_t* __restrict__ component, int32_t* __restrict__ roots,
    int32_t* __restrict__ n_components, double* __restrict__ cost, int32_t* __restrict__ n_hyp) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int lane = (int)threadIdx.x;
  const int E = K - 1, KK = K * K, JR = K * (K - 1);
  double* pose = reinterpret_cast<double*>(smem_raw);                           // [2][B][K][16]
  double* hcost = pose + (size_t)2 * B * K * 16;                                // [2][B]
  uint64_t* hin = reinterpret_cast<uint64_t*>(hcost + 2 * B);                   // [2][B] placed sets
  uint32_t* hedge = reinterpret_cast<uint32_t*>(hin + 2 * B);                   // [2][B][K-1], by edge number
  uint32_t* hnum = nullptr;                                                     // FOREST: [2][B] components | edges << 16
  uint8_t *hcomp = nullptr, *hroot = nullptr;                                   // FOREST: [2][B][K] each, below
  if constexpr (FOREST) {
    hnum = hedge + (size_t)2 * B * E;
    hcomp = reinterpret_cast<uint8_t*>(hnum + 2 * B);                           // the component of every placed piece
    hroot = hcomp + (size_t)2 * B * K;                                          // the root of every component
  }
  const uint64_t NONE = ~(uint64_t)0;
  const double vlimit = vote_score != vote_score ? max_score : vote_score;
  const int grp = lane / L, sub = lane - grp * L;                               // child slot C + rank is lanes grp L .. grp L + L-1
  const int my_slot = grp / C;

  for (int z = (int)blockIdx.x; z < Z; z += (int)gridDim.x) {
    const float* S = score + (size_t)z * KK;
    const float* Tz = T + (size_t)z * KK * 16;
    const double* Mz = moment + (size_t)z * K * 16;
    const int c = count ? count[z] : K;
    const bool live = c >= 2 && c <= K;
    const int cc = live ? c * c : 0;

    int cur = 0, H = 0, ne = 0, r = -1;
    if (live) {
      [[maybe_unused]] const uint64_t all = c == 64 ? NONE : (((uint64_t)1 << c) - 1);      // FOREST
      uint64_t best = NONE;
      for (int t = lane; t < cc; t += PZN_WAVE) {
        const int i = t / c, j = t - i * c;
        const uint64_t k = entry(S[i * K + j], i, j, K);
        best = k < best ? k : best;
      }
      best = wave_min_u64_dpp(best);
      r = __builtin_amdgcn_readfirstlane((int)((uint32_t)best / (uint32_t)K));
      if (lane < 16) pose[16 * r + lane] = (lane >> 2) == (lane & 3) ? 1.0 : 0.0;      // generation 0, slot 0
      if (lane == 0) {
        hcost[0] = 0.0, hin[0] = (uint64_t)1 << r;
        if constexpr (FOREST) hnum[0] = 1u, hcomp[r] = 0, hroot[0] = (uint8_t)r;
      }
      pzn::wave_lds_sync();
      H = 1;

      for (int round = 0; round + 1 < c; ++round) {
        // the candidates of every live hypothesis, or (FOREST) its restart
        uint64_t mine = NONE;
        int restart = -1;                         // FOREST: the new root, in the lanes of a restart child
        for (int h = 0; h < H; ++h) {
          const uint64_t in_h = hin[cur * B + h];
          uint64_t last = 0;                      // (below every key)
          for (int rank = 0; rank < C; ++rank) {
            uint64_t next = NONE;
            for (int t = lane; t < cc; t += PZN_WAVE) {
              const int i = t / c, j = t - i * c;
              if (((in_h >> i) ^ (in_h >> j)) & 1) {
                const uint64_t k = entry(S[i * K + j], i, j, K);
                next = (k > last && k < next) ? k : next;
              }
            }
            next = wave_min_u64_dpp(next);
            const uint32_t w_key = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(next >> 32));
            if (w_key == 0xffffffffu) break;                                            // no pair left
            if (stops(w_key, max_score)) break;                                         // nor any later one
            last = next;
            if (grp == h * C + rank) mine = next;
          }
          if constexpr (FOREST) {
            if (last == 0) {                      // nothing admissible: a new component starts (in_h != all before the last round's end)
              const uint64_t out = all & ~in_h;
              int nr;
              if ((out & (out - 1)) == 0) {
                nr = (int)__builtin_ctzll(out);
              } else {
                uint64_t low = NONE;
                for (int t = lane; t < cc; t += PZN_WAVE) {
                  const int i = t / c, j = t - i * c;
                  if ((out >> i) & (out >> j) & 1) {
                    const uint64_t k = entry(S[i * K + j], i, j, K);
                    low = k < low ? k : low;
                  }
                }
                low = wave_min_u64_dpp(low);
                nr = __builtin_amdgcn_readfirstlane((int)((uint32_t)low / (uint32_t)K));
              }
              if (grp == h * C) restart = nr;
            }
          }
        }

        // the children, L lanes each: every lane composes the child's pose (the same bits), the votes are dealt out
        const bool grow = mine != NONE, has = grow || restart >= 0;
        double ccost = __builtin_inf();
        double gn[16], m[16];
        uint64_t in_p = 0, cin = 0;                // the parent's placed set, the child's
        uint32_t pnum = 0;                         // FOREST: the parent's components | edges << 16
        int flat = 0, nw = 0, jc = 0;              // the entry, the new piece, FOREST: the component it joins
        bool fwd = false;
#pragma unroll
        for (int e = 0; e < 16; ++e) gn[e] = ((e >> 2) == (e & 3)) ? 1.0 : 0.0, m[e] = 0.0;
        const uint8_t* pcomp = nullptr;            // FOREST: the parent's components (read if `has`)
        if constexpr (FOREST) pcomp = hcomp + (size_t)(cur * B + my_slot) * K;
        if (has) {
          in_p = hin[cur * B + my_slot];
          if constexpr (FOREST) pnum = hnum[cur * B + my_slot];
        }
        if (grow) {
          flat = (int)(uint32_t)mine;
          const float key = unordered((uint32_t)(mine >> 32));
          const int i = flat / K, j = flat - i * K;
          fwd = (in_p >> i) & 1;                   // the fixed end is placed: G[j] = G[i] T[i,j]
          nw = fwd ? j : i;
          if constexpr (FOREST) jc = (int)pcomp[fwd ? i : j];
          const double* hp = pose + ((size_t)(cur * B + my_slot) * K) * 16;             // the parent's poses
          double b[16];
          right_factor(Tz + (size_t)flat * 16, fwd, b);
          {
            const double* a = hp + 16 * (fwd ? i : j);
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
              for (int v = 0; v < 4; ++v)
                gn[4 * u + v] = dot4(a[4 * u], b[v], a[4 * u + 1], b[4 + v], a[4 * u + 2], b[8 + v], a[4 * u + 3], b[12 + v]);
          }
          ccost = hcost[cur * B + my_slot] + (double)key;
          if (weight != 0.0) {
#pragma unroll
            for (int e = 0; e < 16; ++e) m[e] = Mz[16 * nw + e];
          }
        } else if (FOREST && has) {                // a restart: the new root with the identity opens component `pnum & 0xffff`
          nw = restart;
          jc = (int)(pnum & 0xffffu);
          ccost = hcost[cur * B + my_slot] + restart_cost;
        }
        cin = in_p | (has ? (uint64_t)1 << nw : 0);
        if (weight != 0.0) {
          // vote v = 2 p + dir: entry (p, n), then (n, p), p ascending over the placed pieces (FOREST: of the joined component).
          // Lane `sub` of a child takes votes sub, sub + L, ...; after every L votes their disagreements are added to the child's
          // ONE running sum in vote order, in all its lanes alike.
          double sum = 0.0;
          int votes = 0;
          for (int v0 = 0; v0 < 2 * c; v0 += L) {                                       // (wavefront-uniform)
            const int v = v0 + sub, p = v >> 1;
            const int vf = (v & 1) ? nw * K + p : p * K + nw;
            bool valid = grow && v < 2 * c && ((in_p >> p) & 1) && vf != flat;          // (not the candidate's own entry)
            if constexpr (FOREST) {
              if (valid) valid = (int)pcomp[p] == jc;                                   // (p < c: a byte of the parent's row)
            }
            if (valid) {
              const float s = S[vf];
              const float k = s != s ? __builtin_inff() : s;
              valid = fabsf(k) < __builtin_inff() && !((double)k > vlimit);
            }
            double d = 0.0;
            if (valid) {
              const double* a = pose + ((size_t)(cur * B + my_slot) * K + p) * 16;
              double b[16], q[3];
              right_factor(Tz + (size_t)vf * 16, !(v & 1), b);
#pragma unroll
              for (int u = 0; u < 3; ++u) {
                double D[4], mm[4];
#pragma unroll
                for (int w = 0; w < 4; ++w)
                  D[w] = dot4(a[4 * u], b[w], a[4 * u + 1], b[4 + w], a[4 * u + 2], b[8 + w], a[4 * u + 3], b[12 + w]) - gn[4 * u + w];
#pragma unroll
                for (int w = 0; w < 4; ++w) mm[w] = dot4(m[4 * w], D[0], m[4 * w + 1], D[1], m[4 * w + 2], D[2], m[4 * w + 3], D[3]);
                q[u] = dot4(D[0], mm[0], D[1], mm[1], D[2], mm[2], D[3], mm[3]);
              }
              d = (q[0] + q[1]) + q[2];
            }
            const int steps = 2 * c - v0 < L ? 2 * c - v0 : L;
            for (int t = 0; t < steps; ++t) {
              const int from = lane - sub + t;
              const double dt = __longlong_as_double((long long)lane_u64((uint64_t)__double_as_longlong(d), from));
              if (__shfl((int)valid, from, PZN_WAVE)) sum = sum + dt, ++votes;
            }
          }
          if (grow) {                              // (a restart has no penalty term)
            const double penalty = votes ? sum / (double)votes : 0.0;
            ccost = ccost + weight * penalty;
          }
        }
        ccost = ccost != ccost ? __builtin_inf() : ccost;

        // selection: (cost, slot, rank) = (cost, lane); the first B distinct placed sets
        uint64_t remaining = __ballot(has && sub == 0);        // a child's first lane stands for it: lane order is still (slot, rank)
        if (remaining == 0) break;                 // a round without any child ends the walk (FOREST: every hypothesis has one)
        const uint64_t ckey = ordered64(ccost);
        uint64_t kept = 0;
        int nk = 0, my_new = -1;
        while (remaining != 0 && nk < B) {
          const bool in_race = (remaining >> lane) & 1;
          const uint64_t w = wave_min_u64_dpp(in_race ? ckey : NONE);
          const int W = __builtin_ctzll(__ballot(in_race && ckey == w));                 // the winner's lane (wavefront-uniform)
          remaining &= ~((uint64_t)1 << W);
          const uint64_t win = lane_u64(cin, W);
          if (__ballot(((kept >> lane) & 1) && cin == win) == 0) {
            if (lane == W) my_new = nk;
            kept |= (uint64_t)1 << W;
            ++nk;
          }
        }

        // the next generation: the parent's poses and edges (FOREST: components and roots), then the winner's own
        const int nxt = cur ^ 1;
        for (int s = 0; s < nk; ++s) {
          const int h = __builtin_ctzll(__ballot(my_new == s)) / L / C;
          int ne_h = round, nc_h = 0;              // the parent's edges - one a round, but for restarts - and FOREST: components
          if constexpr (FOREST) {
            const uint32_t num = hnum[cur * B + h];
            nc_h = (int)(num & 0xffffu), ne_h = (int)(num >> 16);
          }
          const double* from = pose + ((size_t)(cur * B + h) * K) * 16;
          double* to = pose + ((size_t)(nxt * B + s) * K) * 16;
          for (int e = lane; e < 16 * c; e += PZN_WAVE) to[e] = from[e];
          for (int e = lane; e < ne_h; e += PZN_WAVE) hedge[(nxt * B + s) * E + e] = hedge[(cur * B + h) * E + e];
          if constexpr (FOREST) {
            for (int e = lane; e < c; e += PZN_WAVE) hcomp[(nxt * B + s) * K + e] = hcomp[(cur * B + h) * K + e];
            for (int e = lane; e < nc_h; e += PZN_WAVE) hroot[(nxt * B + s) * K + e] = hroot[(cur * B + h) * K + e];
          }
        }
        pzn::wave_lds_sync();
        if (my_new >= 0) {
          const int at = nxt * B + my_new;
          const int nc_p = (int)(pnum & 0xffffu), ne_p = FOREST ? (int)(pnum >> 16) : round;      // nc_p <= round + 1 < K, ne_p <= round < K - 1
          double* to = pose + ((size_t)at * K + nw) * 16;
#pragma unroll
          for (int e = 0; e < 16; ++e) to[e] = gn[e];
          hcost[at] = ccost;
          hin[at] = cin;
          if constexpr (FOREST) hcomp[at * K + nw] = (uint8_t)jc;
          if (grow) {
            hedge[at * E + ne_p] = (uint32_t)flat | ((uint32_t)fwd << 16);
            if constexpr (FOREST) hnum[at] = pnum + (1u << 16);
          } else if constexpr (FOREST) {
            hroot[at * K + nc_p] = (uint8_t)nw;
            hnum[at] = pnum + 1u;
          }
        }
        pzn::wave_lds_sync();
        cur = nxt, H = nk;
        if constexpr (!FOREST) ++ne;               // (an edge a round)
      }
    }

    // the result is slot 0: the walk's outputs
    const uint64_t in = H > 0 ? hin[cur * B] : 0;
    int nc = 0, my_comp = 0, my_root = -1;         // FOREST: components, the component of piece `lane`, the root of component `lane`
    if constexpr (FOREST) {
      const uint32_t num = H > 0 ? hnum[cur * B] : 0;
      nc = (int)(num & 0xffffu), ne = (int)(num >> 16);
      my_comp = (H > 0 && lane < c) ? (int)hcomp[(cur * B) * K + lane] : -1;      // (every piece < c is placed)
      my_root = lane < nc ? (int)hroot[(cur * B) * K + lane] : -1;
      r = __builtin_amdgcn_readfirstlane(my_root);                               // (lane 0: the first component's)
    }
    int my_i = -1, my_j = -1, my_nw = -1;
    float my_s = __builtin_inff();
    uint32_t top = 0;
    if (lane < ne) {
      const uint32_t ed = hedge[(cur * B) * E + lane];
      const int flat = (int)(ed & 0xffffu);
      my_i = flat / K, my_j = flat - my_i * K, my_nw = (ed >> 16) ? my_j : my_i;
      my_s = S[flat];
      top = ordered(my_s);
    }
    top = pzn::wave_max_u32_dpp(top);
    const double worst = ne > 0 ? (double)unordered(top) : -__builtin_inf();      // the largest edge score
    if (lane < K - 1) {
      int32_t* e = edges + ((size_t)z * (K - 1) + lane) * 3;
      e[0] = my_i, e[1] = my_j, e[2] = my_nw;
      edge_score[(size_t)z * (K - 1) + lane] = my_s;
    }
    for (int e = lane; e < 16 * K; e += PZN_WAVE) {
      const double id = ((e >> 2) & 3) == (e & 3) ? 1.0 : 0.0;
      G[(size_t)z * K * 16 + e] = ((in >> (e >> 4)) & 1) ? pose[(size_t)(cur * B) * K * 16 + e] : id;
    }
    if constexpr (FOREST) {
      if (lane < K) component[(size_t)z * K + lane] = my_comp, roots[(size_t)z * K + lane] = my_root;
    }
    if (lane < B) cost[(size_t)z * B + lane] = lane < H ? hcost[cur * B + lane] : __builtin_inf();

    // the placed bytes and the joints (FOREST: of every component), by the walk's rule from the result's own edges
    const int nj = walk_tail(in, c, K, ne, worst, joint_score, S, lane, my_comp, placed + (size_t)z * K, joints + (size_t)z * JR * 2);
    if (lane == 0) {
      root[z] = r, n_edges[z] = ne, n_joints[z] = nj, n_hyp[z] = H;
      if constexpr (FOREST) n_components[z] = nc;
    }
    pzn::wave_lds_sync();      // the hypotheses are replaced by the next puzzle's
  }
}

__global__ __launch_bounds__(AB_T) void assemble_beam_kernel(const float* __restrict__ score, const float* __restrict__ T,
                                                             const double* __restrict__ moment, const int32_t* __restrict__ count,
                                                             double max_score, double vote_score, double joint_score, double weight,
                                                             int Z, int K, int B, int C, int L, int32_t* __restrict__ root,
                                                             int32_t* __restrict__ edges, float* __restrict__ edge_score,
                                                             int32_t* __restrict__ n_edges, double* __restrict__ G,
                                                             uint8_t* __restrict__ placed, int32_t* __restrict__ joints,
                                                             int32_t* __restrict__ n_joints, double* __restrict__ cost,
                                                             int32_t* __restrict__ n_hyp) {
  beam_walk_body<false>(score, T, moment, count, max_score, vote_score, joint_score, weight, 0.0, Z, K, B, C, L, root, edges,
                        edge_score, n_edges, G, placed, joints, n_joints, nullptr, nullptr, nullptr, cost, n_hyp);
}

__global__ __launch_bounds__(AB_T) void assemble_forest_beam_kernel(
    const float* __restrict__ score, const float* __restrict__ T, const double* __restrict__ moment,
    const int32_t* __restrict__ count, double max_score, double vote_score, double joint_score, double weight, double restart_cost,
    int Z, int K, int B, int C, int L, int32_t* __restrict__ root, int32_t* __restrict__ edges, float* __restrict__ edge_score,
    int32_t* __restrict__ n_edges, double* __restrict__ G, uint8_t* __restrict__ placed, int32_t* __restrict__ joints,
    int32_t* __restrict__ n_joints, int32_t* __restrict__ component, int32_t* __restrict__ roots,
    int32_t* __restrict__ n_components, double* __restrict__ cost, int32_t* __restrict__ n_hyp) {
  beam_walk_body<true>(score, T, moment, count, max_score, vote_score, joint_score, weight, restart_cost, Z, K, B, C, L, root, edges,
                       edge_score, n_edges, G, placed, joints, n_joints, component, roots, n_components, cost, n_hyp);
}

bool ab_supported(int K, int B, int C, bool forest) {
  return K >= 2 && K <= AB_MAX_K && B >= 1 && B <= AB_MAX_B && C >= 1 && C <= AB_MAX_C && ab_lds_bytes(K, B, forest) <= AB_MAX_LDS;
}

// the launch of either kernel: its LDS (allowed by attribute above 64 KB), a workgroup per puzzle up to the cap, and the lanes
// per child, which go in front of `outputs...` in the kernel's arguments
template <typename Kernel, typename... Args>
int ab_launch(Kernel kernel, bool forest, hipStream_t st, int Z, int K, int beam, int branch, Args... args) {
  const size_t lds = ab_lds_bytes(K, beam, forest);
  if (lds > 64 * 1024 &&
      hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return PZN_ELAUNCH;
  const int grid = Z < AB_MAX_GRID ? Z : AB_MAX_GRID;
  PZN_LAUNCH(kernel, dim3(grid), dim3(AB_T), lds, st, args...);
  PZN_RETURN_LAUNCH_STATUS();
}

// lanes per child: the largest power of two with B C lanes <= 64
int ab_lanes(int beam, int branch) {
  int lanes = 1;
  while (2 * lanes * beam * branch <= PZN_WAVE) lanes *= 2;
  return lanes;
}

}  // namespace

PZN_EXPORT int pzn_assemble_beam_supported(int K, int B, int C) { return ab_supported(K, B, C, false); }

PZN_EXPORT int pzn_assemble_beam_f32(const float* score, const float* T, const double* moment, const int32_t* count, int beam,
                                     int branch, double weight, double max_score, double vote_score, double joint_score, int Z,
                                     int K, int32_t* root, int32_t* edges, float* edge_score, int32_t* n_edges, double* G,
                                     uint8_t* placed, int32_t* joints, int32_t* n_joints, double* cost, int32_t* n_hyp,
                                     pzn_stream_t stream) {
  if (!pzn_assemble_beam_supported(K, beam, branch)) return PZN_EUNSUPPORTED;
  PZN_CHECK_ARG(Z >= 0);
  PZN_CHECK_ARG(max_score == max_score && weight == weight);
  if (Z == 0) return PZN_OK;
  PZN_CHECK_ARG(score && T && moment && root && edges && edge_score && n_edges && G && placed && joints && n_joints && cost && n_hyp);
  return ab_launch(assemble_beam_kernel, false, pzn_hip_stream(stream), Z, K, beam, branch, score, T, moment, count, max_score,
                   vote_score, joint_score, weight, Z, K, beam, branch, ab_lanes(beam, branch), root, edges, edge_score, n_edges, G,
                   placed, joints, n_joints, cost, n_hyp);
}

PZN_EXPORT int pzn_assemble_forest_beam_supported(int K, int B, int C) { return ab_supported(K, B, C, true); }

PZN_EXPORT int pzn_assemble_forest_beam_f32(const float* score, const float* T, const double* moment, const int32_t* count,
                                            int beam, int branch, double weight, double max_score, double vote_score,
                                            double joint_score, double restart_cost, int Z, int K, int32_t* root, int32_t* edges,
                                            float* edge_score, int32_t* n_edges, double* G, uint8_t* placed, int32_t* joints,
                                            int32_t* n_joints, int32_t* component, int32_t* roots, int32_t* n_components,
                                            double* cost, int32_t* n_hyp, pzn_stream_t stream) {
  if (!pzn_assemble_forest_beam_supported(K, beam, branch)) return PZN_EUNSUPPORTED;
  PZN_CHECK_ARG(Z >= 0);
  PZN_CHECK_ARG(max_score == max_score && weight == weight);
  if (Z == 0) return PZN_OK;
  PZN_CHECK_ARG(score && T && moment && root && edges && edge_score && n_edges && G && placed && joints && n_joints && component &&
                roots && n_components && cost && n_hyp);
  if (restart_cost != restart_cost) restart_cost = (max_score - max_score == 0.0) ? max_score : 0.0;      // NaN: a finite max_score, else 0
  return ab_launch(assemble_forest_beam_kernel, true, pzn_hip_stream(stream), Z, K, beam, branch, score, T, moment, count, max_score,
                   vote_score, joint_score, weight, restart_cost, Z, K, beam, branch, ab_lanes(beam, branch), root, edges,
                   edge_score, n_edges, G, placed, joints, n_joints, component, roots, n_components, cost, n_hyp);
}
