// progressive.hip — one round of Z progressive walks, for gfx950 (assembly.ProgressiveBatch): every puzzle chooses its merge and
// updates its ledger with no host in between.  include/pzn.h states the rule; assembly.progressive_round_rule is its numpy
// statement, and every field here is held to that bit for bit, G included.
//
// One wavefront per puzzle, four puzzles per workgroup, a capped grid with a loop over puzzles (as assemblewalk.hip, whose key,
// arg-min and dot product it shares through pzn_walk.h).  Nothing is shared between wavefronts: no LDS, no barrier, no atomics,
// no workspace.
//   * lane p holds alive[p] and part[p]; one ballot gives the live set;
//   * every lane folds the entries f = lane, lane + 64, ... of the table whose two ends are alive (coalesced), one 64-lane
//     minimum of (key << 32 | i P + j) ends the choice;
//   * a stopped puzzle writes done, took and the safe pick and nothing else;
//   * the merge: sixteen lanes compose one pose, G[p] = T[i,j] G[p], one entry each, four poses a pass; a wavefront's lanes
//     execute one instruction together, so every entry of a pose is read before any is written;
//   * a part's label is the lowest piece whose part it is: the first set bit of a ballot.
// Every index is formed from i, j < P and an edge row below P - 1 (a state whose n_edges is outside [0, P - 2] stops).
#include "pzn_common.h"
#include "pzn_walk.h"

#pragma clang fp contract(off)

namespace {

constexpr int PR_T = 256;                       // four wavefronts = four puzzles in flight per workgroup
constexpr int PR_W = PR_T / PZN_WAVE;
constexpr int PR_MAX_P = 64;                    // a slot per lane
constexpr int PR_MAX_GRID = 256;                // 1024 puzzles in flight; more take their turn in the same wavefronts

__global__ __launch_bounds__(PR_T) void progressive_round_kernel(const float* __restrict__ score, const float* __restrict__ T,
                                                                 double max_score, int Z, int P, uint8_t* alive, int32_t* part,
                                                                 double* G, uint8_t* done, int32_t* n_edges, int32_t* edges,
                                                                 float* edge_score, uint8_t* __restrict__ took,
                                                                 int64_t* __restrict__ pick) {
  const int lane = (int)threadIdx.x & (PZN_WAVE - 1);
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x / PZN_WAVE);      // (the same in the wavefront: say so)
  const uint64_t NONE = ~(uint64_t)0;
  const int PP = P * P;

  for (int z = (int)blockIdx.x * PR_W + wave; z < Z; z += (int)gridDim.x * PR_W) {      // (wavefront-uniform)
    const float* S = score + (size_t)z * PP;
    const bool mine_alive = lane < P && alive[(size_t)z * P + lane] != 0;
    const int mine_part = lane < P ? part[(size_t)z * P + lane] : -1;
    const uint64_t live = __ballot(mine_alive);      // the live slots, bit s = slot s (the same in every lane)
    const int ne = n_edges[z];
    bool stop = done[z] != 0 || __popcll(live) < 2 || ne < 0 || ne >= P - 1;
    int flat = 0;
    if (!stop) {
      uint64_t best = NONE;
      for (int f = lane; f < PP; f += PZN_WAVE) {
        const int i = f / P, j = f - i * P;
        if (((live >> i) & 1) && ((live >> j) & 1)) {
          const uint64_t k = entry(S[f], i, j, P);
          best = k < best ? k : best;
        }
      }
      best = wave_min_u64_dpp(best);
      const uint32_t w_key = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(best >> 32));
      flat = __builtin_amdgcn_readfirstlane((int)(uint32_t)best);
      // (two live slots always give a candidate; its key may be +inf)
      stop = best == NONE || stops(w_key, max_score);
    }
    if (stop) {
      if (lane == 0) {
        done[z] = 1, took[z] = 0;
        pick[2 * (size_t)z] = 0, pick[2 * (size_t)z + 1] = 0;
      }
      continue;
    }
    const int i = flat / P, j = flat - i * P;
    const float* t = T + ((size_t)z * PP + flat) * 16;
    double* Gz = G + (size_t)z * P * 16;
    const int e = lane & 15, u = e >> 2, v = e & 3;
    const double t0 = (double)t[4 * u], t1 = (double)t[4 * u + 1], t2 = (double)t[4 * u + 2], t3 = (double)t[4 * u + 3];
    for (int base = 0; base < P; base += PZN_WAVE / 16) {
      const int p = base + (lane >> 4);
      const int pp = __shfl(mine_part, p < P ? p : 0);
      if (p < P && pp == j) {
        double* g = Gz + 16 * p;
        const double val = dot4(t0, g[v], t1, g[4 + v], t2, g[8 + v], t3, g[12 + v]);
        g[e] = val;      // (the sixteen lanes of a pose have all read before this instruction stores)
      }
    }
    const uint64_t in_i = __ballot(lane < P && mine_part == i), in_j = __ballot(lane < P && mine_part == j);
    const int label_i = in_i ? (int)__ffsll((unsigned long long)in_i) - 1 : i;
    const int label_j = in_j ? (int)__ffsll((unsigned long long)in_j) - 1 : j;
    if (lane < P && mine_part == j) part[(size_t)z * P + lane] = i;
    if (lane == j) alive[(size_t)z * P + j] = 0;
    if (lane == 0) {
      int32_t* row = edges + ((size_t)z * (P - 1) + ne) * 4;
      row[0] = label_i, row[1] = label_j, row[2] = i, row[3] = j;
      edge_score[(size_t)z * (P - 1) + ne] = S[flat];
      n_edges[z] = ne + 1;
      took[z] = 1;
      pick[2 * (size_t)z] = i, pick[2 * (size_t)z + 1] = j;
    }
  }
}

}  // namespace

PZN_EXPORT int pzn_progressive_round_supported(int P) { return P >= 2 && P <= PR_MAX_P; }

PZN_EXPORT int pzn_progressive_round_f32(const float* score, const float* T, double max_score, int Z, int P, uint8_t* alive,
                                         int32_t* part, double* G, uint8_t* done, int32_t* n_edges, int32_t* edges,
                                         float* edge_score, uint8_t* took, int64_t* pick, pzn_stream_t stream) {
  if (!pzn_progressive_round_supported(P)) return PZN_EUNSUPPORTED;
  PZN_CHECK_ARG(Z >= 0);
  PZN_CHECK_ARG(max_score == max_score);
  if (Z == 0) return PZN_OK;
  PZN_CHECK_ARG(score && T && alive && part && G && done && n_edges && edges && edge_score && took && pick);
  const int blocks = (Z + PR_W - 1) / PR_W;
  const int grid = blocks < PR_MAX_GRID ? blocks : PR_MAX_GRID;
  PZN_LAUNCH(progressive_round_kernel, dim3(grid), dim3(PR_T), 0, pzn_hip_stream(stream), score, T, max_score, Z, P, alive, part, G,
             done, n_edges, edges, edge_score, took, pick);
  PZN_RETURN_LAUNCH_STATUS();
}
