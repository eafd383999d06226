// dfgemm.hip — weight gradients dW[N, K] += dY^T X for small weight matrices, fragments straight from
// global memory ("direct fragment"), bf16x3 split precision.
//
//   dW[n, k] += sum_m dY[m, n] * X[m, k]        dY[M, N], X[M, K] row-major, M = 10^4..10^6 rows,
//   db[n]    += sum_m dY[m, n]                   N, K <= a few hundred.
//
// The reduction runs over ROWS, which are the slow index of both operands.  The general tile engine
// (gemm.hip, "TN") stages both tiles in LDS and reads them back transposed, one workgroup barrier per 16
// rows; its waves are parked in s_waitcnt / s_barrier 70 % of the time (profiles/).  But the operand layout
// v_mfma_f32_32x32x16_bf16 wants here — lane l holds, for column l&31 of its 32-column tile, the 8
// consecutive reduction indices (l>>5)*8 .. +7 — is something a lane can fetch itself: 8 dword loads, each of
// which is, across the wavefront, two fully coalesced 128-byte row segments.  So:
//   * no LDS, no barrier: a wavefront owns TI x TJ output tiles of 32 x 32 (accumulators in registers) and
//     streams its share of the rows in steps of 16: (TI + TJ) * 8 dword loads, split into bf16 planes in
//     registers, TI * TJ * 6 MFMAs; the loads of the next step are issued as soon as the current values
//     have been split;
//   * a workgroup = every (TI x TJ) tile block of the output ("wave types") x a few replicas that take
//     interleaved row steps, so the types re-read the same rows out of L1/L2 at about the same time;
//   * partial sums meet in the fp32 atomics of the epilogue (dW is small), as the general engine's split-K
//     path does; the grid is sized so that those atomics stay well below the streaming time (summing the
//     replicas of a workgroup in LDS first was measured slower: one barrier round per replica);
// No alignment requirements (K = 67, 131 are fine), ReLU mask on dY (genY) and the skipped pad column of the
// set-abstraction rows are handled at the loads / stores.
#include <stdlib.h>

#include "pzn_common.h"
#include "pzn_internal.h"

namespace {

#include "pzn_x3.h"

struct DfArgs {
  const float* dy;    // [M, N]
  int ldy;
  const float* genY;  // dY(m,n) *= genY(m,n) > 0 (same layout) or NULL
  const float* x;     // [M, K]
  int ldx;
  float* dW;          // [N, K'] += ...   K' = K - (skip_col >= 0)
  int ldw;
  float* db;          // [N] += ... or NULL
  int M, N, K;
  int skip_col;       // column of X that has no weight (the zero pad of the padded group rows) or -1
  int types_k;        // wave types along K
  int types_per_wg;   // wave types handled by one workgroup (blockIdx.y selects the group)
  int reps;           // replicas per type in a workgroup
  int steps_per_wg;   // 16-row steps per workgroup
  // up to three dY / dW / db triples that share X (the q, k, v projections of an attention block): the N axis is
  // the concatenation of the segments (each a multiple of 64 columns), one launch instead of three
  int nseg;
  const float* sdy[3];
  int sn[3];
  float* sdw[3];
  float* sdb[3];
};

template <int TI, int TJ, bool GENY, bool WITH_DB>
__global__ __launch_bounds__(768) void df_wgrad_kernel(DfArgs p) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // scalar: row offsets must be provably uniform
  const int l31 = lane & 31, half = lane >> 5;
  const int tl = wave / p.reps, rep = wave - tl * p.reps;
  const int type = blockIdx.y * p.types_per_wg + tl;
  const int ti = type / p.types_k, tj = type - ti * p.types_k;
  int n0 = ti * (TI * 32);
  const int k0 = tj * (TJ * 32);
  if (p.nseg) {  // wave-uniform choice of the segment this tile block belongs to
    const int e0 = p.sn[0], e1 = e0 + p.sn[1];
    const int sg = n0 < e0 ? 0 : (n0 < e1 ? 1 : 2);
    n0 -= sg == 0 ? 0 : (sg == 1 ? e0 : e1);
    p.dy = sg == 0 ? p.sdy[0] : (sg == 1 ? p.sdy[1] : p.sdy[2]);
    p.N = sg == 0 ? p.sn[0] : (sg == 1 ? p.sn[1] : p.sn[2]);
    p.ldy = p.N;
    p.dW = sg == 0 ? p.sdw[0] : (sg == 1 ? p.sdw[1] : p.sdw[2]);
    p.db = sg == 0 ? p.sdb[0] : (sg == 1 ? p.sdb[1] : p.sdb[2]);
    if (sg >= p.nseg) n0 = p.N;  // padding type
  }
  const bool active = n0 < p.N;  // false: padding type of the last group

  // This lane's columns.  Columns past N / K are clamped for the loads and NOT zeroed: they only feed output
  // rows / columns that the epilogue never stores.  Per-lane offsets are fixed for the whole walk; the row
  // advance is wave-uniform, so every load is "scalar base + 32-bit lane offset" with no address VALU.
  unsigned offn[TI], offk[TJ];
  bool nok[TI];
#pragma unroll
  for (int i = 0; i < TI; ++i) {
    const int c = n0 + i * 32 + l31;
    nok[i] = c < p.N;
    offn[i] = (unsigned)(half * 8 * p.ldy + (nok[i] ? c : p.N - 1));
  }
#pragma unroll
  for (int j = 0; j < TJ; ++j) {
    const int c = k0 + j * 32 + l31;
    offk[j] = (unsigned)(half * 8 * p.ldx + (c < p.K ? c : p.K - 1));
  }

  const int nsteps = p.M >> 4;  // M % 16 == 0 (checked on the host)
  const int s_begin = blockIdx.x * p.steps_per_wg;
  int s_end = s_begin + p.steps_per_wg;
  s_end = s_end < nsteps ? s_end : nsteps;
  if (!active) s_end = s_begin;

  floatx16 acc[TI][TJ];
#pragma unroll
  for (int i = 0; i < TI; ++i)
#pragma unroll
    for (int j = 0; j < TJ; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  float dbacc[TI];
#pragma unroll
  for (int i = 0; i < TI; ++i) dbacc[i] = 0.f;

  // buffer loads: descriptor (scalar) + wave-uniform row offset (scalar) + fixed lane offset (vector): no address VALU
  const __amdgpu_buffer_rsrc_t rdy = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.dy), 0, -1, 0x00020000);
  const __amdgpu_buffer_rsrc_t rgy = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(GENY ? p.genY : p.dy), 0, -1, 0x00020000);
  const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.x), 0, -1, 0x00020000);
  float ra[TI][8], ry[TI][8], rb[TJ][8];
  auto issue = [&](int s) {  // unconditional loads: the vmcnt bookkeeping stays exact
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int m = s * 16 + e;  // wave-uniform row; byte offsets stay below 2^32 (checked on the host)
      const int sy = m * p.ldy * 4, sx = m * p.ldx * 4;
#pragma unroll
      for (int i = 0; i < TI; ++i) {
        ra[i][e] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rdy, (int)(offn[i] * 4), sy, 0));
        if (GENY) ry[i][e] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rgy, (int)(offn[i] * 4), sy, 0));
      }
#pragma unroll
      for (int j = 0; j < TJ; ++j)
        rb[j][e] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rx, (int)(offk[j] * 4), sx, 0));
    }
  };

  int s = s_begin + rep;
  if (s < s_end) issue(s);
  for (; s < s_end; s += p.reps) {
    bf16x8 pa[TI][3], pb[TJ][3];
#pragma unroll
    for (int i = 0; i < TI; ++i) {
      float v[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        v[e] = (GENY && !(ry[i][e] > 0.f)) ? 0.f : ra[i][e];
        if (WITH_DB) dbacc[i] += v[e];
      }
      split8<split_pair_packed>(v, pa[i]);
    }
#pragma unroll
    for (int j = 0; j < TJ; ++j) split8<split_pair_packed>(rb[j], pb[j]);
    {
      const int sn = s + p.reps;
      issue(sn < s_end ? sn : s);  // the last one re-reads its own rows: harmless, keeps the loop branch-free
    }
#pragma unroll
    for (int i = 0; i < TI; ++i)
#pragma unroll
      for (int j = 0; j < TJ; ++j) acc[i][j] = mma_x3(pa[i], pb[j], acc[i][j]);
  }

  // 2 / 4 / 8 replicas per tile block meet in LDS (lane-major images, halving rounds), so a tile block issues ONE
  // set of atomics per workgroup however many wavefronts streamed its rows
  if (p.reps > 1) {
    extern __shared__ __attribute__((aligned(16))) float red[];
    constexpr int SLOT = TI * TJ * 1024 + TI * 64;
    for (int h = p.reps >> 1; h >= 1; h >>= 1) {
      if (rep >= h && rep < 2 * h) {
        float* mine = red + ((size_t)tl * (p.reps >> 1) + (rep - h)) * SLOT + lane;
#pragma unroll
        for (int i = 0; i < TI; ++i) {
#pragma unroll
          for (int j = 0; j < TJ; ++j)
#pragma unroll
            for (int q = 0; q < 16; ++q) mine[((i * TJ + j) * 16 + q) * 64] = acc[i][j][q];
          if (WITH_DB) mine[TI * TJ * 1024 + i * 64] = dbacc[i];
        }
      }
      __syncthreads();
      if (rep < h) {
        const float* other = red + ((size_t)tl * (p.reps >> 1) + rep) * SLOT + lane;
#pragma unroll
        for (int i = 0; i < TI; ++i) {
#pragma unroll
          for (int j = 0; j < TJ; ++j)
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[i][j][q] += other[((i * TJ + j) * 16 + q) * 64];
          if (WITH_DB) dbacc[i] += other[TI * TJ * 1024 + i * 64];
        }
      }
      if (h > 1) __syncthreads();  // the next round writes the slots this one read
    }
    if (rep != 0) return;
  }
  if (!active) return;

  // epilogue: C element r of lane l = row n = (r&3) + 8*(r>>2) + 4*half of tile i, column k = l31 of tile j
#pragma unroll
  for (int i = 0; i < TI; ++i) {
#pragma unroll
    for (int j = 0; j < TJ; ++j) {
      const int k = k0 + j * 32 + l31;
      if (k >= p.K || k == p.skip_col) continue;
      const int kk = (p.skip_col >= 0 && k > p.skip_col) ? k - 1 : k;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int n = n0 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
        if (n < p.N) atomicAdd(p.dW + (size_t)n * p.ldw + kk, acc[i][j][r]);
      }
    }
    if (WITH_DB && tj == 0) {
      float t = dbacc[i] + __shfl_xor(dbacc[i], 32, PZN_WAVE);
      if (half == 0 && nok[i]) atomicAdd(p.db + n0 + i * 32 + l31, t);
    }
  }
}

template <int TI, int TJ>
int launch_ij(DfArgs p, hipStream_t st) {
  const int types_n = (p.N + TI * 32 - 1) / (TI * 32);
  p.types_k = (p.K + TJ * 32 - 1) / (TJ * 32);
  const int types = types_n * p.types_k;
  constexpr int MAXW = 12;  // wavefronts per workgroup (<= 168 registers each)
  const int nsteps = p.M / 16;
  constexpr int forced = 0;  // tuning aid
  // long streams: all types of a row range in one workgroup (they re-read the same rows out of L1 / L2); >= 8 steps
  // per wave.
  constexpr int tpw_cap = 12;  // tuning aid (12 = all types together measured best)
  // short row counts (M <= 65536: the attention projections, 16384 rows) are bound by the epilogue atomics — every
  // wave ends with TI*TJ*4 KB of them after only a few steps of rows: ONE tile block per workgroup, eight row replicas
  // that meet in LDS (halving rounds) and >= 8 steps per wave cut the atomics 8x against four tile blocks x two
  // replicas (attention block backward 0.30 -> 0.27 ms); long streams keep every tile block of a row range together
  // (L1 / L2 re-use of the rows)
  constexpr int short_tpw = 1;    // tuning aid
  constexpr int short_reps = 8;  // tuning aid
  const bool short_m = p.M <= 65536;
  const int want = short_m ? short_tpw : tpw_cap;
  const int cap = want < MAXW ? want : MAXW;
  const int groups = (types + cap - 1) / cap;
  p.types_per_wg = (types + groups - 1) / groups;
  // replicas (a power of two, they meet in LDS): as many as fit while every wave keeps >= 4 steps of rows.  One or two
  // tile blocks (131072 x 64 x 64, 131072 x 128 x 64) would otherwise leave 2-4 waves per CU to hide the HBM latency.
  const int rmax = MAXW / p.types_per_wg;
  p.reps = rmax >= 8 ? 8 : (rmax >= 4 ? 4 : (rmax >= 2 ? 2 : 1));
  if (short_m) {
    while (p.reps > short_reps) p.reps >>= 1;
  } else {
    while (p.reps > 2 && nsteps / (256 * p.reps) < 4) p.reps >>= 1;
  }
  constexpr int reps_cap = 0;  // tuning aid
  while (reps_cap > 0 && p.reps > reps_cap) p.reps >>= 1;
  int wgs = 256;
  constexpr int min_steps = 8;  // tuning aid
  constexpr int short_min = 8;  // tuning aid
  const int max_by_steps = nsteps / ((short_m ? short_min : (p.reps > 2 ? 4 : min_steps)) * p.reps);
  if (wgs > max_by_steps) wgs = max_by_steps;
  if (forced) wgs = forced;
  if (wgs < 1) wgs = 1;
  const int waves = p.types_per_wg * p.reps;
  p.steps_per_wg = (nsteps + wgs - 1) / wgs;
  wgs = (nsteps + p.steps_per_wg - 1) / p.steps_per_wg;
  const size_t lds = p.reps > 1 ? (size_t)p.types_per_wg * (p.reps / 2) * (TI * TJ * 1024 + TI * 64) * 4 : 0;  // replica reduction
  if (lds > 64 * 1024) {
    const void* fn = p.genY ? (p.db ? (const void*)df_wgrad_kernel<TI, TJ, true, true> : (const void*)df_wgrad_kernel<TI, TJ, true, false>)
                            : (p.db ? (const void*)df_wgrad_kernel<TI, TJ, false, true> : (const void*)df_wgrad_kernel<TI, TJ, false, false>);
    if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) return PZN_ELAUNCH;
  }
  const dim3 grid((unsigned)wgs, (unsigned)groups), block(waves * 64);
  if (p.genY && p.db)
    PZN_LAUNCH((df_wgrad_kernel<TI, TJ, true, true>), grid, block, lds, st, p);
  else if (p.genY)
    PZN_LAUNCH((df_wgrad_kernel<TI, TJ, true, false>), grid, block, lds, st, p);
  else if (p.db)
    PZN_LAUNCH((df_wgrad_kernel<TI, TJ, false, true>), grid, block, lds, st, p);
  else
    PZN_LAUNCH((df_wgrad_kernel<TI, TJ, false, false>), grid, block, lds, st, p);
  PZN_RETURN_LAUNCH_STATUS();
}

bool df_enabled() {
  constexpr bool on = true;  // tuning aid
  return on;
}

}  // namespace

bool pzn_df_wgrad_supported(int M, int N, int K) {
  if (!df_enabled() || M < 2048 || (M & 15) || N < 1 || K < 1) return false;  // narrow N / K: clamped column loads
  if ((double)M * (N > K ? N : K) * 4.0 >= 2147483648.0) return false;  // buffer offsets are computed in (signed) int
  const int tn = (N + 63) / 64, tk = (K + 63) / 64;
  return tn * tk <= 64;
}

int pzn_df_wgrad(const float* dy, int ldy, const float* genY, const float* x, int ldx, int M, int N, int K, float* dW,
                 int ldw, float* db, int skip_col, hipStream_t st) {
  DfArgs p{dy, ldy, genY, x, ldx, dW, ldw, db, M, N, K, skip_col, 0, 0, 0, 0, 0, {nullptr, nullptr, nullptr}, {0, 0, 0},
           {nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr}};
  const int tn = (N + 31) / 32, tk = (K + 31) / 32;
  if (tn >= 2 && tk >= 2) return launch_ij<2, 2>(p, st);
  if (tn >= 2) return launch_ij<2, 1>(p, st);
  if (tk >= 2) return launch_ij<1, 2>(p, st);
  return launch_ij<1, 1>(p, st);
}

// Three weight gradients that share X in one launch (the q, k, v projections): dW_i[N_i, K] += dY_i^T X,
// db_i += column sums; every N_i a multiple of 64, dY_i dense [M, N_i].
int pzn_df_wgrad3(const float* const dy[3], const int n[3], float* const dW[3], float* const db[3], const float* x, int ldx,
                  int M, int K, hipStream_t st) {
  if (!pzn_df_wgrad_supported(M, n[0] + n[1] + n[2], K) || (n[0] & 63) || (n[1] & 63) || (n[2] & 63) || !db[0] || !db[1] ||
      !db[2])
    return PZN_EUNSUPPORTED;
  DfArgs p{dy[0], n[0], nullptr, x, ldx, dW[0], K, db[0], M, n[0] + n[1] + n[2], K, -1, 0, 0, 0, 0, 3,
           {dy[0], dy[1], dy[2]}, {n[0], n[1], n[2]}, {dW[0], dW[1], dW[2]}, {db[0], db[1], db[2]}};
  return (K + 31) / 32 >= 2 ? launch_ij<2, 2>(p, st) : launch_ij<2, 1>(p, st);
}
