// fewrows.hip — chains of nn.Linear (+ReLU) on a FEW rows (M <= 128: the pose head, 64 rows through
// 2048 -> 1024 -> 512 -> 512 -> 256 -> 6), one launch per layer each way, bf16x3 split precision.
//
// A few-row layer is a latency problem: the weights are read once (11.6 MB for the pose head), the MFMA work is
// negligible, and what is left is launch + one chunk of W + a handful of MFMAs + a store.  The general engine's few-row
// path (gemm.hip) spends three launches per layer on it (zero-fill, split-K product with an atomic epilogue on 128-row
// tiles, bias / ReLU) and its sums depend on the order the atomics arrive in.  Here:
//
//   * a workgroup (4 wavefronts) owns ONE tile of 16 output columns and one chunk of the reduction range; each wavefront
//     takes a quarter of the chunk and all ceil(M / 16) row tiles, fragments straight from global memory
//     (v_mfma_f32_16x16x32_bf16: lane (c, g) holds A[c][8g..8g+7] and B[8g..8g+7][c] - eight consecutive floats of an
//     operand row - and D[4g + r][c]); the four accumulator sets meet in LDS in wavefront order and the workgroup stores
//     its partial tile to part[chunk][M][N] with plain stores: no atomics, no zero-fill;
//   * the CONSUMER reduces: the A operand of the next launch is act(sum_s part[s] + bias), summed in ascending s while it
//     is loaded, so no workgroup waits for, signals or counts another one; the workgroups of column tile 0 also write the
//     reduced rows out (the activations the backward needs).  A last small launch reduces the final layer's partials;
//   * the backward is the same kernel the other way: dx_(i-1)'s partials are sums over chunks of N_i with
//     A = [y_i > 0] * sum_s dpart_i[s] and W read along its rows; the weight and bias gradient of layer i ride in the same
//     launch as a second range of blockIdx (dW_i = (gated dy_i)^T x_i sums over the M rows only: no split);
//   * every sum is fp32 in an order fixed by the shapes alone: results are bit-identical from run to run.
#include <stdlib.h>

#include <initializer_list>

#include "pzn_common.h"
#include "pzn_internal.h"

namespace {

#include "pzn_x3.h"

constexpr int FR_MAX_M = 128;     // rows: at most 8 tiles of 16
constexpr int FR_RT = FR_MAX_M / 16;
constexpr int FR_MAX_L = 16;      // layers of one chain
constexpr int FR_MAX_S = 4;       // chunks of a reduction range: what the consumer re-reduces stays small
constexpr int FR_WG = 256;

// rows[M][K] as an operand of a launch, element (m, k):
//   part == NULL: plain rows in up to two column ranges, p0[m * ld0 + k] for k < k0, p1[m * ld1 + k - k0] beyond;
//   part != NULL: act(sum_{s < S} part[s * sstride + m * ld + k] + bias[k]), ascending s (bias may be NULL, relu 0 / 1);
//   gate != NULL: the value counts where gate[m * gld + k] > 0 and is 0 elsewhere (GEN_RELU of gemm.hip).
// vec = 4 / 2 / 1: the widest unit every row start, column range and pointer of the source is aligned to.
struct FrSrc {
  const float* p0;
  const float* p1;
  const float* part;
  const float* bias;
  const float* gate;
  long sstride;
  int k0, ld0, ld1, ld, gld;
  int S, relu, K, vec;
};

struct FrArgs {
  FrSrc a;              // the streamed rows: x (forward) or dy (backward)
  FrSrc x;              // backward: the layer's input rows (weight gradient)
  const float* W;       // [N][ldw]
  float* part_out;      // [S][M][NO]
  float* ysave;         // forward: a's reduced rows [M][a.K], written by the workgroups of column tile 0 (or NULL)
  float* dW;            // backward: [Nw][Kw] or NULL
  float* db;            // backward: [Nw] or NULL
  int ldw, M, R, NO;    // R: reduction length, NO: output columns
  int KC, NB, n_main;   // chunk length (% 128 == 0), column tiles, workgroups of the product
  int Nw, Kw, NTn, NTk, TPG, accumulate;
};

template <int VEC>
__device__ __forceinline__ void fr_ld(const float* p, float (&t)[VEC]) {
  if constexpr (VEC == 4) {
    const float4 v = *reinterpret_cast<const float4*>(p);
    t[0] = v.x, t[1] = v.y, t[2] = v.z, t[3] = v.w;
  } else if constexpr (VEC == 2) {
    const float2 v = *reinterpret_cast<const float2*>(p);
    t[0] = v.x, t[1] = v.y;
  } else {
    t[0] = *p;
  }
}

// VEC consecutive elements (m, k ..) of a source; k % VEC == 0, the caller has checked m < M and k < K
template <int VEC>
__device__ __forceinline__ void fr_unit(const FrSrc& s, int m, int k, float (&t)[VEC]) {
  if (s.part) {
    const float* p = s.part + (long)m * s.ld + k;
    fr_ld<VEC>(p, t);
    for (int i = 1; i < s.S; ++i) {
      float u[VEC];
      fr_ld<VEC>(p + i * s.sstride, u);
#pragma unroll
      for (int e = 0; e < VEC; ++e) t[e] += u[e];
    }
    if (s.bias) {
      float u[VEC];
      fr_ld<VEC>(s.bias + k, u);
#pragma unroll
      for (int e = 0; e < VEC; ++e) t[e] += u[e];
    }
    if (s.relu) {
#pragma unroll
      for (int e = 0; e < VEC; ++e) t[e] = fmaxf(t[e], 0.f);
    }
  } else {
    fr_ld<VEC>(k < s.k0 ? s.p0 + (long)m * s.ld0 + k : s.p1 + (long)m * s.ld1 + (k - s.k0), t);
  }
  if (s.gate) {
    float u[VEC];
    fr_ld<VEC>(s.gate + (long)m * s.gld + k, u);
#pragma unroll
    for (int e = 0; e < VEC; ++e) t[e] = u[e] > 0.f ? t[e] : 0.f;
  }
}

// elements (m, k .. k + 7) -> v (zeros outside the rows / columns); save != NULL: the units are also written to save[m][K]
template <int VEC>
__device__ __forceinline__ void fr_row8(const FrSrc& s, int m, int M, int k, float (&v)[8], float* save) {
#pragma unroll
  for (int u = 0; u < 8 / VEC; ++u) {
    const int kk = k + u * VEC;
    float t[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) t[e] = 0.f;
    if (m < M && kk < s.K) {
      fr_unit<VEC>(s, m, kk, t);
      if (save) {
        float* d = save + (long)m * s.K + kk;
        if constexpr (VEC == 4) *reinterpret_cast<float4*>(d) = make_float4(t[0], t[1], t[2], t[3]);
        else if constexpr (VEC == 2) *reinterpret_cast<float2*>(d) = make_float2(t[0], t[1]);
        else *d = t[0];
      }
    }
#pragma unroll
    for (int e = 0; e < VEC; ++e) v[u * VEC + e] = t[e];
  }
}
__device__ __forceinline__ void fr_row8_any(const FrSrc& s, int m, int M, int k, float (&v)[8], float* save) {
  if (s.vec == 4) fr_row8<4>(s, m, M, k, v, save);
  else if (s.vec == 2) fr_row8<2>(s, m, M, k, v, save);
  else fr_row8<1>(s, m, M, k, v, save);
}
__device__ __forceinline__ float fr_elem(const FrSrc& s, int m, int M, int k) {
  float t[1] = {0.f};
  if (m < M && k < s.K) fr_unit<1>(s, m, k, t);
  return t[0];
}

// WT = false (forward): part_out[s][m][n] = sum over chunk s of a(m, k) W[n][k]
// WT = true (backward): part_out[s][m][k] = sum over chunk s of a(m, n) W[n][k]; workgroups n_main .. carry dW / db
// Operands of any width and alignment (a.vec = 2 / 1: widths that are no multiple of 4), every load behind its own bounds
// check; the aligned case, the pose head's, is fewrow_layer_kernel below - same tiles, same sums, same bits.
template <bool WT>
__global__ __launch_bounds__(FR_WG) void fewrow_layer_any_kernel(FrArgs p) {
  __shared__ float4 red[4][FR_RT][64];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int c = lane & 15, g = lane >> 4;
  const int bx = blockIdx.x;

  if (WT && bx >= p.n_main) {
    // ---- weight / bias gradient: dW[n][k] = sum_m a(m, n) x(m, k), one tile of 16 n per workgroup, TPG tiles of 16 k
    const int j = bx - p.n_main;
    const int nt = j % p.NTn, kg = j / p.NTn;
    const int n = nt * 16 + c;
    const int MS = (p.M + 31) >> 5;            // reduction steps of 32 rows (<= 4)
    bf16x8 af[4][3];
    float colsum = 0.f;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      if (ks < MS) {
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          v[e] = fr_elem(p.a, 32 * ks + 8 * g + e, p.M, n);
          colsum += v[e];
        }
        split8<split_pair_scalar>(v, af[ks]);
      }
    }
    if (kg == 0 && wave == 0 && p.db) {                     // rows 8g .. of every step on lane group g: the four groups in lane order
      const float s1 = colsum + __shfl_xor(colsum, 16, 64);
      const float s2 = s1 + __shfl_xor(s1, 32, 64);
      if (g == 0 && n < p.Nw) p.db[n] = p.accumulate ? p.db[n] + s2 : s2;
    }
    for (int t = wave; t < p.TPG; t += 4) {
      const int kt = kg * p.TPG + t;
      if (kt >= p.NTk) break;
      const int k = kt * 16 + c;
      floatx4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        if (ks < MS) {
          float v[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] = fr_elem(p.x, 32 * ks + 8 * g + e, p.M, k);
          bf16x8 bfr[3];
          split8<split_pair_scalar>(v, bfr);
          acc = mma_x3<3>(af[ks], bfr, acc);
        }
      }
      if (k < p.Kw) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = nt * 16 + 4 * g + r;
          if (row < p.Nw) {
            float* d = p.dW + (long)row * p.Kw + k;
            *d = p.accumulate ? *d + acc[r] : acc[r];
          }
        }
      }
    }
    return;
  }

  // ---- the product: column tile cb, chunk sc; wavefront w walks a quarter of the chunk over every row tile
  const int cb = bx % p.NB, sc = bx / p.NB;
  const int col = cb * 16 + c;
  const bool colok = col < p.NO;
  const int RT = (p.M + 15) >> 4;
  const int kq = p.KC >> 2;                    // % 32 == 0
  const int kbeg = sc * p.KC + wave * kq;
  float* save = (!WT && cb == 0) ? p.ysave : nullptr;
  const bool wvec = !WT && p.a.vec == 4 && (p.ldw & 3) == 0;

  floatx4 acc[FR_RT];
#pragma unroll
  for (int rt = 0; rt < FR_RT; ++rt) acc[rt] = floatx4{0.f, 0.f, 0.f, 0.f};

  for (int kb = kbeg; kb < kbeg + kq && kb < p.R; kb += 32) {
    const int k = kb + 8 * g;
    float w[8];
    if (WT) {
#pragma unroll
      for (int e = 0; e < 8; ++e) w[e] = (colok && k + e < p.R) ? p.W[(long)(k + e) * p.ldw + col] : 0.f;
    } else if (wvec) {
      const float* wp = p.W + (long)col * p.ldw + k;
      const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
      const float4 w0 = (colok && k < p.R) ? *reinterpret_cast<const float4*>(wp) : z;
      const float4 w1 = (colok && k + 4 < p.R) ? *reinterpret_cast<const float4*>(wp + 4) : z;
      w[0] = w0.x, w[1] = w0.y, w[2] = w0.z, w[3] = w0.w, w[4] = w1.x, w[5] = w1.y, w[6] = w1.z, w[7] = w1.w;
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) w[e] = (colok && k + e < p.R) ? p.W[(long)col * p.ldw + k + e] : 0.f;
    }
    bf16x8 bfr[3];
    split8<split_pair_scalar>(w, bfr);
#pragma unroll
    for (int rt = 0; rt < FR_RT; ++rt) {
      if (rt < RT) {
        float v[8];
        fr_row8_any(p.a, 16 * rt + c, p.M, k, v, save);
        bf16x8 afr[3];
        split8<split_pair_scalar>(v, afr);
        acc[rt] = mma_x3<3>(afr, bfr, acc[rt]);
      }
    }
  }

  // the four quarters of the chunk, summed in wavefront order
#pragma unroll
  for (int rt = 0; rt < FR_RT; ++rt)
    if (rt < RT) red[wave][rt][lane] = make_float4(acc[rt][0], acc[rt][1], acc[rt][2], acc[rt][3]);
  __syncthreads();
  float* out = p.part_out + (long)sc * p.M * p.NO;
  for (int rt = wave; rt < RT; rt += 4) {
    const float4 q0 = red[0][rt][lane], q1 = red[1][rt][lane], q2 = red[2][rt][lane], q3 = red[3][rt][lane];
    const float s[4] = {((q0.x + q1.x) + q2.x) + q3.x, ((q0.y + q1.y) + q2.y) + q3.y, ((q0.z + q1.z) + q2.z) + q3.z,
                        ((q0.w + q1.w) + q2.w) + q3.w};
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 16 * rt + 4 * g + r;
      if (row < p.M && colok) out[(long)row * p.NO + col] = s[r];
    }
  }
}

// ---- the aligned case (a.vec == 4).  A few-row launch is a chain of memory round trips, so the loads of a step are issued as
// ONE batch with nothing to branch around: addresses are clamped into the operand instead of checked (rows >= M and
// columns >= N only feed outputs that are never stored; the reduction tail is zeroed by selects), the number of partial
// sums is a template argument chosen by a wavefront-uniform switch, and absent bias / gate pointers are replaced by the
// operand's own address and their values dropped by selects.  RTC = row tiles compiled in: 1, 2, 4 or 8.

__device__ __forceinline__ float4 fr_ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ float4 fr_add4(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }

// address of element (m, k) of the first partial sum / of the plain rows (fr_plain and fr_partial fill p0, p1, k0 alike)
__device__ __forceinline__ const float* fr_base(const FrSrc& s, int m, int k) {
  return k < s.k0 ? s.p0 + (long)m * s.ld0 + k : s.p1 + (long)m * s.ld1 + (k - s.k0);
}

// v[rt][0..7] = a(16 (rt0 + rt) + c, k .. k + 7) for NRT row tiles; save: also written to save[m][K] (rows < M)
// (plain rows of any width, the backward's dy[M][6]: the same batch with eight clamped dword loads per row)
template <int NRT>
__device__ __forceinline__ void fr_batch_dwords(const FrSrc& s, int M, int c, int rt0, int k, float (&v)[NRT][8]) {
  float raw[NRT][8], gt[NRT][8];
#pragma unroll
  for (int rt = 0; rt < NRT; ++rt) {
    const int m = min(16 * (rt0 + rt) + c, M - 1);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int kk = k + e < s.K ? k + e : 0;
      raw[rt][e] = *fr_base(s, m, kk);
      gt[rt][e] = s.gate ? s.gate[(long)m * s.gld + kk] : 1.f;
    }
  }
#pragma unroll
  for (int rt = 0; rt < NRT; ++rt)
#pragma unroll
    for (int e = 0; e < 8; ++e) v[rt][e] = (k + e < s.K && gt[rt][e] > 0.f) ? raw[rt][e] : 0.f;
}

template <int SS, int NRT>
__device__ __forceinline__ void fr_batch(const FrSrc& s, int M, int c, int rt0, int k, float (&v)[NRT][8], float* save) {
  const bool in[2] = {k < s.K, k + 4 < s.K};
  const int kc[2] = {in[0] ? k : 0, in[1] ? k + 4 : 0};
  float4 raw[NRT][2][SS], gt[NRT][2], bs[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) bs[h] = fr_ld4(s.bias ? s.bias + kc[h] : fr_base(s, 0, kc[h]));
#pragma unroll
  for (int rt = 0; rt < NRT; ++rt) {
    const int m = min(16 * (rt0 + rt) + c, M - 1);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const float* b = fr_base(s, m, kc[h]);
#pragma unroll
      for (int i = 0; i < SS; ++i) raw[rt][h][i] = fr_ld4(b + i * s.sstride);
      gt[rt][h] = fr_ld4(s.gate ? s.gate + (long)m * s.gld + kc[h] : b);
    }
  }
  const bool has_bias = s.bias != nullptr, relu = s.relu != 0, gated = s.gate != nullptr;
#pragma unroll
  for (int rt = 0; rt < NRT; ++rt) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      float4 t = raw[rt][h][0];
#pragma unroll
      for (int i = 1; i < SS; ++i) t = fr_add4(t, raw[rt][h][i]);
      if (has_bias) t = fr_add4(t, bs[h]);
      if (relu) t = make_float4(fmaxf(t.x, 0.f), fmaxf(t.y, 0.f), fmaxf(t.z, 0.f), fmaxf(t.w, 0.f));
      const float4 q = gt[rt][h];
      float* o = &v[rt][4 * h];
      o[0] = (in[h] && (!gated || q.x > 0.f)) ? t.x : 0.f;
      o[1] = (in[h] && (!gated || q.y > 0.f)) ? t.y : 0.f;
      o[2] = (in[h] && (!gated || q.z > 0.f)) ? t.z : 0.f;
      o[3] = (in[h] && (!gated || q.w > 0.f)) ? t.w : 0.f;
    }
  }
  if (save) {
#pragma unroll
    for (int rt = 0; rt < NRT; ++rt) {
      const int m = 16 * (rt0 + rt) + c;
#pragma unroll
      for (int h = 0; h < 2; ++h)
        if (m < M && in[h])
          *reinterpret_cast<float4*>(save + (long)m * s.K + k + 4 * h) = make_float4(v[rt][4 * h], v[rt][4 * h + 1], v[rt][4 * h + 2], v[rt][4 * h + 3]);
    }
  }
}
template <int NRT>
__device__ __forceinline__ void fr_batch_any(const FrSrc& s, int M, int c, int rt0, int k, float (&v)[NRT][8], float* save) {
  if (s.vec != 4) {  // (host: a plain source without bias, and nothing to save)
    fr_batch_dwords<NRT>(s, M, c, rt0, k, v);
    return;
  }
  switch (s.S) {   // wavefront-uniform
    case 1: fr_batch<1, NRT>(s, M, c, rt0, k, v, save); break;
    case 2: fr_batch<2, NRT>(s, M, c, rt0, k, v, save); break;
    case 3: fr_batch<3, NRT>(s, M, c, rt0, k, v, save); break;
    default: fr_batch<4, NRT>(s, M, c, rt0, k, v, save); break;
  }
}

// the weight gradient's A operand: v[ks][e] = a(32 ks + 8 g + e, n), zero for rows >= M (the reduction index here)
template <int SS, int MS>
__device__ __forceinline__ void fr_cols(const FrSrc& s, int M, int g, int n, float (&v)[MS][8]) {
  float raw[MS][8][SS], gt[MS][8];
#pragma unroll
  for (int ks = 0; ks < MS; ++ks)
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int m = min(32 * ks + 8 * g + e, M - 1);
      const float* b = fr_base(s, m, n);
#pragma unroll
      for (int i = 0; i < SS; ++i) raw[ks][e][i] = b[i * s.sstride];
      gt[ks][e] = s.gate ? s.gate[(long)m * s.gld + n] : 1.f;
    }
  const bool has_bias = s.bias != nullptr, relu = s.relu != 0;
  const float bv = has_bias ? s.bias[n] : 0.f;
#pragma unroll
  for (int ks = 0; ks < MS; ++ks)
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float t = raw[ks][e][0];
#pragma unroll
      for (int i = 1; i < SS; ++i) t += raw[ks][e][i];
      if (has_bias) t += bv;
      if (relu) t = fmaxf(t, 0.f);
      v[ks][e] = (32 * ks + 8 * g + e < M && gt[ks][e] > 0.f) ? t : 0.f;
    }
}

template <bool WT, int RTC>
__global__ __launch_bounds__(FR_WG) void fewrow_layer_kernel(FrArgs p) {
  __shared__ float4 red[4][RTC][64];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int c = lane & 15, g = lane >> 4;
  const int bx = blockIdx.x;

  if (WT && bx >= p.n_main) {
    // ---- weight / bias gradient: one tile of 16 n per workgroup, TPG tiles of 16 k, two at a time on every wavefront
    constexpr int MS = (RTC + 1) / 2;          // reduction steps of 32 rows
    const int j = bx - p.n_main;
    const int nt = j % p.NTn, kg = j / p.NTn;
    const int n = nt * 16 + c, nc = min(n, p.Nw - 1);
    float v[MS][8];
    switch (p.a.S) {
      case 1: fr_cols<1, MS>(p.a, p.M, g, nc, v); break;
      case 2: fr_cols<2, MS>(p.a, p.M, g, nc, v); break;
      case 3: fr_cols<3, MS>(p.a, p.M, g, nc, v); break;
      default: fr_cols<4, MS>(p.a, p.M, g, nc, v); break;
    }
    bf16x8 af[MS][3];
    float colsum = 0.f;
#pragma unroll
    for (int ks = 0; ks < MS; ++ks) {
#pragma unroll
      for (int e = 0; e < 8; ++e) colsum += v[ks][e];
      split8<split_pair_scalar>(v[ks], af[ks]);
    }
    if (kg == 0 && wave == 0 && p.db) {
      const float s1 = colsum + __shfl_xor(colsum, 16, 64);
      const float s2 = s1 + __shfl_xor(s1, 32, 64);
      if (g == 0 && n < p.Nw) p.db[n] = p.accumulate ? p.db[n] + s2 : s2;
    }
    for (int t = 2 * wave; t < p.TPG; t += 8) {
      const int kt = kg * p.TPG + t;
      if (kt >= p.NTk) break;
      float x[2][MS][8], old[2][4];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int kc = min((kt + u) * 16 + c, p.Kw - 1);
#pragma unroll
        for (int ks = 0; ks < MS; ++ks)
#pragma unroll
          for (int e = 0; e < 8; ++e) x[u][ks][e] = *fr_base(p.x, min(32 * ks + 8 * g + e, p.M - 1), kc);
#pragma unroll
        for (int r = 0; r < 4; ++r)
          old[u][r] = p.accumulate ? p.dW[(long)min(nt * 16 + 4 * g + r, p.Nw - 1) * p.Kw + kc] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        floatx4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < MS; ++ks) {
          bf16x8 bfr[3];
          split8<split_pair_scalar>(x[u][ks], bfr);
          acc = mma_x3<3>(af[ks], bfr, acc);
        }
        const int k = (kt + u) * 16 + c;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = nt * 16 + 4 * g + r;
          if (row < p.Nw && k < p.Kw) p.dW[(long)row * p.Kw + k] = p.accumulate ? old[u][r] + acc[r] : acc[r];
        }
      }
    }
    return;
  }

  // ---- the product: column tile cb, chunk sc; wavefront w walks a quarter of the chunk over every row tile
  const int cb = bx % p.NB, sc = bx / p.NB;
  const int col = cb * 16 + c;
  const bool colok = col < p.NO;
  const int colc = min(col, p.NO - 1);
  const int kq = p.KC >> 2;
  const int kbeg = sc * p.KC + wave * kq;
  float* save = (!WT && cb == 0) ? p.ysave : nullptr;
  constexpr int NRT = RTC < 4 ? RTC : 4;       // row tiles of one batch of loads

  floatx4 acc[RTC];
#pragma unroll
  for (int rt = 0; rt < RTC; ++rt) acc[rt] = floatx4{0.f, 0.f, 0.f, 0.f};

  for (int kb = kbeg; kb < kbeg + kq && kb < p.R; kb += 32) {
    const int k = kb + 8 * g;
    float w[8];
    if (WT) {
#pragma unroll
      for (int e = 0; e < 8; ++e) w[e] = p.W[(long)min(k + e, p.R - 1) * p.ldw + colc];
#pragma unroll
      for (int e = 0; e < 8; ++e) w[e] = k + e < p.R ? w[e] : 0.f;
    } else {
      const float* wp = p.W + (long)colc * p.ldw;
      const float4 w0 = fr_ld4(wp + (k < p.R ? k : 0)), w1 = fr_ld4(wp + (k + 4 < p.R ? k + 4 : 0));
      w[0] = w0.x, w[1] = w0.y, w[2] = w0.z, w[3] = w0.w, w[4] = w1.x, w[5] = w1.y, w[6] = w1.z, w[7] = w1.w;
#pragma unroll
      for (int e = 0; e < 8; ++e) w[e] = k + (e & 4) < p.R ? w[e] : 0.f;
    }
    bf16x8 bfr[3];
#pragma unroll
    for (int rt0 = 0; rt0 < RTC; rt0 += NRT) {
      float v[NRT][8];
      fr_batch_any<NRT>(p.a, p.M, c, rt0, k, v, save);
      if (rt0 == 0) split8<split_pair_scalar>(w, bfr);
#pragma unroll
      for (int rt = 0; rt < NRT; ++rt) {
        bf16x8 afr[3];
        split8<split_pair_scalar>(v[rt], afr);
        acc[rt0 + rt] = mma_x3<3>(afr, bfr, acc[rt0 + rt]);
      }
    }
  }

#pragma unroll
  for (int rt = 0; rt < RTC; ++rt) red[wave][rt][lane] = make_float4(acc[rt][0], acc[rt][1], acc[rt][2], acc[rt][3]);
  __syncthreads();
  float* out = p.part_out + (long)sc * p.M * p.NO;
  const int RT = (p.M + 15) >> 4;
  for (int rt = wave; rt < RT; rt += 4) {
    const float4 q0 = red[0][rt][lane], q1 = red[1][rt][lane], q2 = red[2][rt][lane], q3 = red[3][rt][lane];
    const float s[4] = {((q0.x + q1.x) + q2.x) + q3.x, ((q0.y + q1.y) + q2.y) + q3.y, ((q0.z + q1.z) + q2.z) + q3.z,
                        ((q0.w + q1.w) + q2.w) + q3.w};
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 16 * rt + 4 * g + r;
      if (row < p.M && colok) out[(long)row * p.NO + col] = s[r];
    }
  }
}

// out(m, n) = act(sum_s part[s][m][n] + bias[n]), columns < n0 to out0[M][n0], the others to out1[M][N - n0] (either may be NULL)
__global__ __launch_bounds__(256) void fewrow_reduce_kernel(const float* __restrict__ part, int S, int M, int N,
                                                            const float* __restrict__ bias, int relu, float* out0, int n0,
                                                            float* out1) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long total = (long)M * N;
  if (i >= total) return;
  const int m = (int)(i / N), n = (int)(i - (long)m * N);
  float t = part[i];
  for (int s = 1; s < S; ++s) t += part[s * total + i];
  if (bias) t += bias[n];
  if (relu) t = fmaxf(t, 0.f);
  if (n < n0) {
    if (out0) out0[(long)m * n0 + n] = t;
  } else if (out1) {
    out1[(long)m * (N - n0) + (n - n0)] = t;
  }
}

// ------------------------------------------------------------------------------------------ host

struct FrPlan {
  int NB, S, KC;
};
// chunks of a reduction range R for NO output columns: about `wgs` workgroups, at most FR_MAX_S chunks of a multiple of 128.
// A launch should be ONE round of workgroups (a workgroup fills a CU's registers): the forward aims at 256, the backward
// at 128 for the input gradient beside 128 for the weight gradient.
constexpr int FR_WGS_FWD = 256, FR_WGS_BWD = 128;
FrPlan fr_plan(int R, int NO, int wgs) {
  FrPlan q;
  q.NB = (NO + 15) / 16;
  int s = wgs / q.NB;
  const int most = (R + 127) / 128;
  s = s > FR_MAX_S ? FR_MAX_S : s;
  s = s > most ? most : s;
  s = s < 1 ? 1 : s;
  q.KC = (((R + s - 1) / s + 127) / 128) * 128;
  q.S = (R + q.KC - 1) / q.KC;
  return q;
}

// the batched kernel where the streamed rows are 16-byte units (or, backward, plain rows of any width); RTC from M
template <bool WT>
void fr_launch(const FrArgs& p, int blocks, hipStream_t st) {
  const dim3 grid((unsigned)blocks), block(FR_WG);
  if (!(p.a.vec == 4 || (WT && !p.a.part))) {
    PZN_LAUNCH(fewrow_layer_any_kernel<WT>, grid, block, 0, st, p);
  } else if (p.M <= 16) {
    PZN_LAUNCH((fewrow_layer_kernel<WT, 1>), grid, block, 0, st, p);
  } else if (p.M <= 32) {
    PZN_LAUNCH((fewrow_layer_kernel<WT, 2>), grid, block, 0, st, p);
  } else if (p.M <= 64) {
    PZN_LAUNCH((fewrow_layer_kernel<WT, 4>), grid, block, 0, st, p);
  } else {
    PZN_LAUNCH((fewrow_layer_kernel<WT, 8>), grid, block, 0, st, p);
  }
}

bool fr_aligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

int fr_vec(std::initializer_list<int> lens) {
  int v = 4;
  for (int n : lens) v = (n % 4 == 0) ? v : (n % 2 == 0 ? (v < 2 ? v : 2) : 1);
  return v;
}

FrSrc fr_plain(const float* p0, int k0, const float* p1, int k1) {
  FrSrc s = {};
  s.p0 = p0, s.p1 = p1 ? p1 : p0, s.k0 = k0, s.ld0 = k0, s.ld1 = k1, s.K = k0 + k1, s.S = 1;
  s.vec = k1 > 0 ? fr_vec({k0, k1}) : fr_vec({k0});
  return s;
}
FrSrc fr_partial(const float* part, int S, int M, int K, const float* bias, int relu) {
  FrSrc s = {};
  s.part = part, s.S = S, s.sstride = (long)M * K, s.ld = K, s.K = K, s.bias = bias, s.relu = relu;
  s.p0 = s.p1 = part, s.k0 = s.ld0 = s.ld1 = K;
  s.vec = fr_vec({K});
  return s;
}

bool fr_shapes_ok(int M, int L, const int* widths) {
  if (!widths || M < 1 || M > FR_MAX_M || L < 1 || L > FR_MAX_L) return false;
  for (int i = 0; i <= L; ++i)
    if (widths[i] < 1) return false;
  if (widths[0] < 256) return false;           // the range that is split across the chip
  for (int i = 1; i < L; ++i)
    if (widths[i] <= 64) return false;         // narrower inner layers belong to the per-point chain kernels (pointmlp.hip)
  return true;
}

size_t fr_ws_floats(int M, int L, const int* widths) {
  size_t fwd = 0, bwd = 0;
  for (int i = 0; i < L; ++i) {
    fwd += (size_t)fr_plan(widths[i], widths[i + 1], FR_WGS_FWD).S * M * widths[i + 1];
    bwd += (size_t)fr_plan(widths[i + 1], widths[i], FR_WGS_BWD).S * M * widths[i];
  }
  return fwd > bwd ? fwd : bwd;
}

}  // namespace

PZN_EXPORT int pzn_fewrow_chain_supported(int M, int L, const int* widths) {
  return pzn_gemm_get_precision() != 0 && fr_shapes_ok(M, L, widths) ? 1 : 0;
}

PZN_EXPORT size_t pzn_fewrow_chain_workspace_bytes(int M, int L, const int* widths) {
  if (!fr_shapes_ok(M, L, widths)) return 0;
  return fr_ws_floats(M, L, widths) * sizeof(float);
}

PZN_EXPORT int pzn_fewrow_chain_fwd_f32(const float* x0, int k0, const float* x1, int k1, int M, int L, const int* widths,
                                        const float* const* W, const float* const* bias, const int* relu, float* const* y,
                                        void* workspace, size_t workspace_bytes, pzn_stream_t stream) {
  PZN_CHECK_ARG(x0 && k0 > 0 && k1 >= 0 && (k1 == 0 || x1) && widths && W && bias && relu && y && workspace && L >= 1);
  if (!pzn_fewrow_chain_supported(M, L, widths)) return PZN_EUNSUPPORTED;
  PZN_CHECK_ARG(widths[0] == k0 + k1 && workspace_bytes >= fr_ws_floats(M, L, widths) * sizeof(float));
  if (!fr_aligned(x0) || !fr_aligned(x1) || !fr_aligned(workspace)) return PZN_EUNSUPPORTED;
  for (int i = 0; i < L; ++i) {
    PZN_CHECK_ARG(W[i] && y[i]);
    if (!fr_aligned(W[i]) || !fr_aligned(bias[i]) || !fr_aligned(y[i])) return PZN_EUNSUPPORTED;
  }
  hipStream_t st = pzn_hip_stream(stream);
  float* ws = static_cast<float*>(workspace);
  FrSrc src = fr_plain(x0, k0, x1, k1);
  FrPlan q = {};
  for (int i = 0; i < L; ++i) {
    const int K = widths[i], N = widths[i + 1];
    q = fr_plan(K, N, FR_WGS_FWD);
    FrArgs p = {};
    p.a = src;
    p.W = W[i], p.ldw = K, p.M = M, p.R = K, p.NO = N, p.KC = q.KC, p.NB = q.NB, p.n_main = q.NB * q.S;
    p.part_out = ws;
    p.ysave = i > 0 ? y[i - 1] : nullptr;
    fr_launch<false>(p, p.n_main, st);
    src = fr_partial(ws, q.S, M, N, bias[i], relu[i]);
    ws += (size_t)q.S * M * N;
  }
  const int N = widths[L];
  const long total = (long)M * N;
  PZN_LAUNCH(fewrow_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, src.part, src.S, M, N, src.bias,
             src.relu, y[L - 1], N, static_cast<float*>(nullptr));
  PZN_RETURN_LAUNCH_STATUS();
}

PZN_EXPORT int pzn_fewrow_chain_bwd_f32(const float* dy, const float* x0, int k0, const float* x1, int k1, int M, int L,
                                        const int* widths, const float* const* W, const int* relu, const float* const* y,
                                        float* dx0, float* dx1, float* const* dW, float* const* db, const int* accumulate,
                                        void* workspace, size_t workspace_bytes, pzn_stream_t stream) {
  PZN_CHECK_ARG(dy && x0 && k0 > 0 && k1 >= 0 && (k1 == 0 || x1) && widths && W && relu && y && dW && db && accumulate &&
                workspace && L >= 1);
  if (!pzn_fewrow_chain_supported(M, L, widths)) return PZN_EUNSUPPORTED;
  PZN_CHECK_ARG(widths[0] == k0 + k1 && workspace_bytes >= fr_ws_floats(M, L, widths) * sizeof(float));
  if (!fr_aligned(dy) || !fr_aligned(x0) || !fr_aligned(x1) || !fr_aligned(dx0) || !fr_aligned(dx1) || !fr_aligned(workspace))
    return PZN_EUNSUPPORTED;
  for (int i = 0; i < L; ++i) {
    PZN_CHECK_ARG(W[i] && y[i]);
    if (!fr_aligned(W[i]) || !fr_aligned(y[i]) || !fr_aligned(dW[i]) || !fr_aligned(db[i])) return PZN_EUNSUPPORTED;
  }
  hipStream_t st = pzn_hip_stream(stream);
  float* ws = static_cast<float*>(workspace);
  const bool need_dx = dx0 || dx1;
  FrSrc src = fr_plain(dy, widths[L], nullptr, 0);
  FrPlan q = {};
  for (int i = L - 1; i >= 0; --i) {
    const int K = widths[i], N = widths[i + 1];
    if (relu[i]) src.gate = y[i], src.gld = N;
    q = fr_plan(N, K, FR_WGS_BWD);
    FrArgs p = {};
    p.a = src;
    p.W = W[i], p.ldw = K, p.M = M, p.R = N, p.NO = K, p.KC = q.KC, p.NB = q.NB;
    p.n_main = (i > 0 || need_dx) ? q.NB * q.S : 0;
    p.part_out = ws;
    int n_w = 0;
    if (dW[i]) {
      p.x = i > 0 ? fr_plain(y[i - 1], K, nullptr, 0) : fr_plain(x0, k0, x1, k1);
      p.dW = dW[i], p.db = db[i], p.accumulate = accumulate[i];
      p.Nw = N, p.Kw = K, p.NTn = (N + 15) / 16, p.NTk = (K + 15) / 16;
      const int per = (p.NTn * p.NTk + FR_WGS_BWD - 1) / FR_WGS_BWD;
      p.TPG = per < 8 ? 8 : ((per + 7) / 8) * 8;   // two tiles at a time on each of the four wavefronts
      n_w = p.NTn * ((p.NTk + p.TPG - 1) / p.TPG);
    }
    if (p.n_main + n_w > 0)
      fr_launch<true>(p, p.n_main + n_w, st);
    src = fr_partial(ws, q.S, M, K, nullptr, 0);
    ws += (size_t)q.S * M * K;
  }
  if (need_dx) {
    const long total = (long)M * widths[0];
    PZN_LAUNCH(fewrow_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, src.part, src.S, M, widths[0],
               static_cast<const float*>(nullptr), 0, dx0, k0, dx1);
  }
  PZN_RETURN_LAUNCH_STATUS();
}
