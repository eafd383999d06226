// mergefps.hip — merge two placed pieces and resample the union, for gfx950 (assembly.ProgressiveAssembler).
//
// One workgroup per merge m does what would otherwise be se3.transform_points -> cat -> farthest_point_sample ->
// index_points with a (Na + Nb)-point intermediate, and two things that chain cannot do: rows of the matched faces
// (drop_a / drop_b) start at running distance 0, so they are picked only when every kept row is at 0 too, and every output
// point reports the union row it came from (src).
//   * load: a[m] and b[m] are read from HBM once each, as flat coalesced copies into one SoA image in LDS (a first); the
//     owner of a row of b then replaces it IN the image by T[m] applied to it, x' = ((R00 x + R01 y) + R02 z) + t0, every
//     product and sum rounded on its own (__fmul_rn / __fadd_rn: the order tests/_merge_ref.py restates);
//   * drops: one flag byte per union row in LDS (indices may repeat: every writer stores the same byte);
//   * start: start[m] if that row is kept, otherwise the first kept row at or after it, wrapping round to 0: one
//     wavefront-uniform scan of the flag bytes, 64 rows per step, done by every wavefront alike before the rounds;
//   * rounds: pzn_fps_round.h, the round of fps.hip's image form - the arithmetic is the same code, so with an identity
//     pose and no drops the picks are pzn_fps_f32's on cat(a, b) bit for bit, and the lowest union index wins ties;
//   * epilogue: the round's pick buffer flushes src (int64 union index) and out (the coordinates from the image: a rows as
//     read, b rows as transformed).
// This file's own: the pose transform into the image, the drop flags, the start scan and the coordinate write-out.
// The round is a latency chain (n_out dependent rounds); the launch is parallel over merges only.
#include "pzn_common.h"

namespace {

#include "pzn_fps_round.h"

constexpr int MRG_T = 256;              // four wavefronts: the round's cross-wave part grows with the wave count (fps.hip)
constexpr int MRG_MAX_UNION = 4096;     // 48 KB image + 4 KB flags + slots and pick buffer: below the 64 KB default

template <int T, int PPT>
__global__ __launch_bounds__(T) void merge_resample_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                           const float* __restrict__ pose, const int64_t* __restrict__ start,
                                                           const int64_t* __restrict__ drop_a, int ka,
                                                           const int64_t* __restrict__ drop_b, int kb, int Na, int Nb,
                                                           int n_out, float* __restrict__ out, int64_t* __restrict__ src) {
  constexpr int W = T / PZN_WAVE;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int U = Na + Nb;
  uint64_t* slots = reinterpret_cast<uint64_t*>(smem_raw);                              // [2][W]
  int* sout = reinterpret_cast<int*>(smem_raw + 2 * W * sizeof(uint64_t));              // [FPS_OUT_CHUNK] picks not yet written out
  float* sx = reinterpret_cast<float*>(smem_raw + fps_lds_head(W));
  float* sy = sx + U;
  float* sz = sy + U;
  unsigned char* sdrop = reinterpret_cast<unsigned char*>(sz + U);                      // [U] 1 = dropped row

  const int m = blockIdx.x;
  const int tid = (int)threadIdx.x;
  const int lane = tid & (PZN_WAVE - 1);
  const int wave = tid / PZN_WAVE;
  const float* ga = a + (size_t)m * Na * 3;
  const float* gb = b + (size_t)m * Nb * 3;
  const float* g = pose + (size_t)m * 16;

  // load: both clouds once, flat and coalesced, into the union's SoA image; the flags start clear
  fps_load_soa<T>(ga, Na, sx, sy, sz, 0, tid);
  fps_load_soa<T>(gb, Nb, sx, sy, sz, Na, tid);
  for (int i = tid; i < U; i += T) sdrop[i] = 0;
  __syncthreads();
  // drop lists (an index outside its cloud is ignored)
  if (drop_a)
    for (int i = tid; i < ka; i += T) {
      const int64_t r = drop_a[(size_t)m * ka + i];
      if (r >= 0 && r < Na) sdrop[(int)r] = 1;
    }
  if (drop_b)
    for (int i = tid; i < kb; i += T) {
      const int64_t r = drop_b[(size_t)m * kb + i];
      if (r >= 0 && r < Nb) sdrop[Na + (int)r] = 1;
    }
  const float r00 = g[0], r01 = g[1], r02 = g[2], t0 = g[3];
  const float r10 = g[4], r11 = g[5], r12 = g[6], t1 = g[7];
  const float r20 = g[8], r21 = g[9], r22 = g[10], t2 = g[11];
  __syncthreads();

  // every thread's rows into registers; a row of b is transformed on the way and put back into the image (its owner is the
  // only thread that touches that slot before the barrier below)
  float px[PPT], py[PPT], pz[PPT], dist[PPT];
#pragma unroll
  for (int p = 0; p < PPT; ++p) {
    const int j = tid + p * T;
    const bool ok = j < U;
    float x = ok ? sx[j] : 0.f, y = ok ? sy[j] : 0.f, z = ok ? sz[j] : 0.f;
    if (ok && j >= Na) {
      const float nx = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(r00, x), __fmul_rn(r01, y)), __fmul_rn(r02, z)), t0);
      const float ny = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(r10, x), __fmul_rn(r11, y)), __fmul_rn(r12, z)), t1);
      const float nz = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(r20, x), __fmul_rn(r21, y)), __fmul_rn(r22, z)), t2);
      x = nx, y = ny, z = nz;
      sx[j] = x, sy[j] = y, sz[j] = z;
    }
    px[p] = x, py[p] = y, pz[p] = z;
    dist[p] = (ok && sdrop[j]) ? 0.f : 1e10f;      // pointnet_util.py:64; a dropped row starts (and stays) at 0
  }

  // start: the first kept row at or after start[m], wrapping round (every wavefront scans alike: 64 rows per step)
  int far = (int)start[m];
  far = far < 0 ? 0 : (far >= U ? U - 1 : far);
  {
    const int s0 = far;
    for (int c = 0; c < U; c += PZN_WAVE) {      // (wavefront-uniform)
      const int off = c + lane;
      int r = s0 + off;
      r = r >= U ? r - U : r;
      r = off < U ? r : 0;
      const bool kept = off < U && sdrop[r] == 0;
      const unsigned long long km = __ballot(kept);
      if (km) {
        int f = s0 + c + (int)__builtin_ctzll(km);
        far = f >= U ? f - U : f;
        break;
      }
    }
    far = __builtin_amdgcn_readfirstlane(far);
  }
  __syncthreads();      // the transformed rows are in the image

  const int pmax = (U + T - 1) / T;
  const bool full = U == T * PPT;      // every thread's every slot holds a row: no bounds tests in the rounds
  int64_t* o = src + (size_t)m * n_out;
  float* oc = out + (size_t)m * n_out * 3;

  auto flush = [&](int base, int cnt) {
    for (int t = tid; t < cnt; t += T) o[base + t] = (int64_t)sout[t];
    for (int e = tid; e < 3 * cnt; e += T) {
      const int t = e / 3, c = e - 3 * t;
      const int r = sout[t];
      oc[(size_t)base * 3 + e] = (c == 0 ? sx : (c == 1 ? sy : sz))[r];
    }
  };

  for (int i = 0; i < n_out; ++i) {
    fps_buffer_pick(sout, i, n_out, far, tid, flush);
    const float cx = sx[far], cy = sy[far], cz = sz[far];
    const uint64_t best = fps_wave_argmax<T, PPT>(px, py, pz, dist, cx, cy, cz, tid, U, pmax, full);
    far = (int)(~(uint32_t)fps_cross_wave<W>(slots, i, lane, wave, best));
  }
}

template <int PPT>
int launch(const float* a, const float* b, const float* pose, const int64_t* start, const int64_t* drop_a, int ka,
           const int64_t* drop_b, int kb, int M, int Na, int Nb, int n_out, float* out, int64_t* src, hipStream_t st) {
  constexpr int W = MRG_T / PZN_WAVE;
  const size_t U = (size_t)Na + Nb;
  const size_t lds = fps_lds_head(W) + 3 * U * sizeof(float) + U;
  PZN_LAUNCH((merge_resample_kernel<MRG_T, PPT>), dim3(M), dim3(MRG_T), lds, st, a, b, pose, start, drop_a, ka, drop_b, kb,
             Na, Nb, n_out, out, src);
  PZN_RETURN_LAUNCH_STATUS();
}

}  // namespace

PZN_EXPORT int pzn_merge_resample_supported(int Na, int Nb, int n_out) {
  if (Na < 1 || Nb < 1) return 0;
  const long long U = (long long)Na + Nb;
  return U <= MRG_MAX_UNION && n_out >= 1 && n_out <= U;
}

PZN_EXPORT int pzn_merge_resample_f32(const float* a, const float* b, const float* T, const int64_t* start,
                                      const int64_t* drop_a, int ka, const int64_t* drop_b, int kb, int M, int Na, int Nb,
                                      int n_out, float* out, int64_t* src, pzn_stream_t stream) {
  PZN_CHECK_ARG(a && b && T && start && out && src && M > 0 && Na > 0 && Nb > 0 && n_out > 0 && ka >= 0 && kb >= 0);
  if (!pzn_merge_resample_supported(Na, Nb, n_out)) return PZN_EUNSUPPORTED;
  hipStream_t st = pzn_hip_stream(stream);
  if (!drop_a || ka == 0) drop_a = nullptr, ka = 0;
  if (!drop_b || kb == 0) drop_b = nullptr, kb = 0;
  const int U = Na + Nb;
  if (U <= 256) return launch<1>(a, b, T, start, drop_a, ka, drop_b, kb, M, Na, Nb, n_out, out, src, st);
  if (U <= 512) return launch<2>(a, b, T, start, drop_a, ka, drop_b, kb, M, Na, Nb, n_out, out, src, st);
  if (U <= 1024) return launch<4>(a, b, T, start, drop_a, ka, drop_b, kb, M, Na, Nb, n_out, out, src, st);
  if (U <= 2048) return launch<8>(a, b, T, start, drop_a, ka, drop_b, kb, M, Na, Nb, n_out, out, src, st);
  return launch<16>(a, b, T, start, drop_a, ka, drop_b, kb, M, Na, Nb, n_out, out, src, st);
}
