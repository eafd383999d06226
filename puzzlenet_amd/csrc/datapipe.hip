// datapipe.hip — the cut of the reference's loader (dataset.py:761-775, 1165-1190) as one launch per batch.
//
// `CADDataset.slice` draws a plane (normal = rand(3,1), z = rand(1)/3), splits the raw cloud by the sign of
// points . normal + z and re-draws while a piece holds fewer than N points.  Here the K candidate planes of every sample are
// drawn up front; one workgroup per sample takes the FIRST candidate that leaves >= n_min points on both sides (the
// sequential re-draw's distribution as long as one of the K is valid) and writes both pieces in their original point order
// (a stable partition: the piece's row order decides which point a start index names, dataset.py:1153), padded to `cap`
// rows with copies of the piece's first row (which can never win farthest point sampling), with the piece sizes and the two
// FPS start indices floor(u * size).  The signed distance is evaluated in float64 like numpy does for float32 points times
// float64 draws, every operation individually rounded (no fma): ((x n0 + y n1) + z n2) + offset.
// The kernel is the single-cut body of pzn_cut.h (shared with solidcut.hip) with the plane's side as the predicate; this file
// holds the plane's cut object and the boundary-mask kernel.
//
// Replaces, per batch: one float64 einsum, two stable sorts of [B, M] keys, two gathers, ~25 element-wise launches.
#include "pzn_common.h"

namespace {

#include "pzn_cut.h"

struct CutArgs {
  CutIO io;                // pieces: the up side is distance >= 0
  const double* normals;   // [B, K, 3]
  const double* zs;        // [B, K]
  double* plane;           // [B, 4]: normal, offset of the plane that was taken
};

struct PlaneCut {
  const CutArgs& a;
  __device__ Plane load(int k) const {
    const double* nk = a.normals + ((size_t)blockIdx.x * a.io.K + k) * 3;
    return Plane{nk[0], nk[1], nk[2], a.zs[(size_t)blockIdx.x * a.io.K + k]};
  }
  __device__ bool test(const Plane& p, float x, float y, float z) const { return is_up(x, y, z, p); }
  __device__ void record(int k) const {
    const Plane p = load(k);
    double* out = a.plane + 4 * blockIdx.x;
    out[0] = p.n0, out[1] = p.n1, out[2] = p.n2, out[3] = p.off;
  }
};

__global__ __launch_bounds__(CUT_T) void cut_compact_kernel(CutArgs a) {
  __shared__ int slots[CUT_W];
  __shared__ int wave_base[CUT_W];
  cut_compact_body(a.io, PlaneCut{a}, slots, wave_base);
}

// down_mask / up_mask of dataset.py:1357-1367: 1.0 at the k picked rows of each cloud, 0 elsewhere (one launch for both pieces)
__global__ void pick_mask_kernel(const int64_t* __restrict__ idx, int R, int k, int N, float* __restrict__ mask) {
  const int r = blockIdx.x;
  float* m = mask + (size_t)r * N;
  for (int j = threadIdx.x; j < N; j += blockDim.x) m[j] = 0.f;
  __syncthreads();
  for (int j = threadIdx.x; j < k; j += blockDim.x) {
    const int64_t p = idx[(size_t)r * k + j];
    if (p >= 0 && p < N) m[p] = 1.f;
  }
}

}  // namespace

PZN_EXPORT int pzn_cut_compact_f32(const float* raw, const double* normals, const double* zs, const double* u, int B, int M,
                                   int K, int n_min, int cap, float* pieces, int64_t* counts, int64_t* start, double* plane,
                                   uint8_t* ok, pzn_stream_t stream) {
  PZN_CHECK_ARG(raw && normals && zs && u && pieces && counts && start && plane && ok);
  PZN_CHECK_ARG(B > 0 && M > 0 && K > 0 && cap > 0 && n_min >= 0);
  CutArgs a{{raw, u, B, M, K, n_min, cap, pieces, counts, start, ok}, normals, zs, plane};
  PZN_LAUNCH(cut_compact_kernel, dim3(B), dim3(CUT_T), 0, pzn_hip_stream(stream), a);
  PZN_RETURN_LAUNCH_STATUS();
}

PZN_EXPORT int pzn_pick_mask_f32(const int64_t* idx, int R, int k, int N, float* mask, pzn_stream_t stream) {
  PZN_CHECK_ARG(idx && mask && R > 0 && k > 0 && N > 0);
  PZN_LAUNCH(pick_mask_kernel, dim3(R), dim3(256), 0, pzn_hip_stream(stream), idx, R, k, N, mask);
  PZN_RETURN_LAUNCH_STATUS();
}
