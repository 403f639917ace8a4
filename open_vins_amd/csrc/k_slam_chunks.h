// k_slam_chunks.h — ovgpu_slam_update_chunked (api_slam.inc): the integer and copy kernels that let every chunk of a frame's SLAM update run
// on the stream without a host hand-over in between.  The numerical kernels are the single call's (k_slam_gather, k_system, the Gram /
// Cholesky / tail or the Householder route, k_landmark_update): nothing here computes.
//   k_chunk_offsets   every chunk's meas_offsets, rebased to the chunk's first measurement, written up front (they depend on the batch alone)
//   k_chunk_collect   behind a chunk's update: dx -> its row of dx_seq, the four flag words and the gate-bound counter -> the chunk's slots
//                     (the next chunk's pipeline zeroes the control block)
//   k_chunk_copy      the entry state kept aside / put back (covariance, clones, calibration, intrinsics, landmark values) in one launch
// One thread per element, consecutive lanes on consecutive addresses, no waits: kernel boundaries are the only ordering.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ovg {

// out[first[k] + k + i] = meas_offsets[first[k] + i] - meas_offsets[first[k]],  i = 0 .. first[k + 1] - first[k]   (F + n_chunks entries in all)
__global__ void __launch_bounds__(256) k_chunk_offsets(int n_chunks, int F, const int32_t *__restrict__ first, const int32_t *__restrict__ meas_offsets,
                                                       int32_t *__restrict__ out) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= F + n_chunks) return;
  // the chunk whose table holds entry e: the last k with first[k] + k <= e (the tables' starts are strictly increasing; a binary search, n_chunks is small)
  int lo = 0, hi = n_chunks - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (first[mid] + mid <= e) lo = mid;
    else hi = mid - 1;
  }
  const int f0 = first[lo], i = e - f0 - lo;
  if (f0 < 0 || i < 0 || f0 + i > F) return; // (a table the host did not validate writes nothing)
  out[e] = meas_offsets[f0 + i] - meas_offsets[f0];
}

struct ChunkCollect {
  int N;
  const double *dx;        // [N] the update's correction
  const int32_t *flags;    // [4] sticky error words of the update
  const int32_t *gate;     // [1] features the gate's residual bound accepted
  double *dx_row;          // [N]
  int32_t *flags_out;      // [4]
  int32_t *gate_out;       // [1]
};
__global__ void __launch_bounds__(256) k_chunk_collect(ChunkCollect p) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < p.N) p.dx_row[i] = p.dx[i];
  if (i < 4) p.flags_out[i] = p.flags[i];
  if (i == 4) p.gate_out[0] = p.gate[0];
}

constexpr int CHUNK_COPY_SEGS = 5;
struct ChunkCopy {
  double *dst[CHUNK_COPY_SEGS];
  const double *src[CHUNK_COPY_SEGS];
  uint32_t n[CHUNK_COPY_SEGS]; // doubles
};
__global__ void __launch_bounds__(256) k_chunk_copy(ChunkCopy p) {
  const int sgi = blockIdx.y;
  if (sgi >= CHUNK_COPY_SEGS) return;
  double *__restrict__ d = p.dst[sgi];
  const double *__restrict__ s = p.src[sgi];
  const uint32_t n = p.n[sgi];
  for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) d[i] = s[i];
}

} // namespace ovg
