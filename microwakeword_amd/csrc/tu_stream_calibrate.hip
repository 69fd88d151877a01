// The device half of mww_stream_calibrate (include/mww.h; the entry point is in tu_stream.hip next to
// mww_stream_calibrate_host): what the host form does on the host - the scan of the fed frames for the input range and the
// fold of the per-workgroup partial rows the <REC> launch wrote - done where the frames and the rows already are, so that
// n_tensors * 8 bytes cross to the host and nothing goes up.
//
//   calib_input_kernel   walks every virtual frame of the call's tracks (pad rows read 0, a u16 store value is scaled as
//                        frame_value scales it) with a grid-stride loop; a thread keeps the min / max of its elements, the
//                        workgroup folds them in thread order (rec_fold) and writes ONE (min, max) partial.
//   calib_fold_kernel    one workgroup.  Tensor 0: thread j folds the input partials j, j + 256, ... in that order, rec_fold
//                        folds the threads in thread order.  Tensor t >= 1: one thread folds the launch's partial rows in
//                        workgroup order, the order mww_stream_calibrate_host folds them in.
// min / max are exact, so any fixed order gives the host form's value; the order is fixed all the same and no atomic is used:
// two calls write the same bytes.
#include <hip/hip_runtime.h>

#include "stream_common.hip.h"

using namespace mww_stream_impl;

namespace {

constexpr int kCalItems = 4;   // elements a thread of calib_input_kernel takes before the grid is capped at 2 x CU

__global__ void __launch_bounds__(kStreamThreads) calib_input_kernel(SStores S, SCall a, int64_t n_frames, float* part) {
  __shared__ float red[2 * kStreamThreads], rmin[1], rmax[1];
  if (threadIdx.x == 0) {
    rmin[0] = INFINITY;
    rmax[0] = -INFINITY;
  }
  float lmin = INFINITY, lmax = -INFINITY;
  const int64_t n = n_frames * MWW_FEATURE_BINS;
  for (int64_t idx = (int64_t)blockIdx.x * kStreamThreads + threadIdx.x; idx < n; idx += (int64_t)gridDim.x * kStreamThreads) {
    const float x = frame_value(S, a, idx / MWW_FEATURE_BINS, (int)(idx % MWW_FEATURE_BINS));
    lmin = fminf(lmin, x);
    lmax = fmaxf(lmax, x);
  }
  __syncthreads();
  rec_fold(lmin, lmax, 0, red, rmin, rmax);
  if (threadIdx.x == 0) {
    part[2 * blockIdx.x] = rmin[0];
    part[2 * blockIdx.x + 1] = rmax[0];
  }
}

__global__ void __launch_bounds__(kStreamThreads) calib_fold_kernel(const float* in_part, int n_in, const float* rec, int grid, int nt,
                                                                    float* out) {
  __shared__ float red[2 * kStreamThreads], rmin[1], rmax[1];
  const int tid = threadIdx.x;
  if (tid == 0) {
    rmin[0] = INFINITY;
    rmax[0] = -INFINITY;
  }
  float lmin = INFINITY, lmax = -INFINITY;
  for (int g = tid; g < n_in; g += kStreamThreads) {
    lmin = fminf(lmin, in_part[2 * g]);
    lmax = fmaxf(lmax, in_part[2 * g + 1]);
  }
  __syncthreads();
  rec_fold(lmin, lmax, 0, red, rmin, rmax);
  if (tid == 0) {
    out[0] = rmin[0];
    out[1] = rmax[0];
  }
  for (int t = 1 + tid; t < nt; t += kStreamThreads) {
    float lo = INFINITY, hi = -INFINITY;
    for (int g = 0; g < grid; ++g) {   // workgroup order
      lo = fminf(lo, rec[((int64_t)g * nt + t) * 2]);
      hi = fmaxf(hi, rec[((int64_t)g * nt + t) * 2 + 1]);
    }
    out[2 * t] = lo;
    out[2 * t + 1] = hi;
  }
}

}  // namespace

namespace mww_stream_impl {

int calibrate_buffers(mww_stream* s, SCalBuf* b) {
  const int64_t nt = s->model->n_tensors, wg = 2 * (int64_t)s->n_cu;   // a launch has at most 2 x CU workgroups
  const int rc = grow(&s->rec, &s->cap_rec, wg * nt * 2 + wg * 2 + nt * 2);
  if (rc) return rc;
  b->rec = s->rec;
  b->in_part = b->rec + wg * nt * 2;
  b->ranges = b->in_part + wg * 2;
  return MWW_OK;
}

int calibrate_input(mww_stream* s, const SStores& S, const SCall& a, const SCalBuf& b, int64_t n_frames, int* n_in) {
  const int64_t per_wg = (int64_t)kStreamThreads * kCalItems, want = (n_frames * MWW_FEATURE_BINS + per_wg - 1) / per_wg;
  const int grid = (int)(want < 1 ? 1 : want < 2 * (int64_t)s->n_cu ? want : 2 * (int64_t)s->n_cu);
  hipLaunchKernelGGL(calib_input_kernel, dim3(grid), dim3(kStreamThreads), 0, s->stream, S, a, n_frames, b.in_part);
  SCHK(hipGetLastError());
  *n_in = grid;
  return MWW_OK;
}

int calibrate_fold(mww_stream* s, const SCalBuf& b, int n_in, float* ranges) {
  const int nt = s->model->n_tensors;
  hipLaunchKernelGGL(calib_fold_kernel, dim3(1), dim3(kStreamThreads), 0, s->stream, (const float*)b.in_part, n_in,
                     (const float*)b.rec, s->grid, nt, b.ranges);
  SCHK(hipGetLastError());
  SCHK(hipStreamSynchronize(s->stream));
  SCHK(hipMemcpy(ranges, b.ranges, (size_t)nt * 2 * sizeof(float), hipMemcpyDeviceToHost));
  return MWW_OK;
}

}  // namespace mww_stream_impl
