// Sharpness-aware steps and global-norm gradient clipping (mww_set_sharpness_aware, mww_set_grad_clip): the norm of the whole
// flat gradient between the backward pass and Adam, and the three elementwise passes that use it.  sharpness.py states every
// expression once, with NumPy restatements; the device follows them operation for operation (fp contract off).
//
//   grad_sumsq_kernel   S = sum g[i]^2 in float64.  One workgroup of kSumsqLanes threads; lane j adds (double)g[i] * (double)g[i]
//                       for i = j, j + 1024, j + 2048, ... in ascending order, the lanes are folded by thread 0 in lane order:
//                       S = ((s_0 + s_1) + s_2) + ...  No atomics: two calls write the same bytes.  Thread 0 also derives the
//                       scalar the next launch multiplies with, in float64:
//                         kSumsqPerturb  scale = rho / (sqrt(S) + 1e-12)
//                         kSumsqClip     k = c / max(sqrt(S), c)       (exactly 1.0 at or below the threshold, and for a NaN S)
//   sam_perturb_kernel  saved[i] = w[i] (a bit copy), w[i] = w[i] + (float)(scale * (double)g[i])
//   grad_scale_kernel   g[i] = (float)(k * (double)g[i])
// Nothing is screened: a non-finite gradient gives a non-finite S, scale and w'.
//
// The elementwise kernels are grid-stride over 16-byte groups where every vector is 16-byte aligned (n4 = P / 4 groups, else 0),
// the remaining P - 4 n4 elements one per thread, like weight_ema_kernel.  LDS only for the lane fold.
#pragma once
#include <hip/hip_runtime.h>

struct mww_ctx;

namespace mww {

constexpr int kSumsqLanes = 1024;
constexpr int kSumsqAhead = 8;   // elements a lane loads before it adds them
constexpr int kSamThreads = 256;
enum { kSumsqOnly = 0, kSumsqPerturb = 1, kSumsqClip = 2 };

struct SumsqArgs {
  const float* g;      // [n] flat gradient
  int n;
  int mode;            // which scalar thread 0 derives (kSumsqOnly: none)
  double value;        // rho / the clipping threshold c
  double* s_out;       // S
  double* s_out2;      // a second place for S (null: none)
  double* scalar_out;  // scale / k (unused with kSumsqOnly)
};

struct SamPerturbArgs {
  const float* g;        // [n] gradient at w
  float* w;              // [n] master: w -> w'
  float* saved;          // [n] the bit copy of w the step restores from
  const double* scale;   // device scalar of the sumsq launch in front
  int n, n4;
};

struct GradScaleArgs {
  float* g;              // [n] in place
  const double* k;       // device scalar of the sumsq launch in front
  int n, n4;
};

// An applying train step of a context that has either feature takes its gradient with a separate Adam launch; `saved` = the bit
// copy of the master a sharpness-aware step restores from, `scalars` = {S of the first pass's gradient, its perturbation scale,
// S of the gradient Adam consumes, its clipping factor}
struct SharpState {
  double rho = 0.0, clip_norm = 0.0;
  float* saved = nullptr;
  double* scalars = nullptr;
  bool valid = false;   // a step has written scalars (mww_get_grad_norms)
};

// ---- tu_sam.hip (also mww_set_sharpness_aware, mww_set_grad_clip, mww_get_grad_norms)
int launch_grad_sumsq(const SumsqArgs& a, hipStream_t stream);
int launch_sam_perturb(const SamPerturbArgs& a, hipStream_t stream);
int launch_grad_scale(const GradScaleArgs& a, hipStream_t stream);
bool sharp_step(const mww_ctx* c);   // an applying train step is sharp_sequence (a radius or a threshold is installed)
int sharp_sequence(mww_ctx* c, int B, int flags, int ema);
int enqueue_clip(mww_ctx* c);        // mww_apply_gradients: the gradient as it stands in the buffer is clipped, where a threshold is installed
// Both features are single-device: neither stands next to an exchange hook.  `installing` names the feature being installed
// (null: the hook is); MWW_OK where the other side is absent
int single_device_only(const mww_ctx* c, const char* installing);
void free_sharpness(mww_ctx* c);

#ifdef MWW_SAM_TU
__global__ __launch_bounds__(kSumsqLanes) void grad_sumsq_kernel(SumsqArgs a) {
#pragma clang fp contract(off)
  __shared__ double lane[kSumsqLanes];
  const int j = (int)threadIdx.x;
  double s = 0.0;
  // kSumsqAhead loads in flight per thread, added in ascending order; an element past the end enters as + 0.0, which changes
  // no bit of a sum of squares (never - 0.0)
  for (int i = j; i < a.n; i += kSumsqAhead * kSumsqLanes) {
    float v[kSumsqAhead];
#pragma unroll
    for (int u = 0; u < kSumsqAhead; ++u) {
      const int e = i + u * kSumsqLanes;
      v[u] = e < a.n ? a.g[e] : 0.0f;
    }
#pragma unroll
    for (int u = 0; u < kSumsqAhead; ++u) {
      const double d = (double)v[u];
      const double q = d * d;
      s = s + q;
    }
  }
  lane[j] = s;
  __syncthreads();
  if (j != 0) return;
  double S = lane[0];
  for (int l = 1; l < kSumsqLanes; ++l) S = S + lane[l];
  a.s_out[0] = S;
  if (a.s_out2) a.s_out2[0] = S;
  if (a.mode == kSumsqPerturb) {
    const double r = sqrt(S);
    const double d = r + 1e-12;
    a.scalar_out[0] = a.value / d;
  } else if (a.mode == kSumsqClip) {
    const double r = sqrt(S);
    const double d = r > a.value ? r : a.value;
    a.scalar_out[0] = a.value / d;
  }
}

__device__ __forceinline__ float sam_move(float w, float g, double scale) {
#pragma clang fp contract(off)
  const double t = scale * (double)g;
  const float e = (float)t;
  return w + e;
}

__device__ __forceinline__ float grad_scaled(float g, double k) {
#pragma clang fp contract(off)
  const double t = k * (double)g;
  return (float)t;
}

__global__ __launch_bounds__(kSamThreads) void sam_perturb_kernel(SamPerturbArgs a) {
  const int stride = (int)gridDim.x * kSamThreads;
  const int t0 = (int)blockIdx.x * kSamThreads + (int)threadIdx.x;
  const double sc = a.scale[0];
  const float4* __restrict__ g4 = reinterpret_cast<const float4*>(a.g);
  float4* __restrict__ w4 = reinterpret_cast<float4*>(a.w);
  float4* __restrict__ s4 = reinterpret_cast<float4*>(a.saved);
  for (int i = t0; i < a.n4; i += stride) {
    const float4 w = w4[i];
    const float4 g = g4[i];
    s4[i] = w;
    w4[i] = make_float4(sam_move(w.x, g.x, sc), sam_move(w.y, g.y, sc), sam_move(w.z, g.z, sc), sam_move(w.w, g.w, sc));
  }
  for (int i = 4 * a.n4 + t0; i < a.n; i += stride) {
    const float w = a.w[i];
    a.saved[i] = w;
    a.w[i] = sam_move(w, a.g[i], sc);
  }
}

__global__ __launch_bounds__(kSamThreads) void grad_scale_kernel(GradScaleArgs a) {
  const int stride = (int)gridDim.x * kSamThreads;
  const int t0 = (int)blockIdx.x * kSamThreads + (int)threadIdx.x;
  const double k = a.k[0];
  float4* __restrict__ g4 = reinterpret_cast<float4*>(a.g);
  for (int i = t0; i < a.n4; i += stride) {
    const float4 g = g4[i];
    g4[i] = make_float4(grad_scaled(g.x, k), grad_scaled(g.y, k), grad_scaled(g.z, k), grad_scaled(g.w, k));
  }
  for (int i = 4 * a.n4 + t0; i < a.n; i += stride) a.g[i] = grad_scaled(a.g[i], k);
}
#endif

}  // namespace mww
