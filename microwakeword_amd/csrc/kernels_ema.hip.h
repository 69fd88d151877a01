// Weight averaging (mww_set_weight_ema): ema[P] = an exponential moving average of the fp32 master, one more parameter-sized
// vector next to params, shadow and the Adam moments.  One elementwise launch directly behind an Adam update:
//   first update:  ema[i] = w[i]                                                  (a bit copy)
//   afterwards:    ema[i] = (float)((double)ema[i] + om * ((double)w[i] - (double)ema[i]))
// with om = 1 - decay formed on the host in double: three float64 operations and one rounding to fp32, which is
// averaging.ema_update operation for operation - so the multiply and the add must stay two operations (fp contract off).
// Nothing is screened: a non-finite master propagates into the average.
//
// Grid-stride over 16-byte groups where both vectors are 16-byte aligned (n4 = P / 4 groups, else 0), the remaining
// P - 4 n4 elements one per thread.  No LDS, no atomics; no element is touched by two threads.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

struct mww_ctx;

namespace mww {

constexpr int kEmaThreads = 256;

struct EmaArgs {
  const float* params;   // [P] master
  float* ema;            // [P]
  double om;             // 1 - decay
  int n, n4;             // P; 16-byte groups taken four at a time (0 when a pointer is not 16-byte aligned)
  int first;             // the first update: copy
};

// weight averaging (mww_set_weight_ema): `vec` follows the master by one launch behind every `every`-th Adam update; with the
// "ema_forward" option a non-training forward reads it (`src`, set for the duration of such a call) once it holds a first update
struct EmaState {
  float* vec = nullptr;
  double decay = 0.0;
  int64_t every = 1, updates = 0;
  bool forward = false, src = false;
};

// ---- tu_ema.hip (also mww_set_weight_ema, mww_get_ema_state, mww_set_ema_state)
int launch_weight_ema(const EmaArgs& a, hipStream_t stream);
// what the Adam update that takes the optimizer to c->step is followed by - nothing, the copy that starts the average, or one
// blend; enqueued on the context's stream directly behind that update; counted once the call that enqueued it cannot fail
enum { EMA_NONE = 0, EMA_COPY = 1, EMA_BLEND = 2 };
int ema_due(const mww_ctx* c);
int enqueue_ema(mww_ctx* c, int mode);
void ema_enqueued(mww_ctx* c, int mode);
// a non-training call under "ema_forward" stands on the weight average once it holds a first update; for this call only
bool ema_serves(const mww_ctx* c);
const float* eval_source(const mww_ctx* c);   // the vector such a call stands on: the average where it serves, else the master
struct EmaSource {
  mww_ctx* c;
  EmaSource(mww_ctx* ctx, bool training);
  ~EmaSource();
};
int set_ema_forward(mww_ctx* c, bool on);     // the "ema_forward" option
void free_weight_ema(mww_ctx* c);             // (with the statistics re-estimated for it)

#ifdef MWW_EMA_TU
__device__ __forceinline__ float ema_blend(float e, float w, double om) {
#pragma clang fp contract(off)
  const double d = (double)w - (double)e;
  const double t = om * d;
  const double s = (double)e + t;
  return (float)s;
}

__global__ __launch_bounds__(kEmaThreads) void weight_ema_kernel(EmaArgs a) {
  const int stride = (int)gridDim.x * kEmaThreads;
  const int t0 = (int)blockIdx.x * kEmaThreads + (int)threadIdx.x;
  const float4* __restrict__ w4 = reinterpret_cast<const float4*>(a.params);
  float4* __restrict__ e4 = reinterpret_cast<float4*>(a.ema);
  for (int i = t0; i < a.n4; i += stride) {
    const float4 w = w4[i];
    if (a.first) {
      e4[i] = w;
    } else {
      const float4 e = e4[i];
      e4[i] = make_float4(ema_blend(e.x, w.x, a.om), ema_blend(e.y, w.y, a.om), ema_blend(e.z, w.z, a.om), ema_blend(e.w, w.w, a.om));
    }
  }
  for (int i = 4 * a.n4 + t0; i < a.n; i += stride) a.ema[i] = a.first ? a.params[i] : ema_blend(a.ema[i], a.params[i], a.om);
}
#endif

}  // namespace mww
