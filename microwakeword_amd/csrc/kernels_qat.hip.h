// Weight fake-quantization ("weight_qat" option): shadow[P] = the parameter vector with every weight channel snapped to the
// grid the int8 family ships (quantize.weight_params: symmetric, narrow range, one scale per output channel, ties away from
// zero).  The forward / backward kernels read the shadow; Adam keeps updating the fp32 master (straight-through estimator).
//
// One launch.  The host uploads the channel map once (mww_set_weight_qat) in CSR form: channel c owns the parameter indices
// chan_elem[chan_start[c] .. chan_start[c + 1]); copy_elem lists every parameter outside all channels (biases, BN gamma /
// beta, structurally masked MixConv taps).  Workgroup c < n_channels handles channel c: max |w| over the channel (wave
// shuffles, then LDS across the waves - a max of non-negative values, so the order does not show), then
//   scale = amax > 0 ? (float)((double)amax / 127.0) : 1,  q = clamp(round_half_away((double)w / (double)scale), -127, 127),
//   shadow = (float)q * scale                                                   (one fp32 multiply)
// which is weight_params' float64 arithmetic operation for operation.  The maximum is taken over the bit patterns of |w|
// (monotone for non-negative floats, NaN above infinity): a channel whose maximum is not finite is copied through unchanged.
// The workgroups behind the channels copy copy_elem through, one element per thread.
#pragma once
#include <hip/hip_runtime.h>

struct mww_ctx;

namespace mww {

constexpr int kQatThreads = 1024;   // the longest channel (the dense kernel, thousands of elements) is the launch's critical path

struct QatArgs {
  const float* params;     // [P] master
  float* shadow;           // [P]
  const int* chan_start;   // [n_channels + 1]
  const int* chan_elem;    // [chan_start[n_channels]] indices into params
  const int* copy_elem;    // [n_copy] indices into params
  int n_channels, n_copy;
};

// "weight_qat" option: the forward / backward launches read `shadow`, the master fake-quantized per weight channel, refreshed
// at the start of every call that runs a forward; Adam, set / get_params and checkpoints keep the master.
// The map (mww_set_weight_qat) is device-resident: CSR channels + the list of parameters outside every channel.
struct QatState {
  bool enabled = false;
  const float* held = nullptr;   // inside mww_evaluate_windows: the vector the first batch refreshed the shadow from (it cannot
                                 // change between the batches); a refresh from any other source is not skipped
  float* shadow = nullptr;
  int *start = nullptr, *elem = nullptr, *copy = nullptr;
  int channels = 0, n_copy = 0;
};

// ---- tu_qat.hip (also mww_set_weight_qat, mww_get_forward_params)
int launch_weight_qat(const QatArgs& a, hipStream_t stream);
int refresh_shadow(mww_ctx* c);                       // shadow = fake_quant(the vector this call's forward stands on), where it is due
void hold_shadow(mww_ctx* c, const float* source);    // the shadow serves every further call that stands on `source` (null: no longer)
int set_weight_qat_enabled(mww_ctx* c, bool on);      // the "weight_qat" option
void free_weight_qat(mww_ctx* c);

#ifdef MWW_QAT_TU
__global__ __launch_bounds__(kQatThreads) void weight_qat_kernel(QatArgs a) {
  __shared__ unsigned sMax[kQatThreads / 64];
  const int tid = threadIdx.x;
  if ((int)blockIdx.x >= a.n_channels) {
    const int i = ((int)blockIdx.x - a.n_channels) * kQatThreads + tid;
    if (i < a.n_copy) {
      const int e = a.copy_elem[i];
      a.shadow[e] = a.params[e];
    }
    return;
  }
  const int lo = a.chan_start[blockIdx.x], hi = a.chan_start[blockIdx.x + 1];
  // a thread's first element stays in registers across the reduction: only a channel longer than the workgroup is read twice
  const int i0 = lo + tid;
  int e0 = 0;
  float w0 = 0.0f;
  unsigned m = 0u;
  if (i0 < hi) {
    e0 = a.chan_elem[i0];
    w0 = a.params[e0];
    m = __float_as_uint(w0) & 0x7FFFFFFFu;
  }
  for (int i = i0 + kQatThreads; i < hi; i += kQatThreads) m = max(m, __float_as_uint(a.params[a.chan_elem[i]]) & 0x7FFFFFFFu);
  for (int d = 32; d > 0; d >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, d, 64));
  if ((tid & 63) == 0) sMax[tid >> 6] = m;
  __syncthreads();
  m = sMax[0];
  for (int w = 1; w < kQatThreads / 64; ++w) m = max(m, sMax[w]);
  const bool finite = m < 0x7F800000u;
  const float amax = __uint_as_float(m);
  const float scale = amax > 0.0f ? (float)((double)amax / 127.0) : 1.0f;
  auto snap = [&](float w) {
    if (!finite) return w;
    const double x = (double)w / (double)scale;
    double r = floor(fabs(x) + 0.5);   // round_half_away as quantize.py states it
    r = r > 127.0 ? 127.0 : r;
    if (!(r == r)) r = 0.0;            // 0 / 0 (a denormal maximum whose scale rounds to zero)
    const int q = x < 0.0 ? -(int)r : (int)r;
    return (float)q * scale;
  };
  if (i0 < hi) a.shadow[e0] = snap(w0);
  for (int i = i0 + kQatThreads; i < hi; i += kQatThreads) {
    const int e = a.chan_elem[i];
    a.shadow[e] = snap(a.params[e]);
  }
}
#endif

}  // namespace mww
