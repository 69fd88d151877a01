// Translation unit of weight fake-quantization (kernels_qat.hip.h): the kernel, its launch and the host side of the "weight_qat"
// option - the channel map, the shadow and its refresh.
#define MWW_QAT_TU 1
#define MWW_BLOCK_TU 1   // the non-template kernels of the block-kernel headers belong to mww_lib.hip
#include "engine.hip.h"

namespace mww {

int launch_weight_qat(const QatArgs& a, hipStream_t stream) {
  const int grid = a.n_channels + (a.n_copy + kQatThreads - 1) / kQatThreads;
  if (grid <= 0) return 0;
  hipLaunchKernelGGL(weight_qat_kernel, dim3(grid), dim3(kQatThreads), 0, stream, a);
  return 0;
}

// "weight_qat": shadow = fake_quant(master), on the context's stream ahead of the first launch that reads weights (every
// Adam update and every mww_set_params is ordered on that stream too, or joined to it before the call returns).  In a
// non-training call under "ema_forward" the source is the weight average instead: shadow = fake_quant(ema).  A held shadow
// (mww_evaluate_windows) is only as good as its source - the next call that reads another vector refreshes.
int refresh_shadow(mww_ctx* c) {
  const float* src = fwd_source(c);
  const QatState& q = c->qat;
  if (!q.enabled || q.held == src) return MWW_OK;
  Launcher lp{c};
  lp.begin("weight_qat");
  launch_weight_qat(QatArgs{src, q.shadow, q.start, q.elem, q.copy, q.channels, q.n_copy}, c->stream);
  lp.end();
  return MWW_OK;
}

void hold_shadow(mww_ctx* c, const float* source) { c->qat.held = source; }

int set_weight_qat_enabled(mww_ctx* c, bool on) {
  if (on && !c->qat.shadow) return fail(MWW_ERR_INVALID, "weight_qat needs a channel map: call mww_set_weight_qat first");
  if (c->qat.enabled != on) invalidate_ema_bn(c);
  c->qat.enabled = on;
  return MWW_OK;
}

void free_weight_qat(mww_ctx* c) {
  QatState& q = c->qat;
  void* bufs[] = {q.shadow, q.start, q.elem, q.copy};
  for (void* p : bufs) if (p) (void)hipFree(p);
  q = QatState();
}

}  // namespace mww

using namespace mww;

extern "C" {

int mww_set_weight_qat(mww_ctx* c, const int32_t* chan_start, const int32_t* chan_elem, int32_t n_channels, int64_t n_elems) {
  if (!c || n_channels < 0 || n_elems < 0) return fail(MWW_ERR_INVALID, "bad weight_qat map arguments");
  if (n_channels > 0 && (!chan_start || (n_elems > 0 && !chan_elem))) return fail(MWW_ERR_INVALID, "null weight_qat map");
  // validated before anything changes: a refused map leaves the context as it was
  std::vector<int> copy;
  if (n_channels > 0) {
    if (n_elems > c->P) return fail(MWW_ERR_INVALID, "weight_qat map lists more elements than the model has parameters");
    if (chan_start[0] != 0 || chan_start[n_channels] != n_elems) return fail(MWW_ERR_INVALID, "weight_qat map: chan_start must run from 0 to n_elems");
    for (int32_t i = 0; i < n_channels; ++i)
      if (chan_start[i + 1] < chan_start[i]) return fail(MWW_ERR_INVALID, "weight_qat map: chan_start must be ascending");
    std::vector<unsigned char> seen((size_t)c->P, 0);
    for (int64_t i = 0; i < n_elems; ++i) {
      const int32_t e = chan_elem[i];
      if (e < 0 || e >= c->P) return fail(MWW_ERR_INVALID, "weight_qat map: element index outside the parameter vector");
      if (seen[(size_t)e]) return fail(MWW_ERR_INVALID, "weight_qat map: an element appears in two channels");
      seen[(size_t)e] = 1;
    }
    for (int64_t e = 0; e < c->P; ++e)
      if (!seen[(size_t)e]) copy.push_back((int)e);
  }
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipStreamSynchronize(c->stream));
  drop_graphs(c);   // (a capture holds the shadow's and the map's addresses)
  free_weight_qat(c);
  invalidate_ema_bn(c);
  if (n_channels == 0) return MWW_OK;
  QatState& q = c->qat;
  auto install = [&]() -> int {
    MWW_TRY(dev_alloc(&q.shadow, (size_t)c->P));
    MWW_TRY(dev_alloc(&q.start, (size_t)n_channels + 1));
    MWW_TRY(dev_alloc(&q.elem, (size_t)n_elems));
    MWW_TRY(dev_alloc(&q.copy, copy.size()));
    HIPCHK(hipMemcpy(q.start, chan_start, ((size_t)n_channels + 1) * sizeof(int), hipMemcpyHostToDevice));
    if (n_elems) HIPCHK(hipMemcpy(q.elem, chan_elem, (size_t)n_elems * sizeof(int), hipMemcpyHostToDevice));
    if (!copy.empty()) HIPCHK(hipMemcpy(q.copy, copy.data(), copy.size() * sizeof(int), hipMemcpyHostToDevice));
    return MWW_OK;
  };
  const int rc = install();
  if (rc) { free_weight_qat(c); return rc; }   // (no half-installed map behind a device error)
  q.channels = n_channels;
  q.n_copy = (int)copy.size();
  return MWW_OK;
}

int mww_get_forward_params(mww_ctx* c, float* h, int64_t n) {
  if (!c || !h || n != c->P) return fail(MWW_ERR_INVALID, "parameter vector size mismatch");
  HIPCHK(hipSetDevice(c->device));
  EmaSource source(c, false);
  MWW_TRY(refresh_shadow(c));
  HIPCHK(hipGetLastError());
  return copy_out(c, h, fwd_params(c), (size_t)n * sizeof(float));
}

}  // extern "C"
