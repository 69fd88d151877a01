// Translation unit of weight averaging (kernels_ema.hip.h): the kernel, its launch and the host side of mww_set_weight_ema and
// the "ema_forward" option - when an update is due, and which calls stand on the average.
#define MWW_EMA_TU 1
#define MWW_BLOCK_TU 1   // the non-template kernels of the block-kernel headers belong to mww_lib.hip
#include "engine.hip.h"

#include <algorithm>
#include <cstdint>

namespace mww {

int launch_weight_ema(const EmaArgs& a, hipStream_t stream) {
  if (a.n <= 0) return 0;
  EmaArgs k = a;
  const bool aligned = ((reinterpret_cast<uintptr_t>(a.params) | reinterpret_cast<uintptr_t>(a.ema)) & 15u) == 0;
  k.n4 = aligned ? a.n / 4 : 0;
  const int work = std::max(k.n4, a.n - 4 * k.n4);   // the longer of the two loops
  const int grid = std::min((work + kEmaThreads - 1) / kEmaThreads, 1024);
  hipLaunchKernelGGL(weight_ema_kernel, dim3(grid), dim3(kEmaThreads), 0, stream, k);
  return 0;
}

int ema_due(const mww_ctx* c) {
  if (!c->ema.vec || c->step % c->ema.every != 0) return EMA_NONE;
  return c->ema.updates == 0 ? EMA_COPY : EMA_BLEND;
}

// (under "graphs": one more node of the captured chain)
int enqueue_ema(mww_ctx* c, int mode) {
  if (mode == EMA_NONE) return MWW_OK;
  Launcher lp{c};
  lp.begin("weight_ema");
  launch_weight_ema(EmaArgs{c->params, c->ema.vec, 1.0 - c->ema.decay, (int)c->P, 0, mode == EMA_COPY ? 1 : 0}, c->stream);
  lp.end();
  return MWW_OK;
}

void ema_enqueued(mww_ctx* c, int mode) {
  if (mode == EMA_NONE) return;
  c->ema.updates += 1;
  invalidate_ema_bn(c);
}

bool ema_serves(const mww_ctx* c) { return c->ema.forward && c->ema.vec && c->ema.updates > 0; }
const float* eval_source(const mww_ctx* c) { return ema_serves(c) ? c->ema.vec : c->params; }
EmaSource::EmaSource(mww_ctx* ctx, bool training) : c(ctx) { c->ema.src = !training && ema_serves(c); }
EmaSource::~EmaSource() { c->ema.src = false; }

int set_ema_forward(mww_ctx* c, bool on) {
  if (on && !c->ema.vec) return fail(MWW_ERR_INVALID, "ema_forward needs the weight average: call mww_set_weight_ema first");
  c->ema.forward = on;
  return MWW_OK;
}

void free_weight_ema(mww_ctx* c) {
  free_bn_reestimate(c);
  if (c->ema.vec) (void)hipFree(c->ema.vec);
  c->ema = EmaState();
}

}  // namespace mww

using namespace mww;

extern "C" {

int mww_set_weight_ema(mww_ctx* c, double decay, int64_t every_steps) {
  if (!c) return fail(MWW_ERR_INVALID, "null context");
  // validated before anything changes: a refused call leaves the context as it was
  if (decay != 0.0) {
    if (!(decay > 0.0 && decay < 1.0)) return fail(MWW_ERR_INVALID, "weight_ema: decay must lie in (0, 1), or be 0 to remove the average");
    if (every_steps < 1) return fail(MWW_ERR_INVALID, "weight_ema: every_steps must be at least 1");
  }
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipStreamSynchronize(c->stream));
  drop_graphs(c);   // (a capture holds the average's address, the decay and whether its node copies or blends)
  if (decay == 0.0) {
    free_weight_ema(c);
    return MWW_OK;
  }
  if (!c->ema.vec) MWW_TRY(dev_alloc(&c->ema.vec, (size_t)c->P));
  c->ema.decay = decay;
  c->ema.every = every_steps;
  c->ema.updates = 0;
  invalidate_ema_bn(c);
  return MWW_OK;
}

int mww_get_ema_state(mww_ctx* c, float* h, int64_t n, int64_t* updates) {
  if (!c || !c->ema.vec) return fail(MWW_ERR_INVALID, "no weight average installed: call mww_set_weight_ema first");
  if (n != c->P) return fail(MWW_ERR_INVALID, "weight average size mismatch");
  if (updates) *updates = c->ema.updates;
  return h ? copy_out(c, h, c->ema.vec, (size_t)n * sizeof(float)) : MWW_OK;
}

int mww_set_ema_state(mww_ctx* c, const float* h, int64_t n, int64_t updates) {
  if (!c || !c->ema.vec) return fail(MWW_ERR_INVALID, "no weight average installed: call mww_set_weight_ema first");
  if (!h || n != c->P || updates < 0) return fail(MWW_ERR_INVALID, "weight average size mismatch");
  MWW_TRY(copy_in(c, c->ema.vec, h, (size_t)n * sizeof(float)));
  if ((c->ema.updates == 0) != (updates == 0)) drop_graphs(c);   // (a captured step's node copies or blends)
  c->ema.updates = updates;
  invalidate_ema_bn(c);
  return MWW_OK;
}

}  // extern "C"
