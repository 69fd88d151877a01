// Translation unit of sharpness-aware steps and global-norm clipping (kernels_sam.hip.h): the gradient-norm, perturbation and
// gradient-scaling kernels, their launches, and the host side of mww_set_sharpness_aware / mww_set_grad_clip - the step
// sequence of a context that has either (include/mww.h states it).
#define MWW_SAM_TU 1
#define MWW_BLOCK_TU 1   // the non-template kernels of the block-kernel headers belong to mww_lib.hip
#include "engine.hip.h"

#include <algorithm>
#include <cmath>
#include <cstdint>

namespace mww {

namespace {
// workgroups of an elementwise launch over n elements, n4 of them as 16-byte groups: the longer of its two loops
int elementwise_grid(int n, int n4) {
  const int work = std::max(n4, n - 4 * n4);
  return std::max(1, std::min((work + kSamThreads - 1) / kSamThreads, 1024));
}
bool aligned16(const void* a, const void* b = nullptr, const void* c = nullptr) {
  return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c)) & 15u) == 0;
}
}  // namespace

int launch_grad_sumsq(const SumsqArgs& a, hipStream_t stream) {
  hipLaunchKernelGGL(grad_sumsq_kernel, dim3(1), dim3(kSumsqLanes), 0, stream, a);   // (n == 0: S = 0)
  return 0;
}

int launch_sam_perturb(const SamPerturbArgs& a, hipStream_t stream) {
  if (a.n <= 0) return 0;
  SamPerturbArgs k = a;
  k.n4 = aligned16(a.g, a.w, a.saved) ? a.n / 4 : 0;
  hipLaunchKernelGGL(sam_perturb_kernel, dim3(elementwise_grid(k.n, k.n4)), dim3(kSamThreads), 0, stream, k);
  return 0;
}

int launch_grad_scale(const GradScaleArgs& a, hipStream_t stream) {
  if (a.n <= 0) return 0;
  GradScaleArgs k = a;
  k.n4 = aligned16(a.g) ? a.n / 4 : 0;
  hipLaunchKernelGGL(grad_scale_kernel, dim3(elementwise_grid(k.n, k.n4)), dim3(kSamThreads), 0, stream, k);
  return 0;
}

namespace {

enum { NORM_FIRST = 0, NORM_SCALE = 1, NORM_FINAL = 2, NORM_CLIP = 3, NORM_SCALARS = 4 };

// S of the gradient as it stands -> scalars[slot] (and [also], if >= 0), with the scalar of `mode` behind it
int enqueue_grad_sumsq(mww_ctx* c, int slot, int also, int mode, double value) {
  double* const sc = c->sharp.scalars;
  Launcher lp{c};
  lp.begin("grad_sumsq");
  launch_grad_sumsq(SumsqArgs{c->grads, (int)c->P, mode, value, sc + slot, also >= 0 ? sc + also : nullptr, sc + slot + 1}, c->stream);
  lp.end();
  return MWW_OK;
}

// what stands between the gradient Adam is about to consume and Adam: its S (first: this is also the step's first-pass
// gradient) and, with clipping installed, the scaling
int enqueue_final_norm(mww_ctx* c, bool first) {
  const bool clip = c->sharp.clip_norm > 0.0;
  MWW_TRY(enqueue_grad_sumsq(c, NORM_FINAL, first ? NORM_FIRST : -1, clip ? kSumsqClip : kSumsqOnly, c->sharp.clip_norm));
  if (clip) {
    Launcher lp{c};
    lp.begin("grad_clip");
    launch_grad_scale(GradScaleArgs{c->grads, c->sharp.scalars + NORM_CLIP, (int)c->P, 0}, c->stream);
    lp.end();
  }
  c->sharp.valid = true;
  return MWW_OK;
}

// installs (value > 0) or removes (0) one of the two features; the buffers live while either is installed
int set_sharpness(mww_ctx* c, double value, bool sam, const char* what) {
  if (!c) return fail(MWW_ERR_INVALID, "null context");
  // validated before anything changes: a refused call leaves the context as it was
  if (!(value >= 0.0) || std::isinf(value)) return fail(MWW_ERR_INVALID, std::string(what) + " must be a finite number > 0, or 0 to remove it");
  if (value > 0.0) MWW_TRY(single_device_only(c, what));
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipStreamSynchronize(c->stream));
  drop_graphs(c);   // (a step with either feature is not the captured sequence)
  SharpState& s = c->sharp;
  const double rho = sam ? value : s.rho, clip = sam ? s.clip_norm : value;
  if (rho == 0.0 && clip == 0.0) {
    free_sharpness(c);
    return MWW_OK;
  }
  if (!s.scalars) MWW_TRY(dev_alloc(&s.scalars, (size_t)NORM_SCALARS));
  if (rho > 0.0 && !s.saved) MWW_TRY(dev_alloc(&s.saved, (size_t)c->P));
  if (rho == 0.0 && s.saved) {
    (void)hipFree(s.saved);
    s.saved = nullptr;
  }
  s.rho = rho;
  s.clip_norm = clip;
  return MWW_OK;
}

}  // namespace

bool sharp_step(const mww_ctx* c) { return c->sharp.rho > 0.0 || c->sharp.clip_norm > 0.0; }

int single_device_only(const mww_ctx* c, const char* installing) {
  if (installing)
    return c->xch.hook ? fail(MWW_ERR_UNSUPPORTED, std::string(installing) + " is single-device: it cannot be installed next to an exchange hook") : MWW_OK;
  return sharp_step(c) ? fail(MWW_ERR_UNSUPPORTED, "sharpness-aware steps and gradient clipping are single-device: remove them before installing an exchange hook") : MWW_OK;
}

void free_sharpness(mww_ctx* c) {
  if (c->sharp.saved) (void)hipFree(c->sharp.saved);
  if (c->sharp.scalars) (void)hipFree(c->sharp.scalars);
  c->sharp = SharpState();
}

int enqueue_clip(mww_ctx* c) { return c->sharp.clip_norm > 0.0 ? enqueue_final_norm(c, true) : MWW_OK; }

// the applying step of a context with a sharpness-aware radius or a clipping threshold: the gradient is assembled without
// Adam, Adam is a launch of its own
int sharp_sequence(mww_ctx* c, int B, int flags, int ema) {
  const SharpState& s = c->sharp;
  const bool sam = s.rho > 0.0;
  MWW_TRY(refresh_shadow(c));
  MWW_TRY(c->model->enqueue_forward(c, B, true, true, true, !(flags & MWW_STEP_NO_METRICS)));
  MWW_TRY(c->model->enqueue_backward(c, B, false));   // g(w)
  if (sam) {
    MWW_TRY(enqueue_grad_sumsq(c, NORM_FIRST, -1, kSumsqPerturb, s.rho));
    Launcher lp{c};
    lp.begin("sam_perturb");
    launch_sam_perturb(SamPerturbArgs{c->grads, c->params, s.saved, s.scalars + NORM_SCALE, (int)c->P, 0}, c->stream);
    lp.end();
    // the second pass: the same batch (a descriptor-only one is gathered through the same mailbox slot, committed behind this
    // call), the same dropout mask (the step's counter, or the pinned mask), batch statistics of its own that leave the moving
    // statistics alone, no metrics; the accumulator parities flip as in a second gradient-only step
    MWW_TRY(refresh_shadow(c));   // "weight_qat": fake_quant(w')
    MWW_TRY(c->model->enqueue_forward(c, B, true, false, true, false));
    MWW_TRY(c->model->enqueue_backward(c, B, false));   // g(w')
    lp.begin("sam_restore");
    HIPCHK(hipMemcpyAsync(c->params, s.saved, (size_t)c->P * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    lp.end();
  }
  MWW_TRY(enqueue_final_norm(c, !sam));
  MWW_TRY(enqueue_adam(c));
  return enqueue_ema(c, ema);
}

}  // namespace mww

using namespace mww;

extern "C" {

int mww_set_sharpness_aware(mww_ctx* c, double rho) { return set_sharpness(c, rho, true, "sharpness_aware: rho"); }
int mww_set_grad_clip(mww_ctx* c, double global_norm) { return set_sharpness(c, global_norm, false, "grad_clip: global_norm"); }

int mww_get_grad_norms(mww_ctx* c, double* first_sumsq, double* final_sumsq) {
  if (!c) return fail(MWW_ERR_INVALID, "null context");
  if (!c->sharp.valid) return fail(MWW_ERR_STATE, "grad_norms: no sharpness-aware or clipped step has run yet");
  double h[NORM_SCALARS];
  MWW_TRY(copy_out(c, h, c->sharp.scalars, sizeof(h)));
  if (first_sumsq) *first_sumsq = h[NORM_FIRST];
  if (final_sumsq) *final_sumsq = h[NORM_FINAL];
  return MWW_OK;
}

}  // extern "C"
