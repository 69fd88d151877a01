// Translation unit of the gradient-norm, perturbation and gradient-scaling kernels (kernels_sam.hip.h) and their launches.
#define MWW_SAM_TU 1
#include "kernels_sam.hip.h"

#include <algorithm>
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

}  // namespace mww
