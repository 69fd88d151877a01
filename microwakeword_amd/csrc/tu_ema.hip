// Translation unit of the weight-averaging kernel (kernels_ema.hip.h) and its launch.
#define MWW_EMA_TU 1
#include "kernels_ema.hip.h"

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

}  // namespace mww
