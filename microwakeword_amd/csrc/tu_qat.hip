// Translation unit of the weight fake-quantization kernel (kernels_qat.hip.h) and its launch.
#define MWW_QAT_TU 1
#include "kernels_qat.hip.h"

namespace mww {

int launch_weight_qat(const QatArgs& a, hipStream_t stream) {
  const int grid = a.n_channels + (a.n_copy + kQatThreads - 1) / kQatThreads;
  if (grid <= 0) return 0;
  hipLaunchKernelGGL(weight_qat_kernel, dim3(grid), dim3(kQatThreads), 0, stream, a);
  return 0;
}

}  // namespace mww
