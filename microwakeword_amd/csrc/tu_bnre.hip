// Translation unit of the BatchNorm re-estimation kernels (kernels_bnre.hip.h) and their launches.  The collect kernel calls
// the summation helpers of the two engines' own folds (reduce_partials_256; gfold_load_sums, block_sum2), so it sees their headers.
#define MWW_BLOCK_TU 1        // the non-template kernels of the block-kernel headers belong to mww_lib.hip,
#define MWW_GRAPH_HOST_TU 1   // those of the graph kernel headers to tu_graph.hip
#define MWW_BNRE_TU 1
#include "kernels_graph.hip.h"   // (includes kernels_fwd.hip.h)
#include "kernels_bnre.hip.h"

namespace mww {

int launch_bnre_collect(const BnreCollectArgs& a, int blocks, hipStream_t stream) {
  if (blocks <= 0 || a.n_rows <= 0) return 0;
  hipLaunchKernelGGL(bnre_collect_kernel, dim3(blocks), dim3(kThreads), 0, stream, a);
  return 0;
}

int launch_bnre_commit(const BnreCommitArgs& a, hipStream_t stream) {
  if (a.n <= 0) return 0;
  hipLaunchKernelGGL(bnre_commit_kernel, dim3((a.n + kThreads - 1) / kThreads), dim3(kThreads), 0, stream, a);
  return 0;
}

}  // namespace mww
