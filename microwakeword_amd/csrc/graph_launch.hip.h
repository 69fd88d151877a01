// Launchers of the conv/BN graph kernels (kernels_graph.hip.h), in the manner of block_launch.hip.h: the kernels are instantiated
// in a translation unit of their own (tu_graph.hip) so that build() compiles them next to the other units and a host-side edit
// does not recompile them.  The tables below are the one place that lists instantiations.
// The occupancy query and the LDS attribute need the kernel's address, so the grid of a launch is chosen here, next to the
// instantiation, from the few values of the context that GLaunch carries.
#pragma once
#include <algorithm>
#include <map>
#include <utility>

#include "kernels_graph.hip.h"

#ifdef MWW_SLIM
#define MWW_G_WIDTHS(X) X(48)
#else
#define MWW_G_WIDTHS(X) X(8) X(10) X(12) X(16) X(20) X(24) X(30) X(32) X(36) X(40) X(48) X(60) X(64)
#endif

// Static shapes (kernels_graph.hip.h GShape): the ops of the reference's default Inception flags (inception.py:146-209:
// 5x1 stem over the 40 spectrogram bins; per block a fused 1x1 head, 5x1 convolutions over channel slices of it and over
// each other, and the 1x1 convolution over the aligned concatenation).  (id, K, sources, C0, LD0, C1, LD1, C2, LD2); dilation
// and stride 1, no residual branches, whole windows.  Any other op takes the run-time kernels.
#ifdef MWW_SLIM
#define MWW_G_SHAPES(X)
#else
#define MWW_G_SHAPES(X)                                                                                                   \
  X(1, 5, 1, 40, 40, 0, 0, 0, 0) X(2, 1, 1, 24, 24, 0, 0, 0, 0) X(3, 5, 1, 10, 30, 0, 0, 0, 0) X(4, 5, 1, 10, 10, 0, 0, 0, 0)    \
  X(5, 1, 3, 10, 30, 10, 10, 10, 10) X(6, 1, 1, 10, 10, 0, 0, 0, 0) X(7, 5, 1, 16, 48, 0, 0, 0, 0) X(8, 5, 1, 16, 16, 0, 0, 0, 0) \
  X(9, 1, 3, 16, 48, 16, 16, 16, 16) X(10, 1, 3, 10, 10, 10, 10, 10, 10) X(11, 1, 3, 16, 16, 16, 16, 16, 16)
#endif
// (shape id, filters) of the forward / weight-gradient instantiations, (id, filters, input channels) of the backward pairs
#ifdef MWW_SLIM
#define MWW_G_SHAPE_FWD(X)
#define MWW_G_SHAPE_FWD2(X)
#define MWW_G_SHAPE_WG(X)
#define MWW_G_SHAPE_XG(X)
#define MWW_G_SHAPE_BWD(X)
#define MWW_G_SHAPE_BWD2(X)
#else
#define MWW_G_SHAPE_FWD(X) X(1, 24) X(2, 30) X(3, 10) X(4, 10) X(5, 10) X(6, 30) X(6, 48) X(7, 16) X(8, 16) X(9, 16) X(10, 10) X(11, 16)
#define MWW_G_SHAPE_FWD2(X) X(3, 10) X(7, 16) X(4, 10) X(8, 16)
#define MWW_G_SHAPE_WG(X) X(1, 24)
#define MWW_G_SHAPE_XG(X) X(1, 24)   // forward + weight gradient with the input gathered from the feature stores (gconv_xg_kernel)
#define MWW_G_SHAPE_BWD(X) X(2, 30, 24) X(3, 10, 10) X(4, 10, 10) X(5, 10, 30) X(6, 30, 10) X(6, 48, 10) X(7, 16, 16) X(8, 16, 16) X(9, 16, 48) X(10, 10, 30) X(11, 16, 48)
#define MWW_G_SHAPE_BWD2(X) X(3, 10) X(7, 16) X(4, 10) X(8, 16)
#endif

// (filters, input channels) pairs with a fused weight-gradient + data-gradient launch; others use two launches
#ifdef MWW_SLIM
#define MWW_G_BWD_PAIRS(X) X(48, 48)
#else
#define MWW_G_BWD_PAIRS(X) X(30, 24) X(10, 10) X(10, 30) X(30, 10) X(48, 10) X(16, 16) X(16, 48) X(24, 16) X(16, 24) X(36, 24) X(12, 36) X(48, 32) X(48, 48) X(64, 32) X(64, 64)
#endif

// widths with a twin launch (two independent ops of one shape in one launch)
#ifdef MWW_SLIM
#define MWW_G_TWIN_WIDTHS(X) X(32)
#else
#define MWW_G_TWIN_WIDTHS(X) X(8) X(10) X(12) X(16) X(20) X(24) X(32)
#endif

namespace mww {

#define X(ID, K, N, C0, L0, C1, L1, C2, L2) typedef GShape<K, N, C0, L0, C1, L1, C2, L2> GSh##ID;
MWW_G_SHAPES(X)
#undef X

// what a launch reads of the context (mww_ctx): the stream, the CU count, "graph_dgrad_share" and the occupancy cache
struct GLaunch {
  hipStream_t stream;
  int n_cu;
  int dgrad_share;
  std::map<std::pair<const void*, size_t>, int>* occ;   // workgroups per CU of (kernel, dynamic LDS)
};

// Workgroups per role of a conv/BN graph launch.  The kernels are latency-bound (one wave per SIMD and workgroup, ~15
// cycles per issued instruction), so a launch wants as many resident workgroups as its own LDS tile and registers let a
// CU hold - and no more: a workgroup that has to wait for a free slot costs more than it brings.  With one grid for the
// whole step (3 workgroups per CU, the best single value) the 48-channel ops, whose tiles fit twice, ran a third of their
// workgroups as a second round, and the 10- and 16-channel ops left half of the CU's wave slots empty.  Same-session
// sweeps of the Inception step (B = 1024, tools/gpu_knobs.sh): one grid of 768 = 0.993 ms; per launch
// n_cu x min(occupancy, cap) with caps forward / backward 4 / 2 = 1.035, 4 / 3 = 0.941, 3 / 4 = 0.96 (cap 3 forward),
// 4 / 4 = 0.884 (default), 8 / 4 = 0.882, 4 / 5 with the 10-channel backward kernels compiled for five waves = 0.881 (not
// kept); rounding a role's workgroups down to the fewest that keep the number of windows per workgroup = 0.981 (the
// workgroups with one window fewer leave the CU early: fewer, evenly loaded ones are slower).
// `fixed` > 0 (no statistics hand-over: the partial statistics rows of a tensor are shared by all its launches; or
// "grid_graph" set by the caller) keeps the given grid.
struct GridPick {
  int fixed;          // workgroups per role, or 0: choose
  int B, roles, cap;  // windows; roles sharing the launch's workgroups; workgroups per CU at most
  int* used;          // out: workgroups per role
};

inline int g_role_grid(const GLaunch& L, const void* func, size_t lds, const GridPick& pk) {
  int grid = pk.fixed;
  if (grid <= 0) {
    const auto key = std::make_pair(func, lds);
    auto it = L.occ->find(key);
    if (it == L.occ->end()) {
      int occ = 0;
      if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, func, kThreads, lds) != hipSuccess || occ < 1) occ = 3;
      it = L.occ->emplace(key, occ).first;
    }
    const int wpc = std::max(1, std::min(it->second, pk.cap));
    grid = std::max(1, std::min(std::min(pk.B, L.n_cu * 4), L.n_cu * wpc / std::max(1, pk.roles)));   // (n_cu * 4 rows of weight-gradient partials)
  }
  if (pk.used) *pk.used = grid;
  return grid;
}

// weight-gradient and data-gradient roles that divide a launch's workgroups (pk.roles > 1) need not take equal halves:
// "graph_dgrad_share" percent of an op's workgroups form the data gradient
inline void g_share_roles(const GLaunch& L, const GridPick& pk, int* nbw, int* nbd) {
  if (pk.roles > 1 && L.dgrad_share != 50) {
    const int pair = *nbw + *nbd;
    *nbd = std::max(1, std::min(pair - 1, (pair * L.dgrad_share + 50) / 100));
    *nbw = std::max(1, pair - *nbd);
  }
  if (pk.used) *pk.used = *nbw;
}

// The two launch forms.  Both return 0, kGNoKernel, or the hipError_t of a refused LDS attribute (gfx950 has 160 KB of LDS
// per CU; tiles above the 64 KB default need the function attribute).
constexpr int kGNoKernel = -1;

// every workgroup plays the same role; TWIN: two ops, 2 x grid workgroups, the kernel takes the grid of one op last.
// MAX_PER_WG > 0: no launch if a workgroup would see more windows than that.
template <bool TWIN = false, int MAX_PER_WG = 0, class K, class... A>
int g_launch(const GLaunch& L, K k, size_t lds, const GridPick& pk, const A&... args) {
  const void* f = reinterpret_cast<const void*>(k);
  if (lds > 64 * 1024) {
    const hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
  }
  const int grid = g_role_grid(L, f, lds, pk);
  if (MAX_PER_WG > 0 && (pk.B + grid - 1) / grid > MAX_PER_WG) return kGNoKernel;
  if constexpr (TWIN) hipLaunchKernelGGL(k, dim3(2 * grid), dim3(kThreads), lds, L.stream, args..., grid);
  else hipLaunchKernelGGL(k, dim3(grid), dim3(kThreads), lds, L.stream, args...);
  return 0;
}

// weight-gradient + data-gradient roles: nbw + nbd workgroups (TWIN: for each of two ops), the kernel takes (nbw, nbd) last
template <bool TWIN = false, class K, class... A>
int g_launch_wd(const GLaunch& L, K k, size_t lds, const GridPick& pk, const A&... args) {
  const void* f = reinterpret_cast<const void*>(k);
  if (lds > 64 * 1024) {
    const hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
  }
  int nbw = g_role_grid(L, f, lds, pk), nbd = nbw;
  g_share_roles(L, pk, &nbw, &nbd);
  hipLaunchKernelGGL(k, dim3((TWIN ? 2 : 1) * (nbw + nbd)), dim3(kThreads), lds, L.stream, args..., nbw, nbd);
  return 0;
}

// Dynamic LDS of the MFMA graph kernels: `tiles` floats of weights and window tiles; gconv_body's publish scratch aliases the
// first 2 * kThreads floats, its MODE 1 keeps the statistics pairs of the second and third source behind the tiles.
inline size_t g_up4(int v) { return (size_t)((v + 3) & ~3); }
inline size_t g_lds_body(size_t tiles, int pairs) { return (std::max(tiles, (size_t)2 * kThreads) + (size_t)pairs * 2 * kThreads + 4) * sizeof(float); }
// dynamic LDS of a static shape's forward launch: the direct form (gconv_body "DIRECT") has no output tile and narrower weight rows
template <class SH, int NC>
size_t g_lds_fwd_static(size_t lds, const GConvArgs& a) {
  if constexpr (g_fwd_direct<SH, 0>()) return g_lds_body((size_t)g_direct_tiles(SH::K, SH::CIN, NC, a.Tin), 0);
  else return lds;
}

// tu_graph.hip.  `ch`: the frame-chunk instantiations (a.S > 1); `shape`: the op's static shape (MWW_G_SHAPES id), or 0.
int k_launch_gconv(const GLaunch& L, bool ch, int nc, const GConvArgs& a, const GridPick& pk, size_t lds, int shape);
// (the stem gathering a descriptor-only batch; kGNoKernel also when the grid would leave a workgroup more than kXMaxSamples windows)
int k_launch_gconv_xg(const GLaunch& L, int nc, const GConvArgs& a, const XGather& xg, const GridPick& pk, size_t lds, int shape);
int k_launch_gfwd2(const GLaunch& L, int nc, const GConvArgs& a0, const GConvArgs& a1, const GridPick& pk, size_t lds, int shape);
// weight gradient and data gradient in launches of their own
int k_launch_gwgrad(const GLaunch& L, bool ch, int nc, const GWgradArgs& a, const GridPick& pk, size_t lds, int shape);
int k_launch_gwgrad_xg(const GLaunch& L, int nc, const GWgradArgs& a, const XGather& xg, const GridPick& pk, size_t lds, int shape);
int k_launch_gdgrad(const GLaunch& L, bool ch, int nc, const GConvArgs& a, const GridPick& pk, size_t lds);
// both gradients of an op (of two twin ops) in one launch
int k_launch_gbwd(const GLaunch& L, bool ch, int nco, int nci, const GWgradArgs& w, const GConvArgs& d, const GridPick& pk, size_t lds, int shape);
int k_launch_gbwd2(const GLaunch& L, int nc, const GWgradArgs& w0, const GConvArgs& d0, const GWgradArgs& w1, const GConvArgs& d1,
                   const GridPick& pk, size_t lds, int shape);
// depthwise ops: forward (mode 0) / data gradient (mode 1), and the weight gradient
int k_launch_gdw(const GLaunch& L, int mode, const GDwArgs& a, const GridPick& pk, size_t lds);
int k_launch_gdw_wgrad(const GLaunch& L, const GDwArgs& a, const GridPick& pk, size_t lds);

}  // namespace mww
