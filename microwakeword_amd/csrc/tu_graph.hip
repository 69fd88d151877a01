// Translation unit of the conv/BN graph kernels (see graph_launch.hip.h): every instantiation of kernels_graph.hip.h and
// its non-template kernels.  One unit, not one per family: the compiler's result for a kernel depends on
// which other kernels share its module (profiles/graph_split_kernel_identity.txt), and this set compiles to the device code
// the engine was tuned and measured with.
#define MWW_BLOCK_TU 1
#include "graph_launch.hip.h"

namespace mww {

// ---- forward convolution
int k_launch_gconv(const GLaunch& L, bool ch, int nc, const GConvArgs& a, const GridPick& pk, size_t lds, int shape) {
  if (!ch) {
#define XS(ID, N) if (shape == ID && nc == N) return g_launch(L, &gconv_kernel<N, 0, GSh##ID>, g_lds_fwd_static<GSh##ID, N>(lds, a), pk, a);
    MWW_G_SHAPE_FWD(XS)
#undef XS
  }
#define X(N) if (nc == N) return ch ? g_launch(L, &gconv_chunk_kernel<N, 0>, lds, pk, a) : g_launch(L, &gconv_kernel<N, 0>, lds, pk, a);
  MWW_G_WIDTHS(X)
#undef X
  return kGNoKernel;
}

int k_launch_gconv_xg(const GLaunch& L, int nc, const GConvArgs& a, const XGather& xg, const GridPick& pk, size_t lds, int shape) {
#define XS(ID, N)                                                                                              \
  if (shape == ID && nc == N && a.n_src == 1 && a.Tin <= kGXRows)                                              \
    return g_launch<false, kXMaxSamples>(L, &gconv_xg_kernel<N, GSh##ID>, g_lds_fwd_static<GSh##ID, N>(lds, a) + sizeof(XShared) + 16, pk, a, xg);
  MWW_G_SHAPE_XG(XS)
#undef XS
  return kGNoKernel;
}

int k_launch_gfwd2(const GLaunch& L, int nc, const GConvArgs& a0, const GConvArgs& a1, const GridPick& pk, size_t lds, int shape) {
#define XS(ID, N)                                                                                              \
  if (shape == ID && nc == N)                                                                                  \
    return g_launch<true>(L, &gconv_fwd2_kernel<N, GSh##ID>, std::max(g_lds_fwd_static<GSh##ID, N>(lds, a0), g_lds_fwd_static<GSh##ID, N>(lds, a1)), pk, GConv2Args{{a0, a1}});
  MWW_G_SHAPE_FWD2(XS)
#undef XS
#define X(N) if (nc == N) return g_launch<true>(L, &gconv_fwd2_kernel<N>, lds, pk, GConv2Args{{a0, a1}});
  MWW_G_TWIN_WIDTHS(X)
#undef X
  return kGNoKernel;
}

// ---- weight gradient and data gradient in launches of their own
int k_launch_gwgrad(const GLaunch& L, bool ch, int nc, const GWgradArgs& a, const GridPick& pk, size_t lds, int shape) {
  if (!ch) {
#define XS(ID, N) if (shape == ID && nc == N) return g_launch(L, &gconv_wgrad_kernel<N, GSh##ID>, lds, pk, a);
    MWW_G_SHAPE_WG(XS)
#undef XS
  }
#define X(N) if (nc == N) return ch ? g_launch(L, &gconv_wgrad_chunk_kernel<N>, lds, pk, a) : g_launch(L, &gconv_wgrad_kernel<N>, lds, pk, a);
  MWW_G_WIDTHS(X)
#undef X
  return kGNoKernel;
}

int k_launch_gwgrad_xg(const GLaunch& L, int nc, const GWgradArgs& a, const XGather& xg, const GridPick& pk, size_t lds, int shape) {
#define XS(ID, N)                                                                                              \
  if (shape == ID && nc == N && a.n_src == 1 && a.Tin <= kGXRows) {                                            \
    const size_t narrow = MWW_G_WGRAD_XG_NARROW ? g_up4(a.Tout) * (size_t)(gwg_dp_pitch(N) - (N + 7) / 8 * 8) * sizeof(float) : 0; \
    return g_launch<false, kXMaxSamples>(L, &gconv_wgrad_xg_kernel<N, GSh##ID>, lds - narrow + sizeof(XShared) + 16, pk, a, xg); \
  }
  MWW_G_SHAPE_XG(XS)
#undef XS
  return kGNoKernel;
}

int k_launch_gdgrad(const GLaunch& L, bool ch, int nc, const GConvArgs& a, const GridPick& pk, size_t lds) {
#define X(N) if (nc == N) return ch ? g_launch(L, &gconv_chunk_kernel<N, 1>, lds, pk, a) : g_launch(L, &gconv_kernel<N, 1>, lds, pk, a);
  MWW_G_WIDTHS(X)
#undef X
  return kGNoKernel;
}

// ---- both gradients of an op (of two twin ops) in one launch
int k_launch_gbwd(const GLaunch& L, bool ch, int nco, int nci, const GWgradArgs& w, const GConvArgs& d, const GridPick& pk, size_t lds, int shape) {
  if (!ch) {
#define XS(ID, NCO, NCI) if (shape == ID && nco == NCO && nci == NCI) return g_launch_wd(L, &gconv_bwd_kernel<NCO, NCI, GSh##ID>, lds, pk, w, d);
    MWW_G_SHAPE_BWD(XS)
#undef XS
  }
#define X(NCO, NCI)                                                                                            \
  if (nco == NCO && nci == NCI)                                                                                \
    return ch ? g_launch_wd(L, &gconv_bwd_chunk_kernel<NCO, NCI>, lds, pk, w, d) : g_launch_wd(L, &gconv_bwd_kernel<NCO, NCI>, lds, pk, w, d);
  MWW_G_BWD_PAIRS(X)
#undef X
  return kGNoKernel;
}

int k_launch_gbwd2(const GLaunch& L, int nc, const GWgradArgs& w0, const GConvArgs& d0, const GWgradArgs& w1, const GConvArgs& d1,
                   const GridPick& pk, size_t lds, int shape) {
#define XS(ID, N) if (shape == ID && nc == N) return g_launch_wd<true>(L, &gconv_bwd2_kernel<N, N, GSh##ID>, lds, pk, GBwd2Args{{w0, w1}, {d0, d1}});
  MWW_G_SHAPE_BWD2(XS)
#undef XS
#define X(N) if (nc == N) return g_launch_wd<true>(L, &gconv_bwd2_kernel<N, N>, lds, pk, GBwd2Args{{w0, w1}, {d0, d1}});
  MWW_G_TWIN_WIDTHS(X)
#undef X
  return kGNoKernel;
}

// depthwise ops: forward (mode 0) / data gradient (mode 1), and the weight gradient
int k_launch_gdw(const GLaunch& L, int mode, const GDwArgs& a, const GridPick& pk, size_t lds) {
  return mode == 0 ? g_launch(L, &gdw_kernel<0>, lds, pk, a) : g_launch(L, &gdw_kernel<1>, lds, pk, a);
}
int k_launch_gdw_wgrad(const GLaunch& L, const GDwArgs& a, const GridPick& pk, size_t lds) { return g_launch(L, &gdw_wgrad_kernel, lds, pk, a); }

}  // namespace mww
