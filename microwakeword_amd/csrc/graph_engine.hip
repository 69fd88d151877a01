// The conv/BN graph engine of libmww_hip.so (Inception, and every MixedNet off the block kernels' shape table): validation and
// planning of a mww_convnet_desc, LDS sizing, and the forward / backward launch sequences.  The convolution kernels are
// instantiated and launched in tu_graph.hip (graph_launch.hip.h); the small non-template kernels are defined there too
// and launched from here.
#define MWW_BLOCK_TU 1        // the non-template kernels of the block-kernel headers belong to mww_lib.hip,
#define MWW_GRAPH_HOST_TU 1   // those of the graph kernel headers to tu_graph.hip
#include <cstring>
#include <map>

#include "engine.hip.h"
#include "graph_launch.hip.h"
#include "kernels_bnre.hip.h"

namespace mww {

static_assert(kGMaxSrc == MWW_MAX_OP_SOURCES, "GOp holds MWW_MAX_OP_SOURCES sources");

namespace {

// gfx950 has 160 KB of LDS per CU; tiles above the 64 KB default need the function attribute
constexpr size_t kMaxDynLds = 144 * 1024;
// planar tensors (GOp::planes) lie kPlanePad floats further apart than their size: without it two planes lie a multiple of 4-8 KB
// apart - max_batch x T x pc x 4 bytes - and twin ops that walk their planes in step hit the same HBM channels: the 16-channel
// twin backward launch went 45 -> 55 us
constexpr long long kPlanePad = 1088;   // 17 x 256 bytes

struct GraphModel : Model {
  std::vector<GOp> G;
  int64_t plan_P = 0, plan_S = 0;   // sizes of the flat vectors behind the ops (the head's parameters follow)
  float dropout = 0.f;
  float* keep = nullptr;            // [max_batch][t_last*c_last] dropout keep-scale
  bool keep_explicit = false;       // set by mww_set_dropout_mask: do not regenerate
  unsigned long long dropout_seed = 0x5EEDull, dropout_counter = 0;
  bool head2 = false;               // attention / pooled head (ghead_att_kernel)
  bool head_att = false;
  int head_pool = 0;
  int64_t o_att = 0;
  float *hact = nullptr, *watt_part = nullptr;
  size_t lds_head2 = 0;
  float *ones = nullptr, *zeros = nullptr;   // [256] constants standing in for the BN arrays of ops without a BN
  int grid_g = 0;
  int g_cap_fwd = 4, g_cap_bwd = 4;   // "graph_fwd_wg_per_cu" / "graph_bwd_wg_per_cu" (g_role_grid)
  bool g_planar = true;   // "graph_planar": tensors read only as equal channel slices are stored one plane per slice
  bool g_static = true;   // "graph_static_shapes": ops whose shape has a compile-time instantiation (MWW_G_SHAPES) use it
  int frame_chunks = 0;   // "graph_frame_chunks" (g_chunks())
  int g_dgrad_share = 50;   // "graph_dgrad_share"
  bool grid_g_auto = true;   // per-launch grids from the kernel's occupancy (g_role_grid); "grid_graph" > 0 fixes one grid
  std::map<std::pair<const void*, size_t>, int> g_occ;   // workgroups per CU of (kernel, dynamic LDS)
  bool g_role_split = true;   // launches that hold several roles (twin ops, weight + data gradient) divide the workgroups between the
                              // roles instead of multiplying them ("graph_role_split"; needs the statistics hand-over: the partial-row
                              // readers assume one row count per tensor)
  bool g_inline_ok = false;   // every op is a convolution with a BatchNorm and no residual branch => hand-over possible
  bool profile_split = false;   // "profile_split" option: keep weight- and data-gradient of an op in separate launches

  ~GraphModel() override {
    for (GOp& o : G) tensor_free(&o);
    void* own[] = {keep, hact, watt_part, ones, zeros};
    for (void* p : own) if (p) (void)hipFree(p);
  }
  int layout(mww_ctx* c) override;
  int alloc(mww_ctx* c, std::vector<BnSlots>* bn) override;
  int enqueue_forward(mww_ctx* c, int B, bool training, bool update_moving, bool loss, bool metrics) override;
  int enqueue_backward(mww_ctx* c, int B, bool fuse_adam) override;
  int enqueue_bn_collect(mww_ctx* c, int B) override;
  std::vector<int> stat_widths() const override {
    std::vector<int> w;
    for (const GOp& o : G) w.push_back(o.cout);
    return w;
  }
  // (the stem's launches check their own grids and write x out themselves if a workgroup would own too many windows)
  bool lazy_ok(const mww_ctx* c, int) const override;
  bool step_counter(unsigned long long* n) override {
    if (!(dropout > 0.f) || keep_explicit) return false;
    *n = dropout_counter++;
    return true;
  }
  // the statistics hand-over instead of finalize launches (kernels_graph.hip.h): the graph and its options allow it / this
  // context runs it (sync-BN has to exchange the sums in between)
  bool handover_possible() const { return g_inline_ok && !profile_split; }
  bool handover(const mww_ctx* c) const { return c->bn_inline && !(c->xch.hook && c->xch.sync_bn) && handover_possible(); }
  unsigned replay_key(bool* handover) const override {
    *handover = handover_possible();
    return (g_role_split ? 1 : 0) | (grid_g_auto ? 2 : 0) | (frame_chunks << 2) | (g_cap_fwd << 5) | (g_cap_bwd << 9) | (g_dgrad_share << 13);
  }
  int debug_tensor(mww_ctx* c, const char* name, int B, DebugTensor* t) override;
  int set_option(mww_ctx* c, const OptionRow& o, int64_t v) override;
  int set_dropout_mask(mww_ctx* c, const uint8_t* keep, int B) override;
};

GraphModel& gm(const mww_ctx* c) { return *static_cast<GraphModel*>(c->model); }

bool g_width_supported(int n) {
#define X(N) if (n == N) return true;
  MWW_G_WIDTHS(X)
#undef X
  return false;
}

// Dynamic LDS of the MFMA graph kernels (kernels_graph.hip.h) for an op whose tiles hold rin input rows / rout output rows
// (forward naming; the whole window, or a frame chunk of a 1x1 op): weights [k][cin4][NCW] zero-padded to whole k-steps /
// filter tiles; gconv_body's publish scratch aliases the first 2 * kThreads floats, its MODE 1 keeps the statistics pairs of
// the second and third source behind the tiles.
size_t g_up16(int v) { return (size_t)((v + 15) / 16 * 16); }
size_t g_lds_fwd(const GOp& o, int rin, int rout) {
  return g_lds_body((size_t)o.k * g_up4(o.cin) * g_up16(o.cout) + (size_t)rin * (o.cin | 1) + (size_t)rout * (o.cout | 1), 0);
}
size_t g_lds_dx(const GOp& o, int rows_dp_padded, int rows_dx) {
  return g_lds_body((size_t)o.k * g_up4(o.cout) * g_up16(o.cin) + (size_t)rows_dp_padded * (o.cout | 1) + (size_t)rows_dx * (o.cin | 1), o.n_src - 1);
}
size_t g_lds_wg(const GOp& o, int rin, int rout) {
  const int tasks = o.k * o.cin, mt = (tasks + 15) / 16, nt = (o.cout + 15) / 16;
  size_t b = (((size_t)rin * (o.cin | 1) + 6) / 4 * 4 + g_up4(rout) * (size_t)gwg_dp_pitch(o.cout)) * sizeof(float);
  if (gwg_kparts(tasks) > 1) b = std::max(b, (size_t)gwg_kparts(tasks) * mt * nt * 256 * sizeof(float));   // scratch of the sum over the frame parts
  return b;
}

// Frame chunks ("graph_frame_chunks"; kernels_graph.hip.h, CH instantiations): S work items of Tc output frames per window -
// the 1x1 ops in all three roles, ops with k > 1 in the forward convolution and in a weight gradient that has no data
// gradient next to it (the stem).  0 = whole windows (the default: the chunked kernels are covered by the parity tests but have not been timed
// on the GPU yet), 1 = as many chunks (<= 4) as it takes for the launch's tiles to fit four times per CU, 2..4 = that many.
// Only with the statistics hand-over (such graphs have no residual branches, which the chunked data gradient does not
// handle) and never for twin launches.
// input frames (with halo) of a chunk of t output frames
int g_chunk_in(const GOp& o, int t) { return (t - 1) * o.stride + (o.k - 1) * o.dil + 1; }

int g_chunks(const mww_ctx* c, const GOp& o, bool inl, bool backward, int* Tc) {
  *Tc = o.tout;
  // the data gradient is only chunked without a halo (k = 1); forward convolution and a weight gradient on its own take any k
  if (!inl || gm(c).frame_chunks == 0 || o.kind != MWW_OP_CONV || o.tout < 32 || (backward && o.needs_dx && o.k != 1)) return 1;
  int S = gm(c).frame_chunks;
  if (S == 1) {
    for (S = 1; S < 4; ++S) {
      const int t = (o.tout + S - 1) / S, ti = g_chunk_in(o, t);
      const size_t lds = backward ? std::max(g_lds_wg(o, ti, t), o.needs_dx ? g_lds_dx(o, t, t) : 0) : g_lds_fwd(o, ti, t);
      if (lds + 3072 <= 40960) break;
    }
  }
  S = std::min(S, 4);
  *Tc = (o.tout + S - 1) / S;
  return (S - 1) * *Tc < o.tout ? S : 1;   // (every chunk non-empty)
}

int g_planes(const mww_ctx* c, const GOp& o) { return (gm(c).g_planar && o.planes > 1) ? o.planes : 1; }
long long g_pstride(const mww_ctx* c, const GOp& o) { return (long long)c->max_batch * o.tout * o.pc + kPlanePad; }

// the static shape of op `o`, or 0
int g_shape_id(const mww_ctx* c, const GOp& o) {
  if (!gm(c).g_static || o.kind != MWW_OP_CONV || o.dil != 1 || o.stride != 1 || o.res_src >= 0 || o.n_src < 1) return 0;
  if (o.tin > kGTmax || o.tout > kGTmax) return 0;   // a window's rows travel in a fixed set of registers (GSliceRegs)
  int C[kGMaxSrc] = {0, 0, 0}, L[kGMaxSrc] = {0, 0, 0};
  for (int i = 0; i < o.n_src; ++i) {
    if (o.src[i] < 0) {
      C[i] = L[i] = MWW_FEATURE_BINS;
    } else {
      const GOp& pr = gm(c).G[o.src[i]];
      if (pr.res_src >= 0) return 0;
      C[i] = o.scn[i];
      L[i] = g_planes(c, pr) > 1 ? o.scn[i] : pr.cout;   // (a plane of a planar producer is a whole tensor of its own)
    }
    const int v = ((C[i] | L[i]) & 3) == 0 ? 4 : (((C[i] | L[i]) & 1) == 0 ? 2 : 1);
    if (o.src[i] >= 0 && L[i] != C[i] && o.sc0[i] % v) return 0;   // the slice must start on the vector width the static staging uses
  }
#define X(ID, K, N, C0, L0, C1, L1, C2, L2)                                                                     \
  if (o.k == K && o.n_src == N && C[0] == C0 && L[0] == L0 && C[1] == C1 && L[1] == L1 && C[2] == C2 && L[2] == L2) return ID;
  MWW_G_SHAPES(X)
#undef X
  return 0;
}

// The stem of a conv/BN graph can read a descriptor-only batch in place ("fused_input", kernels_graph.hip.h XG): exactly one
// op reads the spectrogram, as its only source, and its shape has a gathering instantiation.
bool g_stem_gathers(const mww_ctx* c) {
  if (!c->fused_input || c->frames > kGXRows) return false;
  int readers = 0, stem = -1;
  for (size_t i = 0; i < gm(c).G.size(); ++i)
    for (int s = 0; s < gm(c).G[i].n_src; ++s)
      if (gm(c).G[i].src[s] < 0) {
        ++readers;
        stem = (int)i;
      }
  if (readers != 1) return false;
  const GOp& o = gm(c).G[stem];
  if (o.n_src != 1 || o.toff[0] != 0 || o.tin != c->frames) return false;
  const int shape = g_shape_id(c, o);
#define XS(ID, N) if (shape == ID && o.cout == N) return true;
  MWW_G_SHAPE_XG(XS)
#undef XS
  return false;
}
bool GraphModel::lazy_ok(const mww_ctx* c, int) const { return g_stem_gathers(c); }

bool g_reads_lazy_x(const mww_ctx* c, const GSrc* src, int n) {
  if (!c->x_lazy) return false;
  for (int i = 0; i < n; ++i)
    if (src[i].p == c->x) return true;
  return false;
}

GLaunch g_launch_ctx(mww_ctx* c) { return GLaunch{c->stream, c->n_cu, gm(c).g_dgrad_share, &gm(c).g_occ}; }

// result of a launcher of graph_launch.hip.h -> MWW_* code
int g_rc(int r, const char* no_kernel = "conv width not instantiated") {
  if (r == 0) return MWW_OK;
  if (r == kGNoKernel) return fail(MWW_ERR_UNSUPPORTED, no_kernel);
  return fail(MWW_ERR_HIP, std::string("hipFuncSetAttribute(hipFuncAttributeMaxDynamicSharedMemorySize): ") + hipGetErrorString((hipError_t)r));
}

// forward convolution (ch: the frame-chunk instantiations, a.S > 1)
int launch_gconv(mww_ctx* c, bool ch, int nc, const GConvArgs& a, const GridPick& pk, size_t lds, int shape = 0) {
  if (g_reads_lazy_x(c, a.src, a.n_src)) {
    // descriptor-only batch: the gathering instantiation if there is one and the grid leaves every workgroup at most
    // kXMaxSamples windows; else x is written out first
    const int r = ch ? kGNoKernel : k_launch_gconv_xg(g_launch_ctx(c), nc, a, x_gather(c), pk, lds, shape);
    if (r != kGNoKernel) return g_rc(r);
    int rcx = materialise_x(c);
    if (rcx) return rcx;
  }
  return g_rc(k_launch_gconv(g_launch_ctx(c), ch, nc, a, pk, lds, shape));
}

int launch_gwgrad(mww_ctx* c, bool ch, int nc, const GWgradArgs& a, const GridPick& pk, size_t lds, int shape = 0) {
  if (g_reads_lazy_x(c, a.src, a.n_src)) {   // (as in launch_gconv)
    const int r = ch ? kGNoKernel : k_launch_gwgrad_xg(g_launch_ctx(c), nc, a, x_gather(c), pk, lds, shape);
    if (r != kGNoKernel) return g_rc(r);
    int rcx = materialise_x(c);
    if (rcx) return rcx;
  }
  return g_rc(k_launch_gwgrad(g_launch_ctx(c), ch, nc, a, pk, lds, shape));
}

float* gbn_slot(const GOp& o, int i) { return o.bn + (size_t)i * o.cout; }

// an argument struct with every field 0: the builders below name what their launch reads
template <typename T>
T g_zero() {
  T t;
  memset(&t, 0, sizeof(t));
  return t;
}

// the folded BN of op o as a consumer reads it / the residual branch added before o's activation (a: GSrc, GFoldFwd, GHeadArgs)
template <class A>
void g_bn_arrays(A& a, const GOp& o) {
  a.scale = gbn_slot(o, BN_SCALE); a.shift = gbn_slot(o, BN_SHIFT); a.mean = gbn_slot(o, BN_MEAN); a.rstd = gbn_slot(o, BN_RSTD);
}
template <class A>
void g_residual(A& a, const std::vector<GOp>& G, const GOp& o) {
  if (o.res_src < 0) return;
  const GOp& rr = G[o.res_src];
  a.rp = rr.p; a.rscale = gbn_slot(rr, BN_SCALE); a.rshift = gbn_slot(rr, BN_SHIFT); a.rT = rr.tout; a.rdrop = o.res_drop;
}

// 1 / (the elements behind one statistic of op o - a channel's, or a sub-spectral group's - in a batch of B windows)
float g_inv_n(const GOp& o, int B) { return 1.0f / ((float)B * (float)o.tout * (float)(o.groups > 1 ? o.cout / o.groups : 1)); }

// What the steps of one walk over the ops share.  The argument builders (g_make_*, g_*_args, g_fold_*) read it, the model and
// the context and write nothing: each returns what one role of one launch is handed, whatever was built before it.  The steps
// (g_fwd_*, g_bwd_*) launch; the backward ones list the weight-gradient partial rows they leave behind in `ga`.
struct GWalk {
  mww_ctx* c;
  const GraphModel& m;
  int B;
  bool inl;     // statistics hand-over instead of finalize launches (kernels_graph.hip.h)
  bool pick;    // per-launch grids (g_role_grid)
  bool split;   // a launch that holds several roles divides its workgroups between them
  bool pair;    // twin ops share their launches
  int gg;       // workgroups of a launch whose grid is fixed
  Launcher lp;
  bool training = false, update_moving = false;   // (forward walk)
  int ghead = 0;                                  // (backward walk) workgroups of the head launch
  GradReduceArgs ga;
  GWalk(mww_ctx* c_, const GraphModel& m_, int B_, bool inl_)
      : c(c_), m(m_), B(B_), inl(inl_), pick(inl_ && m_.grid_g_auto), split(inl_ && m_.g_role_split),
        pair(!(c_->xch.hook && c_->xch.sync_bn) && !m_.profile_split), gg(std::min(B_, m_.grid_g)), lp{c_} {
    ga.nseg = 0;
  }
};

// source i of op `oi` as the kernels see it; `backward` adds the gradient routing flags
GSrc g_make_src(const mww_ctx* c, int oi, int i, bool backward, bool inl = false) {
  const GOp& o = gm(c).G[oi];
  GSrc s = g_zero<GSrc>();
  s.toff = o.toff[i];
  if (o.src[i] < 0) {
    s.p = c->x;
    s.T = c->frames;
    s.C = s.ld = s.sld = MWW_FEATURE_BINS;
    s.flags = GSRC_IDENTITY;
    return s;
  }
  const GOp& pr = gm(c).G[o.src[i]];
  s.p = pr.p;
  if (pr.norm == MWW_NORM_BN) {
    g_bn_arrays(s, pr);
  } else {   // a bias (or nothing) instead of a BN: y = p * 1 + bias
    s.scale = gm(c).ones;
    s.shift = pr.norm == MWW_NORM_BIAS ? fwd_params(c) + pr.o_beta : gm(c).zeros;
    s.mean = gm(c).zeros;
    s.rstd = gm(c).ones;
  }
  s.g = pr.g;
  s.gstat_part = pr.gstat_part;
  s.T = pr.tout;
  s.C = o.scn[i];
  s.ld = s.sld = pr.cout;
  s.c0 = s.scb = o.sc0[i];
  if (g_planes(c, pr) > 1) {
    // the producer's tensors are planar and this slice is one of the planes: whole rows of C channels, BN arrays at the plane
    const long long off = (long long)(o.sc0[i] / pr.pc) * g_pstride(c, pr);
    s.p += off;
    s.g += off;
    s.scale += s.c0;
    s.shift += s.c0;
    s.mean += s.c0;
    s.rstd += s.c0;
    s.ld = s.C;
    s.c0 = 0;
  }
  if (pr.act == MWW_ACT_LINEAR) s.flags |= GSRC_LINEAR;
  g_residual(s, gm(c).G, pr);
  if (backward) s.flags |= GSRC_GRAD | (o.src_first[i] ? 0 : GSRC_ACCUM) | (o.src_last[i] ? GSRC_STATS : 0);
  if (backward && inl && o.src_last[i]) s.gacc = bwd_rows(c, pr);   // the slice's backward sums go to the producer's accumulator rows
  return s;
}

GBnBwd g_make_bnbwd(const mww_ctx* c, const GOp& o) {
  GBnBwd y = g_zero<GBnBwd>();
  y.g = o.g;
  y.p = o.p;
  if (o.norm != MWW_NORM_BN) {   // dp = g
    y.mean = gm(c).zeros; y.rstd = gm(c).ones; y.c1 = gm(c).ones; y.mg = gm(c).zeros; y.mgx = gm(c).zeros;
  } else {
    y.mean = gbn_slot(o, BN_MEAN); y.rstd = gbn_slot(o, BN_RSTD); y.c1 = gbn_slot(o, BN_C1); y.mg = gbn_slot(o, BN_MG); y.mgx = gbn_slot(o, BN_MGX);
  }
  y.planes = g_planes(c, o);
  y.pc = o.pc;
  y.pstride = g_pstride(c, o);
  return y;
}

GDwArgs g_make_dw(const mww_ctx* c, int oi, int B, bool backward, bool inl = false) {
  const GOp& o = gm(c).G[oi];
  GDwArgs a = g_zero<GDwArgs>();
  a.src = g_make_src(c, oi, 0, backward, inl);
  a.w = fwd_params(c) + o.o_w;
  a.k = o.k; a.C = o.cout; a.B = B; a.Tin = o.tin; a.Tout = o.tout;
  a.out = o.p;
  a.y = g_make_bnbwd(c, o);
  a.grad_part = o.grad_part;
  return a;
}

// ---- forward roles
// the fold of op pi's forward sums inside a consumer's launch (publish: that consumer also writes the BN arrays out)
GFoldFwd g_fold_fwd(const GWalk& w, int pi, bool publish) {
  const mww_ctx* c = w.c;
  const GOp& pr = w.m.G[pi];
  GFoldFwd f = g_zero<GFoldFwd>();
  f.acc = fwd_rows(c, pr).acc;
  f.C = pr.cout;
  f.groups = pr.groups;
  f.inv_n = g_inv_n(pr, w.B);
  f.publish = publish ? 1 : 0;
  f.update_moving = w.update_moving ? 1 : 0;
  f.gamma = fwd_params(c) + pr.o_gamma; f.beta = fwd_params(c) + pr.o_beta;
  f.moving_mean = c->bn_state + pr.o_mm; f.moving_var = c->bn_state + pr.o_mv;
  g_bn_arrays(f, pr);
  return f;
}

// what the three roles of a convolution share: its sources (grad: with the gradient routing), taps and batch (a: GConvArgs, GWgradArgs)
template <class A>
void g_conv_common(A& a, const GWalk& w, int oi, bool grad) {
  const GOp& q = w.m.G[oi];
  a.n_src = q.n_src;
  for (int s = 0; s < q.n_src; ++s) a.src[s] = g_make_src(w.c, oi, s, grad, w.inl);
  a.k = q.k; a.dil = q.dil; a.B = w.B;
}

int g_leader(const GraphModel& m, int oi) { return (oi > 0 && m.G[oi - 1].twin_next) ? oi - 1 : oi; }   // first op of the launch op oi rides in

GConvArgs g_fwd_args(const GWalk& w, int oi) {
  const mww_ctx* c = w.c;
  const GraphModel& m = w.m;
  const GOp& q = m.G[oi];
  GConvArgs a = g_zero<GConvArgs>();
  g_conv_common(a, w, oi, false);
  a.w = fwd_params(c) + q.o_w;
  a.cin = q.cin; a.stride = q.stride; a.Tin = q.tin; a.Tout = q.tout;
  a.out = q.p; a.out_planes = g_planes(c, q); a.out_pc = q.pc; a.out_pstride = g_pstride(c, q);
  a.stat_part = (w.training && q.norm == MWW_NORM_BN) ? q.stat_part : nullptr;
  if (!w.inl) return a;
  a.sacc = fwd_rows(c, q);
  for (int s = 0; s < q.n_src; ++s) {
    const int pi = q.src[s];
    if (pi < 0 || m.G[pi].norm != MWW_NORM_BN) continue;   // (no statistics to fold)
    const int fc = m.G[pi].first_consumer;
    if (g_leader(m, oi) != g_leader(m, fc)) continue;   // a later launch: the arrays were published by the first one
    bool first_ref = true;
    for (int s2 = 0; s2 < s; ++s2) first_ref = first_ref && q.src[s2] != pi;
    a.fold[s] = g_fold_fwd(w, pi, oi == fc && first_ref);
  }
  return a;
}

GBnEvalArgs g_bn_eval_args(const mww_ctx* c, const GOp& o) {
  return GBnEvalArgs{fwd_params(c) + o.o_gamma, fwd_params(c) + o.o_beta, eval_bn_state(c) + o.o_mm, eval_bn_state(c) + o.o_mv,
                     gbn_slot(o, BN_SCALE), gbn_slot(o, BN_SHIFT), o.cout, o.groups};
}

GBnFwdArgs g_bn_fwd_args(const GWalk& w, const GOp& q, const StatSource& ss) {
  const mww_ctx* c = w.c;
  return GBnFwdArgs{ss.part, ss.G, q.cout, q.groups, ss.inv_n,
                    fwd_params(c) + q.o_gamma, fwd_params(c) + q.o_beta, c->bn_state + q.o_mm, c->bn_state + q.o_mv,
                    gbn_slot(q, BN_SCALE), gbn_slot(q, BN_SHIFT), gbn_slot(q, BN_MEAN), gbn_slot(q, BN_RSTD), w.update_moving ? 1 : 0};
}

// drop: Dropout is active (the train step only: Keras training=True); gen_inline: ghead_kernel draws the mask itself
GHeadArgs g_head_args(const GWalk& w, bool loss, bool metrics, bool drop, bool gen_inline) {
  const mww_ctx* c = w.c;
  const GraphModel& m = w.m;
  const int last = (int)m.G.size() - 1;
  const GOp& lo = m.G[last];
  GHeadArgs h = g_zero<GHeadArgs>();
  h.p = lo.p;
  g_bn_arrays(h, lo);
  h.wd = fwd_params(c) + c->o_dense_w;
  h.bd = fwd_params(c) + c->o_dense_b;
  h.y = (loss || metrics) ? c->y_cur : nullptr;
  h.sw = c->sw_cur;
  h.keep = (drop && !gen_inline) ? m.keep : nullptr;
  if (gen_inline) {
    h.keep_gen = m.keep; h.seed = m.dropout_seed; h.rate = m.dropout;
    h.counter = reinterpret_cast<const unsigned*>(mail_hyper(w.c)) + 2;
  }
  h.z = c->z; h.prob = c->prob; h.dz = c->dz; h.loss_part = c->loss_part;
  h.g = lo.g; h.gstat_part = lo.gstat_part;
  h.B = w.B; h.T = lo.tout; h.C = lo.cout;
  h.inv_b = 1.0f / (float)w.B;
  h.training = (loss ? kHeadTraining : 0) | (c->bce_clipped ? kHeadClippedLoss : 0);
  if (w.inl) {
    h.fold = g_fold_fwd(w, last, true);   // the head is the first (and only) consumer of the last op
    if (loss) h.gacc = bwd_rows(c, lo);
  }
  g_residual(h, m.G, lo);
  return h;
}

GHead2Args g_head2_args(const GWalk& w, const GHeadArgs& h) {
  GHead2Args h2;
  h2.h = h;
  h2.watt = w.m.head_att ? fwd_params(w.c) + w.m.o_att : nullptr;
  h2.pool = w.m.head_pool;
  h2.hact = w.m.hact;
  h2.watt_part = w.m.watt_part;
  return h2;
}

// ---- backward roles
// the fold of op q's backward sums inside its own backward launch (publish: the weight-gradient role writes c1 / mg / mgx /
// dgamma / dbeta out)
GFoldBwd g_fold_bwd(const GWalk& w, const GOp& q, bool publish) {
  const mww_ctx* c = w.c;
  GFoldBwd f = g_zero<GFoldBwd>();
  if (!w.inl || q.norm != MWW_NORM_BN) return f;
  f.acc = bwd_rows(c, q).acc;
  f.groups = q.groups;
  f.inv_n = g_inv_n(q, w.B);
  f.dscale = 1.0f;
  f.publish = publish ? 1 : 0;
  f.gamma = fwd_params(c) + q.o_gamma;
  f.c1 = gbn_slot(q, BN_C1); f.mg = gbn_slot(q, BN_MG); f.mgx = gbn_slot(q, BN_MGX);
  f.dgamma = c->grads + q.o_gamma; f.dbeta = c->grads + q.o_beta;
  return f;
}

GBnBwdArgs g_bn_bwd_args(const mww_ctx* c, const GOp& q, const StatSource& ss) {
  return GBnBwdArgs{ss.part, ss.G, q.cout, q.groups, ss.inv_n,
                    fwd_params(c) + q.o_gamma, gbn_slot(q, BN_RSTD), gbn_slot(q, BN_C1), gbn_slot(q, BN_MG), gbn_slot(q, BN_MGX),
                    c->grads + q.o_gamma, c->grads + q.o_beta, ss.dscale, 0};
}
// d bias = sum of the output gradient = the first statistic the consumers already accumulated
GBnBwdArgs g_bias_grad_args(const mww_ctx* c, const GOp& q, int rows) {
  return GBnBwdArgs{q.gstat_part, rows, q.cout, 1, 0.f, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, c->grads + q.o_beta, 1.0f, 1};
}

GWgradArgs g_wgrad_args(const GWalk& w, int oi) {
  const GOp& q = w.m.G[oi];
  GWgradArgs a = g_zero<GWgradArgs>();
  g_conv_common(a, w, oi, false);
  a.y = g_make_bnbwd(w.c, q);
  a.y.fold = g_fold_bwd(w, q, true);
  a.cin = q.cin; a.stride = q.stride; a.Tin = q.tin; a.Tout = q.tout;
  a.grad_part = q.grad_part;
  return a;
}

GConvArgs g_dgrad_args(const GWalk& w, int oi) {
  const GOp& q = w.m.G[oi];
  GConvArgs a = g_zero<GConvArgs>();
  g_conv_common(a, w, oi, true);
  a.w = fwd_params(w.c) + q.o_w;   // (the data-gradient kernel reads them transposed / tap-reversed in place)
  a.cin = q.cout; a.stride = 1; a.Tin = q.tout; a.Tout = q.tin;
  a.y = g_make_bnbwd(w.c, q);
  a.y.fold = g_fold_bwd(w, q, false);
  return a;
}

// the gradient of a residual op, gathered from the ops that add it
GResGatherArgs g_res_gather_args(const GraphModel& m, const GOp& o, int B) {
  GResGatherArgs ra = g_zero<GResGatherArgs>();
  ra.n = (int)o.adders.size();
  for (int q = 0; q < ra.n; ++q) {
    const GOp& x = m.G[o.adders[q]];
    ra.gx[q] = x.g; ra.Tx[q] = x.tout; ra.drop[q] = x.res_drop;
  }
  ra.p = o.p; ra.mean = gbn_slot(o, BN_MEAN); ra.rstd = gbn_slot(o, BN_RSTD);
  ra.g = o.g; ra.gstat_part = o.gstat_part;
  ra.B = B; ra.T = o.tout; ra.C = o.cout;
  return ra;
}

// `rows` partial rows of the n weights at dst of the flat gradient
void g_add_segment(GradReduceArgs& ga, const float* part, int rows, int n, int64_t dst) {
  ga.seg[ga.nseg++] = GradSegment{part, rows, n, n, (int)dst};
}

// ---- the steps of the forward walk
void g_fwd_bn_eval(GWalk& w, int i, bool bracket) {
  const GBnEvalArgs e = g_bn_eval_args(w.c, w.m.G[i]);
  if (bracket) w.lp.begin("bn_eval_prepare", i);
  hipLaunchKernelGGL(gbn_eval_prepare_kernel, dim3(1), dim3(kThreads), 0, w.c->stream, e);
  if (bracket) w.lp.end();
}

int g_fwd_depthwise(GWalk& w, int i) {
  const GraphModel& m = w.m;
  const GOp& o = m.G[i];
  GDwArgs dw = g_make_dw(w.c, i, w.B, false);
  if (w.inl && o.src[0] >= 0 && m.G[o.src[0]].norm == MWW_NORM_BN && m.G[o.src[0]].first_consumer == i)
    dw.fold = g_fold_fwd(w, o.src[0], true);
  w.lp.begin("dw_fwd", i);
  // (no statistics leave this launch: its grid is free to follow its occupancy even without the hand-over)
  const int rc = g_rc(k_launch_gdw(g_launch_ctx(w.c), 0, dw, GridPick{m.grid_g_auto ? 0 : w.gg, w.B, 1, m.g_cap_fwd, nullptr}, o.lds_fwd));
  w.lp.end();
  return rc;
}

// twins (i, i + 1): one convolution launch and one finalize launch for the pair.  *launched stays false where the width has
// no twin instantiation: no convolution went out and both ops take the single-op route
int g_fwd_twins(GWalk& w, int i, bool* launched) {
  mww_ctx* c = w.c;
  const GraphModel& m = w.m;
  const GOp &o = m.G[i], &o2 = m.G[i + 1];
  if (!w.training) g_fwd_bn_eval(w, i + 1, false);
  const GConvArgs fa0 = g_fwd_args(w, i), fa1 = g_fwd_args(w, i + 1);
  w.lp.begin("conv_fwd2_", i);
  const int r2 = k_launch_gfwd2(g_launch_ctx(c), o.cout, fa0, fa1, GridPick{w.pick ? 0 : (w.split ? std::max(1, w.gg / 2) : w.gg), w.B, w.split ? 2 : 1, m.g_cap_fwd, nullptr},
                                std::max(o.lds_fwd, o2.lds_fwd), g_shape_id(c, o) == g_shape_id(c, o2) ? g_shape_id(c, o) : 0);
  w.lp.end();
  if (r2 == kGNoKernel) {
    w.lp.cancel();
    return MWW_OK;
  }
  if (r2) return g_rc(r2);
  *launched = true;
  if (w.training && !w.inl) {
    const float inv_n = g_inv_n(o, w.B);
    const StatSource s0{o.stat_part, w.gg, inv_n, 1.0f}, s1{o2.stat_part, w.gg, inv_n, 1.0f};
    const GBnFwdArgs f0 = g_bn_fwd_args(w, o, s0), f1 = g_bn_fwd_args(w, o2, s1);
    const int n0 = o.slots;
    w.lp.begin("bn_fwd_finalize2_", i);
    hipLaunchKernelGGL(gbn_fwd_finalize2_kernel, dim3(o.slots + o2.slots), dim3(kThreads), 0, c->stream, f0, f1, n0);
    w.lp.end();
  }
  return MWW_OK;
}

int g_fwd_conv(GWalk& w, int i) {
  mww_ctx* c = w.c;
  const GOp& o = w.m.G[i];
  GConvArgs fa = g_fwd_args(w, i);
  int Tc = 0;
  const int S = g_chunks(c, o, w.inl, false, &Tc);
  const bool ch = S > 1;   // frame chunks: S work items per window, no static shape
  if (ch) { fa.S = S; fa.Tc = Tc; }
  w.lp.begin("conv_fwd", i);
  const int rc = launch_gconv(c, ch, o.cout, fa, GridPick{w.pick ? 0 : w.gg, w.B * S, 1, w.m.g_cap_fwd, nullptr},
                              ch ? g_lds_fwd(o, g_chunk_in(o, Tc), Tc) : o.lds_fwd, ch ? 0 : g_shape_id(c, o));
  w.lp.end();
  return rc;
}

// without the hand-over: the partial rows (behind a sync-BN exchange: the row of global sums) -> the BN arrays of op i
int g_fwd_bn_finalize(GWalk& w, int i) {
  const GOp& o = w.m.G[i];
  StatSource ss;
  MWW_TRY(exchange_stats(w.c, w.lp, "bn_stat_exchange", i, o.stat_part, w.gg, o.cout, 0, g_inv_n(o, w.B), &ss));
  const GBnFwdArgs f = g_bn_fwd_args(w, o, ss);
  w.lp.begin("bn_fwd_finalize", i);
  hipLaunchKernelGGL(gbn_fwd_finalize_kernel, dim3(o.slots), dim3(kThreads), 0, w.c->stream, f);
  w.lp.end();
  return MWW_OK;
}

// the dropout mask where the head does not draw it itself, the head, and what rides behind it
int g_fwd_head(GWalk& w, bool loss, bool metrics) {
  mww_ctx* c = w.c;
  const GraphModel& m = w.m;
  const GOp& lo = m.G.back();
  const bool drop = loss && m.dropout > 0.f;   // Dropout is active in the train step only (Keras training=True)
  const bool gen_inline = drop && !m.keep_explicit && !m.head2;   // ghead_kernel draws the mask itself
  if (drop && !m.keep_explicit && !gen_inline) {
    const long long ne = (long long)w.B * c->t_last * c->c_last;
    DropoutMaskArgs dm{m.keep, ne, m.dropout_seed, reinterpret_cast<const unsigned*>(mail_hyper(c)) + 2, m.dropout};
    w.lp.begin("dropout_mask");
    hipLaunchKernelGGL(dropout_mask_kernel, dim3((unsigned)((ne + kThreads - 1) / kThreads)), dim3(kThreads), 0, c->stream, dm);
    w.lp.end();
  }
  const int ghead = std::min(w.B, c->grid_head);
  const GHeadArgs h = g_head_args(w, loss, metrics, drop, gen_inline);
  // the head's fold was the last reader of this walk's forward rows: the walk's last word on parity (fwd_rows)
  if (w.inl) c->fpar ^= 1;
  if (m.head2) {
    const GHead2Args h2 = g_head2_args(w, h);
    const size_t lds = m.lds_head2;
    if (lds > 64 * 1024)
      HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&ghead_att_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    w.lp.begin("head");
    hipLaunchKernelGGL(ghead_att_kernel, dim3(ghead), dim3(kThreads), lds, c->stream, h2);
    w.lp.end();
    // the dense layer sees hact (already activated): identity "BN" for the dense-weight gradient
    DenseSource ds;
    ds.p = m.hact;
    ds.scale = m.ones;
    ds.shift = m.zeros;
    return enqueue_side_work(c, w.B, metrics, loss, ds);
  }
  w.lp.begin("head");
  hipLaunchKernelGGL(ghead_kernel, dim3(ghead), dim3(kThreads), 0, c->stream, h);
  w.lp.end();
  const DenseSource ds{lo.p, h.scale, h.shift, drop ? m.keep : nullptr, h.rp, h.rscale, h.rshift, h.rT, h.rdrop, 0};
  return enqueue_side_work(c, w.B, metrics, loss, ds);
}

// ---- the steps of the backward walk
// twins (i - 1, i): one finalize launch and one four-role backward launch for the pair
int g_bwd_twins(GWalk& w, int i) {
  mww_ctx* c = w.c;
  const GraphModel& m = w.m;
  const GOp &o = m.G[i], &o1 = m.G[i - 1];
  const float inv_n = g_inv_n(o, w.B);
  const StatSource s0{o.gstat_part, w.gg, inv_n, 1.0f}, s1{o1.gstat_part, w.gg, inv_n, 1.0f};
  const GBnBwdArgs bf0 = g_bn_bwd_args(c, o, s0), bf1 = g_bn_bwd_args(c, o1, s1);
  const GWgradArgs w0 = g_wgrad_args(w, i), w1 = g_wgrad_args(w, i - 1);
  const GConvArgs d0 = g_dgrad_args(w, i), d1 = g_dgrad_args(w, i - 1);
  const int n0 = o.slots, gg4 = w.split ? std::max(1, w.gg / 4) : w.gg;
  w.lp.begin("conv_bwd2_", i);
  if (!w.inl) hipLaunchKernelGGL(gbn_bwd_finalize2_kernel, dim3(o.slots + o1.slots), dim3(kThreads), 0, c->stream, bf0, bf1, n0);
  int rows = gg4;
  const int r2 = k_launch_gbwd2(g_launch_ctx(c), o.cout, w0, d0, w1, d1, GridPick{w.pick ? 0 : gg4, w.B, w.split ? 4 : 1, m.g_cap_bwd, &rows},
                               std::max(std::max(o.lds_wg, o.lds_dx), std::max(o1.lds_wg, o1.lds_dx)),
                               g_shape_id(c, o) == g_shape_id(c, o1) ? g_shape_id(c, o) : 0);
  w.lp.end();
  if (r2) return g_rc(r2, "twin ops without a fused backward instantiation");
  g_add_segment(w.ga, o.grad_part, rows, o.k * o.cin * o.cout, o.o_w);
  g_add_segment(w.ga, o1.grad_part, rows, o1.k * o1.cin * o1.cout, o1.o_w);
  return MWW_OK;
}

void g_bwd_res_gather(GWalk& w, int i) {
  const GResGatherArgs ra = g_res_gather_args(w.m, w.m.G[i], w.B);
  w.lp.begin("residual_gather", i);
  hipLaunchKernelGGL(gres_gather_kernel, dim3(w.gg), dim3(kThreads), 0, w.c->stream, ra);
  w.lp.end();
}

// without the hand-over: op i's backward sums (behind a sync-BN exchange) -> c1 / mg / mgx and the gradients of gamma and beta,
// or of a bias
int g_bwd_finalize(GWalk& w, int i) {
  mww_ctx* c = w.c;
  const GOp& o = w.m.G[i];
  if (o.norm == MWW_NORM_BN) {
    StatSource ss;
    MWW_TRY(exchange_stats(c, w.lp, "bn_gstat_exchange", i, o.gstat_part, i == (int)w.m.G.size() - 1 ? w.ghead : w.gg, o.cout, 1, g_inv_n(o, w.B), &ss));
    const GBnBwdArgs f = g_bn_bwd_args(c, o, ss);
    w.lp.begin("bn_bwd_finalize", i);
    hipLaunchKernelGGL(gbn_bwd_finalize_kernel, dim3(o.slots), dim3(kThreads), 0, c->stream, f);
    w.lp.end();
  } else if (o.norm == MWW_NORM_BIAS) {
    const GBnBwdArgs f = g_bias_grad_args(c, o, w.gg);
    w.lp.begin("bias_grad", i);
    hipLaunchKernelGGL(gbn_bwd_finalize_kernel, dim3(o.cout), dim3(kThreads), 0, c->stream, f);
    w.lp.end();
  }
  return MWW_OK;
}

int g_bwd_depthwise(GWalk& w, int i) {
  mww_ctx* c = w.c;
  const GraphModel& m = w.m;
  const GOp& o = m.G[i];
  GDwArgs dw = g_make_dw(c, i, w.B, true, w.inl);
  if (w.inl && o.norm == MWW_NORM_BIAS) {   // the rows this op's consumer added (sum g, ..) to: folded by the weight-gradient launch
    dw.bias_acc = bwd_rows(c, o).acc;
    dw.dbeta = c->grads + o.o_beta;
  }
  w.lp.begin("dw_wgrad", i);
  int gwg = 0;   // (its partial rows are its own)
  int rc = g_rc(k_launch_gdw_wgrad(g_launch_ctx(c), dw, GridPick{m.grid_g_auto ? 0 : w.gg, w.B, 1, m.g_cap_bwd, &gwg}, o.lds_wg));
  w.lp.end();
  if (rc) return rc;
  if (o.needs_dx) {
    w.lp.begin("dw_dgrad", i);
    // (partial statistics rows are shared without the hand-over)
    rc = g_rc(k_launch_gdw(g_launch_ctx(c), 1, dw, GridPick{w.pick ? 0 : w.gg, w.B, 1, m.g_cap_bwd, nullptr}, o.lds_dx));
    w.lp.end();
    if (rc) return rc;
  }
  g_add_segment(w.ga, o.grad_part, gwg, o.k * o.cout, o.o_w);
  return MWW_OK;
}

// weight and data gradient of op i: one launch with both roles, or - no such instantiation, no data gradient, or
// "profile_split" - a launch each
int g_bwd_conv(GWalk& w, int i) {
  mww_ctx* c = w.c;
  const GraphModel& m = w.m;
  const GOp& o = m.G[i];
  GWgradArgs wa = g_wgrad_args(w, i);
  GConvArgs da = o.needs_dx ? g_dgrad_args(w, i) : g_zero<GConvArgs>();
  int rows = w.gg, Tc = 0;
  const int S = g_chunks(c, o, w.inl, true, &Tc);   // frame chunks (1x1 ops): S work items per window for both roles
  size_t lds_wg = o.lds_wg, lds_dx = o.lds_dx;
  if (S > 1) {
    wa.S = da.S = S;
    wa.Tc = da.Tc = Tc;
    lds_wg = g_lds_wg(o, g_chunk_in(o, Tc), Tc);
    lds_dx = o.needs_dx ? g_lds_dx(o, Tc, Tc) : 0;
  }
  const int items = w.B * S;
  bool fused = false;
  if (o.needs_dx && !m.profile_split) {
    w.lp.begin("conv_bwd", i);
    const GridPick pkf{w.pick ? 0 : (w.split ? std::max(1, w.gg / 2) : w.gg), items, w.split ? 2 : 1, m.g_cap_bwd, &rows};
    const int rf = k_launch_gbwd(g_launch_ctx(c), S > 1, o.cout, o.cin, wa, da, pkf, std::max(lds_wg, lds_dx), g_shape_id(c, o));
    w.lp.end();
    if (rf > 0) return g_rc(rf);
    fused = rf == 0;
    if (!fused) w.lp.cancel();
  }
  if (!fused) {
    w.lp.begin("conv_wgrad", i);
    const GridPick pkw{w.pick ? 0 : w.gg, items, 1, m.g_cap_bwd, &rows};
    int rc = launch_gwgrad(c, S > 1, o.cout, wa, pkw, lds_wg, g_shape_id(c, o));
    w.lp.end();
    if (rc) return rc;
    if (o.needs_dx) {
      w.lp.begin("conv_dgrad", i);
      const GridPick pkd{w.pick ? 0 : w.gg, items, 1, m.g_cap_bwd, nullptr};
      rc = g_rc(k_launch_gdgrad(g_launch_ctx(c), S > 1, o.cin, da, pkd, lds_dx));
      w.lp.end();
      if (rc) return rc;
    }
  }
  g_add_segment(w.ga, o.grad_part, rows, o.k * o.cin * o.cout, o.o_w);
  return MWW_OK;
}

}  // namespace

// The forward plan: per op its eval-mode BN fold, then its launch - a depthwise op's, a twin pair's, or a convolution's with,
// outside the hand-over, its BN finalize - and the head behind the last op.
int GraphModel::enqueue_forward(mww_ctx* c, int B, bool training, bool update_moving, bool loss, bool metrics) {
  if (c->x_lazy && !g_stem_gathers(c)) MWW_TRY(materialise_x(c));   // (an option changed since the batch was assembled)
  GWalk w(c, *this, B, training && handover(c));
  w.training = training;
  w.update_moving = update_moving;
  const int n = (int)G.size();
  for (int i = 0; i < n; ++i) {
    const GOp& o = G[i];
    if (!training && o.norm == MWW_NORM_BN) g_fwd_bn_eval(w, i, true);
    if (o.kind == MWW_OP_DEPTHWISE) {
      MWW_TRY(g_fwd_depthwise(w, i));
      continue;
    }
    if (o.twin_next && w.pair) {
      bool launched = false;
      MWW_TRY(g_fwd_twins(w, i, &launched));
      if (launched) {
        ++i;   // the twin is done
        continue;
      }
    }
    MWW_TRY(g_fwd_conv(w, i));
    if (training && o.norm == MWW_NORM_BN && !w.inl) MWW_TRY(g_fwd_bn_finalize(w, i));
  }
  return g_fwd_head(w, loss, metrics);
}

// BN re-estimation: where the training forward of B windows just enqueued left the sums of every op with a BatchNorm - the
// accumulator rows its first consumer folded (gfold_forward_finish), or the partial rows (behind a sync-BN exchange: the row of
// global sums) gbn_fwd_finalize_body read - with the inv_n of that fold
int GraphModel::enqueue_bn_collect(mww_ctx* c, int B) {
  const bool inl = handover(c);
  const int gg = std::min(B, grid_g);
  std::vector<BnreRow> rows;
  for (size_t i = 0; i < G.size(); ++i) {
    const GOp& o = G[i];
    if (o.norm != MWW_NORM_BN) continue;
    BnreRow r = g_zero<BnreRow>();
    r.C = o.cout;
    r.groups = o.groups;
    r.o_mm = (int)o.o_mm;
    r.o_mv = (int)o.o_mv;
    if (inl) {
      if (o.groups > 1 && o.cout > kGFoldC) return fail(MWW_ERR_UNSUPPORTED, "bn_reestimate: a SubSpectralNormalization wider than a wave");
      r.form = BNRE_ROWS;
      r.acc[0] = o.facc[0];
      r.acc[1] = o.facc[1];
      r.inv_n = g_inv_n(o, B);
    } else {
      const StatSource ss = forward_stat_source(c, (int)i, o.stat_part, gg, o.cout, g_inv_n(o, B));
      r.form = BNRE_PART_GRAPH;
      r.part = ss.part;
      r.G = ss.G;
      r.inv_n = ss.inv_n;
    }
    rows.push_back(r);
  }
  return enqueue_bnre_collect(c, rows);
}

// The backward plan, from the last op down: a twin pair's launch; or the gradient gathered for a residual op, outside the
// hand-over the BN / bias finalize, and the op's own launches.  With the hand-over every op folds the sums its consumers (or
// the head) added to its accumulator rows inside its own launch.
int GraphModel::enqueue_backward(mww_ctx* c, int B, bool fuse_adam) {
  GWalk w(c, *this, B, handover(c));
  w.ghead = std::min(B, c->grid_head);
  for (int i = (int)G.size() - 1; i >= 0; --i) {
    const GOp& o = G[i];
    if (i > 0 && G[i - 1].twin_next && w.pair) {
      MWW_TRY(g_bwd_twins(w, i));
      --i;
      continue;
    }
    if (!o.adders.empty()) g_bwd_res_gather(w, i);
    if (!w.inl) MWW_TRY(g_bwd_finalize(w, i));
    if (o.kind == MWW_OP_DEPTHWISE) MWW_TRY(g_bwd_depthwise(w, i));
    else MWW_TRY(g_bwd_conv(w, i));
  }
  if (head2 && head_att) g_add_segment(w.ga, watt_part, w.ghead, 8, o_att);
  if (w.inl) c->gpar ^= 1;   // behind the last reader of this step's backward rows: the walk's last word on parity (bwd_rows)
  return enqueue_grad_assembly(c, B, w.ga, fuse_adam);
}

namespace {
int plan_ops(const mww_convnet_desc& d, GraphModel* plan) {
  if (d.n_ops < 1 || d.n_ops > MWW_MAX_GRAPH_OPS) return fail(MWW_ERR_INVALID, "n_ops out of range");
  if (d.max_batch <= 0 || d.frames <= 0) return fail(MWW_ERR_INVALID, "frames and max_batch must be positive");
  if (!(d.dropout >= 0.f && d.dropout < 1.f)) return fail(MWW_ERR_INVALID, "dropout rate must be in [0, 1)");
  std::vector<GOp>& ops = plan->G;
  ops.assign(d.n_ops, GOp());
  std::vector<int> n_consumers(d.n_ops, 0);
  int64_t off = 0, soff = 0;
  for (int i = 0; i < d.n_ops; ++i) {
    const mww_conv_bn_op& s = d.ops[i];
    GOp& o = ops[i];
    const std::string tag = "op " + std::to_string(i) + ": ";
    if (s.n_src < 1 || s.n_src > MWW_MAX_OP_SOURCES) return fail(MWW_ERR_INVALID, tag + "1..3 sources");
    if (s.kernel < 1 || s.dilation < 1 || s.filters < 1 || s.bn_groups < 1) return fail(MWW_ERR_INVALID, tag + "bad kernel / dilation / filters / groups");
    if (s.filters % s.bn_groups) return fail(MWW_ERR_INVALID, tag + "filters must be a multiple of the sub-spectral groups");
    if (s.kind != MWW_OP_CONV && s.kind != MWW_OP_DEPTHWISE) return fail(MWW_ERR_INVALID, tag + "unknown op kind");
    if (s.norm < MWW_NORM_BN || s.norm > MWW_NORM_NONE || (s.act != MWW_ACT_RELU && s.act != MWW_ACT_LINEAR)) return fail(MWW_ERR_INVALID, tag + "unknown norm / activation");
    o.res_src = s.residual > 0 ? s.residual - 1 : -1;
    o.res_drop = s.residual_drop;
    o.kind = s.kind;
    o.stride = s.stride > 1 ? s.stride : 1;
    o.norm = s.norm;
    o.act = s.act;
    o.n_src = s.n_src;
    o.k = s.kernel;
    o.dil = s.dilation;
    o.cout = s.filters;
    o.groups = s.bn_groups;
    o.slots = s.norm == MWW_NORM_BN ? (s.bn_groups > 1 ? s.bn_groups : s.filters) : 0;
    o.cin = 0;
    o.tin = -1;
    for (int j = 0; j < s.n_src; ++j) {
      const int src = s.src[j];
      if (src < -1 || src >= i) return fail(MWW_ERR_INVALID, tag + "sources must be earlier ops (or -1 for the spectrogram)");
      for (int j2 = 0; j2 < j; ++j2)
        if (s.src[j2] == src) return fail(MWW_ERR_UNSUPPORTED, tag + "the same source twice");
      if (s.src_drop[j] < 0) return fail(MWW_ERR_INVALID, tag + "negative frame drop");
      const int T = src < 0 ? d.frames : ops[src].tout, Cfull = src < 0 ? MWW_FEATURE_BINS : ops[src].cout;
      const int c0 = s.src_cn[j] > 0 ? s.src_c0[j] : 0, C = s.src_cn[j] > 0 ? s.src_cn[j] : Cfull;
      if (c0 < 0 || c0 + C > Cfull || (src < 0 && C != Cfull)) return fail(MWW_ERR_INVALID, tag + "bad channel slice");
      const int rows = T - s.src_drop[j];
      if (o.tin >= 0 && rows != o.tin) return fail(MWW_ERR_INVALID, tag + "sources are not aligned to the same number of frames");
      o.tin = rows;
      o.cin += C;
      o.src[j] = src;
      o.toff[j] = s.src_drop[j];
      o.sc0[j] = c0;
      o.scn[j] = C;
      if (src >= 0) {
        o.needs_dx = true;
        n_consumers[src]++;
      }
    }
    const int span = o.tin - (o.k - 1) * o.dil;
    if (span <= 0) return fail(MWW_ERR_INVALID, tag + "spectrogram too short for the kernel sizes");
    o.tout = (span - 1) / o.stride + 1;
    if (o.stride > 1 && o.needs_dx) return fail(MWW_ERR_UNSUPPORTED, tag + "a time stride is only implemented for ops fed by the spectrogram");
    const int pad = (o.k - 1) * o.dil;
    if (o.kind == MWW_OP_DEPTHWISE) {
      if (o.n_src != 1 || o.cin != o.cout || o.dil != 1 || o.stride != 1) return fail(MWW_ERR_INVALID, tag + "a depthwise op has one source with as many channels as filters, no dilation, no stride");
      if (o.norm == MWW_NORM_BN) return fail(MWW_ERR_UNSUPPORTED, tag + "depthwise + BatchNorm is not implemented (bias or nothing)");
      if (o.cout > kThreads || o.k * o.cout > kGDwTasks * kThreads) return fail(MWW_ERR_UNSUPPORTED, tag + "depthwise op too large (channels <= 256, taps x channels <= 2048)");
      // tap blocks of 8 with zero weights, kGDwTail zero rows behind every staged window (kernels_graph.hip.h)
      const size_t pi = (size_t)(o.cout | 1), wsz = (size_t)gdw_kpad(o.k) * o.cout;
      o.lds_fwd = (wsz + (size_t)(o.tin + kGDwTail) * pi) * sizeof(float);
      o.lds_dx = o.needs_dx ? (wsz + (size_t)(o.tout + 2 * pad + kGDwTail) * pi) * sizeof(float) : 0;
      o.lds_wg = std::max((size_t)(o.tin + kGDwTail) * pi + (size_t)(o.tout + kGDwJ) * pi, (size_t)2 * kThreads * kGDwJ) * sizeof(float);   // (.. or the scratch of the final sum)
    } else {
      if (!g_width_supported(o.cout)) return fail(MWW_ERR_UNSUPPORTED, tag + "filter count not instantiated (8,10,12,16,20,24,30,32,36,40,48,60,64)");
      if (o.needs_dx && !g_width_supported(o.cin)) return fail(MWW_ERR_UNSUPPORTED, tag + "input channel count not instantiated");
      if (o.k * o.cin > kThreads) return fail(MWW_ERR_UNSUPPORTED, tag + "kernel x input channels exceeds 256");
      o.lds_fwd = g_lds_fwd(o, o.tin, o.tout);   // (g_lds_*: the LDS tiles of the MFMA kernels)
      o.lds_dx = o.needs_dx ? g_lds_dx(o, o.tout + 2 * pad, o.tin) : 0;
      o.lds_wg = g_lds_wg(o, o.tin, o.tout);
    }
    if (std::max(o.lds_fwd, std::max(o.lds_dx, o.lds_wg)) > kMaxDynLds) return fail(MWW_ERR_UNSUPPORTED, tag + "window does not fit the LDS tile");
    o.o_w = off; off += o.kind == MWW_OP_DEPTHWISE ? (int64_t)o.k * o.cout : (int64_t)o.k * o.cin * o.cout;
    if (o.norm == MWW_NORM_BN) {
      o.o_gamma = off; off += o.slots;
      o.o_beta = off; off += o.slots;
      o.o_mm = soff; soff += o.slots;
      o.o_mv = soff; soff += o.slots;
    } else if (o.norm == MWW_NORM_BIAS) {
      o.o_beta = off; off += o.cout;
    }
  }
  for (int i = 0; i < d.n_ops; ++i) {
    GOp& o = ops[i];
    if (o.res_src < 0) continue;
    const std::string tag = "op " + std::to_string(i) + ": ";
    if (o.res_src >= i) return fail(MWW_ERR_INVALID, tag + "the residual op must come earlier");
    GOp& r = ops[o.res_src];
    if (r.kind != MWW_OP_CONV || r.norm != MWW_NORM_BN || r.act != MWW_ACT_LINEAR || o.norm != MWW_NORM_BN)
      return fail(MWW_ERR_UNSUPPORTED, tag + "a residual is a conv + BatchNorm + linear op added to a BatchNorm output");
    if (r.cout != o.cout || o.res_drop < 0 || r.tout - o.res_drop != o.tout) return fail(MWW_ERR_INVALID, tag + "residual shape does not match");
    if (n_consumers[o.res_src] != 0) return fail(MWW_ERR_UNSUPPORTED, tag + "a residual op cannot also be a regular source");
    if ((int)r.adders.size() >= kGMaxAdders) return fail(MWW_ERR_UNSUPPORTED, tag + "too many ops add the same residual");
    r.adders.push_back(i);
    for (int i2 = i + 1; i2 < d.n_ops; ++i2)
      for (int j2 = 0; j2 < ops[i2].n_src; ++j2)
        if (ops[i2].src[j2] == i && ops[i2].scn[j2] != o.cout) return fail(MWW_ERR_UNSUPPORTED, tag + "an op with a residual must be read whole (no channel slice)");
  }
  for (int i = 0; i + 1 < d.n_ops; ++i)
    if (n_consumers[i] == 0 && ops[i].adders.empty()) return fail(MWW_ERR_INVALID, "op " + std::to_string(i) + " has no consumer");
  // twins: consecutive, mutually independent convolutions of one shape (Inception's second-level k x 1 convs of
  // branch 2 and branch 3) share their forward, finalize and backward launches
  auto twin_width = [](int n) {
#define X(N) if (n == N) return true;
    MWW_G_TWIN_WIDTHS(X)
#undef X
    return false;
  };
  for (int i = 0; i + 2 < d.n_ops; ++i) {
    GOp &a = ops[i], &b = ops[i + 1];
    const bool same = a.kind == MWW_OP_CONV && b.kind == MWW_OP_CONV && a.k == b.k && a.dil == b.dil && a.cin == b.cin && a.cout == b.cout &&
                      a.groups == b.groups && a.norm == MWW_NORM_BN && b.norm == MWW_NORM_BN && a.act == b.act && a.stride == 1 &&
                      b.stride == 1 && a.tin == b.tin && a.n_src == 1 && b.n_src == 1 && a.src[0] >= 0 && b.src[0] >= 0 &&
                      b.src[0] != i && a.res_src < 0 && b.res_src < 0 && a.adders.empty() && b.adders.empty() && a.cin == a.cout &&
                      twin_width(a.cout);
    // twins run concurrently inside one launch: they must not route gradient into the same channels of one producer
    // (store vs accumulate would race; e.g. the unfused 1x1 branch heads of an Inception block with sub-spectral groups)
    const bool shared = a.src[0] == b.src[0] && a.sc0[0] < b.sc0[0] + b.cin && b.sc0[0] < a.sc0[0] + a.cin;
    if (same && !shared && (i == 0 || !ops[i - 1].twin_next)) a.twin_next = true;
  }
  // gradient routing: per producer, the slices its consumers read must be identical or disjoint and cover
  // every channel; in the backward pass (descending op index) the first consumer of a slice stores, later
  // ones accumulate and the last one also emits the BN statistics partials of that slice
  for (int pi = 0; pi + 1 < d.n_ops; ++pi) {
    if (!ops[pi].adders.empty()) continue;   // residual ops: gradient gathered from their adders
    std::vector<int> covered(ops[pi].cout, 0);
    for (int i = d.n_ops - 1; i > pi; --i)
      for (int j = 0; j < ops[i].n_src; ++j) {
        if (ops[i].src[j] != pi) continue;
        const int c0 = ops[i].sc0[j], cn = ops[i].scn[j];
        bool first = true, last = true;
        for (int i2 = pi + 1; i2 < d.n_ops; ++i2)
          for (int j2 = 0; j2 < ops[i2].n_src; ++j2) {
            if (ops[i2].src[j2] != pi || (i2 == i && j2 == j)) continue;
            const int d0 = ops[i2].sc0[j2], dn = ops[i2].scn[j2];
            if (d0 + dn <= c0 || c0 + cn <= d0) continue;   // disjoint
            if (d0 != c0 || dn != cn) return fail(MWW_ERR_UNSUPPORTED, "op " + std::to_string(pi) + ": consumers read overlapping, unequal channel slices");
            if (i2 > i) first = false;
            if (i2 < i) last = false;
          }
        ops[i].src_first[j] = first;
        ops[i].src_last[j] = last;
        for (int cc = c0; cc < c0 + cn; ++cc) covered[cc] = 1;
      }
    for (int cc = 0; cc < ops[pi].cout; ++cc)
      if (!covered[cc]) return fail(MWW_ERR_UNSUPPORTED, "op " + std::to_string(pi) + ": channel " + std::to_string(cc) + " has no consumer");
  }
  // planar tensors: a convolution + BatchNorm op whose consumers are all convolutions that read one of `planes` equal slices
  // each (the fused 1x1 branch heads of an Inception block: 30 = 3 x 10, 48 = 3 x 16 channels).  Only for the widths whose
  // own backward staging is the direct one (kernels_graph.hip.h GDpPipe is not planar-aware: 30 and 48 exceed its registers).
  for (int pi = 0; pi + 1 < d.n_ops; ++pi) {
    GOp& pr = ops[pi];
    if (pr.kind != MWW_OP_CONV || pr.norm != MWW_NORM_BN || pr.res_src >= 0 || !pr.adders.empty() || (pr.cout != 30 && pr.cout != 48)) continue;
    int cn = 0;
    bool ok = true;
    for (int i = pi + 1; i < d.n_ops && ok; ++i)
      for (int j = 0; j < ops[i].n_src; ++j) {
        if (ops[i].src[j] != pi) continue;
        if (ops[i].kind != MWW_OP_CONV || ops[i].res_src >= 0 || ops[i].stride != 1) ok = false;
        if (cn == 0) cn = ops[i].scn[j];
        if (ops[i].scn[j] != cn || ops[i].scn[j] >= pr.cout || ops[i].sc0[j] % cn) ok = false;
      }
    if (ok && cn > 0 && pr.cout % cn == 0 && (cn % 2) == 0) {
      pr.planes = pr.cout / cn;
      pr.pc = cn;
    }
  }
  if (n_consumers[d.n_ops - 1] != 0) return fail(MWW_ERR_INVALID, "the last op feeds the classifier head and cannot have other consumers");
  {
    const GOp& lo = ops[d.n_ops - 1];
    if (lo.kind != MWW_OP_CONV || lo.norm != MWW_NORM_BN || lo.act != MWW_ACT_RELU)
      return fail(MWW_ERR_UNSUPPORTED, "the classifier head expects a convolution + BatchNorm + ReLU as the last op");
  }
  // frame chunks ("graph_frame_chunks"): automatic for graphs with depthwise ops, i.e. MixedNet flag sets on this engine - their
  // wide 1x1 ops hold 45-105 KB of LDS per whole-window workgroup; measured on the default MixedNet forced onto this engine
  // 0.877 -> 0.815 ms/step (3: 0.818).  Off for pure convolution graphs: Inception 0.892 / 0.897 / 0.957 / 0.960 ms for 0 / 1 / 2 / 3
  // (profiles/round3_frame_chunks.txt)
  for (const GOp& o : ops)
    if (o.kind == MWW_OP_DEPTHWISE) plan->frame_chunks = 1;
  {
    // statistics hand-over: possible when every op is a convolution followed by a BatchNorm / SSN (or by nothing: a
    // MixedNet's first convolution) or a depthwise op with a bias (or nothing), none has a residual branch and every folded
    // tensor fits the kernels' fold table; first_consumer = the op whose launch folds
    bool ok = true;
    for (int i = 0; i < d.n_ops; ++i) {
      GOp& o = ops[i];
      const bool conv_ok = o.kind == MWW_OP_CONV && (o.norm == MWW_NORM_BN || o.norm == MWW_NORM_NONE);
      const bool dw_ok = o.kind == MWW_OP_DEPTHWISE && (o.norm == MWW_NORM_BIAS || o.norm == MWW_NORM_NONE);
      if (!(conv_ok || dw_ok) || o.res_src >= 0 || !o.adders.empty() || o.cout > kGFoldC) ok = false;
      for (int j = 0; j < o.n_src; ++j)
        if (o.src[j] >= 0 && ops[o.src[j]].first_consumer < 0) ops[o.src[j]].first_consumer = i;
    }
    plan->g_inline_ok = ok && !d.head_attention && !d.head_pool;
  }
  plan->plan_P = off;
  plan->plan_S = soff;
  plan->dropout = d.dropout;
  plan->head_att = d.head_attention != 0;   // (whether the model gets that head: layout)
  plan->head_pool = d.head_pool;
  return MWW_OK;
}
}  // namespace

int plan_convnet(const mww_convnet_desc& d, Model** out) {
  GraphModel* m = new GraphModel();
  const int rc = plan_ops(d, m);
  if (rc) delete m;
  else *out = m;
  return rc;
}

// the head and the dense layer behind the ops
int GraphModel::layout(mww_ctx* c) {
  int64_t off = plan_P;
  GOp& lo = G.back();
  c->t_last = lo.tout;
  c->c_last = lo.cout;
  const bool want_att = head_att;
  const int want_pool = head_pool;
  head_att = false;
  head_pool = 0;
  if (lo.tout > 1 && (want_att || want_pool)) {   // mixednet.py:362: only if more than one frame remains
    if (want_pool < 0 || want_pool > 2) return fail(MWW_ERR_INVALID, "head_pool must be 0, 1 or 2");
    if (want_att && lo.tout < 4) return fail(MWW_ERR_INVALID, "spatial attention needs at least 4 frames");
    if (dropout > 0.f) return fail(MWW_ERR_UNSUPPORTED, "dropout with the attention / pooled head");
    head2 = true;
    head_att = want_att;
    head_pool = want_pool;
    const int to = lo.tout - (head_att ? 3 : 0);
    c->t_last = head_pool ? 1 : to;
    if (head_att) { o_att = off; off += 8; }
    lds_head2 = ((size_t)lo.tout * (lo.cout | 1) + 7 * (size_t)lo.tout + 3 * (size_t)lo.cout) * sizeof(float);
    if (lds_head2 > kMaxDynLds) return fail(MWW_ERR_UNSUPPORTED, "window does not fit the head's LDS tile");
  }
  c->o_dense_w = off; off += (int64_t)c->t_last * lo.cout;
  c->o_dense_b = off; off += 1;
  c->P = off;
  c->S = plan_S;
  c->dwd_stride = c->t_last * lo.cout + 4;
  grid_g = c->n_cu * 3;   // measured on the Inception step: 3 workgroups per CU and launch (roles share them) beats 2 and 4
  return MWW_OK;
}

int GraphModel::alloc(mww_ctx* c, std::vector<BnSlots>* bn) {
  const size_t mb = (size_t)c->max_batch;
  const size_t gmax = (size_t)c->n_cu * 4;   // ("grid_graph" may be raised to it)
  GOp& lo = G.back();
  MWW_TRY(dev_alloc(&keep, mb * lo.tout * lo.cout));
  if (head2) {
    MWW_TRY(dev_alloc(&hact, mb * c->t_last * lo.cout));
    MWW_TRY(dev_alloc(&watt_part, gmax * 8));
  }
  for (GOp& o : G) {
    MWW_TRY(dev_alloc(&o.p, mb * o.tout * o.cout + (size_t)o.planes * kPlanePad));
    MWW_TRY(dev_alloc(&o.g, mb * o.tout * o.cout + (size_t)o.planes * kPlanePad));
    MWW_TRY(tensor_alloc(&o, o.cout, gmax, gmax, gmax * o.k * (o.kind == MWW_OP_DEPTHWISE ? 1 : o.cin) * o.cout));
    if (o.norm == MWW_NORM_BN) bn->push_back(BnSlots{o.o_gamma, o.o_beta, o.o_mv, o.slots});
    else if (o.norm == MWW_NORM_BIAS) bn->push_back(BnSlots{o.o_beta, o.o_beta, -1, o.cout});   // bias gradient is written directly too
  }
  MWW_TRY(dev_alloc(&ones, (size_t)kThreads));
  MWW_TRY(dev_alloc(&zeros, (size_t)kThreads));
  const std::vector<float> one((size_t)kThreads, 1.0f);
  HIPCHK(hipMemcpy(ones, one.data(), one.size() * sizeof(float), hipMemcpyHostToDevice));
  return MWW_OK;
}

int GraphModel::set_option(mww_ctx* c, const OptionRow& o, int64_t v) {
  const std::string name = o.name;
  if (o.owner != OPT_GRAPH) return (v && (name == "pointwise_bf16" || name == "storage_bf16")) ? fail(MWW_ERR_UNSUPPORTED, "the conv/BN graph kernels have no bf16 mode") : MWW_OK;
  const std::pair<const char*, bool GraphModel::*> flags[] = {{"graph_role_split", &GraphModel::g_role_split}, {"graph_static_shapes", &GraphModel::g_static},
                                                              {"graph_planar", &GraphModel::g_planar}, {"profile_split", &GraphModel::profile_split}};
  const std::pair<const char*, int GraphModel::*> ints[] = {{"graph_fwd_wg_per_cu", &GraphModel::g_cap_fwd}, {"graph_bwd_wg_per_cu", &GraphModel::g_cap_bwd},
                                                            {"graph_frame_chunks", &GraphModel::frame_chunks}, {"graph_dgrad_share", &GraphModel::g_dgrad_share}};
  for (auto& f : flags) if (name == f.first) this->*f.second = v != 0;
  for (auto& f : ints) if (name == f.first) this->*f.second = (int)v;
  if (name == "grid_graph") {
    grid_g_auto = v == 0;
    if (v > 0) grid_g = (int)v;
  }
  if (name == "dropout_seed") { dropout_seed = (unsigned long long)v; dropout_counter = 0; }
  return MWW_OK;
}

int GraphModel::set_dropout_mask(mww_ctx* c, const uint8_t* mask, int B) {
  if (!mask) { keep_explicit = false; return MWW_OK; }
  if (B <= 0 || B > c->max_batch) return fail(MWW_ERR_INVALID, "bad batch size");
  if (!(dropout > 0.f)) return fail(MWW_ERR_STATE, "model was created with dropout = 0");
  const size_t n = (size_t)B * c->t_last * c->c_last;
  std::vector<float> h(n);
  const float sc = 1.0f / (1.0f - dropout);
  for (size_t i = 0; i < n; ++i) h[i] = mask[i] ? sc : 0.f;
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipMemcpyAsync(keep, h.data(), n * sizeof(float), hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  keep_explicit = true;
  return MWW_OK;
}

// p<i> / g<i> / bn<i> of op i (1-based), keep, and x (written out first where the batch is descriptor-only)
int GraphModel::debug_tensor(mww_ctx* c, const char* name, int B, DebugTensor* t) {
  auto gidx = [&](const char* prefix) -> int {
    const size_t pl = strlen(prefix);
    if (strncmp(name, prefix, pl) != 0 || name[pl] < '0' || name[pl] > '9') return -1;
    const int kk = atoi(name + pl);
    return (kk >= 1 && kk <= (int)G.size()) ? kk - 1 : -1;
  };
  int k;
  if ((k = gidx("p")) >= 0 || (k = gidx("g")) >= 0) {
    const GOp& o = G[k];
    *t = DebugTensor{name[0] == 'p' ? o.p : o.g, (int64_t)B * o.tout * o.cout, false, g_planes(c, o), o.pc, o.cout, g_pstride(c, o)};
  }
  else if ((k = gidx("bn")) >= 0) { t->src = G[k].bn; t->n = (int64_t)9 * G[k].cout; }
  else if (!strcmp(name, "keep")) { t->src = keep; t->n = (int64_t)B * c->t_last * c->c_last; }
  else if (!strcmp(name, "x")) {
    if (materialise_x(c)) return -1;
    t->src = c->x;
    t->n = (int64_t)B * c->frames * MWW_FEATURE_BINS;
  }
  else return 0;
  return 1;
}

}  // namespace mww
