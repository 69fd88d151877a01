// What the two engines of libmww_hip.so share: the context, its per-layer / per-op records, error reporting, profiling brackets and
// the helpers of mww_lib.hip that the conv/BN graph engine (graph_engine.hip) calls.  Internal: the ABI is include/mww.h.
#pragma once
#include <hip/hip_runtime.h>

#include <map>
#include <string>
#include <utility>
#include <vector>

#include "../../include/mww.h"
#include "kernels_bwd.hip.h"    // GradReduceArgs, XGather
#include "kernels_data.hip.h"   // AssembleArgs

// the fp32 block backward runs as the wide-workgroup form (option "bwd_wide"; kernels_bwdw.hip.h) unless told otherwise
// options "conv1_x6" (the conv1 weight gradient in the first block's backward kernel) and "conv1_x6_fwd" (the first convolution
// itself): see common.hip.h "fp32-grade products on the bf16 matrix pipe".  Same-session A/B at B = 1024 (profiles/round6_conv1_x6_ab.txt):
// backward 49.7 -> 44.0 us; forward 33.5 -> 36-37 us (the matrix pipe's 6.5 us are paid back by the slicing of x and W1 in a
// launch whose workgroups see three tiles each) - so the default is backward only.
#ifndef MWW_CONV1_X6_DEFAULT
#define MWW_CONV1_X6_DEFAULT 1
#endif
#ifndef MWW_CONV1_X6_FWD_DEFAULT
#define MWW_CONV1_X6_FWD_DEFAULT 0
#endif
#ifndef MWW_BWD_FIRST_WIDE_DEFAULT   // option "bwd_first_wide"
#define MWW_BWD_FIRST_WIDE_DEFAULT 0
#endif
#ifndef MWW_BWD_WIDE_DEFAULT
#define MWW_BWD_WIDE_DEFAULT 1
#endif
// option "dp_commit_late": the fp32 backward kernels commit the dp rows of a tile behind the depthwise recompute instead of with the
// input rows in P0 (kernels_bwdw.hip.h bwd_blockw_kernel, bwd_first_body.inc).  Bit-identical results; the default of each kernel
// family is the order that won its same-session A/B (profiles/dp_commit_late_ab.txt): the middle blocks and the first
// block gain 0.5-1 us per launch, the last block's launch (its group B is p_k, the dense kernel's rows and dz) reads the same either way.
#ifndef MWW_DP_COMMIT_LATE_BLOCK_DEFAULT   // bwd_blockw_kernel, middle blocks
#define MWW_DP_COMMIT_LATE_BLOCK_DEFAULT 1
#endif
#ifndef MWW_DP_COMMIT_LATE_LAST_DEFAULT    // bwd_blockw_kernel, the last block (LAST)
#define MWW_DP_COMMIT_LATE_LAST_DEFAULT 0
#endif
#ifndef MWW_DP_COMMIT_LATE_FIRST_DEFAULT   // bwd_first_kernel (x6 form), bwd_firstw_kernel
#define MWW_DP_COMMIT_LATE_FIRST_DEFAULT 1
#endif

namespace mww {

struct MetricState;   // kernels_head.hip.h

int fail(int code, const std::string& msg);   // sets mww_last_error(), returns code

#define HIPCHK(expr)                                                                              \
  do {                                                                                            \
    hipError_t e_ = (expr);                                                                       \
    if (e_ != hipSuccess)                                                                         \
      return fail(MWW_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));                \
  } while (0)

struct Layer {
  int cin, cout, k, tin, tout;
  // offsets into the flat parameter / state vectors
  int64_t o_dw_w, o_dw_b, o_pw_w, o_gamma, o_beta, o_mm, o_mv;
  // device buffers
  float* p = nullptr;          // pre-BN output [maxB][tout][cout]
  float* g = nullptr;          // gradient at the BN output (masked by ReLU) [maxB][tout][cout]
  float* stat_part = nullptr;  // [grid_fwd][2][cout]
  float* gstat_part = nullptr; // [grid_bwd or grid_head][2][cout]
  float* grad_part = nullptr;  // [grid_bwd][params of the block (+ conv1 for block 0)]
  int grad_part_stride = 0;
  float* bn = nullptr;         // 9 x cout: scale, shift, mean, rstd, c1, mg, mgx, (spare x2)
  // statistics hand-over without finalize launches (common.hip.h): [parity][kStatRows][2][cout] for the forward
  // sums (x, x^2) and the backward sums (g, g*xhat); *_cur = rows the latest producer launch added to
  double* facc[2] = {nullptr, nullptr};
  double* gacc[2] = {nullptr, nullptr};
  double* facc_cur = nullptr;
  double* gacc_cur = nullptr;
};

// one conv -> BN/SSN -> ReLU op of a mww_convnet_desc graph (kernels_graph.hip.h)
struct GOp {
  int n_src = 0, src[MWW_MAX_OP_SOURCES] = {0, 0, 0}, toff[MWW_MAX_OP_SOURCES] = {0, 0, 0};
  int sc0[MWW_MAX_OP_SOURCES] = {0, 0, 0}, scn[MWW_MAX_OP_SOURCES] = {0, 0, 0};   // channel slice of each source
  bool src_first[MWW_MAX_OP_SOURCES] = {false, false, false}, src_last[MWW_MAX_OP_SOURCES] = {false, false, false};   // this op's place among the consumers of that slice (backward order)
  int k = 1, dil = 1, cin = 0, cout = 0, groups = 1, slots = 0, tin = 0, tout = 0;
  int kind = MWW_OP_CONV, stride = 1, norm = MWW_NORM_BN, act = MWW_ACT_RELU;
  int res_src = -1, res_drop = 0;     // residual branch added before this op's activation
  std::vector<int> adders;           // (residual ops) the ops that add this one
  int64_t o_w = 0, o_gamma = 0, o_beta = 0, o_mm = 0, o_mv = 0;
  float *p = nullptr, *g = nullptr, *stat_part = nullptr, *gstat_part = nullptr, *grad_part = nullptr, *bn = nullptr;
  bool needs_dx = false;
  bool twin_next = false;     // op i+1 is an independent op of the same shape: the pair shares its launches
  int planes = 1, pc = 0;     // > 1: every consumer reads one of `planes` equal channel slices of pc channels: the tensors p / g may be
                              // stored one plane per slice (kernels_graph.hip.h GSrc; "graph_planar")
  size_t lds_fwd = 0, lds_dx = 0, lds_wg = 0;
  // statistics hand-over (kernels_graph.hip.h): [parity][kStatRows][2][cout] accumulator rows of the forward / backward sums,
  // *_cur = the rows the latest producer launch added to; first_consumer = the lowest op index that reads this op
  double* facc[2] = {nullptr, nullptr};
  double* gacc[2] = {nullptr, nullptr};
  double* facc_cur = nullptr;
  double* gacc_cur = nullptr;
  int first_consumer = -1;
};

struct ProfileEntry {
  std::string name;
  hipEvent_t a, b;
};

// RCCL bound at run time (dlopen: the library loads on hosts without RCCL and shares the copy a framework in the same
// process has already loaded); only the five entry points the gradient / statistics exchange needs
struct RcclApi {
  void* so = nullptr;
  struct UniqueId { char internal[128]; };
  int (*GetUniqueId)(UniqueId*) = nullptr;
  int (*CommInitRank)(void**, int, UniqueId, int) = nullptr;
  int (*AllReduce)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;
  int (*CommDestroy)(void*) = nullptr;
  int (*CommCount)(void*, int*) = nullptr;   // optional: mww_allreduce_world
  const char* (*GetErrorString)(int) = nullptr;
};

constexpr int kRing = 8;
constexpr int kDenseChunks = 32;  // batch chunks of the dense-weight gradient reduction

}  // namespace mww

struct mww_ctx {
  mww_mixednet_desc d;
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  int n_cu = 256;
  int grid_fwd = 0, grid_bwd = 0, grid_head = 0;
  bool conv1_x6 = MWW_CONV1_X6_DEFAULT != 0;   // conv1 weight gradient as six bf16 slice products per fp32 product (stride-1 shapes, fp32 mode)
  bool conv1_x6_fwd = MWW_CONV1_X6_FWD_DEFAULT != 0;
  bool bwd_first_wide = MWW_BWD_FIRST_WIDE_DEFAULT != 0;   // stride-1 first block (3-tap conv1) with conv1_x6: the 512-thread form of its backward kernel   // ... and the first convolution of the forward kernel
  bool bwd_wide = MWW_BWD_WIDE_DEFAULT != 0;   // fp32 block backward kernels: 512 threads per workgroup (bwd_blockw_kernel) or 256 (bwd_block_kernel)
  int dp_commit_late = -1;   // -1: the per-family defaults above; 0 / 1: every kernel that has both orders
  int64_t P = 0, S = 0;
  int64_t o_conv1 = 0, o_dense_w = 0, o_dense_b = 0;
  int t_last = 0, c_last = 0, dwd_stride = 0;
  std::vector<mww::Layer> L;
  // conv/BN graph models (mww_create_convnet)
  bool generic = false;
  std::vector<mww::GOp> G;
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
  int metric_launches = 0;   // launches of the step being enqueued that carry the metric role (kernels_head.hip.h MetricState: one writer)
  bool g_planar = true;   // "graph_planar": tensors read only as equal channel slices are stored one plane per slice
  bool g_static = true;   // "graph_static_shapes": ops whose shape has a compile-time instantiation (MWW_G_SHAPES) use it
  int g_chunks = 0;   // "graph_frame_chunks" (g_chunks())
  int g_dgrad_share = 50;   // "graph_dgrad_share"
  bool grid_g_auto = true;   // per-launch grids from the kernel's occupancy (g_role_grid); "grid_graph" > 0 fixes one grid
  std::map<std::pair<const void*, size_t>, int> g_occ;   // workgroups per CU of (kernel, dynamic LDS)
  // data-parallel exchange hook (mww_set_allreduce_hook)
  mww_allreduce_fn hook = nullptr;
  void* hook_user = nullptr;
  int world = 1;
  bool sync_bn = false, reduce_grads = false;
  struct RcclState* rccl = nullptr;  // mww_allreduce_init: the library's own communicator + side stream (the hook then points at it)
  float* sync_buf = nullptr;        // [layers][fwd 2C | bwd 2C] statistics sums being exchanged
  std::vector<int64_t> sync_off;    // offset of layer i in sync_buf
  float *params = nullptr, *grads = nullptr, *adam_m = nullptr, *adam_v = nullptr, *mask = nullptr;
  unsigned char* direct = nullptr;
  std::vector<unsigned char> direct_host;   // host copy: which parameters' gradients are written directly by a folding kernel
  bool exchange_pending = false;            // a deferred bucket exchange is in flight (data-parallel step)
  int grad_buckets = 1;                     // data-parallel step: gradient exchanged in this many buckets ("grad_buckets" option; 2 = first
                                            // bucket overlapped with the backward tail - slower at W = 1, unmeasured at W > 1, so not the default)
  float* bn_state = nullptr;
  float *x = nullptr, *y = nullptr, *sw = nullptr, *z = nullptr, *prob = nullptr, *dz = nullptr, *loss_part = nullptr;
  float* a0 = nullptr;     // relu(conv1(x)) [max_batch][Ta][conv1_filters]: written by the training forward, read by bwd_first_kernel
  float* gbuf[2] = {nullptr, nullptr};   // the two buffers the blocks' g_k take in turn (block k uses gbuf[k & 1])
  float* dwd_part = nullptr;
  mww::MetricState* metrics = nullptr;
  // "mailboxes": pinned host memory mapped into the device address space.  The host writes one
  // step's descriptors (windows, masks, labels, weights, Adam step size) into mailbox m and the
  // kernels read them in place over PCIe (56 KB/step) — no H2D copy kernels on the stream.  A
  // mailbox is rewritten only after the event of its previous use has completed.
  char* mail_host[mww::kRing] = {};
  char* mail_dev[mww::kRing] = {};
  hipEvent_t mail_ev[mww::kRing] = {};
  int mail_cur = 0;
  bool mail_open = false;
  size_t mail_off_masks = 0, mail_off_y = 0, mail_off_sw = 0, mail_off_hyper = 0, mail_bytes = 0;
  int targets_in_mail = 0;   // rows of (y, sw) sitting in the current mailbox, not yet on the device
  // side stream: work that is off the critical path of the step (metric update, dense-weight gradient)
  // descriptors reach HBM through a DMA copy on their own stream, issued as soon as the host has
  // written the mailbox — it overlaps the previous step's kernels; only the Adam step size is read in
  // place from the mapped mailbox
  hipStream_t copy_stream = nullptr;
  char* mail_hbm[mww::kRing] = {};
  hipEvent_t ev_copy[mww::kRing] = {};
  hipStream_t side = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  bool side_pending = false;
  int asm_split = 2;        // workgroups per window of the assembly kernel ("assemble_split" option)
  // "fused_input" option (default on, specialised MixedNet kernels only): mww_assemble_batch only uploads the window
  // descriptors; the first block's forward / backward kernels gather their rows from the stores themselves
  // (kernels_fwd.hip.h XGather).  x is materialised (assemble_kernel) only for a reader that needs it.
  bool fused_input = true;
  bool x_lazy = false;
  int lazy_slot = -1;
  mww::AssembleArgs lazy_a;
  const float* y_cur = nullptr;   // labels / sample weights the kernels read: the y / sw buffers, or the rows that
  const float* sw_cur = nullptr;  // travelled in the mailbox of a descriptor-only batch
  // "bn_inline" option (default on): BN statistics travel through replicated fp64 accumulator rows and are folded by
  // their first consumer instead of by a finalize launch (off with sync-BN: the sums must be exchanged in between)
  bool bn_inline = true;
  bool g_role_split = true;   // launches that hold several roles (twin ops, weight + data gradient) divide the workgroups between the
                              // roles instead of multiplying them ("graph_role_split"; needs the statistics hand-over: the partial-row
                              // readers assume one row count per tensor)
  bool g_inline_ok = false;   // conv/BN graph: every op is a convolution with a BatchNorm and no residual branch => hand-over possible
  int fpar = 0, gpar = 0;   // accumulator parity of the next training forward / backward
  bool tail_pending = false, tail_metrics = false;   // dense gradient (+ metrics) ride in the first backward launch
  bool tail_in_reduce = false;   // ... or, with the statistics hand-over, in the gradient-reduction launch ("tail_roles" option)
  bool tail_roles = true;
  void* store[MWW_MAX_STORES] = {};
  int store_dtype[MWW_MAX_STORES] = {};
  int64_t store_elems[MWW_MAX_STORES] = {};
  int64_t step = 0;
  int have_batch = 0, have_targets = 0;
  bool use_graphs = false, profile = false;
  bool profile_split = false;   // "profile_split" option: keep weight- and data-gradient of a graph op in separate launches
  bool use_side = false;  // "side_stream" option: metric update + dense-weight gradient on a second stream (measured: co-running
                          // kernels displace workgroups of the occupancy-tuned block kernels; serial is 8 us/step faster)
  bool pw_bf16 = false;   // 1x1 contractions with bf16 operands (mww_set_option "pointwise_bf16")
  bool st_bf16 = false;   // p_k / g_k stored as bf16 ("storage_bf16", implies pointwise_bf16: BASELINE configs[4])
  bool bce_clipped = false;   // "bce_from_logits" 0: probability-form BCE with the Keras clip instead of the logits form (common.hip.h)
  bool bn_eval_ready = false;   // inside mww_evaluate_windows: the moving statistics are folded once, not per batch
  int ablate = 0;
  unsigned long long* phase_clk = nullptr;   // profiling: [2*layers][2048 workgroups][kClkSlots]
  std::vector<mww::ProfileEntry> prof;
  // cached graphs keyed by (B, flags)
  struct GraphEntry { int B, flags, mail, par; hipGraphExec_t exec; };
  std::vector<GraphEntry> graphs;
};

namespace mww {

struct Launcher {
  mww_ctx* c;
  hipEvent_t ea = nullptr;
  const char* name = nullptr;
  size_t idx = 0;   // this bracket's entry (a launch that has to write x out first opens a bracket of its own inside the caller's)
  void begin(const char* n, int layer = -1) {
    if (!c->profile) return;
    name = n;
    idx = c->prof.size();
    ProfileEntry e;
    e.name = n;
    if (layer >= 0) e.name += std::to_string(layer + 1);
    (void)hipEventCreate(&e.a);
    (void)hipEventCreate(&e.b);
    (void)hipEventRecord(e.a, c->stream);
    c->prof.push_back(e);
  }
  void end() {
    if (!c->profile || idx >= c->prof.size()) return;
    (void)hipEventRecord(c->prof[idx].b, c->stream);
  }
};

enum { BN_SCALE = 0, BN_SHIFT, BN_MEAN, BN_RSTD, BN_C1, BN_MG, BN_MGX };

// ---- mww_lib.hip
const float* mail_hyper(mww_ctx* c);
int materialise_x(mww_ctx* c);   // descriptor-only batch -> x, for readers outside the first block's kernels
XGather x_gather(mww_ctx* c);
int enqueue_side_work(mww_ctx* c, int B, bool metrics, bool loss, const float* p_last, const float* scale, const float* shift, const float* keep);
// sync-BN: the partial rows (or their sum over the ranks) the finalize kernel should read
struct StatSource { const float* part; int G; float inv_n; float dscale; };
int exchange_stats(mww_ctx* c, Launcher& lp, const char* what, int layer, const float* part, int G, int C, int bwd, float local_inv_n, StatSource* out);
int enqueue_grad_assembly(mww_ctx* c, int B, GradReduceArgs& ga, bool fuse_adam, int64_t lo = 0, int64_t hi = -1, bool last_range = true);

// ---- graph_engine.hip: conv/BN graph models (mww_create_convnet)
// gfx950 has 160 KB of LDS per CU; tiles above the 64 KB default need the function attribute
constexpr size_t kMaxDynLds = 144 * 1024;
// planar tensors (GOp::planes) lie kPlanePad floats further apart than their size: without it two planes lie a multiple of 4-8 KB
// apart - max_batch x T x pc x 4 bytes - and twin ops that walk their planes in step hit the same HBM channels: the 16-channel
// twin backward launch went 45 -> 55 us
constexpr long long kPlanePad = 1088;   // 17 x 256 bytes
// planes of op `o`'s tensors in effect (1 = interleaved) and the distance between two planes in floats
int g_planes(const mww_ctx* c, const GOp& o);
long long g_pstride(const mww_ctx* c, const GOp& o);
bool g_stem_gathers(const mww_ctx* c);
// validates a graph description and plans it: ops with their LDS sizes, gradient routing, twins and planar tensors, the offsets
// into the flat parameter / state vectors (P, S: the sizes so far - the head's parameters follow)
struct GPlan {
  std::vector<GOp> ops;
  int64_t P = 0, S = 0;
  bool inline_ok = false;   // statistics hand-over possible (mww_ctx::g_inline_ok)
  int chunks = 0;           // default of "graph_frame_chunks"
};
int g_plan_convnet(const mww_convnet_desc& d, GPlan* plan);
int g_enqueue_forward(mww_ctx* c, int B, bool training, bool update_moving, bool loss, bool metrics);
int g_enqueue_backward(mww_ctx* c, int B, bool fuse_adam);

}  // namespace mww
