// What the units of libmww_hip.so's training side share: the core of a context (mww_ctx), the interface of its model part (Model:
// block_engine.hip, graph_engine.hip), the tensor record of both, error reporting, profiling brackets and the helpers of mww_lib.hip
// that the engines and the step features call.  A step feature's state and interface are declared in its own header
// (kernels_qat / ema / bnre / sam.hip.h) and its host code sits with its kernels (tu_*.hip).  Internal: the ABI is include/mww.h.
#pragma once
#include <hip/hip_runtime.h>

#include <map>
#include <string>
#include <utility>
#include <vector>

#include "../../include/mww.h"
#include "kernels_bwd.hip.h"    // GradReduceArgs, XGather
#include "kernels_data.hip.h"   // AssembleArgs
#include "kernels_bnre.hip.h"   // the step features: BnreState,
#include "kernels_ema.hip.h"    // EmaState,
#include "kernels_qat.hip.h"    // QatState,
#include "kernels_sam.hip.h"    // SharpState

namespace mww {

struct MetricState;   // kernels_head.hip.h
struct RcclState;     // tu_exchange.hip

int fail(int code, const std::string& msg);   // sets mww_last_error(), returns code

#define HIPCHK(expr)                                                                              \
  do {                                                                                            \
    hipError_t e_ = (expr);                                                                       \
    if (e_ != hipSuccess)                                                                         \
      return fail(MWW_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));                \
  } while (0)
#define MWW_TRY(call)                                                                             \
  do {                                                                                            \
    int rc_ = (call);                                                                             \
    if (rc_) return rc_;                                                                          \
  } while (0)

// the device buffers every BN'd tensor of either engine owns: block k of a MixedNet (Layer) or op i of a graph (GOp)
struct Tensor {
  float* p = nullptr;          // pre-BN output [maxB][tout][cout]
  float* g = nullptr;          // gradient at the BN output (masked by ReLU) [maxB][tout][cout]
  float* stat_part = nullptr;  // [rows_fwd][2][cout]
  float* gstat_part = nullptr; // [rows_bwd][2][cout]
  float* grad_part = nullptr;  // [rows][the weights this tensor's backward launch produces]
  float* bn = nullptr;         // 9 x cout: scale, shift, mean, rstd, c1, mg, mgx, (spare x2)
  // statistics hand-over without finalize launches (common.hip.h): [parity][kStatRows][2][cout] for the forward
  // sums (x, x^2) and the backward sums (g, g*xhat); which parity a launch adds to: fwd_rows / bwd_rows below
  double* facc[2] = {nullptr, nullptr};
  double* gacc[2] = {nullptr, nullptr};
};
// everything but p and g (whose sizes and owners are the engine's business) / every buffer that is set
int tensor_alloc(Tensor* t, int cout, size_t rows_fwd, size_t rows_bwd, size_t grad_part);
void tensor_free(Tensor* t);

struct Layer : Tensor {
  int cin, cout, k, tin, tout;
  // offsets into the flat parameter / state vectors
  int64_t o_dw_w, o_dw_b, o_pw_w, o_gamma, o_beta, o_mm, o_mv;
  int grad_part_stride = 0;    // grad_part: [grid_bwd][params of the block (+ conv1 for block 0)]
};

// one conv -> BN/SSN -> ReLU op of a mww_convnet_desc graph (kernels_graph.hip.h)
struct GOp : Tensor {
  int n_src = 0, src[MWW_MAX_OP_SOURCES] = {0, 0, 0}, toff[MWW_MAX_OP_SOURCES] = {0, 0, 0};
  int sc0[MWW_MAX_OP_SOURCES] = {0, 0, 0}, scn[MWW_MAX_OP_SOURCES] = {0, 0, 0};   // channel slice of each source
  bool src_first[MWW_MAX_OP_SOURCES] = {false, false, false}, src_last[MWW_MAX_OP_SOURCES] = {false, false, false};   // this op's place among the consumers of that slice (backward order)
  int k = 1, dil = 1, cin = 0, cout = 0, groups = 1, slots = 0, tin = 0, tout = 0;
  int kind = MWW_OP_CONV, stride = 1, norm = MWW_NORM_BN, act = MWW_ACT_RELU;
  int res_src = -1, res_drop = 0;     // residual branch added before this op's activation
  std::vector<int> adders;           // (residual ops) the ops that add this one
  int64_t o_w = 0, o_gamma = 0, o_beta = 0, o_mm = 0, o_mv = 0;
  bool needs_dx = false;
  bool twin_next = false;     // op i+1 is an independent op of the same shape: the pair shares its launches
  int planes = 1, pc = 0;     // > 1: every consumer reads one of `planes` equal channel slices of pc channels: the tensors p / g may be
                              // stored one plane per slice (kernels_graph.hip.h GSrc; "graph_planar")
  size_t lds_fwd = 0, lds_dx = 0, lds_wg = 0;
  int first_consumer = -1;    // the lowest op index that reads this op: its launch folds the forward statistics
};

struct ProfileEntry {
  std::string name;
  hipEvent_t a, b;
};

// data-parallel exchange (tu_exchange.hip installs it: mww_set_allreduce_hook, mww_allreduce_init; the step of mww_lib.hip and
// the engines read it)
struct Exchange {
  mww_allreduce_fn hook = nullptr;
  void* user = nullptr;
  int world = 1;
  bool sync_bn = false, reduce_grads = false;
  RcclState* rccl = nullptr;        // mww_allreduce_init: the library's own communicator + side stream (the hook then points at it)
  float* sync_buf = nullptr;        // [layers][fwd 2C | bwd 2C] statistics sums being exchanged
  std::vector<int64_t> sync_off;    // offset of layer i in sync_buf
  bool pending = false;             // a deferred bucket exchange is in flight (data-parallel step)
  int buckets = 1;                  // data-parallel step: gradient exchanged in this many buckets ("grad_buckets" option; 2 = first
                                    // bucket overlapped with the backward tail - slower at W = 1, unmeasured at W > 1, so not the default)
};

constexpr int kRing = 8;
constexpr int kDenseChunks = 32;  // batch chunks of the dense-weight gradient reduction

// the last tensor as the dense-weight gradient reads it (kernels_head.hip.h DenseGradArgs): BN'd p_L (bf16: stored so), the
// dropout keep-scale and the residual branch added before the last ReLU, where the model has them
struct DenseSource {
  const float *p = nullptr, *scale = nullptr, *shift = nullptr, *keep = nullptr, *rp = nullptr, *rscale = nullptr, *rshift = nullptr;
  int rT = 0, rdrop = 0, bf16 = 0;
};

enum OptionOwner { OPT_CORE, OPT_BLOCK, OPT_GRAPH };
// one option of mww_set_option: lo <= hi: accepted range (hi_cu > 0: up to hi_cu workgroups per CU) and what a value outside it reports
struct OptionRow { const char* name; OptionOwner owner; int64_t lo, hi; int hi_cu; const char* range_error; };

// what mww_debug_read copies out: n floats at src; stored as bf16 / as `planes` planes of pc channels, pstride floats apart
struct DebugTensor { const float* src = nullptr; int64_t n = 0; bool bf16 = false; int planes = 1, pc = 0, cout = 0; long long pstride = 0; };

struct BnSlots { int64_t o_gamma, o_beta, o_mv; int n; };   // a BN's (or a bias's) places in the flat vectors

// The model part of a context: the topology, its tensors and options, and the launch sequences of one engine
// (block_engine.hip: the specialised MixedNet kernels; graph_engine.hip: conv/BN graphs).  The destructor frees its buffers.
struct Model {
  Model() = default;
  Model(const Model&) = delete;   // (it owns device buffers)
  virtual ~Model() {}
  // after the device is open: the offsets into the flat vectors (sets P, S, o_dense_*, t_last, c_last, dwd_stride) and the
  // default grids; then, behind alloc_common, the model's own buffers (bn: the slots init_defaults marks)
  virtual int layout(mww_ctx* c) = 0;
  virtual int alloc(mww_ctx* c, std::vector<BnSlots>* bn) = 0;
  virtual int enqueue_forward(mww_ctx* c, int B, bool training, bool update_moving, bool loss, bool metrics) = 0;
  virtual int enqueue_backward(mww_ctx* c, int B, bool fuse_adam) = 0;
  // BN re-estimation (kernels_bnre.hip.h): enqueue the collect for the training-mode forward of B windows just enqueued - one
  // table row per BN'd tensor, saying where that forward left the tensor's sums (enqueue_bnre_collect launches them)
  virtual int enqueue_bn_collect(mww_ctx* c, int B) = 0;
  virtual std::vector<int> stat_widths() const = 0;   // channels of every BN'd tensor, in sync-BN order
  virtual bool lazy_ok(const mww_ctx* c, int B) const = 0;   // may this batch stay descriptor-only ("fused_input")?
  virtual bool step_counter(unsigned long long* n) { return false; }   // the counter this step's dropout mask is drawn from, if one is
  // the model's word of the hipGraph cache key; *handover: the statistics hand-over is possible (its parities are baked into a capture)
  virtual unsigned replay_key(bool* handover) const = 0;
  virtual bool eval_fold_cached() const { return false; }   // the eval BN fold survives from batch to batch of one evaluation
  virtual int debug_tensor(mww_ctx* c, const char* name, int B, DebugTensor* t) = 0;   // 1: found, 0: not one of mine, < 0: error
  virtual int set_option(mww_ctx* c, const OptionRow& o, int64_t v) = 0;   // (rows of the other engine: no-op)
  virtual int set_dropout_mask(mww_ctx* c, const uint8_t* keep, int B);
};

}  // namespace mww

// The core of a context: one device + one HIP stream + the flat vectors, mailboxes, step state and options no engine owns.
struct mww_ctx {
  mww::Model* model = nullptr;
  int frames = 0, max_batch = 0;
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  int n_cu = 256;
  int grid_head = 0;
  int64_t P = 0, S = 0;
  int64_t o_dense_w = 0, o_dense_b = 0;
  int t_last = 0, c_last = 0, dwd_stride = 0;
  int metric_launches = 0;   // launches of the step being enqueued that carry the metric role (kernels_head.hip.h MetricState: one writer)
  float *params = nullptr, *grads = nullptr, *adam_m = nullptr, *adam_v = nullptr, *mask = nullptr;
  // the step features, each with its state (the header named), host code and kernels in a unit of its own
  mww::QatState qat;       // kernels_qat.hip.h
  mww::EmaState ema;       // kernels_ema.hip.h
  mww::BnreState bnre;     // kernels_bnre.hip.h
  mww::SharpState sharp;   // kernels_sam.hip.h
  mww::Exchange xch;
  unsigned char* direct = nullptr;
  std::vector<unsigned char> direct_host;   // host copy: which parameters' gradients are written directly by a folding kernel
  float* bn_state = nullptr;
  float *x = nullptr, *y = nullptr, *sw = nullptr, *z = nullptr, *prob = nullptr, *dz = nullptr, *loss_part = nullptr;
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
  // "fused_input" option (default on): mww_assemble_batch only uploads the window descriptors where the model's first
  // kernels gather their rows from the stores themselves (kernels_fwd.hip.h XGather; Model::lazy_ok).  x is materialised
  // (assemble_kernel) only for a reader that needs it.
  bool fused_input = true;
  bool x_lazy = false;
  int lazy_slot = -1;
  mww::AssembleArgs lazy_a;
  const float* y_cur = nullptr;   // labels / sample weights the kernels read: the y / sw buffers, or the rows that
  const float* sw_cur = nullptr;  // travelled in the mailbox of a descriptor-only batch
  // "bn_inline" option (default on): BN statistics travel through replicated fp64 accumulator rows and are folded by
  // their first consumer instead of by a finalize launch (off with sync-BN: the sums must be exchanged in between)
  bool bn_inline = true;
  int fpar = 0, gpar = 0;   // accumulator parity of the next training forward / backward
  bool tail_pending = false, tail_metrics = false;   // dense gradient (+ metrics) ride in the first backward launch
  bool tail_in_reduce = false;   // ... or, with the statistics hand-over, in the gradient-reduction launch ("tail_roles" option)
  mww::DenseSource tail_src;     // what that dense gradient reads
  bool tail_roles = true;
  void* store[MWW_MAX_STORES] = {};
  int store_dtype[MWW_MAX_STORES] = {};
  int64_t store_elems[MWW_MAX_STORES] = {};
  int64_t step = 0;
  int have_batch = 0, have_targets = 0;
  bool use_graphs = false, profile = false;
  bool use_side = false;  // "side_stream" option: metric update + dense-weight gradient on a second stream (measured: co-running
                          // kernels displace workgroups of the occupancy-tuned block kernels; serial is 8 us/step faster)
  bool bce_clipped = false;   // "bce_from_logits" 0: probability-form BCE with the Keras clip instead of the logits form (common.hip.h)
  bool bn_eval_ready = false;   // inside mww_evaluate_windows: the moving statistics are folded once, not per batch
  std::vector<mww::ProfileEntry> prof;
  // cached graphs keyed by (B, flags, mailbox, the core's and the model's option / parity words)
  struct GraphEntry { int B, flags, mail; unsigned core, model; hipGraphExec_t exec; };
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
  // the bracket just opened and closed held no launch: drop its entry
  void cancel() {
    if (!c->profile) return;
    (void)hipEventDestroy(c->prof.back().a);
    (void)hipEventDestroy(c->prof.back().b);
    c->prof.pop_back();
  }
};

enum { BN_SCALE = 0, BN_SHIFT, BN_MEAN, BN_RSTD, BN_C1, BN_MG, BN_MGX };

// The accumulator rows of tensor t in the walk being enqueued: .acc = the rows this walk's producer launches add to and its
// folding launches read, .clear = the other parity's rows, which the producers zero for the next walk.  One expression serves
// the writers and the readers because c->fpar (c->gpar) is constant from the first launch that adds to a tensor's rows to the
// last launch that folds them: the forward sums of a tensor are produced and folded inside one forward walk, the backward sums
// are produced by the head of a step's forward walk or by an op's consumers in its backward walk and folded in that same
// backward walk, and each walk flips its own parity exactly once, as the last thing it does about parity (the forward walk
// after the head's fold is built).  A graph replay (mww_train_step) flips both parities without running a walk: there is
// no per-tensor state for that to leave behind.
inline StatAcc fwd_rows(const mww_ctx* c, const Tensor& t) { return StatAcc{t.facc[c->fpar], t.facc[c->fpar ^ 1]}; }
inline StatAcc bwd_rows(const mww_ctx* c, const Tensor& t) { return StatAcc{t.gacc[c->gpar], t.gacc[c->gpar ^ 1]}; }

// the fp32 vector this call's forward stands on: the master, or the weight average in a non-training call under "ema_forward"
inline float* fwd_source(const mww_ctx* c) { return c->ema.src ? c->ema.vec : c->params; }
// the parameter vector the forward / backward launches read: that vector, or its fake-quantized shadow ("weight_qat")
inline float* fwd_params(const mww_ctx* c) { return c->qat.enabled ? c->qat.shadow : fwd_source(c); }
// the moving statistics an eval-mode fold reads: the master's, or - in a call that stands on the average - the average's own
// re-estimated ones while they are valid
inline float* eval_bn_state(const mww_ctx* c) { return (c->ema.src && c->bnre.valid) ? c->bnre.ema_bn : c->bn_state; }

// ---- mww_lib.hip
template <typename T>
int dev_alloc(T** p, size_t n) {
  HIPCHK(hipMalloc((void**)p, std::max<size_t>(n, 1) * sizeof(T)));
  HIPCHK(hipMemset(*p, 0, std::max<size_t>(n, 1) * sizeof(T)));
  return MWW_OK;
}
int create_context(Model* m, int frames, int max_batch, int device, void* stream, mww_ctx** out);   // takes the model over, also when it fails
// what the step features' units need of the core: the Adam launch, the hipGraph cache, synchronous copies on the context's
// stream, and the opening (batch_ready) and closing (join_side, mail_commit) of a call that runs a forward
int enqueue_adam(mww_ctx* c);
void drop_graphs(mww_ctx* c);
int copy_in(mww_ctx* c, void* dst, const void* src, size_t bytes);
int copy_out(mww_ctx* c, void* dst, const void* src, size_t bytes);
int batch_ready(mww_ctx* c);
int join_side(mww_ctx* c);
int mail_commit(mww_ctx* c);
const float* mail_hyper(mww_ctx* c);
int materialise_x(mww_ctx* c);   // descriptor-only batch -> x, for readers outside the first block's kernels
XGather x_gather(mww_ctx* c);
int enqueue_side_work(mww_ctx* c, int B, bool metrics, bool loss, const DenseSource& last);
// sync-BN: the partial rows (or their sum over the ranks) the finalize kernel should read
struct StatSource { const float* part; int G; float inv_n; float dscale; };
int exchange_stats(mww_ctx* c, Launcher& lp, const char* what, int layer, const float* part, int G, int C, int bwd, float local_inv_n, StatSource* out);
// what exchange_stats handed the forward finalize of `layer` in the forward just enqueued (nothing is launched or exchanged)
StatSource forward_stat_source(const mww_ctx* c, int layer, const float* part, int G, int C, float local_inv_n);
int enqueue_grad_assembly(mww_ctx* c, int B, GradReduceArgs& ga, bool fuse_adam, int64_t lo = 0, int64_t hi = -1, bool last_range = true);
// the block engine's classifier head and the launch that opens its backward pass (BN_L's backward finalize + dense gradient +
// metrics): their kernels share kernels_head.hip.h / kernels_tail.hip.h with the core's own, which one unit alone can include
int head_frame_limit(int ch);   // final frames one head workgroup covers at `ch` channels
int enqueue_block_head(mww_ctx* c, int B, const Tensor& last, int T, int C, bool bf16, const BnFoldArgs& fold, const StatAcc& gacc, bool loss, bool metrics);
int enqueue_head_tail(mww_ctx* c, int B, const BnBwdFinalizeArgs& fin);

// ---- block_engine.hip: MixedNets on the specialised block kernels (mww_create)
bool shape_supported(const mww_mixednet_desc& d, std::string* why, bool bf16 = false);
int plan_mixednet(const mww_mixednet_desc& d, Model** out);

// ---- graph_engine.hip: conv/BN graph models (mww_create_convnet)
// validates a graph description and plans it: ops with their LDS sizes, gradient routing, twins and planar tensors, the offsets
// into the flat parameter / state vectors
int plan_convnet(const mww_convnet_desc& d, Model** out);

}  // namespace mww
