// libmww_hip.so — the C ABI of include/mww.h and the core of a context: device memory, mailboxes, batch assembly, gradient
// assembly / exchange / Adam, side work, the step driver and the option table.  The model part of a context is one of the two
// engines (block_engine.hip, graph_engine.hip); the step features (weight QAT, weight averaging, BN re-estimation, sharpness /
// clipping) and the exchange binding have units of their own (tu_qat / ema / bnre / sam / exchange.hip), reached through the
// interfaces of their headers; engine.hip.h holds what all of them share.
// One context = one device + one HIP stream + one model; every call enqueues on that stream.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <climits>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "engine.hip.h"
#include "kernels_data.hip.h"
#include "kernels_head.hip.h"
#include "kernels_tail.hip.h"

using namespace mww;

namespace {
thread_local std::string g_err;
}  // namespace

int mww::fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

namespace {

// ---------------------------------------------------------------------------------- the block engine's head
constexpr int kHeadMaxRows = 24;   // frames per frame group of the widest head_kernel instantiation below

int launch_head(mww_ctx* c, int ch, int jmax, bool bf16, const HeadArgs& a, int grid) {
#define X(C, J)                                                                                                \
  if (ch == C && jmax <= J) {                                                                                  \
    if (bf16)                                                                                                  \
      hipLaunchKernelGGL((head_kernel<C, J, true>), dim3(grid), dim3(kThreads), 0, c->stream, a);              \
    else                                                                                                       \
      hipLaunchKernelGGL((head_kernel<C, J>), dim3(grid), dim3(kThreads), 0, c->stream, a);                    \
    return MWW_OK;                                                                                             \
  }
  static_assert(kHeadMaxRows == 24, "the widest instantiation below");
  X(32, 2) X(32, 4) X(32, 8) X(32, 12) X(32, 16) X(32, 24) X(48, 2) X(48, 4) X(48, 8) X(48, 12) X(48, 16) X(48, 24) X(64, 2) X(64, 4) X(64, 8) X(64, 12) X(64, 16) X(64, 24)
#undef X
  return fail(MWW_ERR_UNSUPPORTED, "no head kernel for this (channels, frames) shape");
}

}  // namespace

namespace mww {

// final frames one head workgroup covers at `ch` channels (a thread keeps one float4 of every frame of its group)
int head_frame_limit(int ch) { return (kThreads / (ch / 4)) * kHeadMaxRows; }

int enqueue_block_head(mww_ctx* c, int B, const Tensor& last, int T, int C, bool bf16, const BnFoldArgs& fold, const StatAcc& gacc, bool loss, bool metrics) {
  float* const bn = last.bn;
  const HeadArgs h{last.p, bn + (size_t)BN_SCALE * C, bn + (size_t)BN_SHIFT * C, bn + (size_t)BN_MEAN * C, bn + (size_t)BN_RSTD * C,
                   fwd_params(c) + c->o_dense_w, fwd_params(c) + c->o_dense_b, (loss || metrics) ? c->y_cur : nullptr, c->sw_cur, c->z, c->prob, c->dz,
                   c->loss_part, last.gstat_part, B, T, 1.0f / (float)B, (loss ? kHeadTraining : 0) | (c->bce_clipped ? kHeadClippedLoss : 0), fold, gacc};
  const int q = C / 4, nrg = kThreads / q;
  Launcher lp{c};
  lp.begin("head");
  int rc = launch_head(c, C, (T + nrg - 1) / nrg, bf16, h, std::min(B, c->grid_head));
  lp.end();
  return rc;
}

// ---------------------------------------------------------------------------------- sequences
const float* mail_hyper(mww_ctx* c) { return reinterpret_cast<const float*>(c->mail_dev[c->mail_cur] + c->mail_off_hyper); }

// A read of the HBM copy of a descriptor-only batch's mailbox, enqueued after that slot was committed: the slot's stamp
// (mail_commit) lies in front of the read, so it is moved behind it - mail_begin waits for the stamp before the slot is
// rewritten, eight commits later.  (While the slot is still the current one, its commit comes after the read anyway.)
static int restamp_lazy_slot(mww_ctx* c) {
  if (c->lazy_slot >= 0 && c->lazy_slot != c->mail_cur) HIPCHK(hipEventRecord(c->mail_ev[c->lazy_slot], c->stream));
  return MWW_OK;
}

// labels / weights read in place from the mailbox of a descriptor-only batch -> the y / sw buffers (before that
// mailbox slot can be rewritten)
static int bring_targets(mww_ctx* c) {
  if (c->y_cur == c->y) return MWW_OK;
  const size_t n = (size_t)c->lazy_a.B * sizeof(float);
  HIPCHK(hipMemcpyAsync(c->y, c->y_cur, n, hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(c->sw, c->sw_cur, n, hipMemcpyDeviceToDevice, c->stream));
  c->y_cur = c->y;
  c->sw_cur = c->sw;
  return restamp_lazy_slot(c);
}

// descriptor-only batch -> x, for readers outside the first block's kernels
int materialise_x(mww_ctx* c) {
  int rc = bring_targets(c);
  if (rc || !c->x_lazy) return rc;
  AssembleArgs a = c->lazy_a;
  a.n_targets = 0;
  Launcher lp{c};
  lp.begin("assemble");
  hipLaunchKernelGGL(assemble_kernel, dim3(a.B * a.split), dim3(kThreads), 0, c->stream, a);
  lp.end();
  HIPCHK(hipGetLastError());
  c->x_lazy = false;
  return restamp_lazy_slot(c);
}

XGather x_gather(mww_ctx* c) {
  XGather g;
  memset(&g, 0, sizeof(g));
  if (!c->x_lazy) return g;
  const AssembleArgs& a = c->lazy_a;
  g.win = a.win;
  g.masks = a.masks;
  for (int i = 0; i < MWW_MAX_STORES; ++i) { g.store[i] = a.store[i]; g.dtype[i] = a.dtype[i]; }
  g.ntm = a.ntm;
  g.nfm = a.nfm;
  g.T = a.T;
  return g;
}

int join_side(mww_ctx* c) {
  if (c->side_pending) {
    HIPCHK(hipStreamWaitEvent(c->stream, c->ev_join, 0));
    c->side_pending = false;
  }
  return MWW_OK;
}

static DenseGradArgs dense_args(mww_ctx* c, int B, const DenseSource& s, float* part, int stride) {
  return DenseGradArgs{s.p, s.scale, s.shift, c->dz, part, B, c->t_last * c->c_last, c->c_last, stride, (B + kDenseChunks - 1) / kDenseChunks,
                       s.keep, s.rp, s.rscale, s.rshift, s.rT, s.rdrop, s.bf16};
}

// off the critical path: metric update and (training) the dense-weight gradient run on the side
// stream while the backward chain proceeds; joined before the gradient assembly
int enqueue_side_work(mww_ctx* c, int B, bool metrics, bool loss, const DenseSource& last) {
  Launcher lp{c};
  if (metrics || loss) {
    const bool inline_side = c->profile || !c->use_side;
    hipStream_t ss = inline_side ? c->stream : c->side;
    if (!inline_side) {
      HIPCHK(hipEventRecord(c->ev_fork, c->stream));
      HIPCHK(hipStreamWaitEvent(c->side, c->ev_fork, 0));
    }
    const bool one_launch = metrics && loss && inline_side;   // both pieces as roles of one launch (head_tail_kernel without a finalize role)
    if (metrics && !one_launch) {
      MetricsArgs ma{c->prob, c->y_cur, c->metrics, B, c->bce_clipped ? nullptr : c->z};
      lp.begin("metrics");
      hipLaunchKernelGGL(metrics_kernel, dim3(1), dim3(1024), 0, ss, ma);
      c->metric_launches += 1;
      lp.end();
    }
    if (loss) {
      const DenseGradArgs dg = dense_args(c, B, last, c->dwd_part, c->dwd_stride);
      const int ndchunks = (B + dg.chunk - 1) / dg.chunk;
      if (one_launch) {
        HeadTailArgs ht;
        memset(&ht, 0, sizeof(ht));
        ht.dense = dg;
        ht.met = MetricsArgs{c->prob, c->y_cur, c->metrics, B, c->bce_clipped ? nullptr : c->z};
        ht.n_fin = 0;
        ht.ndx = (dg.n + 1 + kThreads - 1) / kThreads;
        ht.ndy = ndchunks;
        ht.do_metrics = 1;
        c->metric_launches += 1;
        lp.begin("dense_grad+metrics");
        hipLaunchKernelGGL(head_tail_kernel, dim3(ht.ndx * ht.ndy + 1), dim3(kThreads), 0, ss, ht);
        lp.end();
      } else {
        lp.begin("dense_grad");
        hipLaunchKernelGGL(dense_grad_kernel, dim3((dg.n + 1 + kThreads - 1) / kThreads, ndchunks), dim3(kThreads), 0, ss, dg);
        lp.end();
      }
    }
    if (!inline_side) {
      HIPCHK(hipEventRecord(c->ev_join, c->side));
      c->side_pending = true;
    }
  }
  return MWW_OK;
}

// sync-BN: collapse this rank's partials, sum them over the ranks through the caller's hook, and hand
// the result to the finalize kernel as a single "partial" row.  Returns the pointer / row count /
// element count the finalize kernel should use.

int exchange_stats(mww_ctx* c, Launcher& lp, const char* what, int layer, const float* part, int G, int C, int bwd,
                   float local_inv_n, StatSource* out) {
  out->part = part;
  out->G = G;
  out->inv_n = local_inv_n;
  out->dscale = 1.0f;
  if (!(c->xch.hook && c->xch.sync_bn)) return MWW_OK;
  float* buf = c->xch.sync_buf + c->xch.sync_off[layer] + (bwd ? 2 * C : 0);
  StatCollapseArgs a{part, G, C, buf};
  lp.begin(what, layer);
  hipLaunchKernelGGL(stat_collapse_kernel, dim3(C), dim3(kThreads), 0, c->stream, a);
  lp.end();
  if (c->xch.hook(c->xch.user, buf, 2 * C, MWW_EXCHANGE_IN_ORDER) != 0) return fail(MWW_ERR_STATE, "all-reduce hook failed");
  out->part = buf;
  out->G = 1;
  out->inv_n = local_inv_n / (float)c->xch.world;
  out->dscale = 1.0f / (float)c->xch.world;
  return MWW_OK;
}

StatSource forward_stat_source(const mww_ctx* c, int layer, const float* part, int G, int C, float local_inv_n) {
  if (!(c->xch.hook && c->xch.sync_bn)) return StatSource{part, G, local_inv_n, 1.0f};
  // (every layer has its own place in sync_buf: the sums of the whole forward are still there)
  return StatSource{c->xch.sync_buf + c->xch.sync_off[layer], 1, local_inv_n / (float)c->xch.world, 1.0f / (float)c->xch.world};
}

}  // namespace mww
namespace {

// gradient assembly: fixed-order sum of the per-workgroup partials (+ the dense layer's, which come
// from the side stream), structural mask, optionally fused with the Adam update

// Gradient assembly of the parameter range [lo, hi): one grad_final_kernel launch (kernels_tail.hip.h) finishes every
// parameter of the range - fixed-order sums of the partial rows listed in `ga` (and of the rows the dense / metric
// roles produce when they ride along), the values the folding kernels already wrote (BN gamma / beta), zeros for
// parameters nothing contributes to - and applies the mask, and Adam when `apply_adam`.
int assemble_range(mww_ctx* c, int B, const GradReduceArgs& ga, int64_t lo, int64_t hi, bool tail_dense, bool metrics, bool apply_adam) {
  Launcher lp{c};
  std::vector<FinalSegment> segs;
  for (int i = 0; i < ga.nseg; ++i) {
    const GradSegment& g = ga.seg[i];
    if (g.dst < lo || g.dst >= hi) continue;
    if (g.dst + g.n > hi) return fail(MWW_ERR_STATE, "gradient segment straddles a bucket boundary");
    segs.push_back(FinalSegment{g.part, g.G, g.stride, g.n, g.dst, kSegPartials, 0});
  }
  GradFinalArgs a;
  memset(&a, 0, sizeof(a));
  if (tail_dense && c->o_dense_w >= lo && c->o_dense_w < hi) {
    a.dense = dense_args(c, B, c->tail_src, nullptr, 0);
    segs.push_back(FinalSegment{nullptr, B, 0, c->t_last * c->c_last + 1, (int)c->o_dense_w, kSegDense, 0});
  }
  std::sort(segs.begin(), segs.end(), [](const FinalSegment& x, const FinalSegment& y) { return x.dst < y.dst; });
  // the gaps between the segments: runs of parameters that are final in grad[] already ("direct") or untouched
  std::vector<FinalSegment> all;
  int64_t cur = lo;
  auto fill = [&](int64_t upto) {
    while (cur < upto) {
      const bool dir = c->direct_host[(size_t)cur] != 0;
      int64_t e = cur;
      while (e < upto && (c->direct_host[(size_t)e] != 0) == dir) ++e;
      all.push_back(FinalSegment{nullptr, 1, 0, (int)(e - cur), (int)cur, dir ? kSegDirect : kSegZero, 0});
      cur = e;
    }
  };
  for (const FinalSegment& sgm : segs) {
    if (sgm.dst < cur) return fail(MWW_ERR_STATE, "overlapping gradient segments");
    fill(sgm.dst);
    all.push_back(sgm);
    cur = sgm.dst + sgm.n;
  }
  fill(hi);
  a.met = MetricsArgs{c->prob, c->y_cur, c->metrics, B, c->bce_clipped ? nullptr : c->z};
  a.mask = c->mask;
  a.grad = c->grads;
  a.scale = 1.0f;
  a.adam = AdamArgs{c->params, c->grads, c->adam_m, c->adam_v, mail_hyper(c), (int)c->P, 0.9f, 0.999f, 1e-7f};
  a.apply_adam = apply_adam ? 1 : 0;
  for (size_t first = 0; first < all.size() || (metrics && first == 0); first += kMaxFinalSegments) {
    const int n = (int)std::min<size_t>(kMaxFinalSegments, all.size() - first);
    // workgroups are dispatched in block order: the longest role (the dense kernel's gradient: B strided rows of p_L per
    // parameter) takes the first blocks, so that it starts first
    int nb = 0, ns = 0;
    for (int pass = 0; pass < 2; ++pass)
      for (int i = 0; i < n; ++i) {
        const FinalSegment& sg = all[first + i];
        if ((sg.kind == kSegDense) != (pass == 0)) continue;
        a.seg[ns] = sg;
        a.seg[ns].block0 = nb;
        a.block0[ns] = nb;
        nb += (sg.n + kFinalCols - 1) / kFinalCols;
        ++ns;
      }
    for (int i = ns; i < kMaxFinalSegments; ++i) a.block0[i] = INT_MAX;
    a.nseg = n;
    a.nblocks = nb;
    a.do_metrics = (metrics && first == 0) ? 1 : 0;
    if (nb + a.do_metrics == 0) break;
    c->metric_launches += a.do_metrics;
    lp.begin(apply_adam ? "grad_final+adam" : "grad_final");
    hipLaunchKernelGGL(grad_final_kernel, dim3(nb + a.do_metrics), dim3(kThreads), 0, c->stream, a);
    lp.end();
    if (all.empty()) break;
  }
  return MWW_OK;
}

// gradient exchange of a finished range through the caller's hook (data-parallel step)
int exchange_range(mww_ctx* c, int64_t lo, int64_t hi, int flags) {
  if (c->xch.hook(c->xch.user, flags == MWW_EXCHANGE_FLUSH ? nullptr : c->grads + lo, flags == MWW_EXCHANGE_FLUSH ? 0 : hi - lo, flags) != 0)
    return fail(MWW_ERR_STATE, "all-reduce hook failed");
  return MWW_OK;
}

}  // namespace

namespace mww {

int enqueue_grad_assembly(mww_ctx* c, int B, GradReduceArgs& ga, bool fuse_adam, int64_t lo, int64_t hi, bool last_range) {
  if (hi < 0) hi = c->P;
  int rcj = join_side(c);
  if (rcj) return rcj;
  const bool tail_here = c->tail_in_reduce && c->o_dense_w >= lo && c->o_dense_w < hi;
  if (tail_here) c->tail_in_reduce = false;
  if (!tail_here && c->o_dense_w >= lo && c->o_dense_w < hi) {
    // the dense-weight gradient came as batch-chunk rows from dense_grad_kernel / head_tail_kernel
    const int dchunk = (B + kDenseChunks - 1) / kDenseChunks;
    GradSegment s;
    s.part = c->dwd_part;
    s.G = (B + dchunk - 1) / dchunk;
    s.stride = c->dwd_stride;
    s.n = c->t_last * c->c_last + 1;
    s.dst = (int)c->o_dense_w;
    ga.seg[ga.nseg++] = s;
  }
  const bool exchange = fuse_adam && c->xch.hook && c->xch.reduce_grads;
  // single device: Adam rides in the assembly launch; data-parallel: local gradient -> sum over the ranks (the 1/W
  // factor travels as the gradient scale next to the step size, see mww_train_step) -> Adam on the average
  int rc = assemble_range(c, B, ga, lo, hi, tail_here, tail_here && c->tail_metrics, fuse_adam && !exchange);
  if (rc || !exchange) return rc;
  rc = exchange_range(c, lo, hi, last_range ? MWW_EXCHANGE_IN_ORDER : MWW_EXCHANGE_DEFERRED);
  if (!last_range) c->xch.pending = true;
  if (rc || !last_range) return rc;
  if (c->xch.pending) {
    rc = exchange_range(c, 0, 0, MWW_EXCHANGE_FLUSH);
    c->xch.pending = false;
    if (rc) return rc;
  }
  return enqueue_adam(c);
}

// first launch of the block engine's backward pass after a train step's head: BN_L's backward finalize, the dense-weight
// gradient of c->tail_src and (tail_metrics) the metric update as roles of one launch
int enqueue_head_tail(mww_ctx* c, int B, const BnBwdFinalizeArgs& fin) {
  const int dchunk = (B + kDenseChunks - 1) / kDenseChunks;
  HeadTailArgs ht;
  ht.fin = fin;
  ht.dense = dense_args(c, B, c->tail_src, c->dwd_part, c->dwd_stride);
  ht.met = MetricsArgs{c->prob, c->y_cur, c->metrics, B, c->bce_clipped ? nullptr : c->z};
  ht.n_fin = fin.C;
  ht.ndx = (ht.dense.n + 1 + kThreads - 1) / kThreads;
  ht.ndy = (B + dchunk - 1) / dchunk;
  ht.do_metrics = c->tail_metrics ? 1 : 0;
  c->metric_launches += ht.do_metrics;
  Launcher lp{c};
  lp.begin("head_tail");
  hipLaunchKernelGGL(head_tail_kernel, dim3(ht.n_fin + ht.ndx * ht.ndy + ht.do_metrics), dim3(kThreads), 0, c->stream, ht);
  lp.end();
  return MWW_OK;
}

int enqueue_adam(mww_ctx* c) {
  Launcher lp{c};
  AdamArgs a{c->params, c->grads, c->adam_m, c->adam_v, mail_hyper(c), (int)c->P, 0.9f, 0.999f, 1e-7f};
  lp.begin("adam");
  hipLaunchKernelGGL(adam_kernel, dim3(((int)c->P + kThreads - 1) / kThreads), dim3(kThreads), 0, c->stream, a);
  lp.end();
  return MWW_OK;
}

// everything enqueued so far may read the current mailbox: stamp it and move on to the next one
int mail_commit(mww_ctx* c) {
  HIPCHK(hipEventRecord(c->mail_ev[c->mail_cur], c->stream));
  c->mail_cur = (c->mail_cur + 1) % kRing;
  c->mail_open = false;
  c->targets_in_mail = 0;
  return MWW_OK;
}

// What every call that runs a forward opens with: the labels / weights written by mww_set_targets that no assembly kernel
// carried to the device, and x written out where the batch is descriptor-only but its mailbox slot is no longer the current
// one (only until then is it gathered in place)
int batch_ready(mww_ctx* c) {
  if (c->targets_in_mail > 0) {
    const char* m = c->mail_host[c->mail_cur];
    const size_t n = (size_t)c->targets_in_mail * sizeof(float);
    HIPCHK(hipMemcpyAsync(c->y, m + c->mail_off_y, n, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(c->sw, m + c->mail_off_sw, n, hipMemcpyHostToDevice, c->stream));
    c->targets_in_mail = 0;
    c->y_cur = c->y;
    c->sw_cur = c->sw;
  }
  return c->lazy_slot != c->mail_cur ? materialise_x(c) : MWW_OK;
}

void drop_graphs(mww_ctx* c) {
  for (auto& g : c->graphs) (void)hipGraphExecDestroy(g.exec);
  c->graphs.clear();
}

}  // namespace mww

namespace {

// the host may rewrite the current mailbox once the GPU work of its previous use has finished (mail_commit)
int mail_begin(mww_ctx* c) {
  if (!c->mail_open) {
    HIPCHK(hipEventSynchronize(c->mail_ev[c->mail_cur]));
    c->mail_open = true;
  }
  return MWW_OK;
}
int push_hyper(mww_ctx* c, float alpha, float gscale) {
  int rc = mail_begin(c);
  if (rc) return rc;
  float* h = reinterpret_cast<float*>(c->mail_host[c->mail_cur] + c->mail_off_hyper);
  h[0] = alpha;
  h[1] = gscale;
  return MWW_OK;
}

float adam_alpha(float lr, int64_t t) {
  // Keras: alpha = lr * sqrt(1 - beta2^t) / (1 - beta1^t), evaluated in float32 like the variables
  const float b1p = powf(0.9f, (float)t), b2p = powf(0.999f, (float)t);
  return lr * sqrtf(1.0f - b2p) / (1.0f - b1p);
}

int step_sequence(mww_ctx* c, int B, int flags, int ema) {
  c->metric_launches = 0;
  int rc;
  if (!(flags & MWW_STEP_NO_APPLY) && sharp_step(c)) {
    rc = sharp_sequence(c, B, flags, ema);
    if (rc) return rc;
  } else {
    rc = refresh_shadow(c);   // (under "graphs": one more node of the captured chain)
    if (rc) return rc;
    rc = c->model->enqueue_forward(c, B, true, true, true, !(flags & MWW_STEP_NO_METRICS));
    if (rc) return rc;
    rc = c->model->enqueue_backward(c, B, !(flags & MWW_STEP_NO_APPLY));
    if (rc) return rc;
    rc = enqueue_ema(c, ema);   // behind the last Adam launch of the step (stream order, also with two gradient buckets)
    if (rc) return rc;
  }
  // the metric state has one writer per step (kernels_head.hip.h MetricState): a second launch with the role would lose counts
  if (c->metric_launches > 1) return fail(MWW_ERR_STATE, "internal: more than one launch of this step carries the metric update");
  return MWW_OK;
}

// mask = 1 everywhere, direct flags on the BN gamma/beta slots; moving variance starts at 1
int init_defaults(mww_ctx* c, const std::vector<BnSlots>& bn) {
  std::vector<float> ones((size_t)c->P, 1.0f);
  std::vector<unsigned char> dir((size_t)c->P, 0);
  std::vector<float> st((size_t)c->S, 0.0f);
  for (const BnSlots& b : bn)
    for (int j = 0; j < b.n; ++j) {
      dir[(size_t)b.o_gamma + j] = 1;
      dir[(size_t)b.o_beta + j] = 1;
      if (b.o_mv >= 0) st[(size_t)b.o_mv + j] = 1.0f;
    }
  HIPCHK(hipMemcpy(c->mask, ones.data(), ones.size() * sizeof(float), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(c->direct, dir.data(), dir.size(), hipMemcpyHostToDevice));
  c->direct_host = dir;
  HIPCHK(hipMemcpy(c->bn_state, st.data(), st.size() * sizeof(float), hipMemcpyHostToDevice));
  return MWW_OK;
}

// buffers, mailboxes and streams that do not depend on the topology (needs P, S, t_last, c_last)
int alloc_common(mww_ctx* c) {
  const size_t mb = (size_t)c->max_batch;
  MWW_TRY(dev_alloc(&c->params, c->P));
  MWW_TRY(dev_alloc(&c->grads, c->P));
  MWW_TRY(dev_alloc(&c->adam_m, c->P));
  MWW_TRY(dev_alloc(&c->adam_v, c->P));
  MWW_TRY(dev_alloc(&c->mask, c->P));
  MWW_TRY(dev_alloc(&c->direct, c->P));
  MWW_TRY(dev_alloc(&c->bn_state, c->S));
  MWW_TRY(dev_alloc(&c->x, mb * c->frames * MWW_FEATURE_BINS));
  MWW_TRY(dev_alloc(&c->y, mb));
  MWW_TRY(dev_alloc(&c->sw, mb));
  c->y_cur = c->y;
  c->sw_cur = c->sw;
  MWW_TRY(dev_alloc(&c->z, mb));
  MWW_TRY(dev_alloc(&c->prob, mb));
  MWW_TRY(dev_alloc(&c->dz, mb));
  MWW_TRY(dev_alloc(&c->loss_part, mb));
  MWW_TRY(dev_alloc(&c->dwd_part, (size_t)kDenseChunks * c->dwd_stride));
  MWW_TRY(dev_alloc(&c->metrics, 1));
  c->mail_off_masks = mb * sizeof(mww_window);
  c->mail_off_y = c->mail_off_masks + mb * kMaxMasks * 2 * sizeof(int);
  c->mail_off_sw = c->mail_off_y + mb * sizeof(float);
  c->mail_off_hyper = c->mail_off_sw + mb * sizeof(float);
  c->mail_bytes = c->mail_off_hyper + 16;
  for (int i = 0; i < kRing; ++i) {
    HIPCHK(hipHostMalloc((void**)&c->mail_host[i], c->mail_bytes, hipHostMallocMapped));
    memset(c->mail_host[i], 0, c->mail_bytes);
    HIPCHK(hipHostGetDevicePointer((void**)&c->mail_dev[i], c->mail_host[i], 0));
    HIPCHK(hipEventCreateWithFlags(&c->mail_ev[i], hipEventDisableTiming));
  }
  HIPCHK(hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
  for (int i = 0; i < kRing; ++i) {
    MWW_TRY(dev_alloc(&c->mail_hbm[i], c->mail_bytes));
    HIPCHK(hipEventCreateWithFlags(&c->ev_copy[i], hipEventDisableTiming));
  }
  HIPCHK(hipStreamCreateWithFlags(&c->side, hipStreamNonBlocking));
  HIPCHK(hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming));
  HIPCHK(hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming));
  return MWW_OK;
}

// device / stream / launch-geometry part of context creation
int open_device(mww_ctx* c, int device, void* stream) {
  int ndev = 0;
  HIPCHK(hipGetDeviceCount(&ndev));
  if (ndev <= 0) return fail(MWW_ERR_HIP, "no HIP device visible");
  if (device < 0 || device >= ndev) return fail(MWW_ERR_INVALID, "device index out of range");
  HIPCHK(hipSetDevice(device));
  c->device = device;
  hipDeviceProp_t prop;
  HIPCHK(hipGetDeviceProperties(&prop, device));
  c->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  if (stream) {
    c->stream = (hipStream_t)stream;
  } else {
    HIPCHK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    c->own_stream = true;
  }
  c->grid_head = c->n_cu * 2;   // one window per workgroup at a time, two resident per CU (177 VGPRs): measured 13.5 us vs 15.4 (x4) / 17.4 (x1)
  return MWW_OK;
}

}  // namespace

namespace mww {

int tensor_alloc(Tensor* t, int cout, size_t rows_fwd, size_t rows_bwd, size_t grad_part) {
  MWW_TRY(dev_alloc(&t->stat_part, rows_fwd * 2 * cout));
  MWW_TRY(dev_alloc(&t->gstat_part, rows_bwd * 2 * cout));
  MWW_TRY(dev_alloc(&t->grad_part, grad_part));
  MWW_TRY(dev_alloc(&t->bn, (size_t)9 * cout));
  for (int par = 0; par < 2; ++par) {
    MWW_TRY(dev_alloc(&t->facc[par], (size_t)kStatRows * 2 * cout));
    MWW_TRY(dev_alloc(&t->gacc[par], (size_t)kStatRows * 2 * cout));
  }
  return MWW_OK;
}

void tensor_free(Tensor* t) {
  void* all[] = {t->p, t->g, t->stat_part, t->gstat_part, t->grad_part, t->bn, t->facc[0], t->facc[1], t->gacc[0], t->gacc[1]};
  for (void* p : all) if (p) (void)hipFree(p);
}

// host <-> device copies of the getters and setters: on the context's stream, waited for
int copy_in(mww_ctx* c, void* dst, const void* src, size_t bytes) {
  HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return MWW_OK;
}
int copy_out(mww_ctx* c, void* dst, const void* src, size_t bytes) {
  HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return MWW_OK;
}

int Model::set_dropout_mask(mww_ctx*, const uint8_t*, int) { return fail(MWW_ERR_INVALID, "context has no dropout layer"); }

// plan (the caller's) -> device -> layout -> the core's buffers -> the model's -> defaults
int create_context(Model* m, int frames, int max_batch, int device, void* stream, mww_ctx** out) {
  mww_ctx* c = new mww_ctx();
  c->model = m;
  c->frames = frames;
  c->max_batch = max_batch;
  std::vector<BnSlots> bn;
  int rc = open_device(c, device, stream);
  if (!rc) rc = m->layout(c);
  if (!rc) rc = alloc_common(c);
  if (!rc) rc = m->alloc(c, &bn);
  if (!rc) rc = init_defaults(c, bn);
  if (rc) { mww_destroy(c); return rc; }
  HIPCHK(hipDeviceSynchronize());
  *out = c;
  return MWW_OK;
}

}  // namespace mww

// ====================================================================================== C ABI
extern "C" {

// mww_version(): version.cpp (carries the sha256 of the source set the library was built from)
const char* mww_last_error(void) { return g_err.c_str(); }

int mww_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int mww_block_kernels_cover(const mww_mixednet_desc* desc, int bf16) {
  if (!desc) return fail(MWW_ERR_INVALID, "null descriptor");
  std::string why;
  if (shape_supported(*desc, &why, bf16 != 0)) return 1;
  g_err = why;
  return 0;
}

int mww_create(const mww_mixednet_desc* desc, int device, void* stream, mww_ctx** out) {
  if (!desc || !out) return fail(MWW_ERR_INVALID, "null argument");
  Model* m = nullptr;
  MWW_TRY(plan_mixednet(*desc, &m));
  return create_context(m, desc->frames, desc->max_batch, device, stream, out);
}

int mww_create_convnet(const mww_convnet_desc* desc, int device, void* stream, mww_ctx** out) {
  if (!desc || !out) return fail(MWW_ERR_INVALID, "null argument");
  Model* m = nullptr;
  MWW_TRY(plan_convnet(*desc, &m));
  return create_context(m, desc->frames, desc->max_batch, device, stream, out);
}

int mww_set_dropout_mask(mww_ctx* c, const uint8_t* keep, int B) {
  if (!c) return fail(MWW_ERR_INVALID, "context has no dropout layer");
  return c->model->set_dropout_mask(c, keep, B);
}

void mww_destroy(mww_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  (void)mww_allreduce_destroy(c);
  for (auto& g : c->graphs) (void)hipGraphExecDestroy(g.exec);
  for (auto& e : c->prof) { (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b); }
  void* flat[] = {c->params, c->grads, c->adam_m, c->adam_v, c->mask, c->direct, c->bn_state, c->x, c->y, c->sw,
                  c->z, c->prob, c->dz, c->loss_part, c->dwd_part, c->metrics, c->xch.sync_buf};
  for (void* p : flat) if (p) (void)hipFree(p);
  free_weight_qat(c);
  free_weight_ema(c);   // (and the statistics re-estimated for it)
  free_sharpness(c);
  for (int i = 0; i < MWW_MAX_STORES; ++i) if (c->store[i]) (void)hipFree(c->store[i]);
  if (c->copy_stream) { (void)hipStreamSynchronize(c->copy_stream); (void)hipStreamDestroy(c->copy_stream); }
  for (int i = 0; i < kRing; ++i) {
    if (c->mail_host[i]) (void)hipHostFree(c->mail_host[i]);
    if (c->mail_ev[i]) (void)hipEventDestroy(c->mail_ev[i]);
    if (c->mail_hbm[i]) (void)hipFree(c->mail_hbm[i]);
    if (c->ev_copy[i]) (void)hipEventDestroy(c->ev_copy[i]);
  }
  if (c->side) { (void)hipStreamSynchronize(c->side); (void)hipStreamDestroy(c->side); }
  if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
  if (c->ev_join) (void)hipEventDestroy(c->ev_join);
  delete c->model;   // (its own buffers)
  if (c->own_stream && c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
}

int mww_synchronize(mww_ctx* c) {
  if (!c) return fail(MWW_ERR_INVALID, "null context");
  HIPCHK(hipStreamSynchronize(c->stream));
  return MWW_OK;
}

int64_t mww_num_params(const mww_ctx* c) { return c ? c->P : 0; }
int64_t mww_num_bn_state(const mww_ctx* c) { return c ? c->S : 0; }

int mww_set_params(mww_ctx* c, const float* h, int64_t n) {
  if (!c || !h || n != c->P) return fail(MWW_ERR_INVALID, "parameter vector size mismatch");
  return copy_in(c, c->params, h, (size_t)n * sizeof(float));
}
int mww_get_params(mww_ctx* c, float* h, int64_t n) {
  if (!c || !h || n != c->P) return fail(MWW_ERR_INVALID, "parameter vector size mismatch");
  return copy_out(c, h, c->params, (size_t)n * sizeof(float));
}
int mww_set_bn_state(mww_ctx* c, const float* h, int64_t n) {
  if (!c || !h || n != c->S) return fail(MWW_ERR_INVALID, "BN state size mismatch");
  return copy_in(c, c->bn_state, h, (size_t)n * sizeof(float));
}
int mww_get_bn_state(mww_ctx* c, float* h, int64_t n) {
  if (!c || !h || n != c->S) return fail(MWW_ERR_INVALID, "BN state size mismatch");
  return copy_out(c, h, c->bn_state, (size_t)n * sizeof(float));
}
int mww_set_grad_mask(mww_ctx* c, const float* h, int64_t n) {
  if (!c || !h || n != c->P) return fail(MWW_ERR_INVALID, "mask size mismatch");
  return copy_in(c, c->mask, h, (size_t)n * sizeof(float));
}
int mww_set_opt_state(mww_ctx* c, const float* m, const float* v, int64_t n, int64_t step) {
  if (!c || !m || !v || n != c->P || step < 0) return fail(MWW_ERR_INVALID, "optimizer state size mismatch");
  int rc = copy_in(c, c->adam_m, m, (size_t)n * sizeof(float));
  if (rc) return rc;
  rc = copy_in(c, c->adam_v, v, (size_t)n * sizeof(float));
  c->step = step;
  return rc;
}
int mww_get_opt_state(mww_ctx* c, float* m, float* v, int64_t n, int64_t* step) {
  if (!c || n != c->P) return fail(MWW_ERR_INVALID, "optimizer state size mismatch");
  int rc = 0;
  if (m) rc = copy_out(c, m, c->adam_m, (size_t)n * sizeof(float));
  if (!rc && v) rc = copy_out(c, v, c->adam_v, (size_t)n * sizeof(float));
  if (step) *step = c->step;
  return rc;
}
int mww_get_grads(mww_ctx* c, float* h, int64_t n) {
  if (!c || !h || n != c->P) return fail(MWW_ERR_INVALID, "gradient vector size mismatch");
  return copy_out(c, h, c->grads, (size_t)n * sizeof(float));
}

int mww_upload_store(mww_ctx* c, int id, const void* data, int64_t n, int dtype) {
  if (!c || !data || id < 0 || id >= MWW_MAX_STORES || n <= 0) return fail(MWW_ERR_INVALID, "bad store arguments");
  if (dtype != MWW_DTYPE_U16 && dtype != MWW_DTYPE_F32) return fail(MWW_ERR_INVALID, "store dtype must be uint16 or float32");
  if (n % MWW_FEATURE_BINS) return fail(MWW_ERR_INVALID, "store length is not a multiple of 40 bins");
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (c->store[id]) { HIPCHK(hipFree(c->store[id])); c->store[id] = nullptr; }
  const size_t bytes = (size_t)n * (dtype == MWW_DTYPE_U16 ? 2 : 4);
  HIPCHK(hipMalloc(&c->store[id], bytes + 16));
  c->store_dtype[id] = dtype;
  c->store_elems[id] = n;
  return copy_in(c, c->store[id], data, bytes);
}

int mww_assemble_batch(mww_ctx* c, const mww_window* win, const int32_t* masks, int B, int ntm, int nfm) {
  if (!c || !win || B <= 0 || B > c->max_batch) return fail(MWW_ERR_INVALID, "bad batch size");
  const int nm = ntm + nfm;
  if (ntm < 0 || nfm < 0 || nm > kMaxMasks || (nm > 0 && !masks)) return fail(MWW_ERR_INVALID, "too many masks");
  const int T = c->frames;
  for (int j = 0; j < B; ++j) {
    const mww_window& w = win[j];
    if (w.store < 0 || w.store >= MWW_MAX_STORES || !c->store[w.store]) return fail(MWW_ERR_INVALID, "window refers to a store that was not uploaded");
    if (w.pad_rows < 0 || w.copy_rows < 0 || w.pad_rows + w.copy_rows != T) return fail(MWW_ERR_INVALID, "window rows do not add up to the spectrogram length");
    if (w.src_elem < 0 || w.src_elem + (int64_t)w.copy_rows * MWW_FEATURE_BINS > c->store_elems[w.store]) return fail(MWW_ERR_INVALID, "window reads past the end of its store");
  }
  HIPCHK(hipSetDevice(c->device));
  int rcm = mail_begin(c);
  if (rcm) return rcm;
  char* mh = c->mail_host[c->mail_cur];
  char* md = c->mail_hbm[c->mail_cur];
  memcpy(mh, win, (size_t)B * sizeof(mww_window));
  if (nm) memcpy(mh + c->mail_off_masks, masks, (size_t)B * nm * 2 * sizeof(int));
  HIPCHK(hipMemcpyAsync(md, mh, c->mail_off_hyper, hipMemcpyHostToDevice, c->copy_stream));
  HIPCHK(hipEventRecord(c->ev_copy[c->mail_cur], c->copy_stream));
  HIPCHK(hipStreamWaitEvent(c->stream, c->ev_copy[c->mail_cur], 0));
  AssembleArgs a;
  for (int i = 0; i < MWW_MAX_STORES; ++i) { a.store[i] = c->store[i]; a.dtype[i] = c->store_dtype[i]; }
  a.win = reinterpret_cast<const mww_window*>(md);
  a.masks = reinterpret_cast<const int*>(md + c->mail_off_masks);
  // labels / weights already in this mailbox ride along: window j's workgroup moves row j to HBM
  a.n_targets = c->targets_in_mail >= B ? B : 0;
  a.y_src = reinterpret_cast<const float*>(md + c->mail_off_y);
  a.sw_src = reinterpret_cast<const float*>(md + c->mail_off_sw);
  a.y_dst = c->y;
  a.sw_dst = c->sw;
  if (a.n_targets) c->targets_in_mail = 0;
  a.x = c->x;
  a.B = B;
  a.T = T;
  a.ntm = ntm;
  a.nfm = nfm;
  a.split = c->asm_split;
  {
    if (c->fused_input && c->model->lazy_ok(c, B) && T <= 32 * kXRowWords && nm <= kXMaxMasks) {
      // descriptor-only batch: the first block's kernels gather from the stores (the labels / weights that
      // arrived in this mailbox are read in place)
      if (a.n_targets) {
        c->y_cur = a.y_src;
        c->sw_cur = a.sw_src;
      } else {
        int rcx = bring_targets(c);   // labels of an earlier descriptor-only batch stay valid past their mailbox slot
        if (rcx) return rcx;
      }
      c->lazy_a = a;
      c->x_lazy = true;
      c->lazy_slot = c->mail_cur;
      c->have_batch = B;
      return MWW_OK;
    }
    if (a.n_targets) {   // the assembly kernel below brings this batch's labels / weights into y / sw
      c->y_cur = c->y;
      c->sw_cur = c->sw;
    } else {
      int rcx = bring_targets(c);
      if (rcx) return rcx;
    }
    c->x_lazy = false;
  }
  {
    Launcher lp{c};
    lp.begin("assemble");
    hipLaunchKernelGGL(assemble_kernel, dim3(B * a.split), dim3(kThreads), 0, c->stream, a);
    lp.end();
  }
  HIPCHK(hipGetLastError());
  c->have_batch = B;
  return MWW_OK;
}

int mww_set_batch(mww_ctx* c, const float* hx, int B) {
  if (!c || !hx || B <= 0 || B > c->max_batch) return fail(MWW_ERR_INVALID, "bad batch size");
  HIPCHK(hipSetDevice(c->device));
  int rc = bring_targets(c);
  if (rc) return rc;
  c->x_lazy = false;
  rc = copy_in(c, c->x, hx, (size_t)B * c->frames * MWW_FEATURE_BINS * sizeof(float));
  if (!rc) c->have_batch = B;
  return rc;
}
int mww_get_batch(mww_ctx* c, float* hx, int B) {
  if (!c || !hx || B <= 0 || B > c->max_batch) return fail(MWW_ERR_INVALID, "bad batch size");
  HIPCHK(hipSetDevice(c->device));
  int rc = materialise_x(c);
  if (rc) return rc;
  return copy_out(c, hx, c->x, (size_t)B * c->frames * MWW_FEATURE_BINS * sizeof(float));
}

int mww_set_targets(mww_ctx* c, const float* hy, const float* hw, int B) {
  if (!c || !hy || !hw || B <= 0 || B > c->max_batch) return fail(MWW_ERR_INVALID, "bad batch size");
  HIPCHK(hipSetDevice(c->device));
  int rc = mail_begin(c);
  if (rc) return rc;
  char* mh = c->mail_host[c->mail_cur];
  memcpy(mh + c->mail_off_y, hy, (size_t)B * sizeof(float));
  memcpy(mh + c->mail_off_sw, hw, (size_t)B * sizeof(float));
  c->targets_in_mail = B;   // picked up by the next mww_assemble_batch, or copied at the next step
  c->have_targets = B;
  return MWW_OK;
}

int mww_assemble_prefetched(mww_ctx* c, mww_prefetcher* p, float* out_labels, float* out_weights) {
  if (!c || !p) return fail(MWW_ERR_INVALID, "null context / prefetcher");
  const mww_window* win = nullptr;
  const int32_t* masks = nullptr;
  const float *y = nullptr, *w = nullptr;
  int rc = mww_prefetch_acquire(p, &win, &masks, &y, &w, nullptr, nullptr);
  if (rc) return fail(rc, "the prefetcher's sampler failed (a provider's truncation strategy cannot form a fixed-length window)");
  int B = 0, ntm = 0, nfm = 0;
  mww_prefetch_shape(p, &B, &ntm, &nfm);
  rc = mww_set_targets(c, y, w, B);
  if (!rc) rc = mww_assemble_batch(c, win, masks, B, ntm, nfm);
  if (!rc && out_labels) memcpy(out_labels, y, (size_t)B * sizeof(float));
  if (!rc && out_weights) memcpy(out_weights, w, (size_t)B * sizeof(float));
  mww_prefetch_release(p);
  return rc;
}

int mww_train_step(mww_ctx* c, int B, float lr, int flags) {
  if (!c || B <= 0 || B > c->max_batch) return fail(MWW_ERR_INVALID, "bad batch size");
  if (c->have_batch < B || c->have_targets < B) return fail(MWW_ERR_STATE, "train step needs a batch and targets of at least B rows");
  HIPCHK(hipSetDevice(c->device));
  int rc = batch_ready(c);
  if (rc) return rc;
  const bool apply = !(flags & MWW_STEP_NO_APPLY);
  if (apply) {
    c->step += 1;
    rc = push_hyper(c, adam_alpha(lr, c->step), (c->xch.hook && c->xch.reduce_grads) ? 1.0f / (float)c->xch.world : 1.0f);
    if (rc) return rc;
  }
  const int ema = apply ? ema_due(c) : EMA_NONE;
  unsigned long long counter = 0;
  const bool gen_dropout = c->model->step_counter(&counter);
  if (gen_dropout) {
    // the mask generator reads this step's counter from the mailbox (a graph node cannot carry it)
    rc = mail_begin(c);
    if (rc) return rc;
    unsigned* h = reinterpret_cast<unsigned*>(c->mail_host[c->mail_cur] + c->mail_off_hyper);
    h[2] = (unsigned)(counter & 0xFFFFFFFFull);
    h[3] = (unsigned)(counter >> 32);
  }
  // a sharpness-aware or clipped step is enqueued eagerly also under "graphs" (two walks flip the parities twice; same bytes)
  const bool sharp = apply && sharp_step(c);
  if (c->use_graphs && !c->profile && !c->xch.hook && !sharp) {   // the exchange hook enqueues foreign work: no capture
    // only the Adam / dropout nodes and the gather of a descriptor-only batch read the mailbox
    const int mail = (apply || gen_dropout || c->x_lazy) ? c->mail_cur : -1;
    // the accumulator parities of the statistics hand-over are baked into the captured kernel arguments
    bool handover = false;
    const unsigned mkey = c->model->replay_key(&handover);
    const bool flips = c->bn_inline && handover;
    const unsigned ckey = (flips ? (4 | c->fpar | (c->gpar << 1)) : 0) | (c->x_lazy ? 8 : 0) | (c->y_cur != c->y ? 16 : 0) | (c->tail_roles ? 32 : 0) | ((unsigned)ema << 6);
    hipGraphExec_t exec = nullptr;
    for (auto& g : c->graphs)
      if (g.B == B && g.flags == flags && g.mail == mail && g.core == ckey && g.model == mkey) exec = g.exec;
    if (exec && flips) {
      c->fpar ^= 1;
      c->gpar ^= 1;
    }
    if (!exec) {
      hipGraph_t graph;
      HIPCHK(hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
      rc = step_sequence(c, B, flags, ema);
      hipError_t e = hipStreamEndCapture(c->stream, &graph);
      if (rc) return rc;
      if (e != hipSuccess) return fail(MWW_ERR_HIP, std::string("hipStreamEndCapture: ") + hipGetErrorString(e));
      HIPCHK(hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0));
      HIPCHK(hipGraphDestroy(graph));
      c->graphs.push_back({B, flags, mail, ckey, mkey, exec});
    }
    HIPCHK(hipGraphLaunch(exec, c->stream));
    ema_enqueued(c, ema);
    return mail_commit(c);
  }
  rc = step_sequence(c, B, flags, ema);
  if (rc) return rc;
  HIPCHK(hipGetLastError());
  ema_enqueued(c, ema);
  return mail_commit(c);
}

int mww_apply_gradients(mww_ctx* c, float lr, float gscale) {
  if (!c) return fail(MWW_ERR_INVALID, "null context");
  HIPCHK(hipSetDevice(c->device));
  c->step += 1;
  int rc = push_hyper(c, adam_alpha(lr, c->step), gscale);
  if (rc) return rc;
  rc = enqueue_clip(c);   // the gradient as it stands in the buffer is clipped; grad_scale multiplies behind it, inside Adam
  if (rc) return rc;
  rc = enqueue_adam(c);
  if (rc) return rc;
  const int ema = ema_due(c);
  rc = enqueue_ema(c, ema);
  if (rc) return rc;
  HIPCHK(hipGetLastError());
  ema_enqueued(c, ema);
  return mail_commit(c);
}

int mww_forward(mww_ctx* c, int B, int training, int update_metrics) {
  if (!c || B <= 0 || B > c->max_batch) return fail(MWW_ERR_INVALID, "bad batch size");
  if (c->have_batch < B) return fail(MWW_ERR_STATE, "forward needs a batch of at least B rows");
  if (update_metrics && c->have_targets < B) return fail(MWW_ERR_STATE, "metric update needs targets");
  HIPCHK(hipSetDevice(c->device));
  int rc = batch_ready(c);
  if (rc) return rc;
  EmaSource source(c, training != 0);
  rc = refresh_shadow(c);
  if (rc) return rc;
  rc = c->model->enqueue_forward(c, B, training != 0, false, false, update_metrics != 0);
  if (rc) return rc;
  rc = join_side(c);
  if (rc) return rc;
  HIPCHK(hipGetLastError());
  return mail_commit(c);
}

int mww_evaluate_windows(mww_ctx* c, const mww_window* windows, const float* labels, int64_t n, int batch) {
  if (!c || !windows || !labels || n < 0 || batch <= 0 || batch > c->max_batch) return fail(MWW_ERR_INVALID, "bad evaluation arguments");
  std::vector<float> ones((size_t)batch, 1.0f);
  int rc = MWW_OK;
  for (int64_t s = 0; s < n && !rc; s += batch) {
    const int b = (int)std::min<int64_t>(batch, n - s);
    rc = mww_set_targets(c, labels + s, ones.data(), b);
    if (!rc) rc = mww_assemble_batch(c, windows + s, nullptr, b, 0, 0);
    if (!rc) rc = mww_forward(c, b, 0, 1);
    c->bn_eval_ready = c->model->eval_fold_cached();   // the weights cannot change between the batches of this call
    // ... so the first batch's shadow serves them all (the source mww_forward chose: the master, or the weight average)
    hold_shadow(c, eval_source(c));
  }
  c->bn_eval_ready = false;
  hold_shadow(c, nullptr);
  return rc;
}

int mww_read_outputs(mww_ctx* c, int B, float* probs, float* logits, float* loss) {
  if (!c || B <= 0 || B > c->max_batch) return fail(MWW_ERR_INVALID, "bad batch size");
  if (probs) HIPCHK(hipMemcpyAsync(probs, c->prob, (size_t)B * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  if (logits) HIPCHK(hipMemcpyAsync(logits, c->z, (size_t)B * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  std::vector<float> lp;
  if (loss) {
    lp.resize(B);
    HIPCHK(hipMemcpyAsync(lp.data(), c->loss_part, (size_t)B * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  }
  HIPCHK(hipStreamSynchronize(c->stream));
  if (loss) {
    double s = 0.0;
    for (int i = 0; i < B; ++i) s += lp[i];
    *loss = (float)s;
  }
  return MWW_OK;
}

int mww_metrics_read(mww_ctx* c, mww_metrics* out) {
  if (!c || !out) return fail(MWW_ERR_INVALID, "null argument");
  static_assert(sizeof(mww_metrics) == sizeof(MetricState), "metric layouts must match");
  return copy_out(c, out, c->metrics, sizeof(MetricState));
}
int mww_metrics_reset(mww_ctx* c) {
  if (!c) return fail(MWW_ERR_INVALID, "null context");
  HIPCHK(hipMemsetAsync(c->metrics, 0, sizeof(MetricState), c->stream));
  return MWW_OK;
}

void* mww_device_ptr(mww_ctx* c, int which) {
  if (!c) return nullptr;
  switch (which) {
    case MWW_BUF_PARAMS: return c->params;
    case MWW_BUF_GRADS: return c->grads;
    case MWW_BUF_BN_STATE: return c->bn_state;
    case MWW_BUF_X: return c->x;
    case MWW_HANDLE_STREAM: return c->stream;
    default: return nullptr;
  }
}

int64_t mww_debug_read(mww_ctx* c, const char* name, int B, float* host, int64_t cap) {
  if (!c || !name || !host || B <= 0 || B > c->max_batch) return fail(MWW_ERR_INVALID, "bad debug_read arguments");
  DebugTensor t;
  const int found = c->model->debug_tensor(c, name, B, &t);   // the model's tensors first: p<k>, g<k>, bn<k> and its own
  if (found < 0) return found;
  if (!found) {
    if (!strcmp(name, "dz")) { t.src = c->dz; t.n = B; }
    else if (!strcmp(name, "x")) { t.src = c->x; t.n = (int64_t)B * c->frames * MWW_FEATURE_BINS; }
    else return fail(MWW_ERR_INVALID, std::string("unknown tensor name: ") + name);
  }
  const int64_t n = t.n;
  if (n > cap) return fail(MWW_ERR_INVALID, "host buffer too small");
  if (t.planes > 1) {
    // a planar tensor is handed out interleaved [B][T][C], as the caller expects it
    const int64_t rows = n / t.cout;
    std::vector<float> tmp((size_t)rows * t.pc);
    for (int pl = 0; pl < t.planes; ++pl) {
      int rcp = copy_out(c, tmp.data(), t.src + (size_t)pl * t.pstride, tmp.size() * sizeof(float));
      if (rcp) return rcp;
      for (int64_t r = 0; r < rows; ++r)
        for (int cc = 0; cc < t.pc; ++cc) host[r * t.cout + pl * t.pc + cc] = tmp[(size_t)r * t.pc + cc];
    }
    return n;
  }
  if (t.bf16) {
    std::vector<unsigned short> half((size_t)n);
    int rch = copy_out(c, half.data(), t.src, (size_t)n * sizeof(unsigned short));
    if (rch) return rch;
    for (int64_t i = 0; i < n; ++i) {
      const unsigned bits = (unsigned)half[(size_t)i] << 16;
      memcpy(host + i, &bits, 4);
    }
    return n;
  }
  int rc = copy_out(c, host, t.src, (size_t)n * sizeof(float));
  return rc ? rc : n;
}

namespace {
// every option of mww_set_option (include/mww.h): its owner sets it; a value outside [lo, hi] (hi_cu: hi workgroups per CU) is refused
const OptionRow kOptions[] = {
    {"graphs", OPT_CORE, 1, 0, 0, nullptr},
    {"profile", OPT_CORE, 1, 0, 0, nullptr},
    {"side_stream", OPT_CORE, 1, 0, 0, nullptr},
    {"bn_inline", OPT_CORE, 1, 0, 0, nullptr},
    {"tail_roles", OPT_CORE, 1, 0, 0, nullptr},
    {"bce_from_logits", OPT_CORE, 1, 0, 0, nullptr},
    {"grad_buckets", OPT_CORE, 1, 2, 0, "grad_buckets must be 1 or 2"},
    {"fused_input", OPT_CORE, 1, 0, 0, nullptr},
    {"assemble_split", OPT_CORE, 1, 8, 0, "assemble_split out of range"},
    {"grid_head", OPT_CORE, 1, 4, 1, "grid_head out of range"},
    {"weight_qat", OPT_CORE, 0, 1, 0, "weight_qat must be 0 or 1"},
    {"ema_forward", OPT_CORE, 0, 1, 0, "ema_forward must be 0 or 1"},
    {"ablate", OPT_BLOCK, 1, 0, 0, nullptr},
    {"pointwise_bf16", OPT_BLOCK, 1, 0, 0, nullptr},
    {"storage_bf16", OPT_BLOCK, 1, 0, 0, nullptr},
    {"bwd_wide", OPT_BLOCK, 1, 0, 0, nullptr},
    {"conv1_x6", OPT_BLOCK, 1, 0, 0, nullptr},
    {"conv1_x6_fwd", OPT_BLOCK, 1, 0, 0, nullptr},
    {"bwd_first_wide", OPT_BLOCK, 1, 0, 0, nullptr},
    {"dp_commit_late", OPT_BLOCK, -1, 1, 0, "dp_commit_late must be -1 (per-family defaults), 0 or 1"},
    {"grid_fwd", OPT_BLOCK, 1, 4, 1, "grid_fwd out of range"},
    {"grid_bwd", OPT_BLOCK, 1, 2, 1, "grid_bwd out of range"},
    {"graph_role_split", OPT_GRAPH, 1, 0, 0, nullptr},
    {"graph_static_shapes", OPT_GRAPH, 1, 0, 0, nullptr},
    {"graph_planar", OPT_GRAPH, 1, 0, 0, nullptr},
    {"graph_fwd_wg_per_cu", OPT_GRAPH, 1, 8, 0, "graph_fwd_wg_per_cu must be 1..8"},
    {"graph_bwd_wg_per_cu", OPT_GRAPH, 1, 8, 0, "graph_bwd_wg_per_cu must be 1..8"},
    {"graph_frame_chunks", OPT_GRAPH, 0, 4, 0, "graph_frame_chunks must be 0..4"},
    {"graph_dgrad_share", OPT_GRAPH, 10, 90, 0, "graph_dgrad_share must be 10..90"},
    {"profile_split", OPT_GRAPH, 1, 0, 0, nullptr},
    {"grid_graph", OPT_GRAPH, 0, 4, 1, "grid_graph out of range"},   // 0: per-launch grids by occupancy (default); > 0: this many workgroups per launch
    {"dropout_seed", OPT_GRAPH, 1, 0, 0, nullptr},
};

int set_core_option(mww_ctx* c, const std::string& name, int64_t v) {
  const std::pair<const char*, bool*> flags[] = {{"graphs", &c->use_graphs}, {"profile", &c->profile}, {"side_stream", &c->use_side}, {"bn_inline", &c->bn_inline},
                                                 {"tail_roles", &c->tail_roles}, {"fused_input", &c->fused_input}};
  const std::pair<const char*, int*> ints[] = {{"grad_buckets", &c->xch.buckets}, {"assemble_split", &c->asm_split}, {"grid_head", &c->grid_head}};
  for (auto& f : flags) if (name == f.first) *f.second = v != 0;
  for (auto& f : ints) if (name == f.first) *f.second = (int)v;
  if (name == "bce_from_logits") c->bce_clipped = v == 0;
  if (name == "weight_qat") MWW_TRY(set_weight_qat_enabled(c, v != 0));
  if (name == "ema_forward") MWW_TRY(set_ema_forward(c, v != 0));
  if (name == "profile") {   // (the events recorded so far)
    for (auto& e : c->prof) { (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b); }
    c->prof.clear();
  }
  return (name == "fused_input" && !v) ? materialise_x(c) : MWW_OK;
}
}  // namespace

int mww_set_option(mww_ctx* c, const char* name, int64_t v) {
  if (!c || !name) return fail(MWW_ERR_INVALID, "null argument");
  const OptionRow* o = nullptr;
  for (const OptionRow& r : kOptions)
    if (!strcmp(name, r.name)) o = &r;
  if (!o) return fail(MWW_ERR_INVALID, std::string("unknown option: ") + name);
  if (o->lo <= o->hi && (v < o->lo || v > (o->hi_cu ? (int64_t)c->n_cu * o->hi : o->hi))) return fail(MWW_ERR_INVALID, o->range_error);
  MWW_TRY(o->owner == OPT_CORE ? set_core_option(c, name, v) : c->model->set_option(c, *o, v));
  drop_graphs(c);
  return MWW_OK;
}

int mww_profile_read(mww_ctx* c, char* names, int names_cap, float* ms, int cap) {
  if (!c) return fail(MWW_ERR_INVALID, "null context");
  HIPCHK(hipStreamSynchronize(c->stream));
  int n = 0, pos = 0;
  for (auto& e : c->prof) {
    if (n >= cap) break;
    float t = 0.f;
    (void)hipEventElapsedTime(&t, e.a, e.b);
    ms[n] = t;
    const int len = (int)e.name.size();
    if (names && pos + len + 1 < names_cap) {
      memcpy(names + pos, e.name.c_str(), len);
      names[pos + len] = '\n';
      pos += len + 1;
    }
    ++n;
  }
  if (names && names_cap > 0) names[pos < names_cap ? pos : names_cap - 1] = 0;
  for (auto& e : c->prof) { (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b); }
  c->prof.clear();
  return n;
}

}  // extern "C"

// ---- borrowed by tu_stream.hip (streaming evaluation, mww_stream_*): a stream object runs on its context's device and
// HIP stream, reads the context's resident feature stores and reports errors through the same thread-local message.
namespace mww {
int ctx_borrow(mww_ctx* c, int* device, hipStream_t* stream, void** stores, int* dtypes, int64_t* elems, int* n_cu) {
  if (!c) return fail(MWW_ERR_INVALID, "no context");
  *device = c->device;
  *stream = c->stream;
  *n_cu = c->n_cu;
  for (int i = 0; i < MWW_MAX_STORES; ++i) { stores[i] = c->store[i]; dtypes[i] = c->store_dtype[i]; elems[i] = c->store_elems[i]; }
  return MWW_OK;
}
int set_error(int code, const char* msg) { return fail(code, msg); }
}  // namespace mww
