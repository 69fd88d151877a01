// libmww_hip.so — context, device memory, the MixedNet block engine's launch sequences, gradient assembly, RCCL and the C ABI of
// include/mww.h.  The conv/BN graph engine is graph_engine.hip; engine.hip.h holds what the two share.
// One context = one device + one HIP stream + one model; every call enqueues on that stream.
#include <hip/hip_runtime.h>

#include <dlfcn.h>

#include <cmath>
#include <cstdio>
#include <climits>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "engine.hip.h"
#include "block_launch.hip.h"
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

// ---------------------------------------------------------------------------------- dispatch
// The block kernels are instantiated and launched in their own translation units (tu_fwd.hip, tu_bwd.hip, tu_bwdw.hip:
// compiled in parallel by build()); block_launch.hip.h declares their launchers and the table of specialised shapes.
int launch_fwd_first(mww_ctx* c, int k1, int c1, int cout, int k, int st, const FwdFirstArgs& a, int grid) {
  if (k_launch_fwd_first(c->stream, c->st_bf16 ? 2 : (c->pw_bf16 ? 1 : 0), k1, c1, cout, k, st, a, grid, c->conv1_x6_fwd)) return MWW_OK;
  return fail(MWW_ERR_UNSUPPORTED, "no first-block kernel for this (conv1 kernel, filters, pointwise, depthwise) shape");
}

int launch_bwd_first(mww_ctx* c, int k1, int c1, int cout, int k, int st, const BwdFirstArgs& a, int grid) {
  const bool late = c->dp_commit_late < 0 ? MWW_DP_COMMIT_LATE_FIRST_DEFAULT != 0 : c->dp_commit_late != 0;
  if (c->bwd_wide && !c->pw_bf16 && !c->st_bf16 && k_launch_bwd_firstw(c->stream, k1, c1, cout, k, st, a, grid, c->conv1_x6 && c->bwd_first_wide, late)) return MWW_OK;
  if (k_launch_bwd_first(c->stream, c->st_bf16 ? 2 : (c->pw_bf16 ? 1 : 0), k1, c1, cout, k, st, a, grid, c->conv1_x6, late)) return MWW_OK;
  return fail(MWW_ERR_UNSUPPORTED, "no first-block backward kernel for this shape");
}

int launch_fwd_block(mww_ctx* c, int cin, int cout, int k, const FwdBlockArgs& a, int grid) {
  if (k_launch_fwd_block(c->stream, c->st_bf16 ? 2 : (c->pw_bf16 ? 1 : 0), cin, cout, k, a, grid)) return MWW_OK;
  return fail(MWW_ERR_UNSUPPORTED, "no block kernel for this (cin, cout, depthwise) shape");
}

int launch_bwd_block(mww_ctx* c, int cin, int cout, int k, bool last, const BwdBlockArgs& a, int grid) {
  const int mode = c->st_bf16 ? 2 : (c->pw_bf16 ? 1 : 0);
  const bool late = c->dp_commit_late < 0 ? (last ? MWW_DP_COMMIT_LATE_LAST_DEFAULT : MWW_DP_COMMIT_LATE_BLOCK_DEFAULT) != 0 : c->dp_commit_late != 0;
  if (c->bwd_wide && k_launch_bwd_blockw(c->stream, mode, cin, cout, k, last, a, grid, late)) return MWW_OK;
  if (k_launch_bwd_block(c->stream, c->st_bf16 ? 2 : (c->pw_bf16 ? 1 : 0), cin, cout, k, last, a, grid)) return MWW_OK;
  return fail(MWW_ERR_UNSUPPORTED, "no block backward kernel for this shape");
}

constexpr int kHeadMaxRows = 24;   // frames per frame group of the widest head_kernel instantiation below
// final frames one head workgroup covers at `ch` channels (a thread keeps one float4 of every frame of its group)
int head_frame_limit(int ch) { return (kThreads / (ch / 4)) * kHeadMaxRows; }

int launch_head(mww_ctx* c, int ch, int jmax, const HeadArgs& a, int grid) {
#define X(C, J)                                                                                                \
  if (ch == C && jmax <= J) {                                                                                  \
    if (c->st_bf16)                                                                                            \
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

// does every block of the model have a specialised kernel (bf16: in the bf16 modes too)?
bool shape_supported(const mww_mixednet_desc& d, std::string* why, bool bf16 = false) {
  if (d.n_blocks < 2 || d.n_blocks > MWW_MAX_BLOCKS) { *why = "the block kernels serve 2.." + std::to_string(MWW_MAX_BLOCKS) + " blocks"; return false; }
  bool ok = false;
#define X(K1, C1, CO, K, S) ok = ok || (d.conv1_kernel == K1 && d.conv1_filters == C1 && d.block_filters[0] == CO && d.block_kernel[0] == K && d.conv1_stride == S);
  if (bf16) { MWW_FIRST_SHAPES_BF16(X) } else { MWW_FIRST_SHAPES(X) }
#undef X
  if (!ok) { *why = "first block (conv1 kernel/filters/stride, pointwise filters, depthwise kernel) not instantiated"; return false; }
  for (int i = 1; i < d.n_blocks; ++i) {
    ok = false;
#define X(CI, CO, K) ok = ok || (d.block_filters[i - 1] == CI && d.block_filters[i] == CO && d.block_kernel[i] == K);
    if (bf16) { MWW_BLOCK_SHAPES_BF16(X) } else { MWW_BLOCK_SHAPES(X) }
#undef X
    if (!ok) { *why = "block " + std::to_string(i) + " (cin, cout, depthwise kernel) not instantiated"; return false; }
  }
  const int cl = d.block_filters[d.n_blocks - 1];
  if (cl != 32 && cl != 48 && cl != 64) { *why = "head kernel needs 32, 48 or 64 channels"; return false; }
  // the classifier head keeps a window's final frames in registers: more of them than its widest instantiation holds would only
  // surface as MWW_ERR_UNSUPPORTED at the first forward (found by tools/gpu_x6_fuzz.py case 460: 64 channels x 390 frames)
  int t = d.frames >= d.conv1_kernel && d.conv1_stride > 0 ? (d.frames - d.conv1_kernel) / d.conv1_stride + 1 : 0;
  for (int i = 0; i < d.n_blocks; ++i) t -= d.block_kernel[i] - 1;
  if (t > head_frame_limit(cl)) {
    *why = "head kernel holds at most " + std::to_string(head_frame_limit(cl)) + " final frames at " + std::to_string(cl) + " channels (" + std::to_string(t) + " here)";
    return false;
  }
  return true;
}

float* bn_slot(Layer& l, int i) { return l.bn + (size_t)i * l.cout; }

}  // namespace

namespace mww {

// ---------------------------------------------------------------------------------- sequences
const float* mail_hyper(mww_ctx* c) { return reinterpret_cast<const float*>(c->mail_dev[c->mail_cur] + c->mail_off_hyper); }

// labels / weights read in place from the mailbox of a descriptor-only batch -> the y / sw buffers (before that
// mailbox slot can be rewritten)
static int bring_targets(mww_ctx* c) {
  if (c->y_cur == c->y) return MWW_OK;
  const size_t n = (size_t)c->lazy_a.B * sizeof(float);
  HIPCHK(hipMemcpyAsync(c->y, c->y_cur, n, hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(c->sw, c->sw_cur, n, hipMemcpyDeviceToDevice, c->stream));
  c->y_cur = c->y;
  c->sw_cur = c->sw;
  return MWW_OK;
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
  return MWW_OK;
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

static int join_side(mww_ctx* c) {
  if (c->side_pending) {
    HIPCHK(hipStreamWaitEvent(c->stream, c->ev_join, 0));
    c->side_pending = false;
  }
  return MWW_OK;
}

// off the critical path: metric update and (training) the dense-weight gradient run on the side
// stream while the backward chain proceeds; joined before the gradient assembly
int enqueue_side_work(mww_ctx* c, int B, bool metrics, bool loss, const float* p_last, const float* scale,
                      const float* shift, const float* keep) {
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
      const int dchunk = (B + kDenseChunks - 1) / kDenseChunks;
      const int ndchunks = (B + dchunk - 1) / dchunk;
      DenseGradArgs dg{p_last, scale, shift, c->dz, c->dwd_part, B, c->t_last * c->c_last, c->c_last, c->dwd_stride, dchunk, keep,
                       nullptr, nullptr, nullptr, 0, 0, c->st_bf16 ? 1 : 0};
      if (c->generic && !c->head2 && c->G.back().res_src >= 0) {
        GOp& rr = c->G[c->G.back().res_src];
        dg.rp = rr.p;
        dg.rscale = rr.bn + (size_t)BN_SCALE * rr.cout;
        dg.rshift = rr.bn + (size_t)BN_SHIFT * rr.cout;
        dg.rT = rr.tout;
        dg.rdrop = c->G.back().res_drop;
      }
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
  if (!(c->hook && c->sync_bn)) return MWW_OK;
  float* buf = c->sync_buf + c->sync_off[layer] + (bwd ? 2 * C : 0);
  StatCollapseArgs a{part, G, C, buf};
  lp.begin(what, layer);
  hipLaunchKernelGGL(stat_collapse_kernel, dim3(C), dim3(kThreads), 0, c->stream, a);
  lp.end();
  if (c->hook(c->hook_user, buf, 2 * C, MWW_EXCHANGE_IN_ORDER) != 0) return fail(MWW_ERR_STATE, "all-reduce hook failed");
  out->part = buf;
  out->G = 1;
  out->inv_n = local_inv_n / (float)c->world;
  out->dscale = 1.0f / (float)c->world;
  return MWW_OK;
}

}  // namespace mww

namespace {

// Workgroups of one forward block launch: its (window, time tile) items over at most the workgroups the instantiation
// keeps resident (the __launch_bounds__ of fwd_block_kernel), so that no launch runs a partial second dispatch round.
int fwd_block_grid(const mww_ctx* c, const Layer& l, int B) {
  const int per_cu = l.cin > 48 ? 2 : (l.k > 13 ? 3 : 4);
  const long long items = (long long)B * ((l.tout + TT - 1) / TT);
  return (int)std::min<long long>(items, std::min(c->grid_fwd, c->n_cu * per_cu));
}

int enqueue_forward(mww_ctx* c, int B, bool training, bool update_moving, bool loss, bool metrics) {
  if (c->generic) return g_enqueue_forward(c, B, training, update_moving, loss, metrics);
  Launcher lp{c};
  const mww_mixednet_desc& d = c->d;
  const int nb = d.n_blocks;
  if (!training && !c->bn_eval_ready) {
    for (int i = 0; i < nb; ++i) {
      Layer& l = c->L[i];
      BnEvalPrepareArgs a{c->params + l.o_gamma, c->params + l.o_beta, c->bn_state + l.o_mm, c->bn_state + l.o_mv,
                          bn_slot(l, BN_SCALE), bn_slot(l, BN_SHIFT), l.cout};
      lp.begin("bn_eval_prepare", i);
      hipLaunchKernelGGL(bn_eval_prepare_kernel, dim3(1), dim3(64), 0, c->stream, a);
      lp.end();
    }
  }
  // statistics of BN_i: accumulator rows folded by the next kernel, or partial rows + a finalize launch
  const bool inl = training && c->bn_inline && !(c->hook && c->sync_bn);
  auto fold_of = [&](Layer& pl) {
    BnFoldArgs f;
    memset(&f, 0, sizeof(f));
    if (!inl) return f;
    f.acc = pl.facc_cur;
    f.inv_n = 1.0f / ((float)B * (float)pl.tout);
    f.update_moving = update_moving ? 1 : 0;
    f.gamma = c->params + pl.o_gamma;
    f.beta = c->params + pl.o_beta;
    f.moving_mean = c->bn_state + pl.o_mm;
    f.moving_var = c->bn_state + pl.o_mv;
    f.scale = bn_slot(pl, BN_SCALE);
    f.shift = bn_slot(pl, BN_SHIFT);
    f.mean = bn_slot(pl, BN_MEAN);
    f.rstd = bn_slot(pl, BN_RSTD);
    return f;
  };
  for (int i = 0; i < nb; ++i) {
    Layer& l = c->L[i];
    const int grid = i == 0 ? std::min(B, c->grid_fwd) : fwd_block_grid(c, l, B);
    StatAcc sacc{nullptr, nullptr};
    if (inl) {
      sacc.acc = l.facc[c->fpar];
      sacc.clear = l.facc[c->fpar ^ 1];
      l.facc_cur = sacc.acc;
    }
    if (i == 0) {
      FwdFirstArgs a{c->x, c->params + c->o_conv1, c->params + l.o_dw_w, c->params + l.o_dw_b, c->params + l.o_pw_w,
                     l.p, l.stat_part, B, d.frames, l.tout, 0, sacc, x_gather(c), training ? c->a0 : nullptr};
      lp.begin("fwd_block", i);
      int rc = launch_fwd_first(c, d.conv1_kernel, d.conv1_filters, l.cout, l.k, d.conv1_stride, a, grid);
      lp.end();
      if (rc) return rc;
    } else {
      Layer& pl = c->L[i - 1];
      FwdBlockArgs a{pl.p, bn_slot(pl, BN_SCALE), bn_slot(pl, BN_SHIFT), c->params + l.o_dw_w, c->params + l.o_dw_b,
                     c->params + l.o_pw_w, l.p, l.stat_part, B, l.tin, l.tout, c->ablate, c->phase_clk + (size_t)(2 * i) * 2048 * kClkSlots,
                     sacc, fold_of(pl)};
      lp.begin("fwd_block", i);
      int rc = launch_fwd_block(c, l.cin, l.cout, l.k, a, grid);
      lp.end();
      if (rc) return rc;
    }
    if (training && !inl) {
      StatSource ss;
      int rcs = exchange_stats(c, lp, "bn_stat_exchange", i, l.stat_part, grid, l.cout, 0, 1.0f / ((float)B * (float)l.tout), &ss);
      if (rcs) return rcs;
      BnFwdFinalizeArgs f{ss.part, ss.G, l.cout, ss.inv_n, c->params + l.o_gamma,
                          c->params + l.o_beta, c->bn_state + l.o_mm, c->bn_state + l.o_mv, bn_slot(l, BN_SCALE),
                          bn_slot(l, BN_SHIFT), bn_slot(l, BN_MEAN), bn_slot(l, BN_RSTD), update_moving ? 1 : 0};
      lp.begin("bn_fwd_finalize", i);
      hipLaunchKernelGGL(bn_fwd_finalize_kernel, dim3(l.cout), dim3(kThreads), 0, c->stream, f);
      lp.end();
    }
  }
  Layer& ll = c->L[nb - 1];
  const int ghead = std::min(B, c->grid_head);
  HeadArgs h;
  h.p = ll.p;
  h.scale = bn_slot(ll, BN_SCALE);
  h.shift = bn_slot(ll, BN_SHIFT);
  h.mean = bn_slot(ll, BN_MEAN);
  h.rstd = bn_slot(ll, BN_RSTD);
  h.wd = c->params + c->o_dense_w;
  h.bd = c->params + c->o_dense_b;
  h.y = (loss || metrics) ? c->y_cur : nullptr;
  h.sw = c->sw_cur;
  h.z = c->z;
  h.prob = c->prob;
  h.dz = c->dz;
  h.loss_part = c->loss_part;
  h.gstat_part = ll.gstat_part;
  h.B = B;
  h.T = ll.tout;
  h.inv_b = 1.0f / (float)B;
  h.training = (loss ? kHeadTraining : 0) | (c->bce_clipped ? kHeadClippedLoss : 0);
  h.fold = fold_of(ll);
  if (inl) c->fpar ^= 1;
  // train step with the statistics hand-over: BN_L's backward sums go to accumulator rows (folded by the last block's
  // backward kernel) and the dense-weight gradient / metric update ride in the gradient-reduction launch
  const bool tail_late = loss && inl && c->tail_roles;
  h.gacc = StatAcc{nullptr, nullptr};
  if (tail_late) {
    h.gacc.acc = ll.gacc[c->gpar];
    h.gacc.clear = ll.gacc[c->gpar ^ 1];
    ll.gacc_cur = h.gacc.acc;
  }
  const int q = ll.cout / 4, nrg = kThreads / q;
  lp.begin("head");
  int rc = launch_head(c, ll.cout, (ll.tout + nrg - 1) / nrg, h, ghead);
  lp.end();
  if (rc) return rc;
  if (tail_late) {
    c->tail_in_reduce = true;
    c->tail_metrics = metrics;
    return MWW_OK;
  }
  if (loss && !(c->hook && c->sync_bn)) {
    // train step: the dense-weight gradient and the metric update share the launch of the last block's
    // BN-backward finalize (head_tail_kernel, first thing in enqueue_backward)
    c->tail_pending = true;
    c->tail_metrics = metrics;
    return MWW_OK;
  }
  return enqueue_side_work(c, B, metrics, loss, ll.p, bn_slot(ll, BN_SCALE), bn_slot(ll, BN_SHIFT), nullptr);
}

// gradient assembly: fixed-order sum of the per-workgroup partials (+ the dense layer's, which come
// from the side stream), structural mask, optionally fused with the Adam update
int enqueue_adam(mww_ctx* c);

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
    Layer& ll = c->L[c->d.n_blocks - 1];
    a.dense = DenseGradArgs{ll.p, bn_slot(ll, BN_SCALE), bn_slot(ll, BN_SHIFT), c->dz, nullptr, B, c->t_last * c->c_last,
                            c->c_last, 0, (B + kDenseChunks - 1) / kDenseChunks, nullptr, nullptr, nullptr, nullptr, 0, 0, c->st_bf16 ? 1 : 0};
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
  if (c->hook(c->hook_user, flags == MWW_EXCHANGE_FLUSH ? nullptr : c->grads + lo, flags == MWW_EXCHANGE_FLUSH ? 0 : hi - lo, flags) != 0)
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
  const bool exchange = fuse_adam && c->hook && c->reduce_grads;
  // single device: Adam rides in the assembly launch; data-parallel: local gradient -> sum over the ranks (the 1/W
  // factor travels as the gradient scale next to the step size, see mww_train_step) -> Adam on the average
  int rc = assemble_range(c, B, ga, lo, hi, tail_here, tail_here && c->tail_metrics, fuse_adam && !exchange);
  if (rc || !exchange) return rc;
  rc = exchange_range(c, lo, hi, last_range ? MWW_EXCHANGE_IN_ORDER : MWW_EXCHANGE_DEFERRED);
  if (!last_range) c->exchange_pending = true;
  if (rc || !last_range) return rc;
  if (c->exchange_pending) {
    rc = exchange_range(c, 0, 0, MWW_EXCHANGE_FLUSH);
    c->exchange_pending = false;
    if (rc) return rc;
  }
  return enqueue_adam(c);
}

}  // namespace mww

namespace {

// the weight-gradient partial rows of blocks [b0, b1)
void block_segments(mww_ctx* c, int gbwd, int b0, int b1, GradReduceArgs* ga) {
  memset(ga, 0, sizeof(*ga));
  for (int i = b0; i < b1; ++i) {
    Layer& l = c->L[i];
    GradSegment s;
    s.part = l.grad_part;
    s.G = gbwd;
    s.stride = l.grad_part_stride;
    s.n = l.grad_part_stride;
    s.dst = (int)(i == 0 ? c->o_conv1 : l.o_dw_w);
    ga->seg[ga->nseg++] = s;
  }
}

int enqueue_backward(mww_ctx* c, int B, bool fuse_adam) {
  if (c->generic) return g_enqueue_backward(c, B, fuse_adam);
  Launcher lp{c};
  const mww_mixednet_desc& d = c->d;
  const int nb = d.n_blocks;
  const int gbwd = std::min(B, c->grid_bwd);
  const int ghead = std::min(B, c->grid_head);
  const bool inl = c->bn_inline && !(c->hook && c->sync_bn);
  // data-parallel step: the gradient of [blocks >= split, dense] (a contiguous tail of the flat vector) is final once
  // block `split`'s backward kernel is enqueued; it is assembled and handed to the exchange hook there, so that the
  // all-reduce runs next to the remaining backward kernels.  Needs the statistics hand-over (the BN
  // gamma / beta gradients of a block are then written by that block's own backward kernel).
  const int split = nb >= 3 ? nb - 2 : 0;
  const bool bucketed = fuse_adam && c->hook && c->reduce_grads && !c->sync_bn && inl && c->tail_in_reduce && c->grad_buckets == 2 && split > 0;
  for (int i = nb - 1; i >= 0; --i) {
    Layer& l = c->L[i];
    const bool last = (i == nb - 1);
    // BN_i's backward sums: the last block's come from the head kernel's partial rows (folded by head_tail);
    // the others arrive in accumulator rows and are folded by this block's backward kernel
    const bool fold_here = inl && (!last || c->tail_in_reduce);
    StatSource ss{nullptr, 0, 0.f, 1.0f};
    if (!fold_here) {
      int rcs = exchange_stats(c, lp, "bn_gstat_exchange", i, l.gstat_part, last ? ghead : gbwd, l.cout, 1,
                               1.0f / ((float)B * (float)l.tout), &ss);
      if (rcs) return rcs;
    }
    BnBwdFinalizeArgs f{ss.part, ss.G, l.cout, ss.inv_n,
                        c->params + l.o_gamma, bn_slot(l, BN_RSTD), bn_slot(l, BN_C1), bn_slot(l, BN_MG),
                        bn_slot(l, BN_MGX), c->grads + l.o_gamma, c->grads + l.o_beta, ss.dscale};
    BnGradFoldArgs gf;
    memset(&gf, 0, sizeof(gf));
    if (fold_here) {
      gf.acc = l.gacc_cur;
      gf.inv_n = 1.0f / ((float)B * (float)l.tout);
      gf.dscale = 1.0f;
      gf.gamma = c->params + l.o_gamma;
      gf.c1 = bn_slot(l, BN_C1);
      gf.mg = bn_slot(l, BN_MG);
      gf.mgx = bn_slot(l, BN_MGX);
      gf.dgamma = c->grads + l.o_gamma;
      gf.dbeta = c->grads + l.o_beta;
    }
    if (fold_here) {
      // no launch
    } else if (last && c->tail_pending) {
      c->tail_pending = false;
      const int dchunk = (B + kDenseChunks - 1) / kDenseChunks;
      HeadTailArgs ht;
      ht.fin = f;
      ht.dense = DenseGradArgs{l.p, bn_slot(l, BN_SCALE), bn_slot(l, BN_SHIFT), c->dz, c->dwd_part, B, c->t_last * c->c_last,
                               c->c_last, c->dwd_stride, dchunk, nullptr, nullptr, nullptr, nullptr, 0, 0, c->st_bf16 ? 1 : 0};
      ht.met = MetricsArgs{c->prob, c->y_cur, c->metrics, B, c->bce_clipped ? nullptr : c->z};
      ht.n_fin = l.cout;
      ht.ndx = (ht.dense.n + 1 + kThreads - 1) / kThreads;
      ht.ndy = (B + dchunk - 1) / dchunk;
      ht.do_metrics = c->tail_metrics ? 1 : 0;
      c->metric_launches += ht.do_metrics;
      lp.begin("head_tail");
      hipLaunchKernelGGL(head_tail_kernel, dim3(ht.n_fin + ht.ndx * ht.ndy + ht.do_metrics), dim3(kThreads), 0, c->stream, ht);
      lp.end();
    } else {
      lp.begin("bn_bwd_finalize", i);
      hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3(l.cout), dim3(kThreads), 0, c->stream, f);
      lp.end();
    }
    if (i > 0) {
      Layer& pl = c->L[i - 1];
      BwdBlockArgs a;
      a.in = pl.p;
      a.in_scale = bn_slot(pl, BN_SCALE);
      a.in_shift = bn_slot(pl, BN_SHIFT);
      a.in_mean = bn_slot(pl, BN_MEAN);
      a.in_rstd = bn_slot(pl, BN_RSTD);
      a.pk = l.p;
      a.gk = l.g;
      a.k_mean = bn_slot(l, BN_MEAN);
      a.k_rstd = bn_slot(l, BN_RSTD);
      a.k_c1 = bn_slot(l, BN_C1);
      a.k_mg = bn_slot(l, BN_MG);
      a.k_mgx = bn_slot(l, BN_MGX);
      a.k_scale = bn_slot(l, BN_SCALE);
      a.k_shift = bn_slot(l, BN_SHIFT);
      a.wd = c->params + c->o_dense_w;
      a.dz = c->dz;
      a.dw_w = c->params + l.o_dw_w;
      a.dw_b = c->params + l.o_dw_b;
      a.pw_w = c->params + l.o_pw_w;
      a.g_out = pl.g;
      a.gstat_part = pl.gstat_part;
      a.grad_part = l.grad_part;
      a.B = B;
      a.Tin = l.tin;
      a.Tout = l.tout;
      a.ablate = c->ablate;
      a.phase_clk = c->phase_clk + (size_t)(2 * i + 1) * 2048 * kClkSlots;
      a.gacc = StatAcc{nullptr, nullptr};
      if (inl) {
        a.gacc.acc = pl.gacc[c->gpar];
        a.gacc.clear = pl.gacc[c->gpar ^ 1];
        pl.gacc_cur = a.gacc.acc;
      }
      a.gfold = gf;
      lp.begin("bwd_block", i);
      int rc = launch_bwd_block(c, l.cin, l.cout, l.k, last, a, gbwd);
      lp.end();
      if (rc) return rc;
      if (bucketed && i == split) {
        GradReduceArgs gb;
        block_segments(c, gbwd, split, nb, &gb);
        rc = enqueue_grad_assembly(c, B, gb, fuse_adam, l.o_dw_w, c->P, false);
        if (rc) return rc;
      }
    } else {
      if (last) return fail(MWW_ERR_UNSUPPORTED, "single-block models are not supported");
      BwdFirstArgs a{c->x, c->a0, l.p, l.g, bn_slot(l, BN_MEAN), bn_slot(l, BN_RSTD), bn_slot(l, BN_C1),
                     bn_slot(l, BN_MG), bn_slot(l, BN_MGX), c->params + l.o_dw_w, c->params + l.o_dw_b,
                     c->params + l.o_pw_w, l.grad_part, B, d.frames, l.tout, gf, x_gather(c), c->ablate,
                     c->phase_clk + (size_t)(2 * i + 1) * 2048 * kClkSlots};
      lp.begin("bwd_block", i);
      int rc = launch_bwd_first(c, d.conv1_kernel, d.conv1_filters, l.cout, l.k, d.conv1_stride, a, gbwd);
      lp.end();
      if (rc) return rc;
    }
  }
  if (inl) c->gpar ^= 1;
  GradReduceArgs ga;
  block_segments(c, gbwd, 0, bucketed ? split : nb, &ga);
  return enqueue_grad_assembly(c, B, ga, fuse_adam, 0, bucketed ? c->L[split].o_dw_w : c->P, true);
}

int enqueue_adam(mww_ctx* c) {
  Launcher lp{c};
  AdamArgs a{c->params, c->grads, c->adam_m, c->adam_v, mail_hyper(c), (int)c->P, 0.9f, 0.999f, 1e-7f};
  lp.begin("adam");
  hipLaunchKernelGGL(adam_kernel, dim3(((int)c->P + kThreads - 1) / kThreads), dim3(kThreads), 0, c->stream, a);
  lp.end();
  return MWW_OK;
}

// the host may rewrite the current mailbox once the GPU work of its previous use has finished
int mail_begin(mww_ctx* c) {
  if (!c->mail_open) {
    HIPCHK(hipEventSynchronize(c->mail_ev[c->mail_cur]));
    c->mail_open = true;
  }
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
int push_hyper(mww_ctx* c, float alpha, float gscale) {
  int rc = mail_begin(c);
  if (rc) return rc;
  float* h = reinterpret_cast<float*>(c->mail_host[c->mail_cur] + c->mail_off_hyper);
  h[0] = alpha;
  h[1] = gscale;
  return MWW_OK;
}
// labels / weights written by mww_set_targets that no assembly kernel carried to the device
int flush_targets(mww_ctx* c) {
  if (c->targets_in_mail > 0) {
    const char* m = c->mail_host[c->mail_cur];
    const size_t n = (size_t)c->targets_in_mail * sizeof(float);
    HIPCHK(hipMemcpyAsync(c->y, m + c->mail_off_y, n, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(c->sw, m + c->mail_off_sw, n, hipMemcpyHostToDevice, c->stream));
    c->targets_in_mail = 0;
    c->y_cur = c->y;
    c->sw_cur = c->sw;
  }
  return MWW_OK;
}

float adam_alpha(float lr, int64_t t) {
  // Keras: alpha = lr * sqrt(1 - beta2^t) / (1 - beta1^t), evaluated in float32 like the variables
  const float b1p = powf(0.9f, (float)t), b2p = powf(0.999f, (float)t);
  return lr * sqrtf(1.0f - b2p) / (1.0f - b1p);
}

int step_sequence(mww_ctx* c, int B, int flags) {
  c->metric_launches = 0;
  int rc = enqueue_forward(c, B, true, true, true, !(flags & MWW_STEP_NO_METRICS));
  if (rc) return rc;
  rc = enqueue_backward(c, B, !(flags & MWW_STEP_NO_APPLY));
  if (rc) return rc;
  // the metric state has one writer per step (kernels_head.hip.h MetricState): a second launch with the role would lose counts
  if (c->metric_launches > 1) return fail(MWW_ERR_STATE, "internal: more than one launch of this step carries the metric update");
  return MWW_OK;
}

template <typename T>
int dev_alloc(T** p, size_t n) {
  HIPCHK(hipMalloc((void**)p, std::max<size_t>(n, 1) * sizeof(T)));
  HIPCHK(hipMemset(*p, 0, std::max<size_t>(n, 1) * sizeof(T)));
  return MWW_OK;
}

struct BnSlots { int64_t o_gamma, o_beta, o_mv; int n; };

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
  const mww_mixednet_desc& d = c->d;
  const size_t mb = (size_t)d.max_batch;
  int rc = 0;
#define A(call) if ((rc = (call)) != 0) return rc;
#define H(call) if ((call) != hipSuccess) return fail(MWW_ERR_HIP, #call);
  A(dev_alloc(&c->params, c->P));
  A(dev_alloc(&c->grads, c->P));
  A(dev_alloc(&c->adam_m, c->P));
  A(dev_alloc(&c->adam_v, c->P));
  A(dev_alloc(&c->mask, c->P));
  A(dev_alloc(&c->direct, c->P));
  A(dev_alloc(&c->bn_state, c->S));
  A(dev_alloc(&c->x, mb * d.frames * MWW_FEATURE_BINS));
  A(dev_alloc(&c->y, mb));
  A(dev_alloc(&c->sw, mb));
  c->y_cur = c->y;
  c->sw_cur = c->sw;
  A(dev_alloc(&c->z, mb));
  A(dev_alloc(&c->prob, mb));
  A(dev_alloc(&c->dz, mb));
  A(dev_alloc(&c->loss_part, mb));
  A(dev_alloc(&c->dwd_part, (size_t)kDenseChunks * c->dwd_stride));
  A(dev_alloc(&c->metrics, 1));
  A(dev_alloc(&c->phase_clk, (size_t)2 * MWW_MAX_BLOCKS * 2048 * kClkSlots));
  c->mail_off_masks = mb * sizeof(mww_window);
  c->mail_off_y = c->mail_off_masks + mb * kMaxMasks * 2 * sizeof(int);
  c->mail_off_sw = c->mail_off_y + mb * sizeof(float);
  c->mail_off_hyper = c->mail_off_sw + mb * sizeof(float);
  c->mail_bytes = c->mail_off_hyper + 16;
  for (int i = 0; i < kRing; ++i) {
    H(hipHostMalloc((void**)&c->mail_host[i], c->mail_bytes, hipHostMallocMapped));
    memset(c->mail_host[i], 0, c->mail_bytes);
    H(hipHostGetDevicePointer((void**)&c->mail_dev[i], c->mail_host[i], 0));
    H(hipEventCreateWithFlags(&c->mail_ev[i], hipEventDisableTiming));
  }
  H(hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
  for (int i = 0; i < kRing; ++i) {
    A(dev_alloc(&c->mail_hbm[i], c->mail_bytes));
    H(hipEventCreateWithFlags(&c->ev_copy[i], hipEventDisableTiming));
  }
  H(hipStreamCreateWithFlags(&c->side, hipStreamNonBlocking));
  H(hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming));
  H(hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming));
#undef A
#undef H
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
  c->grid_fwd = c->n_cu * 4;
  c->grid_bwd = c->n_cu * 2;
  bool wide64 = false;
  for (int i = 0; i < c->d.n_blocks; ++i) wide64 = wide64 || c->d.block_filters[i] > 48;
  if (!c->generic && wide64) {
    // 64-wide blocks: the backward kernels fit once per CU (LDS), the forward kernels twice - grids of resident workgroups
    // only, no second dispatch round (tools/gpu_r3g.sh: notebook topology grid sweep)
    c->grid_fwd = c->n_cu * 2;
    c->grid_bwd = c->n_cu;
  }
  c->grid_head = c->n_cu * 2;   // one window per workgroup at a time, two resident per CU (177 VGPRs): measured 13.5 us vs 15.4 (x4) / 17.4 (x1)
  c->grid_g = c->n_cu * 3;   // measured on the Inception step: 3 workgroups per CU and launch (roles share them) beats 2 and 4
  return MWW_OK;
}

}  // namespace

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
  const mww_mixednet_desc& d = *desc;
  if (d.n_blocks < 2 || d.n_blocks > MWW_MAX_BLOCKS) return fail(MWW_ERR_INVALID, "n_blocks must be in [2, 8]");
  if (d.conv1_stride < 1 || d.frames < d.conv1_kernel) return fail(MWW_ERR_INVALID, "bad first-conv stride / kernel");
  if (d.conv1_filters <= 0) return fail(MWW_ERR_UNSUPPORTED, "first_conv_filters == 0 is not implemented");
  if (d.max_batch <= 0 || d.frames <= 0) return fail(MWW_ERR_INVALID, "frames and max_batch must be positive");
  std::string why;
  if (!shape_supported(d, &why)) return fail(MWW_ERR_UNSUPPORTED, why);
  mww_ctx* c = new mww_ctx();
  c->d = d;
  {
    int rco = open_device(c, device, stream);
    if (rco) { delete c; return rco; }
  }
  // ---- parameter layout
  int64_t off = 0, soff = 0;
  c->o_conv1 = off;
  off += (int64_t)d.conv1_kernel * MWW_FEATURE_BINS * d.conv1_filters;
  int t = (d.frames - d.conv1_kernel) / d.conv1_stride + 1, ch = d.conv1_filters;
  c->L.resize(d.n_blocks);
  for (int i = 0; i < d.n_blocks; ++i) {
    Layer& l = c->L[i];
    l.cin = ch;
    l.cout = d.block_filters[i];
    l.k = d.block_kernel[i];
    l.tin = t;
    l.tout = t - (l.k - 1);
    if (l.tout <= 0) { mww_destroy(c); return fail(MWW_ERR_INVALID, "spectrogram too short for the kernel sizes"); }
    l.o_dw_w = off; off += (int64_t)l.k * l.cin;
    l.o_dw_b = off; off += l.cin;
    l.o_pw_w = off; off += (int64_t)l.cin * l.cout;
    l.o_gamma = off; off += l.cout;
    l.o_beta = off; off += l.cout;
    l.o_mm = soff; soff += l.cout;
    l.o_mv = soff; soff += l.cout;
    t = l.tout;
    ch = l.cout;
  }
  c->t_last = t;
  c->c_last = ch;
  c->o_dense_w = off; off += (int64_t)t * ch;
  c->o_dense_b = off; off += 1;
  c->P = off;
  c->S = soff;
  c->dwd_stride = t * ch + 4;
  const size_t mb = (size_t)d.max_batch;
  // partial rows are sized for the largest grids the "grid_fwd" / "grid_bwd" / "grid_head" options accept, not for this
  // topology's defaults (until round 3 a 64-wide context - defaults 2 / 1 workgroups per CU - overran them when the options
  // asked for more: found by the shape fuzz on the emulator)
  const int gmax_f = c->n_cu * 4, gmax_b = c->n_cu * 2;
  int rc = 0;
#define A(call) if ((rc = (call)) != 0) { mww_destroy(c); return rc; }
  A(alloc_common(c));
  A(dev_alloc(&c->a0, mb * c->L[0].tin * d.conv1_filters));
#ifndef MWW_G_PINGPONG
#define MWW_G_PINGPONG 1
#endif
  // g_k (the gradient at block k's BN output) is written by the backward launch of block k+1 and read by block k's, once: two
  // buffers taken in turn hold them all (35 MB each at the headline batch instead of one per block - address space the
  // memory-side cache does not have to give up activations for)
  if (MWW_G_PINGPONG) {
    size_t need[2] = {0, 0};
    for (int i = 0; i < d.n_blocks; ++i) need[i & 1] = std::max(need[i & 1], mb * c->L[i].tout * c->L[i].cout);
    for (int par = 0; par < 2; ++par)
      if (need[par]) A(dev_alloc(&c->gbuf[par], need[par]));
  }
  for (int i = 0; i < d.n_blocks; ++i) {
    Layer& l = c->L[i];
    A(dev_alloc(&l.p, mb * l.tout * l.cout));
    if (MWW_G_PINGPONG) l.g = c->gbuf[i & 1];
    else A(dev_alloc(&l.g, mb * l.tout * l.cout));
    A(dev_alloc(&l.stat_part, (size_t)gmax_f * 2 * l.cout));
    A(dev_alloc(&l.gstat_part, (size_t)std::max(gmax_b, c->n_cu * 4) * 2 * l.cout));
    for (int par = 0; par < 2; ++par) {
      A(dev_alloc(&l.facc[par], (size_t)kStatRows * 2 * l.cout));
      A(dev_alloc(&l.gacc[par], (size_t)kStatRows * 2 * l.cout));
    }
    l.grad_part_stride = (l.k + 1) * l.cin + l.cin * l.cout;
    if (i == 0) l.grad_part_stride += d.conv1_kernel * MWW_FEATURE_BINS * d.conv1_filters;
    A(dev_alloc(&l.grad_part, (size_t)gmax_b * l.grad_part_stride));
    A(dev_alloc(&l.bn, (size_t)9 * l.cout));
  }
  {
    std::vector<BnSlots> bn;
    for (int i = 0; i < d.n_blocks; ++i) bn.push_back(BnSlots{c->L[i].o_gamma, c->L[i].o_beta, c->L[i].o_mv, c->L[i].cout});
    A(init_defaults(c, bn));
  }
#undef A
  HIPCHK(hipDeviceSynchronize());
  *out = c;
  return MWW_OK;
}

int mww_create_convnet(const mww_convnet_desc* desc, int device, void* stream, mww_ctx** out) {
  if (!desc || !out) return fail(MWW_ERR_INVALID, "null argument");
  const mww_convnet_desc& d = *desc;
  GPlan plan;
  {
    int rcp = g_plan_convnet(d, &plan);
    if (rcp) return rcp;
  }
  int64_t off = plan.P;
  const int64_t soff = plan.S;

  mww_ctx* c = new mww_ctx();
  memset(&c->d, 0, sizeof(c->d));
  c->d.frames = d.frames;
  c->d.max_batch = d.max_batch;
  c->generic = true;
  c->dropout = d.dropout;
  c->G = std::move(plan.ops);
  c->g_chunks = plan.chunks;
  c->g_inline_ok = plan.inline_ok;
  {
    int rco = open_device(c, device, stream);
    if (rco) { mww_destroy(c); return rco; }
  }
  GOp& lo = c->G.back();
  c->t_last = lo.tout;
  c->c_last = lo.cout;
  if (lo.tout > 1 && (d.head_attention || d.head_pool)) {   // mixednet.py:362: only if more than one frame remains
    if (d.head_pool < 0 || d.head_pool > 2) { mww_destroy(c); return fail(MWW_ERR_INVALID, "head_pool must be 0, 1 or 2"); }
    if (d.head_attention && lo.tout < 4) { mww_destroy(c); return fail(MWW_ERR_INVALID, "spatial attention needs at least 4 frames"); }
    if (d.dropout > 0.f) { mww_destroy(c); return fail(MWW_ERR_UNSUPPORTED, "dropout with the attention / pooled head"); }
    c->head2 = true;
    c->head_att = d.head_attention != 0;
    c->head_pool = d.head_pool;
    const int to = lo.tout - (c->head_att ? 3 : 0);
    c->t_last = c->head_pool ? 1 : to;
    if (c->head_att) { c->o_att = off; off += 8; }
    c->lds_head2 = ((size_t)lo.tout * (lo.cout | 1) + 7 * (size_t)lo.tout + 3 * (size_t)lo.cout) * sizeof(float);
    if (c->lds_head2 > kMaxDynLds) { mww_destroy(c); return fail(MWW_ERR_UNSUPPORTED, "window does not fit the head's LDS tile"); }
  }
  c->o_dense_w = off; off += (int64_t)c->t_last * lo.cout;
  c->o_dense_b = off; off += 1;
  c->P = off;
  c->S = soff;
  c->dwd_stride = c->t_last * lo.cout + 4;
  const size_t mb = (size_t)d.max_batch;
  const int gmax = c->n_cu * 4;
  int rc = 0;
#define A(call) if ((rc = (call)) != 0) { mww_destroy(c); return rc; }
  A(alloc_common(c));
  A(dev_alloc(&c->keep, mb * lo.tout * lo.cout));
  if (c->head2) {
    A(dev_alloc(&c->hact, mb * c->t_last * lo.cout));
    A(dev_alloc(&c->watt_part, (size_t)gmax * 8));
  }
  std::vector<BnSlots> bn;
  for (GOp& o : c->G) {
    A(dev_alloc(&o.p, mb * o.tout * o.cout + (size_t)o.planes * kPlanePad));
    A(dev_alloc(&o.g, mb * o.tout * o.cout + (size_t)o.planes * kPlanePad));
    A(dev_alloc(&o.stat_part, (size_t)gmax * 2 * o.cout));
    A(dev_alloc(&o.gstat_part, (size_t)gmax * 2 * o.cout));
    A(dev_alloc(&o.grad_part, (size_t)gmax * o.k * (o.kind == MWW_OP_DEPTHWISE ? 1 : o.cin) * o.cout));   // ("grid_graph" may be raised to gmax)
    A(dev_alloc(&o.bn, (size_t)9 * o.cout));
    for (int par = 0; par < 2; ++par) {
      A(dev_alloc(&o.facc[par], (size_t)kStatRows * 2 * o.cout));
      A(dev_alloc(&o.gacc[par], (size_t)kStatRows * 2 * o.cout));
    }
    if (o.norm == MWW_NORM_BN) bn.push_back(BnSlots{o.o_gamma, o.o_beta, o.o_mv, o.slots});
    else if (o.norm == MWW_NORM_BIAS) bn.push_back(BnSlots{o.o_beta, o.o_beta, -1, o.cout});   // bias gradient is written directly too
  }
  {
    A(dev_alloc(&c->ones, (size_t)kThreads));
    A(dev_alloc(&c->zeros, (size_t)kThreads));
    std::vector<float> one((size_t)kThreads, 1.0f);
    if (hipMemcpy(c->ones, one.data(), one.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) { mww_destroy(c); return fail(MWW_ERR_HIP, "hipMemcpy"); }
  }
  A(init_defaults(c, bn));
#undef A
  HIPCHK(hipDeviceSynchronize());
  *out = c;
  return MWW_OK;
}

int mww_set_allreduce_hook(mww_ctx* c, mww_allreduce_fn fn, void* user, int world_size, int sync_bn, int reduce_grads) {
  if (!c) return fail(MWW_ERR_INVALID, "null context");
  if (fn && world_size < 1) return fail(MWW_ERR_INVALID, "world size must be positive");
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipStreamSynchronize(c->stream));
  c->hook = fn;
  c->hook_user = user;
  c->world = fn ? world_size : 1;
  c->sync_bn = fn && sync_bn;
  c->reduce_grads = fn && reduce_grads;
  if (c->sync_bn && !c->sync_buf) {
    int64_t off = 0;
    c->sync_off.clear();
    if (c->generic) for (auto& o : c->G) { c->sync_off.push_back(off); off += 4 * (int64_t)o.cout; }
    else for (auto& l : c->L) { c->sync_off.push_back(off); off += 4 * (int64_t)l.cout; }
    int rc = dev_alloc(&c->sync_buf, (size_t)off);
    if (rc) return rc;
  }
  return MWW_OK;
}

// ---- RCCL inside the library (mww_allreduce_init).  The exchange the caller's hook performed through
// Python / torch.distributed (two ctypes callbacks, two dispatcher round trips and a pair of cross-stream event waits
// per step: +38 us at W = 1 for the two-bucket schedule in round 2) is issued here, from the launching thread:
//   MWW_EXCHANGE_IN_ORDER  ncclAllReduce on the context's stream itself
//   MWW_EXCHANGE_DEFERRED  event on the context's stream -> the library's side stream waits for it -> ncclAllReduce there
//   MWW_EXCHANGE_FLUSH     the context's stream waits for the side stream's last exchange
struct RcclState {
  RcclApi api;
  void* comm = nullptr;
  hipStream_t side = nullptr;
  hipEvent_t ev_ready = nullptr, ev_done = nullptr;
  mww_ctx* c = nullptr;
  bool deferred = false;
};

namespace {
int rccl_load(RcclApi* a) {
  if (a->so) return MWW_OK;
  const char* names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1", "/opt/rocm/lib/librccl.so"};
  for (const char* n : names) {
    a->so = dlopen(n, RTLD_NOW | RTLD_GLOBAL);
    if (a->so) break;
  }
  if (!a->so) return fail(MWW_ERR_UNSUPPORTED, std::string("librccl.so not found: ") + dlerror());
  a->GetUniqueId = reinterpret_cast<decltype(a->GetUniqueId)>(dlsym(a->so, "ncclGetUniqueId"));
  a->CommInitRank = reinterpret_cast<decltype(a->CommInitRank)>(dlsym(a->so, "ncclCommInitRank"));
  a->AllReduce = reinterpret_cast<decltype(a->AllReduce)>(dlsym(a->so, "ncclAllReduce"));
  a->CommDestroy = reinterpret_cast<decltype(a->CommDestroy)>(dlsym(a->so, "ncclCommDestroy"));
  a->GetErrorString = reinterpret_cast<decltype(a->GetErrorString)>(dlsym(a->so, "ncclGetErrorString"));
  a->CommCount = reinterpret_cast<decltype(a->CommCount)>(dlsym(a->so, "ncclCommCount"));
  if (!a->GetUniqueId || !a->CommInitRank || !a->AllReduce || !a->CommDestroy || !a->GetErrorString)
    return fail(MWW_ERR_UNSUPPORTED, "librccl.so lacks an entry point");
  return MWW_OK;
}

int rccl_exchange(void* user, float* buf, int64_t n, int flags) {
  RcclState* r = static_cast<RcclState*>(user);
  mww_ctx* c = r->c;
  constexpr int kFloat = 7, kSum = 0;   // ncclFloat32, ncclSum (rccl.h)
  if (flags == MWW_EXCHANGE_FLUSH) {
    if (r->deferred) {
      if (hipStreamWaitEvent(c->stream, r->ev_done, 0) != hipSuccess) return -1;
      r->deferred = false;
    }
    return 0;
  }
  hipStream_t st = c->stream;
  if (flags == MWW_EXCHANGE_DEFERRED) {
    if (hipEventRecord(r->ev_ready, c->stream) != hipSuccess) return -1;
    if (hipStreamWaitEvent(r->side, r->ev_ready, 0) != hipSuccess) return -1;
    st = r->side;
  }
  const int e = r->api.AllReduce(buf, buf, (size_t)n, kFloat, kSum, r->comm, st);
  if (e != 0) {
    g_err = std::string("ncclAllReduce: ") + r->api.GetErrorString(e);
    return -1;
  }
  if (flags == MWW_EXCHANGE_DEFERRED) {
    if (hipEventRecord(r->ev_done, r->side) != hipSuccess) return -1;
    r->deferred = true;
  }
  return 0;
}
}  // namespace

int mww_allreduce_unique_id(void* out_id, int capacity) {
  if (!out_id || capacity < MWW_UNIQUE_ID_BYTES) return fail(MWW_ERR_INVALID, "unique-id buffer too small");
  static RcclApi api;
  int rc = rccl_load(&api);
  if (rc) return rc;
  RcclApi::UniqueId id;
  const int e = api.GetUniqueId(&id);
  if (e != 0) return fail(MWW_ERR_HIP, std::string("ncclGetUniqueId: ") + api.GetErrorString(e));
  memcpy(out_id, id.internal, sizeof(id.internal));
  return MWW_OK;
}

int mww_allreduce_destroy(mww_ctx* c) {
  if (!c) return fail(MWW_ERR_INVALID, "null context");
  RcclState* r = c->rccl;
  if (!r) return MWW_OK;
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->stream);
  if (r->side) (void)hipStreamSynchronize(r->side);
  if (c->hook == rccl_exchange) {
    c->hook = nullptr;
    c->hook_user = nullptr;
    c->world = 1;
    c->sync_bn = c->reduce_grads = false;
  }
  if (r->comm) (void)r->api.CommDestroy(r->comm);
  if (r->side) (void)hipStreamDestroy(r->side);
  if (r->ev_ready) (void)hipEventDestroy(r->ev_ready);
  if (r->ev_done) (void)hipEventDestroy(r->ev_done);
  delete r;
  c->rccl = nullptr;
  return MWW_OK;
}

int mww_allreduce_world(mww_ctx* c) {
  if (!c) return fail(MWW_ERR_INVALID, "null context");
  if (!c->rccl || !c->rccl->comm) return 0;
  int n = 0;
  if (!c->rccl->api.CommCount) return fail(MWW_ERR_UNSUPPORTED, "librccl.so lacks ncclCommCount");
  const int e = c->rccl->api.CommCount(c->rccl->comm, &n);
  if (e != 0) return fail(MWW_ERR_HIP, std::string("ncclCommCount: ") + c->rccl->api.GetErrorString(e));
  return n;
}

int mww_allreduce_init(mww_ctx* c, int rank, int world, const void* unique_id, int sync_bn) {
  if (!c || !unique_id || world < 1 || rank < 0 || rank >= world) return fail(MWW_ERR_INVALID, "bad rank / world size");
  int rc = mww_allreduce_destroy(c);
  if (rc) return rc;
  HIPCHK(hipSetDevice(c->device));
  RcclState* r = new RcclState();
  r->c = c;
  rc = rccl_load(&r->api);
  if (rc) { delete r; return rc; }
  RcclApi::UniqueId id;
  memcpy(id.internal, unique_id, sizeof(id.internal));
  const int e = r->api.CommInitRank(&r->comm, world, id, rank);
  if (e != 0) {
    const std::string msg = std::string("ncclCommInitRank: ") + r->api.GetErrorString(e);
    delete r;
    return fail(MWW_ERR_HIP, msg);
  }
  c->rccl = r;
  HIPCHK(hipStreamCreateWithFlags(&r->side, hipStreamNonBlocking));
  HIPCHK(hipEventCreateWithFlags(&r->ev_ready, hipEventDisableTiming));
  HIPCHK(hipEventCreateWithFlags(&r->ev_done, hipEventDisableTiming));
  return mww_set_allreduce_hook(c, rccl_exchange, r, world, sync_bn, 1);
}

int mww_set_dropout_mask(mww_ctx* c, const uint8_t* keep, int B) {
  if (!c || !c->generic) return fail(MWW_ERR_INVALID, "context has no dropout layer");
  if (!keep) { c->keep_explicit = false; return MWW_OK; }
  if (B <= 0 || B > c->d.max_batch) return fail(MWW_ERR_INVALID, "bad batch size");
  if (!(c->dropout > 0.f)) return fail(MWW_ERR_STATE, "model was created with dropout = 0");
  const size_t n = (size_t)B * c->t_last * c->c_last;
  std::vector<float> h(n);
  const float sc = 1.0f / (1.0f - c->dropout);
  for (size_t i = 0; i < n; ++i) h[i] = keep[i] ? sc : 0.f;
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipMemcpyAsync(c->keep, h.data(), n * sizeof(float), hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  c->keep_explicit = true;
  return MWW_OK;
}

void mww_destroy(mww_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  (void)mww_allreduce_destroy(c);
  for (auto& g : c->graphs) (void)hipGraphExecDestroy(g.exec);
  for (auto& e : c->prof) { (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b); }
  void* flat[] = {c->params, c->grads, c->adam_m, c->adam_v, c->mask, c->direct, c->bn_state, c->x, c->y, c->sw,
                  c->z, c->prob, c->dz, c->loss_part, c->dwd_part, c->metrics, c->phase_clk, c->a0};
  for (void* p : flat) if (p) (void)hipFree(p);
  for (auto& l : c->L) {
    void* lp[] = {l.p, (c->gbuf[0] || c->gbuf[1]) ? nullptr : l.g, l.stat_part, l.gstat_part, l.grad_part, l.bn, l.facc[0], l.facc[1], l.gacc[0], l.gacc[1]};
    for (void* p : lp) if (p) (void)hipFree(p);
  }
  for (float* p : c->gbuf) if (p) (void)hipFree(p);
  for (auto& o : c->G) {
    void* op[] = {o.p, o.g, o.stat_part, o.gstat_part, o.grad_part, o.bn, o.facc[0], o.facc[1], o.gacc[0], o.gacc[1]};
    for (void* p : op) if (p) (void)hipFree(p);
  }
  if (c->sync_buf) (void)hipFree(c->sync_buf);
  if (c->hact) (void)hipFree(c->hact);
  if (c->watt_part) (void)hipFree(c->watt_part);
  if (c->ones) (void)hipFree(c->ones);
  if (c->zeros) (void)hipFree(c->zeros);
  if (c->keep) (void)hipFree(c->keep);
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

static int copy_in(mww_ctx* c, void* dst, const void* src, size_t bytes) {
  HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return MWW_OK;
}
static int copy_out(mww_ctx* c, void* dst, const void* src, size_t bytes) {
  HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return MWW_OK;
}

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
  if (!c || !win || B <= 0 || B > c->d.max_batch) return fail(MWW_ERR_INVALID, "bad batch size");
  const int nm = ntm + nfm;
  if (ntm < 0 || nfm < 0 || nm > kMaxMasks || (nm > 0 && !masks)) return fail(MWW_ERR_INVALID, "too many masks");
  const int T = c->d.frames;
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
    const int per_fwd = (B + std::min(B, c->grid_fwd) - 1) / std::min(B, c->grid_fwd);
    const int per_bwd = (B + std::min(B, c->grid_bwd) - 1) / std::min(B, c->grid_bwd);
    // (conv/BN graphs: the stem's launches check their own grids and write x out themselves if a workgroup would own too many windows)
    const bool lazy_ok = c->generic ? g_stem_gathers(c) : (per_fwd <= kXMaxSamples && per_bwd <= kXMaxSamples);
    if (c->fused_input && lazy_ok && T <= 32 * kXRowWords && nm <= kXMaxMasks) {
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
  if (!c || !hx || B <= 0 || B > c->d.max_batch) return fail(MWW_ERR_INVALID, "bad batch size");
  HIPCHK(hipSetDevice(c->device));
  int rc = bring_targets(c);
  if (rc) return rc;
  c->x_lazy = false;
  rc = copy_in(c, c->x, hx, (size_t)B * c->d.frames * MWW_FEATURE_BINS * sizeof(float));
  if (!rc) c->have_batch = B;
  return rc;
}
int mww_get_batch(mww_ctx* c, float* hx, int B) {
  if (!c || !hx || B <= 0 || B > c->d.max_batch) return fail(MWW_ERR_INVALID, "bad batch size");
  HIPCHK(hipSetDevice(c->device));
  int rc = materialise_x(c);
  if (rc) return rc;
  return copy_out(c, hx, c->x, (size_t)B * c->d.frames * MWW_FEATURE_BINS * sizeof(float));
}

int mww_set_targets(mww_ctx* c, const float* hy, const float* hw, int B) {
  if (!c || !hy || !hw || B <= 0 || B > c->d.max_batch) return fail(MWW_ERR_INVALID, "bad batch size");
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
  if (!c || B <= 0 || B > c->d.max_batch) return fail(MWW_ERR_INVALID, "bad batch size");
  if (c->have_batch < B || c->have_targets < B) return fail(MWW_ERR_STATE, "train step needs a batch and targets of at least B rows");
  HIPCHK(hipSetDevice(c->device));
  int rc = flush_targets(c);
  if (rc) return rc;
  if (c->lazy_slot != c->mail_cur) {   // a descriptor-only batch is gathered in place only while its mailbox slot is current
    rc = materialise_x(c);
    if (rc) return rc;
  }
  const bool apply = !(flags & MWW_STEP_NO_APPLY);
  if (apply) {
    c->step += 1;
    rc = push_hyper(c, adam_alpha(lr, c->step), (c->hook && c->reduce_grads) ? 1.0f / (float)c->world : 1.0f);
    if (rc) return rc;
  }
  const bool gen_dropout = c->generic && c->dropout > 0.f && !c->keep_explicit;
  if (gen_dropout) {
    // the mask generator reads this step's counter from the mailbox (a graph node cannot carry it)
    rc = mail_begin(c);
    if (rc) return rc;
    unsigned* h = reinterpret_cast<unsigned*>(c->mail_host[c->mail_cur] + c->mail_off_hyper);
    h[2] = (unsigned)(c->dropout_counter & 0xFFFFFFFFull);
    h[3] = (unsigned)(c->dropout_counter >> 32);
    c->dropout_counter += 1;
  }
  if (c->use_graphs && !c->profile && !c->hook) {   // the exchange hook enqueues foreign work: no capture
    // only the Adam / dropout nodes and the gather of a descriptor-only batch read the mailbox
    const int mail = (apply || gen_dropout || c->x_lazy) ? c->mail_cur : -1;
    // the accumulator parities of the statistics hand-over are baked into the captured kernel arguments
    const bool flips = c->bn_inline && (!c->generic || (c->g_inline_ok && !c->profile_split));
    const int par = (flips ? (4 | c->fpar | (c->gpar << 1)) : 0) | (c->x_lazy ? 8 : 0) | (c->y_cur != c->y ? 16 : 0) | (c->tail_roles ? 32 : 0) | (c->g_role_split ? 64 : 0) | (c->grid_g_auto ? 128 : 0) | (c->g_dgrad_share << 8) | (c->g_cap_fwd << 16) | (c->g_cap_bwd << 20) | (c->g_chunks << 24);
    hipGraphExec_t exec = nullptr;
    for (auto& g : c->graphs)
      if (g.B == B && g.flags == flags && g.mail == mail && g.par == par) exec = g.exec;
    if (exec && flips) {
      c->fpar ^= 1;
      c->gpar ^= 1;
    }
    if (!exec) {
      hipGraph_t graph;
      HIPCHK(hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
      rc = step_sequence(c, B, flags);
      hipError_t e = hipStreamEndCapture(c->stream, &graph);
      if (rc) return rc;
      if (e != hipSuccess) return fail(MWW_ERR_HIP, std::string("hipStreamEndCapture: ") + hipGetErrorString(e));
      HIPCHK(hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0));
      HIPCHK(hipGraphDestroy(graph));
      c->graphs.push_back({B, flags, mail, par, exec});
    }
    HIPCHK(hipGraphLaunch(exec, c->stream));
    return mail_commit(c);
  }
  rc = step_sequence(c, B, flags);
  if (rc) return rc;
  HIPCHK(hipGetLastError());
  return mail_commit(c);
}

int mww_apply_gradients(mww_ctx* c, float lr, float gscale) {
  if (!c) return fail(MWW_ERR_INVALID, "null context");
  HIPCHK(hipSetDevice(c->device));
  c->step += 1;
  int rc = push_hyper(c, adam_alpha(lr, c->step), gscale);
  if (rc) return rc;
  rc = enqueue_adam(c);
  if (rc) return rc;
  HIPCHK(hipGetLastError());
  return mail_commit(c);
}

int mww_forward(mww_ctx* c, int B, int training, int update_metrics) {
  if (!c || B <= 0 || B > c->d.max_batch) return fail(MWW_ERR_INVALID, "bad batch size");
  if (c->have_batch < B) return fail(MWW_ERR_STATE, "forward needs a batch of at least B rows");
  if (update_metrics && c->have_targets < B) return fail(MWW_ERR_STATE, "metric update needs targets");
  HIPCHK(hipSetDevice(c->device));
  int rc = flush_targets(c);
  if (rc) return rc;
  if (c->lazy_slot != c->mail_cur) {
    rc = materialise_x(c);
    if (rc) return rc;
  }
  rc = enqueue_forward(c, B, training != 0, false, false, update_metrics != 0);
  if (rc) return rc;
  rc = join_side(c);
  if (rc) return rc;
  HIPCHK(hipGetLastError());
  return mail_commit(c);
}

int mww_evaluate_windows(mww_ctx* c, const mww_window* windows, const float* labels, int64_t n, int batch) {
  if (!c || !windows || !labels || n < 0 || batch <= 0 || batch > c->d.max_batch) return fail(MWW_ERR_INVALID, "bad evaluation arguments");
  std::vector<float> ones((size_t)batch, 1.0f);
  int rc = MWW_OK;
  for (int64_t s = 0; s < n && !rc; s += batch) {
    const int b = (int)std::min<int64_t>(batch, n - s);
    rc = mww_set_targets(c, labels + s, ones.data(), b);
    if (!rc) rc = mww_assemble_batch(c, windows + s, nullptr, b, 0, 0);
    if (!rc) rc = mww_forward(c, b, 0, 1);
    c->bn_eval_ready = !c->generic;   // the weights cannot change between the batches of this call
  }
  c->bn_eval_ready = false;
  return rc;
}

int mww_read_outputs(mww_ctx* c, int B, float* probs, float* logits, float* loss) {
  if (!c || B <= 0 || B > c->d.max_batch) return fail(MWW_ERR_INVALID, "bad batch size");
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
  if (!c || !name || !host || B <= 0 || B > c->d.max_batch) return fail(MWW_ERR_INVALID, "bad debug_read arguments");
  const float* src = nullptr;
  int64_t n = 0;
  const int nb = c->d.n_blocks;
  auto idx = [&](const char* prefix) -> int {
    const size_t pl = strlen(prefix);
    if (strncmp(name, prefix, pl) != 0) return -1;
    const int k = atoi(name + pl);
    return (k >= 1 && k <= nb && name[pl] >= '0' && name[pl] <= '9') ? k - 1 : -1;
  };
  int k;
  if (c->generic) {
    const int no = (int)c->G.size();
    auto gidx = [&](const char* prefix) -> int {
      const size_t pl = strlen(prefix);
      if (strncmp(name, prefix, pl) != 0 || name[pl] < '0' || name[pl] > '9') return -1;
      const int kk = atoi(name + pl);
      return (kk >= 1 && kk <= no) ? kk - 1 : -1;
    };
    if ((k = gidx("p")) >= 0) { src = c->G[k].p; n = (int64_t)B * c->G[k].tout * c->G[k].cout; }
    else if ((k = gidx("g")) >= 0) { src = c->G[k].g; n = (int64_t)B * c->G[k].tout * c->G[k].cout; }
    else if ((k = gidx("bn")) >= 0) { src = c->G[k].bn; n = (int64_t)9 * c->G[k].cout; }
    else if (!strcmp(name, "dz")) { src = c->dz; n = B; }
    else if (!strcmp(name, "keep")) { src = c->keep; n = (int64_t)B * c->t_last * c->c_last; }
    else if (!strcmp(name, "x")) {
      if (materialise_x(c)) return -1;
      src = c->x;
      n = (int64_t)B * c->d.frames * MWW_FEATURE_BINS;
    }
    else return fail(MWW_ERR_INVALID, std::string("unknown tensor name: ") + name);
    if (n > cap) return fail(MWW_ERR_INVALID, "host buffer too small");
    const int kpl = gidx("p") >= 0 ? gidx("p") : gidx("g");
    if (kpl >= 0 && g_planes(c, c->G[kpl]) > 1) {
      // a planar tensor is handed out interleaved [B][T][C], as the caller expects it
      const GOp& o = c->G[kpl];
      const int planes = g_planes(c, o);
      std::vector<float> tmp((size_t)B * o.tout * o.pc);
      for (int pl = 0; pl < planes; ++pl) {
        int rcp = copy_out(c, tmp.data(), src + (size_t)pl * g_pstride(c, o), tmp.size() * sizeof(float));
        if (rcp) return rcp;
        for (int64_t r = 0; r < (int64_t)B * o.tout; ++r)
          for (int cc = 0; cc < o.pc; ++cc) host[r * o.cout + pl * o.pc + cc] = tmp[(size_t)r * o.pc + cc];
      }
      return n;
    }
    int rcg = copy_out(c, host, src, (size_t)n * sizeof(float));
    return rcg ? rcg : n;
  }
  bool stored = false;   // p_k / g_k: bf16 in HBM under "storage_bf16", widened for the caller
  if ((k = idx("p")) >= 0) { src = c->L[k].p; n = (int64_t)B * c->L[k].tout * c->L[k].cout; stored = true; }
  else if ((k = idx("g")) >= 0) { src = c->L[k].g; n = (int64_t)B * c->L[k].tout * c->L[k].cout; stored = true; }
  else if ((k = idx("bn")) >= 0) { src = c->L[k].bn; n = (int64_t)9 * c->L[k].cout; }
  else if (!strcmp(name, "dz")) { src = c->dz; n = B; }
  else if (!strcmp(name, "a0")) { src = c->a0; n = (int64_t)B * c->L[0].tin * c->d.conv1_filters; }   // relu(conv1(x)) as the first block stored it
  else if (!strncmp(name, "clkf", 4) || !strncmp(name, "clkb", 4)) {
    // phase clocks of layer k (1-based) as raw 64-bit counters viewed as floats: 2048 x kClkSlots x 2 words
    const int kk = atoi(name + 4);
    if (kk < 1 || kk > nb) return fail(MWW_ERR_INVALID, "bad layer");
    src = reinterpret_cast<const float*>(c->phase_clk + (size_t)(2 * (kk - 1) + (name[3] == 'b' ? 1 : 0)) * 2048 * kClkSlots);
    n = 2048 * kClkSlots * 2;
  }
  else if (!strcmp(name, "x")) { src = c->x; n = (int64_t)B * c->d.frames * MWW_FEATURE_BINS; }
  else return fail(MWW_ERR_INVALID, std::string("unknown tensor name: ") + name);
  if (n > cap) return fail(MWW_ERR_INVALID, "host buffer too small");
  if (stored && c->st_bf16) {
    std::vector<unsigned short> half((size_t)n);
    int rch = copy_out(c, half.data(), src, (size_t)n * sizeof(unsigned short));
    if (rch) return rch;
    for (int64_t i = 0; i < n; ++i) {
      const unsigned bits = (unsigned)half[(size_t)i] << 16;
      memcpy(host + i, &bits, 4);
    }
    return n;
  }
  int rc = copy_out(c, host, src, (size_t)n * sizeof(float));
  return rc ? rc : n;
}

int mww_set_option(mww_ctx* c, const char* name, int64_t v) {
  if (!c || !name) return fail(MWW_ERR_INVALID, "null argument");
  if (!strcmp(name, "graphs")) c->use_graphs = v != 0;
  else if (!strcmp(name, "profile")) {
    c->profile = v != 0;
    for (auto& e : c->prof) { (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b); }
    c->prof.clear();
  }
  else if (!strcmp(name, "ablate")) c->ablate = (int)v;
  else if (!strcmp(name, "side_stream")) c->use_side = v != 0;
  else if (!strcmp(name, "bn_inline")) c->bn_inline = v != 0;
  else if (!strcmp(name, "graph_role_split")) c->g_role_split = v != 0;
  else if (!strcmp(name, "graph_static_shapes")) c->g_static = v != 0;
  else if (!strcmp(name, "graph_planar")) c->g_planar = v != 0;
  else if (!strcmp(name, "graph_fwd_wg_per_cu")) { if (v < 1 || v > 8) return fail(MWW_ERR_INVALID, "graph_fwd_wg_per_cu must be 1..8"); c->g_cap_fwd = (int)v; }
  else if (!strcmp(name, "graph_bwd_wg_per_cu")) { if (v < 1 || v > 8) return fail(MWW_ERR_INVALID, "graph_bwd_wg_per_cu must be 1..8"); c->g_cap_bwd = (int)v; }
  else if (!strcmp(name, "graph_frame_chunks")) { if (v < 0 || v > 4) return fail(MWW_ERR_INVALID, "graph_frame_chunks must be 0..4"); c->g_chunks = (int)v; }
  else if (!strcmp(name, "graph_dgrad_share")) { if (v < 10 || v > 90) return fail(MWW_ERR_INVALID, "graph_dgrad_share must be 10..90"); c->g_dgrad_share = (int)v; }
  else if (!strcmp(name, "tail_roles")) c->tail_roles = v != 0;
  else if (!strcmp(name, "bce_from_logits")) c->bce_clipped = v == 0;
  else if (!strcmp(name, "grad_buckets")) { if (v < 1 || v > 2) return fail(MWW_ERR_INVALID, "grad_buckets must be 1 or 2"); c->grad_buckets = (int)v; }
  else if (!strcmp(name, "fused_input")) {
    c->fused_input = v != 0;
    if (!v) { int rc = materialise_x(c); if (rc) return rc; }
  }
  else if (!strcmp(name, "assemble_split")) { if (v < 1 || v > 8) return fail(MWW_ERR_INVALID, "assemble_split out of range"); c->asm_split = (int)v; }
  else if (!strcmp(name, "profile_split")) c->profile_split = v != 0;
  else if (!strcmp(name, "pointwise_bf16")) {
    if (c->generic && v) return fail(MWW_ERR_UNSUPPORTED, "the conv/BN graph kernels have no bf16 mode");
    { std::string why; if (v && !shape_supported(c->d, &why, true)) return fail(MWW_ERR_UNSUPPORTED, "no bf16 mode for this topology: " + why); }
    c->pw_bf16 = v != 0;
    if (!v) c->st_bf16 = false;
  }
  else if (!strcmp(name, "storage_bf16")) {
    if (c->generic && v) return fail(MWW_ERR_UNSUPPORTED, "the conv/BN graph kernels have no bf16 mode");
    { std::string why; if (v && !shape_supported(c->d, &why, true)) return fail(MWW_ERR_UNSUPPORTED, "no bf16 mode for this topology: " + why); }
    c->st_bf16 = v != 0;
    if (v) c->pw_bf16 = true;
  }
  else if (!strcmp(name, "bwd_wide")) c->bwd_wide = v != 0;
  else if (!strcmp(name, "conv1_x6")) c->conv1_x6 = v != 0;
  else if (!strcmp(name, "conv1_x6_fwd")) c->conv1_x6_fwd = v != 0;
  else if (!strcmp(name, "bwd_first_wide")) c->bwd_first_wide = v != 0;
  else if (!strcmp(name, "dp_commit_late")) { if (v < -1 || v > 1) return fail(MWW_ERR_INVALID, "dp_commit_late must be -1 (per-family defaults), 0 or 1"); c->dp_commit_late = (int)v; }
  else if (!strcmp(name, "grid_fwd")) { if (v < 1 || v > c->n_cu * 4) return fail(MWW_ERR_INVALID, "grid_fwd out of range"); c->grid_fwd = (int)v; }
  else if (!strcmp(name, "grid_bwd")) { if (v < 1 || v > c->n_cu * 2) return fail(MWW_ERR_INVALID, "grid_bwd out of range"); c->grid_bwd = (int)v; }
  else if (!strcmp(name, "grid_graph")) {   // 0: per-launch grids by occupancy (default); > 0: this many workgroups per launch
    if (v < 0 || v > c->n_cu * 4) return fail(MWW_ERR_INVALID, "grid_graph out of range");
    c->grid_g_auto = v == 0;
    if (v > 0) c->grid_g = (int)v;
  }
  else if (!strcmp(name, "dropout_seed")) { c->dropout_seed = (unsigned long long)v; c->dropout_counter = 0; }
  else if (!strcmp(name, "grid_head")) { if (v < 1 || v > c->n_cu * 4) return fail(MWW_ERR_INVALID, "grid_head out of range"); c->grid_head = (int)v; }
  else return fail(MWW_ERR_INVALID, std::string("unknown option: ") + name);
  for (auto& g : c->graphs) (void)hipGraphExecDestroy(g.exec);
  c->graphs.clear();
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
