// The MixedNet block engine of libmww_hip.so: validation and parameter layout of a mww_mixednet_desc, the dispatch into the
// specialised block kernels (instantiated and launched in tu_fwd.hip, tu_bwd*.hip, tu_bwdw.hip, tu_bwd_first.hip:
// block_launch.hip.h declares their launchers and the table of specialised shapes) and the forward / backward launch sequences.
#define MWW_BLOCK_TU 1   // the non-template kernels of the block-kernel headers are defined once, in mww_lib.hip
#include <cstring>

#include "engine.hip.h"
#include "block_launch.hip.h"
#include "kernels_bnre.hip.h"

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

// launched here, defined in mww_lib.hip (kernels_fwd.hip.h, kernels_bwd.hip.h)
__global__ void bn_fwd_finalize_kernel(BnFwdFinalizeArgs a);
__global__ void bn_eval_prepare_kernel(BnEvalPrepareArgs a);
__global__ void bn_bwd_finalize_kernel(BnBwdFinalizeArgs a);

namespace {

float* bn_slot(Layer& l, int i) { return l.bn + (size_t)i * l.cout; }
// 1 / (the elements behind one channel's statistics in a batch of B windows)
float b_inv_n(const Layer& l, int B) { return 1.0f / ((float)B * (float)l.tout); }
// statistics hand-over instead of finalize launches ("bn_inline"; sync-BN exchanges the sums in between)
bool b_handover(const mww_ctx* c) { return c->bn_inline && !(c->xch.hook && c->xch.sync_bn); }

struct BlockModel : Model {
  mww_mixednet_desc d;
  std::vector<Layer> L;
  int64_t o_conv1 = 0;
  int grid_fwd = 0, grid_bwd = 0;
  float* a0 = nullptr;     // relu(conv1(x)) [max_batch][Ta][conv1_filters]: written by the training forward, read by bwd_first_kernel
  float* gbuf[2] = {nullptr, nullptr};   // the two buffers the blocks' g_k take in turn (block k uses gbuf[k & 1])
  bool conv1_x6 = MWW_CONV1_X6_DEFAULT != 0;   // conv1 weight gradient as six bf16 slice products per fp32 product (stride-1 shapes, fp32 mode)
  bool conv1_x6_fwd = MWW_CONV1_X6_FWD_DEFAULT != 0;   // ... and the first convolution of the forward kernel
  bool bwd_first_wide = MWW_BWD_FIRST_WIDE_DEFAULT != 0;   // stride-1 first block (3-tap conv1) with conv1_x6: the 512-thread form of its backward kernel
  bool bwd_wide = MWW_BWD_WIDE_DEFAULT != 0;   // fp32 block backward kernels: 512 threads per workgroup (bwd_blockw_kernel) or 256 (bwd_block_kernel)
  int dp_commit_late = -1;   // -1: the per-family defaults above; 0 / 1: every kernel that has both orders
  bool pw_bf16 = false;   // 1x1 contractions with bf16 operands (mww_set_option "pointwise_bf16")
  bool st_bf16 = false;   // p_k / g_k stored as bf16 ("storage_bf16", implies pointwise_bf16: BASELINE configs[4])
  int ablate = 0;
  unsigned long long* phase_clk = nullptr;   // profiling: [2*layers][2048 workgroups][kClkSlots]

  ~BlockModel() override {
    for (Layer& l : L) {
      if (gbuf[0] || gbuf[1]) l.g = nullptr;   // (theirs)
      tensor_free(&l);
    }
    void* own[] = {gbuf[0], gbuf[1], a0, phase_clk};
    for (void* p : own) if (p) (void)hipFree(p);
  }
  int layout(mww_ctx* c) override;
  int alloc(mww_ctx* c, std::vector<BnSlots>* bn) override;
  int enqueue_forward(mww_ctx* c, int B, bool training, bool update_moving, bool loss, bool metrics) override;
  int enqueue_backward(mww_ctx* c, int B, bool fuse_adam) override;
  int enqueue_bn_collect(mww_ctx* c, int B) override;
  std::vector<int> stat_widths() const override {
    std::vector<int> w;
    for (const Layer& l : L) w.push_back(l.cout);
    return w;
  }
  bool lazy_ok(const mww_ctx*, int B) const override {   // the first block's kernels gather at most kXMaxSamples windows per workgroup
    const int per_fwd = (B + std::min(B, grid_fwd) - 1) / std::min(B, grid_fwd);
    const int per_bwd = (B + std::min(B, grid_bwd) - 1) / std::min(B, grid_bwd);
    return per_fwd <= kXMaxSamples && per_bwd <= kXMaxSamples;
  }
  unsigned replay_key(bool* handover) const override { *handover = true; return 0; }
  bool eval_fold_cached() const override { return true; }
  int debug_tensor(mww_ctx* c, const char* name, int B, DebugTensor* t) override;
  int set_option(mww_ctx* c, const OptionRow& o, int64_t v) override;

  int launch_fwd_first(mww_ctx* c, int k1, int c1, int cout, int k, int st, const FwdFirstArgs& a, int grid);
  int launch_bwd_first(mww_ctx* c, int k1, int c1, int cout, int k, int st, const BwdFirstArgs& a, int grid);
  int launch_fwd_block(mww_ctx* c, int cin, int cout, int k, const FwdBlockArgs& a, int grid);
  int launch_bwd_block(mww_ctx* c, int cin, int cout, int k, bool last, const BwdBlockArgs& a, int grid);
  int fwd_block_grid(const mww_ctx* c, const Layer& l, int B);
  void block_segments(int gbwd, int b0, int b1, GradReduceArgs* ga);
};

// ---------------------------------------------------------------------------------- dispatch
// The block kernels are instantiated and launched in their own translation units (tu_fwd.hip, tu_bwd.hip, tu_bwdw.hip:
// compiled in parallel by build()); block_launch.hip.h declares their launchers and the table of specialised shapes.
int BlockModel::launch_fwd_first(mww_ctx* c, int k1, int c1, int cout, int k, int st, const FwdFirstArgs& a, int grid) {
  if (k_launch_fwd_first(c->stream, st_bf16 ? 2 : (pw_bf16 ? 1 : 0), k1, c1, cout, k, st, a, grid, conv1_x6_fwd)) return MWW_OK;
  return fail(MWW_ERR_UNSUPPORTED, "no first-block kernel for this (conv1 kernel, filters, pointwise, depthwise) shape");
}

int BlockModel::launch_bwd_first(mww_ctx* c, int k1, int c1, int cout, int k, int st, const BwdFirstArgs& a, int grid) {
  const bool late = dp_commit_late < 0 ? MWW_DP_COMMIT_LATE_FIRST_DEFAULT != 0 : dp_commit_late != 0;
  if (bwd_wide && !pw_bf16 && !st_bf16 && k_launch_bwd_firstw(c->stream, k1, c1, cout, k, st, a, grid, conv1_x6 && bwd_first_wide, late)) return MWW_OK;
  if (k_launch_bwd_first(c->stream, st_bf16 ? 2 : (pw_bf16 ? 1 : 0), k1, c1, cout, k, st, a, grid, conv1_x6, late)) return MWW_OK;
  return fail(MWW_ERR_UNSUPPORTED, "no first-block backward kernel for this shape");
}

int BlockModel::launch_fwd_block(mww_ctx* c, int cin, int cout, int k, const FwdBlockArgs& a, int grid) {
  if (k_launch_fwd_block(c->stream, st_bf16 ? 2 : (pw_bf16 ? 1 : 0), cin, cout, k, a, grid)) return MWW_OK;
  return fail(MWW_ERR_UNSUPPORTED, "no block kernel for this (cin, cout, depthwise) shape");
}

int BlockModel::launch_bwd_block(mww_ctx* c, int cin, int cout, int k, bool last, const BwdBlockArgs& a, int grid) {
  const int mode = st_bf16 ? 2 : (pw_bf16 ? 1 : 0);
  const bool late = dp_commit_late < 0 ? (last ? MWW_DP_COMMIT_LATE_LAST_DEFAULT : MWW_DP_COMMIT_LATE_BLOCK_DEFAULT) != 0 : dp_commit_late != 0;
  if (bwd_wide && k_launch_bwd_blockw(c->stream, mode, cin, cout, k, last, a, grid, late)) return MWW_OK;
  if (k_launch_bwd_block(c->stream, st_bf16 ? 2 : (pw_bf16 ? 1 : 0), cin, cout, k, last, a, grid)) return MWW_OK;
  return fail(MWW_ERR_UNSUPPORTED, "no block backward kernel for this shape");
}

}  // namespace

// does every block of the model have a specialised kernel (bf16: in the bf16 modes too)?
bool shape_supported(const mww_mixednet_desc& d, std::string* why, bool bf16) {
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

namespace {

// ---------------------------------------------------------------------------------- sequences
// Workgroups of one forward block launch: its (window, time tile) items over at most the workgroups the instantiation
// keeps resident (the __launch_bounds__ of fwd_block_kernel), so that no launch runs a partial second dispatch round.
int BlockModel::fwd_block_grid(const mww_ctx* c, const Layer& l, int B) {
  const int per_cu = l.cin > 48 ? 2 : (l.k > 13 ? 3 : 4);
  const long long items = (long long)B * ((l.tout + TT - 1) / TT);
  return (int)std::min<long long>(items, std::min(grid_fwd, c->n_cu * per_cu));
}

int BlockModel::enqueue_forward(mww_ctx* c, int B, bool training, bool update_moving, bool loss, bool metrics) {
  Launcher lp{c};
  const int nb = d.n_blocks;
  if (!training && !c->bn_eval_ready) {
    for (int i = 0; i < nb; ++i) {
      Layer& l = L[i];
      BnEvalPrepareArgs a{fwd_params(c) + l.o_gamma, fwd_params(c) + l.o_beta, eval_bn_state(c) + l.o_mm, eval_bn_state(c) + l.o_mv,
                          bn_slot(l, BN_SCALE), bn_slot(l, BN_SHIFT), l.cout};
      lp.begin("bn_eval_prepare", i);
      hipLaunchKernelGGL(bn_eval_prepare_kernel, dim3(1), dim3(64), 0, c->stream, a);
      lp.end();
    }
  }
  // statistics of BN_i: accumulator rows folded by the next kernel, or partial rows + a finalize launch
  const bool inl = training && b_handover(c);
  auto fold_of = [&](Layer& pl) {
    BnFoldArgs f;
    memset(&f, 0, sizeof(f));
    if (!inl) return f;
    f.acc = fwd_rows(c, pl).acc;
    f.inv_n = b_inv_n(pl, B);
    f.update_moving = update_moving ? 1 : 0;
    f.gamma = fwd_params(c) + pl.o_gamma;
    f.beta = fwd_params(c) + pl.o_beta;
    f.moving_mean = c->bn_state + pl.o_mm;
    f.moving_var = c->bn_state + pl.o_mv;
    f.scale = bn_slot(pl, BN_SCALE);
    f.shift = bn_slot(pl, BN_SHIFT);
    f.mean = bn_slot(pl, BN_MEAN);
    f.rstd = bn_slot(pl, BN_RSTD);
    return f;
  };
  for (int i = 0; i < nb; ++i) {
    Layer& l = L[i];
    const int grid = i == 0 ? std::min(B, grid_fwd) : fwd_block_grid(c, l, B);
    const StatAcc sacc = inl ? fwd_rows(c, l) : StatAcc{nullptr, nullptr};
    if (i == 0) {
      FwdFirstArgs a{c->x, fwd_params(c) + o_conv1, fwd_params(c) + l.o_dw_w, fwd_params(c) + l.o_dw_b, fwd_params(c) + l.o_pw_w,
                     l.p, l.stat_part, B, d.frames, l.tout, 0, sacc, x_gather(c), training ? a0 : nullptr};
      lp.begin("fwd_block", i);
      int rc = launch_fwd_first(c, d.conv1_kernel, d.conv1_filters, l.cout, l.k, d.conv1_stride, a, grid);
      lp.end();
      if (rc) return rc;
    } else {
      Layer& pl = L[i - 1];
      FwdBlockArgs a{pl.p, bn_slot(pl, BN_SCALE), bn_slot(pl, BN_SHIFT), fwd_params(c) + l.o_dw_w, fwd_params(c) + l.o_dw_b,
                     fwd_params(c) + l.o_pw_w, l.p, l.stat_part, B, l.tin, l.tout, ablate, phase_clk + (size_t)(2 * i) * 2048 * kClkSlots,
                     sacc, fold_of(pl)};
      lp.begin("fwd_block", i);
      int rc = launch_fwd_block(c, l.cin, l.cout, l.k, a, grid);
      lp.end();
      if (rc) return rc;
    }
    if (training && !inl) {
      StatSource ss;
      int rcs = exchange_stats(c, lp, "bn_stat_exchange", i, l.stat_part, grid, l.cout, 0, b_inv_n(l, B), &ss);
      if (rcs) return rcs;
      BnFwdFinalizeArgs f{ss.part, ss.G, l.cout, ss.inv_n, fwd_params(c) + l.o_gamma,
                          fwd_params(c) + l.o_beta, c->bn_state + l.o_mm, c->bn_state + l.o_mv, bn_slot(l, BN_SCALE),
                          bn_slot(l, BN_SHIFT), bn_slot(l, BN_MEAN), bn_slot(l, BN_RSTD), update_moving ? 1 : 0};
      lp.begin("bn_fwd_finalize", i);
      hipLaunchKernelGGL(bn_fwd_finalize_kernel, dim3(l.cout), dim3(kThreads), 0, c->stream, f);
      lp.end();
    }
  }
  Layer& ll = L[nb - 1];
  const BnFoldArgs hfold = fold_of(ll);
  if (inl) c->fpar ^= 1;   // (behind the last reader of this walk's forward rows)
  // train step with the statistics hand-over: BN_L's backward sums go to accumulator rows (folded by the last block's
  // backward kernel) and the dense-weight gradient / metric update ride in the gradient-reduction launch
  const bool tail_late = loss && inl && c->tail_roles;
  const StatAcc hgacc = tail_late ? bwd_rows(c, ll) : StatAcc{nullptr, nullptr};
  int rc = enqueue_block_head(c, B, ll, ll.tout, ll.cout, st_bf16, hfold, hgacc, loss, metrics);
  if (rc) return rc;
  c->tail_src = DenseSource{ll.p, bn_slot(ll, BN_SCALE), bn_slot(ll, BN_SHIFT), nullptr, nullptr, nullptr, nullptr, 0, 0, st_bf16 ? 1 : 0};
  if (tail_late) {
    c->tail_in_reduce = true;
    c->tail_metrics = metrics;
    return MWW_OK;
  }
  if (loss && !(c->xch.hook && c->xch.sync_bn)) {
    // train step: the dense-weight gradient and the metric update share the launch of the last block's
    // BN-backward finalize (head_tail_kernel, first thing in enqueue_backward)
    c->tail_pending = true;
    c->tail_metrics = metrics;
    return MWW_OK;
  }
  return enqueue_side_work(c, B, metrics, loss, c->tail_src);
}

// BN re-estimation: where the training forward of B windows just enqueued left every block's sums - the accumulator rows its
// first consumer folded, or the partial rows (behind a sync-BN exchange: the row of global sums) bn_fwd_finalize_kernel read -
// with the inv_n of that fold
int BlockModel::enqueue_bn_collect(mww_ctx* c, int B) {
  const bool inl = b_handover(c);
  std::vector<BnreRow> rows(L.size());
  memset(rows.data(), 0, rows.size() * sizeof(BnreRow));
  for (size_t i = 0; i < L.size(); ++i) {
    Layer& l = L[i];
    BnreRow& r = rows[i];
    const float inv_n = b_inv_n(l, B);
    r.C = l.cout;
    r.groups = 1;
    r.o_mm = (int)l.o_mm;
    r.o_mv = (int)l.o_mv;
    if (inl) {
      r.form = BNRE_ROWS;
      r.acc[0] = l.facc[0];
      r.acc[1] = l.facc[1];
      r.inv_n = inv_n;
    } else {
      const int grid = i == 0 ? std::min(B, grid_fwd) : fwd_block_grid(c, l, B);
      const StatSource ss = forward_stat_source(c, (int)i, l.stat_part, grid, l.cout, inv_n);
      r.form = BNRE_PART_BLOCK;
      r.part = ss.part;
      r.G = ss.G;
      r.inv_n = ss.inv_n;
    }
  }
  return enqueue_bnre_collect(c, rows);
}

// the weight-gradient partial rows of blocks [b0, b1)
void BlockModel::block_segments(int gbwd, int b0, int b1, GradReduceArgs* ga) {
  memset(ga, 0, sizeof(*ga));
  for (int i = b0; i < b1; ++i) {
    Layer& l = L[i];
    GradSegment s;
    s.part = l.grad_part;
    s.G = gbwd;
    s.stride = l.grad_part_stride;
    s.n = l.grad_part_stride;
    s.dst = (int)(i == 0 ? o_conv1 : l.o_dw_w);
    ga->seg[ga->nseg++] = s;
  }
}

int BlockModel::enqueue_backward(mww_ctx* c, int B, bool fuse_adam) {
  Launcher lp{c};
  const int nb = d.n_blocks;
  const int gbwd = std::min(B, grid_bwd);
  const int ghead = std::min(B, c->grid_head);
  const bool inl = b_handover(c);
  // data-parallel step: the gradient of [blocks >= split, dense] (a contiguous tail of the flat vector) is final once
  // block `split`'s backward kernel is enqueued; it is assembled and handed to the exchange hook there, so that the
  // all-reduce runs next to the remaining backward kernels.  Needs the statistics hand-over (the BN
  // gamma / beta gradients of a block are then written by that block's own backward kernel).
  const int split = nb >= 3 ? nb - 2 : 0;
  const bool bucketed = fuse_adam && c->xch.hook && c->xch.reduce_grads && !c->xch.sync_bn && inl && c->tail_in_reduce && c->xch.buckets == 2 && split > 0;
  for (int i = nb - 1; i >= 0; --i) {
    Layer& l = L[i];
    const bool last = (i == nb - 1);
    // BN_i's backward sums: the last block's come from the head kernel's partial rows (folded by head_tail);
    // the others arrive in accumulator rows and are folded by this block's backward kernel
    const bool fold_here = inl && (!last || c->tail_in_reduce);
    StatSource ss{nullptr, 0, 0.f, 1.0f};
    if (!fold_here) {
      int rcs = exchange_stats(c, lp, "bn_gstat_exchange", i, l.gstat_part, last ? ghead : gbwd, l.cout, 1, b_inv_n(l, B), &ss);
      if (rcs) return rcs;
    }
    BnBwdFinalizeArgs f{ss.part, ss.G, l.cout, ss.inv_n,
                        fwd_params(c) + l.o_gamma, bn_slot(l, BN_RSTD), bn_slot(l, BN_C1), bn_slot(l, BN_MG),
                        bn_slot(l, BN_MGX), c->grads + l.o_gamma, c->grads + l.o_beta, ss.dscale};
    BnGradFoldArgs gf;
    memset(&gf, 0, sizeof(gf));
    if (fold_here) {
      gf.acc = bwd_rows(c, l).acc;
      gf.inv_n = b_inv_n(l, B);
      gf.dscale = 1.0f;
      gf.gamma = fwd_params(c) + l.o_gamma;
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
      int rch = enqueue_head_tail(c, B, f);
      if (rch) return rch;
    } else {
      lp.begin("bn_bwd_finalize", i);
      hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3(l.cout), dim3(kThreads), 0, c->stream, f);
      lp.end();
    }
    if (i > 0) {
      Layer& pl = L[i - 1];
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
      a.wd = fwd_params(c) + c->o_dense_w;
      a.dz = c->dz;
      a.dw_w = fwd_params(c) + l.o_dw_w;
      a.dw_b = fwd_params(c) + l.o_dw_b;
      a.pw_w = fwd_params(c) + l.o_pw_w;
      a.g_out = pl.g;
      a.gstat_part = pl.gstat_part;
      a.grad_part = l.grad_part;
      a.B = B;
      a.Tin = l.tin;
      a.Tout = l.tout;
      a.ablate = ablate;
      a.phase_clk = phase_clk + (size_t)(2 * i + 1) * 2048 * kClkSlots;
      a.gacc = inl ? bwd_rows(c, pl) : StatAcc{nullptr, nullptr};
      a.gfold = gf;
      lp.begin("bwd_block", i);
      int rc = launch_bwd_block(c, l.cin, l.cout, l.k, last, a, gbwd);
      lp.end();
      if (rc) return rc;
      if (bucketed && i == split) {
        GradReduceArgs gb;
        block_segments(gbwd, split, nb, &gb);
        rc = enqueue_grad_assembly(c, B, gb, fuse_adam, l.o_dw_w, c->P, false);
        if (rc) return rc;
      }
    } else {
      if (last) return fail(MWW_ERR_UNSUPPORTED, "single-block models are not supported");
      BwdFirstArgs a{c->x, a0, l.p, l.g, bn_slot(l, BN_MEAN), bn_slot(l, BN_RSTD), bn_slot(l, BN_C1),
                     bn_slot(l, BN_MG), bn_slot(l, BN_MGX), fwd_params(c) + l.o_dw_w, fwd_params(c) + l.o_dw_b,
                     fwd_params(c) + l.o_pw_w, l.grad_part, B, d.frames, l.tout, gf, x_gather(c), ablate,
                     phase_clk + (size_t)(2 * i + 1) * 2048 * kClkSlots};
      lp.begin("bwd_block", i);
      int rc = launch_bwd_first(c, d.conv1_kernel, d.conv1_filters, l.cout, l.k, d.conv1_stride, a, gbwd);
      lp.end();
      if (rc) return rc;
    }
  }
  if (inl) c->gpar ^= 1;
  GradReduceArgs ga;
  block_segments(gbwd, 0, bucketed ? split : nb, &ga);
  return enqueue_grad_assembly(c, B, ga, fuse_adam, 0, bucketed ? L[split].o_dw_w : c->P, true);
}

// ---------------------------------------------------------------------------------- creation, options, debug
int BlockModel::layout(mww_ctx* c) {
  int64_t off = 0, soff = 0;
  o_conv1 = off;
  off += (int64_t)d.conv1_kernel * MWW_FEATURE_BINS * d.conv1_filters;
  int t = (d.frames - d.conv1_kernel) / d.conv1_stride + 1, ch = d.conv1_filters;
  L.resize(d.n_blocks);
  for (int i = 0; i < d.n_blocks; ++i) {
    Layer& l = L[i];
    l.cin = ch;
    l.cout = d.block_filters[i];
    l.k = d.block_kernel[i];
    l.tin = t;
    l.tout = t - (l.k - 1);
    if (l.tout <= 0) return fail(MWW_ERR_INVALID, "spectrogram too short for the kernel sizes");
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
  grid_fwd = c->n_cu * 4;
  grid_bwd = c->n_cu * 2;
  bool wide64 = false;
  for (int i = 0; i < d.n_blocks; ++i) wide64 = wide64 || d.block_filters[i] > 48;
  if (wide64) {
    // 64-wide blocks: the backward kernels fit once per CU (LDS), the forward kernels twice - grids of resident workgroups
    // only, no second dispatch round (tools/gpu_r3g.sh: notebook topology grid sweep)
    grid_fwd = c->n_cu * 2;
    grid_bwd = c->n_cu;
  }
  return MWW_OK;
}

int BlockModel::alloc(mww_ctx* c, std::vector<BnSlots>* bn) {
  const size_t mb = (size_t)d.max_batch;
  // partial rows are sized for the largest grids the "grid_fwd" / "grid_bwd" / "grid_head" options accept, not for this
  // topology's defaults (until round 3 a 64-wide context - defaults 2 / 1 workgroups per CU - overran them when the options
  // asked for more: found by the shape fuzz on the emulator)
  const int gmax_f = c->n_cu * 4, gmax_b = c->n_cu * 2;
  MWW_TRY(dev_alloc(&a0, mb * L[0].tin * d.conv1_filters));
#ifndef MWW_G_PINGPONG
#define MWW_G_PINGPONG 1
#endif
  // g_k (the gradient at block k's BN output) is written by the backward launch of block k+1 and read by block k's, once: two
  // buffers taken in turn hold them all (35 MB each at the headline batch instead of one per block - address space the
  // memory-side cache does not have to give up activations for)
  if (MWW_G_PINGPONG) {
    size_t need[2] = {0, 0};
    for (int i = 0; i < d.n_blocks; ++i) need[i & 1] = std::max(need[i & 1], mb * L[i].tout * L[i].cout);
    for (int par = 0; par < 2; ++par)
      if (need[par]) MWW_TRY(dev_alloc(&gbuf[par], need[par]));
  }
  for (int i = 0; i < d.n_blocks; ++i) {
    Layer& l = L[i];
    MWW_TRY(dev_alloc(&l.p, mb * l.tout * l.cout));
    if (MWW_G_PINGPONG) l.g = gbuf[i & 1];
    else MWW_TRY(dev_alloc(&l.g, mb * l.tout * l.cout));
    l.grad_part_stride = (l.k + 1) * l.cin + l.cin * l.cout;
    if (i == 0) l.grad_part_stride += d.conv1_kernel * MWW_FEATURE_BINS * d.conv1_filters;
    MWW_TRY(tensor_alloc(&l, l.cout, gmax_f, std::max(gmax_b, c->n_cu * 4), (size_t)gmax_b * l.grad_part_stride));
    bn->push_back(BnSlots{l.o_gamma, l.o_beta, l.o_mv, l.cout});
  }
  MWW_TRY(dev_alloc(&phase_clk, (size_t)2 * MWW_MAX_BLOCKS * 2048 * kClkSlots));
  return MWW_OK;
}

int BlockModel::set_option(mww_ctx* c, const OptionRow& o, int64_t v) {
  if (o.owner != OPT_BLOCK) return MWW_OK;
  const std::string name = o.name;
  if (name == "pointwise_bf16" || name == "storage_bf16") {
    std::string why;
    if (v && !shape_supported(d, &why, true)) return fail(MWW_ERR_UNSUPPORTED, "no bf16 mode for this topology: " + why);
    if (name == "pointwise_bf16") { pw_bf16 = v != 0; if (!v) st_bf16 = false; }
    else { st_bf16 = v != 0; if (v) pw_bf16 = true; }
  }
  const std::pair<const char*, bool BlockModel::*> flags[] = {{"bwd_wide", &BlockModel::bwd_wide}, {"conv1_x6", &BlockModel::conv1_x6},
                                                              {"conv1_x6_fwd", &BlockModel::conv1_x6_fwd}, {"bwd_first_wide", &BlockModel::bwd_first_wide}};
  const std::pair<const char*, int BlockModel::*> ints[] = {{"ablate", &BlockModel::ablate}, {"dp_commit_late", &BlockModel::dp_commit_late},
                                                            {"grid_fwd", &BlockModel::grid_fwd}, {"grid_bwd", &BlockModel::grid_bwd}};
  for (auto& f : flags) if (name == f.first) this->*f.second = v != 0;
  for (auto& f : ints) if (name == f.first) this->*f.second = (int)v;
  return MWW_OK;
}

// p<k> / g<k> / bn<k> of block k (1-based), a0, and the phase clocks clkf<k> / clkb<k>
int BlockModel::debug_tensor(mww_ctx* c, const char* name, int B, DebugTensor* t) {
  const int nb = d.n_blocks;
  auto idx = [&](const char* prefix) -> int {
    const size_t pl = strlen(prefix);
    if (strncmp(name, prefix, pl) != 0) return -1;
    const int k = atoi(name + pl);
    return (k >= 1 && k <= nb && name[pl] >= '0' && name[pl] <= '9') ? k - 1 : -1;
  };
  int k;
  if ((k = idx("p")) >= 0 || (k = idx("g")) >= 0) {   // bf16 in HBM under "storage_bf16", widened for the caller
    t->src = name[0] == 'p' ? L[k].p : L[k].g;
    t->n = (int64_t)B * L[k].tout * L[k].cout;
    t->bf16 = st_bf16;
  }
  else if ((k = idx("bn")) >= 0) { t->src = L[k].bn; t->n = (int64_t)9 * L[k].cout; }
  else if (!strcmp(name, "a0")) { t->src = a0; t->n = (int64_t)B * L[0].tin * d.conv1_filters; }   // relu(conv1(x)) as the first block stored it
  else if (!strncmp(name, "clkf", 4) || !strncmp(name, "clkb", 4)) {
    // phase clocks of layer k (1-based) as raw 64-bit counters viewed as floats: 2048 x kClkSlots x 2 words
    const int kk = atoi(name + 4);
    if (kk < 1 || kk > nb) return fail(MWW_ERR_INVALID, "bad layer");
    t->src = reinterpret_cast<const float*>(phase_clk + (size_t)(2 * (kk - 1) + (name[3] == 'b' ? 1 : 0)) * 2048 * kClkSlots);
    t->n = 2048 * kClkSlots * 2;
  }
  else return 0;
  return 1;
}

}  // namespace

int plan_mixednet(const mww_mixednet_desc& d, Model** out) {
  if (d.n_blocks < 2 || d.n_blocks > MWW_MAX_BLOCKS) return fail(MWW_ERR_INVALID, "n_blocks must be in [2, 8]");
  if (d.conv1_stride < 1 || d.frames < d.conv1_kernel) return fail(MWW_ERR_INVALID, "bad first-conv stride / kernel");
  if (d.conv1_filters <= 0) return fail(MWW_ERR_UNSUPPORTED, "first_conv_filters == 0 is not implemented");
  if (d.max_batch <= 0 || d.frames <= 0) return fail(MWW_ERR_INVALID, "frames and max_batch must be positive");
  std::string why;
  if (!shape_supported(d, &why)) return fail(MWW_ERR_UNSUPPORTED, why);
  BlockModel* m = new BlockModel();
  m->d = d;
  *out = m;
  return MWW_OK;
}

}  // namespace mww
