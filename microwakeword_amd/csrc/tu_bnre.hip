// Translation unit of BatchNorm re-estimation for the weight average (kernels_bnre.hip.h): the kernels, their launches and the
// host side of mww_bn_reestimate_* - the pass, its collect table and the validity of its result.  The collect kernel calls
// the summation helpers of the two engines' own folds (reduce_partials_256; gfold_load_sums, block_sum2), so it sees their headers.
#define MWW_BLOCK_TU 1        // the non-template kernels of the block-kernel headers belong to mww_lib.hip,
#define MWW_GRAPH_HOST_TU 1   // those of the graph kernel headers to tu_graph.hip
#define MWW_BNRE_TU 1
#include "kernels_graph.hip.h"   // (includes kernels_fwd.hip.h)
#include "engine.hip.h"          // (includes kernels_bnre.hip.h)

#include <cstring>

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

void invalidate_ema_bn(mww_ctx* c) {
  c->bnre.valid = false;
  c->bnre.batches = -1;
}

void free_bn_reestimate(mww_ctx* c) {
  BnreState& r = c->bnre;
  void* bufs[] = {r.ema_bn, r.acc, r.table};
  for (void* p : bufs) if (p) (void)hipFree(p);
  r = BnreState();
}

int enqueue_bnre_collect(mww_ctx* c, std::vector<BnreRow>& rows) {
  if (rows.empty()) return MWW_OK;
  BnreState& r = c->bnre;
  int blocks = 0;
  for (BnreRow& row : rows) {
    row.nblocks = row.form == BNRE_ROWS ? 1 : (row.groups > 1 ? row.groups : row.C);
    row.block0 = blocks;
    blocks += row.nblocks;
  }
  const size_t bytes = rows.size() * sizeof(BnreRow);
  if (r.table_host.size() != bytes || memcmp(r.table_host.data(), rows.data(), bytes) != 0) {
    // a row changes with the batch size, the statistics path ("bn_inline", sync-BN) or a grid option - not from batch to
    // batch of a pass (the accumulator parity travels as a launch argument) - so this wait is paid once per configuration
    HIPCHK(hipStreamSynchronize(c->stream));   // (the launches that read the old table are done)
    if (r.table_rows < (int)rows.size()) {
      if (r.table) HIPCHK(hipFree(r.table));
      r.table = nullptr;
      r.table_rows = 0;
      MWW_TRY(dev_alloc(&r.table, rows.size()));
      r.table_rows = (int)rows.size();
    }
    r.table_host.clear();
    HIPCHK(hipMemcpy(r.table, rows.data(), bytes, hipMemcpyHostToDevice));
    r.table_host.assign(reinterpret_cast<const char*>(rows.data()), reinterpret_cast<const char*>(rows.data()) + bytes);
  }
  Launcher lp{c};
  lp.begin("bn_reestimate_collect");
  // the forward flipped the parity behind its last launch: its rows are the other one's
  launch_bnre_collect(BnreCollectArgs{r.table, (int)rows.size(), c->fpar ^ 1, r.acc}, blocks, c->stream);
  lp.end();
  return MWW_OK;
}

}  // namespace mww

using namespace mww;

extern "C" {

int mww_bn_reestimate_begin(mww_ctx* c) {
  if (!c) return fail(MWW_ERR_INVALID, "null context");
  if (!c->ema.vec || c->ema.updates == 0) return fail(MWW_ERR_INVALID, "bn_reestimate needs a weight average that has taken an update");
  HIPCHK(hipSetDevice(c->device));
  BnreState& r = c->bnre;
  if (!r.ema_bn) MWW_TRY(dev_alloc(&r.ema_bn, (size_t)c->S));
  if (!r.acc) MWW_TRY(dev_alloc(&r.acc, (size_t)c->S));
  HIPCHK(hipMemsetAsync(r.acc, 0, (size_t)c->S * sizeof(double), c->stream));
  r.batches = 0;
  return MWW_OK;
}

int mww_bn_reestimate_batch(mww_ctx* c, int B) {
  if (!c || B <= 0 || B > c->max_batch) return fail(MWW_ERR_INVALID, "bad batch size");
  if (c->bnre.batches < 0) return fail(MWW_ERR_STATE, "bn_reestimate: no pass is open (call mww_bn_reestimate_begin; an update of the average closes a pass)");
  if (c->have_batch < B) return fail(MWW_ERR_STATE, "forward needs a batch of at least B rows");
  HIPCHK(hipSetDevice(c->device));
  int rc = batch_ready(c);
  if (rc) return rc;
  // the forward of mww_forward(training = 1, update_metrics = 0) - batch statistics, moving statistics untouched, no loss, no
  // metrics, no dropout - standing on the average (with "weight_qat": on its shadow); never captured
  EmaSource source(c, true);
  c->ema.src = true;
  rc = refresh_shadow(c);
  if (rc) return rc;
  rc = c->model->enqueue_forward(c, B, true, false, false, false);
  if (rc) return rc;
  rc = join_side(c);
  if (rc) return rc;
  rc = c->model->enqueue_bn_collect(c, B);   // directly behind the forward: its accumulator parity is still the current one
  if (rc) return rc;
  HIPCHK(hipGetLastError());
  c->bnre.batches += 1;
  return mail_commit(c);
}

int mww_bn_reestimate_commit(mww_ctx* c) {
  if (!c) return fail(MWW_ERR_INVALID, "null context");
  BnreState& r = c->bnre;
  if (r.batches <= 0) return fail(MWW_ERR_STATE, "bn_reestimate: commit without a collected batch");
  HIPCHK(hipSetDevice(c->device));
  Launcher lp{c};
  lp.begin("bn_reestimate_commit");
  launch_bnre_commit(BnreCommitArgs{r.acc, r.ema_bn, (double)r.batches, (int)c->S}, c->stream);
  lp.end();
  HIPCHK(hipGetLastError());
  r.batches = -1;
  r.valid = true;
  return MWW_OK;
}

int mww_bn_reestimate_windows(mww_ctx* c, const mww_window* windows, int64_t n, int batch) {
  if (!c || !windows || batch <= 0 || batch > c->max_batch) return fail(MWW_ERR_INVALID, "bad re-estimation arguments");
  if (n <= 0 || n % batch != 0) return fail(MWW_ERR_INVALID, "bn_reestimate: the window count must be a positive multiple of the batch size (every batch weighs the same)");
  if (!c->ema.vec || c->ema.updates == 0) return fail(MWW_ERR_INVALID, "bn_reestimate needs a weight average that has taken an update");
  // the first batch is assembled before the pass opens: windows the stores refuse leave the context as it was
  int rc = mww_assemble_batch(c, windows, nullptr, batch, 0, 0);
  if (!rc) rc = mww_bn_reestimate_begin(c);
  for (int64_t s = 0; s < n && !rc; s += batch) {
    if (s) rc = mww_assemble_batch(c, windows + s, nullptr, batch, 0, 0);
    if (!rc) rc = mww_bn_reestimate_batch(c, batch);
    hold_shadow(c, c->ema.vec);   // the average cannot change between the batches: the first batch's shadow serves them all
  }
  hold_shadow(c, nullptr);
  if (rc) { c->bnre.batches = -1; return rc; }
  return mww_bn_reestimate_commit(c);
}

int mww_get_ema_bn_state(mww_ctx* c, float* h, int64_t n, int* valid) {
  if (!c || !c->ema.vec) return fail(MWW_ERR_INVALID, "no weight average installed: call mww_set_weight_ema first");
  if (n != c->S) return fail(MWW_ERR_INVALID, "BN state size mismatch");
  if (valid) *valid = c->bnre.valid ? 1 : 0;
  return h ? copy_out(c, h, c->bnre.valid ? c->bnre.ema_bn : c->bn_state, (size_t)n * sizeof(float)) : MWW_OK;
}

int mww_set_ema_bn_state(mww_ctx* c, const float* h, int64_t n) {
  if (!c || !c->ema.vec) return fail(MWW_ERR_INVALID, "no weight average installed: call mww_set_weight_ema first");
  if (!h || n != c->S) return fail(MWW_ERR_INVALID, "BN state size mismatch");
  HIPCHK(hipSetDevice(c->device));
  if (!c->bnre.ema_bn) MWW_TRY(dev_alloc(&c->bnre.ema_bn, (size_t)c->S));
  MWW_TRY(copy_in(c, c->bnre.ema_bn, h, (size_t)n * sizeof(float)));
  c->bnre.batches = -1;
  c->bnre.valid = true;
  return MWW_OK;
}

}  // extern "C"
