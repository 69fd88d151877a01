// BatchNorm re-estimation for the weight average (mww_bn_reestimate_*): ema_bn[S] = the mean, over the K batches of a pass, of
// the batch mean and the biased batch variance a training-mode forward AT THE AVERAGE normalised with - laid out and indexed
// like bn_state.  Two launches:
//   collect (one per batch, directly behind the forward):  acc[o_mm + s] += (double)meanf[s],  acc[o_mv + s] += (double)varf[s]
//   commit  (one per pass):                                ema_bn[i] = (float)(acc[i] / (double)K)
// acc[S] is float64.  No atomics: a slot's two sums have one writer per launch, the batches add in stream order, so two passes
// over the same batches write the same bytes.
//
// meanf / varf are re-derived from the sums the forward's own fold consumed, with that fold's expressions and its summation
// order, so that they are the floats the forward normalised with (the published rstd = 1 / sqrt(varf + eps) is another float):
//   accumulator rows (statistics hand-over: bn_fold_channel, gfold_forward_finish) - the kStatRows rows in ascending order,
//     a SubSpectralNormalization slot's members first (gfold_load_sums itself);
//   partial rows behind a finalize launch - the 2 x 128-thread strided sums of reduce_partials_256 (block engine) or the
//     strided sums + block_sum2 tree of gbn_fwd_finalize_body (graph engine), by calling those functions.
// A 256-thread reduction tree has no one-thread equivalent short of 256 private partial sums, so the partial-row forms take one
// workgroup per slot; the accumulator-row form takes one thread per slot (one workgroup per tensor).
//
// Visibility: the accumulator rows were written by memory-side atomics and agent-scope stores in earlier launches
// (common.hip.h publish_stat); the kernel boundary publishes them, and they are read here with agent-scope loads like the
// producers' accesses, so no line of them is left in an XCD's L2.  acc[] has one writer per element and is only read by the
// next launch on the same stream.  Nothing synchronises inside a launch beyond the finalize orders' own barriers.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "common.hip.h"

struct mww_ctx;

namespace mww {

enum { BNRE_ROWS = 0, BNRE_PART_BLOCK = 1, BNRE_PART_GRAPH = 2 };

// one BN'd tensor of the model as the forward just enqueued left its statistics (device-resident table, one row per tensor)
struct BnreRow {
  const double* acc[2];   // BNRE_ROWS: [kStatRows][2][C] accumulator rows of either parity (the launch says which is current)
  const float* part;      // BNRE_PART_*: [G][2][C] partial rows (or the one row of sums a sync-BN exchange left)
  int G, C, groups;       // groups > 1: SubSpectralNormalization with that many slots (slot s owns channels s, s + groups, ...)
  int form;               // BNRE_*
  float inv_n;            // the forward's own 1 / (B * T * channels per slot) (sync-BN: over the global batch)
  int o_mm, o_mv;         // the tensor's slots in bn_state / ema_bn / acc
  int block0, nblocks;    // its workgroups in the collect launch: 1 (BNRE_ROWS) or one per slot
};

struct BnreCollectArgs {
  const BnreRow* rows;
  int n_rows;
  int parity;             // accumulator parity of the forward just enqueued
  double* acc;            // [S]
};

struct BnreCommitArgs {
  const double* acc;      // [S]
  float* ema_bn;          // [S]
  double batches;         // K
  int n;                  // S
};

// BatchNorm re-estimation for the average (mww_bn_reestimate_*): `ema_bn` = the batch statistics of training-mode forwards at
// the average, averaged over a pass; while `valid`, a non-training forward that stands on the average folds them instead of the
// master's moving statistics (eval_bn_state).  Allocated by the first pass.
struct BnreState {
  float* ema_bn = nullptr;
  bool valid = false;
  double* acc = nullptr;          // [S] float64 sums of the pass in progress
  int64_t batches = -1;           // batches collected by the pass in progress; -1: none is open
  BnreRow* table = nullptr;       // device-resident table of the collect launch
  int table_rows = 0;
  std::vector<char> table_host;   // what it holds (uploaded again only when a row changes)
};

// ---- tu_bnre.hip (also mww_bn_reestimate_*, mww_get_ema_bn_state, mww_set_ema_bn_state)
int launch_bnre_collect(const BnreCollectArgs& a, int blocks, hipStream_t stream);
int launch_bnre_commit(const BnreCommitArgs& a, hipStream_t stream);
// Whatever changes what a forward at the average reads - an update of the average, mww_set_ema_state, installing / removing the
// average, the "weight_qat" option or map - leaves the re-estimated statistics describing another model: evaluations read the
// master's moving statistics again, and a pass in progress is closed
void invalidate_ema_bn(mww_ctx* c);
void free_bn_reestimate(mww_ctx* c);
// (Model::enqueue_bn_collect) block0 / nblocks of the rows are filled in, the device table is brought up to date, the collect is launched
int enqueue_bnre_collect(mww_ctx* c, std::vector<BnreRow>& rows);

#ifdef MWW_BNRE_TU
// sums -> the fp32 batch mean and biased batch variance; the expressions of bn_fold_channel / bn_fwd_finalize_kernel /
// gfold_forward_finish / gbn_fwd_finalize_body, token for token
__device__ __forceinline__ void bnre_mean_var(double t1, double t2, float inv_n, float& meanf, float& varf) {
  const double m = t1 * (double)inv_n;
  double var = t2 * (double)inv_n - m * m;   // biased batch variance
  if (var < 0.0) var = 0.0;
  meanf = (float)m;
  varf = (float)var;
}

__device__ __forceinline__ void bnre_add(double* acc, const BnreRow& r, int slot, float meanf, float varf) {
  acc[r.o_mm + slot] = acc[r.o_mm + slot] + (double)meanf;
  acc[r.o_mv + slot] = acc[r.o_mv + slot] + (double)varf;
}

__device__ __forceinline__ double bnre_load(const double* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__global__ __launch_bounds__(kThreads) void bnre_collect_kernel(BnreCollectArgs a) {
  __shared__ __attribute__((aligned(16))) double sAcc[2 * kThreads];
  __shared__ double sOut[2];
  const int tid = threadIdx.x, bid = blockIdx.x;
  int ri = 0;
  while (ri < a.n_rows - 1 && bid >= a.rows[ri].block0 + a.rows[ri].nblocks) ++ri;   // (uniform)
  const BnreRow& r = a.rows[ri];
  const int C = r.C;
  if (r.form == BNRE_ROWS) {
    const double* acc = a.parity ? r.acc[1] : r.acc[0];
    if (r.groups > 1) {
      // lanes = channels (C <= kGFoldC = a wave, as in the folding launches); whole waves call the exchange
      if (tid < 64) {
        GFoldRegs g;
        gfold_load_sums(acc, C, r.groups, tid, g);
        if (tid < r.groups) {
          double t1 = 0.0, t2 = 0.0;
#pragma unroll
          for (int j = 0; j < kStatRows; ++j) {
            t1 += g.v1[j];
            t2 += g.v2[j];
          }
          float meanf, varf;
          bnre_mean_var(t1, t2, r.inv_n, meanf, varf);
          bnre_add(a.acc, r, tid, meanf, varf);
        }
      }
      return;
    }
    for (int ch = tid; ch < C; ch += kThreads) {
      double v1[kStatRows], v2[kStatRows];
#pragma unroll
      for (int j = 0; j < kStatRows; ++j) {
        v1[j] = bnre_load(acc + (size_t)j * 2 * C + ch);
        v2[j] = bnre_load(acc + (size_t)j * 2 * C + C + ch);
      }
      double s1 = 0.0, s2 = 0.0;
#pragma unroll
      for (int j = 0; j < kStatRows; ++j) {
        s1 += v1[j];
        s2 += v2[j];
      }
      float meanf, varf;
      bnre_mean_var(s1, s2, r.inv_n, meanf, varf);
      bnre_add(a.acc, r, ch, meanf, varf);
    }
    return;
  }
  const int slot = bid - r.block0;
  if (r.form == BNRE_PART_BLOCK) {   // bn_fwd_finalize_kernel
    const double s = reduce_partials_256(r.part, r.G, C, slot, sAcc, tid);
    if ((tid & 127) == 0) sOut[tid >> 7] = s;
    __syncthreads();
    if (tid == 0) {
      float meanf, varf;
      bnre_mean_var(sOut[0], sOut[1], r.inv_n, meanf, varf);
      bnre_add(a.acc, r, slot, meanf, varf);
    }
    return;
  }
  // gbn_fwd_finalize_body
  const int members = r.groups > 1 ? C / r.groups : 1, cstride = r.groups > 1 ? r.groups : 0;
  double t1 = 0.0, t2 = 0.0;
  for (int it = tid; it < r.G * members; it += kThreads) {
    const int jj = it / members, c = slot + (it % members) * cstride;
    t1 += (double)r.part[(size_t)jj * 2 * C + c];
    t2 += (double)r.part[(size_t)jj * 2 * C + C + c];
  }
  block_sum2(t1, t2, sAcc, tid);
  if (tid == 0) {
    float meanf, varf;
    bnre_mean_var(t1, t2, r.inv_n, meanf, varf);
    bnre_add(a.acc, r, slot, meanf, varf);
  }
}

__global__ __launch_bounds__(kThreads) void bnre_commit_kernel(BnreCommitArgs a) {
  const int i = (int)blockIdx.x * kThreads + (int)threadIdx.x;
  if (i < a.n) a.ema_bn[i] = (float)(a.acc[i] / a.batches);
}
#endif

}  // namespace mww
