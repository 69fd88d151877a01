// mww_stream_operating_bootstrap (include/mww.h): the operating-point grid of mww_stream_operating_summary resampled
// on the device - R bootstrap replicates over the evaluation units, ambient blocks and positive tracks - with one small record
// per replicate read back.  The definitions (units, draws, replicate grid, records) are stated in include/mww.h and restated in
// NumPy by streaming.operating_bootstrap_host; everything is integer arithmetic or single IEEE float64 operations, so the
// records equal the restatement byte for byte.
//
// The call is an OpCall (stream_oppoints.hip.h): op_segment_kernel builds the transfer tables of the ambient tracks' segments
// per pass of windows, then
//   boot_ambient_kernel    one thread per (ambient track, window, cutoff): the walk of ops_ambient_kernel (op_walk), with each
//                          segment's accepts folded into the block that owns the segment - a block is a whole number of
//                          segments - instead of into one total: blk_cnt [W][NB][C] u32; the thread of cutoff 0 writes the
//                          blocks' lengths blk_len [W][NB].
//   boot_level_kernel      one thread per (positive track, window): the track's score (op_score) as ONE level, the number of
//                          cutoffs it exceeds - the cutoffs ascend strictly, so it exceeds exactly the first `level` of them -:
//                          level [n_pos][W] u8, a track's windows side by side (one draw serves all windows).
// and after the last pass
//   boot_replicate_kernel  one workgroup of BOOT_THREADS per replicate, the replicate's whole grid in LDS:
//                            ambient    the NB draws in chunks of BOOT_THREADS (thread i hashes draw base + i into LDS); thread
//                                       `id` owns the items id, id + BOOT_THREADS, ... of the W * C counts and W slice sums and
//                                       adds the drawn rows to them: no two threads share an item, no atomics;
//                            positives  thread i takes the draws i, i + BOOT_THREADS, ...: one hash, then the drawn track's W
//                                       levels into the level histograms [W][C + 1] with integer LDS atomics (integer addition
//                                       commutes: the histogram does not depend on the arrival order); thread k then turns
//                                       window k's histogram into its suffix sums, accepts_r[k][c] = #{level > c};
//                            selection  thread k walks window k's cutoffs from the largest down while faph_r <= target (the
//                                       rule's "at every larger cutoff"), thread 0 takes the minimum of (frr, faph, window,
//                                       row) over the windows in row order and writes the record.
// No float atomics, no order of arrival anywhere: two calls write the same bytes.  LDS per workgroup: (W * C + W) * 8 +
// W * (C + 1) * 4 + W * 24 + BOOT_THREADS * 4 bytes, 52 KB at the limits (32 windows x 128 cutoffs), 13 KB at 10 x 101.
// The device scratch (blk_cnt, blk_len, level) is capped; beyond the cap the call is MWW_ERR_UNSUPPORTED and names a larger block.
#include "stream_oppoints.hip.h"

namespace {

constexpr int BOOT_THREADS = 256;                      // of boot_replicate_kernel; boot_level_kernel has the same
constexpr int64_t BOOT_SCRATCH = (int64_t)256 << 20;   // default cap on blk_cnt + blk_len + level
static_assert(MWW_BOOT_BLOCK_UNIT == POST_SEG, "a block is a whole number of segments");
static_assert(POST_MAX_CUTOFFS <= 255, "a level fits a byte");

struct BootArgs {
  const int* amb;            // [n_amb] the kind-0 tracks, in track order
  const int* pos;            // [n_pos] the kind-1 tracks, in track order
  const int* blk_first;      // [n_amb + 1] first block of each ambient track
  const int* usable;         // [n_win] the window is usable on the full data
  int n_amb, n_pos, n_blk, n_win;
  int seg_per_blk;           // segments per block; 0: a track is one block
  int stride;
  double step_s, target;
  unsigned long long seed;
  int fixed_row, fixed_cut;  // -1: none
  unsigned* blk_cnt;         // [n_win][n_blk][n_cut]
  int64_t* blk_len;          // [n_win][n_blk]
  unsigned char* level;      // [n_pos][n_win]
  mww_boot_record* rec;      // [replicates]
};

// draw(seed, kind, r, i, n) of include/mww.h: a splitmix64 counter hash, multiply-shift onto 0 .. n - 1 (no rejection: the
// bias is below n / 2^32)
__device__ __forceinline__ unsigned boot_draw(unsigned long long seed, unsigned kind, unsigned r, unsigned i, unsigned n) {
  const unsigned long long ctr = (unsigned long long)kind << 56 | (unsigned long long)r << 32 | i;
  unsigned long long z = seed + ctr * 0x9E3779B97F4A7C15ull;
  z ^= z >> 30;
  z *= 0xBF58476D1CE4E5B9ull;
  z ^= z >> 27;
  z *= 0x94D049BB133111EBull;
  z ^= z >> 31;
  return (unsigned)(((z >> 32) * n) >> 32);
}

__global__ void __launch_bounds__(256) boot_ambient_kernel(OpArgs a, BootArgs o) {
  const int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= (int64_t)o.n_amb * a.pw * a.n_cut) return;
  const int c = (int)(id % a.n_cut), wk = (int)(id / a.n_cut % a.pw), j = (int)(id / a.n_cut / a.pw);
  const int wi = a.w0 + wk, t = o.amb[j];
  const int64_t m = op_len(a, t, wi);
  const int n_segs = (int)((m + POST_SEG - 1) / POST_SEG);
  const int b0 = o.blk_first[j], nb = o.blk_first[j + 1] - b0;
  if (nb == 0) return;   // a track without a probability under block > 0
  // the track's blocks at (wi, c): block b at out[b * n_cut].  A segment s lies in block s / seg_per_blk < nb: its first value
  // s * POST_SEG < m <= the track's probabilities
  unsigned* out = o.blk_cnt + ((int64_t)wi * o.n_blk + b0) * a.n_cut + c;
  for (int b = 0; b < nb; ++b) out[(int64_t)b * a.n_cut] = 0u;
  int cur = 0;
  unsigned acc = 0u;
  op_walk(a, a.tab_first[t], n_segs, wk, c, [&](int s, unsigned cnt) {
    const int b = o.seg_per_blk ? s / o.seg_per_blk : 0;
    if (b != cur) {
      out[(int64_t)cur * a.n_cut] = acc;
      acc = 0u;
      cur = b;
    }
    acc += cnt;
  });
  out[(int64_t)cur * a.n_cut] = acc;
  if (c != 0) return;
  int64_t* len = o.blk_len + (int64_t)wi * o.n_blk + b0;
  if (!o.seg_per_blk) {
    len[0] = m;
    return;
  }
  const int64_t L = (int64_t)o.seg_per_blk * POST_SEG;
  for (int b = 0; b < nb; ++b) {   // [b L, min((b + 1) L, m)), possibly empty
    const int64_t hi = (b + 1) * L < m ? (b + 1) * L : m;
    len[b] = hi > b * L ? hi - b * L : 0;
  }
}

__global__ void __launch_bounds__(BOOT_THREADS) boot_level_kernel(OpArgs a, BootArgs o) {
  const int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= (int64_t)o.n_pos * a.pw) return;
  const int wk = (int)(id % a.pw), i = (int)(id / a.pw);
  const int wi = a.w0 + wk, t = o.pos[i];
  const int64_t m = op_len(a, t, wi);
  const double score = (double)op_score(a, wi, a.seg_first[t], (int)((m + POST_SEG - 1) / POST_SEG));
  int lv = 0;
  for (int c = 0; c < a.n_cut; ++c) lv += score > a.cut[c];   // strict; -inf (no value) exceeds none
  o.level[(int64_t)i * o.n_win + wi] = (unsigned char)lv;
}

__global__ void __launch_bounds__(BOOT_THREADS) boot_replicate_kernel(OpArgs a, BootArgs o) {
  HIP_DYNAMIC_SHARED(unsigned long long, s_mem)
  const int W = o.n_win, C = a.n_cut, tid = threadIdx.x;
  const unsigned r = blockIdx.x;
  const int n_items = W * C + W;   // counts_r [W][C], then slices_r [W]
  unsigned long long* s_acc = s_mem;
  double* s_frr = reinterpret_cast<double*>(s_acc + n_items);   // [W] at the chosen cutoff
  double* s_faph = s_frr + W;
  unsigned* s_hist = reinterpret_cast<unsigned*>(s_faph + W);   // [W][C + 1]; after the suffix sums accepts_r[k][c] at [k][c + 1]
  int* s_chosen = reinterpret_cast<int*>(s_hist + W * (C + 1)); // [W]
  unsigned* s_draw = reinterpret_cast<unsigned*>(s_chosen + W); // [BOOT_THREADS]
  for (int q = tid; q < n_items; q += BOOT_THREADS) s_acc[q] = 0ull;
  for (int q = tid; q < W * (C + 1); q += BOOT_THREADS) s_hist[q] = 0u;
  __syncthreads();
  // ambient: NB draws of a block
  for (int base = 0; base < o.n_blk; base += BOOT_THREADS) {
    const int nd = o.n_blk - base < BOOT_THREADS ? o.n_blk - base : BOOT_THREADS;
    if (tid < nd) s_draw[tid] = boot_draw(o.seed, 0u, r, (unsigned)(base + tid), (unsigned)o.n_blk);
    __syncthreads();
    for (int q = tid; q < n_items; q += BOOT_THREADS) {
      unsigned long long sum = 0ull;
      if (q < W * C) {
        const unsigned* col = o.blk_cnt + (int64_t)(q / C) * o.n_blk * C + q % C;
        for (int d = 0; d < nd; ++d) sum += col[(int64_t)s_draw[d] * C];
      } else {
        const int64_t* len = o.blk_len + (int64_t)(q - W * C) * o.n_blk;
        for (int d = 0; d < nd; ++d) sum += (unsigned long long)len[s_draw[d]];
      }
      s_acc[q] += sum;
    }
    __syncthreads();
  }
  // positives: n_pos draws of a track, its level at every window
  for (int i = tid; i < o.n_pos; i += BOOT_THREADS) {
    const unsigned char* lv = o.level + (int64_t)boot_draw(o.seed, 1u, r, (unsigned)i, (unsigned)o.n_pos) * W;
    for (int k = 0; k < W; ++k) atomicAdd(&s_hist[k * (C + 1) + lv[k]], 1u);
  }
  __syncthreads();
  if (tid < W) {
#pragma clang fp contract(off)
    const int k = tid;
    unsigned* h = s_hist + k * (C + 1);
    unsigned run = 0u;
    for (int c = C - 1; c >= 0; --c) {   // accepts_r[k][c] = the tracks of level > c
      run += h[c + 1];
      h[c + 1] = run;
    }
    const int64_t slices = (int64_t)s_acc[W * C + k];
    int chosen = -1;
    double faph_at = 0.0;
    if (o.usable[k] && slices > 0) {
      const double prod = (double)(slices * (int64_t)o.stride) * o.step_s;
      const double hours = prod / 3600.0;
      for (int c = C - 1; c >= 0; --c) {   // the smallest cutoff with faph <= target there and at every larger one
        const double faph = (double)s_acc[k * C + c] / hours;
        if (!(faph <= o.target)) break;
        chosen = c;
        faph_at = faph;
      }
    }
    s_chosen[k] = chosen;
    if (chosen >= 0) {
      const double quot = (double)h[chosen + 1] / (double)o.n_pos;
      s_frr[k] = 1.0 - quot;
      s_faph[k] = faph_at;
    }
  }
  __syncthreads();
  if (tid != 0) return;
  int best = -1;
  for (int k = 0; k < W; ++k) {   // the minimum of (frr, faph, window, row), rows in order
    if (s_chosen[k] < 0) continue;
    bool less = best < 0;
    if (!less) {
      if (s_frr[k] != s_frr[best]) less = s_frr[k] < s_frr[best];
      else if (s_faph[k] != s_faph[best]) less = s_faph[k] < s_faph[best];
      else less = a.win[k] < a.win[best];
    }
    if (less) best = k;
  }
  mww_boot_record out{};
  out.sel_row = best;
  out.sel_cutoff = best >= 0 ? s_chosen[best] : -1;
  if (best >= 0) {
    out.sel_counts = s_acc[best * C + out.sel_cutoff];
    out.sel_slices = (int64_t)s_acc[W * C + best];
    out.sel_accepts = s_hist[best * (C + 1) + out.sel_cutoff + 1];
  }
  if (o.fixed_row >= 0) {
    out.fixed_counts = s_acc[o.fixed_row * C + o.fixed_cut];
    out.fixed_slices = (int64_t)s_acc[W * C + o.fixed_row];
    out.fixed_accepts = s_hist[o.fixed_row * (C + 1) + o.fixed_cut + 1];
  }
  o.rec[r] = out;
}

}  // namespace

extern "C" int mww_stream_operating_bootstrap(mww_stream* s, const int64_t* offsets, const int32_t* kind, int64_t n_tracks,
                                              const int32_t* windows, int n_windows, int skip, int cooldown, const double* cutoffs,
                                              int n_cutoffs, int stride, double step_s, int replicates, uint64_t seed, int64_t block,
                                              double target_faph, int fixed_row, int fixed_cutoff, int64_t max_scratch_bytes,
                                              mww_boot_record* records) {
  if (!s || !offsets || !kind || !windows || !cutoffs || !records) return mww::set_error(MWW_ERR_INVALID, "null argument");
  if (stride < 1 || !(step_s > 0)) return mww::set_error(MWW_ERR_INVALID, "bad operating-bootstrap arguments (stride >= 1, step_s > 0)");
  if (replicates < 1 || replicates > MWW_BOOT_MAX_REPLICATES)
    return mww::set_error(MWW_ERR_INVALID, ("replicates must lie in 1.." + std::to_string(MWW_BOOT_MAX_REPLICATES)).c_str());
  if (block < 0 || block % MWW_BOOT_BLOCK_UNIT || block / MWW_BOOT_BLOCK_UNIT > INT32_MAX)
    return mww::set_error(MWW_ERR_INVALID, ("block must be 0 or a positive multiple of " + std::to_string(MWW_BOOT_BLOCK_UNIT)).c_str());
  if (max_scratch_bytes < 0) return mww::set_error(MWW_ERR_INVALID, "max_scratch_bytes must be 0 (the default) or a positive size");
  OpCall c;
  if (int rc = c.begin(s, offsets, kind, n_tracks, windows, n_windows, skip, cooldown, cutoffs, n_cutoffs, true)) return rc;
  for (int q = 1; q < n_cutoffs; ++q)
    if (!(cutoffs[q] > cutoffs[q - 1])) return mww::set_error(MWW_ERR_INVALID, "the cutoffs of a bootstrap must ascend strictly");
  if ((fixed_row < 0) != (fixed_cutoff < 0) || fixed_row >= n_windows || fixed_cutoff >= n_cutoffs)
    return mww::set_error(MWW_ERR_INVALID, "the fixed point must be a (row, cutoff) of the grid, or (-1, -1) for none");
  const int64_t W = n_windows, C = n_cutoffs;
  std::vector<int32_t> amb, pos, blk_first, usable((size_t)W, 1);
  for (int64_t t = 0; t < n_tracks; ++t) (kind[t] ? pos : amb).push_back((int32_t)t);
  const int64_t n_amb = (int64_t)amb.size(), n_pos = (int64_t)pos.size();
  int64_t n_blk = 0;
  for (int64_t j = 0; j < n_amb; ++j) {
    blk_first.push_back((int32_t)n_blk);
    const int64_t n = offsets[amb[(size_t)j] + 1] - offsets[amb[(size_t)j]];
    n_blk += block ? (n + block - 1) / block : 1;
    if (n_blk > INT32_MAX) return mww::set_error(MWW_ERR_INVALID, "too many blocks for one call");
  }
  blk_first.push_back((int32_t)n_blk);
  // a window is usable on the full data as in the summary: an ambient track exists and no track is without a value
  for (int64_t k = 0; k < W; ++k) {
    bool ok = n_amb > 0 && n_pos > 0;
    for (int64_t t = 0; ok && t < n_tracks; ++t) ok = offsets[t + 1] - offsets[t] - (kind[t] ? skip : 0) >= windows[k];
    usable[(size_t)k] = ok;
  }
  const int64_t cap = max_scratch_bytes ? max_scratch_bytes : BOOT_SCRATCH;
  const int64_t scratch = W * n_blk * C * 4 + W * n_blk * 8 + n_pos * W;
  if (scratch > cap)
    return mww::set_error(MWW_ERR_UNSUPPORTED, ("the bootstrap's block tables need " + std::to_string(scratch) + " bytes of device scratch, above the cap of " +
                                                std::to_string(cap) + ": use a larger block (" + std::to_string(n_blk) + " blocks now)").c_str());
  BootArgs o{};
  c.tab.add(&o.amb, n_amb, amb.data());
  c.tab.add(&o.pos, n_pos, pos.data());
  c.tab.add(&o.blk_first, n_amb + 1, blk_first.data());
  c.tab.add(&o.usable, W, usable.data());
  c.tab.add(&c.a.tab_first, n_tracks + 1, c.plan.tab_first.data());   // table rows for the ambient tracks' segments alone
  c.tab.end_host();
  c.tab.add(&o.rec, (int64_t)replicates);
  c.tab.add(&o.blk_cnt, W * n_blk * C);
  c.tab.add(&o.blk_len, W * n_blk);
  c.tab.add(&o.level, n_pos * W);
  if (int rc = c.commit(s)) return rc;
  o.n_amb = (int)n_amb;
  o.n_pos = (int)n_pos;
  o.n_blk = (int)n_blk;
  o.n_win = n_windows;
  o.seg_per_blk = (int)(block / MWW_BOOT_BLOCK_UNIT);
  o.stride = stride;
  o.step_s = step_s;
  o.target = target_faph;
  o.seed = seed;
  o.fixed_row = fixed_row;
  o.fixed_cut = fixed_cutoff;
  const int rc = c.passes(s, [&](const OpArgs& a) {
    if (n_amb) {
      const int64_t n_thr = n_amb * a.pw * C;
      hipLaunchKernelGGL(boot_ambient_kernel, dim3((unsigned)((n_thr + 255) / 256)), dim3(256), 0, s->stream, a, o);
      SCHK(hipGetLastError());
    }
    if (n_pos) {
      const int64_t n_thr = n_pos * a.pw;
      hipLaunchKernelGGL(boot_level_kernel, dim3((unsigned)((n_thr + BOOT_THREADS - 1) / BOOT_THREADS)), dim3(BOOT_THREADS), 0, s->stream, a, o);
      SCHK(hipGetLastError());
    }
    return (int)MWW_OK;
  });
  if (rc) return rc;
  const size_t lds = (size_t)((W * C + W) * 8 + W * 16 + W * (C + 1) * 4 + W * 4 + BOOT_THREADS * 4);
  hipLaunchKernelGGL(boot_replicate_kernel, dim3((unsigned)replicates), dim3(BOOT_THREADS), lds, s->stream, c.a, o);
  SCHK(hipGetLastError());
  SCHK(hipMemcpyAsync(records, o.rec, (size_t)replicates * sizeof(mww_boot_record), hipMemcpyDeviceToHost, s->stream));
  SCHK(hipStreamSynchronize(s->stream));
  return MWW_OK;
}
