// The metrics of the probabilities a stream holds: at one window (mww_stream_metrics), on a grid of windows
// (mww_stream_operating_points) and the grid reduced on the device (mww_stream_operating_summary).  The moving average, the
// values of a track, the segment plan, the track-table check and the table packing are those of stream_post.hip.h, shared
// with the detection launches.
//
// mww_stream_metrics: test.py:94-137 compute_false_accepts_per_hour, :329-376.  The independent form the grid is
// tested against, and deliberately the simple one:
//   stream_metrics_kernel     one workgroup per track: thread j < n_cut scans the ambient track's moving average sequentially
//                             with the cooldown of cutoff j; one thread takes the positive track's score.
//   stream_counts_sum_kernel  one thread per cutoff: the tracks' counts summed in track order.
//
// mww_stream_operating_points (include/mww.h): the false-accept counts of every (window, cutoff) pair and the
// positive scores of every window in one call, on the probabilities a stream holds.  Row k is mww_stream_metrics at windows[k].
//
// The cooldown walk is cut into segments of POST_SEG moving-average values, as in stream_detect.hip.h, and the work is parallel
// over (segment, window):
//   op_segment_kernel  one workgroup per (segment, window): stages the POST_SEG + w - 1 probabilities in LDS once, forms the
//                      averages there (the expression of the metrics kernel), and thread j < n_cutoffs builds cutoff j's
//                      transfer table from them: entry state e (next_ok - segment start) -> (accepts, last accepted offset).
//                      One BACKWARD sweep serves all entry states: F(i), the walk that enters with next_ok = i, is
//                      F(i + 1) when i is no candidate and 1 + F(i + cdp) when it is, so a ring of cdp slots (slot i mod cdp
//                      holds F(i + cdp) until F(i) replaces it) ends holding F(0 .. cdp - 1): the table.  A positive track's
//                      segment reduces its maximum instead.
//   op_track_kernel    one thread per (track, window, cutoff): composes the tables in segment order (op_compose), one
//                      dependent load per segment; thread 0 of a (track, window) takes the length and the positive score
//                      (op_score: the segments' maxima in order).
//   op_sum_kernel      one thread per (window, cutoff): the tracks' counts summed in track order.
// The tables of `pw` windows are resident at a time (OP_SCRATCH bytes at most, one window at least): the windows run in passes.
// Nothing depends on an arrival order, so two calls write the same bytes.
//
// mww_stream_operating_summary is the same grid reduced on the device to what a choice of operating point reads:
// per (window, cutoff) the ambient count and the number of positive tracks accepted, per window the ambient hours and the
// tracks without a value.  It shares op_segment_kernel; the tables have rows for the ambient tracks' segments alone (tab_first:
// a positive track's segment only reduces its maximum), so their size does not grow with the positives.  What follows differs:
//   ops_ambient_kernel   op_compose for the kind-0 tracks alone: one thread per (ambient track, window, cutoff),
//                        count rows [W][n_ambient][C].  A positive track has no thread and no row here.
//   ops_positive_kernel  one workgroup per (OPS_POS positive tracks, window): thread i takes track i's score (op_score) into
//                        LDS, then thread c counts the scores above cutoff c: an integer partial per (window, workgroup,
//                        cutoff), and the workgroup's tracks without a value.
//   ops_final_kernel     one thread per (window, cutoff) sums the ambient rows in track order and the partials in workgroup
//                        order; one thread per window walks the ambient tracks in order for the hours (float64: product,
//                        division, add, uncontracted) and the short-track counts.
// Every sum is an integer sum in a fixed order (no atomics), the hours a serial float64 sum: two calls write the same bytes.
// The host reads back the result block alone: W * C * 16 + W * 24 + 16 bytes.
//
// Both grid entry points are an OpCall (stream_oppoints.hip.h, which also holds op_segment_kernel, the composition op_walk /
// op_compose and op_score: mww_stream_operating_bootstrap in tu_stream_bootstrap.hip shares them): begin() checks, plans and
// packs the common inputs, the entry point adds the sections that are its own, commit() uploads and fills OpArgs, passes() runs
// op_segment_kernel and the entry point's launches per pass.
#include "stream_oppoints.hip.h"

namespace {

// ---- mww_stream_metrics: one workgroup per track, a sequential scan per cutoff
__global__ void __launch_bounds__(128) stream_metrics_kernel(const float* prob, const int64_t* off, const int* kind, int n_trk,
                                                             int win, int skip, int cooldown, const double* cut, int n_cut,
                                                             unsigned long long* counts, int64_t* ma_len, float* score) {
  const int t = blockIdx.x;
  if (t >= n_trk) return;
  const int j = threadIdx.x;
  const PostValues v = post_values(off, kind, skip, t, win);
  const float* p = prob + v.b;
  const int64_t m = v.m;
  if (kind[t] == 0) {
    if (j == 0) { ma_len[t] = m; score[t] = 0.f; }
    if (j < n_cut) {
      const double c = cut[j];
      int cd = cooldown;
      unsigned long long fa = 0;
      for (int64_t i = 0; i < m; ++i) {
        const float avg = post_avg(p + i, win);
        cd = cd > 0 ? cd - 1 : 0;
        if (cd == 0 && (double)avg > c) {
          ++fa;
          cd = cooldown;
        }
      }
      counts[(int64_t)t * n_cut + j] = fa;
    }
  } else {
    if (j < n_cut) counts[(int64_t)t * n_cut + j] = 0;
    if (j == 0) {
      float best = -INFINITY;
      for (int64_t i = 0; i < m; ++i) {
        const float avg = post_avg(p + i, win);
        best = avg > best ? avg : best;
      }
      ma_len[t] = m;
      score[t] = best;
    }
  }
}

// per-cutoff sum over the tracks, in track order
__global__ void stream_counts_sum_kernel(const unsigned long long* counts, int n_trk, int n_cut, unsigned long long* total) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n_cut) return;
  total[j] = post_sum_rows(counts + j, n_trk, n_cut);
}

// ---- mww_stream_operating_points
__global__ void __launch_bounds__(256) op_track_kernel(OpArgs a) {
  const int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= (int64_t)a.n_trk * a.pw * a.n_cut) return;
  const int c = (int)(id % a.n_cut), wk = (int)(id / a.n_cut % a.pw), t = (int)(id / a.n_cut / a.pw);
  const int wi = a.w0 + wk;
  const int64_t m = op_len(a, t, wi);
  const int n_segs = (int)((m + POST_SEG - 1) / POST_SEG);
  const bool positive = a.kind[t] != 0;
  a.trk_cnt[((int64_t)wi * a.n_trk + t) * a.n_cut + c] = positive ? 0ull : op_compose(a, a.tab_first[t], n_segs, wk, c);
  if (c == 0) {
    a.ma_len[(int64_t)wi * a.n_trk + t] = m;
    a.score[(int64_t)wi * a.n_trk + t] = positive ? op_score(a, wi, a.seg_first[t], n_segs) : 0.f;
  }
}

// per (window, cutoff) sum over the tracks, in track order
__global__ void __launch_bounds__(256) op_sum_kernel(OpArgs a) {
  const int id = blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= a.pw * a.n_cut) return;
  const int c = id % a.n_cut, wi = a.w0 + id / a.n_cut;
  a.total[(int64_t)wi * a.n_cut + c] = post_sum_rows(a.trk_cnt + (int64_t)wi * a.n_trk * a.n_cut + c, a.n_trk, a.n_cut);
}

// ---- mww_stream_operating_summary
constexpr int OPS_POS = 256;                        // positive tracks per workgroup of ops_positive_kernel (>= the 128 cutoffs)
struct OpsArgs {
  const int* amb;            // [n_amb] the kind-0 tracks, in track order
  const int* pos;            // [n_pos] the kind-1 tracks, in track order
  int n_amb, n_pos, n_pblk;  // n_pblk: workgroups of OPS_POS positive tracks
  int stride;
  double step_s;
  unsigned long long* amb_cnt;   // [n_win][n_amb][n_cut]
  unsigned* part_acc;            // [n_win][n_pblk][n_cut] positive tracks of the workgroup above the cutoff
  unsigned* part_short;          // [n_win][n_pblk] positive tracks of the workgroup without a moving-average value
  unsigned long long* counts;    // the result block: [n_win][n_cut]
  unsigned long long* accepts;   // [n_win][n_cut]
  double* hours;                 // [n_win]
  int64_t* short_tracks;         // [n_win][2]
  int64_t* n_kind;               // [2]
};

// op_compose for the ambient tracks alone: count rows [W][n_ambient][C]
__global__ void __launch_bounds__(256) ops_ambient_kernel(OpArgs a, OpsArgs o) {
  const int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= (int64_t)o.n_amb * a.pw * a.n_cut) return;
  const int c = (int)(id % a.n_cut), wk = (int)(id / a.n_cut % a.pw), j = (int)(id / a.n_cut / a.pw);
  const int wi = a.w0 + wk, t = o.amb[j];
  const int n_segs = (int)((op_len(a, t, wi) + POST_SEG - 1) / POST_SEG);
  o.amb_cnt[((int64_t)wi * o.n_amb + j) * a.n_cut + c] = op_compose(a, a.tab_first[t], n_segs, wk, c);   // table rows: a positive track has none
}

__global__ void __launch_bounds__(OPS_POS) ops_positive_kernel(OpArgs a, OpsArgs o) {
  __shared__ float s_score[OPS_POS];
  __shared__ unsigned s_short[OPS_POS];
  const int blk = blockIdx.x, wi = a.w0 + blockIdx.y, i = threadIdx.x;
  const int first = blk * OPS_POS;
  const int n = o.n_pos - first < OPS_POS ? o.n_pos - first : OPS_POS;
  if (i < n) {
    const int t = o.pos[first + i];
    const int64_t m = op_len(a, t, wi);
    s_score[i] = op_score(a, wi, a.seg_first[t], (int)((m + POST_SEG - 1) / POST_SEG));
    s_short[i] = m == 0;
  }
  __syncthreads();
  if (i < a.n_cut) {
    const double c = a.cut[i];
    unsigned cnt = 0;
    for (int q = 0; q < n; ++q) cnt += (double)s_score[q] > c;   // strict: a score equal to the cutoff is rejected, -inf always
    o.part_acc[((int64_t)wi * o.n_pblk + blk) * a.n_cut + i] = cnt;
  }
  if (i == OPS_POS - 1) {
    unsigned cnt = 0;
    for (int q = 0; q < n; ++q) cnt += s_short[q];
    o.part_short[(int64_t)wi * o.n_pblk + blk] = cnt;
  }
}

// thread (window, cutoff): the two integer sums, in track / workgroup order; the window's thread of cutoff 0: hours and short tracks
__global__ void __launch_bounds__(256) ops_final_kernel(OpArgs a, OpsArgs o) {
  const int id = blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= a.pw * a.n_cut) return;
  const int c = id % a.n_cut, wi = a.w0 + id / a.n_cut;
  unsigned long long acc = 0;
  for (int b = 0; b < o.n_pblk; ++b) acc += o.part_acc[((int64_t)wi * o.n_pblk + b) * a.n_cut + c];
  o.counts[(int64_t)wi * a.n_cut + c] = post_sum_rows(o.amb_cnt + (int64_t)wi * o.n_amb * a.n_cut + c, o.n_amb, a.n_cut);
  o.accepts[(int64_t)wi * a.n_cut + c] = acc;
  if (c != 0) return;
  // streaming.track_hours: h += ((n * stride) * step_s) / 3600.0 in track order, three separate float64 operations
  double h = 0.0;
  int64_t short_amb = 0, short_pos = 0;
  for (int j = 0; j < o.n_amb; ++j) {
#pragma clang fp contract(off)
    const int64_t m = op_len(a, o.amb[j], wi);
    const double prod = (double)(m * (int64_t)o.stride) * o.step_s;
    const double quot = prod / 3600.0;
    h = h + quot;
    short_amb += m == 0;
  }
  for (int b = 0; b < o.n_pblk; ++b) short_pos += o.part_short[(int64_t)wi * o.n_pblk + b];
  o.hours[wi] = h;
  o.short_tracks[2 * wi] = short_amb;
  o.short_tracks[2 * wi + 1] = short_pos;
  if (wi == 0) {
    o.n_kind[0] = o.n_amb;
    o.n_kind[1] = o.n_pos;
  }
}


}  // namespace

extern "C" {

int mww_stream_metrics(mww_stream* s, const int64_t* offsets, const int32_t* kind, int64_t n_tracks, int window, int skip,
                       int cooldown, const double* cutoffs, int n_cutoffs, uint64_t* counts, int64_t* ma_len, float* score) {
  if (!s || !offsets || !kind || !cutoffs || !counts || !ma_len || !score) return mww::set_error(MWW_ERR_INVALID, "null argument");
  const bool args_ok = window > 0 && skip >= 0 && cooldown >= 0 && n_cutoffs > 0 && n_cutoffs <= POST_MAX_CUTOFFS;
  if (int rc = post_check_tracks(s, offsets, kind, n_tracks, args_ok, "bad metric arguments (1.." + std::to_string(POST_MAX_CUTOFFS) + " cutoffs)", false))
    return rc;
  const int64_t* off;
  const int* knd;
  const double* cut;
  unsigned long long *cnt, *tot;
  int64_t* len;
  float* sc;
  PostTable tab;
  tab.add(&off, n_tracks + 1, offsets);
  tab.add(&knd, n_tracks, kind);
  tab.add(&cut, n_cutoffs, cutoffs);
  tab.end_host();
  tab.add(&cnt, n_tracks * n_cutoffs);
  tab.add(&len, n_tracks);
  tab.add(&sc, n_tracks);
  tab.add(&tot, n_cutoffs);
  SCHK(hipSetDevice(s->device));
  if (int rc = tab.commit(&s->post_tab, &s->cap_post_tab, s->stream)) return rc;
  hipLaunchKernelGGL(stream_metrics_kernel, dim3((unsigned)n_tracks), dim3(128), 0, s->stream, (const float*)s->prob, off, knd,
                     (int)n_tracks, window, skip, cooldown, cut, n_cutoffs, cnt, len, sc);
  SCHK(hipGetLastError());
  hipLaunchKernelGGL(stream_counts_sum_kernel, dim3(1), dim3(128), 0, s->stream, (const unsigned long long*)cnt, (int)n_tracks, n_cutoffs, tot);
  SCHK(hipGetLastError());
  SCHK(hipMemcpyAsync(counts, tot, (size_t)n_cutoffs * 8, hipMemcpyDeviceToHost, s->stream));
  SCHK(hipMemcpyAsync(ma_len, len, (size_t)n_tracks * 8, hipMemcpyDeviceToHost, s->stream));
  SCHK(hipMemcpyAsync(score, sc, (size_t)n_tracks * 4, hipMemcpyDeviceToHost, s->stream));
  SCHK(hipStreamSynchronize(s->stream));
  return MWW_OK;
}

int mww_stream_operating_points(mww_stream* s, const int64_t* offsets, const int32_t* kind, int64_t n_tracks, const int32_t* windows,
                                int n_windows, int skip, int cooldown, const double* cutoffs, int n_cutoffs, uint64_t* counts,
                                int64_t* ma_len, float* score) {
  if (!s || !offsets || !kind || !windows || !cutoffs || !counts || !ma_len || !score) return mww::set_error(MWW_ERR_INVALID, "null argument");
  OpCall c;
  if (int rc = c.begin(s, offsets, kind, n_tracks, windows, n_windows, skip, cooldown, cutoffs, n_cutoffs, false)) return rc;
  const int64_t W = n_windows;
  c.tab.end_host();
  c.tab.add(&c.a.total, W * n_cutoffs);
  c.tab.add(&c.a.ma_len, W * n_tracks);
  c.tab.add(&c.a.score, W * n_tracks);
  c.tab.add(&c.a.trk_cnt, W * n_tracks * n_cutoffs);
  if (int rc = c.commit(s)) return rc;
  const int rc = c.passes(s, [&](const OpArgs& a) {
    const int64_t n_thr = n_tracks * a.pw * n_cutoffs;
    hipLaunchKernelGGL(op_track_kernel, dim3((unsigned)((n_thr + 255) / 256)), dim3(256), 0, s->stream, a);
    SCHK(hipGetLastError());
    hipLaunchKernelGGL(op_sum_kernel, dim3((unsigned)((a.pw * n_cutoffs + 255) / 256)), dim3(256), 0, s->stream, a);
    SCHK(hipGetLastError());
    return (int)MWW_OK;
  });
  if (rc) return rc;
  SCHK(hipMemcpyAsync(counts, c.a.total, (size_t)(W * n_cutoffs) * 8, hipMemcpyDeviceToHost, s->stream));
  SCHK(hipMemcpyAsync(ma_len, c.a.ma_len, (size_t)(W * n_tracks) * 8, hipMemcpyDeviceToHost, s->stream));
  SCHK(hipMemcpyAsync(score, c.a.score, (size_t)(W * n_tracks) * 4, hipMemcpyDeviceToHost, s->stream));
  SCHK(hipStreamSynchronize(s->stream));
  return MWW_OK;
}

int mww_stream_operating_summary(mww_stream* s, const int64_t* offsets, const int32_t* kind, int64_t n_tracks, const int32_t* windows,
                                 int n_windows, int skip, int cooldown, const double* cutoffs, int n_cutoffs, int stride, double step_s,
                                 uint64_t* counts, uint64_t* accepts, double* hours, int64_t* short_tracks, int64_t* n_kind) {
  if (!s || !offsets || !kind || !windows || !cutoffs || !counts || !accepts || !hours || !short_tracks || !n_kind)
    return mww::set_error(MWW_ERR_INVALID, "null argument");
  if (stride < 1 || !(step_s > 0)) return mww::set_error(MWW_ERR_INVALID, "bad operating-summary arguments (stride >= 1, step_s > 0)");
  OpCall c;
  if (int rc = c.begin(s, offsets, kind, n_tracks, windows, n_windows, skip, cooldown, cutoffs, n_cutoffs, true)) return rc;
  std::vector<int32_t> amb, pos;
  for (int64_t t = 0; t < n_tracks; ++t) (kind[t] ? pos : amb).push_back((int32_t)t);
  const int64_t n_amb = (int64_t)amb.size(), n_pos = (int64_t)pos.size(), n_pblk = (n_pos + OPS_POS - 1) / OPS_POS;
  const int64_t W = n_windows, C = n_cutoffs;
  // inputs, then the result block (counts, accepts, hours, short_tracks, n_kind: contiguous, read back in one copy), then scratch
  OpsArgs o{};
  char* res;
  c.tab.add(&o.amb, n_amb, amb.data());
  c.tab.add(&o.pos, n_pos, pos.data());
  c.tab.add(&c.a.tab_first, n_tracks + 1, c.plan.tab_first.data());   // table rows for the ambient tracks' segments alone
  c.tab.end_host();
  const int64_t r_cnt = 0, r_acc = r_cnt + W * C * 8, r_hours = r_acc + W * C * 8, r_short = r_hours + W * 8, r_kind = r_short + W * 16,
                r_bytes = r_kind + 16;
  c.tab.add(&res, r_bytes);
  c.tab.add(&o.amb_cnt, W * n_amb * C);
  c.tab.add(&o.part_acc, W * n_pblk * C);
  c.tab.add(&o.part_short, W * n_pblk);
  if (int rc = c.commit(s)) return rc;
  o.n_amb = (int)n_amb;
  o.n_pos = (int)n_pos;
  o.n_pblk = (int)n_pblk;
  o.stride = stride;
  o.step_s = step_s;
  o.counts = reinterpret_cast<unsigned long long*>(res + r_cnt);
  o.accepts = reinterpret_cast<unsigned long long*>(res + r_acc);
  o.hours = reinterpret_cast<double*>(res + r_hours);
  o.short_tracks = reinterpret_cast<int64_t*>(res + r_short);
  o.n_kind = reinterpret_cast<int64_t*>(res + r_kind);
  const int rc = c.passes(s, [&](const OpArgs& a) {
    if (n_amb) {
      const int64_t n_thr = n_amb * a.pw * C;
      hipLaunchKernelGGL(ops_ambient_kernel, dim3((unsigned)((n_thr + 255) / 256)), dim3(256), 0, s->stream, a, o);
      SCHK(hipGetLastError());
    }
    if (n_pos) {
      hipLaunchKernelGGL(ops_positive_kernel, dim3((unsigned)n_pblk, (unsigned)a.pw), dim3(OPS_POS), 0, s->stream, a, o);
      SCHK(hipGetLastError());
    }
    hipLaunchKernelGGL(ops_final_kernel, dim3((unsigned)((a.pw * C + 255) / 256)), dim3(256), 0, s->stream, a, o);
    SCHK(hipGetLastError());
    return (int)MWW_OK;
  });
  if (rc) return rc;
  std::vector<char> r((size_t)r_bytes);
  SCHK(hipMemcpyAsync(r.data(), res, (size_t)r_bytes, hipMemcpyDeviceToHost, s->stream));   // W * C * 16 + W * 24 + 16 bytes
  SCHK(hipStreamSynchronize(s->stream));
  std::memcpy(counts, &r[r_cnt], (size_t)(W * C) * 8);
  std::memcpy(accepts, &r[r_acc], (size_t)(W * C) * 8);
  std::memcpy(hours, &r[r_hours], (size_t)W * 8);
  std::memcpy(short_tracks, &r[r_short], (size_t)W * 16);
  std::memcpy(n_kind, &r[r_kind], 16);
  return MWW_OK;
}

}  // extern "C"
