// The detection launches shared by mww_stream_detections (tu_stream_detect.hip) and mww_stream_mine (tu_stream_mine.hip).
// mww_stream_detections (include/mww.h): WHERE the moving average of the probabilities a stream holds crosses one
// cutoff, in the cooldown semantics of test.py:119-135, and which moving-average index gives a positive track its score.
//
// The moving average, the values of a track, the segment plan and the table packing are those of stream_post.hip.h.
//
// The cooldown walk is the only sequential part, and it is cut into segments of POST_SEG moving-average values:
//   detect_segment_kernel  one workgroup per segment: moving averages and candidate flags (avg > cutoff) in parallel, the
//                          candidate offsets compacted IN INDEX ORDER by an LDS prefix scan over the threads' counts (thread j
//                          owns the DET_ITEMS consecutive values j * DET_ITEMS ..., so position = values before it: no atomic
//                          decides a position).  The walk's state at a segment boundary is (next_ok - segment start), which
//                          lies in [0, max(cooldown, 1)): the workgroup tabulates, for each such entry state, the accepts
//                          of this segment and the exit state.  A positive track's segment reduces (max, first index).
//   detect_track_kernel    one thread per track: composes the segments' tables in order (one dependent load per segment, not
//                          per value or per candidate) -> each segment's entry state and first event, the track's count; for
//                          positive tracks the maximum over the segments in order.
//   detect_scan_kernel     exclusive scan of the track counts in track order -> where a track's events start, and the total.
//   detect_write_kernel    one workgroup per segment again: walks its candidates from its entry state and writes its events
//                          (track, index, average) at the positions the scans fixed, below `capacity`.
// Every position is a function of the data alone, so two runs write the same bytes.
#pragma once
#include "stream_post.hip.h"

namespace {

constexpr int DET_THREADS = 256;
constexpr int DET_ITEMS = 4;
static_assert(DET_THREADS * DET_ITEMS == POST_SEG, "thread j owns the DET_ITEMS consecutive values of a segment from j * DET_ITEMS");

struct DetArgs {
  const float* prob;
  const int64_t* off;       // [n_trk + 1]
  const int* kind;          // [n_trk]
  const int* seg_first;     // [n_trk + 1] first segment of each track
  int n_trk, n_seg;
  int win, skip;
  int cdp;                  // max(cooldown, 1): distance from an accept to the next index that may be accepted
  int first_ok;             // max(cooldown - 1, 0): the first index of a track that may be accepted
  int n_entry;              // min(cdp, POST_SEG): entry states a segment tabulates
  double cutoff;
  unsigned short* cand;     // [n_seg][POST_SEG] candidate offsets of each segment, ascending
  int* seg_ncand;           // [n_seg]
  int* tab_exit;            // [n_seg][n_entry]
  int* tab_cnt;             // [n_seg][n_entry]
  float* seg_best;          // [n_seg] positive tracks: the segment's maximum ...
  int64_t* seg_bidx;        // [n_seg] ... and the first index that attains it (-1: none)
  int* seg_entry;           // [n_seg] entry state of the segment in the track's walk
  int64_t* seg_base;        // [n_seg] events of the track before this segment
  int64_t* trk_count;       // [n_trk]
  int64_t* trk_base;        // [n_trk + 1] events before the track; [n_trk] the total
  int64_t* trk_bidx;        // [n_trk]
  float* trk_score;         // [n_trk]
  mww_detection* out;
  int64_t capacity;
};

struct DetSeg {
  int t;
  int64_t b;     // first probability of the track's moving-average sequence (after the skip of a positive track)
  int64_t i0;    // first moving-average index of the segment
  int len;       // values in the segment (1 .. POST_SEG)
  int kind;
};

__device__ __forceinline__ DetSeg det_segment(const DetArgs& a, int seg) {
  DetSeg g;
  g.t = post_track_of(a.seg_first, a.n_trk, seg);
  g.kind = a.kind[g.t];
  const PostValues v = post_values(a.off, a.kind, a.skip, g.t, a.win);   // m > 0: the track has a segment
  g.b = v.b;
  g.i0 = (int64_t)(seg - a.seg_first[g.t]) * POST_SEG;
  g.len = (int)(v.m - g.i0 < POST_SEG ? v.m - g.i0 : POST_SEG);
  return g;
}

// first position in the ascending list cand[0..n) whose offset is >= x
__device__ __forceinline__ int det_lower_bound(const unsigned short* cand, int n, int64_t x) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if ((int64_t)cand[mid] < x) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// The closed-form walk over one segment's candidates from entry state `entry` (offset of next_ok from the segment start):
// accepts the first candidate >= next_ok, then next_ok = that + cdp.  Returns the accepts, *exit_state = next_ok relative to
// the next segment (floor 0); acc (may be null) receives the accepted offsets.
__device__ __forceinline__ int det_walk(const unsigned short* cand, int n_cand, int64_t entry, int cdp, int* exit_state, unsigned short* acc) {
  int64_t next = entry;
  int cnt = 0;
  if (cdp == 1) {   // every candidate from next_ok on
    const int p = det_lower_bound(cand, n_cand, next);
    cnt = n_cand - p;
    if (acc)
      for (int j = 0; j < cnt; ++j) acc[j] = cand[p + j];
    if (cnt) next = (int64_t)cand[n_cand - 1] + 1;
  } else {
    int p = 0;
    while (next < POST_SEG) {
      p += det_lower_bound(cand + p, n_cand - p, next);
      if (p >= n_cand) break;
      if (acc) acc[cnt] = cand[p];
      ++cnt;
      next = (int64_t)cand[p] + cdp;
      ++p;
    }
  }
  *exit_state = next > POST_SEG ? (int)(next - POST_SEG) : 0;
  return cnt;
}

__global__ void __launch_bounds__(DET_THREADS) detect_segment_kernel(DetArgs a) {
  __shared__ int s_scan[DET_THREADS];
  __shared__ unsigned short s_cand[POST_SEG];
  __shared__ float s_best[DET_THREADS];
  __shared__ int s_bidx[DET_THREADS];
  const int seg = blockIdx.x, j = threadIdx.x;
  if (seg >= a.n_seg) return;
  const DetSeg g = det_segment(a, seg);
  const float* p = a.prob + g.b + g.i0;
  float avg[DET_ITEMS];
  for (int k = 0; k < DET_ITEMS; ++k) {
    const int o = j * DET_ITEMS + k;
    avg[k] = o < g.len ? post_avg(p + o, a.win) : 0.f;
  }
  if (g.kind == 0) {
    bool flag[DET_ITEMS];
    int mine = 0;
    for (int k = 0; k < DET_ITEMS; ++k) {
      flag[k] = j * DET_ITEMS + k < g.len && (double)avg[k] > a.cutoff;
      mine += flag[k];
    }
    // inclusive scan of the threads' counts, in thread order
    s_scan[j] = mine;
    __syncthreads();
    for (int d = 1; d < DET_THREADS; d <<= 1) {
      const int add = j >= d ? s_scan[j - d] : 0;
      __syncthreads();
      s_scan[j] += add;
      __syncthreads();
    }
    int at = s_scan[j] - mine;
    const int n_cand = s_scan[DET_THREADS - 1];
    for (int k = 0; k < DET_ITEMS; ++k)
      if (flag[k]) s_cand[at++] = (unsigned short)(j * DET_ITEMS + k);
    __syncthreads();
    unsigned short* gc = a.cand + (int64_t)seg * POST_SEG;
    for (int q = j; q < n_cand; q += DET_THREADS) gc[q] = s_cand[q];
    if (j == 0) a.seg_ncand[seg] = n_cand;
    for (int e = j; e < a.n_entry; e += DET_THREADS) {
      int ex;
      a.tab_cnt[(int64_t)seg * a.n_entry + e] = det_walk(s_cand, n_cand, e, a.cdp, &ex, nullptr);
      a.tab_exit[(int64_t)seg * a.n_entry + e] = ex;
    }
  } else {
    float best = -INFINITY;
    int bi = -1;
    for (int k = 0; k < DET_ITEMS; ++k)
      if (j * DET_ITEMS + k < g.len && avg[k] > best) { best = avg[k]; bi = j * DET_ITEMS + k; }
    s_best[j] = best;
    s_bidx[j] = bi;
    __syncthreads();
    for (int d = DET_THREADS >> 1; d > 0; d >>= 1) {   // a tie goes to the smaller offset (an offset of -1 holds -inf: never a tie with a value)
      if (j < d && (s_best[j + d] > s_best[j] || (s_best[j + d] == s_best[j] && s_bidx[j + d] < s_bidx[j]))) {
        s_best[j] = s_best[j + d];
        s_bidx[j] = s_bidx[j + d];
      }
      __syncthreads();
    }
    if (j == 0) {
      a.seg_best[seg] = s_best[0];
      a.seg_bidx[seg] = s_bidx[0] >= 0 ? g.i0 + s_bidx[0] : -1;
    }
  }
}

__global__ void __launch_bounds__(64) detect_track_kernel(DetArgs a) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= a.n_trk) return;
  const int s0 = a.seg_first[t], s1 = a.seg_first[t + 1];
  if (a.kind[t] == 0) {
    int64_t state = a.first_ok, total = 0;
    for (int s = s0; s < s1; ++s) {
      a.seg_base[s] = total;
      if (state >= POST_SEG) {   // still cooling down beyond this segment
        a.seg_entry[s] = POST_SEG;
        state -= POST_SEG;
      } else {
        a.seg_entry[s] = (int)state;
        total += a.tab_cnt[(int64_t)s * a.n_entry + state];
        state = a.tab_exit[(int64_t)s * a.n_entry + state];
      }
    }
    a.trk_count[t] = total;
    a.trk_bidx[t] = -1;
    a.trk_score[t] = 0.f;
  } else {
    float best = -INFINITY;
    int64_t bi = -1;
    for (int s = s0; s < s1; ++s)
      if (a.seg_best[s] > best) { best = a.seg_best[s]; bi = a.seg_bidx[s]; }
    a.trk_count[t] = 0;
    a.trk_bidx[t] = bi;
    a.trk_score[t] = best;
  }
}

// exclusive scan in track order: thread j sums its contiguous chunk, the chunk sums are scanned in LDS
__global__ void __launch_bounds__(DET_THREADS) detect_scan_kernel(DetArgs a) {
  __shared__ long long s_sum[DET_THREADS];
  const int j = threadIdx.x;
  const int chunk = (a.n_trk + DET_THREADS - 1) / DET_THREADS;
  const int t0 = min(j * chunk, a.n_trk), t1 = min(t0 + chunk, a.n_trk);
  long long mine = 0;
  for (int t = t0; t < t1; ++t) mine += a.trk_count[t];
  s_sum[j] = mine;
  __syncthreads();
  for (int d = 1; d < DET_THREADS; d <<= 1) {
    const long long add = j >= d ? s_sum[j - d] : 0;
    __syncthreads();
    s_sum[j] += add;
    __syncthreads();
  }
  long long at = s_sum[j] - mine;
  for (int t = t0; t < t1; ++t) {
    a.trk_base[t] = at;
    at += a.trk_count[t];
  }
  if (j == DET_THREADS - 1) a.trk_base[a.n_trk] = s_sum[j];
}

__global__ void __launch_bounds__(DET_THREADS) detect_write_kernel(DetArgs a) {
  __shared__ unsigned short s_cand[POST_SEG];
  __shared__ unsigned short s_acc[POST_SEG];
  __shared__ int s_n;
  const int seg = blockIdx.x, j = threadIdx.x;
  if (seg >= a.n_seg) return;
  const DetSeg g = det_segment(a, seg);
  if (g.kind != 0) return;
  const int entry = a.seg_entry[seg];
  const int64_t base = a.trk_base[g.t] + a.seg_base[seg];
  const int n_cand = a.seg_ncand[seg];
  if (entry >= POST_SEG || n_cand == 0 || base >= a.capacity) return;   // uniform over the workgroup
  const unsigned short* gc = a.cand + (int64_t)seg * POST_SEG;
  for (int q = j; q < n_cand; q += DET_THREADS) s_cand[q] = gc[q];
  __syncthreads();
  if (j == 0) {
    int ex;
    s_n = det_walk(s_cand, n_cand, entry, a.cdp, &ex, s_acc);
  }
  __syncthreads();
  const int n = s_n;
  for (int q = j; q < n; q += DET_THREADS) {
    if (base + q >= a.capacity) break;
    const int o = s_acc[q];
    mww_detection d;
    d.track = g.t;
    d.reserved = 0;
    d.index = g.i0 + o;
    d.average = post_avg(a.prob + g.b + g.i0 + o, a.win);
    d.reserved2 = 0.f;
    a.out[base + q] = d;
  }
}

// The segment, track and scan launches of one call on the probabilities `s` holds: after them every event's position is fixed
// (a->trk_count, a->trk_base, the segments' entry states) and nothing is written yet.  `kind` null: every track is ambient.
inline int det_locate(mww_stream* s, const int64_t* offsets, const int32_t* kind, int64_t n_tracks, int window, int skip, int cooldown,
                      double cutoff, DetArgs* out) {
  if (int rc = post_check_tracks(s, offsets, kind, n_tracks, window > 0 && skip >= 0 && cooldown >= 0, "bad detection arguments", true)) return rc;
  PostPlan plan;
  if (int rc = post_plan(offsets, kind, n_tracks, skip, window, false, &plan)) return rc;
  const int64_t n_seg = plan.n_seg;
  const int cdp = std::max(cooldown, 1), n_entry = std::min(cdp, POST_SEG);
  DetArgs a{};
  // inputs, per-track results, per-segment results: one table
  PostTable tab;
  tab.add(&a.off, n_tracks + 1, offsets);
  tab.add(&a.kind, n_tracks, kind);
  tab.add(&a.seg_first, n_tracks + 1, plan.seg_first.data());
  tab.end_host();
  tab.add(&a.trk_count, n_tracks);
  tab.add(&a.trk_base, n_tracks + 1);
  tab.add(&a.trk_bidx, n_tracks);
  tab.add(&a.trk_score, n_tracks);
  tab.add(&a.seg_ncand, n_seg);
  tab.add(&a.seg_entry, n_seg);
  tab.add(&a.seg_base, n_seg);
  tab.add(&a.seg_best, n_seg);
  tab.add(&a.seg_bidx, n_seg);
  // candidates and transfer tables: sized from this call's segments and cooldown
  PostTable scr;
  scr.add(&a.cand, n_seg * POST_SEG);
  scr.add(&a.tab_exit, n_seg * n_entry);
  scr.add(&a.tab_cnt, n_seg * n_entry);
  SCHK(hipSetDevice(s->device));
  int rc = tab.commit(&s->post_tab, &s->cap_post_tab, s->stream);
  if (!rc) rc = scr.commit(&s->post_scr, &s->cap_post_scr, s->stream);
  if (rc) return rc;
  a.prob = s->prob;
  a.n_trk = (int)n_tracks;
  a.n_seg = (int)n_seg;
  a.win = window;
  a.skip = skip;
  a.cdp = cdp;
  a.first_ok = std::max(cooldown - 1, 0);
  a.n_entry = n_entry;
  a.cutoff = cutoff;
  a.out = nullptr;
  a.capacity = 0;
  if (n_seg) {
    hipLaunchKernelGGL(detect_segment_kernel, dim3((unsigned)n_seg), dim3(DET_THREADS), 0, s->stream, a);
    SCHK(hipGetLastError());
  }
  hipLaunchKernelGGL(detect_track_kernel, dim3((unsigned)((n_tracks + 63) / 64)), dim3(64), 0, s->stream, a);
  SCHK(hipGetLastError());
  hipLaunchKernelGGL(detect_scan_kernel, dim3(1), dim3(DET_THREADS), 0, s->stream, a);
  SCHK(hipGetLastError());
  *out = a;
  return MWW_OK;
}

// The write launch: the first `n_write` (> 0) events of the located call into s->det_out, grown on demand
inline int det_events(mww_stream* s, DetArgs* a, int64_t n_write) {
  const int rc = grow(&s->det_out, &s->cap_det_out, n_write);
  if (rc) return rc;
  a->out = s->det_out;
  a->capacity = n_write;
  hipLaunchKernelGGL(detect_write_kernel, dim3((unsigned)a->n_seg), dim3(DET_THREADS), 0, s->stream, *a);
  SCHK(hipGetLastError());
  return MWW_OK;
}

}  // namespace
