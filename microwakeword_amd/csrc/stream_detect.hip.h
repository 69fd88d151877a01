// The detection launches shared by mww_stream_detections (tu_stream_detect.hip) and mww_stream_mine (tu_stream_mine.hip).
// mww_stream_detections (include/mww.h): WHERE the moving average of the probabilities a stream holds crosses one
// cutoff, in the cooldown semantics of test.py:119-135, and which moving-average index gives a positive track its score.
//
// The cooldown walk is the only sequential part, and it is cut into segments of DET_SEG moving-average values:
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
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "stream_common.hip.h"

using namespace mww_stream_impl;

namespace {

constexpr int DET_THREADS = 256;
constexpr int DET_ITEMS = 4;
constexpr int DET_SEG = DET_THREADS * DET_ITEMS;   // 1024 moving-average values per segment (tests/stream_detect_checks.py names it)

struct DetArgs {
  const float* prob;
  const int64_t* off;       // [n_trk + 1]
  const int* kind;          // [n_trk]
  const int* seg_first;     // [n_trk + 1] first segment of each track
  int n_trk, n_seg;
  int win, skip;
  int cdp;                  // max(cooldown, 1): distance from an accept to the next index that may be accepted
  int first_ok;             // max(cooldown - 1, 0): the first index of a track that may be accepted
  int n_entry;              // min(cdp, DET_SEG): entry states a segment tabulates
  double cutoff;
  unsigned short* cand;     // [n_seg][DET_SEG] candidate offsets of each segment, ascending
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

// the moving average of mww_stream_metrics: float32 sum in order, then one division
__device__ __forceinline__ float det_avg(const float* p, int win) {
  float s = 0.f;
  for (int k = 0; k < win; ++k) s += p[k];
  return s / (float)win;
}

// track of segment `seg`: the last t with seg_first[t] <= seg (tracks without a segment share their successor's entry)
__device__ __forceinline__ int det_track_of(const int* seg_first, int n_trk, int seg) {
  int lo = 0, hi = n_trk;   // seg_first[lo] <= seg < seg_first[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (seg_first[mid] <= seg) lo = mid; else hi = mid;
  }
  return lo;
}

struct DetSeg {
  int t;
  int64_t b;     // first probability of the track's moving-average sequence (after the skip of a positive track)
  int64_t i0;    // first moving-average index of the segment
  int len;       // values in the segment (1 .. DET_SEG)
  int kind;
};

__device__ __forceinline__ DetSeg det_segment(const DetArgs& a, int seg) {
  DetSeg g;
  g.t = det_track_of(a.seg_first, a.n_trk, seg);
  g.kind = a.kind[g.t];
  const int64_t sk = g.kind ? a.skip : 0;
  const int64_t n = a.off[g.t + 1] - a.off[g.t] - sk;   // >= win: the track has a segment
  const int64_t m = n - a.win + 1;
  g.b = a.off[g.t] + sk;
  g.i0 = (int64_t)(seg - a.seg_first[g.t]) * DET_SEG;
  g.len = (int)(m - g.i0 < DET_SEG ? m - g.i0 : DET_SEG);
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
    while (next < DET_SEG) {
      p += det_lower_bound(cand + p, n_cand - p, next);
      if (p >= n_cand) break;
      if (acc) acc[cnt] = cand[p];
      ++cnt;
      next = (int64_t)cand[p] + cdp;
      ++p;
    }
  }
  *exit_state = next > DET_SEG ? (int)(next - DET_SEG) : 0;
  return cnt;
}

__global__ void __launch_bounds__(DET_THREADS) detect_segment_kernel(DetArgs a) {
  __shared__ int s_scan[DET_THREADS];
  __shared__ unsigned short s_cand[DET_SEG];
  __shared__ float s_best[DET_THREADS];
  __shared__ int s_bidx[DET_THREADS];
  const int seg = blockIdx.x, j = threadIdx.x;
  if (seg >= a.n_seg) return;
  const DetSeg g = det_segment(a, seg);
  const float* p = a.prob + g.b + g.i0;
  float avg[DET_ITEMS];
  for (int k = 0; k < DET_ITEMS; ++k) {
    const int o = j * DET_ITEMS + k;
    avg[k] = o < g.len ? det_avg(p + o, a.win) : 0.f;
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
    unsigned short* gc = a.cand + (int64_t)seg * DET_SEG;
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
      if (state >= DET_SEG) {   // still cooling down beyond this segment
        a.seg_entry[s] = DET_SEG;
        state -= DET_SEG;
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
  __shared__ unsigned short s_cand[DET_SEG];
  __shared__ unsigned short s_acc[DET_SEG];
  __shared__ int s_n;
  const int seg = blockIdx.x, j = threadIdx.x;
  if (seg >= a.n_seg) return;
  const DetSeg g = det_segment(a, seg);
  if (g.kind != 0) return;
  const int entry = a.seg_entry[seg];
  const int64_t base = a.trk_base[g.t] + a.seg_base[seg];
  const int n_cand = a.seg_ncand[seg];
  if (entry >= DET_SEG || n_cand == 0 || base >= a.capacity) return;   // uniform over the workgroup
  const unsigned short* gc = a.cand + (int64_t)seg * DET_SEG;
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
    d.average = det_avg(a.prob + g.b + g.i0 + o, a.win);
    d.reserved2 = 0.f;
    a.out[base + q] = d;
  }
}

// The segment, track and scan launches of one call on the probabilities `s` holds: after them every event's position is fixed
// (a->trk_count, a->trk_base, the segments' entry states) and nothing is written yet.  `kind` null: every track is ambient.
inline int det_locate(mww_stream* s, const int64_t* offsets, const int32_t* kind, int64_t n_tracks, int window, int skip, int cooldown,
                      double cutoff, DetArgs* out) {
  if (n_tracks <= 0 || n_tracks > INT32_MAX || window <= 0 || skip < 0 || cooldown < 0)
    return mww::set_error(MWW_ERR_INVALID, "bad detection arguments");
  if (offsets[0] < 0 || offsets[n_tracks] > s->n_out) return mww::set_error(MWW_ERR_INVALID, "track offsets exceed the probabilities held");
  for (int64_t t = 0; t < n_tracks; ++t)
    if (offsets[t + 1] < offsets[t]) return mww::set_error(MWW_ERR_INVALID, "track offsets must not decrease");
  for (int64_t t = 0; kind && t < n_tracks; ++t)
    if (kind[t] != 0 && kind[t] != 1) return mww::set_error(MWW_ERR_INVALID, "track kind must be 0 (ambient) or 1 (positive)");
  std::vector<int32_t> seg_first((size_t)n_tracks + 1);
  int64_t n_seg = 0;
  for (int64_t t = 0; t < n_tracks; ++t) {
    seg_first[(size_t)t] = (int32_t)n_seg;
    const int64_t n = offsets[t + 1] - offsets[t] - (kind && kind[t] ? skip : 0);
    const int64_t m = n >= window ? n - window + 1 : 0;
    n_seg += (m + DET_SEG - 1) / DET_SEG;
    if (n_seg > INT32_MAX) return mww::set_error(MWW_ERR_INVALID, "too many probabilities for one call");
  }
  seg_first[(size_t)n_tracks] = (int32_t)n_seg;
  const int cdp = std::max(cooldown, 1), n_entry = std::min(cdp, DET_SEG);
  auto al = [](int64_t b) { return (b + 255) & ~(int64_t)255; };
  // inputs, per-track results, per-segment results: one table
  const int64_t o_off = 0, o_kind = al((n_tracks + 1) * 8), o_sf = al(o_kind + n_tracks * 4), o_in_end = al(o_sf + (n_tracks + 1) * 4),
                o_cnt = o_in_end, o_base = al(o_cnt + n_tracks * 8), o_bidx = al(o_base + (n_tracks + 1) * 8),
                o_sc = al(o_bidx + n_tracks * 8), o_nc = al(o_sc + n_tracks * 4), o_ent = al(o_nc + n_seg * 4),
                o_sbase = al(o_ent + n_seg * 4), o_sbest = al(o_sbase + n_seg * 8), o_sbidx = al(o_sbest + n_seg * 4),
                bytes = al(o_sbidx + n_seg * 8);
  // candidates and transfer tables: sized from this call's segments and cooldown
  const int64_t c_cand = 0, c_exit = al(n_seg * DET_SEG * 2), c_tcnt = al(c_exit + n_seg * n_entry * 4),
                c_bytes = al(c_tcnt + n_seg * n_entry * 4);
  SCHK(hipSetDevice(s->device));
  int rc = grow(&s->det_tab, &s->cap_det_tab, bytes);
  if (!rc) rc = grow(&s->det_cand, &s->cap_det_cand, c_bytes);
  if (rc) return rc;
  std::vector<char> h((size_t)o_in_end, 0);
  std::memcpy(&h[o_off], offsets, (size_t)(n_tracks + 1) * 8);
  if (kind) std::memcpy(&h[o_kind], kind, (size_t)n_tracks * 4);
  std::memcpy(&h[o_sf], seg_first.data(), (size_t)(n_tracks + 1) * 4);
  SCHK(hipMemcpyAsync(s->det_tab, h.data(), (size_t)o_in_end, hipMemcpyHostToDevice, s->stream));
  DetArgs a{};
  a.prob = s->prob;
  a.off = reinterpret_cast<const int64_t*>(s->det_tab + o_off);
  a.kind = reinterpret_cast<const int*>(s->det_tab + o_kind);
  a.seg_first = reinterpret_cast<const int*>(s->det_tab + o_sf);
  a.n_trk = (int)n_tracks;
  a.n_seg = (int)n_seg;
  a.win = window;
  a.skip = skip;
  a.cdp = cdp;
  a.first_ok = std::max(cooldown - 1, 0);
  a.n_entry = n_entry;
  a.cutoff = cutoff;
  a.cand = reinterpret_cast<unsigned short*>(s->det_cand + c_cand);
  a.tab_exit = reinterpret_cast<int*>(s->det_cand + c_exit);
  a.tab_cnt = reinterpret_cast<int*>(s->det_cand + c_tcnt);
  a.seg_ncand = reinterpret_cast<int*>(s->det_tab + o_nc);
  a.seg_entry = reinterpret_cast<int*>(s->det_tab + o_ent);
  a.seg_base = reinterpret_cast<int64_t*>(s->det_tab + o_sbase);
  a.seg_best = reinterpret_cast<float*>(s->det_tab + o_sbest);
  a.seg_bidx = reinterpret_cast<int64_t*>(s->det_tab + o_sbidx);
  a.trk_count = reinterpret_cast<int64_t*>(s->det_tab + o_cnt);
  a.trk_base = reinterpret_cast<int64_t*>(s->det_tab + o_base);
  a.trk_bidx = reinterpret_cast<int64_t*>(s->det_tab + o_bidx);
  a.trk_score = reinterpret_cast<float*>(s->det_tab + o_sc);
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
