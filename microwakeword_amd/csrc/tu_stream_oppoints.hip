// mww_stream_operating_points (include/mww.h): the false-accept counts of every (window, cutoff) pair and the
// positive scores of every window in one call, on the probabilities a stream holds.  Row k is mww_stream_metrics at windows[k].
//
// The cooldown walk is cut into segments of OP_SEG moving-average values, as in tu_stream_detect.hip, and the work is parallel
// over (segment, window):
//   op_segment_kernel  one workgroup per (segment, window): stages the OP_SEG + w - 1 probabilities in LDS once, forms the
//                      averages there (the expression of the metrics kernel), and thread j < n_cutoffs builds cutoff j's
//                      transfer table from them: entry state e (next_ok - segment start) -> (accepts, last accepted offset).
//                      One BACKWARD sweep serves all entry states: F(i), the walk that enters with next_ok = i, is
//                      F(i + 1) when i is no candidate and 1 + F(i + cdp) when it is, so a ring of cdp slots (slot i mod cdp
//                      holds F(i + cdp) until F(i) replaces it) ends holding F(0 .. cdp - 1): the table.  A positive track's
//                      segment reduces its maximum instead.
//   op_track_kernel    one thread per (track, window, cutoff): composes the tables in segment order, one dependent load per
//                      segment; thread 0 of a (track, window) takes the length and the positive score (segments in order).
//   op_sum_kernel      one thread per (window, cutoff): the tracks' counts summed in track order.
// The tables of `pw` windows are resident at a time (OP_SCRATCH bytes at most, one window at least): the windows run in passes.
// Nothing depends on an arrival order, so two calls write the same bytes.
//
// mww_stream_operating_summary is the same grid reduced on the device to what a choice of operating point reads:
// per (window, cutoff) the ambient count and the number of positive tracks accepted, per window the ambient hours and the
// tracks without a value.  It shares op_segment_kernel; the tables have rows for the ambient tracks' segments alone (tab_first:
// a positive track's segment only reduces its maximum), so their size does not grow with the positives.  What follows differs:
//   ops_ambient_kernel   op_track_kernel's walk for the kind-0 tracks alone: one thread per (ambient track, window, cutoff),
//                        count rows [W][n_ambient][C].  A positive track has no thread and no row here.
//   ops_positive_kernel  one workgroup per (OPS_POS positive tracks, window): thread i takes track i's score (its segments'
//                        maxima in order) into LDS, then thread c counts the scores above cutoff c: an integer partial per
//                        (window, workgroup, cutoff), and the workgroup's tracks without a value.
//   ops_final_kernel     one thread per (window, cutoff) sums the ambient rows in track order and the partials in workgroup
//                        order; one thread per window walks the ambient tracks in order for the hours (float64: product,
//                        division, add, uncontracted) and the short-track counts.
// Every sum is an integer sum in a fixed order (no atomics), the hours a serial float64 sum: two calls write the same bytes.
// The host reads back the result block alone: W * C * 16 + W * 24 + 16 bytes.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "stream_common.hip.h"

using namespace mww_stream_impl;

namespace {

constexpr int OP_THREADS = 128;                     // >= the 128 cutoffs of a call: one thread per cutoff
constexpr int OP_SEG = 1024;                        // moving-average values per segment (tests/operating_point_checks.py names it)
constexpr int OP_CNT_BITS = 11;                     // a table entry: accepts (<= OP_SEG) | last accepted offset << OP_CNT_BITS
constexpr int64_t OP_SCRATCH = (int64_t)96 << 20;   // transfer tables resident at a time
constexpr int OP_RING_LDS = 32 * 1024;              // a ring of n_cutoffs * n_entry words up to this size lives in LDS
constexpr int OPS_POS = 256;                        // positive tracks per workgroup of ops_positive_kernel (>= the 128 cutoffs)

struct OpArgs {
  const float* prob;
  const int64_t* off;        // [n_trk + 1]
  const int* kind;           // [n_trk]
  const int* seg_first;      // [n_trk + 1] first segment of each track (segments of the smallest window: the most)
  const int* tab_first;      // [n_trk] table row of a track's first segment: seg_first, or (the summary) the ambient tracks' segments alone
  const int* win;            // [n_win]
  const double* cut;         // [n_cut]
  int n_trk, n_seg, n_cut;
  int skip;
  int cdp;                   // max(cooldown, 1): distance from an accept to the next index that may be accepted
  int first_ok;              // max(cooldown - 1, 0): the first index of a track that may be accepted
  int n_entry;               // min(cdp, OP_SEG): entry states a segment tabulates = slots of the ring
  int w0, pw;                // this pass: windows w0 .. w0 + pw - 1
  int ring_lds;              // the ring is in LDS (else it is the table itself)
  unsigned* tab;             // [table rows][pw][n_entry][n_cut]
  float* seg_best;           // [n_win][n_seg] positive tracks: the segment's maximum
  unsigned long long* trk_cnt;   // [n_win][n_trk][n_cut]
  int64_t* ma_len;           // [n_win][n_trk]
  float* score;              // [n_win][n_trk]
  unsigned long long* total; // [n_win][n_cut]
};

// track of segment `seg`: the last t with seg_first[t] <= seg (tracks without a segment share their successor's entry)
__device__ __forceinline__ int op_track_of(const int* seg_first, int n_trk, int seg) {
  int lo = 0, hi = n_trk;   // seg_first[lo] <= seg < seg_first[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (seg_first[mid] <= seg) lo = mid; else hi = mid;
  }
  return lo;
}

// moving-average values of track t at window w (after the skip of a positive track); *b: its first probability
__device__ __forceinline__ int64_t op_values(const OpArgs& a, int t, int w, int64_t* b) {
  const int64_t sk = a.kind[t] ? a.skip : 0;
  const int64_t n = a.off[t + 1] - a.off[t] - sk;
  *b = a.off[t] + sk;
  return n >= w ? n - w + 1 : 0;
}

__global__ void __launch_bounds__(OP_THREADS) op_segment_kernel(OpArgs a) {
  __shared__ float s_p[OP_SEG + MWW_OP_MAX_WINDOW - 1];
  __shared__ float s_avg[OP_SEG];
  __shared__ float s_best[OP_THREADS];
  HIP_DYNAMIC_SHARED(unsigned, s_ring)
  const int seg = blockIdx.x, wk = blockIdx.y, j = threadIdx.x;
  const int w = a.win[a.w0 + wk];
  const int t = op_track_of(a.seg_first, a.n_trk, seg);
  int64_t b;
  const int64_t m = op_values(a, t, w, &b);
  const int64_t i0 = (int64_t)(seg - a.seg_first[t]) * OP_SEG;
  if (m <= i0) return;   // this window has fewer segments than the smallest one (uniform over the workgroup)
  const int len = (int)(m - i0 < OP_SEG ? m - i0 : OP_SEG);
  const float* p = a.prob + b + i0;
  for (int q = j; q < len + w - 1; q += OP_THREADS) s_p[q] = p[q];   // ends at the track's last probability
  __syncthreads();
  for (int q = j; q < len; q += OP_THREADS) {   // the moving average of mww_stream_metrics: float32 sum in order, one division
    float s = 0.f;
    for (int k = 0; k < w; ++k) s += s_p[q + k];
    s_avg[q] = s / (float)w;
  }
  __syncthreads();
  if (a.kind[t] != 0) {
    float best = -INFINITY;
    for (int q = j; q < len; q += OP_THREADS) best = s_avg[q] > best ? s_avg[q] : best;
    s_best[j] = best;
    __syncthreads();
    for (int d = OP_THREADS >> 1; d > 0; d >>= 1) {
      if (j < d && s_best[j + d] > s_best[j]) s_best[j] = s_best[j + d];
      __syncthreads();
    }
    if (j == 0) a.seg_best[(int64_t)(a.w0 + wk) * a.n_seg + seg] = s_best[0];
    return;
  }
  if (j >= a.n_cut) return;
  const double c = a.cut[j];
  const int nc = a.n_cut, ne = a.n_entry;
  unsigned* tab = a.tab + ((int64_t)(a.tab_first[t] + (seg - a.seg_first[t])) * a.pw + wk) * ne * nc + j;   // entry e at tab[e * nc]
  unsigned* ring = a.ring_lds ? s_ring + j : tab;                     // slot q at ring[q * nc]
  for (int e = len; e < ne; ++e) ring[(int64_t)e * nc] = 0u;          // a short last segment: entering past its end accepts nothing
  unsigned cur = 0u;                                                  // F(i + 1); F past the end is (0, -)
  int slot = (len - 1) % ne;
  for (int i = len - 1; i >= 0; --i) {
    if ((double)s_avg[i] > c) {
      const unsigned nxt = a.cdp < len - i ? ring[(int64_t)slot * nc] : 0u;   // F(i + cdp), in the slot F(i) takes
      const unsigned cnt = nxt & ((1u << OP_CNT_BITS) - 1);
      cur = cnt ? nxt + 1u : 1u | (unsigned)i << OP_CNT_BITS;                 // the chain's last accept stays
    }
    ring[(int64_t)slot * nc] = cur;
    slot = slot ? slot - 1 : ne - 1;
  }
  if (a.ring_lds)
    for (int e = 0; e < ne; ++e) tab[(int64_t)e * nc] = ring[e * nc];
}

__global__ void __launch_bounds__(256) op_track_kernel(OpArgs a) {
  const int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= (int64_t)a.n_trk * a.pw * a.n_cut) return;
  const int c = (int)(id % a.n_cut), wk = (int)(id / a.n_cut % a.pw), t = (int)(id / a.n_cut / a.pw);
  const int wi = a.w0 + wk;
  int64_t b;
  const int64_t m = op_values(a, t, a.win[wi], &b);
  const int s0 = a.seg_first[t], s1 = s0 + (int)((m + OP_SEG - 1) / OP_SEG);
  const bool positive = a.kind[t] != 0;
  unsigned long long total = 0;
  if (!positive) {
    int64_t state = a.first_ok;
    for (int s = s0; s < s1; ++s) {
      if (state >= OP_SEG) {   // still cooling down beyond this segment
        state -= OP_SEG;
        continue;
      }
      const unsigned v = a.tab[(((int64_t)s * a.pw + wk) * a.n_entry + state) * a.n_cut + c];
      const unsigned cnt = v & ((1u << OP_CNT_BITS) - 1);
      total += cnt;
      const int64_t next = cnt ? (int64_t)(v >> OP_CNT_BITS) + a.cdp : state;
      state = next > OP_SEG ? next - OP_SEG : 0;
    }
  }
  a.trk_cnt[((int64_t)wi * a.n_trk + t) * a.n_cut + c] = total;
  if (c == 0) {
    float best = positive ? -INFINITY : 0.f;
    if (positive)
      for (int s = s0; s < s1; ++s) {
        const float v = a.seg_best[(int64_t)wi * a.n_seg + s];
        best = v > best ? v : best;
      }
    a.ma_len[(int64_t)wi * a.n_trk + t] = m;
    a.score[(int64_t)wi * a.n_trk + t] = best;
  }
}

// per (window, cutoff) sum over the tracks, in track order
__global__ void __launch_bounds__(256) op_sum_kernel(OpArgs a) {
  const int id = blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= a.pw * a.n_cut) return;
  const int c = id % a.n_cut, wi = a.w0 + id / a.n_cut;
  unsigned long long s = 0;
  for (int t = 0; t < a.n_trk; ++t) s += a.trk_cnt[((int64_t)wi * a.n_trk + t) * a.n_cut + c];
  a.total[(int64_t)wi * a.n_cut + c] = s;
}

// ---- mww_stream_operating_summary
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

// op_track_kernel's walk, for the ambient tracks alone
__global__ void __launch_bounds__(256) ops_ambient_kernel(OpArgs a, OpsArgs o) {
  const int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= (int64_t)o.n_amb * a.pw * a.n_cut) return;
  const int c = (int)(id % a.n_cut), wk = (int)(id / a.n_cut % a.pw), j = (int)(id / a.n_cut / a.pw);
  const int wi = a.w0 + wk, t = o.amb[j];
  int64_t b;
  const int64_t m = op_values(a, t, a.win[wi], &b);
  const int s0 = a.tab_first[t], s1 = s0 + (int)((m + OP_SEG - 1) / OP_SEG);   // table rows: a positive track has none
  unsigned long long total = 0;
  int64_t state = a.first_ok;
  for (int s = s0; s < s1; ++s) {
    if (state >= OP_SEG) {   // still cooling down beyond this segment
      state -= OP_SEG;
      continue;
    }
    const unsigned v = a.tab[(((int64_t)s * a.pw + wk) * a.n_entry + state) * a.n_cut + c];
    const unsigned cnt = v & ((1u << OP_CNT_BITS) - 1);
    total += cnt;
    const int64_t next = cnt ? (int64_t)(v >> OP_CNT_BITS) + a.cdp : state;
    state = next > OP_SEG ? next - OP_SEG : 0;
  }
  o.amb_cnt[((int64_t)wi * o.n_amb + j) * a.n_cut + c] = total;
}

__global__ void __launch_bounds__(OPS_POS) ops_positive_kernel(OpArgs a, OpsArgs o) {
  __shared__ float s_score[OPS_POS];
  __shared__ unsigned s_short[OPS_POS];
  const int blk = blockIdx.x, wi = a.w0 + blockIdx.y, i = threadIdx.x;
  const int first = blk * OPS_POS;
  const int n = o.n_pos - first < OPS_POS ? o.n_pos - first : OPS_POS;
  if (i < n) {
    const int t = o.pos[first + i];
    int64_t b;
    const int64_t m = op_values(a, t, a.win[wi], &b);
    const int s0 = a.seg_first[t], s1 = s0 + (int)((m + OP_SEG - 1) / OP_SEG);
    float best = -INFINITY;   // the score of op_track_kernel: the segments in order; no value: -inf
    for (int s = s0; s < s1; ++s) {
      const float v = a.seg_best[(int64_t)wi * a.n_seg + s];
      best = v > best ? v : best;
    }
    s_score[i] = best;
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
  unsigned long long cnt = 0, acc = 0;
  for (int j = 0; j < o.n_amb; ++j) cnt += o.amb_cnt[((int64_t)wi * o.n_amb + j) * a.n_cut + c];
  for (int b = 0; b < o.n_pblk; ++b) acc += o.part_acc[((int64_t)wi * o.n_pblk + b) * a.n_cut + c];
  o.counts[(int64_t)wi * a.n_cut + c] = cnt;
  o.accepts[(int64_t)wi * a.n_cut + c] = acc;
  if (c != 0) return;
  // streaming.track_hours: h += ((n * stride) * step_s) / 3600.0 in track order, three separate float64 operations
  double h = 0.0;
  int64_t short_amb = 0, short_pos = 0;
  for (int j = 0; j < o.n_amb; ++j) {
#pragma clang fp contract(off)
    int64_t b;
    const int64_t m = op_values(a, o.amb[j], a.win[wi], &b);
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

// what both entry points check and derive from their arguments (after the null-pointer check)
struct OpPlan {
  std::vector<int32_t> seg_first;   // [n_tracks + 1]
  std::vector<int32_t> tab_first;   // [n_tracks + 1] with ambient_tables: the first table row of each track, kind-1 tracks taking none
  int64_t n_seg, per_window;        // segments of the smallest window; bytes of one window's transfer tables
  int cdp, n_entry, pw;             // pw: windows per pass
};

int op_plan(const mww_stream* s, const int64_t* offsets, const int32_t* kind, int64_t n_tracks, const int32_t* windows, int n_windows,
            int skip, int cooldown, int n_cutoffs, bool ambient_tables, OpPlan* p) {
  if (n_tracks <= 0 || n_tracks > INT32_MAX || skip < 0 || cooldown < 0 || n_cutoffs <= 0 || n_cutoffs > 128)
    return mww::set_error(MWW_ERR_INVALID, "bad operating-point arguments (1..128 cutoffs)");
  if (n_windows <= 0 || n_windows > MWW_OP_MAX_WINDOWS)
    return mww::set_error(MWW_ERR_INVALID, ("1.." + std::to_string(MWW_OP_MAX_WINDOWS) + " windows per call").c_str());
  int wmin = MWW_OP_MAX_WINDOW;
  for (int k = 0; k < n_windows; ++k) {
    if (windows[k] <= 0 || windows[k] > MWW_OP_MAX_WINDOW)
      return mww::set_error(MWW_ERR_INVALID, ("a window must lie in 1.." + std::to_string(MWW_OP_MAX_WINDOW)).c_str());
    wmin = std::min(wmin, (int)windows[k]);
  }
  if (offsets[0] < 0 || offsets[n_tracks] > s->n_out) return mww::set_error(MWW_ERR_INVALID, "track offsets exceed the probabilities held");
  for (int64_t t = 0; t < n_tracks; ++t)
    if (offsets[t + 1] < offsets[t]) return mww::set_error(MWW_ERR_INVALID, "track offsets must not decrease");
  p->seg_first.resize((size_t)n_tracks + 1);
  if (ambient_tables) p->tab_first.resize((size_t)n_tracks + 1);
  int64_t n_seg = 0, n_rows = 0;
  for (int64_t t = 0; t < n_tracks; ++t) {
    p->seg_first[(size_t)t] = (int32_t)n_seg;
    if (ambient_tables) p->tab_first[(size_t)t] = (int32_t)n_rows;
    const int64_t n = offsets[t + 1] - offsets[t] - (kind[t] ? skip : 0);
    const int64_t m = n >= wmin ? n - wmin + 1 : 0;
    n_seg += (m + OP_SEG - 1) / OP_SEG;
    if (!kind[t]) n_rows += (m + OP_SEG - 1) / OP_SEG;
    if (n_seg > INT32_MAX) return mww::set_error(MWW_ERR_INVALID, "too many probabilities for one call");
  }
  p->seg_first[(size_t)n_tracks] = (int32_t)n_seg;
  if (ambient_tables) p->tab_first[(size_t)n_tracks] = (int32_t)n_rows;
  p->n_seg = n_seg;
  p->cdp = std::max(cooldown, 1);
  p->n_entry = std::min(p->cdp, OP_SEG);
  p->per_window = std::max<int64_t>(ambient_tables ? n_rows : n_seg, 1) * p->n_entry * n_cutoffs * 4;
  p->pw = (int)std::min<int64_t>(n_windows, std::max<int64_t>(OP_SCRATCH / p->per_window, 1));
  return MWW_OK;
}

}  // namespace

extern "C" {

int mww_stream_operating_points(mww_stream* s, const int64_t* offsets, const int32_t* kind, int64_t n_tracks, const int32_t* windows,
                                int n_windows, int skip, int cooldown, const double* cutoffs, int n_cutoffs, uint64_t* counts,
                                int64_t* ma_len, float* score) {
  if (!s || !offsets || !kind || !windows || !cutoffs || !counts || !ma_len || !score) return mww::set_error(MWW_ERR_INVALID, "null argument");
  OpPlan plan;
  if (int rc = op_plan(s, offsets, kind, n_tracks, windows, n_windows, skip, cooldown, n_cutoffs, false, &plan)) return rc;
  const std::vector<int32_t>& seg_first = plan.seg_first;
  const int64_t n_seg = plan.n_seg, per_window = plan.per_window;
  const int cdp = plan.cdp, n_entry = plan.n_entry, pw = plan.pw;
  auto al = [](int64_t b) { return (b + 255) & ~(int64_t)255; };
  const int64_t W = n_windows;
  const int64_t o_off = 0, o_kind = al((n_tracks + 1) * 8), o_sf = al(o_kind + n_tracks * 4), o_win = al(o_sf + (n_tracks + 1) * 4),
                o_cut = al(o_win + W * 4), o_in_end = al(o_cut + n_cutoffs * 8), o_tot = o_in_end, o_len = al(o_tot + W * n_cutoffs * 8),
                o_sc = al(o_len + W * n_tracks * 8), o_cnt = al(o_sc + W * n_tracks * 4), o_best = al(o_cnt + W * n_tracks * n_cutoffs * 8),
                bytes = al(o_best + W * n_seg * 4);
  SCHK(hipSetDevice(s->device));
  int rc = grow(&s->op_tab, &s->cap_op_tab, bytes);
  if (!rc) rc = grow(&s->op_scr, &s->cap_op_scr, per_window * pw);
  if (rc) return rc;
  std::vector<char> h((size_t)o_in_end, 0);
  std::memcpy(&h[o_off], offsets, (size_t)(n_tracks + 1) * 8);
  std::memcpy(&h[o_kind], kind, (size_t)n_tracks * 4);
  std::memcpy(&h[o_sf], seg_first.data(), (size_t)(n_tracks + 1) * 4);
  std::memcpy(&h[o_win], windows, (size_t)W * 4);
  std::memcpy(&h[o_cut], cutoffs, (size_t)n_cutoffs * 8);
  SCHK(hipMemcpyAsync(s->op_tab, h.data(), (size_t)o_in_end, hipMemcpyHostToDevice, s->stream));
  OpArgs a{};
  a.prob = s->prob;
  a.off = reinterpret_cast<const int64_t*>(s->op_tab + o_off);
  a.kind = reinterpret_cast<const int*>(s->op_tab + o_kind);
  a.seg_first = reinterpret_cast<const int*>(s->op_tab + o_sf);
  a.tab_first = a.seg_first;   // a table row per segment
  a.win = reinterpret_cast<const int*>(s->op_tab + o_win);
  a.cut = reinterpret_cast<const double*>(s->op_tab + o_cut);
  a.n_trk = (int)n_tracks;
  a.n_seg = (int)n_seg;
  a.n_cut = n_cutoffs;
  a.skip = skip;
  a.cdp = cdp;
  a.first_ok = std::max(cooldown - 1, 0);
  a.n_entry = n_entry;
  a.ring_lds = (int64_t)n_cutoffs * n_entry * 4 <= OP_RING_LDS;
  a.tab = reinterpret_cast<unsigned*>(s->op_scr);
  a.total = reinterpret_cast<unsigned long long*>(s->op_tab + o_tot);
  a.ma_len = reinterpret_cast<int64_t*>(s->op_tab + o_len);
  a.score = reinterpret_cast<float*>(s->op_tab + o_sc);
  a.trk_cnt = reinterpret_cast<unsigned long long*>(s->op_tab + o_cnt);
  a.seg_best = reinterpret_cast<float*>(s->op_tab + o_best);
  const size_t lds = a.ring_lds ? (size_t)n_cutoffs * n_entry * 4 : 0;
  for (int w0 = 0; w0 < n_windows; w0 += pw) {   // stream order: a pass reuses the tables of the one before
    a.w0 = w0;
    a.pw = std::min(pw, n_windows - w0);
    if (n_seg) {
      hipLaunchKernelGGL(op_segment_kernel, dim3((unsigned)n_seg, (unsigned)a.pw), dim3(OP_THREADS), lds, s->stream, a);
      SCHK(hipGetLastError());
    }
    const int64_t n_thr = n_tracks * a.pw * n_cutoffs;
    hipLaunchKernelGGL(op_track_kernel, dim3((unsigned)((n_thr + 255) / 256)), dim3(256), 0, s->stream, a);
    SCHK(hipGetLastError());
    hipLaunchKernelGGL(op_sum_kernel, dim3((unsigned)((a.pw * n_cutoffs + 255) / 256)), dim3(256), 0, s->stream, a);
    SCHK(hipGetLastError());
  }
  SCHK(hipMemcpyAsync(counts, a.total, (size_t)(W * n_cutoffs) * 8, hipMemcpyDeviceToHost, s->stream));
  SCHK(hipMemcpyAsync(ma_len, a.ma_len, (size_t)(W * n_tracks) * 8, hipMemcpyDeviceToHost, s->stream));
  SCHK(hipMemcpyAsync(score, a.score, (size_t)(W * n_tracks) * 4, hipMemcpyDeviceToHost, s->stream));
  SCHK(hipStreamSynchronize(s->stream));
  return MWW_OK;
}

int mww_stream_operating_summary(mww_stream* s, const int64_t* offsets, const int32_t* kind, int64_t n_tracks, const int32_t* windows,
                                 int n_windows, int skip, int cooldown, const double* cutoffs, int n_cutoffs, int stride, double step_s,
                                 uint64_t* counts, uint64_t* accepts, double* hours, int64_t* short_tracks, int64_t* n_kind) {
  if (!s || !offsets || !kind || !windows || !cutoffs || !counts || !accepts || !hours || !short_tracks || !n_kind)
    return mww::set_error(MWW_ERR_INVALID, "null argument");
  if (stride < 1 || !(step_s > 0)) return mww::set_error(MWW_ERR_INVALID, "bad operating-summary arguments (stride >= 1, step_s > 0)");
  OpPlan plan;
  if (int rc = op_plan(s, offsets, kind, n_tracks, windows, n_windows, skip, cooldown, n_cutoffs, true, &plan)) return rc;
  std::vector<int32_t> amb, pos;
  for (int64_t t = 0; t < n_tracks; ++t) (kind[t] ? pos : amb).push_back((int32_t)t);
  const int64_t n_amb = (int64_t)amb.size(), n_pos = (int64_t)pos.size(), n_pblk = (n_pos + OPS_POS - 1) / OPS_POS;
  const int64_t n_seg = plan.n_seg, W = n_windows, C = n_cutoffs;
  const int pw = plan.pw;
  auto al = [](int64_t b) { return (b + 255) & ~(int64_t)255; };
  // inputs, then the result block (counts, accepts, hours, short_tracks, n_kind: contiguous, read back in one copy), then scratch
  const int64_t o_off = 0, o_kind = al((n_tracks + 1) * 8), o_sf = al(o_kind + n_tracks * 4), o_win = al(o_sf + (n_tracks + 1) * 4),
                o_cut = al(o_win + W * 4), o_amb = al(o_cut + C * 8), o_pos = al(o_amb + n_amb * 4), o_tf = al(o_pos + n_pos * 4), o_in_end = al(o_tf + (n_tracks + 1) * 4);
  const int64_t r_cnt = 0, r_acc = r_cnt + W * C * 8, r_hours = r_acc + W * C * 8, r_short = r_hours + W * 8, r_kind = r_short + W * 16,
                r_bytes = r_kind + 16;
  const int64_t o_res = o_in_end, o_acnt = al(o_res + r_bytes), o_pacc = al(o_acnt + W * n_amb * C * 8), o_pshort = al(o_pacc + W * n_pblk * C * 4),
                o_best = al(o_pshort + W * n_pblk * 4), bytes = al(o_best + W * n_seg * 4);
  SCHK(hipSetDevice(s->device));
  int rc = grow(&s->op_tab, &s->cap_op_tab, bytes);
  if (!rc) rc = grow(&s->op_scr, &s->cap_op_scr, plan.per_window * pw);
  if (rc) return rc;
  std::vector<char> h((size_t)o_in_end, 0);
  std::memcpy(&h[o_off], offsets, (size_t)(n_tracks + 1) * 8);
  std::memcpy(&h[o_kind], kind, (size_t)n_tracks * 4);
  std::memcpy(&h[o_sf], plan.seg_first.data(), (size_t)(n_tracks + 1) * 4);
  std::memcpy(&h[o_win], windows, (size_t)W * 4);
  std::memcpy(&h[o_cut], cutoffs, (size_t)C * 8);
  if (n_amb) std::memcpy(&h[o_amb], amb.data(), (size_t)n_amb * 4);
  if (n_pos) std::memcpy(&h[o_pos], pos.data(), (size_t)n_pos * 4);
  std::memcpy(&h[o_tf], plan.tab_first.data(), (size_t)(n_tracks + 1) * 4);
  SCHK(hipMemcpyAsync(s->op_tab, h.data(), (size_t)o_in_end, hipMemcpyHostToDevice, s->stream));
  OpArgs a{};
  a.prob = s->prob;
  a.off = reinterpret_cast<const int64_t*>(s->op_tab + o_off);
  a.kind = reinterpret_cast<const int*>(s->op_tab + o_kind);
  a.seg_first = reinterpret_cast<const int*>(s->op_tab + o_sf);
  a.tab_first = reinterpret_cast<const int*>(s->op_tab + o_tf);   // table rows for the ambient tracks' segments alone
  a.win = reinterpret_cast<const int*>(s->op_tab + o_win);
  a.cut = reinterpret_cast<const double*>(s->op_tab + o_cut);
  a.n_trk = (int)n_tracks;
  a.n_seg = (int)n_seg;
  a.n_cut = n_cutoffs;
  a.skip = skip;
  a.cdp = plan.cdp;
  a.first_ok = std::max(cooldown - 1, 0);
  a.n_entry = plan.n_entry;
  a.ring_lds = C * plan.n_entry * 4 <= OP_RING_LDS;
  a.tab = reinterpret_cast<unsigned*>(s->op_scr);
  a.seg_best = reinterpret_cast<float*>(s->op_tab + o_best);
  OpsArgs o{};
  o.amb = reinterpret_cast<const int*>(s->op_tab + o_amb);
  o.pos = reinterpret_cast<const int*>(s->op_tab + o_pos);
  o.n_amb = (int)n_amb;
  o.n_pos = (int)n_pos;
  o.n_pblk = (int)n_pblk;
  o.stride = stride;
  o.step_s = step_s;
  o.amb_cnt = reinterpret_cast<unsigned long long*>(s->op_tab + o_acnt);
  o.part_acc = reinterpret_cast<unsigned*>(s->op_tab + o_pacc);
  o.part_short = reinterpret_cast<unsigned*>(s->op_tab + o_pshort);
  char* res = s->op_tab + o_res;
  o.counts = reinterpret_cast<unsigned long long*>(res + r_cnt);
  o.accepts = reinterpret_cast<unsigned long long*>(res + r_acc);
  o.hours = reinterpret_cast<double*>(res + r_hours);
  o.short_tracks = reinterpret_cast<int64_t*>(res + r_short);
  o.n_kind = reinterpret_cast<int64_t*>(res + r_kind);
  const size_t lds = a.ring_lds ? (size_t)C * plan.n_entry * 4 : 0;
  for (int w0 = 0; w0 < n_windows; w0 += pw) {   // stream order: a pass reuses the tables of the one before
    a.w0 = w0;
    a.pw = std::min(pw, n_windows - w0);
    if (n_seg) {
      hipLaunchKernelGGL(op_segment_kernel, dim3((unsigned)n_seg, (unsigned)a.pw), dim3(OP_THREADS), lds, s->stream, a);
      SCHK(hipGetLastError());
    }
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
  }
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
