// What the entry points on a (window, cutoff) grid share (mww_stream_operating_points, _operating_summary:
// tu_stream_oppoints.hip; mww_stream_operating_bootstrap: tu_stream_bootstrap.hip), each written here and nowhere else: the
// arguments of a call, the transfer tables of the cooldown walk (op_segment_kernel) and their composition (op_walk), a
// positive track's score, and OpCall - the checks, the segment plan, the table packing and the window passes of a call.
#pragma once
#include "stream_post.hip.h"

namespace {

constexpr int OP_THREADS = 128;                     // >= the 128 cutoffs of a call: one thread per cutoff
constexpr int OP_CNT_BITS = 11;                     // a table entry: accepts (<= POST_SEG) | last accepted offset << OP_CNT_BITS
static_assert(OP_THREADS >= POST_MAX_CUTOFFS && POST_SEG < (1 << OP_CNT_BITS), "a thread per cutoff; a count fits its bits");
constexpr int64_t OP_SCRATCH = (int64_t)96 << 20;   // transfer tables resident at a time
constexpr int OP_RING_LDS = 32 * 1024;              // a ring of n_cutoffs * n_entry words up to this size lives in LDS

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
  int n_entry;               // min(cdp, POST_SEG): entry states a segment tabulates = slots of the ring
  int w0, pw;                // this pass: windows w0 .. w0 + pw - 1
  int ring_lds;              // the ring is in LDS (else it is the table itself)
  unsigned* tab;             // [table rows][pw][n_entry][n_cut]
  float* seg_best;           // [n_win][n_seg] positive tracks: the segment's maximum
  unsigned long long* trk_cnt;   // [n_win][n_trk][n_cut]
  int64_t* ma_len;           // [n_win][n_trk]
  float* score;              // [n_win][n_trk]
  unsigned long long* total; // [n_win][n_cut]
};

// moving-average values of track t at window index wi
__device__ __forceinline__ int64_t op_len(const OpArgs& a, int t, int wi) { return post_values(a.off, a.kind, a.skip, t, a.win[wi]).m; }

// The cooldown walk of an ambient track at pass window wk and cutoff c: the transfer tables of its `n_rows` segments from table
// row `row0` composed in order, one dependent load per segment.  each(segment of the track, its accepts) is called for every
// segment the walk enters able to accept; a segment it crosses still cooling down has none.
template <class F>
__device__ __forceinline__ void op_walk(const OpArgs& a, int row0, int n_rows, int wk, int c, F&& each) {
  int64_t state = a.first_ok;
  for (int s = row0; s < row0 + n_rows; ++s) {
    if (state >= POST_SEG) {   // still cooling down beyond this segment
      state -= POST_SEG;
      continue;
    }
    const unsigned v = a.tab[(((int64_t)s * a.pw + wk) * a.n_entry + state) * a.n_cut + c];
    const unsigned cnt = v & ((1u << OP_CNT_BITS) - 1);
    each(s - row0, cnt);
    const int64_t next = cnt ? (int64_t)(v >> OP_CNT_BITS) + a.cdp : state;
    state = next > POST_SEG ? next - POST_SEG : 0;
  }
}

// An ambient track's count: the accepts of its segments summed
__device__ __forceinline__ unsigned long long op_compose(const OpArgs& a, int row0, int n_rows, int wk, int c) {
  unsigned long long total = 0;
  op_walk(a, row0, n_rows, wk, c, [&](int, unsigned cnt) { total += cnt; });
  return total;
}

// A positive track's score at window wi: the maxima of its `n` segments from segment s0, in order; no value: -inf
__device__ __forceinline__ float op_score(const OpArgs& a, int wi, int s0, int n) {
  float best = -INFINITY;
  for (int s = s0; s < s0 + n; ++s) {
    const float v = a.seg_best[(int64_t)wi * a.n_seg + s];
    best = v > best ? v : best;
  }
  return best;
}

__global__ void __launch_bounds__(OP_THREADS) op_segment_kernel(OpArgs a) {
  __shared__ float s_p[POST_SEG + MWW_OP_MAX_WINDOW - 1];
  __shared__ float s_avg[POST_SEG];
  __shared__ float s_best[OP_THREADS];
  HIP_DYNAMIC_SHARED(unsigned, s_ring)
  const int seg = blockIdx.x, wk = blockIdx.y, j = threadIdx.x;
  const int w = a.win[a.w0 + wk];
  const int t = post_track_of(a.seg_first, a.n_trk, seg);
  const PostValues tv = post_values(a.off, a.kind, a.skip, t, w);
  const int64_t b = tv.b, m = tv.m;
  const int64_t i0 = (int64_t)(seg - a.seg_first[t]) * POST_SEG;
  if (m <= i0) return;   // this window has fewer segments than the smallest one (uniform over the workgroup)
  const int len = (int)(m - i0 < POST_SEG ? m - i0 : POST_SEG);
  const float* p = a.prob + b + i0;
  for (int q = j; q < len + w - 1; q += OP_THREADS) s_p[q] = p[q];   // ends at the track's last probability
  __syncthreads();
  for (int q = j; q < len; q += OP_THREADS) s_avg[q] = post_avg(s_p + q, w);
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

// What the two grid entry points share, in the order a call goes through it.
struct OpCall {
  PostPlan plan;
  PostTable tab;
  OpArgs a{};
  int n_windows = 0, pw = 0;   // pw: windows per pass
  int64_t per_window = 0;      // bytes of one window's transfer tables
  size_t lds = 0;              // of op_segment_kernel: the ring, when it fits

  // checks the arguments (after the entry point's null check), plans the segments and the passes, and opens the table with
  // the inputs both entry points have.  The entry point goes on with its own inputs, tab.end_host(), its result sections.
  int begin(const mww_stream* s, const int64_t* offsets, const int32_t* knd, int64_t n_tracks, const int32_t* windows, int n_win,
            int skip, int cooldown, const double* cutoffs, int n_cutoffs, bool ambient_tables) {
    const std::string bad = "bad operating-point arguments (1.." + std::to_string(POST_MAX_CUTOFFS) + " cutoffs)";
    if (n_tracks <= 0 || n_tracks > INT32_MAX || skip < 0 || cooldown < 0 || n_cutoffs <= 0 || n_cutoffs > POST_MAX_CUTOFFS)
      return mww::set_error(MWW_ERR_INVALID, bad.c_str());
    if (n_win <= 0 || n_win > MWW_OP_MAX_WINDOWS)
      return mww::set_error(MWW_ERR_INVALID, ("1.." + std::to_string(MWW_OP_MAX_WINDOWS) + " windows per call").c_str());
    int wmin = MWW_OP_MAX_WINDOW;
    for (int k = 0; k < n_win; ++k) {
      if (windows[k] <= 0 || windows[k] > MWW_OP_MAX_WINDOW)
        return mww::set_error(MWW_ERR_INVALID, ("a window must lie in 1.." + std::to_string(MWW_OP_MAX_WINDOW)).c_str());
      wmin = std::min(wmin, (int)windows[k]);
    }
    if (int rc = post_check_tracks(s, offsets, knd, n_tracks, true, bad, false)) return rc;
    if (int rc = post_plan(offsets, knd, n_tracks, skip, wmin, ambient_tables, &plan)) return rc;   // the smallest window has the most segments
    n_windows = n_win;
    a.prob = s->prob;
    a.n_trk = (int)n_tracks;
    a.n_seg = (int)plan.n_seg;
    a.n_cut = n_cutoffs;
    a.skip = skip;
    a.cdp = std::max(cooldown, 1);
    a.first_ok = std::max(cooldown - 1, 0);
    a.n_entry = std::min(a.cdp, POST_SEG);
    a.ring_lds = (int64_t)n_cutoffs * a.n_entry * 4 <= OP_RING_LDS;
    lds = a.ring_lds ? (size_t)n_cutoffs * a.n_entry * 4 : 0;
    per_window = std::max<int64_t>(ambient_tables ? plan.n_rows : plan.n_seg, 1) * a.n_entry * n_cutoffs * 4;
    pw = (int)std::min<int64_t>(n_win, std::max<int64_t>(OP_SCRATCH / per_window, 1));
    tab.add(&a.off, n_tracks + 1, offsets);
    tab.add(&a.kind, n_tracks, knd);
    tab.add(&a.seg_first, n_tracks + 1, plan.seg_first.data());
    tab.add(&a.win, n_win, windows);
    tab.add(&a.cut, n_cutoffs, cutoffs);
    return MWW_OK;
  }

  // closes the table with the segments' maxima, uploads it and so points OpArgs at it (a table row per segment, unless the
  // entry point added a tab_first of its own)
  int commit(mww_stream* s) {
    tab.add(&a.seg_best, (int64_t)n_windows * plan.n_seg);
    SCHK(hipSetDevice(s->device));
    int rc = tab.commit(&s->post_tab, &s->cap_post_tab, s->stream);
    if (!rc) rc = grow(&s->post_scr, &s->cap_post_scr, per_window * pw);
    if (rc) return rc;
    if (!a.tab_first) a.tab_first = a.seg_first;
    a.tab = reinterpret_cast<unsigned*>(s->post_scr);
    return MWW_OK;
  }

  // the windows in passes of pw, in stream order (a pass reuses the tables of the one before): op_segment_kernel, then the
  // entry point's launches `follow(a)`
  template <class F>
  int passes(mww_stream* s, F&& follow) {
    for (int w0 = 0; w0 < n_windows; w0 += pw) {
      a.w0 = w0;
      a.pw = std::min(pw, n_windows - w0);
      if (a.n_seg) {
        hipLaunchKernelGGL(op_segment_kernel, dim3((unsigned)a.n_seg, (unsigned)a.pw), dim3(OP_THREADS), lds, s->stream, a);
        SCHK(hipGetLastError());
      }
      if (int rc = follow(a)) return rc;
    }
    return MWW_OK;
  }
};

}  // namespace
