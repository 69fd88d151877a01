// mww_stream_mine (include/mww.h): the hard negatives of one mining round, selected and cut into clips on the device.
//
// The events come from the launches of stream_detect.hip.h (every track ambient) and stay in s->det_out; the tables of this
// unit are packed by stream_post.hip.h's PostTable into s->mine_buf.  What follows keeps
// the `max_new` highest moving averages (ties to the earlier event), drops the clips without a row and writes the rest in event
// order - the chain mww_stream_detections -> stable argsort -> streaming.detection_clips, byte for byte:
//   mine_hist_kernel   x 4  radix select of the max_new-th largest key, 8 bits per launch, most significant first.  The key is
//                           a monotone 32-bit image of the average (-0 folded onto +0: they compare equal).  A workgroup counts
//                           its events' digits in LDS (integer atomics: a count does not depend on arrival order) and adds the
//                           256 counts to the launch's global histogram; the digit the previous launches fixed is resolved again
//                           by every workgroup from their histograms (a suffix scan of 256 counts), so no launch sits between.
//   mine_ties_kernel        the events whose key EQUALS the threshold, counted per workgroup.
//   mine_count_kernel       an event is kept when its key is above the threshold, or equal and fewer than `k_ties` equal keys
//                           come before it IN EVENT ORDER (the workgroups' tie counts before it + an LDS prefix scan over the
//                           threads, each owning consecutive events); the kept events with a non-empty clip, per workgroup.
//   mine_write_kernel       the same flags again, the position = kept non-empty clips before the event -> clip and event.
// max_new < 0 or >= the detections keeps every event: the select and the tie count are skipped.
// No floating-point atomic and no arrival order decides a position or a value: two calls write the same bytes.
#include "stream_detect.hip.h"

namespace {

constexpr int MINE_THREADS = 256;
constexpr int MINE_ITEMS = 4;
constexpr int MINE_CHUNK = MINE_THREADS * MINE_ITEMS;   // events per workgroup; thread j owns events j * MINE_ITEMS ... of the chunk
constexpr int MINE_PASSES = 4;

struct MineArgs {
  const mww_detection* ev;   // [n_ev] in (track, index) order
  const mww_window* trk;     // [n_trk] the tracks that were run
  int n_ev, n_blk;
  int select;                // 0: every event is kept
  unsigned k;                // events to keep (select)
  int win, frames, stride, stream_mode, before, after;
  unsigned* hist;            // [MINE_PASSES][256]
  int* blk_ties;             // [n_blk]
  int* blk_keep;             // [n_blk]
  long long* n_kept;         // clips kept in the whole call
  mww_window* out_clip;      // [capacity]
  mww_detection* out_ev;     // [capacity]
  long long capacity;
};

// larger average <=> larger key; -0 and +0 share a key (NaN is never an event: it is not above any cutoff)
__device__ __forceinline__ unsigned mine_key(float avg) {
  unsigned u = __float_as_uint(avg);
  if (avg == 0.f) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// The digits the first `n_pass` launches fixed: *prefix = the top 8 * n_pass bits of the k-th largest key, *k = its rank among
// the keys that share them.  Whole workgroup; s_suf [256], s_res [2].
__device__ __forceinline__ void mine_resolve(const unsigned* hist, int n_pass, unsigned* prefix, unsigned* k, unsigned* s_suf, unsigned* s_res) {
  const int j = threadIdx.x;
  for (int p = 0; p < n_pass; ++p) {
    s_suf[j] = hist[p * 256 + j];
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {   // s_suf[j] = keys whose digit is >= j
      const unsigned add = j + d < 256 ? s_suf[j + d] : 0u;
      __syncthreads();
      s_suf[j] += add;
      __syncthreads();
    }
    const unsigned above = j < 255 ? s_suf[j + 1] : 0u;
    if (s_suf[j] >= *k && above < *k) {   // exactly one j: the counts do not increase with j and s_suf[0] >= k
      s_res[0] = (unsigned)j;
      s_res[1] = above;
    }
    __syncthreads();
    *prefix = (*prefix << 8) | s_res[0];
    *k -= s_res[1];
    __syncthreads();
  }
}

__global__ void __launch_bounds__(MINE_THREADS) mine_hist_kernel(MineArgs a, int pass) {
  __shared__ unsigned s_suf[256];
  __shared__ unsigned s_res[2];
  __shared__ unsigned s_hist[256];
  const int j = threadIdx.x;
  unsigned prefix = 0u, k = a.k;
  mine_resolve(a.hist, pass, &prefix, &k, s_suf, s_res);
  s_hist[j] = 0u;
  __syncthreads();
  const int shift = 24 - 8 * pass;
  const long long e0 = (long long)blockIdx.x * MINE_CHUNK + j * MINE_ITEMS;
  for (int i = 0; i < MINE_ITEMS; ++i) {
    if (e0 + i >= a.n_ev) break;
    const unsigned key = mine_key(a.ev[e0 + i].average);
    if (pass == 0 || (key >> (shift + 8)) == prefix) atomicAdd(&s_hist[(key >> shift) & 255u], 1u);
  }
  __syncthreads();
  if (s_hist[j]) atomicAdd(&a.hist[pass * 256 + j], s_hist[j]);
}

// sum of v[0 .. n) over the workgroup (integer: the order of the additions does not matter); s_sum is one LDS word
__device__ __forceinline__ int mine_sum_before(const int* v, int n, int* s_sum) {
  const int j = threadIdx.x;
  if (j == 0) *s_sum = 0;
  __syncthreads();
  int mine = 0;
  for (int q = j; q < n; q += MINE_THREADS) mine += v[q];
  if (mine) atomicAdd(s_sum, mine);
  __syncthreads();
  const int r = *s_sum;
  __syncthreads();
  return r;
}

// exclusive prefix of the threads' counts in thread order; *total = the workgroup's sum.  s_scan [MINE_THREADS]
__device__ __forceinline__ int mine_scan(int mine, int* s_scan, int* total) {
  const int j = threadIdx.x;
  s_scan[j] = mine;
  __syncthreads();
  for (int d = 1; d < MINE_THREADS; d <<= 1) {
    const int add = j >= d ? s_scan[j - d] : 0;
    __syncthreads();
    s_scan[j] += add;
    __syncthreads();
  }
  const int at = s_scan[j] - mine;
  *total = s_scan[MINE_THREADS - 1];
  __syncthreads();
  return at;
}

__global__ void __launch_bounds__(MINE_THREADS) mine_ties_kernel(MineArgs a) {
  __shared__ unsigned s_suf[256];
  __shared__ unsigned s_res[2];
  __shared__ int s_sum;
  const int j = threadIdx.x;
  unsigned thr = 0u, k = a.k;
  mine_resolve(a.hist, MINE_PASSES, &thr, &k, s_suf, s_res);
  if (j == 0) s_sum = 0;
  __syncthreads();
  const long long e0 = (long long)blockIdx.x * MINE_CHUNK + j * MINE_ITEMS;
  int mine = 0;
  for (int i = 0; i < MINE_ITEMS; ++i)
    if (e0 + i < a.n_ev && mine_key(a.ev[e0 + i].average) == thr) ++mine;
  if (mine) atomicAdd(&s_sum, mine);
  __syncthreads();
  if (j == 0) a.blk_ties[blockIdx.x] = s_sum;
}

// streaming.detection_clips for one event: the store rows behind it, false when there is none
__device__ __forceinline__ bool mine_clip(const MineArgs& a, const mww_detection& d, mww_window* c) {
  const mww_window w = a.trk[d.track];
  const long long n = d.index + a.win - 1;
  const long long e = a.stream_mode ? (n + 1) * a.stride : (long long)a.frames + n * a.stride;
  long long lo = e - a.frames - a.before - w.pad_rows, hi = e + a.after - w.pad_rows;
  if (lo < 0) lo = 0;
  if (hi > w.copy_rows) hi = w.copy_rows;
  if (hi <= lo) return false;
  c->store = w.store;
  c->pad_rows = 0;
  c->copy_rows = (int32_t)(hi - lo);
  c->reserved = 0;
  c->src_elem = w.src_elem + lo * MWW_FEATURE_BINS;
  return true;
}

// The workgroup's events that are kept AND have a clip: bit i of the result for event e0 + i of this thread (clip[i] filled).
// Whole workgroup.
__device__ __forceinline__ unsigned mine_flags(const MineArgs& a, mww_window* clip, unsigned* s_suf, unsigned* s_res, int* s_scan, int* s_sum) {
  const int j = threadIdx.x;
  const long long e0 = (long long)blockIdx.x * MINE_CHUNK + j * MINE_ITEMS;
  unsigned keep = 0u;
  if (a.select) {
    unsigned thr = 0u, k = a.k;
    mine_resolve(a.hist, MINE_PASSES, &thr, &k, s_suf, s_res);   // k: the ties to keep, the first in event order
    const int tie_base = mine_sum_before(a.blk_ties, blockIdx.x, s_sum);
    unsigned tie = 0u;
    int mine = 0;
    for (int i = 0; i < MINE_ITEMS; ++i) {
      if (e0 + i >= a.n_ev) break;
      const unsigned key = mine_key(a.ev[e0 + i].average);
      if (key > thr) keep |= 1u << i;
      if (key == thr) { tie |= 1u << i; ++mine; }
    }
    int total;
    long long rank = (long long)tie_base + mine_scan(mine, s_scan, &total);
    for (int i = 0; i < MINE_ITEMS; ++i)
      if (tie >> i & 1u) {
        if (rank < (long long)k) keep |= 1u << i;
        ++rank;
      }
  } else {
    for (int i = 0; i < MINE_ITEMS; ++i)
      if (e0 + i < a.n_ev) keep |= 1u << i;
  }
  unsigned full = 0u;
  for (int i = 0; i < MINE_ITEMS; ++i)
    if ((keep >> i & 1u) && mine_clip(a, a.ev[e0 + i], &clip[i])) full |= 1u << i;
  return full;
}

template <bool WRITE>
__global__ void __launch_bounds__(MINE_THREADS) mine_compact_kernel(MineArgs a) {
  __shared__ unsigned s_suf[256];
  __shared__ unsigned s_res[2];
  __shared__ int s_scan[MINE_THREADS];
  __shared__ int s_sum;
  const int j = threadIdx.x;
  mww_window clip[MINE_ITEMS];
  const unsigned full = mine_flags(a, clip, s_suf, s_res, s_scan, &s_sum);
  int mine = 0;
  for (int i = 0; i < MINE_ITEMS; ++i) mine += (int)(full >> i & 1u);
  int total;
  const int at = mine_scan(mine, s_scan, &total);
  if (!WRITE) {
    if (j == 0) a.blk_keep[blockIdx.x] = total;
    return;
  }
  const long long base = mine_sum_before(a.blk_keep, blockIdx.x, &s_sum);
  if (blockIdx.x == (unsigned)(a.n_blk - 1) && j == 0) *a.n_kept = base + total;
  const long long e0 = (long long)blockIdx.x * MINE_CHUNK + j * MINE_ITEMS;
  long long pos = base + at;
  for (int i = 0; i < MINE_ITEMS; ++i)
    if (full >> i & 1u) {
      if (pos < a.capacity) {
        a.out_clip[pos] = clip[i];
        a.out_ev[pos] = a.ev[e0 + i];
      }
      ++pos;
    }
}

}  // namespace

extern "C" {

int64_t mww_stream_mine(mww_stream* s, const mww_window* tracks, const int64_t* offsets, int64_t n_tracks, int window, int cooldown,
                        double cutoff, int before, int after, int64_t max_new, mww_window* clips, mww_detection* events,
                        int64_t capacity, int64_t* n_detections, int64_t* track_count) {
  if (!s || !tracks || !offsets || !n_detections || !track_count || ((!clips || !events) && capacity != 0))
    return mww::set_error(MWW_ERR_INVALID, "null argument");
  if (capacity < 0) return mww::set_error(MWW_ERR_INVALID, "bad detection arguments");
  const SGeom& g = s->model->g;
  DetArgs d{};
  int rc = det_locate(s, offsets, nullptr, n_tracks, window, 0, cooldown, cutoff, &d);
  if (rc) return rc;
  int64_t total = 0;
  SCHK(hipMemcpyAsync(&total, d.trk_base + n_tracks, 8, hipMemcpyDeviceToHost, s->stream));
  SCHK(hipStreamSynchronize(s->stream));
  if (total > INT32_MAX) return mww::set_error(MWW_ERR_INVALID, "too many detections for one call");
  *n_detections = total;
  const int64_t k = max_new < 0 || max_new > total ? total : max_new;
  if (k == 0) {   // nothing fired, or nothing is wanted: the counts alone
    SCHK(hipMemcpyAsync(track_count, d.trk_count, (size_t)n_tracks * 8, hipMemcpyDeviceToHost, s->stream));
    SCHK(hipStreamSynchronize(s->stream));
    return 0;
  }
  if ((rc = det_events(s, &d, total))) return rc;
  const int64_t n_blk = (total + MINE_CHUNK - 1) / MINE_CHUNK, n_read = std::min(k, capacity);
  // what the host reads back comes first: the count, the clips, the events
  MineArgs a{};
  PostTable tab;
  const int64_t kept_at = tab.add(&a.n_kept, 1), clip_at = tab.add(&a.out_clip, n_read), ev_at = tab.add(&a.out_ev, n_read);
  const int64_t read_end = tab.size;
  tab.add(&a.hist, MINE_PASSES * 256);
  tab.add(&a.blk_ties, n_blk);
  tab.add(&a.blk_keep, n_blk);
  tab.add(&a.trk, n_tracks);
  if ((rc = tab.commit(&s->mine_buf, &s->cap_mine_buf, s->stream))) return rc;
  a.ev = s->det_out;
  a.n_ev = (int)total;
  a.n_blk = (int)n_blk;
  a.select = k < total ? 1 : 0;
  a.k = (unsigned)k;
  a.win = window;
  a.frames = g.frames;
  a.stride = g.stride;
  a.stream_mode = g.mode == MWW_STREAM_MODE_STREAM ? 1 : 0;
  a.before = before;
  a.after = after;
  a.capacity = n_read;
  SCHK(hipMemcpyAsync(const_cast<mww_window*>(a.trk), tracks, (size_t)n_tracks * sizeof(mww_window), hipMemcpyHostToDevice, s->stream));
  const dim3 grid((unsigned)n_blk), block(MINE_THREADS);
  if (a.select) {
    SCHK(hipMemsetAsync(a.hist, 0, MINE_PASSES * 256 * 4, s->stream));
    for (int pass = 0; pass < MINE_PASSES; ++pass) {
      hipLaunchKernelGGL(mine_hist_kernel, grid, block, 0, s->stream, a, pass);
      SCHK(hipGetLastError());
    }
    hipLaunchKernelGGL(mine_ties_kernel, grid, block, 0, s->stream, a);
    SCHK(hipGetLastError());
  }
  hipLaunchKernelGGL(mine_compact_kernel<false>, grid, block, 0, s->stream, a);
  SCHK(hipGetLastError());
  hipLaunchKernelGGL(mine_compact_kernel<true>, grid, block, 0, s->stream, a);
  SCHK(hipGetLastError());
  // the kept clips and events (at most min(max_new, capacity) of each) and the per-track counts: never the event list
  std::vector<char> h((size_t)read_end);
  SCHK(hipMemcpyAsync(h.data(), s->mine_buf, (size_t)read_end, hipMemcpyDeviceToHost, s->stream));
  SCHK(hipMemcpyAsync(track_count, d.trk_count, (size_t)n_tracks * 8, hipMemcpyDeviceToHost, s->stream));
  SCHK(hipStreamSynchronize(s->stream));
  long long kept = 0;
  std::memcpy(&kept, &h[(size_t)kept_at], 8);
  const int64_t n_copy = std::min<int64_t>(kept, n_read);
  if (n_copy > 0) {
    std::memcpy(clips, &h[(size_t)clip_at], (size_t)n_copy * sizeof(mww_window));
    std::memcpy(events, &h[(size_t)ev_at], (size_t)n_copy * sizeof(mww_detection));
  }
  return kept;
}

}  // extern "C"
