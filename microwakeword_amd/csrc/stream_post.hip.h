// What the entry points on the probabilities a stream holds have in common (mww_stream_metrics, _operating_points,
// _operating_summary: tu_stream_oppoints.hip; _operating_bootstrap: tu_stream_bootstrap.hip; mww_stream_detections, mww_stream_mine:
// stream_detect.hip.h), each written here and
// nowhere else: the moving average (every test of the family rests on all its users forming the same bits), the values of a
// track, the segment search, the shared sizes, the track-table check, the segment plan and the packing of a call's tables.
// No two entry points run at once and each synchronises before it returns, so they share two scratch buffers of the stream:
// post_tab (a call's tables) and post_scr (transfer tables and candidates).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "stream_common.hip.h"

using namespace mww_stream_impl;

namespace {

constexpr int POST_SEG = 1024;          // moving-average values per segment of a cooldown walk
constexpr int POST_MAX_CUTOFFS = 128;   // cutoffs of one call: one thread each

// the moving average at p (global memory or LDS): float32 sum in order, then one division (numpy .mean of the float32 window)
__device__ __forceinline__ float post_avg(const float* p, int win) {
  float s = 0.f;
  for (int k = 0; k < win; ++k) s += p[k];
  return s / (float)win;
}

struct PostValues {
  int64_t b;   // first probability of the track's moving-average sequence (after the skip of a positive track)
  int64_t m;   // moving-average values (0: the track is shorter than skip + window)
};

__device__ __forceinline__ PostValues post_values(const int64_t* off, const int* kind, int skip, int t, int win) {
  const int64_t sk = kind[t] ? skip : 0;
  const int64_t n = off[t + 1] - off[t] - sk;
  return {off[t] + sk, n >= win ? n - win + 1 : 0};
}

// track of segment `seg`: the last t with seg_first[t] <= seg (tracks without a segment share their successor's entry)
__device__ __forceinline__ int post_track_of(const int* seg_first, int n_trk, int seg) {
  int lo = 0, hi = n_trk;   // seg_first[lo] <= seg < seg_first[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (seg_first[mid] <= seg) lo = mid; else hi = mid;
  }
  return lo;
}

// sum of n rows of one column, in row order: col[0], col[stride], ...
__device__ __forceinline__ unsigned long long post_sum_rows(const unsigned long long* col, int n, int stride) {
  unsigned long long s = 0;
  for (int t = 0; t < n; ++t) s += col[(int64_t)t * stride];
  return s;
}

// The track table of a call.  `args_ok`: the entry point's own scalar arguments are in range; `bad_args`: its text for when
// they (or n_tracks) are not.  `check_kind`: a kind outside {0, 1} is refused (else non-zero is positive).
inline int post_check_tracks(const mww_stream* s, const int64_t* offsets, const int32_t* kind, int64_t n_tracks, bool args_ok,
                             const std::string& bad_args, bool check_kind) {
  if (!args_ok || n_tracks <= 0 || n_tracks > INT32_MAX) return mww::set_error(MWW_ERR_INVALID, bad_args.c_str());
  if (offsets[0] < 0 || offsets[n_tracks] > s->n_out) return mww::set_error(MWW_ERR_INVALID, "track offsets exceed the probabilities held");
  for (int64_t t = 0; t < n_tracks; ++t)
    if (offsets[t + 1] < offsets[t]) return mww::set_error(MWW_ERR_INVALID, "track offsets must not decrease");
  for (int64_t t = 0; check_kind && kind && t < n_tracks; ++t)
    if (kind[t] != 0 && kind[t] != 1) return mww::set_error(MWW_ERR_INVALID, "track kind must be 0 (ambient) or 1 (positive)");
  return MWW_OK;
}

// The tracks cut into segments of POST_SEG values of the moving average over `window` (of several windows the smallest: it
// has the most).  `kind` null: every track is ambient.
struct PostPlan {
  std::vector<int32_t> seg_first;   // [n_tracks + 1] first segment of each track
  std::vector<int32_t> tab_first;   // [n_tracks + 1] with ambient_rows: the same prefix over the kind-0 tracks' segments alone
  int64_t n_seg = 0, n_rows = 0;    // segments; segments of the kind-0 tracks
};

inline int post_plan(const int64_t* offsets, const int32_t* kind, int64_t n_tracks, int skip, int window, bool ambient_rows, PostPlan* p) {
  p->seg_first.resize((size_t)n_tracks + 1);
  if (ambient_rows) p->tab_first.resize((size_t)n_tracks + 1);
  int64_t n_seg = 0, n_rows = 0;
  for (int64_t t = 0; t < n_tracks; ++t) {
    p->seg_first[(size_t)t] = (int32_t)n_seg;
    if (ambient_rows) p->tab_first[(size_t)t] = (int32_t)n_rows;
    const bool positive = kind && kind[t];
    const int64_t n = offsets[t + 1] - offsets[t] - (positive ? skip : 0);
    const int64_t segs = ((n >= window ? n - window + 1 : 0) + POST_SEG - 1) / POST_SEG;
    n_seg += segs;
    if (!positive) n_rows += segs;
    if (n_seg > INT32_MAX) return mww::set_error(MWW_ERR_INVALID, "too many probabilities for one call");
  }
  p->seg_first[(size_t)n_tracks] = (int32_t)n_seg;
  if (ambient_rows) p->tab_first[(size_t)n_tracks] = (int32_t)n_rows;
  p->n_seg = n_seg;
  p->n_rows = n_rows;
  return MWW_OK;
}

// One device buffer cut into sections that start at multiples of 256 bytes, in the order they are added.  add() reserves
// `count` elements for the pointer `*to`, which commit() sets, and returns the section's offset.  The sections added before
// end_host() are filled by the host (from `src`; zeros without one) and go up in one copy; the rest is the kernels'.
// The table keeps the ADDRESS of every pointer it is to set: the struct that holds them must stay where it is (not copied or
// moved) from its first add() to commit(); after commit() it is an ordinary value.  The staging copy `host` may go once
// commit() has returned: it is pageable memory, which hipMemcpyAsync has read by the time it returns.
struct PostTable {
  int64_t size = 0, host_end = 0;
  std::vector<char> host;
  std::vector<std::pair<void*, int64_t>> ptrs;   // (where a section's pointer goes, its offset)

  template <class P>
  int64_t add(P** to, int64_t count, const typename std::remove_const<P>::type* src = nullptr) {
    const int64_t at = size;
    size = (at + count * (int64_t)sizeof(P) + 255) & ~(int64_t)255;
    ptrs.emplace_back((void*)to, at);
    if (src && count > 0) {
      host.resize((size_t)size, 0);
      std::memcpy(&host[(size_t)at], src, (size_t)count * sizeof(P));
    }
    return at;
  }
  void end_host() {
    host_end = size;
    host.resize((size_t)size, 0);
  }
  // grows *buf to hold every section, uploads the host-filled ones and sets the sections' pointers
  int commit(char** buf, int64_t* cap, hipStream_t stream) {
    if (int rc = grow(buf, cap, size)) return rc;
    if (host_end) SCHK(hipMemcpyAsync(*buf, host.data(), (size_t)host_end, hipMemcpyHostToDevice, stream));
    for (const auto& p : ptrs) {
      char* at = *buf + p.second;
      std::memcpy(p.first, &at, sizeof at);
    }
    return MWW_OK;
  }
};

}  // namespace
