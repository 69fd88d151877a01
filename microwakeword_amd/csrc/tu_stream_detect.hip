// mww_stream_detections (include/mww.h): the launches are in stream_detect.hip.h, shared with tu_stream_mine.hip; what
// they share with the metric entry points of tu_stream_oppoints.hip is stream_post.hip.h.
#include "stream_detect.hip.h"

extern "C" {

int64_t mww_stream_detections(mww_stream* s, const int64_t* offsets, const int32_t* kind, int64_t n_tracks, int window, int skip,
                              int cooldown, double cutoff, mww_detection* out, int64_t capacity, int64_t* track_count,
                              int64_t* best_index, float* score) {
  if (!s || !offsets || !kind || !track_count || !best_index || !score || (!out && capacity != 0))
    return mww::set_error(MWW_ERR_INVALID, "null argument");
  if (capacity < 0) return mww::set_error(MWW_ERR_INVALID, "bad detection arguments");
  DetArgs a{};
  int rc = det_locate(s, offsets, kind, n_tracks, window, skip, cooldown, cutoff, &a);
  if (rc) return rc;
  int64_t total = 0;
  SCHK(hipMemcpyAsync(&total, a.trk_base + n_tracks, 8, hipMemcpyDeviceToHost, s->stream));
  SCHK(hipMemcpyAsync(track_count, a.trk_count, (size_t)n_tracks * 8, hipMemcpyDeviceToHost, s->stream));
  SCHK(hipMemcpyAsync(best_index, a.trk_bidx, (size_t)n_tracks * 8, hipMemcpyDeviceToHost, s->stream));
  SCHK(hipMemcpyAsync(score, a.trk_score, (size_t)n_tracks * 4, hipMemcpyDeviceToHost, s->stream));
  SCHK(hipStreamSynchronize(s->stream));
  const int64_t n_write = std::min(total, capacity);
  if (n_write > 0) {
    if ((rc = det_events(s, &a, n_write))) return rc;
    SCHK(hipMemcpyAsync(out, s->det_out, (size_t)n_write * sizeof(mww_detection), hipMemcpyDeviceToHost, s->stream));
    SCHK(hipStreamSynchronize(s->stream));
  }
  return total;
}

}  // extern "C"
