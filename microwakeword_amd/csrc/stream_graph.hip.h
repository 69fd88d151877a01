// Shared by the float (tu_stream_graph.hip) and the int8 (tu_stream_graph_q8.hip) kernels of a conv/BN graph stream: the
// planned ops (sources, reach, placement of every tensor in the workgroup's tile, barrier flags) and the graph part of the
// stream object.  Both kernels walk the same ops, tiles and rings; the float plan counts floats, the int8 plan bytes.
#pragma once
#include "stream_common.hip.h"

namespace mww_stream_impl {

constexpr int kGraphTileOutputs = 256;   // outputs per tile

struct GOp {
  int n_src, k, d, cin, cout, R, reach, sync;
  int src_C[MWW_MAX_OP_SOURCES];       // row pitch of the source tensor
  int src_c0[MWW_MAX_OP_SOURCES];      // first channel of the slice read
  int src_cn[MWW_MAX_OP_SOURCES];      // channels read
  int src_reach[MWW_MAX_OP_SOURCES];   // reach of the source tensor (its first row in a tile: max(0, c0 - reach))
  int64_t src_buf[MWW_MAX_OP_SOURCES]; // offset of the source tensor in the workgroup's scratch
  int64_t out_buf, w, b, ring;         // scratch offset of the output; weight [k][cin][cout] / bias [cout] / ring [R][cin] offsets
};

struct GNet {
  int n_ops, tf, c_last, in_reach;
  int64_t in_buf, last_buf, wd, bd, ring_head;
  const GOp* ops;   // [n_ops], device memory
};

// The int8 plan is the same structure counted in bytes: rows have the pitch r4(C), src_C is that pitch, src_buf / out_buf /
// in_buf / last_buf are 4-byte aligned byte offsets of the tile, w / wd offsets into the int8 weights, b / bd into the int32
// values (bias, multiplier, shift [cout] each); ring offsets are unchanged (one byte per value).
inline int64_t r4(int64_t n) { return (n + 3) & ~(int64_t)3; }

}  // namespace mww_stream_impl

struct mww_stream_graph {
  mww_stream_impl::GNet net{};
  std::vector<mww_stream_impl::GOp> ops;
  std::vector<int> groups;   // bn_groups of each op
  std::vector<int> src;      // [n_ops][MWW_MAX_OP_SOURCES] producing op of each source (-1: the spectrogram)
  mww_stream_impl::GOp* d_ops = nullptr;
  int64_t scratch_per_wg = 0;
  // int8 form (mww_stream_create_convnet_q8)
  bool int8 = false;
  mww_stream_impl::GNet qnet{};
  std::vector<mww_stream_impl::GOp> qops;
  mww_stream_impl::GOp* d_qops = nullptr;
  int64_t q_tile_bytes = 0;      // the byte plan of one tile
  int64_t q_nw = 0, q_ni = 0;    // int8 weights / int32 values mww_stream_set_quantized expects
  int64_t q_izp = 0;             // offset of the n_ops + 2 zero points in the int32 values
};
