// Shared by the float (tu_stream_graph.hip) and the int8 (tu_stream_graph_q8.hip) kernels of a conv/BN graph stream: the
// planned ops (sources, reach, placement of every tensor in the workgroup's tile, barrier flags) and the graph model part
// of a stream (stream_common.hip.h).  Both kernels walk the same ops, tiles and rings; the float plan counts floats, the
// int8 plan bytes.
#pragma once
#include "stream_common.hip.h"

namespace mww_stream_impl {

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

struct Graph : SModel {
  GNet net{};
  std::vector<GOp> ops;
  std::vector<int> groups;   // bn_groups of each op
  std::vector<int> src;      // [n_ops][MWW_MAX_OP_SOURCES] producing op of each source (-1: the spectrogram)
  GOp* d_ops = nullptr;
  // int8 form (mww_stream_create_convnet_q8): the byte plan
  GNet qnet{};
  std::vector<GOp> qops;
  GOp* d_qops = nullptr;
  int plan(const mww_convnet_desc& d, int mode);
  ~Graph() override {
    if (d_ops) (void)hipFree(d_ops);
    if (d_qops) (void)hipFree(d_qops);
  }
  int upload() override;
  int64_t fold_weights(const float* h, float* w) const override;
  void launch(const SStores& S, const SCall& a, int grid, hipStream_t hs) const override;
  void q8_state0(const int32_t* zp, int8_t* st0) const override;
  const void* q8_kernel() const override;
  void launch_q8(const SStores& S, const SCall& a, const SQ8& q, int grid, size_t lds, hipStream_t hs) const override;
};

}  // namespace mww_stream_impl
