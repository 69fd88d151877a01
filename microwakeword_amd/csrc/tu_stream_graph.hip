// Streaming / non-streaming inference of a conv -> BN/SSN -> ReLU graph (mww_stream_create_convnet, include/mww.h): the
// Inception model of microwakeword/inception.py:233-338 in Modes.STREAM_INTERNAL_STATE_INFERENCE, one spectrogram frame
// per step, behind the same mww_stream handle, track tables and metrics as the MixedNet stream (tu_stream.hip).
//
// What the reference keeps per layer:
//   stem i        Stream(Conv2D(k_i x 1, valid, no bias), use_one_step=True) -> SubSpectralNormalization -> ReLU
//                 (inception.py:256-274); its ring holds k_i rows of the layer's input INCLUDING the current frame
//                 (layers/stream.py:241-245, :566-575), so k_i - 1 earlier rows can influence an output;
//   b1, b2a, b3a  1x1 convolutions on the current frame, no state;
//   b2b, b3b, b3c Stream(Conv2D(k x 1, dilation d, valid), use_one_step=False, pad_time_dim="None"): a ring of d(k - 1)
//                 rows of the layer's own input (stream.py:246-255).  "None" is neither causal nor same, so nothing is
//                 padded and no Delay is built (inception.py:121-122, stream.py:671-693); StridedDrop is the identity
//                 outside NON_STREAM_INFERENCE (strided_drop.py:40-44): the three branches meet at the current frame;
//   head          Stream(Flatten()) (use_one_step=True: T_f rows including the current one, stream.py:273-283) ->
//                 Dropout (inactive) -> Dense(1, sigmoid).
// SSN / BN use the moving statistics with eps 1e-3, channel c takes slot c mod g (sub_spectral_normalization.py:38-62);
// they are folded into the convolution's weights and a bias once, in set_weights.  Every ring starts as zeros
// (stream.py:580-594).
//
// Whole-sequence form (the one tu_stream.hip uses): positions are frame indices of the segment; every convolution runs
// valid and right-aligned, out[i] = sum_j w[j] . in[i - (k - 1 - j) d], positions before the start of the stream read the
// op's ring (its R = d(k - 1) last input rows, all sources concatenated), the Dense reads the last T_f rows of the final map
// at every position.  Right alignment is what src_drop (StridedDrop of LEADING frames) states for the non-streaming
// model, so the same position arithmetic serves both modes: stream mode pads with the rings, non-stream mode scores the
// windows ending at frames T, T + 1, ... of each track, whose receptive field (T - 1 frames) lies inside the track.
//
// Tiling: a workgroup takes a tile of consecutive outputs and recomputes the halo every tensor needs in front of it (its
// reach: the frames between its rows and the first head input of the tile) in a private global scratch region; tensors
// share that region by liveness (a buffer is reused once its last consumer has run).  An op gets a barrier in front of it
// only when it reads or overwrites something touched since the last one (in Keras order: b1 and b2a share an interval).  The tile that ends a stream-mode call
// writes the final rings into the other half of the double-buffered state.  Every sum runs in a fixed order that does not
// depend on the partition (taps, then sources, then channels): no atomics, runs are bit-identical, and a position computes
// the same bits whether its inputs come from a ring or from the tile.
//
// Here: the float kernel, the planner (float and byte placement) and the float half of the graph model part, and the two
// creators.  The host path of the stream is tu_stream.hip; the head and the calibration folds are in stream_common.hip.h.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "stream_graph.hip.h"

using namespace mww_stream_impl;

namespace {

constexpr double kBnEps = 1e-3;
constexpr int kMaxGraphTensors = MWW_MAX_GRAPH_OPS + 2;

// REC (calibration, mww_stream_calibrate_host on a stream of mww_stream_create_convnet_q8): every thread keeps the min / max
// of the values it computes for the current tensor (1 + o: the output of op o; n_ops + 1: the logit), the block folds them in
// thread order after each op (rec_fold) and writes its [n_tensors] partial row once, at the end.  <false> is the kernel
// as it was before recording existed.
template <bool REC>
__global__ void __launch_bounds__(kStreamThreads) stream_graph_kernel(GNet net, SStores S, SCall a) {
  const int tid = threadIdx.x;
  __shared__ float red[REC ? 2 * kStreamThreads : 1], rmin[REC ? kMaxGraphTensors : 1], rmax[REC ? kMaxGraphTensors : 1];
  float lmin = INFINITY, lmax = -INFINITY;
  if (REC) rec_init(a, rmin, rmax);
  float* B = a.scratch + (int64_t)blockIdx.x * a.scratch_per_wg;
  for (int tile = blockIdx.x; tile < a.n_tiles; tile += gridDim.x) {
    const STile T = tile_of(a, tile);
    const int64_t c0 = T.c0, c1 = T.c1, v_seg = T.v_seg, N = T.c1;   // positions are frames of the segment
    const bool last = T.last;
    // ---- gather the spectrogram rows [lo, c1) the tile reads
    int64_t lo = c0 - net.in_reach;
    if (lo < 0) lo = 0;
    {
      float* G = B + net.in_buf;
      for (int64_t idx = tid; idx < (c1 - lo) * MWW_FEATURE_BINS; idx += kStreamThreads)
        G[idx] = frame_value(S, a, v_seg + lo + idx / MWW_FEATURE_BINS, (int)(idx % MWW_FEATURE_BINS));
    }
    for (int o = 0; o < net.n_ops; ++o) {
      const GOp& L = net.ops[o];
      if (L.sync) __syncthreads();
      const int K = L.k, D = L.d, Ci = L.cin, Co = L.cout, R = L.R, ns = L.n_src;
      int64_t o_lo = c0 - L.reach;
      if (o_lo < 0) o_lo = 0;
      const int64_t no = c1 - o_lo;
      const float* ring = a.st_in + L.ring;
      const float* xs[MWW_MAX_OP_SOURCES];   // row 0 of each source's slice, as if the tensor started at position 0
      for (int s = 0; s < ns; ++s) {
        int64_t s_lo = c0 - L.src_reach[s];
        if (s_lo < 0) s_lo = 0;
        xs[s] = B + L.src_buf[s] - s_lo * L.src_C[s] + L.src_c0[s];
      }
      float* out = B + L.out_buf;
      for (int64_t idx = tid; idx < no * Co; idx += kStreamThreads) {
        const int64_t i = o_lo + idx / Co;
        const int co = (int)(idx % Co);
        float acc = a.w[L.b + co];
        for (int j = 0; j < K; ++j) {
          const int64_t q = i - (int64_t)(K - 1 - j) * D;
          const float* w = a.w + L.w + (int64_t)j * Ci * Co + co;
          if (q >= 0) {
            for (int s = 0; s < ns; ++s) {
              const float* x = xs[s] + q * L.src_C[s];
              const int cn = L.src_cn[s];
              for (int ci = 0; ci < cn; ++ci) acc = fmaf(x[ci], w[(int64_t)ci * Co], acc);
              w += (int64_t)cn * Co;
            }
          } else {
            const float* x = ring + (R + q) * Ci;
            for (int ci = 0; ci < Ci; ++ci) acc = fmaf(x[ci], w[(int64_t)ci * Co], acc);
          }
        }
        out[idx] = acc > 0.f ? acc : 0.f;
        if (REC) {
          lmin = fminf(lmin, out[idx]);
          lmax = fmaxf(lmax, out[idx]);
        }
      }
      if (REC) {
        rec_fold(lmin, lmax, 1 + o, red, rmin, rmax);
        lmin = INFINITY;
        lmax = -INFINITY;
      }
      if (last && R > 0) {   // this op's ring after the call: its input at positions [N - R, N)
        for (int idx = tid; idx < R * Ci; idx += kStreamThreads) {
          const int64_t q = N - R + idx / Ci;
          int c = idx % Ci;
          float v;
          if (q >= 0) {
            int s = 0;
            while (c >= L.src_cn[s]) c -= L.src_cn[s++];
            v = xs[s][q * L.src_C[s] + c];
          } else {
            v = ring[(R + q) * Ci + c];
          }
          a.st_out[L.ring + idx] = v;
        }
      }
    }
    __syncthreads();
    // ---- head: Dense over the last T_f rows of the final map at every output position
    const int C = net.c_last, TF = net.tf;
    int64_t f_lo = c0 - (TF - 1);
    if (f_lo < 0) f_lo = 0;
    const float* fin = B + net.last_buf - f_lo * C;
    const float* hring = a.st_in + net.ring_head;
    dense_head<REC>(a, T, fin, C, hring, net.wd, net.bd, C, TF, lmin, lmax);
    if (REC) {
      rec_fold(lmin, lmax, net.n_ops + 1, red, rmin, rmax);
      lmin = INFINITY;
      lmax = -INFINITY;
    }
    if (last) head_ring_store(a.st_out + net.ring_head, T, fin, C, hring, C, TF);
    __syncthreads();   // the next tile reuses the scratch
  }
  if (REC) rec_flush(a, rmin, rmax);
}

inline int bad(int op, const char* field, const std::string& why) {
  return unsupported((op >= 0 ? "op " + std::to_string(op) + ": " : std::string()) + field + " " + why);
}

// first-fit allocator over float offsets of the workgroup's scratch
struct Arena {
  std::vector<std::pair<int64_t, int64_t>> free_;   // (offset, size), sorted by offset, merged
  int64_t top = 0;
  int64_t take(int64_t n) {
    for (size_t i = 0; i < free_.size(); ++i)
      if (free_[i].second >= n) {
        const int64_t off = free_[i].first;
        free_[i].first += n;
        free_[i].second -= n;
        if (!free_[i].second) free_.erase(free_.begin() + (long)i);
        return off;
      }
    const int64_t off = top;
    top += n;
    return off;
  }
  void give(int64_t off, int64_t n) {
    free_.emplace_back(off, n);
    std::sort(free_.begin(), free_.end());
    for (size_t i = 0; i + 1 < free_.size();)
      if (free_[i].first + free_[i].second == free_[i + 1].first) {
        free_[i].second += free_[i + 1].second;
        free_.erase(free_.begin() + (long)i + 1);
      } else {
        ++i;
      }
  }
};

}  // namespace

namespace mww_stream_impl {

// topology, weight / ring layout, reach of every tensor, scratch plan, barrier flags and call geometry from the description
int Graph::plan(const mww_convnet_desc& d, int mode) {
  if (mode != MWW_STREAM_MODE_STREAM && mode != MWW_STREAM_MODE_NON_STREAM) return bad(-1, "mode", "must be stream or non_stream");
  if (d.n_ops <= 0 || d.n_ops > MWW_MAX_GRAPH_OPS) return bad(-1, "n_ops", "must be 1.." + std::to_string(MWW_MAX_GRAPH_OPS));
  if (d.frames <= 0) return bad(-1, "frames", "must be positive");
  if (d.head_attention) return bad(-1, "head_attention", "is outside the streaming graph vocabulary");
  if (d.head_pool) return bad(-1, "head_pool", "is outside the streaming graph vocabulary");
  const int n = d.n_ops, tile = g.tile_outputs;
  std::vector<int> len((size_t)n), ch((size_t)n), reach((size_t)n, 0), last_use((size_t)n, -1);
  ops.assign((size_t)n, GOp{});
  groups.assign((size_t)n, 1);
  src.assign((size_t)n * MWW_MAX_OP_SOURCES, -1);
  int64_t kw = 0, dw = 0, st = 0;
  for (int i = 0; i < n; ++i) {
    const mww_conv_bn_op& o = d.ops[i];
    if (o.kind != MWW_OP_CONV) return bad(i, "kind", "must be MWW_OP_CONV (depthwise ops are outside the streaming graph vocabulary)");
    if (o.stride != 0 && o.stride != 1) return bad(i, "stride", "must be 0 or 1");
    if (o.norm != MWW_NORM_BN) return bad(i, "norm", "must be MWW_NORM_BN");
    if (o.act != MWW_ACT_RELU) return bad(i, "act", "must be MWW_ACT_RELU");
    if (o.residual) return bad(i, "residual", "is outside the streaming graph vocabulary");
    if (o.kernel <= 0 || o.kernel > 1024) return bad(i, "kernel", "must be 1..1024");
    if (o.dilation <= 0 || o.dilation > 1024) return bad(i, "dilation", "must be 1..1024");
    if (o.filters <= 0 || o.filters > 1024) return bad(i, "filters", "must be 1..1024");
    if (o.bn_groups <= 0 || o.filters % o.bn_groups) return bad(i, "bn_groups", "must divide the filters");
    if (o.n_src <= 0 || o.n_src > MWW_MAX_OP_SOURCES) return bad(i, "n_src", "must be 1..3");
    GOp& L = ops[(size_t)i];
    L.n_src = o.n_src;
    L.k = o.kernel;
    L.d = o.dilation;
    L.cout = o.filters;
    L.R = (o.kernel - 1) * o.dilation;
    int tin = -1, cin = 0;
    for (int j = 0; j < o.n_src; ++j) {
      const int src = o.src[j];
      if (src < -1 || src >= i) return bad(i, "src", "must name an earlier op or -1");
      const int sl = src < 0 ? d.frames : len[(size_t)src], sc = src < 0 ? MWW_FEATURE_BINS : ch[(size_t)src];
      if (o.src_drop[j] < 0 || o.src_drop[j] >= sl) return bad(i, "src_drop", "must leave at least one frame");
      if (j && sl - o.src_drop[j] != tin) return bad(i, "src_drop", "does not align the sources to one length");
      tin = sl - o.src_drop[j];
      const int cn = o.src_cn[j] ? o.src_cn[j] : sc - o.src_c0[j];
      if (o.src_c0[j] < 0 || cn <= 0 || o.src_c0[j] + cn > sc) return bad(i, "src_c0 / src_cn", "is not a slice of the source");
      L.src_C[j] = sc;
      this->src[(size_t)i * MWW_MAX_OP_SOURCES + j] = src;
      L.src_c0[j] = o.src_c0[j];
      L.src_cn[j] = cn;
      cin += cn;
      if (src >= 0) last_use[(size_t)src] = i;
    }
    if (tin - L.R <= 0) return bad(i, "kernel", "does not fit frames = " + std::to_string(d.frames) + " (the window is too short for this graph)");
    len[(size_t)i] = tin - L.R;
    ch[(size_t)i] = o.filters;
    L.cin = cin;
    groups[(size_t)i] = o.bn_groups;
    const int slots = o.bn_groups > 1 ? o.bn_groups : o.filters;
    kw += (int64_t)o.kernel * cin * o.filters + 4 * slots;   // kernel, gamma, beta, moving mean, moving variance
    L.w = dw; dw += (int64_t)o.kernel * cin * o.filters;
    L.b = dw; dw += o.filters;
    L.ring = st; st += (int64_t)L.R * cin;
  }
  net.n_ops = n;
  net.tf = len[(size_t)n - 1];
  net.c_last = ch[(size_t)n - 1];
  if ((int64_t)net.tf * net.c_last > (1 << 24)) return bad(-1, "frames", "leaves a final map too large for the head");
  net.wd = dw; dw += (int64_t)net.tf * net.c_last;
  net.bd = dw; dw += 1;
  kw += (int64_t)net.tf * net.c_last + 1;
  net.ring_head = st; st += (int64_t)(net.tf - 1) * net.c_last;
  // reach: frames between a tensor's rows and the first head input of a tile
  reach[(size_t)n - 1] = net.tf - 1;
  int in_reach = 0;
  for (int i = n - 1; i >= 0; --i) {
    const GOp& L = ops[(size_t)i];
    for (int j = 0; j < L.n_src; ++j) {
      int& r = d.ops[i].src[j] < 0 ? in_reach : reach[(size_t)d.ops[i].src[j]];
      r = std::max(r, reach[(size_t)i] + L.R);
    }
  }
  if (in_reach > d.frames - 1) return bad(-1, "frames", "is shorter than the graph's receptive field");   // cannot happen with aligned sources
  net.in_reach = in_reach;
  // scratch plan by liveness + barrier flags: once in floats (pitch C), once in bytes for the int8 kernel (pitch r4(C), so
  // every offset stays 4-byte aligned); the two differ in which buffers the arena reuses, hence in the barrier flags too
  int in_last = -1;
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < d.ops[i].n_src; ++j)
      if (d.ops[i].src[j] < 0) in_last = i;
  auto place = [&](std::vector<GOp>& ops, GNet& pn, bool bytes) {
    Arena ar;
    std::vector<int64_t> buf((size_t)n), size((size_t)n);
    const int64_t in_size = (int64_t)(tile + in_reach) * MWW_FEATURE_BINS;
    pn.in_buf = ar.take(in_size);
    typedef std::pair<int64_t, int64_t> Iv;
    std::vector<Iv> rd, wr;   // regions read / written since the last barrier
    wr.emplace_back(pn.in_buf, in_size);
    auto hits = [](const std::vector<Iv>& v, int64_t off, int64_t sz) {
      for (const Iv& r : v)
        if (off < r.first + r.second && r.first < off + sz) return true;
      return false;
    };
    for (int i = 0; i < n; ++i) {
      GOp& L = ops[(size_t)i];
      L.reach = reach[(size_t)i];
      size[(size_t)i] = (int64_t)(tile + L.reach) * (bytes ? r4(L.cout) : L.cout);
      buf[(size_t)i] = L.out_buf = ar.take(size[(size_t)i]);
      bool need = hits(rd, L.out_buf, size[(size_t)i]) || hits(wr, L.out_buf, size[(size_t)i]);
      for (int j = 0; j < L.n_src; ++j) {
        const int src = d.ops[i].src[j];
        L.src_buf[j] = src < 0 ? pn.in_buf : buf[(size_t)src];
        L.src_reach[j] = src < 0 ? in_reach : reach[(size_t)src];
        if (bytes) L.src_C[j] = (int)r4(L.src_C[j]);
        need = need || hits(wr, L.src_buf[j], src < 0 ? in_size : size[(size_t)src]);
      }
      L.sync = need ? 1 : 0;
      if (need) {
        rd.clear();
        wr.clear();
      }
      wr.emplace_back(L.out_buf, size[(size_t)i]);
      for (int j = 0; j < L.n_src; ++j) {
        const int src = d.ops[i].src[j];
        rd.emplace_back(L.src_buf[j], src < 0 ? in_size : size[(size_t)src]);
      }
      // buffers whose last consumer this op is go back to the arena (an op nobody reads: at once; the last op: the head reads it)
      if (in_last == i) ar.give(pn.in_buf, in_size);
      for (int t = 0; t < i; ++t)
        if (last_use[(size_t)t] == i) ar.give(buf[(size_t)t], size[(size_t)t]);
      if (last_use[(size_t)i] < 0 && i != n - 1) ar.give(buf[(size_t)i], size[(size_t)i]);
    }
    pn.last_buf = buf[(size_t)n - 1];
    return ar.top;
  };
  qops = ops;   // before the float placement: src_C still counts channels
  scratch_per_wg = (place(ops, net, false) + 255) & ~(int64_t)255;
  // int8 form: weights [Co][k][sources, each r4(cn)], int32 values bias / multiplier / shift [Co] per op, then the Dense
  qnet = net;
  int64_t qw = 0, qi = 0;
  for (int i = 0; i < n; ++i) {
    GOp& L = qops[(size_t)i];
    int64_t kp = 0;
    for (int j = 0; j < L.n_src; ++j) kp += r4(L.src_cn[j]);
    L.w = qw; qw += (int64_t)L.cout * L.k * kp;
    L.b = qi; qi += 3 * (int64_t)L.cout;
    q8_requant.emplace_back(L.b, L.cout);
  }
  qnet.wd = qw; qw += (int64_t)net.tf * r4(net.c_last);
  qnet.bd = qi; qi += 3;
  q8_requant.emplace_back(qnet.bd, 1);
  q8_izp = qi; qi += n + 2;
  q8_nw = qw;
  q8_ni = qi;
  q8_tile_bytes = place(qops, qnet, true);
  g.frames = d.frames;
  g.mode = mode;
  g.reach = in_reach;
  g.j0 = mode == MWW_STREAM_MODE_NON_STREAM ? d.frames - 1 : 0;   // the first window's last frame
  n_weights = kw;
  n_dev_w = dw;
  n_state = st;
  n_tensors = n + 2;
  return MWW_OK;
}

int Graph::upload() {
  int rc = upload_table(&d_ops, ops);
  if (!rc && int8) rc = upload_table(&d_qops, qops);
  net.ops = d_ops;
  qnet.ops = d_qops;
  return rc;
}

int64_t Graph::fold_weights(const float* h, float* w) const {
  // Keras get_weights() order (inception.py:233-338): per convolution kernel [k,1,Cin,F], then gamma, beta, moving_mean,
  // moving_variance [slots] (slots = SSN groups, or F for BatchNormalization); dense [T_f*C,1], bias.  The normalisation
  // (moving statistics, eps 1e-3, channel c -> slot c mod g: sub_spectral_normalization.py:38-62) is folded here, once.
  int64_t p = 0;
  for (size_t i = 0; i < ops.size(); ++i) {
    const GOp& L = ops[i];
    const int grp = groups[i], Co = L.cout, slots = grp > 1 ? grp : Co;
    const int64_t rows = (int64_t)L.k * L.cin;
    const float *kern = h + p, *gamma = kern + rows * Co, *beta = gamma + slots, *mean = beta + slots, *var = mean + slots;
    for (int co = 0; co < Co; ++co) {
      const int sl = grp > 1 ? co % grp : co;
      const double sc = (double)gamma[sl] / std::sqrt((double)var[sl] + kBnEps);
      for (int64_t r = 0; r < rows; ++r) w[L.w + r * Co + co] = (float)((double)kern[r * Co + co] * sc);
      w[L.b + co] = (float)((double)beta[sl] - (double)mean[sl] * sc);
    }
    p += rows * Co + 4 * slots;
  }
  const int64_t nd = (int64_t)net.tf * net.c_last;
  std::memcpy(&w[net.wd], h + p, (size_t)nd * sizeof(float));
  w[net.bd] = h[p + nd];
  return p + nd + 1;
}

void Graph::launch(const SStores& S, const SCall& a, int grid, hipStream_t hs) const {
  if (a.rec)
    hipLaunchKernelGGL(stream_graph_kernel<true>, dim3(grid), dim3(kStreamThreads), 0, hs, net, S, a);
  else
    hipLaunchKernelGGL(stream_graph_kernel<false>, dim3(grid), dim3(kStreamThreads), 0, hs, net, S, a);
}

}  // namespace mww_stream_impl

static int create_graph_stream(mww_ctx* ctx, const mww_convnet_desc* d, int32_t mode, bool int8, mww_stream** out) {
  if (!ctx || !d || !out) return mww::set_error(MWW_ERR_INVALID, "null argument");
  *out = nullptr;
  Graph* m = new Graph();
  m->int8 = int8;
  return stream_create(ctx, m, m->plan(*d, mode), out);
}

extern "C" int mww_stream_create_convnet(mww_ctx* ctx, const mww_convnet_desc* d, int32_t mode, mww_stream** out) {
  return create_graph_stream(ctx, d, mode, false, out);
}

extern "C" int mww_stream_create_convnet_q8(mww_ctx* ctx, const mww_convnet_desc* d, int32_t mode, mww_stream** out) {
  return create_graph_stream(ctx, d, mode, true, out);
}
