// Streaming inference (mww_stream_*, include/mww.h): the evaluation that follows training in the
// reference (model_train_eval.py:131-272 evaluate_model -> test.py:293-403 tflite_streaming_model_roc, inference.py:82-125
// Model.predict_spectrogram), computed from the HBM-resident feature stores of a context.
//
// The streaming model (Modes.STREAM_INTERNAL_STATE_INFERENCE) keeps, per Stream layer, the last R frames of that layer's
// input in a ring that starts as zeros (layers/stream.py:580-594); one call consumes `stride` spectrogram frames and yields
// one probability.  Ring sizes: conv1 max(0, k1 - s) (stream.py:247-255, use_one_step=False), MixConv max(ks) - 1
// (mixednet.py:193,202-206; no ring when max(ks) == 1, :347), the head's Stream(Identity) T_f - 1 (mixednet.py:365-373);
// StridedKeep(ks) keeps the last ks frames of the shared MixConv ring (strided_drop.py), i.e. right alignment.
//
// Whole-sequence form computed here: every layer's input is left-padded with its R ring frames, every layer then runs
// valid and right-aligned, and the head's Dense reads the last T_f frames of the final map at every position.  Positions
// are counted in conv1 outputs: output n of a call is the head at conv1 index n, conv1 output n reads padded input rows
// [n*s, n*s + k1).  Tracks, concatenated in order, form one virtual stream (stream mode) or one segment each with no
// state (non-stream mode: the non-streaming model on the windows ending at frames T, T+s, ... of the track).
//
// Tiling: a workgroup takes a tile of consecutive outputs of one segment and recomputes its halo (the receptive field of
// each layer: T_f - 1 + sum(K - 1) conv1 frames) in a private global scratch region; positions before the start of the
// stream read the layers' rings instead.  The tile that ends the call also writes the final rings (double-buffered
// state, so no tile reads a ring another tile writes).  Every sum runs in a fixed order: no atomics, runs are bit-identical.
//
// Here: the float MixedNet kernel and the float half of the MixedNet model part (Keras-order weight folding, launch), and
// the host path of EVERY stream - creation, reset, the float and the int8 launch epilogue, calibration (over host frames, and
// over resident windows with the reductions of tu_stream_calibrate.hip), mww_stream_set_quantized - written once against SModel
// (stream_common.hip.h); the conv/BN graph model part and its two
// creators are tu_stream_graph.hip / tu_stream_graph_q8.hip.  What is computed FROM the probabilities a stream holds - the
// detection metrics (mww_stream_metrics), the operating-point grid, detections, mining - is tu_stream_oppoints.hip,
// tu_stream_detect.hip and tu_stream_mine.hip over stream_post.hip.h.  A MixedNet with residual connections, a pooled head or
// spatial attention (mww_stream_create_mixednet) is the same model part with three more plan inputs and the <VAR> form of the
// kernel below; a plain plan runs the form without VAR.
#include <hip/hip_runtime.h>

#include "stream_common.hip.h"

using namespace mww_stream_impl;

namespace {

constexpr int kMaxTensors = 3 + 2 * MWW_MAX_BLOCKS * MWW_STREAM_MAX_REPEAT;
// VAR: input, conv1, the logit; per block a residual; per repeat MixConv, 1x1 and ADD
constexpr int kMaxVarTensors = 3 + MWW_MAX_BLOCKS + 3 * MWW_MAX_BLOCKS * MWW_STREAM_MAX_REPEAT;
constexpr int kPoolChannels = 8;   // channels a head thread pools at a time (registers)

// Head over the last TP positions of the (gated) final map: pooling per channel when `pool`, then the Dense, sigmoid.
// gate: a[q] at gate[q - g_lo], or NULL.  Positions before the stream start read the head ring [TF - 1][C].
template <bool REC>
__device__ inline void variant_head(const SCall& a, const STile& T, const float* fin, int pitch, const float* hring, int64_t wd_at,
                                    int64_t bd_at, int C, int TF, int TP, int pool, const float* gate, int64_t g_lo, float& lmin,
                                    float& lmax) {
  for (int o = threadIdx.x; o < T.n; o += kStreamThreads) {
    const int64_t c = T.c0 + o, q0 = c - (TP - 1);
    float acc = a.w[bd_at];
    if (pool) {   // kPoolChannels channels at a time: a row is visited C / kPoolChannels times, not C times
      for (int ch0 = 0; ch0 < C; ch0 += kPoolChannels) {
        const int nc = C - ch0 < kPoolChannels ? C - ch0 : kPoolChannels;
        float p[kPoolChannels];
        for (int t = 0; t < TP; ++t) {   // every channel's frames in order
          const int64_t q = q0 + t;
          const float* x = (q >= 0 ? fin + q * pitch : hring + (TF - 1 + q) * C) + ch0;
          const float g = gate ? gate[q - g_lo] : 1.f;
#pragma unroll
          for (int j = 0; j < kPoolChannels; ++j) {
            if (j < nc) {
              const float v = gate ? x[j] * g : x[j];
              p[j] = t == 0 ? v : (pool == 1 ? p[j] + v : fmaxf(p[j], v));
            }
          }
        }
#pragma unroll
        for (int j = 0; j < kPoolChannels; ++j)
          if (j < nc) acc = fmaf(pool == 1 ? p[j] / (float)TP : p[j], a.w[wd_at + ch0 + j], acc);
      }
    } else {
      for (int t = 0; t < TP; ++t) {
        const int64_t q = q0 + t;
        const float* wd = a.w + wd_at + (int64_t)t * C;
        const float* x = q >= 0 ? fin + q * pitch : hring + (TF - 1 + q) * C;
        const float g = gate ? gate[q - g_lo] : 1.f;
        for (int ch = 0; ch < C; ++ch) acc = fmaf(x[ch] * g, wd[ch], acc);
      }
    }
    const int64_t g = T.out0 + o;
    a.logit[g] = acc;
    a.prob[g] = 1.f / (1.f + expf(-acc));
    if (REC) {
      lmin = fminf(lmin, acc);
      lmax = fmaxf(lmax, acc);
    }
  }
}

// The float MixedNet kernel: one tile walk, four instantiations.  <VAR> is the form of a plan with residual connections, a
// pooled head or spatial attention (mixednet.py:234-275 SpatialAttention, :340-358 residual, :362-381 pooled head); all it adds
// sits behind the compile-time VAR, so <false, *> - the kernel a plain plan runs (MixedNet::launch) - holds none of it:
//
//   residual   layer kind 2: r = folded BN(1x1(block input)), linear, over the block-input range [in_lo, c1) of the tile, in a
//              third activation buffer of the workgroup (allocated only when a block has a residual).  It has no ring: an
//              output position >= 0 reads the block input at the same position, which the tile holds.  Layer kind 3 - the 1x1
//              layers of that block, every repeat over its own output range - adds r at equal positions before the ReLU.
//   pooling    the head reduces the T_f frames it holds (head ring before the stream start: cold zeros take part) per channel,
//              average (sum in frame order, divided by the frames) or max, and the Dense reads the C pooled values.
//   attention  non_stream mode only.  a[q] depends on positions only, so it is one more right-aligned layer of reach 3: per
//              final-map position the channel mean and max, then the 4-tap gate; the head reads h[q] a[q] at the last T_f - 3.
//
// <REC> is the calibration form (mww_stream_calibrate_host): every thread keeps the min / max of the tensor it is computing - a
// kind-2 layer records r, a kind-3 layer the value before the add and the value after add + ReLU as two tensors, the head the
// logit -, rec_fold runs per layer, one partial row per workgroup.  <*, false> is the kernel without any of it.  The calibrated
// tensor of layer l is var.lt[l]; without VAR that is 2 + l, which needs no table.
template <bool VAR, bool REC>
__global__ void __launch_bounds__(kStreamThreads) stream_forward_kernel(SNet net, SVar var, SStores S, SCall a) {
  const int tid = threadIdx.x;
  constexpr int kRec = VAR ? kMaxVarTensors : kMaxTensors;
  __shared__ float red[REC ? 2 * kStreamThreads : 1], rmin[REC ? kRec : 1], rmax[REC ? kRec : 1];
  float lmin = INFINITY, lmax = -INFINITY, lmin2 = INFINITY, lmax2 = -INFINITY;   // (2, VAR: the ADD output of a kind-3 layer)
  if (REC) rec_init(a, rmin, rmax);
  float* G = a.scratch + (int64_t)blockIdx.x * a.scratch_per_wg;            // gathered padded input rows [.][40]
  float* B0 = G + ((a.buf_rows - 1) * net.s + net.k1) * MWW_FEATURE_BINS;   // two activation buffers [rows][cmax]
  float* B1 = B0 + a.buf_rows * net.cmax;
  float* Rb = B1 + a.buf_rows * net.cmax;                                   // VAR: the block's residual [rows][cmax] (has_res)
  float* At = Rb + (VAR && var.has_res ? a.buf_rows * net.cmax : 0);        // VAR: attention mean, max, gate [rows] each (att)
  const int r1 = a.use_state ? net.r1 : 0;
  for (int tile = blockIdx.x; tile < a.n_tiles; tile += gridDim.x) {
    const STile T = tile_of(a, tile);
    const int64_t c0 = T.c0, c1 = T.c1, v_seg = T.v_seg, N = T.c1;   // positions are conv1 indices
    const bool last = T.last;
    // ---- gather the padded input rows the tile's conv1 outputs read: P index p = v + r1 (v virtual frame in the segment)
    int64_t lo = c0 - net.reach1;
    if (lo < 0) lo = 0;
    const int64_t p0 = lo * net.s, p1 = (c1 - 1) * net.s + net.k1;
    for (int64_t idx = tid; idx < (p1 - p0) * MWW_FEATURE_BINS; idx += kStreamThreads) {
      const int64_t p = p0 + idx / MWW_FEATURE_BINS;
      const int bin = (int)(idx % MWW_FEATURE_BINS);
      const int64_t v = p - r1;
      const float x = v < 0 ? a.st_in[net.ring1 + (r1 + v) * MWW_FEATURE_BINS + bin] : frame_value(S, a, v_seg + v, bin);
      G[idx] = x;
      // conv1 ring after the call: the last r1 padded rows, P indices [N*s, N*s + r1)
      if (last && p >= N * net.s && p < N * net.s + r1) a.st_out[net.ring1 + (p - N * net.s) * MWW_FEATURE_BINS + bin] = x;
    }
    __syncthreads();
    // ---- conv1 (valid, stride s, no bias) + ReLU over positions [lo, c1)
    const int64_t n1 = c1 - lo;
    for (int64_t idx = tid; idx < n1 * net.c1; idx += kStreamThreads) {
      const int64_t i = idx / net.c1;
      const int co = (int)(idx % net.c1);
      const float* g = G + i * net.s * MWW_FEATURE_BINS;
      const float* w = a.w + net.w1 + co;
      float acc = 0.f;
      for (int r = 0; r < net.k1 * MWW_FEATURE_BINS; ++r) acc = fmaf(g[r], w[(int64_t)r * net.c1], acc);
      B0[i * net.cmax + co] = acc > 0.f ? acc : 0.f;
      if (REC) {
        lmin = fminf(lmin, B0[i * net.cmax + co]);
        lmax = fmaxf(lmax, B0[i * net.cmax + co]);
      }
    }
    __syncthreads();
    if (REC) {
      rec_fold(lmin, lmax, 1, red, rmin, rmax);
      lmin = INFINITY;
      lmax = -INFINITY;
    }
    float* in = B0;
    float* out = B1;
    int64_t in_lo = lo, r_lo = lo;   // (r_lo, VAR: the position of Rb's first row)
    for (int l = 0; l < net.n_layers; ++l) {
      const SLayer& L = net.L[l];
      const int lt = VAR ? var.lt[l] : 2 + l;   // the calibrated tensor (REC)
      if (VAR && L.kind == 2) {   // the block's residual over the block-input range; the buffers are not swapped
        const int Ci = L.cin, Co = L.cout;
        r_lo = in_lo;
        for (int64_t idx = tid; idx < (c1 - in_lo) * Co; idx += kStreamThreads) {
          const int64_t i = in_lo + idx / Co;
          const int co = (int)(idx % Co);
          const float* x = in + (i - in_lo) * net.cmax;
          const float* w = a.w + L.w + co;
          float acc = a.w[L.b + co];
          for (int ci = 0; ci < Ci; ++ci) acc = fmaf(x[ci], w[(int64_t)ci * Co], acc);
          Rb[(i - r_lo) * net.cmax + co] = acc;
          if (REC) {
            lmin = fminf(lmin, acc);
            lmax = fmaxf(lmax, acc);
          }
        }
        __syncthreads();
        if (REC) {
          rec_fold(lmin, lmax, lt, red, rmin, rmax);
          lmin = INFINITY;
          lmax = -INFINITY;
        }
        continue;
      }
      int64_t o_lo = c0 - L.reach;
      if (o_lo < 0) o_lo = 0;
      const int64_t no = c1 - o_lo;
      if (L.kind == 0) {
        const int C = L.cin, K = L.k, R = K - 1;
        const float* ring = a.st_in + L.ring;
        for (int64_t idx = tid; idx < no * C; idx += kStreamThreads) {
          const int64_t i = o_lo + idx / C;
          const int c = (int)(idx % C);
          float acc = a.w[L.b + c];
          for (int j = 0; j < K; ++j) {
            const int64_t q = i - R + j;
            const float x = q >= 0 ? in[(q - in_lo) * net.cmax + c] : ring[(R + q) * C + c];
            acc = fmaf(a.w[L.w + (int64_t)j * C + c], x, acc);
          }
          out[(i - o_lo) * net.cmax + c] = acc;
          if (REC) {
            lmin = fminf(lmin, acc);
            lmax = fmaxf(lmax, acc);
          }
        }
        if (last) {   // this layer's ring after the call: its input at positions [N - R, N)
          for (int idx = tid; idx < R * C; idx += kStreamThreads) {
            const int64_t q = N - R + idx / C;
            const int c = idx % C;
            a.st_out[L.ring + idx] = q >= 0 ? in[(q - in_lo) * net.cmax + c] : ring[(R + q) * C + c];
          }
        }
      } else {
        const int Ci = L.cin, Co = L.cout;
        const bool res = VAR && L.kind == 3;
        for (int64_t idx = tid; idx < no * Co; idx += kStreamThreads) {
          const int64_t i = o_lo + idx / Co;
          const int co = (int)(idx % Co);
          const float* x = in + (i - in_lo) * net.cmax;
          const float* w = a.w + L.w + co;
          float acc = a.w[L.b + co];
          for (int ci = 0; ci < Ci; ++ci) acc = fmaf(x[ci], w[(int64_t)ci * Co], acc);
          if (REC && res) {   // the 1x1 output before the add is a tensor of its own
            lmin = fminf(lmin, acc);
            lmax = fmaxf(lmax, acc);
          }
          if (res) acc += Rb[(i - r_lo) * net.cmax + co];   // o_lo >= r_lo: the residual covers the block input
          out[(i - o_lo) * net.cmax + co] = acc > 0.f ? acc : 0.f;
          if (REC && res) {   // (no reference picking one of the two pairs: that put them on the stack)
            lmin2 = fminf(lmin2, out[(i - o_lo) * net.cmax + co]);
            lmax2 = fmaxf(lmax2, out[(i - o_lo) * net.cmax + co]);
          } else if (REC) {
            lmin = fminf(lmin, out[(i - o_lo) * net.cmax + co]);
            lmax = fmaxf(lmax, out[(i - o_lo) * net.cmax + co]);
          }
        }
      }
      __syncthreads();
      if (REC) {
        rec_fold(lmin, lmax, lt, red, rmin, rmax);
        if (VAR && L.kind == 3) rec_fold(lmin2, lmax2, lt + 1, red, rmin, rmax);
        lmin = lmin2 = INFINITY;
        lmax = lmax2 = -INFINITY;
      }
      float* t = in;
      in = out;
      out = t;
      in_lo = o_lo;
    }
    // ---- head: Dense over the last T_f frames of the final map at every output position; VAR: gated and / or pooled first
    const float* fin = in - in_lo * net.cmax;
    const float* hring = a.st_in + net.ring_head;
    const float* gate = nullptr;
    if (VAR && var.att) {   // non_stream: every position the head reads is >= 0 and in the tile, in_lo = c0 - (tf - 1)
      const int C = net.c_last;
      const int64_t nq = c1 - in_lo;
      float *avg = At, *mx = At + a.buf_rows, *gt = mx + a.buf_rows;
      for (int64_t i = tid; i < nq; i += kStreamThreads) {
        const float* x = in + i * net.cmax;
        float s = 0.f, m = x[0];
        for (int ch = 0; ch < C; ++ch) {
          s += x[ch];
          m = fmaxf(m, x[ch]);
        }
        avg[i] = s / (float)C;
        mx[i] = m;
      }
      __syncthreads();
      const float* wa = a.w + var.wa;
      for (int64_t i = 3 + tid; i < nq; i += kStreamThreads) {
        float s = 0.f;
        for (int j = 0; j < 4; ++j) {
          s = fmaf(wa[2 * j], avg[i - 3 + j], s);
          s = fmaf(wa[2 * j + 1], mx[i - 3 + j], s);
        }
        gt[i] = 1.f / (1.f + expf(-s));
      }
      __syncthreads();
      gate = gt;
    }
    if (VAR && (var.att || var.pool)) {
      variant_head<REC>(a, T, fin, net.cmax, hring, net.wd, net.bd, net.c_last, net.tf, var.tp, var.pool, gate, in_lo, lmin, lmax);
    } else {
      dense_head<REC>(a, T, fin, net.cmax, hring, net.wd, net.bd, net.c_last, net.tf, lmin, lmax);
    }
    if (REC) {
      rec_fold(lmin, lmax, VAR ? var.n_tensors - 1 : 2 + net.n_layers, red, rmin, rmax);
      lmin = INFINITY;
      lmax = -INFINITY;
    }
    if (last) head_ring_store(a.st_out + net.ring_head, T, fin, net.cmax, hring, net.c_last, net.tf);
    __syncthreads();   // the next tile reuses the scratch
  }
  if (REC) rec_flush(a, rmin, rmax);
}

}  // namespace

// ---- MixedNet, float half of the model part (tu_stream_q8.hip has the int8 half)
namespace mww_stream_impl {

int MixedNet::upload() {
  int rc = upload_table(&d_layers, layers);
  if (!rc) rc = upload_table(&d_q8_off, q8_off);
  if (!rc) rc = upload_table(&d_lt, lt);
  net.L = d_layers;
  var.lt = d_lt;
  q.lw = d_q8_off;
  q.li = d_q8_off + net.n_layers;
  return rc;
}

int64_t MixedNet::fold_weights(const float* h, float* w) const {
  // Keras get_weights() order (mixednet.py:307-386): conv1.kernel [k1,1,40,F]; per block and repeat: per MixConv group
  // kernel [k,1,gc,1] + bias [gc], pointwise kernel [1,1,C,F], BN gamma, beta, moving_mean, moving_variance; dense [T_f*C,1], bias.
  // BatchNormalization (inference: moving statistics, eps 1e-3) is folded into the 1x1 weights and a bias once, here.
  int64_t p = 0;
  const int64_t n1 = (int64_t)net.k1 * MWW_FEATURE_BINS * net.c1;
  std::memcpy(&w[net.w1], h, (size_t)n1 * sizeof(float));
  p += n1;
  // a 1x1 layer (a block's residual included): kernel [1,1,Ci,Co], gamma, beta, moving_mean, moving_variance
  auto fold_pw = [&](const SLayer& P) {
    const int Ci = P.cin, Co = P.cout;
    const float* kern = h + p;
    const float *gamma = kern + (int64_t)Ci * Co, *beta = gamma + Co, *mean = beta + Co, *variance = mean + Co;
    for (int co = 0; co < Co; ++co) {
      const double sc = (double)gamma[co] / std::sqrt((double)variance[co] + 1e-3);
      for (int ci = 0; ci < Ci; ++ci) w[P.w + (int64_t)ci * Co + co] = (float)((double)kern[(int64_t)ci * Co + co] * sc);
      w[P.b + co] = (float)((double)beta[co] - (double)mean[co] * sc);
    }
    p += (int64_t)Ci * Co + 4 * Co;
  };
  int l = 0;
  for (int b = 0; b < d.n_blocks; ++b) {
    const int nk = d.n_kernels[b];
    if (residual[b]) fold_pw(layers[l++]);   // b.res.kernel + BN, in front of the block's repeats
    for (int r = 0; r < d.repeat[b]; ++r) {
      if (layers[l].kind == 0) {
        const SLayer& L = layers[l++];
        const int C = L.cin, K = L.k;
        int c0 = 0;
        for (int g = 0; g < nk; ++g) {
          const int gc = C / nk + (g == 0 ? C % nk : 0), k = d.kernels[b][g];
          for (int j = 0; j < k; ++j)
            for (int q = 0; q < gc; ++q) w[L.w + (int64_t)(K - k + j) * C + c0 + q] = h[p + (int64_t)j * gc + q];   // right-aligned taps
          p += (int64_t)k * gc;
          for (int q = 0; q < gc; ++q) w[L.b + c0 + q] = h[p + q];
          p += gc;
          c0 += gc;
        }
      }
      fold_pw(layers[l++]);
    }
  }
  if (var.att) {   // attention.kernel [4,1,2,1]: tap i, (avg, max)
    std::memcpy(&w[var.wa], h + p, 8 * sizeof(float));
    p += 8;
  }
  const int64_t nd = (int64_t)(var.pool ? 1 : var.tp) * net.c_last;
  std::memcpy(&w[net.wd], h + p, (size_t)nd * sizeof(float));
  w[net.bd] = h[p + nd];
  return p + nd + 1;
}

void MixedNet::launch(const SStores& S, const SCall& a, int grid, hipStream_t hs) const {
  auto kernel = variant() ? (a.rec ? stream_forward_kernel<true, true> : stream_forward_kernel<true, false>)
                          : (a.rec ? stream_forward_kernel<false, true> : stream_forward_kernel<false, false>);
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(kStreamThreads), 0, hs, net, var, S, a);
}

// ---- the host path of every stream: the front of mww_stream; whatever differs between the models is behind SModel
int stream_create(mww_ctx* ctx, SModel* m, int rc, mww_stream** out) {
  mww_stream* s = new mww_stream();
  s->ctx = ctx;
  s->model = m;
  void* stores[MWW_MAX_STORES];
  int dt[MWW_MAX_STORES];
  int64_t el[MWW_MAX_STORES];
  if (!rc) rc = mww::ctx_borrow(ctx, &s->device, &s->stream, stores, dt, el, &s->n_cu);
  if (!rc && hipSetDevice(s->device) != hipSuccess) rc = mww::set_error(MWW_ERR_HIP, "hipSetDevice failed");
  if (!rc && hipMalloc((void**)&s->w, (size_t)m->n_dev_w * sizeof(float)) != hipSuccess) rc = mww::set_error(MWW_ERR_HIP, "hipMalloc weights");
  if (!rc) rc = m->upload();
  for (int i = 0; i < 2 && !rc; ++i)
    if (hipMalloc((void**)&s->st[i], (size_t)(m->n_state + 1) * sizeof(float)) != hipSuccess) rc = mww::set_error(MWW_ERR_HIP, "hipMalloc state");
  if (!rc) rc = mww_stream_reset(s);
  if (rc) {
    mww_stream_destroy(s);
    return rc;
  }
  *out = s;
  return MWW_OK;
}

}  // namespace mww_stream_impl

namespace {

int no_int8(const mww_stream* s) {
  if (!s->model->int8_refusal.empty()) return mww::set_error(MWW_ERR_UNSUPPORTED, s->model->int8_refusal.c_str());
  return mww::set_error(MWW_ERR_UNSUPPORTED, "the int8 streaming model covers MixedNet streams only (this is a conv/BN graph stream; "
                                               "mww_stream_create_convnet_q8 creates one that takes int8 parameters)");
}

void q8_free(mww_stream* s) {
  for (void* p : {(void*)s->q8_w, (void*)s->q8_i, (void*)s->q8_lut, (void*)s->q8_st[0], (void*)s->q8_st[1], (void*)s->q8_out,
                  (void*)s->q8_scratch})
    if (p) (void)hipFree(p);
  s->q8_w = nullptr;
  s->q8_i = nullptr;
  s->q8_lut = nullptr;
  s->q8_st[0] = s->q8_st[1] = nullptr;
  s->q8_out = nullptr;
  s->q8_scratch = nullptr;
  s->cap_q8_out = s->cap_q8_scratch = 0;
  s->q8 = false;
}

// after a launch: in stream mode the rings this call wrote are the state of the next one
int64_t finish_call(mww_stream* s, int* cur, int64_t n_out) {
  SCHK(hipGetLastError());
  SCHK(hipStreamSynchronize(s->stream));
  if (s->model->g.mode == MWW_STREAM_MODE_STREAM) *cur ^= 1;
  return n_out;
}

int64_t launch_float(mww_stream* s, const SStores& S, SCall& a, int grid, float* rec) {
  const SModel& m = *s->model;
  int rc = grow(&s->scratch, &s->cap_scratch, m.scratch_per_wg * grid);
  if (rc) return rc;
  a.scratch = s->scratch;
  a.scratch_per_wg = m.scratch_per_wg;
  a.rec = rec;
  a.n_tensors = rec ? m.n_tensors : 0;
  m.launch(S, a, grid, s->stream);
  return finish_call(s, &s->cur, a.n_out);
}

// a tile's int8 buffers sit in LDS when they fit, else in a per-workgroup global scratch
int64_t launch_q8(mww_stream* s, const SStores& S, SCall& a, int grid) {
  const SModel& m = *s->model;
  int rc = grow(&s->q8_out, &s->cap_q8_out, a.n_out);
  if (rc) return rc;
  SQ8 q{};
  q.w = s->q8_w;
  q.iv = s->q8_i;
  q.lut = s->q8_lut;
  q.izp = m.q8_izp;
  q.in_scale = s->q8_in_scale;
  q.in_zp = s->q8_in_zp;
  q.out = s->q8_out;
  q.st_in = s->q8_st[s->q8_cur];
  q.st_out = s->q8_st[s->q8_cur ^ 1];
  q.use_lds = m.q8_tile_bytes <= kMaxLds;
  size_t lds = 0;
  if (q.use_lds) {
    lds = (size_t)m.q8_tile_bytes;
    if (lds > 64 * 1024) SCHK(hipFuncSetAttribute(m.q8_kernel(), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  } else {
    a.scratch_per_wg = (m.q8_tile_bytes + 255) & ~(int64_t)255;
    if ((rc = grow(&s->q8_scratch, &s->cap_q8_scratch, a.scratch_per_wg * grid))) return rc;
    q.scratch = s->q8_scratch;
  }
  m.launch_q8(S, a, q, grid, lds, s->stream);
  return finish_call(s, &s->q8_cur, a.n_out);
}

// one call over a track list: the int8 kernel once int8 parameters are loaded (except for calibration), else the float one
int64_t run_tracks(mww_stream* s, const mww_window* trk, int64_t n_trk, int64_t* out_off, int64_t n_host_frames, float* rec = nullptr) {
  if (!s->weights_set && !s->q8) return mww::set_error(MWW_ERR_STATE, "mww_stream_set_weights first");
  if (rec && s->model->g.mode != MWW_STREAM_MODE_STREAM) return mww::set_error(MWW_ERR_STATE, "calibration runs a stream-mode object");
  if (rec && !s->weights_set) return mww::set_error(MWW_ERR_STATE, "calibration runs the float weights: mww_stream_set_weights first");
  SStores S;
  SCall a;
  int grid = 0;
  const int64_t n_out = prepare_call(s, trk, n_trk, out_off, n_host_frames, S, a, &grid);
  if (n_out <= 0) return n_out;
  return s->q8 && !rec ? launch_q8(s, S, a, grid) : launch_float(s, S, a, grid, rec);
}

// the frames of a host call, uploaded as the one track of store kHostStore
int64_t run_host(mww_stream* s, const float* frames, int64_t n_frames, float* rec = nullptr) {
  SCHK(hipSetDevice(s->device));
  int rc = grow(&s->host_frames, &s->cap_host_frames, (n_frames + 1) * MWW_FEATURE_BINS);
  if (rc) return rc;
  if (n_frames) SCHK(hipMemcpyAsync(s->host_frames, frames, (size_t)n_frames * MWW_FEATURE_BINS * sizeof(float), hipMemcpyHostToDevice, s->stream));
  mww_window w{};
  w.store = -1;
  w.copy_rows = (int32_t)n_frames;
  int64_t off[2];
  return run_tracks(s, &w, 1, off, n_frames, rec);
}

}  // namespace

extern "C" {

int mww_stream_create(mww_ctx* ctx, const mww_stream_desc* d, mww_stream** out) {
  if (!ctx || !d || !out) return mww::set_error(MWW_ERR_INVALID, "null argument");
  *out = nullptr;
  MixedNet* m = new MixedNet();
  m->d = *d;
  return stream_create(ctx, m, m->plan(), out);
}

static int create_mixednet(mww_ctx* ctx, const mww_mixednet_stream_desc* d, bool q8_variant, mww_stream** out) {
  if (!ctx || !d || !out) return mww::set_error(MWW_ERR_INVALID, "null argument");
  *out = nullptr;
  MixedNet* m = new MixedNet();
  m->q8_variant = q8_variant;
  mww_stream_desc& b = m->d;   // the common part, field by field
  b.conv1_filters = d->conv1_filters;
  b.conv1_kernel = d->conv1_kernel;
  b.stride = d->stride;
  b.n_blocks = d->n_blocks;
  std::memcpy(b.repeat, d->repeat, sizeof(b.repeat));
  std::memcpy(b.n_kernels, d->n_kernels, sizeof(b.n_kernels));
  std::memcpy(b.kernels, d->kernels, sizeof(b.kernels));
  std::memcpy(b.pointwise_filters, d->pointwise_filters, sizeof(b.pointwise_filters));
  b.t_final = d->t_final;
  b.frames = d->frames;
  b.mode = d->mode;
  std::memcpy(m->residual, d->residual, sizeof(m->residual));
  m->att = d->spatial_attention;
  m->pool = d->pool;
  return stream_create(ctx, m, m->plan(), out);
}

int mww_stream_create_mixednet(mww_ctx* ctx, const mww_mixednet_stream_desc* d, mww_stream** out) {
  return create_mixednet(ctx, d, false, out);
}

int mww_stream_create_mixednet_q8(mww_ctx* ctx, const mww_mixednet_stream_desc* d, mww_stream** out) {
  return create_mixednet(ctx, d, true, out);
}

void mww_stream_destroy(mww_stream* s) {
  if (!s) return;
  (void)hipSetDevice(s->device);
  if (s->stream) (void)hipStreamSynchronize(s->stream);
  for (void* p : {(void*)s->w, (void*)s->st[0], (void*)s->st[1], (void*)s->prob, (void*)s->logit, (void*)s->scratch,
                  (void*)s->tables, (void*)s->host_frames, (void*)s->rec,
                  (void*)s->post_tab, (void*)s->post_scr, (void*)s->det_out, (void*)s->mine_buf})
    if (p) (void)hipFree(p);
  q8_free(s);
  delete s->model;
  delete s;
}

int64_t mww_stream_num_weights(const mww_stream* s) { return s ? s->model->n_weights : 0; }
int64_t mww_stream_num_state(const mww_stream* s) { return s ? s->model->n_state : 0; }

int mww_stream_set_weights(mww_stream* s, const float* h, int64_t n) {
  if (!s || !h) return mww::set_error(MWW_ERR_INVALID, "null argument");
  const SModel& m = *s->model;
  if (n != m.n_weights) return mww::set_error(MWW_ERR_INVALID, ("expected " + std::to_string(m.n_weights) + " Keras-order floats").c_str());
  std::vector<float> w((size_t)m.n_dev_w, 0.f);
  if (m.fold_weights(h, w.data()) != n) return mww::set_error(MWW_ERR_INVALID, "weight layout mismatch");
  SCHK(hipSetDevice(s->device));
  SCHK(hipMemcpyAsync(s->w, w.data(), (size_t)m.n_dev_w * sizeof(float), hipMemcpyHostToDevice, s->stream));
  SCHK(hipStreamSynchronize(s->stream));
  s->weights_set = true;
  return MWW_OK;
}

int mww_stream_reset(mww_stream* s) {
  if (!s) return mww::set_error(MWW_ERR_INVALID, "null argument");
  SCHK(hipSetDevice(s->device));
  SCHK(hipMemsetAsync(s->st[s->cur], 0, (size_t)(s->model->n_state + 1) * sizeof(float), s->stream));
  if (s->q8) SCHK(hipMemcpyAsync(s->q8_st[s->q8_cur], s->q8_state0.data(), s->q8_state0.size(), hipMemcpyHostToDevice, s->stream));
  SCHK(hipStreamSynchronize(s->stream));
  return MWW_OK;
}

int mww_stream_get_state(mww_stream* s, float* h, int64_t n) {
  if (!s || !h || n != s->model->n_state) return mww::set_error(MWW_ERR_INVALID, "state size mismatch");
  SCHK(hipSetDevice(s->device));
  SCHK(hipMemcpyAsync(h, s->st[s->cur], (size_t)n * sizeof(float), hipMemcpyDeviceToHost, s->stream));
  SCHK(hipStreamSynchronize(s->stream));
  return MWW_OK;
}

int64_t mww_stream_run(mww_stream* s, const mww_window* tracks, int64_t n_tracks, int64_t* out_offsets) {
  if (!s) return mww::set_error(MWW_ERR_INVALID, "null stream");
  for (int64_t t = 0; t < n_tracks; ++t)
    if (tracks[t].store < 0) return mww::set_error(MWW_ERR_INVALID, "track refers to a store that was not uploaded");
  return run_tracks(s, tracks, n_tracks, out_offsets, 0);
}

int64_t mww_stream_run_host(mww_stream* s, const float* frames, int64_t n_frames) {
  if (!s || (n_frames && !frames) || n_frames < 0 || n_frames > INT32_MAX) return mww::set_error(MWW_ERR_INVALID, "bad frames");
  return run_host(s, frames, n_frames);
}

int mww_stream_num_tensors(const mww_stream* s) {
  if (s && !s->model->int8) return no_int8(s);
  return s ? s->model->n_tensors : 0;
}

int mww_stream_calibrate_host(mww_stream* s, const float* frames, int64_t n_frames, float* ranges) {
  if (!s || !ranges || (n_frames && !frames) || n_frames < 0 || n_frames > INT32_MAX) return mww::set_error(MWW_ERR_INVALID, "bad frames");
  if (!s->model->int8) return no_int8(s);
  const int nt = s->model->n_tensors, stride = s->model->g.stride;
  for (int t = 0; t < nt; ++t) {
    ranges[2 * t] = INFINITY;
    ranges[2 * t + 1] = -INFINITY;
  }
  // the input tensor: every frame fed (chunks of s; the trailing L mod s frames are not), in order
  const int64_t fed = n_frames / stride * stride;
  for (int64_t i = 0; i < fed * MWW_FEATURE_BINS; ++i) {
    ranges[0] = fminf(ranges[0], frames[i]);
    ranges[1] = fmaxf(ranges[1], frames[i]);
  }
  SCHK(hipSetDevice(s->device));
  int rc = grow(&s->rec, &s->cap_rec, (int64_t)2 * s->n_cu * nt * 2);   // a launch has at most 2 x CU workgroups
  if (rc) return rc;
  const int64_t n_out = run_host(s, frames, n_frames, s->rec);
  if (n_out <= 0) return (int)n_out;
  std::vector<float> part((size_t)s->grid * nt * 2);   // one partial row per workgroup of the call just made
  SCHK(hipMemcpy(part.data(), s->rec, part.size() * sizeof(float), hipMemcpyDeviceToHost));
  for (int g = 0; g < s->grid; ++g)   // fixed order
    for (int t = 1; t < nt; ++t) {
      ranges[2 * t] = fminf(ranges[2 * t], part[((size_t)g * nt + t) * 2]);
      ranges[2 * t + 1] = fmaxf(ranges[2 * t + 1], part[((size_t)g * nt + t) * 2 + 1]);
    }
  return MWW_OK;
}

// The same over windows of resident stores: mww_stream_run with the <REC> form, the input range and the fold of the partial
// rows on the device (tu_stream_calibrate.hip).  Every track a whole number of strides, so the call is one concatenated stream.
int64_t mww_stream_calibrate(mww_stream* s, const mww_window* tracks, int64_t n_tracks, int64_t* out_offsets, float* ranges) {
  if (!s || !ranges || !out_offsets || (n_tracks > 0 && !tracks)) return mww::set_error(MWW_ERR_INVALID, "null argument");
  if (!s->model->int8) return no_int8(s);
  if (n_tracks <= 0) return mww::set_error(MWW_ERR_INVALID, "calibration needs at least one track");
  const int nt = s->model->n_tensors, stride = s->model->g.stride;
  for (int64_t t = 0; t < n_tracks; ++t) {
    if (tracks[t].store < 0) return mww::set_error(MWW_ERR_INVALID, "track refers to a store that was not uploaded");
    const int64_t rows = (int64_t)tracks[t].pad_rows + tracks[t].copy_rows;
    if (tracks[t].pad_rows >= 0 && tracks[t].copy_rows >= 0 && rows % stride)
      return mww::set_error(MWW_ERR_INVALID, ("calibration track " + std::to_string(t) + " has " + std::to_string(rows) +
                                              " rows, not a multiple of the stride " + std::to_string(stride)).c_str());
  }
  if (!s->weights_set) return mww::set_error(MWW_ERR_STATE, "calibration runs the float weights: mww_stream_set_weights first");
  if (s->model->g.mode != MWW_STREAM_MODE_STREAM) return mww::set_error(MWW_ERR_STATE, "calibration runs a stream-mode object");
  SCHK(hipSetDevice(s->device));
  SCalBuf b;
  int rc = calibrate_buffers(s, &b);
  if (rc) return rc;
  SStores S;
  SCall a;
  int grid = 0, n_in = 0;
  const int64_t n_out = prepare_call(s, tracks, n_tracks, out_offsets, 0, S, a, &grid);
  if (n_out < 0) return n_out;
  if (n_out == 0) {   // no frame fed: empty ranges, as the host form
    for (int t = 0; t < nt; ++t) {
      ranges[2 * t] = INFINITY;
      ranges[2 * t + 1] = -INFINITY;
    }
    return 0;
  }
  if ((rc = calibrate_input(s, S, a, b, n_out * stride, &n_in))) return rc;
  const int64_t n = launch_float(s, S, a, grid, b.rec);
  if (n < 0) return n;
  if ((rc = calibrate_fold(s, b, n_in, ranges))) return rc;
  return n;
}

int mww_stream_read(mww_stream* s, float* probs, float* logits, int64_t n) {
  if (!s || n < 0 || n > s->n_out) return mww::set_error(MWW_ERR_INVALID, "more outputs requested than the last run produced");
  if (!n) return MWW_OK;
  SCHK(hipSetDevice(s->device));
  if (probs) SCHK(hipMemcpyAsync(probs, s->prob, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, s->stream));
  if (logits && s->logit && n <= s->cap_logit) SCHK(hipMemcpyAsync(logits, s->logit, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, s->stream));
  SCHK(hipStreamSynchronize(s->stream));
  return MWW_OK;
}

int mww_stream_set_probs(mww_stream* s, const float* probs, int64_t n) {
  if (!s || n < 0 || (n && !probs)) return mww::set_error(MWW_ERR_INVALID, "bad probabilities");
  SCHK(hipSetDevice(s->device));
  int rc = grow(&s->prob, &s->cap_out, n + 1);
  if (rc) return rc;
  if (n) SCHK(hipMemcpyAsync(s->prob, probs, (size_t)n * sizeof(float), hipMemcpyHostToDevice, s->stream));
  SCHK(hipStreamSynchronize(s->stream));
  s->n_out = n;
  return MWW_OK;
}

// ---- int8 parameters (layout: include/mww.h); the model part says what it expects, validation and upload are here
int64_t mww_stream_q8_sizes(const mww_stream* s, int64_t* n_ints) {
  if (!s) return mww::set_error(MWW_ERR_INVALID, "null stream");
  if (!s->model->int8) return no_int8(s);
  if (n_ints) *n_ints = s->model->q8_ni;
  return s->model->q8_nw;
}

int mww_stream_set_quantized(mww_stream* s, const int8_t* weights, int64_t n_weights, const int32_t* ints, int64_t n_ints,
                             float input_scale, const uint8_t* lut) {
  if (!s || !weights || !ints || !lut) return mww::set_error(MWW_ERR_INVALID, "null argument");
  const SModel& m = *s->model;
  if (!m.int8) return no_int8(s);
  const int64_t nw = m.q8_nw, ni = m.q8_ni, izp = m.q8_izp;
  if (n_weights != nw || n_ints != ni)
    return mww::set_error(MWW_ERR_INVALID, ("expected " + std::to_string(nw) + " int8 weights and " + std::to_string(ni) + " int32 values").c_str());
  if (!(input_scale > 0.f) || !std::isfinite(input_scale)) return mww::set_error(MWW_ERR_INVALID, "input scale must be positive");
  for (int t = 0; t < m.n_tensors; ++t)
    if (ints[izp + t] < -128 || ints[izp + t] > 127) return mww::set_error(MWW_ERR_INVALID, "zero points must lie in [-128, 127]");
  // q8_requant shifts by at most 31 bits either way: QuantizeMultiplier emits shifts in [-31, 30] and multipliers >= 0,
  // anything else (from a hand-made .npz) would reach x >> e with e >= 32 on the device
  auto bad_requant = [&](int64_t at, int64_t cout) {
    for (int64_t c = 0; c < cout; ++c)
      if (ints[at + cout + c] < 0 || ints[at + 2 * cout + c] < -31 || ints[at + 2 * cout + c] > 30) return true;
    return false;
  };
  for (const auto& op : m.q8_requant)
    if (bad_requant(op.first, op.second))
      return mww::set_error(MWW_ERR_INVALID, "requantization multipliers must be >= 0 and shifts lie in [-31, 30]");
  for (int64_t at : m.q8_add)   // TFLite's int8 Add: three multipliers below one
    for (int k = 0; k < 3; ++k)
      if (ints[at + 2 * k] < 0 || ints[at + 2 * k + 1] < -31 || ints[at + 2 * k + 1] > 0)
        return mww::set_error(MWW_ERR_INVALID, "ADD multipliers must be >= 0 and their shifts lie in [-31, 0]");
  q8_free(s);
  std::vector<int8_t> st0((size_t)m.n_state + 4, 0);
  m.q8_state0(ints + izp, st0.data());
  SCHK(hipSetDevice(s->device));
  SCHK(hipMalloc((void**)&s->q8_w, (size_t)nw + 64));
  SCHK(hipMalloc((void**)&s->q8_i, (size_t)ni * 4 + 64));
  SCHK(hipMalloc((void**)&s->q8_lut, 256 + 64));
  for (int i = 0; i < 2; ++i) SCHK(hipMalloc((void**)&s->q8_st[i], st0.size()));
  SCHK(hipMemcpyAsync(s->q8_w, weights, (size_t)nw, hipMemcpyHostToDevice, s->stream));
  SCHK(hipMemcpyAsync(s->q8_i, ints, (size_t)ni * 4, hipMemcpyHostToDevice, s->stream));
  SCHK(hipMemcpyAsync(s->q8_lut, lut, 256, hipMemcpyHostToDevice, s->stream));
  SCHK(hipMemcpyAsync(s->q8_st[0], st0.data(), st0.size(), hipMemcpyHostToDevice, s->stream));   // the float state stays as it is
  SCHK(hipStreamSynchronize(s->stream));
  s->q8_state0 = st0;
  s->q8_in_scale = input_scale;
  s->q8_in_zp = ints[izp];
  s->q8_cur = 0;
  s->q8 = true;
  return MWW_OK;
}

int mww_stream_read_q8(mww_stream* s, uint8_t* out, int64_t n) {
  if (s && !s->model->int8) return no_int8(s);
  if (!s || !s->q8 || n < 0 || n > s->n_out || n > s->cap_q8_out || (n && !out)) return mww::set_error(MWW_ERR_INVALID, "more outputs requested than the last int8 run produced");
  if (!n) return MWW_OK;
  SCHK(hipSetDevice(s->device));
  SCHK(hipMemcpyAsync(out, s->q8_out, (size_t)n, hipMemcpyDeviceToHost, s->stream));
  SCHK(hipStreamSynchronize(s->stream));
  return MWW_OK;
}

int mww_stream_get_state_q8(mww_stream* s, int8_t* h, int64_t n) {
  if (s && !s->model->int8) return no_int8(s);
  if (!s || !s->q8 || !h || n != s->model->n_state) return mww::set_error(MWW_ERR_INVALID, "state size mismatch (or no int8 parameters)");
  SCHK(hipSetDevice(s->device));
  SCHK(hipMemcpyAsync(h, s->q8_st[s->q8_cur], (size_t)n, hipMemcpyDeviceToHost, s->stream));
  SCHK(hipStreamSynchronize(s->stream));
  return MWW_OK;
}

}  // extern "C"