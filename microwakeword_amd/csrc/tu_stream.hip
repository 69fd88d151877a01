// Streaming inference and detection metrics (mww_stream_*, include/mww.h): the evaluation that follows training in the
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
#include <hip/hip_runtime.h>

#include "stream_common.hip.h"

using namespace mww_stream_impl;

namespace mww {
int64_t stream_q8_launch(mww_stream* s, const mww_stream_impl::SStores& S, mww_stream_impl::SCall& a, int grid);
int stream_q8_reset(mww_stream* s);
void stream_q8_free(mww_stream* s);
// conv/BN graph streams (tu_stream_graph.hip)
int stream_graph_set_weights(mww_stream* s, const float* h, int64_t n);
int64_t stream_graph_launch(mww_stream* s, const mww_stream_impl::SStores& S, mww_stream_impl::SCall& a, int grid);
void stream_graph_free(mww_stream* s);
int stream_graph_no_int8(const mww_stream* s);
bool stream_graph_int8(const mww_stream* s);   // created by mww_stream_create_convnet_q8
int stream_graph_num_tensors(const mww_stream* s);
int64_t stream_graph_q8_launch(mww_stream* s, const mww_stream_impl::SStores& S, mww_stream_impl::SCall& a, int grid);   // tu_stream_graph_q8.hip
}  // namespace mww

namespace {

constexpr int kMaxTensors = 3 + 2 * MWW_MAX_BLOCKS * MWW_STREAM_MAX_REPEAT;

template <bool REC>
__global__ void __launch_bounds__(kStreamThreads) stream_forward_kernel(SNet net, SStores S, SCall a) {
  const int tid = threadIdx.x;
  __shared__ float red[REC ? 2 * kStreamThreads : 1], rmin[REC ? kMaxTensors : 1], rmax[REC ? kMaxTensors : 1];
  float lmin = INFINITY, lmax = -INFINITY;
  if (REC) {
    for (int t = tid; t < a.n_tensors; t += kStreamThreads) {
      rmin[t] = INFINITY;
      rmax[t] = -INFINITY;
    }
    __syncthreads();
  }
  float* G = a.scratch + (int64_t)blockIdx.x * a.scratch_per_wg;            // gathered padded input rows [.][40]
  float* B0 = G + ((a.buf_rows - 1) * net.s + net.k1) * MWW_FEATURE_BINS;   // two activation buffers [rows][cmax]
  float* B1 = B0 + a.buf_rows * net.cmax;
  const int r1 = a.use_state ? net.r1 : 0;
  for (int tile = blockIdx.x; tile < a.n_tiles; tile += gridDim.x) {
    const int sg = a.tile_seg[tile];
    const int64_t c0 = a.tile_m0[tile] + a.seg_coff[sg];
    const int64_t c1 = c0 + a.tile_n[tile];
    const int64_t v_seg = a.seg_v0[sg];
    const bool last = a.use_state && a.tile_out0[tile] + a.tile_n[tile] == a.n_out;
    const int64_t N = c1;   // in stream mode the segment is the call and output n is conv1 index n
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
    int64_t in_lo = lo;
    for (int l = 0; l < net.n_layers; ++l) {
      const SLayer& L = net.L[l];
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
        for (int64_t idx = tid; idx < no * Co; idx += kStreamThreads) {
          const int64_t i = o_lo + idx / Co;
          const int co = (int)(idx % Co);
          const float* x = in + (i - in_lo) * net.cmax;
          const float* w = a.w + L.w + co;
          float acc = a.w[L.b + co];
          for (int ci = 0; ci < Ci; ++ci) acc = fmaf(x[ci], w[(int64_t)ci * Co], acc);
          out[(i - o_lo) * net.cmax + co] = acc > 0.f ? acc : 0.f;
          if (REC) {
            lmin = fminf(lmin, out[(i - o_lo) * net.cmax + co]);
            lmax = fmaxf(lmax, out[(i - o_lo) * net.cmax + co]);
          }
        }
      }
      __syncthreads();
      if (REC) {
        rec_fold(lmin, lmax, 2 + l, red, rmin, rmax);
        lmin = INFINITY;
        lmax = -INFINITY;
      }
      float* t = in;
      in = out;
      out = t;
      in_lo = o_lo;
    }
    // ---- head: Dense over the last T_f frames of the final map at every output position
    const int C = net.c_last, TF = net.tf;
    const float* hring = a.st_in + net.ring_head;
    for (int o = tid; o < a.tile_n[tile]; o += kStreamThreads) {
      const int64_t c = c0 + o;
      float acc = a.w[net.bd];
      for (int t = 0; t < TF; ++t) {
        const int64_t q = c - (TF - 1) + t;
        const float* wd = a.w + net.wd + (int64_t)t * C;
        if (q >= 0) {
          const float* x = in + (q - in_lo) * net.cmax;
          for (int ch = 0; ch < C; ++ch) acc = fmaf(x[ch], wd[ch], acc);
        } else {
          const float* x = hring + (TF - 1 + q) * C;
          for (int ch = 0; ch < C; ++ch) acc = fmaf(x[ch], wd[ch], acc);
        }
      }
      const int64_t g = a.tile_out0[tile] + o;
      a.logit[g] = acc;
      a.prob[g] = 1.f / (1.f + expf(-acc));
      if (REC) {
        lmin = fminf(lmin, acc);
        lmax = fmaxf(lmax, acc);
      }
    }
    if (REC) {
      rec_fold(lmin, lmax, 2 + net.n_layers, red, rmin, rmax);
      lmin = INFINITY;
      lmax = -INFINITY;
    }
    if (last) {
      for (int idx = tid; idx < (TF - 1) * C; idx += kStreamThreads) {
        const int64_t q = N - (TF - 1) + idx / C;
        const int ch = idx % C;
        a.st_out[net.ring_head + idx] = q >= 0 ? in[(q - in_lo) * net.cmax + ch] : hring[(TF - 1 + q) * C + ch];
      }
    }
    __syncthreads();   // the next tile reuses the scratch
  }
  if (REC)
    for (int t = tid; t < a.n_tensors; t += kStreamThreads) {
      a.rec[((int64_t)blockIdx.x * a.n_tensors + t) * 2] = rmin[t];
      a.rec[((int64_t)blockIdx.x * a.n_tensors + t) * 2 + 1] = rmax[t];
    }
}

// Detection metrics (test.py:94-137 compute_false_accepts_per_hour, :329-376).  One workgroup per track: thread j < n_cut
// scans the ambient track's moving average sequentially with the cooldown of cutoff j; one thread takes the positive
// track's score.  Moving average: float32, summed in order then divided (numpy .mean of the float32 sliding window).
__global__ void __launch_bounds__(128) stream_metrics_kernel(const float* prob, const int64_t* off, const int* kind, int n_trk,
                                                             int win, int skip, int cooldown, const double* cut, int n_cut,
                                                             unsigned long long* counts, int64_t* ma_len, float* score) {
  const int t = blockIdx.x;
  if (t >= n_trk) return;
  const int j = threadIdx.x;
  const int64_t b = off[t], n = off[t + 1] - off[t];
  if (kind[t] == 0) {
    const int64_t m = n >= win ? n - win + 1 : 0;
    if (j == 0) { ma_len[t] = m; score[t] = 0.f; }
    if (j < n_cut) {
      const double c = cut[j];
      int cd = cooldown;
      unsigned long long fa = 0;
      for (int64_t i = 0; i < m; ++i) {
        float s = 0.f;
        for (int k = 0; k < win; ++k) s += prob[b + i + k];
        const float avg = s / (float)win;
        cd = cd > 0 ? cd - 1 : 0;
        if (cd == 0 && (double)avg > c) {
          ++fa;
          cd = cooldown;
        }
      }
      counts[(int64_t)t * n_cut + j] = fa;
    }
  } else {
    if (j < n_cut) counts[(int64_t)t * n_cut + j] = 0;
    if (j == 0) {
      const int64_t r = n > skip ? n - skip : 0;
      const int64_t m = r >= win ? r - win + 1 : 0;
      float best = -INFINITY;
      for (int64_t i = 0; i < m; ++i) {
        float s = 0.f;
        for (int k = 0; k < win; ++k) s += prob[b + skip + i + k];
        const float avg = s / (float)win;
        best = avg > best ? avg : best;
      }
      ma_len[t] = m;
      score[t] = best;
    }
  }
}

// per-cutoff sum over the tracks, in track order
__global__ void stream_counts_sum_kernel(const unsigned long long* counts, int n_trk, int n_cut, unsigned long long* total) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n_cut) return;
  unsigned long long s = 0;
  for (int t = 0; t < n_trk; ++t) s += counts[(int64_t)t * n_cut + j];
  total[j] = s;
}

}  // namespace

extern "C" {

int mww_stream_create(mww_ctx* ctx, const mww_stream_desc* d, mww_stream** out) {
  if (!ctx || !d || !out) return mww::set_error(MWW_ERR_INVALID, "null argument");
  *out = nullptr;
  mww_stream* s = new mww_stream();
  s->ctx = ctx;
  s->d = *d;
  int rc = plan(*d, s->net, s->layers, &s->n_weights, &s->n_dev_w, &s->n_state, &s->j0);
  void* stores[MWW_MAX_STORES];
  int dt[MWW_MAX_STORES];
  int64_t el[MWW_MAX_STORES];
  if (!rc) rc = mww::ctx_borrow(ctx, &s->device, &s->stream, stores, dt, el, &s->n_cu);
  if (!rc && hipSetDevice(s->device) != hipSuccess) rc = mww::set_error(MWW_ERR_HIP, "hipSetDevice failed");
  if (!rc && hipMalloc((void**)&s->w, (size_t)s->n_dev_w * sizeof(float)) != hipSuccess) rc = mww::set_error(MWW_ERR_HIP, "hipMalloc weights");
  if (!rc && hipMalloc((void**)&s->d_layers, s->layers.size() * sizeof(SLayer) + 64) != hipSuccess) rc = mww::set_error(MWW_ERR_HIP, "hipMalloc layers");
  if (!rc && hipMemcpy(s->d_layers, s->layers.data(), s->layers.size() * sizeof(SLayer), hipMemcpyHostToDevice) != hipSuccess)
    rc = mww::set_error(MWW_ERR_HIP, "hipMemcpy layers");
  s->net.L = s->d_layers;
  for (int i = 0; i < 2 && !rc; ++i)
    if (hipMalloc((void**)&s->st[i], (size_t)(s->n_state + 1) * sizeof(float)) != hipSuccess) rc = mww::set_error(MWW_ERR_HIP, "hipMalloc state");
  if (!rc) rc = mww_stream_reset(s);
  if (rc) {
    mww_stream_destroy(s);
    return rc;
  }
  *out = s;
  return MWW_OK;
}

void mww_stream_destroy(mww_stream* s) {
  if (!s) return;
  (void)hipSetDevice(s->device);
  if (s->stream) (void)hipStreamSynchronize(s->stream);
  for (void* p : {(void*)s->w, (void*)s->st[0], (void*)s->st[1], (void*)s->prob, (void*)s->logit, (void*)s->scratch,
                  (void*)s->tables, (void*)s->host_frames, (void*)s->mtab, (void*)s->d_layers, (void*)s->rec})
    if (p) (void)hipFree(p);
  mww::stream_q8_free(s);
  mww::stream_graph_free(s);
  delete s;
}

int64_t mww_stream_num_weights(const mww_stream* s) { return s ? s->n_weights : 0; }
int64_t mww_stream_num_state(const mww_stream* s) { return s ? s->n_state : 0; }

int mww_stream_set_weights(mww_stream* s, const float* h, int64_t n) {
  if (!s || !h) return mww::set_error(MWW_ERR_INVALID, "null argument");
  if (n != s->n_weights) return mww::set_error(MWW_ERR_INVALID, ("expected " + std::to_string(s->n_weights) + " Keras-order floats").c_str());
  if (s->graph) return mww::stream_graph_set_weights(s, h, n);
  // Keras get_weights() order (mixednet.py:307-386): conv1.kernel [k1,1,40,F]; per block and repeat: per MixConv group
  // kernel [k,1,gc,1] + bias [gc], pointwise kernel [1,1,C,F], BN gamma, beta, moving_mean, moving_variance; dense [T_f*C,1], bias.
  // BatchNormalization (inference: moving statistics, eps 1e-3) is folded into the 1x1 weights and a bias once, here.
  const SNet& net = s->net;
  std::vector<float> w((size_t)s->n_dev_w, 0.f);
  int64_t p = 0;
  const int64_t n1 = (int64_t)net.k1 * MWW_FEATURE_BINS * net.c1;
  std::memcpy(&w[net.w1], h, (size_t)n1 * sizeof(float));
  p += n1;
  int l = 0;
  for (int b = 0; b < s->d.n_blocks; ++b) {
    const int nk = s->d.n_kernels[b];
    for (int r = 0; r < s->d.repeat[b]; ++r) {
      if (s->layers[l].kind == 0) {
        const SLayer& L = s->layers[l++];
        const int C = L.cin, K = L.k;
        int c0 = 0;
        for (int g = 0; g < nk; ++g) {
          const int gc = C / nk + (g == 0 ? C % nk : 0), k = s->d.kernels[b][g];
          for (int j = 0; j < k; ++j)
            for (int q = 0; q < gc; ++q) w[L.w + (int64_t)(K - k + j) * C + c0 + q] = h[p + (int64_t)j * gc + q];   // right-aligned taps
          p += (int64_t)k * gc;
          for (int q = 0; q < gc; ++q) w[L.b + c0 + q] = h[p + q];
          p += gc;
          c0 += gc;
        }
      }
      const SLayer& P = s->layers[l++];
      const int Ci = P.cin, Co = P.cout;
      const float* kern = h + p;
      const float *gamma = kern + (int64_t)Ci * Co, *beta = gamma + Co, *mean = beta + Co, *var = mean + Co;
      for (int co = 0; co < Co; ++co) {
        const double sc = (double)gamma[co] / std::sqrt((double)var[co] + 1e-3);
        for (int ci = 0; ci < Ci; ++ci) w[P.w + (int64_t)ci * Co + co] = (float)((double)kern[(int64_t)ci * Co + co] * sc);
        w[P.b + co] = (float)((double)beta[co] - (double)mean[co] * sc);
      }
      p += (int64_t)Ci * Co + 4 * Co;
    }
  }
  const int64_t nd = (int64_t)net.tf * net.c_last;
  std::memcpy(&w[net.wd], h + p, (size_t)nd * sizeof(float));
  w[net.bd] = h[p + nd];
  p += nd + 1;
  if (p != n) return mww::set_error(MWW_ERR_INVALID, "weight layout mismatch");
  SCHK(hipSetDevice(s->device));
  SCHK(hipMemcpyAsync(s->w, w.data(), (size_t)s->n_dev_w * sizeof(float), hipMemcpyHostToDevice, s->stream));
  SCHK(hipStreamSynchronize(s->stream));
  s->weights_set = true;
  return MWW_OK;
}

int mww_stream_reset(mww_stream* s) {
  if (!s) return mww::set_error(MWW_ERR_INVALID, "null argument");
  SCHK(hipSetDevice(s->device));
  SCHK(hipMemsetAsync(s->st[s->cur], 0, (size_t)(s->n_state + 1) * sizeof(float), s->stream));
  SCHK(hipStreamSynchronize(s->stream));
  return s->q8 ? mww::stream_q8_reset(s) : MWW_OK;
}

int mww_stream_get_state(mww_stream* s, float* h, int64_t n) {
  if (!s || !h || n != s->n_state) return mww::set_error(MWW_ERR_INVALID, "state size mismatch");
  SCHK(hipSetDevice(s->device));
  SCHK(hipMemcpyAsync(h, s->st[s->cur], (size_t)n * sizeof(float), hipMemcpyDeviceToHost, s->stream));
  SCHK(hipStreamSynchronize(s->stream));
  return MWW_OK;
}

// one call over a track list: the int8 kernel once int8 parameters are loaded (except for calibration), else the float one
static int64_t run_tracks(mww_stream* s, const mww_window* trk, int64_t n_trk, int64_t* out_off, int64_t n_host_frames,
                          float* rec = nullptr) {
  if (!s->weights_set && !s->q8) return mww::set_error(MWW_ERR_STATE, "mww_stream_set_weights first");
  if (rec && s->d.mode != MWW_STREAM_MODE_STREAM) return mww::set_error(MWW_ERR_STATE, "calibration runs a stream-mode object");
  if (rec && !s->weights_set) return mww::set_error(MWW_ERR_STATE, "calibration runs the float weights: mww_stream_set_weights first");
  SStores S;
  SCall a;
  int grid = 0;
  const int64_t n_out = prepare_call(s, trk, n_trk, out_off, n_host_frames, S, a, &grid);
  if (n_out <= 0) return n_out;
  if (s->graph) {
    if (s->q8 && !rec) return mww::stream_graph_q8_launch(s, S, a, grid);
    a.rec = rec;
    a.n_tensors = rec ? mww::stream_graph_num_tensors(s) : 0;
    return mww::stream_graph_launch(s, S, a, grid);
  }
  if (s->q8 && !rec) return mww::stream_q8_launch(s, S, a, grid);
  const SNet& net = s->net;
  const int64_t rows = a.buf_rows;
  const int64_t per_wg = (((rows - 1) * net.s + net.k1) * MWW_FEATURE_BINS + 2 * rows * net.cmax + 255) & ~(int64_t)255;
  int rc = grow(&s->scratch, &s->cap_scratch, per_wg * grid);
  if (rc) return rc;
  a.w = s->w;
  a.st_in = s->st[s->cur];
  a.st_out = s->st[s->cur ^ 1];
  a.scratch = s->scratch;
  a.scratch_per_wg = per_wg;
  if (rec) {
    a.n_tensors = net.n_layers + 3;
    a.rec = rec;
    hipLaunchKernelGGL(stream_forward_kernel<true>, dim3(grid), dim3(kStreamThreads), 0, s->stream, net, S, a);
  } else {
    hipLaunchKernelGGL(stream_forward_kernel<false>, dim3(grid), dim3(kStreamThreads), 0, s->stream, net, S, a);
  }
  SCHK(hipGetLastError());
  SCHK(hipStreamSynchronize(s->stream));
  if (s->d.mode == MWW_STREAM_MODE_STREAM) s->cur ^= 1;   // the rings this call wrote are the state of the next one
  return n_out;
}

int64_t mww_stream_run(mww_stream* s, const mww_window* tracks, int64_t n_tracks, int64_t* out_offsets) {
  if (!s) return mww::set_error(MWW_ERR_INVALID, "null stream");
  for (int64_t t = 0; t < n_tracks; ++t)
    if (tracks[t].store < 0) return mww::set_error(MWW_ERR_INVALID, "track refers to a store that was not uploaded");
  return run_tracks(s, tracks, n_tracks, out_offsets, 0);
}

int64_t mww_stream_run_host(mww_stream* s, const float* frames, int64_t n_frames) {
  if (!s || (n_frames && !frames) || n_frames < 0 || n_frames > INT32_MAX) return mww::set_error(MWW_ERR_INVALID, "bad frames");
  SCHK(hipSetDevice(s->device));
  int rc = grow(&s->host_frames, &s->cap_host_frames, (n_frames + 1) * MWW_FEATURE_BINS);
  if (rc) return rc;
  if (n_frames) SCHK(hipMemcpyAsync(s->host_frames, frames, (size_t)n_frames * MWW_FEATURE_BINS * sizeof(float), hipMemcpyHostToDevice, s->stream));
  mww_window w{};
  w.store = -1;
  w.copy_rows = (int32_t)n_frames;
  int64_t off[2];
  return run_tracks(s, &w, 1, off, n_frames);
}

int mww_stream_num_tensors(const mww_stream* s) {
  if (s && s->graph) return mww::stream_graph_int8(s) ? mww::stream_graph_num_tensors(s) : mww::stream_graph_no_int8(s);
  return s ? s->net.n_layers + 3 : 0;
}

int mww_stream_calibrate_host(mww_stream* s, const float* frames, int64_t n_frames, float* ranges) {
  if (!s || !ranges || (n_frames && !frames) || n_frames < 0 || n_frames > INT32_MAX) return mww::set_error(MWW_ERR_INVALID, "bad frames");
  if (s->graph && !mww::stream_graph_int8(s)) return mww::stream_graph_no_int8(s);
  const int nt = s->graph ? mww::stream_graph_num_tensors(s) : s->net.n_layers + 3;
  for (int t = 0; t < nt; ++t) {
    ranges[2 * t] = INFINITY;
    ranges[2 * t + 1] = -INFINITY;
  }
  // the input tensor: every frame fed (chunks of s; the trailing L mod s frames are not), in order
  const int64_t fed = n_frames / s->net.s * s->net.s;
  for (int64_t i = 0; i < fed * MWW_FEATURE_BINS; ++i) {
    ranges[0] = fminf(ranges[0], frames[i]);
    ranges[1] = fmaxf(ranges[1], frames[i]);
  }
  SCHK(hipSetDevice(s->device));
  int rc = grow(&s->host_frames, &s->cap_host_frames, (n_frames + 1) * MWW_FEATURE_BINS);
  if (!rc) rc = grow(&s->rec, &s->cap_rec, (int64_t)2 * s->n_cu * nt * 2);
  if (rc) return rc;
  if (n_frames) SCHK(hipMemcpyAsync(s->host_frames, frames, (size_t)n_frames * MWW_FEATURE_BINS * sizeof(float), hipMemcpyHostToDevice, s->stream));
  mww_window w{};
  w.store = -1;
  w.copy_rows = (int32_t)n_frames;
  int64_t off[2];
  const int64_t n_out = run_tracks(s, &w, 1, off, n_frames, s->rec);
  if (n_out <= 0) return (int)n_out;
  const int64_t n_tiles = (n_out + s->tile_outputs - 1) / s->tile_outputs;
  const int grid = (int)(n_tiles < 2 * s->n_cu ? n_tiles : 2 * s->n_cu);
  std::vector<float> part((size_t)grid * nt * 2);
  SCHK(hipMemcpy(part.data(), s->rec, part.size() * sizeof(float), hipMemcpyDeviceToHost));
  for (int g = 0; g < grid; ++g)   // fixed order
    for (int t = 1; t < nt; ++t) {
      ranges[2 * t] = fminf(ranges[2 * t], part[((size_t)g * nt + t) * 2]);
      ranges[2 * t + 1] = fmaxf(ranges[2 * t + 1], part[((size_t)g * nt + t) * 2 + 1]);
    }
  return MWW_OK;
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

int mww_stream_metrics(mww_stream* s, const int64_t* offsets, const int32_t* kind, int64_t n_tracks, int window, int skip,
                       int cooldown, const double* cutoffs, int n_cutoffs, uint64_t* counts, int64_t* ma_len, float* score) {
  if (!s || !offsets || !kind || !cutoffs || !counts || !ma_len || !score) return mww::set_error(MWW_ERR_INVALID, "null argument");
  if (n_tracks <= 0 || n_tracks > INT32_MAX || window <= 0 || skip < 0 || cooldown < 0 || n_cutoffs <= 0 || n_cutoffs > 128)
    return mww::set_error(MWW_ERR_INVALID, "bad metric arguments (1..128 cutoffs)");
  if (offsets[0] < 0 || offsets[n_tracks] > s->n_out) return mww::set_error(MWW_ERR_INVALID, "track offsets exceed the probabilities held");
  for (int64_t t = 0; t < n_tracks; ++t)
    if (offsets[t + 1] < offsets[t]) return mww::set_error(MWW_ERR_INVALID, "track offsets must not decrease");
  auto al = [](int64_t b) { return (b + 255) & ~(int64_t)255; };
  const int64_t o_off = 0, o_kind = al((n_tracks + 1) * 8), o_cut = al(o_kind + n_tracks * 4), o_cnt = al(o_cut + n_cutoffs * 8),
                o_len = al(o_cnt + n_tracks * n_cutoffs * 8), o_sc = al(o_len + n_tracks * 8), o_tot = al(o_sc + n_tracks * 4),
                bytes = al(o_tot + n_cutoffs * 8);
  SCHK(hipSetDevice(s->device));
  int rc = grow(&s->mtab, &s->cap_mtab, bytes);
  if (rc) return rc;
  std::vector<char> h((size_t)o_cnt, 0);
  std::memcpy(&h[o_off], offsets, (size_t)(n_tracks + 1) * 8);
  std::memcpy(&h[o_kind], kind, (size_t)n_tracks * 4);
  std::memcpy(&h[o_cut], cutoffs, (size_t)n_cutoffs * 8);
  SCHK(hipMemcpyAsync(s->mtab, h.data(), (size_t)o_cnt, hipMemcpyHostToDevice, s->stream));
  auto* cnt = reinterpret_cast<unsigned long long*>(s->mtab + o_cnt);
  auto* len = reinterpret_cast<int64_t*>(s->mtab + o_len);
  auto* sc = reinterpret_cast<float*>(s->mtab + o_sc);
  auto* tot = reinterpret_cast<unsigned long long*>(s->mtab + o_tot);
  hipLaunchKernelGGL(stream_metrics_kernel, dim3((unsigned)n_tracks), dim3(128), 0, s->stream, (const float*)s->prob,
                     reinterpret_cast<const int64_t*>(s->mtab + o_off), reinterpret_cast<const int*>(s->mtab + o_kind), (int)n_tracks,
                     window, skip, cooldown, reinterpret_cast<const double*>(s->mtab + o_cut), n_cutoffs, cnt, len, sc);
  SCHK(hipGetLastError());
  hipLaunchKernelGGL(stream_counts_sum_kernel, dim3(1), dim3(128), 0, s->stream, (const unsigned long long*)cnt, (int)n_tracks, n_cutoffs, tot);
  SCHK(hipGetLastError());
  SCHK(hipMemcpyAsync(counts, tot, (size_t)n_cutoffs * 8, hipMemcpyDeviceToHost, s->stream));
  SCHK(hipMemcpyAsync(ma_len, len, (size_t)n_tracks * 8, hipMemcpyDeviceToHost, s->stream));
  SCHK(hipMemcpyAsync(score, sc, (size_t)n_tracks * 4, hipMemcpyDeviceToHost, s->stream));
  SCHK(hipStreamSynchronize(s->stream));
  return MWW_OK;
}

}  // extern "C"