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

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/mww.h"

namespace mww {
int ctx_borrow(mww_ctx* c, int* device, hipStream_t* stream, void** stores, int* dtypes, int64_t* elems, int* n_cu);
int set_error(int code, const char* msg);
}  // namespace mww

namespace {

constexpr int kStreamThreads = 256;
constexpr int kHostStore = MWW_MAX_STORES;   // store slot of the frames mww_stream_run_host uploads
constexpr int kTileOutputs = 256;            // outputs per tile (one head thread each)
constexpr float kScaleU16 = 0.0390625f;      // data.py:268-269 / inference.py:93-94

struct SLayer {
  int kind;          // 0: depthwise K taps + bias (fused MixConv groups, zero leading taps); 1: 1x1 + folded BN + ReLU
  int cin, cout, k;
  int64_t w, b;      // offsets into the weight buffer
  int64_t ring;      // depthwise: offset of its ring ((k - 1) x cin) in the state buffer
  int reach;         // conv1 positions between this layer's OUTPUT and the first head input of a tile
};

struct SNet {
  int k1, s, c1, r1, tf, c_last, n_layers, cmax;
  int64_t w1, wd, bd;        // conv1 [k1][40][c1], dense [tf * c_last], bias
  int64_t ring1, ring_head;  // conv1 ring [r1][40] (spectrogram rows), head ring [tf - 1][c_last]
  int reach1;                // conv1 positions of halo in front of a tile
  const SLayer* L;           // [n_layers], device memory (the kernel argument stays small)
};

struct SStores {
  const void* p[MWW_MAX_STORES + 1];
  int dtype[MWW_MAX_STORES + 1];
};

struct SCall {
  const mww_window* trk;     // [n_trk]
  const int64_t* trk_v0;     // [n_trk + 1] first virtual frame of each track
  int n_trk;
  const int64_t* seg_v0;     // segment start (virtual frame)
  const int* seg_coff;       // conv1 index of the segment's first output
  const int* tile_seg;
  const int64_t* tile_m0;    // first output of the tile inside its segment
  const int* tile_n;
  const int64_t* tile_out0;  // global output index of the tile's first output
  int n_tiles;
  int use_state;             // stream mode: padded positions read the rings
  int64_t n_out;             // outputs of the whole call (stream mode: the tile holding output n_out - 1 writes the rings)
  const float* w;
  const float* st_in;
  float* st_out;
  float* scratch;
  int64_t scratch_per_wg;    // floats
  int64_t buf_rows;          // rows of each activation buffer
  float* prob;
  float* logit;
};

__device__ inline float frame_value(const SStores& S, const SCall& a, int64_t v, int bin) {
  // binary search of the track holding virtual frame v
  int lo = 0, hi = a.n_trk - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (a.trk_v0[mid] <= v) lo = mid; else hi = mid - 1;
  }
  const mww_window w = a.trk[lo];
  const int64_t j = v - a.trk_v0[lo];
  if (j < w.pad_rows) return 0.f;   // fixed_length_spectrogram's zero rows in front of a short clip (data.py:107-113)
  const int64_t e = w.src_elem + (j - w.pad_rows) * MWW_FEATURE_BINS + bin;
  if (S.dtype[w.store] == MWW_DTYPE_U16) return (float)static_cast<const unsigned short*>(S.p[w.store])[e] * kScaleU16;
  return static_cast<const float*>(S.p[w.store])[e];
}

__global__ void __launch_bounds__(kStreamThreads) stream_forward_kernel(SNet net, SStores S, SCall a) {
  const int tid = threadIdx.x;
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
    }
    __syncthreads();
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
        }
      }
      __syncthreads();
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

struct mww_stream {
  mww_ctx* ctx = nullptr;
  int device = 0;
  hipStream_t stream = nullptr;
  int n_cu = 256;
  mww_stream_desc d{};
  SNet net{};
  std::vector<SLayer> layers;   // host copy of net.L
  SLayer* d_layers = nullptr;
  int64_t n_weights = 0;   // Keras-order floats
  int64_t n_dev_w = 0;     // folded device weights
  int64_t n_state = 0;
  int j0 = 0;              // non-stream: conv1 index of a track's first window
  float* w = nullptr;
  float* st[2] = {nullptr, nullptr};
  int cur = 0;
  bool weights_set = false;
  // per-call device buffers, grown on demand
  float* prob = nullptr;
  float* logit = nullptr;
  int64_t cap_out = 0, cap_logit = 0;
  float* scratch = nullptr;
  int64_t cap_scratch = 0;
  char* tables = nullptr;
  int64_t cap_tables = 0;
  float* host_frames = nullptr;
  int64_t cap_host_frames = 0;
  int64_t n_out = 0;       // outputs held in prob (last run or set_probs)
  // metrics
  char* mtab = nullptr;
  int64_t cap_mtab = 0;
};

namespace {

#define SCHK(expr)                                                                                      \
  do {                                                                                                  \
    hipError_t e_ = (expr);                                                                             \
    if (e_ != hipSuccess) return mww::set_error(MWW_ERR_HIP, (std::string(#expr) + ": " + hipGetErrorString(e_)).c_str()); \
  } while (0)

int unsupported(const std::string& m) { return mww::set_error(MWW_ERR_UNSUPPORTED, m.c_str()); }

template <class T>
int grow(T** p, int64_t* cap, int64_t n) {
  if (n <= *cap) return MWW_OK;
  if (*p) SCHK(hipFree(*p));
  *p = nullptr;
  *cap = 0;
  SCHK(hipMalloc((void**)p, (size_t)n * sizeof(T) + 64));
  *cap = n;
  return MWW_OK;
}

// topology + weight / state layout from the description; Keras-order size in *keras
int plan(const mww_stream_desc& d, SNet& net, std::vector<SLayer>& layers, int64_t* keras, int64_t* dev_w, int64_t* state, int* j0) {
  std::memset(&net, 0, sizeof(net));
  layers.assign((size_t)2 * MWW_MAX_BLOCKS * MWW_STREAM_MAX_REPEAT, SLayer{});
  if (d.mode != MWW_STREAM_MODE_STREAM && d.mode != MWW_STREAM_MODE_NON_STREAM) return unsupported("mode must be stream or non_stream");
  if (d.conv1_filters <= 0 || d.conv1_kernel <= 0 || d.stride <= 0)
    return unsupported("streaming needs a first convolution (first_conv_filters > 0, kernel and stride > 0)");
  if (d.n_blocks <= 0 || d.n_blocks > MWW_MAX_BLOCKS) return unsupported("n_blocks must be 1..8");
  if (d.t_final <= 0) return unsupported("t_final must be positive");
  net.k1 = d.conv1_kernel;
  net.s = d.stride;
  net.c1 = d.conv1_filters;
  net.r1 = d.conv1_kernel > d.stride ? d.conv1_kernel - d.stride : 0;
  net.tf = d.t_final;
  int64_t kw = (int64_t)net.k1 * MWW_FEATURE_BINS * net.c1, dw = kw, st = 0;
  net.w1 = 0;
  net.ring1 = st;
  st += (int64_t)net.r1 * MWW_FEATURE_BINS;
  int c = net.c1, cmax = net.c1, nl = 0, sum_r = 0;
  for (int b = 0; b < d.n_blocks; ++b) {
    const int nk = d.n_kernels[b], f = d.pointwise_filters[b];
    if (nk <= 0 || nk > MWW_STREAM_MAX_KERNELS) return unsupported("block " + std::to_string(b) + ": 1..8 MixConv kernels");
    if (d.repeat[b] <= 0 || d.repeat[b] > MWW_STREAM_MAX_REPEAT) return unsupported("block " + std::to_string(b) + ": repeat must be 1..4");
    if (f <= 0 || f > 1024) return unsupported("block " + std::to_string(b) + ": pointwise filters must be 1..1024");
    int K = 0;
    for (int g = 0; g < nk; ++g) {
      if (d.kernels[b][g] <= 0) return unsupported("block " + std::to_string(b) + ": kernel sizes must be positive");
      if (g && d.kernels[b][g] < d.kernels[b][g - 1]) return unsupported("mixconv kernel sizes must be ascending (alignment uses the last one)");
      K = d.kernels[b][g] > K ? d.kernels[b][g] : K;
    }
    for (int r = 0; r < d.repeat[b]; ++r) {
      if (K > 1) {   // MixConv: depthwise groups (+ bias) fused to one [K][C] table, own ring of K - 1 frames
        if (nk > c) return unsupported("more MixConv groups than channels");
        SLayer& L = layers[nl++];
        L.kind = 0; L.cin = c; L.cout = c; L.k = K;
        L.w = dw; dw += (int64_t)K * c;
        L.b = dw; dw += c;
        L.ring = st; st += (int64_t)(K - 1) * c;
        for (int g = 0; g < nk; ++g) kw += (int64_t)d.kernels[b][g] * (c / nk + (g == 0 ? c % nk : 0)) + (c / nk + (g == 0 ? c % nk : 0));
        sum_r += K - 1;
      }
      SLayer& P = layers[nl++];
      P.kind = 1; P.cin = c; P.cout = f; P.k = 1;
      P.w = dw; dw += (int64_t)c * f;
      P.b = dw; dw += f;
      kw += (int64_t)c * f + 4 * f;   // kernel, gamma, beta, moving mean, moving variance
      c = f;
      cmax = c > cmax ? c : cmax;
    }
  }
  net.n_layers = nl;
  net.c_last = c;
  net.cmax = cmax;
  net.wd = dw; dw += (int64_t)net.tf * c;
  net.bd = dw; dw += 1;
  kw += (int64_t)net.tf * c + 1;
  net.ring_head = st;
  st += (int64_t)(net.tf - 1) * c;
  // reach: conv1 positions between a layer's output and the first head input of a tile
  int reach = net.tf - 1;
  for (int l = nl - 1; l >= 0; --l) {
    layers[l].reach = reach;
    if (layers[l].kind == 0) reach += layers[l].k - 1;
  }
  layers.resize((size_t)nl);
  net.reach1 = reach;
  *j0 = 0;
  if (d.mode == MWW_STREAM_MODE_NON_STREAM) {
    if (d.frames < net.k1) return unsupported("non_stream mode needs frames >= the first convolution's kernel");
    const int n1 = (d.frames - net.k1) / net.s + 1;
    if (n1 - sum_r != net.tf)
      return unsupported("t_final " + std::to_string(net.tf) + " does not match a " + std::to_string(d.frames) + "-frame window (" +
                         std::to_string(n1 - sum_r) + " final frames)");
    *j0 = n1 - 1;
  }
  *keras = kw;
  *dev_w = dw;
  *state = st;
  return MWW_OK;
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
                  (void*)s->tables, (void*)s->host_frames, (void*)s->mtab, (void*)s->d_layers})
    if (p) (void)hipFree(p);
  delete s;
}

int64_t mww_stream_num_weights(const mww_stream* s) { return s ? s->n_weights : 0; }
int64_t mww_stream_num_state(const mww_stream* s) { return s ? s->n_state : 0; }

int mww_stream_set_weights(mww_stream* s, const float* h, int64_t n) {
  if (!s || !h) return mww::set_error(MWW_ERR_INVALID, "null argument");
  if (n != s->n_weights) return mww::set_error(MWW_ERR_INVALID, ("expected " + std::to_string(s->n_weights) + " Keras-order floats").c_str());
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
  return MWW_OK;
}

int mww_stream_get_state(mww_stream* s, float* h, int64_t n) {
  if (!s || !h || n != s->n_state) return mww::set_error(MWW_ERR_INVALID, "state size mismatch");
  SCHK(hipSetDevice(s->device));
  SCHK(hipMemcpyAsync(h, s->st[s->cur], (size_t)n * sizeof(float), hipMemcpyDeviceToHost, s->stream));
  SCHK(hipStreamSynchronize(s->stream));
  return MWW_OK;
}

static int64_t run_tracks(mww_stream* s, const mww_window* trk, int64_t n_trk, int64_t* out_off, const float* host_frames,
                          int64_t n_host_frames) {
  if (!s->weights_set) return mww::set_error(MWW_ERR_STATE, "mww_stream_set_weights first");
  if (n_trk < 0 || n_trk > INT32_MAX || (n_trk && !trk) || !out_off) return mww::set_error(MWW_ERR_INVALID, "bad track list");
  SStores S{};
  void* stores[MWW_MAX_STORES];
  int dt[MWW_MAX_STORES];
  int64_t el[MWW_MAX_STORES];
  int dev;
  hipStream_t hs;
  int ncu;
  int rc = mww::ctx_borrow(s->ctx, &dev, &hs, stores, dt, el, &ncu);
  if (rc) return rc;
  for (int i = 0; i < MWW_MAX_STORES; ++i) { S.p[i] = stores[i]; S.dtype[i] = dt[i]; }
  S.p[kHostStore] = s->host_frames;
  S.dtype[kHostStore] = MWW_DTYPE_F32;
  const SNet& net = s->net;
  const bool stream_mode = s->d.mode == MWW_STREAM_MODE_STREAM;
  const int T = s->d.frames;
  // per track: frames fed and outputs (predict_spectrogram: chunks of s, trailing L mod s frames never fed; non-stream:
  // windows ending at T, T + s, ... <= L)
  std::vector<int64_t> v0((size_t)n_trk + 1, 0);
  out_off[0] = 0;
  for (int64_t t = 0; t < n_trk; ++t) {
    const mww_window& w = trk[t];
    const int sid = w.store < 0 ? kHostStore : w.store;
    if (w.pad_rows < 0 || w.copy_rows < 0) return mww::set_error(MWW_ERR_INVALID, "negative track rows");
    if (w.store >= 0) {
      if (w.store >= MWW_MAX_STORES || !stores[w.store]) return mww::set_error(MWW_ERR_INVALID, "track refers to a store that was not uploaded");
      if (w.src_elem < 0 || w.src_elem + (int64_t)w.copy_rows * MWW_FEATURE_BINS > el[w.store])
        return mww::set_error(MWW_ERR_INVALID, "track reads past the end of its store");
    } else if (w.src_elem < 0 || w.src_elem + (int64_t)w.copy_rows * MWW_FEATURE_BINS > n_host_frames * MWW_FEATURE_BINS) {
      return mww::set_error(MWW_ERR_INVALID, "track reads past the host frames");
    }
    (void)sid;
    const int64_t L = (int64_t)w.pad_rows + w.copy_rows;
    int64_t n_o;
    if (stream_mode) {
      n_o = L / net.s;
      v0[t + 1] = v0[t] + n_o * net.s;
    } else {
      n_o = L >= T ? (L - T) / net.s + 1 : 0;
      v0[t + 1] = v0[t] + L;
    }
    out_off[t + 1] = out_off[t] + n_o;
  }
  const int64_t n_out = n_trk ? out_off[n_trk] : 0;
  s->n_out = n_out;
  if (n_out == 0) return 0;
  // segments and tiles
  std::vector<int64_t> seg_v0, tile_m0, tile_out0;
  std::vector<int> seg_coff, tile_seg, tile_n;
  auto add_tiles = [&](int sg, int64_t n, int64_t out0) {
    for (int64_t m = 0; m < n; m += kTileOutputs) {
      tile_seg.push_back(sg);
      tile_m0.push_back(m);
      tile_n.push_back((int)(n - m < kTileOutputs ? n - m : kTileOutputs));
      tile_out0.push_back(out0 + m);
    }
  };
  if (stream_mode) {
    seg_v0.push_back(0);
    seg_coff.push_back(0);
    add_tiles(0, n_out, 0);
  } else {
    for (int64_t t = 0; t < n_trk; ++t) {
      const int64_t n = out_off[t + 1] - out_off[t];
      if (!n) continue;
      seg_v0.push_back(v0[t]);
      seg_coff.push_back(s->j0);
      add_tiles((int)seg_v0.size() - 1, n, out_off[t]);
    }
  }
  const int n_tiles = (int)tile_seg.size();
  const int n_seg = (int)seg_v0.size();
  // one table upload: tracks, v0, segments, tiles
  auto al = [](int64_t b) { return (b + 255) & ~(int64_t)255; };
  const int64_t o_trk = 0, o_v0 = al(o_trk + n_trk * (int64_t)sizeof(mww_window)), o_sv0 = al(o_v0 + (n_trk + 1) * 8),
                o_sco = al(o_sv0 + n_seg * 8), o_tsg = al(o_sco + n_seg * 4), o_tm0 = al(o_tsg + n_tiles * 4),
                o_tn = al(o_tm0 + n_tiles * 8), o_to0 = al(o_tn + n_tiles * 4), bytes = al(o_to0 + n_tiles * 8);
  std::vector<char> tab((size_t)bytes, 0);
  std::memcpy(&tab[o_trk], trk, (size_t)n_trk * sizeof(mww_window));
  for (int64_t t = 0; t < n_trk; ++t)
    if (trk[t].store < 0) reinterpret_cast<mww_window*>(&tab[o_trk])[t].store = kHostStore;
  std::memcpy(&tab[o_v0], v0.data(), (size_t)(n_trk + 1) * 8);
  std::memcpy(&tab[o_sv0], seg_v0.data(), (size_t)n_seg * 8);
  std::memcpy(&tab[o_sco], seg_coff.data(), (size_t)n_seg * 4);
  std::memcpy(&tab[o_tsg], tile_seg.data(), (size_t)n_tiles * 4);
  std::memcpy(&tab[o_tm0], tile_m0.data(), (size_t)n_tiles * 8);
  std::memcpy(&tab[o_tn], tile_n.data(), (size_t)n_tiles * 4);
  std::memcpy(&tab[o_to0], tile_out0.data(), (size_t)n_tiles * 8);
  SCHK(hipSetDevice(s->device));
  if ((rc = grow(&s->tables, &s->cap_tables, bytes))) return rc;
  if ((rc = grow(&s->prob, &s->cap_out, n_out))) return rc;
  if ((rc = grow(&s->logit, &s->cap_logit, n_out))) return rc;
  const int grid = n_tiles < 2 * s->n_cu ? n_tiles : 2 * s->n_cu;
  const int64_t rows = kTileOutputs + net.reach1;
  const int64_t per_wg = al(((rows - 1) * net.s + net.k1) * MWW_FEATURE_BINS + 2 * rows * net.cmax);
  if ((rc = grow(&s->scratch, &s->cap_scratch, per_wg * grid))) return rc;
  SCHK(hipMemcpyAsync(s->tables, tab.data(), (size_t)bytes, hipMemcpyHostToDevice, s->stream));
  SCall a{};
  a.trk = reinterpret_cast<const mww_window*>(s->tables + o_trk);
  a.trk_v0 = reinterpret_cast<const int64_t*>(s->tables + o_v0);
  a.n_trk = (int)n_trk;
  a.seg_v0 = reinterpret_cast<const int64_t*>(s->tables + o_sv0);
  a.seg_coff = reinterpret_cast<const int*>(s->tables + o_sco);
  a.tile_seg = reinterpret_cast<const int*>(s->tables + o_tsg);
  a.tile_m0 = reinterpret_cast<const int64_t*>(s->tables + o_tm0);
  a.tile_n = reinterpret_cast<const int*>(s->tables + o_tn);
  a.tile_out0 = reinterpret_cast<const int64_t*>(s->tables + o_to0);
  a.n_tiles = n_tiles;
  a.use_state = stream_mode ? 1 : 0;
  a.n_out = n_out;
  a.w = s->w;
  a.st_in = s->st[s->cur];
  a.st_out = s->st[s->cur ^ 1];
  a.scratch = s->scratch;
  a.scratch_per_wg = per_wg;
  a.buf_rows = rows;
  a.prob = s->prob;
  a.logit = s->logit;
  hipLaunchKernelGGL(stream_forward_kernel, dim3(grid), dim3(kStreamThreads), 0, s->stream, net, S, a);
  SCHK(hipGetLastError());
  SCHK(hipStreamSynchronize(s->stream));   // the host tables above are released on return
  if (stream_mode) s->cur ^= 1;            // the rings this call wrote are the state of the next one
  return n_out;
}

int64_t mww_stream_run(mww_stream* s, const mww_window* tracks, int64_t n_tracks, int64_t* out_offsets) {
  if (!s) return mww::set_error(MWW_ERR_INVALID, "null stream");
  for (int64_t t = 0; t < n_tracks; ++t)
    if (tracks[t].store < 0) return mww::set_error(MWW_ERR_INVALID, "track refers to a store that was not uploaded");
  return run_tracks(s, tracks, n_tracks, out_offsets, nullptr, 0);
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
  return run_tracks(s, &w, 1, off, frames, n_frames);
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
