// Shared by the streaming units.  A stream (mww_stream) has a front every stream has - context, per-call track /
// segment / tile tables, outputs, float weights and state, int8 parameters and state; its host path is tu_stream.hip - and a
// model part (SModel): MixedNet (tu_stream.hip float, tu_stream_q8.hip int8, each kernel with a <VAR> form for residuals /
// pooling / attention; its plan is here) or a conv/BN graph (stream_graph.hip.h).  The model's virtual functions are the one
// place the two kinds are told apart.  The device code all four kernels share is here too: the tile header, the Dense heads,
// the head-ring write-back and the calibration (REC) folds.
// The kernels walk the same tiles and the same ring layout; only the element type and the arithmetic differ.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/mww.h"
#include "int8_ops.hip.h"

namespace mww {
int ctx_borrow(mww_ctx* c, int* device, hipStream_t* stream, void** stores, int* dtypes, int64_t* elems, int* n_cu);
int set_error(int code, const char* msg);
}  // namespace mww

namespace mww_stream_impl {

constexpr int kStreamThreads = 256;
constexpr int kHostStore = MWW_MAX_STORES;   // store slot of the frames mww_stream_run_host uploads
constexpr int kTileOutputs = 256;            // outputs per tile (one head thread each)
constexpr float kScaleU16 = 0.0390625f;      // data.py:268-269 / inference.py:93-94
constexpr int64_t kMaxLds = 160 * 1024;      // LDS of a gfx950 CU: an int8 tile that fits sits there
constexpr float kInv255 = (float)(1.0 / 255.0);   // inference.py:170 1 / 255 as float32

inline int64_t r4(int64_t n) { return (n + 3) & ~(int64_t)3; }   // int8 rows and weight slices are padded to 32-bit words

struct SLayer {
  int kind;          // 0: depthwise K taps + bias (fused MixConv groups, zero leading taps); 1: 1x1 + folded BN + ReLU;
                     // (the kernels' <VAR> form only) 2: a block's residual 1x1 + folded BN, linear, of the block input, kept
                     // aside; 3: kind 1 with that residual added at equal positions before the ReLU
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

// What a MixedNet with residual connections, a pooled head or spatial attention adds to SNet (read by the kernels' <VAR> form only)
struct SVar {
  int has_res;               // a third activation buffer holds the current block's residual
  int att, pool;             // spatial attention (non_stream mode only); 0 none, 1 average, 2 max pooling
  int tp;                    // frames the Dense or the pooling reads: tf - 3 with attention, else tf
  int64_t wa;                // attention kernel [4][2] (avg, max)
  const int* lt;             // [n_layers] calibrated tensor of each layer's output (kind 3: the 1x1 output, the ADD output next)
  int n_tensors;
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
  float* rec;                // calibration: per-workgroup [n_tensors][2] min / max partials (NULL: not recording)
  int n_tensors;
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

// Calibration (REC): every thread keeps the min / max of the values it computes for the current tensor; the block folds
// them in thread order into its running [n_tensors] min / max, written once per workgroup at the end.
__device__ inline void rec_fold(float lmin, float lmax, int t, float* red, float* rmin, float* rmax) {
  const int tid = threadIdx.x;
  red[tid] = lmin;
  red[kStreamThreads + tid] = lmax;
  __syncthreads();
  if (tid == 0) {
    float lo = rmin[t], hi = rmax[t];
    for (int i = 0; i < kStreamThreads; ++i) {
      lo = fminf(lo, red[i]);
      hi = fmaxf(hi, red[kStreamThreads + i]);
    }
    rmin[t] = lo;
    rmax[t] = hi;
  }
  __syncthreads();
}

// Calibration prologue / epilogue of a workgroup: the running min / max start empty; its partial row [n_tensors][2] at the end
__device__ inline void rec_init(const SCall& a, float* rmin, float* rmax) {
  for (int t = threadIdx.x; t < a.n_tensors; t += kStreamThreads) {
    rmin[t] = INFINITY;
    rmax[t] = -INFINITY;
  }
  __syncthreads();
}

__device__ inline void rec_flush(const SCall& a, const float* rmin, const float* rmax) {
  for (int t = threadIdx.x; t < a.n_tensors; t += kStreamThreads) {
    a.rec[((int64_t)blockIdx.x * a.n_tensors + t) * 2] = rmin[t];
    a.rec[((int64_t)blockIdx.x * a.n_tensors + t) * 2 + 1] = rmax[t];
  }
}

// A tile: outputs [c0, c1) of its segment, counted in positions of the segment (stream mode: the segment is the call and
// output n is position n, so the call ends at N = c1 in the tile that is `last`: that tile writes the rings)
struct STile {
  int64_t c0, c1, v_seg, out0;   // v_seg: the segment's first virtual frame; out0: global index of the tile's first output
  int n;
  bool last;
};

__device__ inline STile tile_of(const SCall& a, int tile) {
  const int sg = a.tile_seg[tile];
  STile t;
  t.c0 = a.tile_m0[tile] + a.seg_coff[sg];
  t.n = a.tile_n[tile];
  t.c1 = t.c0 + t.n;
  t.v_seg = a.seg_v0[sg];
  t.out0 = a.tile_out0[tile];
  t.last = a.use_state && t.out0 + t.n == a.n_out;
  return t;
}

// Float head: Dense over the last TF rows of the final map at every output position, sigmoid.  fin: row 0 of the final map
// as if it started at position 0 (pitch floats a row); positions before the stream start read the head ring.
template <bool REC>
__device__ inline void dense_head(const SCall& a, const STile& T, const float* fin, int pitch, const float* hring, int64_t wd_at,
                                  int64_t bd_at, int C, int TF, float& lmin, float& lmax) {
  for (int o = threadIdx.x; o < T.n; o += kStreamThreads) {
    const int64_t c = T.c0 + o;
    float acc = a.w[bd_at];
    for (int t = 0; t < TF; ++t) {
      const int64_t q = c - (TF - 1) + t;
      const float* wd = a.w + wd_at + (int64_t)t * C;
      const float* x = q >= 0 ? fin + q * pitch : hring + (TF - 1 + q) * C;
      for (int ch = 0; ch < C; ++ch) acc = fmaf(x[ch], wd[ch], acc);
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

// The head ring after the call: the final map at positions [N - (TF - 1), N), N = T.c1 of the last tile
template <class E>
__device__ inline void head_ring_store(E* ring_out, const STile& T, const E* fin, int pitch, const E* hring, int C, int TF) {
  for (int idx = threadIdx.x; idx < (TF - 1) * C; idx += kStreamThreads) {
    const int64_t q = T.c1 - (TF - 1) + idx / C;
    const int ch = idx % C;
    ring_out[idx] = q >= 0 ? fin[q * pitch + ch] : hring[(TF - 1 + q) * C + ch];
  }
}

// int8 form: what both int8 kernels get of the quantized parameters (layout: include/mww.h) and the call
struct SQ8 {
  const int8_t* w;       // int8 weights
  const int32_t* iv;     // per op: bias (input zero point folded), multiplier, shift [cout] each; the Dense's three; the tensor zero points
  const uint8_t* lut;    // [256]: logit q + 128 -> output uint8
  int64_t izp;           // offset of the tensor zero points in iv
  float in_scale;
  int in_zp;
  uint8_t* out;          // [n_out] uint8 outputs
  const int8_t* st_in;
  int8_t* st_out;
  int8_t* scratch;       // global form: per-workgroup tiles of SCall::scratch_per_wg bytes
  int use_lds;
};

// int8 head: Dense (int8 logit; words of the final map's rows of `pitch` bytes, bytes of the unpadded head ring), Logistic
// table, uint8 output, probability u8 / 255.  The Dense's weights are [TF][r4(C)] at wd_at, its three ints at id_at.
__device__ inline void dense_head_q8(const SCall& a, const SQ8& q, const STile& T, const int8_t* fin, int pitch, const int8_t* hring,
                                     int64_t wd_at, int64_t id_at, int zo, int C, int TF) {
  const int32_t bias = q.iv[id_at], mul = q.iv[id_at + 1], shf = q.iv[id_at + 2];
  const int pc = (C + 3) & ~3;
  for (int o = threadIdx.x; o < T.n; o += kStreamThreads) {
    const int64_t c = T.c0 + o;
    int acc = bias;
    for (int t = 0; t < TF; ++t) {
      const int64_t p = c - (TF - 1) + t;
      const int8_t* wd = q.w + wd_at + (int64_t)t * pc;
      if (p >= 0) {
        const int* x = reinterpret_cast<const int*>(fin + p * pitch);
        const int* w = reinterpret_cast<const int*>(wd);
        for (int r = 0; r < pc / 4; ++r) acc = mww_sdot4(x[r], w[r], acc);
      } else {
        const int8_t* x = hring + (TF - 1 + p) * C;
        for (int ch = 0; ch < C; ++ch) acc += (int)x[ch] * (int)wd[ch];
      }
    }
    const int lq = q8_requant(acc, mul, shf, zo, -128);
    const uint8_t u = q.lut[lq + 128];
    const int64_t g = T.out0 + o;
    q.out[g] = u;
    a.logit[g] = (float)lq;
    a.prob[g] = (float)u * kInv255;
  }
}

// What the shared call preparation needs of a model, filled by both planners
struct SGeom {
  int stride = 1;         // frames per output
  int frames = 0;         // the non-stream window
  int mode = 0;           // MWW_STREAM_MODE_*
  int reach = 0;          // positions of input halo in front of a tile: a tile's buffers hold tile_outputs + reach rows
  int j0 = 0;             // non-stream: position of a track's first window
  int tile_outputs = kTileOutputs;
};

// The model part of a stream.  The planner fills the sizes; the virtual functions are all the front ever asks of it.
struct SModel {
  SGeom g;
  int64_t n_weights = 0;        // Keras-order floats
  int64_t n_dev_w = 0;          // folded device weights
  int64_t n_state = 0;          // ring values (floats; the int8 state has one byte for each)
  int64_t scratch_per_wg = 0;   // floats of one workgroup's tile (float kernel)
  int n_tensors = 0;            // calibrated tensors: the input, every op's output, the logit
  bool int8 = true;             // takes int8 parameters (a conv/BN graph: only from mww_stream_create_convnet_q8)
  std::string int8_refusal;     // int8 = false: what the int8 entry points answer (empty: the conv/BN graph's message)
  int64_t q8_nw = 0, q8_ni = 0, q8_izp = 0;   // int8 weights / int32 values expected; offset of the zero points
  int64_t q8_tile_bytes = 0;                  // one workgroup's int8 tile
  std::vector<std::pair<int64_t, int>> q8_requant;   // per op and the Dense: (offset of its bias / multiplier / shift, cout)
  std::vector<int64_t> q8_add;                       // per int8 ADD: offset of its M1, sh1, M2, sh2, Mo, sho
  virtual ~SModel() {}                                // frees the device tables
  virtual int upload() = 0;                           // device tables of the plan (the device is current)
  virtual int64_t fold_weights(const float* h, float* w) const = 0;   // Keras order -> device layout; floats consumed
  virtual void launch(const SStores& S, const SCall& a, int grid, hipStream_t hs) const = 0;   // a.rec: the <REC> form
  virtual void q8_state0(const int32_t* zp, int8_t* st0) const = 0;   // rings at reset: each tensor's zero point
  virtual const void* q8_kernel() const = 0;
  virtual void launch_q8(const SStores& S, const SCall& a, const SQ8& q, int grid, size_t lds, hipStream_t hs) const = 0;
};

}  // namespace mww_stream_impl

struct mww_stream {
  mww_ctx* ctx = nullptr;
  int device = 0;
  hipStream_t stream = nullptr;
  int n_cu = 256;
  mww_stream_impl::SModel* model = nullptr;
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
  int grid = 0;            // workgroups of the last launch
  std::vector<char> htab;   // host copy of the last call's tables
  float* rec = nullptr;     // calibration partials
  int64_t cap_rec = 0;
  // the entry points on the probabilities held (stream_post.hip.h): no two run at once, so they share a call's tables and
  // its transfer tables / candidates
  char* post_tab = nullptr;
  char* post_scr = nullptr;
  int64_t cap_post_tab = 0, cap_post_scr = 0;
  // detections (stream_detect.hip.h): the events; live together with the tables above inside mww_stream_mine, as is mine_buf
  mww_detection* det_out = nullptr;
  int64_t cap_det_out = 0;
  // mining (tu_stream_mine.hip): the tracks' windows, the radix histograms, the per-workgroup counts, the kept clips and events
  char* mine_buf = nullptr;
  int64_t cap_mine_buf = 0;
  // int8 form (mww_stream_set_quantized): runs replace the float kernel with the int8 one
  bool q8 = false;
  int8_t* q8_w = nullptr;
  int32_t* q8_i = nullptr;
  uint8_t* q8_lut = nullptr;
  std::vector<int8_t> q8_state0;       // rings at reset: each ring filled with its tensor's zero point
  int8_t* q8_st[2] = {nullptr, nullptr};
  int q8_cur = 0;
  float q8_in_scale = 1.f;
  int q8_in_zp = 0;
  uint8_t* q8_out = nullptr;
  int64_t cap_q8_out = 0;
  int8_t* q8_scratch = nullptr;
  int64_t cap_q8_scratch = 0;
};

namespace mww_stream_impl {

// tu_stream.hip: a stream around a planned model (takes the model over, also on failure)
int stream_create(mww_ctx* ctx, SModel* m, int rc_plan, mww_stream** out);

#define SCHK(expr)                                                                                      \
  do {                                                                                                  \
    hipError_t e_ = (expr);                                                                             \
    if (e_ != hipSuccess) return mww::set_error(MWW_ERR_HIP, (std::string(#expr) + ": " + hipGetErrorString(e_)).c_str()); \
  } while (0)

// tu_stream_calibrate.hip: the device half of mww_stream_calibrate.  s->rec holds the <REC> launch's partial rows
// [2 x CU][n_tensors][2], then the input partials [2 x CU][2], then the folded ranges [n_tensors][2].
struct SCalBuf {
  float *rec, *in_part, *ranges;
};
int calibrate_buffers(mww_stream* s, SCalBuf* b);   // grows s->rec (the device is current)
// queues the input-range launch over the n_frames virtual frames of a prepared call; *n_in: the partials it writes
int calibrate_input(mww_stream* s, const SStores& S, const SCall& a, const SCalBuf& b, int64_t n_frames, int* n_in);
// folds the input partials and the s->grid partial rows of the launch just made on the device, reads n_tensors * 8 bytes back
int calibrate_fold(mww_stream* s, const SCalBuf& b, int n_in, float* ranges);

inline int unsupported(const std::string& m) { return mww::set_error(MWW_ERR_UNSUPPORTED, m.c_str()); }

template <class T>
inline int grow(T** p, int64_t* cap, int64_t n) {
  if (n <= *cap) return MWW_OK;
  if (*p) SCHK(hipFree(*p));
  *p = nullptr;
  *cap = 0;
  SCHK(hipMalloc((void**)p, (size_t)n * sizeof(T) + 64));
  *cap = n;
  return MWW_OK;
}

// device copy of a plan table (+ 64 bytes, as every buffer here)
template <class T>
inline int upload_table(T** dev, const std::vector<T>& host) {
  SCHK(hipMalloc((void**)dev, host.size() * sizeof(T) + 64));
  if (!host.empty()) SCHK(hipMemcpy(*dev, host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice));
  return MWW_OK;
}

// MixedNet: conv1, per block and repeat a fused MixConv depthwise layer (when max(ks) > 1) and a 1x1 layer, the Dense
struct MixedNet : SModel {
  mww_stream_desc d{};
  int residual[MWW_MAX_BLOCKS] = {};   // mww_stream_create_mixednet: per block; spatial attention; pooling (0 / 1 / 2)
  int att = 0, pool = 0;
  bool q8_variant = false;             // mww_stream_create_mixednet_q8: a residual / pooled plan takes int8 parameters
  SVar var{};
  bool variant() const { return var.has_res || var.att || var.pool; }   // runs the kernels' <VAR> form
  SNet net{};
  std::vector<SLayer> layers;   // host copy of net.L
  SLayer* d_layers = nullptr;
  std::vector<int> lt;          // host copy of var.lt
  int* d_lt = nullptr;
  // int8 layout (tu_stream_q8.hip): weight / int offsets of conv1, the layers and the Dense; pitches
  struct Q8 {
    const int64_t* lw;     // [n_layers] offset of each layer's weights
    const int64_t* li;     // [n_layers] offset of each layer's ints
    int64_t w1, wd, i1, id;
    int kp1;               // conv1 reduction length k1 * 40
    int cp;                // activation row pitch: cmax rounded up to 4
  } q{};
  std::vector<int64_t> q8_off;   // [2 * n_layers]: weight offsets, then int offsets
  int64_t* d_q8_off = nullptr;
  int plan();      // from d
  void plan_q8();
  ~MixedNet() override {
    if (d_layers) (void)hipFree(d_layers);
    if (d_q8_off) (void)hipFree(d_q8_off);
    if (d_lt) (void)hipFree(d_lt);
  }
  int upload() override;
  int64_t fold_weights(const float* h, float* w) const override;
  void launch(const SStores& S, const SCall& a, int grid, hipStream_t hs) const override;
  void q8_state0(const int32_t* zp, int8_t* st0) const override;
  const void* q8_kernel() const override;
  void launch_q8(const SStores& S, const SCall& a, const SQ8& q, int grid, size_t lds, hipStream_t hs) const override;
};

// tu_stream_q8.hip: the call and the layout, one kernel argument
struct SQ8Net : SQ8, MixedNet::Q8 {};

// topology + weight / state layout, reach of every layer and the call geometry from the description
inline int MixedNet::plan() {
  layers.assign((size_t)2 * MWW_MAX_BLOCKS * MWW_STREAM_MAX_REPEAT + MWW_MAX_BLOCKS, SLayer{});
  if (d.mode != MWW_STREAM_MODE_STREAM && d.mode != MWW_STREAM_MODE_NON_STREAM) return unsupported("mode must be stream or non_stream");
  if (d.conv1_filters <= 0 || d.conv1_kernel <= 0 || d.stride <= 0)
    return unsupported("streaming needs a first convolution (first_conv_filters > 0, kernel and stride > 0)");
  if (d.n_blocks <= 0 || d.n_blocks > MWW_MAX_BLOCKS) return unsupported("n_blocks must be 1..8");
  if (d.t_final <= 0) return unsupported("t_final must be positive");
  if (pool < 0 || pool > 2 || att < 0 || att > 1) return unsupported("pool must be 0 (none), 1 (average) or 2 (max), spatial_attention 0 or 1");
  if (att && q8_variant)
    return unsupported("mww_stream_create_mixednet_q8 does not cover spatial_attention: the int8 model is a stream-mode model, stream-mode "
                       "attention has no pinned reading, and TFLite's int8 MUL / Logistic gate is not restated");
  if (att && d.t_final < 4) return unsupported("spatial attention (kernel 4) needs t_final >= 4, not " + std::to_string(d.t_final));
  if (att && d.mode != MWW_STREAM_MODE_NON_STREAM)
    return unsupported("spatial attention runs in non_stream mode only: the reference's streaming clone gates the ring frames with the "
                       "current attention value, which is not the non-streaming computation, and nothing pins that reading");
  if (d.t_final == 1) pool = 0;   // mixednet.py:362: the head options need more than one frame
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
    if (d.repeat[b] <= 0 || d.repeat[b] > MWW_STREAM_MAX_REPEAT) return unsupported("block " + std::to_string(b) + ": repeat must be 1..8");
    if (f <= 0 || f > 1024) return unsupported("block " + std::to_string(b) + ": pointwise filters must be 1..1024");
    int K = 0;
    for (int g = 0; g < nk; ++g) {
      if (d.kernels[b][g] <= 0) return unsupported("block " + std::to_string(b) + ": kernel sizes must be positive");
      if (g && d.kernels[b][g] < d.kernels[b][g - 1]) return unsupported("mixconv kernel sizes must be ascending (alignment uses the last one)");
      K = d.kernels[b][g] > K ? d.kernels[b][g] : K;
    }
    if (residual[b] != 0 && residual[b] != 1) return unsupported("block " + std::to_string(b) + ": residual must be 0 or 1");
    if (residual[b]) {   // 1x1 + BN of the block input, no ring: every repeat's 1x1 layer adds it
      SLayer& Rl = layers[nl++];
      Rl.kind = 2; Rl.cin = c; Rl.cout = f; Rl.k = 1;
      Rl.w = dw; dw += (int64_t)c * f;
      Rl.b = dw; dw += f;
      kw += (int64_t)c * f + 4 * f;
      var.has_res = 1;
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
      P.kind = residual[b] ? 3 : 1; P.cin = c; P.cout = f; P.k = 1;
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
  var.att = att;
  var.pool = pool;
  var.tp = net.tf - 3 * att;
  const int td = pool ? 1 : var.tp;   // frames the Dense reads
  if (att) {
    var.wa = dw; dw += 8;
    kw += 8;
  }
  net.wd = dw; dw += (int64_t)td * c;
  net.bd = dw; dw += 1;
  kw += (int64_t)td * c + 1;
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
  if (d.mode == MWW_STREAM_MODE_NON_STREAM) {
    if (d.frames < net.k1) return unsupported("non_stream mode needs frames >= the first convolution's kernel");
    const int n1 = (d.frames - net.k1) / net.s + 1;
    if (n1 - sum_r != net.tf)
      return unsupported("t_final " + std::to_string(net.tf) + " does not match a " + std::to_string(d.frames) + "-frame window (" +
                         std::to_string(n1 - sum_r) + " final frames)");
    g.j0 = n1 - 1;
  }
  g.stride = net.s;
  g.frames = d.frames;
  g.mode = d.mode;
  g.reach = net.reach1;
  n_weights = kw;
  n_dev_w = dw;
  n_state = st;
  // calibrated tensors: input, conv1, every layer's output (a residual block's 1x1 counts twice: before and after the add), logit
  lt.assign((size_t)nl, 0);
  int nt = 2;
  for (int l = 0; l < nl; ++l) {
    lt[(size_t)l] = nt;
    nt += layers[l].kind == 3 ? 2 : 1;
  }
  n_tensors = nt + 1;
  var.n_tensors = n_tensors;
  // a tile: the gathered input rows and two activation buffers
  const int64_t rows = g.tile_outputs + g.reach, g_rows = ((rows - 1) * net.s + net.k1) * MWW_FEATURE_BINS;
  if (variant()) {   // + the residual buffer, + per position the channel mean, the channel max and the gate
    scratch_per_wg = (g_rows + (2 + var.has_res) * rows * net.cmax + (att ? 3 * rows : 0) + 255) & ~(int64_t)255;
    if (q8_variant) {   // residuals / pooling: the int8 kernel's <VAR> form, one more int8 buffer for r
      q8_tile_bytes = g_rows + (2 + var.has_res) * rows * r4(net.cmax);
      plan_q8();
      return MWW_OK;
    }
    int8 = false;
    int8_refusal = "the int8 streaming model does not cover MixedNet with residual_connection, pooled or spatial_attention "
                   "on a stream of mww_stream_create_mixednet: this stream runs the float model only "
                   "(mww_stream_create_mixednet_q8 creates one that takes int8 parameters for residual_connection and pooled)";
    return MWW_OK;
  }
  scratch_per_wg = (g_rows + 2 * rows * net.cmax + 255) & ~(int64_t)255;
  q8_tile_bytes = g_rows + 2 * rows * r4(net.cmax);
  plan_q8();
  return MWW_OK;
}

// Per-call tables of a track list (tracks, virtual frame offsets, segments, tiles) uploaded to s->tables, the output
// buffers grown, and the kernel arguments filled.  Returns the number of outputs (0: nothing to launch) or an error < 0.
inline int64_t prepare_call(mww_stream* s, const mww_window* trk, int64_t n_trk, int64_t* out_off, int64_t n_host_frames,
                            SStores& S, SCall& a, int* grid_out) {
  if (n_trk < 0 || n_trk > INT32_MAX || (n_trk && !trk) || !out_off) return mww::set_error(MWW_ERR_INVALID, "bad track list");
  S = SStores{};
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
  const SGeom& g = s->model->g;
  const bool stream_mode = g.mode == MWW_STREAM_MODE_STREAM;
  const int T = g.frames;
  // per track: frames fed and outputs (predict_spectrogram: chunks of s, trailing L mod s frames never fed; non-stream:
  // windows ending at T, T + s, ... <= L)
  std::vector<int64_t> v0((size_t)n_trk + 1, 0);
  out_off[0] = 0;
  for (int64_t t = 0; t < n_trk; ++t) {
    const mww_window& w = trk[t];
    if (w.pad_rows < 0 || w.copy_rows < 0) return mww::set_error(MWW_ERR_INVALID, "negative track rows");
    if (w.store >= 0) {
      if (w.store >= MWW_MAX_STORES || !stores[w.store]) return mww::set_error(MWW_ERR_INVALID, "track refers to a store that was not uploaded");
      if (w.src_elem < 0 || w.src_elem + (int64_t)w.copy_rows * MWW_FEATURE_BINS > el[w.store])
        return mww::set_error(MWW_ERR_INVALID, "track reads past the end of its store");
    } else if (w.src_elem < 0 || w.src_elem + (int64_t)w.copy_rows * MWW_FEATURE_BINS > n_host_frames * MWW_FEATURE_BINS) {
      return mww::set_error(MWW_ERR_INVALID, "track reads past the host frames");
    }
    const int64_t L = (int64_t)w.pad_rows + w.copy_rows;
    int64_t n_o;
    if (stream_mode) {
      n_o = L / g.stride;
      v0[t + 1] = v0[t] + n_o * g.stride;
    } else {
      n_o = L >= T ? (L - T) / g.stride + 1 : 0;
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
  const int tile_outputs = g.tile_outputs;
  auto add_tiles = [&](int sg, int64_t n, int64_t out0) {
    for (int64_t m = 0; m < n; m += tile_outputs) {
      tile_seg.push_back(sg);
      tile_m0.push_back(m);
      tile_n.push_back((int)(n - m < tile_outputs ? n - m : tile_outputs));
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
      seg_coff.push_back(g.j0);
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
  std::vector<char>& tab = s->htab;   // kept until the next call: the upload below is asynchronous
  tab.assign((size_t)bytes, 0);
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
  *grid_out = s->grid = n_tiles < 2 * s->n_cu ? n_tiles : 2 * s->n_cu;
  SCHK(hipMemcpyAsync(s->tables, tab.data(), (size_t)bytes, hipMemcpyHostToDevice, s->stream));
  a = SCall{};
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
  a.buf_rows = tile_outputs + g.reach;
  a.prob = s->prob;
  a.logit = s->logit;
  return n_out;
}

}  // namespace mww_stream_impl
