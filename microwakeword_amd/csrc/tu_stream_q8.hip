// int8 streaming inference (mww_stream_set_quantized, include/mww.h): the quantized streaming model the reference converts
// with representative-dataset calibration (utils.py:288-360, --test_tflite_streaming_quantized), restated after TFLite's
// int8 kernels (ConvPerChannel / DepthwiseConvPerChannel / FullyConnected / Logistic reference semantics).
//
// The same whole-sequence form, tiles and ring layout as the float kernel (stream_common.hip.h, tu_stream.hip): a tile of
// up to 256 outputs recomputes its halo; positions before the stream start read the rings, now int8 values of each layer's
// input tensor with that tensor's parameters; the tile that ends a stream-mode call writes the next rings.  Activations
// are int8 [rows][cp] with the row pitch cp = cmax rounded up to 4, so the 1x1 contractions, conv1 and the Dense run as
// v_dot4_i32_i8 (int8_ops.hip.h) over 32-bit words; the input zero point is folded into the bias on the host (exact in
// integers).  The depthwise taps are int32 MACs.  A tile's buffers sit in LDS when they fit (the default topologies:
// 69-80 KB), else in a per-workgroup global scratch.  Every sum runs in a fixed order and every op is an exact integer
// function of its inputs: outputs and rings are bit-identical from run to run and equal to the NumPy restatement.
#include <hip/hip_runtime.h>

#include "int8_ops.hip.h"
#include "stream_common.hip.h"

using namespace mww_stream_impl;

namespace mww {
int stream_graph_no_int8(const mww_stream* s);   // tu_stream_graph.hip: the refusal of a plain conv/BN graph stream
bool stream_graph_int8(const mww_stream* s);     // created by mww_stream_create_convnet_q8: tu_stream_graph_q8.hip serves it
int64_t stream_graph_q8_sizes(const mww_stream* s, int64_t* n_ints);
int stream_graph_set_quantized(mww_stream* s, const int8_t* weights, int64_t n_weights, const int32_t* ints, int64_t n_ints,
                               float input_scale, const uint8_t* lut);
}

namespace {

constexpr int64_t kMaxLds = 160 * 1024;   // LDS of a gfx950 CU
constexpr float kInv255 = (float)(1.0 / 255.0);   // inference.py:170 1 / 255 as float32

__global__ void __launch_bounds__(kStreamThreads) stream_q8_kernel(SNet net, SStores S, SCall a, SQ8 q) {
  HIP_DYNAMIC_SHARED(int, q8_lds)
  const int tid = threadIdx.x;
  const int64_t g_rows = (a.buf_rows - 1) * net.s + net.k1;
  int8_t* G = q.use_lds ? reinterpret_cast<int8_t*>(q8_lds) : q.scratch + (int64_t)blockIdx.x * a.scratch_per_wg;
  int8_t* B0 = G + g_rows * MWW_FEATURE_BINS;   // 40 bytes a row: stays 4-byte aligned
  int8_t* B1 = B0 + a.buf_rows * q.cp;
  const int cp = q.cp;
  const int r1 = a.use_state ? net.r1 : 0;
  const int32_t* zps = q.iv + q.izp;
  for (int tile = blockIdx.x; tile < a.n_tiles; tile += gridDim.x) {
    const int sg = a.tile_seg[tile];
    const int64_t c0 = a.tile_m0[tile] + a.seg_coff[sg];
    const int64_t c1 = c0 + a.tile_n[tile];
    const int64_t v_seg = a.seg_v0[sg];
    const bool last = a.use_state && a.tile_out0[tile] + a.tile_n[tile] == a.n_out;
    const int64_t N = c1;
    // ---- gather + quantize the padded input rows, four bins to a word
    int64_t lo = c0 - net.reach1;
    if (lo < 0) lo = 0;
    const int64_t p0 = lo * net.s, p1 = (c1 - 1) * net.s + net.k1;
    constexpr int kWords = MWW_FEATURE_BINS / 4;
    for (int64_t idx = tid; idx < (p1 - p0) * kWords; idx += kStreamThreads) {
      const int64_t p = p0 + idx / kWords;
      const int b4 = (int)(idx % kWords) * 4;
      const int64_t v = p - r1;
      uint32_t word = 0;
      for (int k = 0; k < 4; ++k) {
        const int8_t x = v < 0 ? q.st_in[net.ring1 + (r1 + v) * MWW_FEATURE_BINS + b4 + k]
                               : quantize_input(frame_value(S, a, v_seg + v, b4 + k), q.in_scale, q.in_zp);
        word |= (uint32_t)(uint8_t)x << (8 * k);
        if (last && p >= N * net.s && p < N * net.s + r1) q.st_out[net.ring1 + (p - N * net.s) * MWW_FEATURE_BINS + b4 + k] = x;
      }
      reinterpret_cast<uint32_t*>(G)[idx] = word;
    }
    __syncthreads();
    // ---- conv1 (valid, stride s, no bias) + ReLU: k1 * 40 / 4 dot4 per output
    const int64_t n1 = c1 - lo;
    {
      const int32_t* bias = q.iv + q.i1;
      const int32_t *mul = bias + net.c1, *shf = mul + net.c1;
      const int zo = zps[1], amin = zo > -128 ? zo : -128;
      for (int64_t idx = tid; idx < n1 * net.c1; idx += kStreamThreads) {
        const int64_t i = idx / net.c1;
        const int co = (int)(idx % net.c1);
        const int* g = reinterpret_cast<const int*>(G + i * net.s * MWW_FEATURE_BINS);
        const int* w = reinterpret_cast<const int*>(q.w + q.w1 + (int64_t)co * q.kp1);
        int acc = bias[co];
        for (int r = 0; r < q.kp1 / 4; ++r) acc = mww_sdot4(g[r], w[r], acc);
        B0[i * cp + co] = (int8_t)q8_requant(acc, mul[co], shf[co], zo, amin);
      }
    }
    __syncthreads();
    int8_t* in = B0;
    int8_t* out = B1;
    int64_t in_lo = lo;
    for (int l = 0; l < net.n_layers; ++l) {
      const SLayer& L = net.L[l];
      int64_t o_lo = c0 - L.reach;
      if (o_lo < 0) o_lo = 0;
      const int64_t no = c1 - o_lo;
      const int8_t* wl = q.w + q.lw[l];
      const int32_t* bias = q.iv + q.li[l];
      const int32_t *mul = bias + L.cout, *shf = mul + L.cout;
      const int zo = zps[2 + l];
      if (L.kind == 0) {
        const int C = L.cin, K = L.k, R = K - 1;
        const int8_t* ring = q.st_in + L.ring;
        for (int64_t idx = tid; idx < no * C; idx += kStreamThreads) {
          const int64_t i = o_lo + idx / C;
          const int c = (int)(idx % C);
          int acc = bias[c];
          for (int j = 0; j < K; ++j) {
            const int64_t qq = i - R + j;
            const int x = qq >= 0 ? in[(qq - in_lo) * cp + c] : ring[(R + qq) * C + c];
            acc += (int)wl[(int64_t)j * C + c] * x;
          }
          out[(i - o_lo) * cp + c] = (int8_t)q8_requant(acc, mul[c], shf[c], zo, -128);
        }
        if (last) {   // this layer's ring after the call: its input at positions [N - R, N)
          for (int idx = tid; idx < R * C; idx += kStreamThreads) {
            const int64_t qq = N - R + idx / C;
            const int c = idx % C;
            q.st_out[L.ring + idx] = qq >= 0 ? in[(qq - in_lo) * cp + c] : ring[(R + qq) * C + c];
          }
        }
      } else {
        const int Ci = L.cin, Co = L.cout, nw = (Ci + 3) / 4;
        const int amin = zo > -128 ? zo : -128;
        for (int64_t idx = tid; idx < no * Co; idx += kStreamThreads) {
          const int64_t i = o_lo + idx / Co;
          const int co = (int)(idx % Co);
          const int* x = reinterpret_cast<const int*>(in + (i - in_lo) * cp);
          const int* w = reinterpret_cast<const int*>(wl + (int64_t)co * nw * 4);
          int acc = bias[co];
          for (int r = 0; r < nw; ++r) acc = mww_sdot4(x[r], w[r], acc);
          out[(i - o_lo) * cp + co] = (int8_t)q8_requant(acc, mul[co], shf[co], zo, amin);
        }
      }
      __syncthreads();
      int8_t* t = in;
      in = out;
      out = t;
      in_lo = o_lo;
    }
    // ---- head: Dense over the last T_f frames (int8 logit), Logistic table, uint8 output, probability u8 / 255
    const int C = net.c_last, TF = net.tf;
    const int8_t* hring = q.st_in + net.ring_head;
    {
      const int32_t bias = q.iv[q.id], mul = q.iv[q.id + 1], shf = q.iv[q.id + 2];
      const int zo = zps[2 + net.n_layers];
      for (int o = tid; o < a.tile_n[tile]; o += kStreamThreads) {
        const int64_t c = c0 + o;
        int acc = bias;
        for (int t = 0; t < TF; ++t) {
          const int64_t qq = c - (TF - 1) + t;
          const int8_t* wd = q.w + q.wd + (int64_t)t * q.cpd;
          if (qq >= 0) {
            const int* x = reinterpret_cast<const int*>(in + (qq - in_lo) * cp);
            const int* w = reinterpret_cast<const int*>(wd);
            for (int r = 0; r < q.cpd / 4; ++r) acc = mww_sdot4(x[r], w[r], acc);
          } else {
            const int8_t* x = hring + (TF - 1 + qq) * C;
            for (int ch = 0; ch < C; ++ch) acc += (int)x[ch] * (int)wd[ch];
          }
        }
        const int lq = q8_requant(acc, mul, shf, zo, -128);
        const uint8_t u = q.lut[lq + 128];
        const int64_t g = a.tile_out0[tile] + o;
        q.out[g] = u;
        a.logit[g] = (float)lq;
        a.prob[g] = (float)u * kInv255;
      }
    }
    if (last) {
      for (int idx = tid; idx < (TF - 1) * C; idx += kStreamThreads) {
        const int64_t qq = N - (TF - 1) + idx / C;
        const int ch = idx % C;
        q.st_out[net.ring_head + idx] = qq >= 0 ? in[(qq - in_lo) * cp + ch] : hring[(TF - 1 + qq) * C + ch];
      }
    }
    __syncthreads();   // the next tile reuses the buffers
  }
}

int64_t r4(int64_t n) { return (n + 3) & ~(int64_t)3; }

// offsets of every op's int8 weights and int32 values (include/mww.h, mww_stream_set_quantized); each op's weights
// start on a 4-byte boundary
void q8_layout(const mww_stream* s, std::vector<int64_t>* lw, std::vector<int64_t>* li, int64_t* w1, int64_t* wd, int64_t* i1,
               int64_t* id, int64_t* izp, int64_t* nw, int64_t* ni) {
  const SNet& net = s->net;
  int64_t w = 0, i = 0;
  *w1 = w;
  w = r4(w + (int64_t)net.c1 * net.k1 * MWW_FEATURE_BINS);
  *i1 = i;
  i += 3 * (int64_t)net.c1;
  for (const SLayer& L : s->layers) {
    if (lw) lw->push_back(w);
    if (li) li->push_back(i);
    w = r4(w + (L.kind == 0 ? (int64_t)L.k * L.cin : (int64_t)L.cout * r4(L.cin)));
    i += 3 * (int64_t)L.cout;
  }
  *wd = w;
  w = r4(w + (int64_t)net.tf * r4(net.c_last));
  *id = i;
  i += 3;
  *izp = i;
  i += net.n_layers + 3;
  *nw = w;
  *ni = i;
}

}  // namespace

namespace mww {

int stream_q8_reset(mww_stream* s) {
  SCHK(hipSetDevice(s->device));
  SCHK(hipMemcpyAsync(s->q8_st[s->q8_cur], s->q8_state0.data(), s->q8_state0.size(), hipMemcpyHostToDevice, s->stream));
  SCHK(hipStreamSynchronize(s->stream));
  return MWW_OK;
}

void stream_q8_free(mww_stream* s) {
  for (void* p : {(void*)s->q8_w, (void*)s->q8_i, (void*)s->q8_lut, (void*)s->q8_off, (void*)s->q8_st[0], (void*)s->q8_st[1],
                  (void*)s->q8_out, (void*)s->q8_scratch})
    if (p) (void)hipFree(p);
  s->q8_w = nullptr;
  s->q8_i = nullptr;
  s->q8_lut = nullptr;
  s->q8_off = nullptr;
  s->q8_st[0] = s->q8_st[1] = nullptr;
  s->q8_out = nullptr;
  s->q8_scratch = nullptr;
  s->cap_q8_out = s->cap_q8_scratch = 0;
  s->q8 = false;
}

int64_t stream_q8_launch(mww_stream* s, const SStores& S, SCall& a, int grid) {
  const SNet& net = s->net;
  SQ8 q{};
  q.w = s->q8_w;
  q.iv = s->q8_i;
  q.lut = s->q8_lut;
  q.lw = s->q8_off;
  q.li = s->q8_off + net.n_layers;
  q.w1 = s->q8_w1;
  q.wd = s->q8_wd;
  q.i1 = s->q8_i1;
  q.id = s->q8_id;
  q.izp = s->q8_izp;
  q.in_scale = s->q8_in_scale;
  q.in_zp = s->q8_in_zp;
  q.kp1 = net.k1 * MWW_FEATURE_BINS;
  q.cpd = (int)r4(net.c_last);
  q.cp = (int)r4(net.cmax);
  const int64_t n_out = a.n_out;
  int rc = grow(&s->q8_out, &s->cap_q8_out, n_out);
  if (rc) return rc;
  q.out = s->q8_out;
  q.st_in = s->q8_st[s->q8_cur];
  q.st_out = s->q8_st[s->q8_cur ^ 1];
  const int64_t bytes = ((a.buf_rows - 1) * net.s + net.k1) * MWW_FEATURE_BINS + 2 * a.buf_rows * q.cp;
  q.use_lds = bytes <= kMaxLds;
  size_t lds = 0;
  if (q.use_lds) {
    lds = (size_t)bytes;
    if (lds > 64 * 1024) SCHK(hipFuncSetAttribute((const void*)stream_q8_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  } else {
    const int64_t per_wg = (bytes + 255) & ~(int64_t)255;
    if ((rc = grow(&s->q8_scratch, &s->cap_q8_scratch, per_wg * grid))) return rc;
    q.scratch = s->q8_scratch;
    a.scratch_per_wg = per_wg;
  }
  hipLaunchKernelGGL(stream_q8_kernel, dim3(grid), dim3(kStreamThreads), lds, s->stream, net, S, a, q);
  SCHK(hipGetLastError());
  SCHK(hipStreamSynchronize(s->stream));
  if (s->d.mode == MWW_STREAM_MODE_STREAM) s->q8_cur ^= 1;
  return n_out;
}

}  // namespace mww

extern "C" {

int64_t mww_stream_q8_sizes(const mww_stream* s, int64_t* n_ints) {
  if (!s) return mww::set_error(MWW_ERR_INVALID, "null stream");
  if (s->graph) return mww::stream_graph_int8(s) ? mww::stream_graph_q8_sizes(s, n_ints) : mww::stream_graph_no_int8(s);
  int64_t w1, wd, i1, id, izp, nw, ni;
  q8_layout(s, nullptr, nullptr, &w1, &wd, &i1, &id, &izp, &nw, &ni);
  if (n_ints) *n_ints = ni;
  return nw;
}

int mww_stream_set_quantized(mww_stream* s, const int8_t* weights, int64_t n_weights, const int32_t* ints, int64_t n_ints,
                             float input_scale, const uint8_t* lut) {
  if (!s || !weights || !ints || !lut) return mww::set_error(MWW_ERR_INVALID, "null argument");
  if (s->graph)
    return mww::stream_graph_int8(s) ? mww::stream_graph_set_quantized(s, weights, n_weights, ints, n_ints, input_scale, lut)
                                     : mww::stream_graph_no_int8(s);
  std::vector<int64_t> lw, li;
  int64_t w1, wd, i1, id, izp, nw, ni;
  q8_layout(s, &lw, &li, &w1, &wd, &i1, &id, &izp, &nw, &ni);
  if (n_weights != nw || n_ints != ni)
    return mww::set_error(MWW_ERR_INVALID, ("expected " + std::to_string(nw) + " int8 weights and " + std::to_string(ni) + " int32 values").c_str());
  if (!(input_scale > 0.f) || !std::isfinite(input_scale)) return mww::set_error(MWW_ERR_INVALID, "input scale must be positive");
  const SNet& net = s->net;
  for (int64_t t = 0; t < net.n_layers + 3; ++t)
    if (ints[izp + t] < -128 || ints[izp + t] > 127) return mww::set_error(MWW_ERR_INVALID, "zero points must lie in [-128, 127]");
  // q8_requant shifts by at most 31 bits either way: QuantizeMultiplier emits shifts in [-31, 30] and multipliers >= 0,
  // anything else (from a hand-made .npz) would reach x >> e with e >= 32 on the device
  auto bad_requant = [&](int64_t at, int64_t cout) {
    for (int64_t c = 0; c < cout; ++c)
      if (ints[at + cout + c] < 0 || ints[at + 2 * cout + c] < -31 || ints[at + 2 * cout + c] > 30) return true;
    return false;
  };
  bool bad = bad_requant(i1, net.c1) || bad_requant(id, 1);
  for (size_t l = 0; l < s->layers.size() && !bad; ++l) bad = bad_requant(li[l], s->layers[l].cout);
  if (bad) return mww::set_error(MWW_ERR_INVALID, "requantization multipliers must be >= 0 and shifts lie in [-31, 30]");
  mww::stream_q8_free(s);
  // rings at reset: real zero, i.e. each ring's tensor zero point (conv1: the input, MixConv: its input, head: the last map)
  std::vector<int8_t> st0((size_t)s->n_state + 4, 0);
  for (int64_t k = 0; k < (int64_t)net.r1 * MWW_FEATURE_BINS; ++k) st0[net.ring1 + k] = (int8_t)ints[izp];
  for (size_t l = 0; l < s->layers.size(); ++l) {
    const SLayer& L = s->layers[l];
    if (L.kind == 0)
      for (int64_t k = 0; k < (int64_t)(L.k - 1) * L.cin; ++k) st0[L.ring + k] = (int8_t)ints[izp + 1 + l];
  }
  for (int64_t k = 0; k < (int64_t)(net.tf - 1) * net.c_last; ++k) st0[net.ring_head + k] = (int8_t)ints[izp + 1 + net.n_layers];
  std::vector<int64_t> off(lw);
  off.insert(off.end(), li.begin(), li.end());
  SCHK(hipSetDevice(s->device));
  SCHK(hipMalloc((void**)&s->q8_w, (size_t)nw + 64));
  SCHK(hipMalloc((void**)&s->q8_i, (size_t)ni * 4 + 64));
  SCHK(hipMalloc((void**)&s->q8_lut, 256 + 64));
  SCHK(hipMalloc((void**)&s->q8_off, off.size() * 8 + 64));
  for (int i = 0; i < 2; ++i) SCHK(hipMalloc((void**)&s->q8_st[i], st0.size()));
  SCHK(hipMemcpyAsync(s->q8_w, weights, (size_t)nw, hipMemcpyHostToDevice, s->stream));
  SCHK(hipMemcpyAsync(s->q8_i, ints, (size_t)ni * 4, hipMemcpyHostToDevice, s->stream));
  SCHK(hipMemcpyAsync(s->q8_lut, lut, 256, hipMemcpyHostToDevice, s->stream));
  if (!off.empty()) SCHK(hipMemcpyAsync(s->q8_off, off.data(), off.size() * 8, hipMemcpyHostToDevice, s->stream));
  SCHK(hipStreamSynchronize(s->stream));
  s->q8_state0 = st0;
  s->q8_in_scale = input_scale;
  s->q8_in_zp = ints[izp];
  s->q8_w1 = w1;
  s->q8_wd = wd;
  s->q8_i1 = i1;
  s->q8_id = id;
  s->q8_izp = izp;
  s->q8_cur = 0;
  s->q8 = true;
  return mww::stream_q8_reset(s);
}

int mww_stream_read_q8(mww_stream* s, uint8_t* out, int64_t n) {
  if (s && s->graph && !mww::stream_graph_int8(s)) return mww::stream_graph_no_int8(s);
  if (!s || !s->q8 || n < 0 || n > s->n_out || n > s->cap_q8_out || (n && !out)) return mww::set_error(MWW_ERR_INVALID, "more outputs requested than the last int8 run produced");
  if (!n) return MWW_OK;
  SCHK(hipSetDevice(s->device));
  SCHK(hipMemcpyAsync(out, s->q8_out, (size_t)n, hipMemcpyDeviceToHost, s->stream));
  SCHK(hipStreamSynchronize(s->stream));
  return MWW_OK;
}

int mww_stream_get_state_q8(mww_stream* s, int8_t* h, int64_t n) {
  if (s && s->graph && !mww::stream_graph_int8(s)) return mww::stream_graph_no_int8(s);
  if (!s || !s->q8 || !h || n != s->n_state) return mww::set_error(MWW_ERR_INVALID, "state size mismatch (or no int8 parameters)");
  SCHK(hipSetDevice(s->device));
  SCHK(hipMemcpyAsync(h, s->q8_st[s->q8_cur], (size_t)n, hipMemcpyDeviceToHost, s->stream));
  SCHK(hipStreamSynchronize(s->stream));
  return MWW_OK;
}

}  // extern "C"
