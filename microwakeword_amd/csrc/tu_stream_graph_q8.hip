// int8 streaming inference of a conv -> BN/SSN -> ReLU graph (mww_stream_create_convnet_q8, include/mww.h): the quantized
// streaming Inception model the reference converts with representative-dataset calibration (utils.py:288-360,
// --test_tflite_streaming_quantized), restated after TFLite's int8 kernels (ConvPerChannel / FullyConnected / Logistic
// reference semantics; CONCATENATION with one scale and zero point for all its inputs - microwakeword_amd/quantize_graph.py
// derives the parameters, INTEGRATION.md states the contract).
//
// The same whole-sequence form, tiles (256 outputs + every tensor's reach), segment tables, rings and double-buffered state
// as the float graph kernel (tu_stream_graph.hip).  Tensors are int8 rows of pitch r4(C); the liveness plan places them in
// bytes at 4-byte aligned offsets (plan_graph), in dynamic LDS when the tile fits 160 KB, else in a per-workgroup global
// scratch.  One thread computes one (position, output channel): taps, then sources, then 32-bit words of the source's slice
// as v_dot4_i32_i8 (int8_ops.hip.h).  The word path needs the slice to start on a word (src_c0 % 4 == 0); it may read up to
// three bytes past the slice inside the row, which meet zero weights (the weights of a source are padded to r4(cn)).  A slice
// that starts elsewhere, and every position before the stream start (the op's ring: [R][Cin] int8, sources concatenated,
// unpadded), takes a byte-MAC path.  The input zero point is folded into the bias on the host, exact in integers: a ring at
// reset holds zero points, so it contributes what the fold assumes.  Every sum runs in a fixed order and every op is an
// exact integer function of its inputs: no atomics, outputs and rings are bit-identical from run to run and equal to the
// NumPy restatement (tests/quant_graph_oracle.py).
#include <hip/hip_runtime.h>

#include "int8_ops.hip.h"
#include "stream_graph.hip.h"

using namespace mww_stream_impl;

namespace mww {
int stream_q8_reset(mww_stream* s);
void stream_q8_free(mww_stream* s);
}  // namespace mww

namespace {

constexpr int64_t kMaxLds = 160 * 1024;   // LDS of a gfx950 CU
constexpr float kInv255 = (float)(1.0 / 255.0);   // inference.py:170 1 / 255 as float32

struct GQ8 {
  const int8_t* w;       // int8 weights: per op [Co][k][source 0: r4(cn_0)] ... [source n-1], then the Dense [T_f][r4(C_last)]
  const int32_t* iv;     // per op bias (input zero point folded), multiplier, shift [Co] each; the Dense's three; the zero points
  const uint8_t* lut;    // [256]: logit q + 128 -> output uint8
  int64_t izp;           // offset of the n_ops + 2 tensor zero points in iv
  float in_scale;
  int in_zp;
  uint8_t* out;          // [n_out] uint8 outputs
  const int8_t* st_in;
  int8_t* st_out;
  int8_t* scratch;       // global form: per-workgroup tiles
  int64_t scratch_per_wg;
  int use_lds;
};

__global__ void __launch_bounds__(kStreamThreads) stream_graph_q8_kernel(GNet net, SStores S, SCall a, GQ8 q) {
  HIP_DYNAMIC_SHARED(int, gq8_lds)
  const int tid = threadIdx.x;
  int8_t* B = q.use_lds ? reinterpret_cast<int8_t*>(gq8_lds) : q.scratch + (int64_t)blockIdx.x * q.scratch_per_wg;
  const int32_t* zps = q.iv + q.izp;
  for (int tile = blockIdx.x; tile < a.n_tiles; tile += gridDim.x) {
    const int sg = a.tile_seg[tile];
    const int64_t c0 = a.tile_m0[tile] + a.seg_coff[sg];
    const int64_t c1 = c0 + a.tile_n[tile];
    const int64_t v_seg = a.seg_v0[sg];
    const bool last = a.use_state && a.tile_out0[tile] + a.tile_n[tile] == a.n_out;
    const int64_t N = c1;   // stream mode: the segment is the call, position n is frame n of the call
    // ---- gather + quantize the spectrogram rows [lo, c1) the tile reads, four bins to a word
    int64_t lo = c0 - net.in_reach;
    if (lo < 0) lo = 0;
    {
      constexpr int kWords = MWW_FEATURE_BINS / 4;
      uint32_t* G = reinterpret_cast<uint32_t*>(B + net.in_buf);
      for (int64_t idx = tid; idx < (c1 - lo) * kWords; idx += kStreamThreads) {
        const int64_t v = v_seg + lo + idx / kWords;
        const int b4 = (int)(idx % kWords) * 4;
        uint32_t word = 0;
        for (int k = 0; k < 4; ++k)
          word |= (uint32_t)(uint8_t)quantize_input(frame_value(S, a, v, b4 + k), q.in_scale, q.in_zp) << (8 * k);
        G[idx] = word;
      }
    }
    for (int o = 0; o < net.n_ops; ++o) {
      const GOp& L = net.ops[o];
      if (L.sync) __syncthreads();
      const int K = L.k, D = L.d, Ci = L.cin, Co = L.cout, R = L.R, ns = L.n_src;
      int64_t o_lo = c0 - L.reach;
      if (o_lo < 0) o_lo = 0;
      const int64_t no = c1 - o_lo;
      const int8_t* ring = q.st_in + L.ring;
      const int8_t* xs[MWW_MAX_OP_SOURCES];   // row 0 of each source's slice, as if the tensor started at position 0
      int kp = 0;                             // weights of one tap: every source's slice padded to a word
      for (int s = 0; s < ns; ++s) {
        int64_t s_lo = c0 - L.src_reach[s];
        if (s_lo < 0) s_lo = 0;
        xs[s] = B + L.src_buf[s] - s_lo * L.src_C[s] + L.src_c0[s];
        kp += (L.src_cn[s] + 3) & ~3;
      }
      int8_t* out = B + L.out_buf;
      const int po = (Co + 3) & ~3;
      const int32_t* bias = q.iv + L.b;
      const int32_t *mul = bias + Co, *shf = mul + Co;
      const int zo = zps[1 + o], amin = zo > -128 ? zo : -128;   // every op has a fused ReLU
      for (int64_t idx = tid; idx < no * Co; idx += kStreamThreads) {
        const int64_t i = o_lo + idx / Co;
        const int co = (int)(idx % Co);
        const int8_t* w = q.w + L.w + (int64_t)co * K * kp;
        int acc = bias[co];
        for (int j = 0; j < K; ++j) {
          const int64_t p = i - (int64_t)(K - 1 - j) * D;
          if (p >= 0) {
            for (int s = 0; s < ns; ++s) {
              const int8_t* x = xs[s] + p * L.src_C[s];
              const int cn = L.src_cn[s];
              if ((L.src_c0[s] & 3) == 0) {
                const int* xw = reinterpret_cast<const int*>(x);
                const int* ww = reinterpret_cast<const int*>(w);
                for (int r = 0; r < (cn + 3) / 4; ++r) acc = mww_sdot4(xw[r], ww[r], acc);
              } else {
                for (int ci = 0; ci < cn; ++ci) acc += (int)x[ci] * (int)w[ci];
              }
              w += (cn + 3) & ~3;
            }
          } else {
            const int8_t* x = ring + (R + p) * Ci;
            for (int s = 0; s < ns; ++s) {
              const int cn = L.src_cn[s];
              for (int ci = 0; ci < cn; ++ci) acc += (int)x[ci] * (int)w[ci];
              x += cn;
              w += (cn + 3) & ~3;
            }
          }
        }
        out[(i - o_lo) * po + co] = (int8_t)q8_requant(acc, mul[co], shf[co], zo, amin);
      }
      if (last && R > 0) {   // this op's ring after the call: its input at positions [N - R, N)
        for (int idx = tid; idx < R * Ci; idx += kStreamThreads) {
          const int64_t p = N - R + idx / Ci;
          int c = idx % Ci;
          int8_t v;
          if (p >= 0) {
            int s = 0;
            while (c >= L.src_cn[s]) c -= L.src_cn[s++];
            v = xs[s][p * L.src_C[s] + c];
          } else {
            v = ring[(R + p) * Ci + c];
          }
          q.st_out[L.ring + idx] = v;
        }
      }
    }
    __syncthreads();
    // ---- head: Dense over the last T_f rows of the final map (int8 logit), Logistic table, uint8 output, probability u8 / 255
    const int C = net.c_last, TF = net.tf, pc = (C + 3) & ~3;
    int64_t f_lo = c0 - (TF - 1);
    if (f_lo < 0) f_lo = 0;
    const int8_t* fin = B + net.last_buf - f_lo * pc;
    const int8_t* hring = q.st_in + net.ring_head;
    {
      const int32_t bias = q.iv[net.bd], mul = q.iv[net.bd + 1], shf = q.iv[net.bd + 2];
      const int zo = zps[net.n_ops + 1];
      for (int o = tid; o < a.tile_n[tile]; o += kStreamThreads) {
        const int64_t c = c0 + o;
        int acc = bias;
        for (int t = 0; t < TF; ++t) {
          const int64_t p = c - (TF - 1) + t;
          const int8_t* wd = q.w + net.wd + (int64_t)t * pc;
          if (p >= 0) {
            const int* x = reinterpret_cast<const int*>(fin + p * pc);
            const int* w = reinterpret_cast<const int*>(wd);
            for (int r = 0; r < pc / 4; ++r) acc = mww_sdot4(x[r], w[r], acc);
          } else {
            const int8_t* x = hring + (TF - 1 + p) * C;
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
        const int64_t p = N - (TF - 1) + idx / C;
        const int ch = idx % C;
        q.st_out[net.ring_head + idx] = p >= 0 ? fin[p * pc + ch] : hring[(TF - 1 + p) * C + ch];
      }
    }
    __syncthreads();   // the next tile reuses the buffers
  }
}

}  // namespace

namespace mww {

int64_t stream_graph_q8_sizes(const mww_stream* s, int64_t* n_ints) {
  if (n_ints) *n_ints = s->graph->q_ni;
  return s->graph->q_nw;
}

int stream_graph_set_quantized(mww_stream* s, const int8_t* weights, int64_t n_weights, const int32_t* ints, int64_t n_ints,
                               float input_scale, const uint8_t* lut) {
  const mww_stream_graph* g = s->graph;
  const int n = g->net.n_ops;
  const int64_t nw = g->q_nw, ni = g->q_ni, izp = g->q_izp;
  if (n_weights != nw || n_ints != ni)
    return set_error(MWW_ERR_INVALID, ("expected " + std::to_string(nw) + " int8 weights and " + std::to_string(ni) + " int32 values").c_str());
  if (!(input_scale > 0.f) || !std::isfinite(input_scale)) return set_error(MWW_ERR_INVALID, "input scale must be positive");
  for (int t = 0; t < n + 2; ++t)
    if (ints[izp + t] < -128 || ints[izp + t] > 127) return set_error(MWW_ERR_INVALID, "zero points must lie in [-128, 127]");
  // q8_requant shifts by at most 31 bits either way (see mww_stream_set_quantized of a MixedNet stream)
  auto bad_requant = [&](int64_t at, int64_t cout) {
    for (int64_t c = 0; c < cout; ++c)
      if (ints[at + cout + c] < 0 || ints[at + 2 * cout + c] < -31 || ints[at + 2 * cout + c] > 30) return true;
    return false;
  };
  bool bad = bad_requant(g->qnet.bd, 1);
  for (int i = 0; i < n && !bad; ++i) bad = bad_requant(g->qops[(size_t)i].b, g->qops[(size_t)i].cout);
  if (bad) return set_error(MWW_ERR_INVALID, "requantization multipliers must be >= 0 and shifts lie in [-31, 30]");
  stream_q8_free(s);
  // rings at reset: real zero, i.e. the zero point of the tensor each ring column holds
  std::vector<int8_t> st0((size_t)s->n_state + 4, 0);
  for (int i = 0; i < n; ++i) {
    const GOp& L = g->qops[(size_t)i];
    for (int r = 0; r < L.R; ++r) {
      int64_t at = L.ring + (int64_t)r * L.cin;
      for (int j = 0; j < L.n_src; ++j) {
        const int8_t zp = (int8_t)ints[izp + 1 + g->src[(size_t)i * MWW_MAX_OP_SOURCES + j]];   // source -1: tensor 0, the input
        for (int c = 0; c < L.src_cn[j]; ++c) st0[(size_t)at++] = zp;
      }
    }
  }
  for (int64_t k = 0; k < (int64_t)(g->net.tf - 1) * g->net.c_last; ++k) st0[(size_t)(g->net.ring_head + k)] = (int8_t)ints[izp + n];
  SCHK(hipSetDevice(s->device));
  SCHK(hipMalloc((void**)&s->q8_w, (size_t)nw + 64));
  SCHK(hipMalloc((void**)&s->q8_i, (size_t)ni * 4 + 64));
  SCHK(hipMalloc((void**)&s->q8_lut, 256 + 64));
  for (int i = 0; i < 2; ++i) SCHK(hipMalloc((void**)&s->q8_st[i], st0.size()));
  SCHK(hipMemcpyAsync(s->q8_w, weights, (size_t)nw, hipMemcpyHostToDevice, s->stream));
  SCHK(hipMemcpyAsync(s->q8_i, ints, (size_t)ni * 4, hipMemcpyHostToDevice, s->stream));
  SCHK(hipMemcpyAsync(s->q8_lut, lut, 256, hipMemcpyHostToDevice, s->stream));
  SCHK(hipStreamSynchronize(s->stream));
  s->q8_state0 = st0;
  s->q8_in_scale = input_scale;
  s->q8_in_zp = ints[izp];
  s->q8_izp = izp;
  s->q8_cur = 0;
  s->q8 = true;
  return stream_q8_reset(s);
}

int64_t stream_graph_q8_launch(mww_stream* s, const SStores& S, SCall& a, int grid) {
  const mww_stream_graph* g = s->graph;
  GQ8 q{};
  q.w = s->q8_w;
  q.iv = s->q8_i;
  q.lut = s->q8_lut;
  q.izp = s->q8_izp;
  q.in_scale = s->q8_in_scale;
  q.in_zp = s->q8_in_zp;
  const int64_t n_out = a.n_out;
  int rc = grow(&s->q8_out, &s->cap_q8_out, n_out);
  if (rc) return rc;
  q.out = s->q8_out;
  q.st_in = s->q8_st[s->q8_cur];
  q.st_out = s->q8_st[s->q8_cur ^ 1];
  const int64_t bytes = g->q_tile_bytes;
  q.use_lds = bytes <= kMaxLds;
  size_t lds = 0;
  if (q.use_lds) {
    lds = (size_t)bytes;
    if (lds > 64 * 1024)
      SCHK(hipFuncSetAttribute((const void*)stream_graph_q8_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  } else {
    const int64_t per_wg = (bytes + 255) & ~(int64_t)255;
    if ((rc = grow(&s->q8_scratch, &s->cap_q8_scratch, per_wg * grid))) return rc;
    q.scratch = s->q8_scratch;
    q.scratch_per_wg = per_wg;
  }
  hipLaunchKernelGGL(stream_graph_q8_kernel, dim3(grid), dim3(kStreamThreads), lds, s->stream, g->qnet, S, a, q);
  SCHK(hipGetLastError());
  SCHK(hipStreamSynchronize(s->stream));
  if (s->d.mode == MWW_STREAM_MODE_STREAM) s->q8_cur ^= 1;
  return n_out;
}

}  // namespace mww
