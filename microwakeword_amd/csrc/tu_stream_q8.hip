// int8 streaming inference of a MixedNet (mww_stream_set_quantized, include/mww.h): the quantized streaming model the
// reference converts with representative-dataset calibration (utils.py:288-360, --test_tflite_streaming_quantized), restated
// after TFLite's int8 kernels (ConvPerChannel / DepthwiseConvPerChannel / FullyConnected / Logistic reference semantics).
//
// The same whole-sequence form, tiles and ring layout as the float kernel (stream_common.hip.h, tu_stream.hip): a tile of
// up to 256 outputs recomputes its halo; positions before the stream start read the rings, now int8 values of each layer's
// input tensor with that tensor's parameters; the tile that ends a stream-mode call writes the next rings.  Activations
// are int8 [rows][cp] with the row pitch cp = cmax rounded up to 4, so the 1x1 contractions, conv1 and the Dense run as
// v_dot4_i32_i8 (int8_ops.hip.h) over 32-bit words; the input zero point is folded into the bias on the host (exact in
// integers).  The depthwise taps are int32 MACs.  A tile's buffers sit in LDS when they fit (the default topologies:
// 69-80 KB), else in a per-workgroup global scratch (the host path of tu_stream.hip decides).  Every sum runs in a fixed
// order and every op is an exact integer function of its inputs: outputs and rings are bit-identical from run to run and
// equal to the NumPy restatement.
//
// Here: the kernel and the int8 half of the MixedNet model part (layout of the parameters, rings at reset, launch).  The
// head and the head-ring write-back are the shared ones of stream_common.hip.h.
#include <hip/hip_runtime.h>

#include "stream_common.hip.h"

using namespace mww_stream_impl;

namespace {

__global__ void __launch_bounds__(kStreamThreads) stream_q8_kernel(SNet net, SStores S, SCall a, SQ8Net q) {
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
    const STile T = tile_of(a, tile);
    const int64_t c0 = T.c0, c1 = T.c1, v_seg = T.v_seg, N = T.c1;
    const bool last = T.last;
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
    const int8_t* fin = in - in_lo * cp;
    const int8_t* hring = q.st_in + net.ring_head;
    dense_head_q8(a, q, T, fin, cp, hring, q.wd, q.id, zps[2 + net.n_layers], net.c_last, net.tf);
    if (last) head_ring_store(q.st_out + net.ring_head, T, fin, cp, hring, net.c_last, net.tf);
    __syncthreads();   // the next tile reuses the buffers
  }
}

}  // namespace

namespace mww_stream_impl {

// offsets of every op's int8 weights and int32 values (include/mww.h, mww_stream_set_quantized); each op's weights
// start on a 4-byte boundary
void MixedNet::plan_q8() {
  int64_t w = 0, i = 0;
  auto ints = [&](int cout) {   // bias, multiplier, shift [cout]
    q8_requant.emplace_back(i, cout);
    i += 3 * (int64_t)cout;
    return q8_requant.back().first;
  };
  q.w1 = w;
  w = r4(w + (int64_t)net.c1 * net.k1 * MWW_FEATURE_BINS);
  q.i1 = ints(net.c1);
  std::vector<int64_t> li;
  for (const SLayer& L : layers) {
    q8_off.push_back(w);
    li.push_back(ints(L.cout));
    if (L.kind == 3) {   // the ADD of a residual block's 1x1: M1, sh1, M2, sh2, Mo, sho
      q8_add.push_back(i);
      i += 6;
    }
    w = r4(w + (L.kind == 0 ? (int64_t)L.k * L.cin : (int64_t)L.cout * r4(L.cin)));
  }
  q8_off.insert(q8_off.end(), li.begin(), li.end());
  q.wd = w;
  w = r4(w + (int64_t)(var.pool ? 1 : net.tf) * r4(net.c_last));   // a pooled Dense reads the C pooled values
  q.id = ints(1);
  q8_izp = i;
  q8_nw = w;
  q8_ni = i + n_tensors;
  q.kp1 = net.k1 * MWW_FEATURE_BINS;
  q.cp = (int)r4(net.cmax);
}

// rings at reset: real zero, i.e. the zero point of the tensor under each ring (conv1: the input, MixConv: its input - in a
// residual block's repeat >= 1 the previous ADD output -, head: the final map)
void MixedNet::q8_state0(const int32_t* zp, int8_t* st0) const {
  for (int64_t k = 0; k < (int64_t)net.r1 * MWW_FEATURE_BINS; ++k) st0[net.ring1 + k] = (int8_t)zp[0];
  int t_in = 1;   // the tensor the next layer reads
  for (size_t l = 0; l < layers.size(); ++l) {
    const SLayer& L = layers[l];
    if (L.kind == 0)
      for (int64_t k = 0; k < (int64_t)(L.k - 1) * L.cin; ++k) st0[L.ring + k] = (int8_t)zp[t_in];
    if (L.kind != 2) t_in = lt[l] + (L.kind == 3 ? 1 : 0);   // a residual is kept aside: the next layer still reads the block input
  }
  for (int64_t k = 0; k < (int64_t)(net.tf - 1) * net.c_last; ++k) st0[net.ring_head + k] = (int8_t)zp[t_in];
}

const void* MixedNet::q8_kernel() const { return variant() ? mixednet_variant_q8_kernel() : (const void*)stream_q8_kernel; }

void MixedNet::launch_q8(const SStores& S, const SCall& a, const SQ8& c, int grid, size_t lds, hipStream_t hs) const {
  SQ8Net k;
  static_cast<SQ8&>(k) = c;
  static_cast<MixedNet::Q8&>(k) = q;
  if (variant())   // residuals / pooled head: tu_stream_mixednet_q8.hip; a plain plan never leaves the kernel above
    launch_mixednet_variant_q8(net, var, S, a, k, grid, lds, hs);
  else
    hipLaunchKernelGGL(stream_q8_kernel, dim3(grid), dim3(kStreamThreads), lds, hs, net, S, a, k);
}

}  // namespace mww_stream_impl
