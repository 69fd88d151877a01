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
// Here: the kernel - <VAR> with TFLite's int8 Add and pooling for a MixedNet with residual connections or a pooled head
// (mww_stream_create_mixednet_q8), <false> for a plain one - and the int8 half of the MixedNet model part (layout of the
// parameters, rings at reset, launch).  The Dense head and the head-ring write-back are the shared ones of stream_common.hip.h.
#include <hip/hip_runtime.h>

#include "stream_common.hip.h"

using namespace mww_stream_impl;

namespace {

// One output of conv1, a 1x1 layer or a residual: the bias, then nw dot4 over a word-aligned row, in word order
__device__ inline int q8_row_dot(int bias, const int8_t* x, const int8_t* w, int nw) {
  const int* xi = reinterpret_cast<const int*>(x);
  const int* wi = reinterpret_cast<const int*>(w);
  int acc = bias;
  for (int r = 0; r < nw; ++r) acc = mww_sdot4(xi[r], wi[r], acc);
  return acc;
}

// ---- <VAR> only: TFLite's int8 Add and the pooled head
constexpr int kPoolChannels = 8;   // channels a head thread pools at a time: two words of the Dense row
constexpr int kAddLeftShift = 20;  // TFLite int8 Add

// TFLite's int8 Add of q1 (zero point z1) and q2 (z2): A = M1, sh1, M2, sh2, Mo, sho, every shift <= 0 (the
// MultiplyByQuantizedMultiplierSmallerThanOneExp form).  |q - z| <= 255, so the left shift fits int32.
__device__ inline int q8_add(int q1, int z1, int q2, int z2, const int32_t* A, int zo, int act_min) {
  const int32_t x1 = (q1 - z1) * (1 << kAddLeftShift), x2 = (q2 - z2) * (1 << kAddLeftShift);
  const int32_t s1 = q8_rdpot(q8_srdhm(x1, A[0]), -A[1]);
  const int32_t s2 = q8_rdpot(q8_srdhm(x2, A[2]), -A[3]);
  int32_t v = q8_rdpot(q8_srdhm(s1 + s2, A[4]), -A[5]) + zo;
  v = v < act_min ? act_min : v;
  return v > 127 ? 127 : v;
}

// Pooled head: per output the T_f frames reduced per channel (average: int32 sum, rounded division away from zero; max), the
// Dense over the C pooled int8 values, then the logit requantization, table and probability of dense_head_q8.
__device__ inline void pooled_head_q8(const SCall& a, const SQ8& q, const STile& T, const int8_t* fin, int pitch, const int8_t* hring,
                                      int64_t wd_at, int64_t id_at, int zo, int C, int TF, int pool) {
  const int32_t bias = q.iv[id_at], mul = q.iv[id_at + 1], shf = q.iv[id_at + 2];
  const int* wd = reinterpret_cast<const int*>(q.w + wd_at);
  for (int o = threadIdx.x; o < T.n; o += kStreamThreads) {
    const int64_t c = T.c0 + o, q0 = c - (TF - 1);
    int acc = bias;
    for (int ch0 = 0; ch0 < C; ch0 += kPoolChannels) {
      const int nc = C - ch0 < kPoolChannels ? C - ch0 : kPoolChannels;
      int p[kPoolChannels];
      for (int t = 0; t < TF; ++t) {   // every channel's frames in order
        const int64_t pos = q0 + t;
        const int8_t* x = (pos >= 0 ? fin + pos * pitch : hring + (TF - 1 + pos) * C) + ch0;
#pragma unroll
        for (int j = 0; j < kPoolChannels; ++j) {
          if (j < nc) {
            const int v = x[j];
            p[j] = t == 0 ? v : (pool == 1 ? p[j] + v : (v > p[j] ? v : p[j]));
          }
        }
      }
      uint32_t w0 = 0, w1 = 0;   // the pooled bytes, four to a word (channels past C: 0 against the row's zero padding)
#pragma unroll
      for (int j = 0; j < kPoolChannels; ++j) {
        int v = 0;
        if (j < nc) {
          v = p[j];
          if (pool == 1) {
            v = v > 0 ? (v + TF / 2) / TF : (v - TF / 2) / TF;
            v = v < -128 ? -128 : (v > 127 ? 127 : v);
          }
        }
        if (j < 4) w0 |= (uint32_t)(uint8_t)(int8_t)v << (8 * j);
        else w1 |= (uint32_t)(uint8_t)(int8_t)v << (8 * (j - 4));
      }
      acc = mww_sdot4((int)w0, wd[ch0 / 4], acc);
      if (nc > 4) acc = mww_sdot4((int)w1, wd[ch0 / 4 + 1], acc);
    }
    const int lq = q8_requant(acc, mul, shf, zo, -128);
    const uint8_t u = q.lut[lq + 128];
    const int64_t g = T.out0 + o;
    q.out[g] = u;
    a.logit[g] = (float)lq;
    a.prob[g] = (float)u * kInv255;
  }
}

// The int8 MixedNet kernel: one tile walk, two instantiations.  <VAR> is the form of a plan with residual connections or a
// pooled head (mww_stream_create_mixednet_q8; contract: INTEGRATION.md 6, "residual and pooled MixedNets"; every item our
// reading of TFLite's reference kernels, not pinned to TFLite, restated in tests/quant_mixednet_oracle.py); all it adds sits
// behind the compile-time VAR, so <false> - the kernel a plain plan runs (MixedNet::launch_q8) - holds none of it:
//
//   residual   layer kind 2: r = 1x1 + folded BN of the block input, requantized LINEARLY (no fused activation) to its own
//              parameters, over the block-input range [in_lo, c1) of the tile, in a third int8 buffer Rb of pitch cp.  No ring.
//              Layer kind 3: the repeat's 1x1 requantized linearly to the pre-add parameters in a register, then TFLite's int8
//              Add (reference_integer_ops::AddElementwise, left_shift 20) with Rb at equal positions, the ReLU fused into the
//              ADD's clamp [max(-128, zp_out), 127], one store.
//   pooling    AVERAGE_POOL_2D / MAX_POOL_2D over (T_f, 1): a head thread reduces kPoolChannels channels at a time in registers
//              over the T_f frames (head ring before the stream start), packs the pooled bytes to words and runs dot4 against
//              the Dense row [1][r4(C)].  The pooled value shares the final map's scale and zero point.
//
// The tile - gathered rows and 2 (VAR: + has_res) int8 buffers - sits in dynamic LDS or the global scratch.  The calibrated
// tensor of layer l is var.lt[l]; without VAR that is 2 + l, which needs no table.
template <bool VAR>
__global__ void __launch_bounds__(kStreamThreads) stream_q8_kernel(SNet net, SVar var, SStores S, SCall a, SQ8Net q) {
  HIP_DYNAMIC_SHARED(int, q8_lds)
  const int tid = threadIdx.x;
  const int64_t g_rows = (a.buf_rows - 1) * net.s + net.k1;
  int8_t* G = q.use_lds ? reinterpret_cast<int8_t*>(q8_lds) : q.scratch + (int64_t)blockIdx.x * a.scratch_per_wg;
  int8_t* B0 = G + g_rows * MWW_FEATURE_BINS;   // 40 bytes a row: stays 4-byte aligned
  int8_t* B1 = B0 + a.buf_rows * q.cp;
  int8_t* Rb = B1 + a.buf_rows * q.cp;          // VAR: the block's residual [rows][cp] (has_res)
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
        const int acc = q8_row_dot(bias[co], G + i * net.s * MWW_FEATURE_BINS, q.w + q.w1 + (int64_t)co * q.kp1, q.kp1 / 4);
        B0[i * cp + co] = (int8_t)q8_requant(acc, mul[co], shf[co], zo, amin);
      }
    }
    __syncthreads();
    int8_t* in = B0;
    int8_t* out = B1;
    int64_t in_lo = lo, r_lo = lo;   // (r_lo, VAR: the position of Rb's first row)
    int t_res = 1;                   // (VAR: the tensor in Rb)
    for (int l = 0; l < net.n_layers; ++l) {
      const SLayer& L = net.L[l];
      const int8_t* wl = q.w + q.lw[l];
      const int32_t* bias = q.iv + q.li[l];
      const int32_t *mul = bias + L.cout, *shf = mul + L.cout;
      const int t_out = VAR ? var.lt[l] : 2 + l;
      const int zo = zps[t_out];
      const int Co = L.cout, nw = (L.cin + 3) / 4;
      // channel co of a 1x1 layer at position i, before its epilogue
      auto pw_dot = [&](int64_t i, int co) { return q8_row_dot(bias[co], in + (i - in_lo) * cp, wl + (int64_t)co * nw * 4, nw); };
      if (VAR && L.kind == 2) {   // the block's residual over the block-input range, linear; the buffers are not swapped
        r_lo = in_lo;
        t_res = t_out;
        for (int64_t idx = tid; idx < (c1 - in_lo) * Co; idx += kStreamThreads) {
          const int64_t i = in_lo + idx / Co;
          const int co = (int)(idx % Co);
          Rb[(i - r_lo) * cp + co] = (int8_t)q8_requant(pw_dot(i, co), mul[co], shf[co], zo, -128);
        }
        __syncthreads();
        continue;
      }
      int64_t o_lo = c0 - L.reach;
      if (o_lo < 0) o_lo = 0;
      const int64_t no = c1 - o_lo;
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
      } else if (!VAR || L.kind == 1) {
        const int amin = zo > -128 ? zo : -128;
        for (int64_t idx = tid; idx < no * Co; idx += kStreamThreads) {
          const int64_t i = o_lo + idx / Co;
          const int co = (int)(idx % Co);
          out[(i - o_lo) * cp + co] = (int8_t)q8_requant(pw_dot(i, co), mul[co], shf[co], zo, amin);
        }
      } else {   // kind 3: linear 1x1 in a register, + r at equal positions (o_lo >= r_lo), ReLU fused into the ADD's clamp
        const int32_t* A = shf + Co;   // M1, sh1, M2, sh2, Mo, sho
        const int z2 = zps[t_res], za = zps[t_out + 1], amin = za > -128 ? za : -128;
        for (int64_t idx = tid; idx < no * Co; idx += kStreamThreads) {
          const int64_t i = o_lo + idx / Co;
          const int co = (int)(idx % Co);
          const int q1 = q8_requant(pw_dot(i, co), mul[co], shf[co], zo, -128);
          out[(i - o_lo) * cp + co] = (int8_t)q8_add(q1, zo, Rb[(i - r_lo) * cp + co], z2, A, za, amin);
        }
      }
      __syncthreads();
      int8_t* t = in;
      in = out;
      out = t;
      in_lo = o_lo;
    }
    // ---- head: pooling + Dense, or the Dense over the last T_f frames; Logistic table, uint8 output, probability u8 / 255
    const int8_t* fin = in - in_lo * cp;
    const int8_t* hring = q.st_in + net.ring_head;
    const int z_logit = zps[VAR ? var.n_tensors - 1 : 2 + net.n_layers];
    if (VAR && var.pool)
      pooled_head_q8(a, q, T, fin, cp, hring, q.wd, q.id, z_logit, net.c_last, net.tf, var.pool);
    else
      dense_head_q8(a, q, T, fin, cp, hring, q.wd, q.id, z_logit, net.c_last, net.tf);
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

const void* MixedNet::q8_kernel() const {
  return variant() ? (const void*)stream_q8_kernel<true> : (const void*)stream_q8_kernel<false>;
}

void MixedNet::launch_q8(const SStores& S, const SCall& a, const SQ8& c, int grid, size_t lds, hipStream_t hs) const {
  SQ8Net k;
  static_cast<SQ8&>(k) = c;
  static_cast<MixedNet::Q8&>(k) = q;
  auto kernel = variant() ? stream_q8_kernel<true> : stream_q8_kernel<false>;
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(kStreamThreads), lds, hs, net, var, S, a, k);
}

}  // namespace mww_stream_impl
