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
//
// Here: the kernel (int8 weights per op [Co][k][source 0: r4(cn_0)] ... [source n-1], then the Dense [T_f][r4(C_last)]) and
// the int8 half of the graph model part.  The head is the shared one of stream_common.hip.h, the host path tu_stream.hip.
#include <hip/hip_runtime.h>

#include "stream_graph.hip.h"

using namespace mww_stream_impl;

namespace {

__global__ void __launch_bounds__(kStreamThreads) stream_graph_q8_kernel(GNet net, SStores S, SCall a, SQ8 q) {
  HIP_DYNAMIC_SHARED(int, gq8_lds)
  const int tid = threadIdx.x;
  int8_t* B = q.use_lds ? reinterpret_cast<int8_t*>(gq8_lds) : q.scratch + (int64_t)blockIdx.x * a.scratch_per_wg;
  const int32_t* zps = q.iv + q.izp;
  for (int tile = blockIdx.x; tile < a.n_tiles; tile += gridDim.x) {
    const STile T = tile_of(a, tile);
    const int64_t c0 = T.c0, c1 = T.c1, v_seg = T.v_seg, N = T.c1;   // positions are frames of the segment
    const bool last = T.last;
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
    dense_head_q8(a, q, T, fin, pc, hring, net.wd, net.bd, zps[net.n_ops + 1], C, TF);
    if (last) head_ring_store(q.st_out + net.ring_head, T, fin, pc, hring, C, TF);
    __syncthreads();   // the next tile reuses the buffers
  }
}

}  // namespace

namespace mww_stream_impl {

// rings at reset: real zero, i.e. the zero point of the tensor each ring column holds
void Graph::q8_state0(const int32_t* zp, int8_t* st0) const {
  const int n = net.n_ops;
  for (int i = 0; i < n; ++i) {
    const GOp& L = qops[(size_t)i];
    for (int r = 0; r < L.R; ++r) {
      int64_t at = L.ring + (int64_t)r * L.cin;
      for (int j = 0; j < L.n_src; ++j) {
        const int8_t z = (int8_t)zp[1 + src[(size_t)i * MWW_MAX_OP_SOURCES + j]];   // source -1: tensor 0, the input
        for (int c = 0; c < L.src_cn[j]; ++c) st0[at++] = z;
      }
    }
  }
  for (int64_t k = 0; k < (int64_t)(net.tf - 1) * net.c_last; ++k) st0[net.ring_head + k] = (int8_t)zp[n];
}

const void* Graph::q8_kernel() const { return (const void*)stream_graph_q8_kernel; }

void Graph::launch_q8(const SStores& S, const SCall& a, const SQ8& q, int grid, size_t lds, hipStream_t hs) const {
  hipLaunchKernelGGL(stream_graph_q8_kernel, dim3(grid), dim3(kStreamThreads), lds, hs, qnet, S, a, q);
}

}  // namespace mww_stream_impl
