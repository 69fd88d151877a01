// The float streaming kernel of a MixedNet with residual connections, a pooled head or spatial attention
// (mww_stream_create_mixednet, include/mww.h; mixednet.py:234-275 SpatialAttention, :340-358 residual, :362-381 pooled head).
// It walks the tiles, the rings and the state layout of stream_forward_kernel (tu_stream.hip), whose comment describes them; a
// plain MixedNet never comes here (MixedNet::launch), so its kernel and its bits are untouched.  What is added:
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
// Every sum runs in a fixed order, nothing is atomic: two runs give the same bits.
//
// <REC> is the calibration form (mww_stream_calibrate_host on a stream of mww_stream_create_mixednet_q8): every thread keeps the
// min / max of the tensor it is computing - a kind-2 layer records r, a kind-3 layer the value before the add and the value
// after add + ReLU as two tensors, the head the logit -, rec_fold runs per layer, one partial row per workgroup.  <false> is the
// kernel without any of it.
#include <hip/hip_runtime.h>

#include "stream_common.hip.h"

using namespace mww_stream_impl;

namespace {

constexpr int kPoolChannels = 8;   // channels a head thread pools at a time (registers)
// input, conv1, the logit; per block a residual; per repeat MixConv, 1x1 and ADD
constexpr int kMaxVarTensors = 3 + MWW_MAX_BLOCKS + 3 * MWW_MAX_BLOCKS * MWW_STREAM_MAX_REPEAT;

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

template <bool REC>
__global__ void __launch_bounds__(kStreamThreads) stream_mixednet_kernel(SNet net, SVar var, SStores S, SCall a) {
  const int tid = threadIdx.x;
  __shared__ float red[REC ? 2 * kStreamThreads : 1], rmin[REC ? kMaxVarTensors : 1], rmax[REC ? kMaxVarTensors : 1];
  float lmin = INFINITY, lmax = -INFINITY, lmin2 = INFINITY, lmax2 = -INFINITY;   // (2: the ADD output of a kind-3 layer)
  if (REC) rec_init(a, rmin, rmax);
  float* G = a.scratch + (int64_t)blockIdx.x * a.scratch_per_wg;            // gathered padded input rows [.][40]
  float* B0 = G + ((a.buf_rows - 1) * net.s + net.k1) * MWW_FEATURE_BINS;   // two activation buffers [rows][cmax]
  float* B1 = B0 + a.buf_rows * net.cmax;
  float* Rb = B1 + a.buf_rows * net.cmax;                                   // the block's residual [rows][cmax] (has_res)
  float* At = Rb + (var.has_res ? a.buf_rows * net.cmax : 0);               // attention: mean, max, gate [rows] each (att)
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
    int64_t in_lo = lo, r_lo = lo;
    for (int l = 0; l < net.n_layers; ++l) {
      const SLayer& L = net.L[l];
      if (L.kind == 2) {   // the block's residual over the block-input range; the buffers are not swapped
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
          rec_fold(lmin, lmax, var.lt[l], red, rmin, rmax);
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
        const bool res = L.kind == 3;
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
          if (REC) {
            float& mn = res ? lmin2 : lmin;
            float& mx = res ? lmax2 : lmax;
            mn = fminf(mn, out[(i - o_lo) * net.cmax + co]);
            mx = fmaxf(mx, out[(i - o_lo) * net.cmax + co]);
          }
        }
      }
      __syncthreads();
      if (REC) {
        rec_fold(lmin, lmax, var.lt[l], red, rmin, rmax);
        if (L.kind == 3) rec_fold(lmin2, lmax2, var.lt[l] + 1, red, rmin, rmax);
        lmin = lmin2 = INFINITY;
        lmax = lmax2 = -INFINITY;
      }
      float* t = in;
      in = out;
      out = t;
      in_lo = o_lo;
    }
    // ---- head
    const float* fin = in - in_lo * net.cmax;
    const float* hring = a.st_in + net.ring_head;
    const float* gate = nullptr;
    if (var.att) {   // non_stream: every position the head reads is >= 0 and in the tile, in_lo = c0 - (tf - 1)
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
    if (var.att || var.pool) {
      variant_head<REC>(a, T, fin, net.cmax, hring, net.wd, net.bd, net.c_last, net.tf, var.tp, var.pool, gate, in_lo, lmin, lmax);
    } else {
      dense_head<REC>(a, T, fin, net.cmax, hring, net.wd, net.bd, net.c_last, net.tf, lmin, lmax);
    }
    if (REC) {
      rec_fold(lmin, lmax, var.n_tensors - 1, red, rmin, rmax);
      lmin = INFINITY;
      lmax = -INFINITY;
    }
    if (last) head_ring_store(a.st_out + net.ring_head, T, fin, net.cmax, hring, net.c_last, net.tf);
    __syncthreads();   // the next tile reuses the scratch
  }
  if (REC) rec_flush(a, rmin, rmax);
}

}  // namespace

namespace mww_stream_impl {

void launch_mixednet_variant(const SNet& net, const SVar& var, const SStores& S, const SCall& a, int grid, hipStream_t hs) {
  if (a.rec)
    hipLaunchKernelGGL(stream_mixednet_kernel<true>, dim3(grid), dim3(kStreamThreads), 0, hs, net, var, S, a);
  else
    hipLaunchKernelGGL(stream_mixednet_kernel<false>, dim3(grid), dim3(kStreamThreads), 0, hs, net, var, S, a);
}

}  // namespace mww_stream_impl
