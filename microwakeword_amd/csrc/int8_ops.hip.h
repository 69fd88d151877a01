// Integer dot product of the int8 streaming kernels (tu_stream_q8.hip, tu_stream_graph_q8.hip), the input quantization and TFLite's fixed-point requantization.
// On gfx950 mww_sdot4 is v_dot4_i32_i8 (__builtin_amdgcn_sdot4); under the host emulator (HIPEMU) it is a plain C++ twin,
// exact because the arithmetic is integer.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

// sum over the four byte lanes of int8(a) * int8(b), plus c (no clamp: wraps as int32)
#ifdef HIPEMU
static inline int mww_sdot4(int a, int b, int c) {
  uint32_t s = (uint32_t)c;
  for (int k = 0; k < 4; ++k) s += (uint32_t)((int)(int8_t)(a >> (8 * k)) * (int)(int8_t)(b >> (8 * k)));
  return (int)s;
}
#else
__device__ inline int mww_sdot4(int a, int b, int c) { return __builtin_amdgcn_sdot4(a, b, c, false); }
#endif

__device__ inline int8_t quantize_input(float x, float scale, int zp) {
  // inference.py:127-147 (data / scale + zp).astype(int8) with the float32 reading: IEEE division, float32 add, truncation;
  // saturated to [-128, 127]
  float t = x / scale + (float)zp;
  t = truncf(t);
  t = t < -128.f ? -128.f : (t > 127.f ? 127.f : t);
  return (int8_t)(int)t;
}

// SaturatingRoundingDoublingHighMul: (a * b + nudge) / 2^31, C division (truncating)
__device__ inline int32_t q8_srdhm(int32_t a, int32_t b) {
  if (a == INT32_MIN && b == INT32_MIN) return INT32_MAX;
  const int64_t ab = (int64_t)a * (int64_t)b;
  const int64_t v = ab + (ab >= 0 ? ((int64_t)1 << 30) : (1 - ((int64_t)1 << 30)));
  return (int32_t)(v >= 0 ? v >> 31 : -((-v) >> 31));
}

// RoundingDivideByPOT: x / 2^e, ties away from zero
__device__ inline int32_t q8_rdpot(int32_t x, int e) {
  const int32_t mask = (int32_t)(((int64_t)1 << e) - 1);
  const int32_t r = x & mask;
  const int32_t t = (mask >> 1) + (x < 0 ? 1 : 0);
  return (x >> e) + (r > t ? 1 : 0);
}

// MultiplyByQuantizedMultiplier, then + zero point, clamped to [act_min, 127]
__device__ inline int q8_requant(int32_t x, int32_t m, int32_t shift, int zp, int act_min) {
  const int left = shift > 0 ? shift : 0, right = shift > 0 ? 0 : -shift;
  int32_t v = q8_rdpot(q8_srdhm((int32_t)((uint32_t)x << left), m), right) + zp;
  v = v < act_min ? act_min : v;
  return v > 127 ? 127 : v;
}
