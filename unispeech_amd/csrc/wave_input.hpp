// The waveform input layer shared by csrc/resample.hip, csrc/mfcc.hip and csrc/fbank.hip: x is a [B, L] batch of fp32 samples
// or int16 PCM (WL_I16, scaled by 1 / 32768 on load) with a row stride in elements, `lengths` (optional, int32 [B]) ends a row
// early, and a workgroup stages the samples under its tile into LDS once, zero outside the row.  The entry points' checks of
// that argument group and the opt-in for dynamic LDS above 48 KiB live here too.
#pragma once
#include "common.hpp"

__device__ __forceinline__ float wave_load(const void* x, long i, int dt) {
  return dt == WL_I16 ? (float)((const short*)x)[i] * (1.0f / 32768.0f) : ((const float*)x)[i];
}

// samples of row b: lengths[b] clamped to [0, L], or L without lengths
__device__ __forceinline__ long wave_row_len(const int* lengths, int b, long L) {
  long len = L;
  if (lengths) { const long l = lengths[b]; len = l < 0 ? 0 : (l < L ? l : L); }
  return len;
}

__device__ __forceinline__ const void* wave_row(const void* x, int b, long x_stride, int dt) {
  return (const char*)x + (size_t)b * x_stride * (dt == WL_I16 ? 2 : 4);
}

// s_x[k] = x[g0 + k] for k < span, zero where the index is outside [0, len); nt threads, this one is tid.  REFLECT: the index
// is first reflected once at either end of the row without repeating the edge sample (g < 0 -> -g; g >= len -> 2 (len - 1) - g)
template <bool REFLECT = false>
__device__ __forceinline__ void wave_stage(float* s_x, const void* xrow, int dt, long g0, int span, long len, int tid, int nt) {
  for (int k = tid; k < span; k += nt) {
    long g = g0 + k;
    if (REFLECT) {
      if (g < 0) g = -g;
      if (g >= len) g = 2 * (len - 1) - g;
    }
    s_x[k] = (g >= 0 && g < len) ? wave_load(xrow, g, dt) : 0.f;
  }
}

// the x / x_dtype / x_stride / B / L arguments of an entry point: B rows fit gridDim.y, 1 <= L <= max_L (the op's own bound,
// which keeps its index arithmetic inside int64), rows do not overlap
static inline int wave_check_input(const void* x, int32_t x_dtype, int64_t x_stride, int32_t B, int64_t L, int64_t max_L) {
  if (!x || B <= 0 || B > 65535 || L <= 0 || L > max_L) return WL_EINVAL;
  if (x_dtype != WL_F32 && x_dtype != WL_I16) return WL_EINVAL;
  return x_stride < L ? WL_EINVAL : WL_OK;
}

// a launch with more than 48 KiB of dynamic LDS needs the kernel's opt-in, up to `budget` bytes.  Set on every such call: the
// attribute is per device, and a flag kept here would be neither per device nor thread-safe
template <typename K>
static inline int wl_dynamic_lds(K kernel, size_t bytes, int budget) {
  if (bytes > 48 * 1024 &&
      hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, budget) != hipSuccess)
    return WL_ELAUNCH;
  return WL_OK;
}
