// Transformer LM, incremental decoding: single-query attention over a tree-shaped KV cache (additive to ABI 30).
//
//   wavlm_attn_step   the self-attention of one new token per row (src/fairseq/modules/multihead_attention.py under
//                     incremental_state, one step) where the prefixes of the rows form a tree: a cache entry ("slot") holds
//                     the K and the V of one token for one layer, a row names the slots of its ancestors in position order
//                     and the slot its own k and v go to.  One wave owns one (row, head): key j of the row sits on lane
//                     j % 64, K and V rows go straight from memory to registers (a lane reads its key's whole head row, 64 to
//                     256 contiguous bytes), every lane keeps an online softmax (running maximum, sum and output) over its own
//                     keys in fp32, and the 64 lane states are folded once at the end through LDS in lane order.  The own k
//                     and v are read from the packed row, used from registers as the last key, and stored to the slot from
//                     those registers: nothing written by a launch is read by it.  No atomics; a row's bits depend neither on
//                     R nor on its place in the batch.
#include "common.hpp"
#include "../../include/wavlm_hip.h"

#include <math.h>

namespace {

constexpr int AS_NT = 64;              // one wave per workgroup

template <typename T, int DK> struct StepRow;
template <int DK> struct StepRow<float, DK> {
  static constexpr int NV = DK / 4;    // 16-byte vectors per head row
  static __device__ __forceinline__ void unpack(const uint4& u, float* f) {
    f[0] = __uint_as_float(u.x); f[1] = __uint_as_float(u.y); f[2] = __uint_as_float(u.z); f[3] = __uint_as_float(u.w);
  }
  static constexpr int PER = 4;
};
template <int DK> struct StepRow<bf16_t, DK> {
  static constexpr int NV = DK / 8;
  static __device__ __forceinline__ void unpack(const uint4& u, float* f) {
    f[0] = __uint_as_float(u.x << 16); f[1] = __uint_as_float(u.x & 0xffff0000u);
    f[2] = __uint_as_float(u.y << 16); f[3] = __uint_as_float(u.y & 0xffff0000u);
    f[4] = __uint_as_float(u.z << 16); f[5] = __uint_as_float(u.z & 0xffff0000u);
    f[6] = __uint_as_float(u.w << 16); f[7] = __uint_as_float(u.w & 0xffff0000u);
  }
  static constexpr int PER = 8;
};

// grid: row * H + head
template <typename T, int DK>
__global__ __launch_bounds__(AS_NT) void attn_step_kernel(const T* __restrict__ qkv, int64_t ld_qkv, T* __restrict__ Kc,
                                                          T* __restrict__ Vc, int64_t ld_kv, int64_t slots,
                                                          const int* __restrict__ slot, const int* __restrict__ anc,
                                                          int64_t ld_anc, const int* __restrict__ lengths, int max_length,
                                                          T* __restrict__ O, int64_t ld_o, int H, float scale) {
  typedef StepRow<T, DK> RW;
  constexpr int NV = RW::NV, PER = RW::PER;
  __shared__ float fold[AS_NT][DK + 1];            // lane i's scaled output, its scaled sum in column DK
  const int lane = threadIdx.x;
  const int64_t r = blockIdx.x / H;
  const int h = blockIdx.x % H;
  const int L = lengths[r];
  T* orow = O + r * ld_o + h * DK;
  if (L <= 0) {                                    // a skipped row: zeros, nothing stored
    if (lane < DK) orow[lane] = (T)0;
    return;
  }
  const int own = slot[r];
  // what the caller must not pass: the row comes back as NaN and stores nothing (no address is formed from a bad index)
  bool bad = L > max_length || own < 0 || own >= slots;
  const T* qrow = qkv + r * ld_qkv + h * DK;
  float q[DK];
#pragma unroll
  for (int i = 0; i < NV; ++i) RW::unpack(*(const uint4*)(qrow + PER * i), q + PER * i);

  float m = -INFINITY, l = 0.f, o[DK];
#pragma unroll
  for (int c = 0; c < DK; ++c) o[c] = 0.f;

  const int nanc = bad ? 0 : L - 1;                // ancestors: keys 0 .. L - 2; the own key is key L - 1
  for (int j0 = 0; j0 < L && !bad; j0 += AS_NT) {  // uniform over the wave
    const int j = j0 + lane;
    const bool is_anc = j < nanc, is_own = j == L - 1;
    int a = 0;
    if (is_anc) a = anc[r * ld_anc + j];
    const bool oob = is_anc && (a < 0 || a >= slots);
    if (__any(oob)) { bad = true; break; }
    if (!is_anc && !is_own) continue;
    const T* krow = is_own ? qrow + H * DK : Kc + (int64_t)a * ld_kv + h * DK;
    const T* vrow = is_own ? qrow + 2 * H * DK : Vc + (int64_t)a * ld_kv + h * DK;
    uint4 kv[NV], vv[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) kv[i] = *(const uint4*)(krow + PER * i);
#pragma unroll
    for (int i = 0; i < NV; ++i) vv[i] = *(const uint4*)(vrow + PER * i);
    if (is_own) {                                  // the cache write, from the registers the softmax uses
      T* kdst = Kc + (int64_t)own * ld_kv + h * DK;
      T* vdst = Vc + (int64_t)own * ld_kv + h * DK;
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        *(uint4*)(kdst + PER * i) = kv[i];
        *(uint4*)(vdst + PER * i) = vv[i];
      }
    }
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      float f[PER];
      RW::unpack(kv[i], f);
#pragma unroll
      for (int e = 0; e < PER; ++e) s = fmaf(q[PER * i + e], f[e], s);
    }
    float mn, rs, p;
    {
      // s * scale must round before mn is subtracted: contracted into fma(s, scale, -mn) the difference is the product's
      // rounding error instead of 0 at a lane's first key, and p = exp(0) = 1 is lost (a single key returns v bitwise)
#pragma clang fp contract(off)
      s = s * scale;
      mn = fmaxf(m, s);
      rs = expf(m - mn);                           // exp(-inf) = 0 at the lane's first key
      p = expf(s - mn);
    }
    m = mn;
    l = l * rs + p;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      float f[PER];
      RW::unpack(vv[i], f);
#pragma unroll
      for (int e = 0; e < PER; ++e) o[PER * i + e] = fmaf(p, f[e], o[PER * i + e] * rs);
    }
  }
  if (bad) {
    if (lane < DK) {
      if (sizeof(T) == 4) ((float*)orow)[lane] = __builtin_nanf("");
      else ((bf16_t*)orow)[lane] = (bf16_t)0x7fc0;
    }
    return;
  }
  // fold the 64 lane states: the row maximum, every lane's state scaled to it, the sums in lane order
  const float M = wave_max(m);                     // finite: the own key exists
  const float w = expf(m - M);                     // 0 for a lane without a key
#pragma unroll
  for (int c = 0; c < DK; ++c) fold[lane][c] = o[c] * w;
  fold[lane][DK] = l * w;
  __syncthreads();
  float lsum = 0.f, osum = 0.f;
  const int c = lane < DK ? lane : 0;
  for (int i = 0; i < AS_NT; ++i) {
    lsum += fold[i][DK];
    osum += fold[i][c];
  }
  if (lane < DK) {
    const float y = osum / lsum;
    if (sizeof(T) == 4) ((float*)orow)[lane] = y;
    else ((bf16_t*)orow)[lane] = f2bf(y);
  }
}

inline bool step_dt_ok(int dt) { return dt == WL_F32 || dt == WL_BF16; }

}  // namespace

extern "C" {

int wavlm_attn_step_supported(int32_t head_dim, int32_t dtype) {
  return (head_dim == 32 || head_dim == 64) && step_dt_ok(dtype) ? 1 : 0;
}

int wavlm_attn_step(const void* qkv, int64_t ld_qkv, void* Kc, void* Vc, int64_t ld_kv, int64_t slots, const int32_t* slot,
                    const int32_t* anc, int64_t ld_anc, const int32_t* lengths, int32_t max_length, void* O, int64_t ld_o,
                    int32_t R, int32_t H, int32_t head_dim, int32_t dtype, float scale, void* stream) {
  if (!qkv || !Kc || !Vc || !slot || !anc || !lengths || !O || R < 1 || H < 1 || slots < 1 || max_length < 1 ||
      !wavlm_attn_step_supported(head_dim, dtype))
    return WL_EINVAL;
  const int64_t es = (int64_t)wl_esize(dtype), D = (int64_t)H * head_dim;
  if (ld_qkv < 3 * D || ld_kv < D || ld_o < D || ld_anc < (int64_t)max_length - 1 || ld_anc < 0) return WL_EINVAL;
  if (((uintptr_t)qkv & 15) || ((uintptr_t)Kc & 15) || ((uintptr_t)Vc & 15) || ((uintptr_t)O & 15) || (ld_qkv * es) % 16 ||
      (ld_kv * es) % 16 || (ld_o * es) % 16 || ((uintptr_t)slot & 3) || ((uintptr_t)anc & 3) || ((uintptr_t)lengths & 3))
    return WL_EINVAL;
  // qkv, Kc, Vc and O must not overlap: the byte ranges [first row, end of the last row) are compared, not only the pointers
  const uintptr_t b[4] = {(uintptr_t)qkv, (uintptr_t)Kc, (uintptr_t)Vc, (uintptr_t)O};
  const uint64_t n[4] = {(uint64_t)(((int64_t)R - 1) * ld_qkv + 3 * D) * es, (uint64_t)((slots - 1) * ld_kv + D) * es,
                         (uint64_t)((slots - 1) * ld_kv + D) * es, (uint64_t)(((int64_t)R - 1) * ld_o + D) * es};
  for (int i = 0; i < 4; ++i)
    for (int j = i + 1; j < 4; ++j)
      if (b[i] < b[j] + n[j] && b[j] < b[i] + n[i]) return WL_EINVAL;
  if ((int64_t)R * H > 0x7fffffffll) return WL_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)((int64_t)R * H)), block(AS_NT);
#define AS_GO(T, DK)                                                                                                        \
  WL_LAUNCH((attn_step_kernel<T, DK>), grid, block, 0, st, (const T*)qkv, ld_qkv, (T*)Kc, (T*)Vc, ld_kv, slots, slot, anc, \
            ld_anc, lengths, (int)max_length, (T*)O, ld_o, (int)H, scale)
  if (dtype == WL_BF16) {
    if (head_dim == 32) AS_GO(bf16_t, 32); else AS_GO(bf16_t, 64);
  } else {
    if (head_dim == 32) AS_GO(float, 32); else AS_GO(float, 64);
  }
#undef AS_GO
  return wl_check_launch();
}

}  // extern "C"
