// Speaker-diarization head (EEND with vector clustering over the upstream's layer states) on the device: the inference path
// of the reference's downstreams/speaker_diarization/models/models.py and models/transformer.py.  The Linear layers are
// wavlm_gemm calls and the LayerNorms wavlm_layernorm_fwd calls (host side, unispeech_amd/diarization.py); this file holds the
// three steps that had no kernel.
//
// Entry points (include/wavlm_hip.h, "diarization head"):
//   wavlm_diar_front      models.py:210-225 with context_size 0: softmax-weighted layer mix + 1e-6, InstanceNorm1d over time,
//                         every `subsampling`-th frame, linear interpolation in time to T_out frames, channel-last.  One
//                         workgroup owns (chunk, 16 channels) over all of T' and keeps the mixed slab in LDS as fp32 (96 KiB at
//                         1536 frames): for T' <= 1536 every state element is read from HBM ONCE.  A frame beyond the 1536 the
//                         slab holds is mixed again wherever it is used: once for the variance and once per interpolation tap
//                         that lands on it (at most twice when T_out <= T_in), i.e. up to four reads of those frames only.
//   wavlm_attn_plain_fwd  transformer.py:55-69: O = softmax(Q K^T / sqrt(d_k)) V from the packed [B, T, 3 H d_k] tensor, d_k =
//                         32, any T, online softmax; no bias, no mask, no dropout, nothing of size [B H, T, T].  bf16: a wave
//                         owns 32 queries; S^T = K Q^T and O^T = V^T P^T on v_mfma_f32_32x32x16_bf16, so the query sits on the
//                         lane in both accumulators, the softmax state is per lane and P goes from the first accumulator into
//                         the second product's operand without leaving the registers (the keys of a 16-key step are taken in
//                         the order the accumulator holds them, and V^T is read from LDS in that same order).  fp32 (parity
//                         mode): one thread per query, fp32 FMA against K / V tiles in LDS.
//   wavlm_diar_estimate   models.py:232-250, 325-344: from Z = [logits | S speaker-vector projections] per frame: activities =
//                         sigmoid(logits) and v[b, s] = normalize(sum_t sigmoid(y[b, t, s]) z[b, t, s, :] / |z[b, t, s, :]|).
//                         One workgroup per (chunk, speaker): waves stride over time, then a fixed-order sum over the waves.
// Arithmetic is fp32 everywhere but for the bf16 MFMA operands of the attention; nothing is reduced across workgroups, so
// results are bitwise reproducible, and no chunk's result depends on the batch it is in.
#include "common.hpp"
#include "tile_loaders.hpp"
#include "../../include/wavlm_hip.h"

#include <math.h>

namespace {

constexpr int DIAR_MAX_STATES = 32;
constexpr int FR_CS = 16;           // channels per workgroup
constexpr int FR_NT = 512;          // 32 time phases
constexpr int FR_SLAB_T = 1536;     // frames of the mixed slab kept in LDS (96 KiB)

struct DiarStates {
  const void* p[DIAR_MAX_STATES];
  int64_t sb[DIAR_MAX_STATES];
  int64_t st[DIAR_MAX_STATES];
};

inline bool diar_dt_ok(int dt) { return dt == WL_F32 || dt == WL_BF16; }

// ---------------------------------------------------------------------------- layer mix + instance norm + interpolation
__device__ __forceinline__ float front_mix(const DiarStates& S, int n, int dt, const float* ws, int64_t b, int64_t t, int c,
                                           float add) {
  float m = 0.f;
  for (int l = 0; l < n; ++l) m = fmaf(ws[l], ld_elem(S.p[l], b * S.sb[l] + t * S.st[l] + c, dt), m);
  return m + add;
}

// sum over the phases of one channel, in phase order, by every thread of that channel (identical in all of them)
template <int PH>
__device__ __forceinline__ float front_reduce(float* red, int cl, int ph, float v) {
  __syncthreads();
  red[ph * FR_CS + cl] = v;
  __syncthreads();
  float s = 0.f;
  for (int p = 0; p < PH; ++p) s += red[p * FR_CS + cl];
  return s;
}

// grid (ceil(D / 16), B): thread (channel, phase of 32)
__global__ __launch_bounds__(FR_NT) void diar_front_kernel(DiarStates S, int n, int dt, const float* __restrict__ w, int T, int D,
                                                           int sub, int T_out, void* out, int odt, int64_t osb, int64_t ost,
                                                           float add, float eps, int slab_T) {
  extern __shared__ float slab[];  // [slab_T][FR_CS]
  constexpr int PH = FR_NT / FR_CS;
  __shared__ float red[PH * FR_CS];
  __shared__ float ws[DIAR_MAX_STATES];
  const int tid = threadIdx.x, cl = tid % FR_CS, ph = tid / FR_CS;
  const int b = blockIdx.y, c = blockIdx.x * FR_CS + cl;
  const bool cin = c < D;
  if (tid < n) ws[tid] = w[tid];
  __syncthreads();

  float sum = 0.f;
  if (cin)
    for (int t = ph; t < T; t += PH) {
      const float m = front_mix(S, n, dt, ws, b, t, c, add);
      if (t < slab_T) slab[t * FR_CS + cl] = m;
      sum += m;
    }
  sum = front_reduce<PH>(red, cl, ph, sum);
  const float inv_n = 1.f / (float)T;
  const float mean = sum * inv_n;
  float sq = 0.f;
  if (cin)
    for (int t = ph; t < T; t += PH) {
      const float m = t < slab_T ? slab[t * FR_CS + cl] : front_mix(S, n, dt, ws, b, t, c, add);
      const float d = m - mean;
      sq = fmaf(d, d, sq);
    }
  sq = front_reduce<PH>(red, cl, ph, sq);
  const float rstd = 1.f / sqrtf(sq * inv_n + eps);
  if (!cin) return;
  // F.interpolate(mode="linear", align_corners=False) over the subsampled frames x[i] = normed[i * sub]
  const int T_in = (T + sub - 1) / sub;
  const float scale = (float)T_in / (float)T_out;
  for (int j = ph; j < T_out; j += PH) {
    float src = scale * ((float)j + 0.5f) - 0.5f;
    if (src < 0.f) src = 0.f;
    int i0 = (int)src;
    if (i0 > T_in - 1) i0 = T_in - 1;
    const int i1 = i0 + 1 < T_in ? i0 + 1 : T_in - 1;
    const float f = src - (float)i0;
    const int t0 = i0 * sub, t1 = i1 * sub;
    const float m0 = t0 < slab_T ? slab[t0 * FR_CS + cl] : front_mix(S, n, dt, ws, b, t0, c, add);
    const float m1 = t1 < slab_T ? slab[t1 * FR_CS + cl] : front_mix(S, n, dt, ws, b, t1, c, add);
    const float y = (1.f - f) * ((m0 - mean) * rstd) + f * ((m1 - mean) * rstd);
    st_elem(out, (int64_t)b * osb + (int64_t)j * ost + c, odt, y);
  }
}

// ------------------------------------------------------------------------------------------------------ plain attention
constexpr int AP_DK = 32;           // head width

// fp32: grid (ceil(T / 128), B * H); one thread per query, K / V tiles of 64 keys in LDS (broadcast reads)
constexpr int APF_Q = 128;
constexpr int APF_KT = 64;

__global__ __launch_bounds__(APF_Q) void attn_plain_f32_kernel(const float* __restrict__ qkv, float* __restrict__ O, int T, int H,
                                                               float scale) {
  __shared__ float4 Ks[APF_KT][AP_DK / 4];
  __shared__ float4 Vs[APF_KT][AP_DK / 4];
  const int tid = threadIdx.x;
  const int b = blockIdx.y / H, h = blockIdx.y % H;
  const int64_t ld = (int64_t)3 * H * AP_DK;
  const float* base = qkv + (int64_t)b * T * ld + h * AP_DK;
  const int q = blockIdx.x * APF_Q + tid;
  const int qr = q < T ? q : T - 1;
  float4 qv[AP_DK / 4], o[AP_DK / 4];
#pragma unroll
  for (int i = 0; i < AP_DK / 4; ++i) {
    qv[i] = *(const float4*)(base + (int64_t)qr * ld + 4 * i);
    o[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  float m = -INFINITY, l = 0.f;
  for (int k0 = 0; k0 < T; k0 += APF_KT) {
    const int kn = T - k0 < APF_KT ? T - k0 : APF_KT;
    __syncthreads();
    for (int e = tid; e < APF_KT * (AP_DK / 4); e += APF_Q) {
      const int r = e / (AP_DK / 4), c4 = e % (AP_DK / 4);
      float4 kv = make_float4(0.f, 0.f, 0.f, 0.f), vv = kv;
      if (r < kn) {
        const float* row = base + (int64_t)(k0 + r) * ld + 4 * c4;
        kv = *(const float4*)(row + H * AP_DK);
        vv = *(const float4*)(row + 2 * H * AP_DK);
      }
      Ks[r][c4] = kv; Vs[r][c4] = vv;
    }
    __syncthreads();
    for (int kk = 0; kk < kn; kk += 8) {
      float s[8];
      float cm = -INFINITY;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float d = 0.f;
#pragma unroll
        for (int i = 0; i < AP_DK / 4; ++i) {
          const float4 kv = Ks[kk + j][i];
          d = fmaf(qv[i].x, kv.x, d); d = fmaf(qv[i].y, kv.y, d); d = fmaf(qv[i].z, kv.z, d); d = fmaf(qv[i].w, kv.w, d);
        }
        s[j] = kk + j < kn ? d * scale : -INFINITY;
        cm = fmaxf(cm, s[j]);
      }
      const float mn = fmaxf(m, cm);          // finite: key kk exists
      const float r = expf(m - mn);           // exp(-inf) = 0 at the first chunk
      l *= r;
#pragma unroll
      for (int i = 0; i < AP_DK / 4; ++i) { o[i].x *= r; o[i].y *= r; o[i].z *= r; o[i].w *= r; }
      m = mn;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float p = expf(s[j] - mn);
        l += p;
#pragma unroll
        for (int i = 0; i < AP_DK / 4; ++i) {
          const float4 vv = Vs[kk + j][i];
          o[i].x = fmaf(p, vv.x, o[i].x); o[i].y = fmaf(p, vv.y, o[i].y); o[i].z = fmaf(p, vv.z, o[i].z);
          o[i].w = fmaf(p, vv.w, o[i].w);
        }
      }
    }
  }
  if (q >= T) return;
  const float inv = 1.f / l;
  float* orow = O + ((int64_t)b * T + q) * (H * AP_DK) + h * AP_DK;
#pragma unroll
  for (int i = 0; i < AP_DK / 4; ++i)
    *(float4*)(orow + 4 * i) = make_float4(o[i].x * inv, o[i].y * inv, o[i].z * inv, o[i].w * inv);
}

// bf16: grid (ceil(T / 128), B * H); 4 waves, wave w owns queries [32 w, 32 w + 32) of the workgroup's 128; key tiles of 64
// in LDS: K row-major (A operand of S^T = K Q^T), V transposed (A operand of O^T = V^T P^T).
constexpr int APM_NT = 256;
constexpr int APM_Q = 128;
constexpr int APM_KT = 64;
constexpr int APM_KLD = AP_DK + 8;     // bf16 per K row: 80 bytes, 16-byte aligned
constexpr int APM_VLD = APM_KT + 4;    // bf16 per V^T row: 136 bytes, 8-byte aligned

typedef __attribute__((ext_vector_type(16))) float ap_f32x16;

__global__ __launch_bounds__(APM_NT) void attn_plain_bf16_kernel(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ O, int T,
                                                                 int H, float scale) {
  __shared__ __attribute__((aligned(16))) bf16_t Ks[APM_KT * APM_KLD];
  __shared__ __attribute__((aligned(16))) bf16_t Vt[AP_DK * APM_VLD];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int r = lane & 31, hi = lane >> 5;
  const int b = blockIdx.y / H, h = blockIdx.y % H;
  const int64_t ld = (int64_t)3 * H * AP_DK;
  const bf16_t* base = qkv + (int64_t)b * T * ld + h * AP_DK;
  const int q = blockIdx.x * APM_Q + wv * 32 + r;
  const int qr = q < T ? q : T - 1;
  // B operand of S^T: Q[query r][d = 16 s + 8 hi + j]
  bf16x8_t qf[2];
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    U4 u; u.v = *(const uint4*)(base + (int64_t)qr * ld + 16 * s + 8 * hi);
    qf[s] = u.b;
  }
  ap_f32x16 oacc;
#pragma unroll
  for (int i = 0; i < 16; ++i) oacc[i] = 0.f;
  float m = -INFINITY, l = 0.f;   // l: this half-wave's part of the row sum

  for (int k0 = 0; k0 < T; k0 += APM_KT) {
    __syncthreads();
    {  // thread: key tid / 4, 8 channels (tid % 4) * 8 of K and of V
      const int kr = tid >> 2, c8 = (tid & 3) * 8;
      U4 ku, vu;
      ku.v = make_uint4(0u, 0u, 0u, 0u); vu.v = ku.v;
      if (k0 + kr < T) {
        const bf16_t* row = base + (int64_t)(k0 + kr) * ld + c8;
        ku.v = *(const uint4*)(row + H * AP_DK);
        vu.v = *(const uint4*)(row + 2 * H * AP_DK);
      }
      *(uint4*)(Ks + kr * APM_KLD + c8) = ku.v;
#pragma unroll
      for (int j = 0; j < 8; ++j)
        Vt[(c8 + j) * APM_VLD + kr] = (bf16_t)((vu.u[j >> 1] >> ((j & 1) * 16)) & 0xffffu);
    }
    __syncthreads();
#pragma unroll
    for (int kt = 0; kt < APM_KT / 32; ++kt) {
      const int kb = k0 + kt * 32;
      if (kb >= T) break;                     // uniform over the workgroup
      ap_f32x16 sacc;
#pragma unroll
      for (int i = 0; i < 16; ++i) sacc[i] = 0.f;
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        U4 a; a.v = *(const uint4*)(Ks + (kt * 32 + r) * APM_KLD + 16 * s + 8 * hi);
        sacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.b, qf[s], sacc, 0, 0, 0);
      }
      // sacc[i]: key kb + (i & 3) + 8 (i >> 2) + 4 hi, query r
      float cm = -INFINITY;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int key = kb + (i & 3) + 8 * (i >> 2) + 4 * hi;
        const float v = key < T ? sacc[i] * scale : -INFINITY;
        sacc[i] = v;
        cm = fmaxf(cm, v);
      }
      cm = wl_max_xor32(cm);                  // both halves of a query's keys: finite (key kb exists)
      const float mn = fmaxf(m, cm);
      const float rs = __expf(m - mn);
      m = mn;
      l *= rs;
#pragma unroll
      for (int i = 0; i < 16; ++i) oacc[i] *= rs;
      float p[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) { p[i] = __expf(sacc[i] - mn); l += p[i]; }
      // O^T += V^T P^T over this tile's keys in two steps of 16; step s, slot e of half hi is accumulator register 8 s + e,
      // i.e. key kb + 16 s + 8 (e >> 2) + 4 hi + (e & 3): V^T is read in that order
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        U4 pb;
#pragma unroll
        for (int e = 0; e < 4; ++e) pb.u[e] = pack_bf16x2(p[8 * s + 2 * e], p[8 * s + 2 * e + 1]);
        const bf16_t* vrow = Vt + r * APM_VLD + kt * 32 + 16 * s + 4 * hi;
        const uint2 v0 = *(const uint2*)vrow, v1 = *(const uint2*)(vrow + 8);
        U4 va; va.u[0] = v0.x; va.u[1] = v0.y; va.u[2] = v1.x; va.u[3] = v1.y;
        oacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(va.b, pb.b, oacc, 0, 0, 0);
      }
    }
  }
  l = wl_sum_xor32(l);
  if (q >= T) return;
  const float inv = 1.f / l;
  // oacc[i]: channel (i & 3) + 8 (i >> 2) + 4 hi of query r
  bf16_t* orow = O + ((int64_t)b * T + q) * (H * AP_DK) + h * AP_DK + 4 * hi;
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    uint2 v;
    v.x = pack_bf16x2(oacc[4 * g] * inv, oacc[4 * g + 1] * inv);
    v.y = pack_bf16x2(oacc[4 * g + 2] * inv, oacc[4 * g + 3] * inv);
    *(uint2*)(orow + 8 * g) = v;
  }
}

// ---------------------------------------------------------------------------------------------------------------- read-out
constexpr int EST_NT = 1024;        // 16 waves
constexpr int EST_NW = EST_NT / 64;
constexpr int EST_MAXV = 8;         // E <= 512

// grid (S, B): wave w takes frames w, w + 16, ...; lane holds channels lane + 64 j
__global__ __launch_bounds__(EST_NT) void diar_estimate_kernel(const void* Z, int zdt, int64_t sbz, int64_t ldz, int T, int S,
                                                               int E, float* __restrict__ act, void* vec, int vdt) {
  extern __shared__ float part[];   // [EST_NW][E]
  __shared__ float red[EST_NW];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int s = blockIdx.x, b = blockIdx.y;
  float acc[EST_MAXV];
#pragma unroll
  for (int j = 0; j < EST_MAXV; ++j) acc[j] = 0.f;
  for (int t = wv; t < T; t += EST_NW) {
    const int64_t row = (int64_t)b * sbz + (int64_t)t * ldz;
    const float a = 1.f / (1.f + expf(-ld_elem(Z, row + s, zdt)));
    if (lane == 0) act[((int64_t)b * T + t) * S + s] = a;
    float v[EST_MAXV], ss = 0.f;
#pragma unroll
    for (int j = 0; j < EST_MAXV; ++j) {
      const int e = lane + 64 * j;
      v[j] = e < E ? ld_elem(Z, row + S + (int64_t)s * E + e, zdt) : 0.f;
      ss = fmaf(v[j], v[j], ss);
    }
    const float inv = 1.f / sqrtf(wave_sum(ss));
#pragma unroll
    for (int j = 0; j < EST_MAXV; ++j) acc[j] = fmaf(v[j] * inv, a, acc[j]);
  }
#pragma unroll
  for (int j = 0; j < EST_MAXV; ++j) {
    const int e = lane + 64 * j;
    if (e < E) part[wv * E + e] = acc[j];
  }
  __syncthreads();
  float sum = 0.f;
  if (tid < E)
    for (int w = 0; w < EST_NW; ++w) sum += part[w * E + tid];
  const float ws2 = wave_sum(sum * sum);
  if (lane == 0) red[wv] = ws2;
  __syncthreads();
  float tot = 0.f;
  for (int w = 0; w < EST_NW; ++w) tot += red[w];
  if (tid < E) st_elem(vec, ((int64_t)b * S + s) * E + tid, vdt, sum / sqrtf(tot));
}

}  // namespace

extern "C" {

int wavlm_diar_front(const void* const* states, const int64_t* stride_b, const int64_t* stride_t, int32_t n_states,
                     int32_t dtype, const float* weights, int32_t B, int32_t T, int32_t D, int32_t subsampling, int32_t T_out,
                     void* out, int32_t out_dtype, int64_t out_stride_b, int64_t out_stride_t, float add, float eps,
                     void* stream) {
  if (!states || !stride_b || !stride_t || !weights || !out || n_states < 1 || n_states > DIAR_MAX_STATES || B < 1 ||
      B > 65535 || T < 1 || D < 1 || subsampling < 1 || T_out < 1 || !diar_dt_ok(dtype) || !diar_dt_ok(out_dtype) ||
      out_stride_t < D)
    return WL_EINVAL;
  DiarStates S;
  for (int l = 0; l < n_states; ++l) {
    if (!states[l] || stride_t[l] < D) return WL_EINVAL;
    S.p[l] = states[l]; S.sb[l] = stride_b[l]; S.st[l] = stride_t[l];
  }
  for (int l = n_states; l < DIAR_MAX_STATES; ++l) { S.p[l] = nullptr; S.sb[l] = 0; S.st[l] = 0; }
  const int slab_T = T < FR_SLAB_T ? T : FR_SLAB_T;
  const size_t smem = (size_t)slab_T * FR_CS * sizeof(float);
  // set on every such call: the attribute is per device, and a flag kept here would be neither per device nor thread-safe
  if (smem > 48 * 1024 &&
      hipFuncSetAttribute((const void*)diar_front_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)(FR_SLAB_T * FR_CS * sizeof(float))) != hipSuccess)
    return WL_ELAUNCH;
  WL_LAUNCH(diar_front_kernel, dim3((D + FR_CS - 1) / FR_CS, B), dim3(FR_NT), smem, (hipStream_t)stream, S, (int)n_states,
            (int)dtype, weights, (int)T, (int)D, (int)subsampling, (int)T_out, out, (int)out_dtype, out_stride_b, out_stride_t,
            add, eps, slab_T);
  return wl_check_launch();
}

int wavlm_attn_plain_fwd(const void* qkv, void* O, int32_t B, int32_t H, int32_t T, int32_t head_dim, int32_t dtype,
                         float scale, void* stream) {
  if (!qkv || !O || qkv == O || B < 1 || H < 1 || T < 1 || head_dim != AP_DK || (int64_t)B * H > 65535 || !diar_dt_ok(dtype) ||
      ((uintptr_t)qkv & 15) || ((uintptr_t)O & 15))
    return WL_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == WL_BF16)
    WL_LAUNCH(attn_plain_bf16_kernel, dim3((T + APM_Q - 1) / APM_Q, B * H), dim3(APM_NT), 0, st, (const bf16_t*)qkv, (bf16_t*)O,
              (int)T, (int)H, scale);
  else
    WL_LAUNCH(attn_plain_f32_kernel, dim3((T + APF_Q - 1) / APF_Q, B * H), dim3(APF_Q), 0, st, (const float*)qkv, (float*)O,
              (int)T, (int)H, scale);
  return wl_check_launch();
}

int wavlm_diar_estimate(const void* z, int32_t z_dtype, int64_t z_stride_b, int64_t ldz, int32_t B, int32_t T, int32_t S,
                        int32_t E, float* activities, void* vectors, int32_t v_dtype, void* stream) {
  if (!z || !activities || !vectors || B < 1 || B > 65535 || T < 1 || S < 1 || S > 65535 || E < 1 || E > 64 * EST_MAXV ||
      ldz < (int64_t)S + (int64_t)S * E || !diar_dt_ok(z_dtype) || !diar_dt_ok(v_dtype))
    return WL_EINVAL;
  WL_LAUNCH(diar_estimate_kernel, dim3(S, B), dim3(EST_NT), (size_t)EST_NW * E * sizeof(float), (hipStream_t)stream, z,
            (int)z_dtype, z_stride_b, ldz, (int)T, (int)S, (int)E, activities, vectors, (int)v_dtype);
  return wl_check_launch();
}

}  // extern "C"
