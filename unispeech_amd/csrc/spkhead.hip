// Speaker-embedding head (ECAPA-TDNN over the upstream's layer states) on the device: the inference path of the reference's
// downstreams/speaker_verification/models/ecapa_tdnn.py.  The k = 5 and 1x1 convolutions are wavlm_gemm calls (host side,
// unispeech_amd/speaker.py); this file holds everything between them.
//
// Entry points (include/wavlm_hip.h, "speaker head"):
//   wavlm_spk_mix_norm     x = sum_l w_l h_l + 1e-6, InstanceNorm1d over time (ecapa_tdnn.py:261-270).  One workgroup owns
//                          (utterance, 32-channel slab) over all of T' and keeps the mixed slab in LDS as fp32: every state
//                          is read ONCE, the result written once.  Frames beyond the 1024 the slab holds (20.5 s) are mixed
//                          again in the variance and the write pass (three reads of those frames only).
//                          A single state (the fbank front end's log-mel features, unispeech_amd/fbank.py) is summed about
//                          its first frame: a constant column normalises to exactly zero.
//   wavlm_spk_rowact       y = act(x) * scale + shift per channel (ReLU then BatchNorm's affine: Conv1dReluBn, :63-64; plain
//                          ReLU, :282; tanh, :154), absent frames zeroed, and optionally the time mean of y over the valid
//                          frames (SE_Connect's x.mean(dim=2), :78) from the same pass: a workgroup owns (utterance, 64
//                          channels) over all frames, so the mean needs neither a pass of its own nor atomics.
//   wavlm_spk_res2         Res2Conv1dReluBn (:34-50) in ONE launch: seven dependent dilated 64 -> 64 convolutions with the
//                          running add, ReLU and the BatchNorm affine, the eighth split copied.  A workgroup owns 128 output
//                          frames of one utterance plus a halo of 7 * dilation frames per side which it recomputes (the
//                          receptive field of the chain); the running tensor lives in LDS, fp32.  Halo recomputation (44 %
//                          more arithmetic at dilation 4) was chosen over walking the chain split by split across a whole
//                          utterance because the latter leaves B workgroups for 256 CUs.  bf16 input: each step is a
//                          [frames x 192] x [192 x 64] product on v_mfma_f32_32x32x16_bf16 -- the running tensor is rounded
//                          to bf16 only as the MFMA operand (accumulation, running add, ReLU and affine stay fp32); fp32
//                          input (the parity mode): fp32 FMA throughout.
//   wavlm_spk_se_residual  SE_Connect (:77-83) + the block's residual add (:125): gate = sigmoid(W2 relu(W1 mean + b1) + b2)
//                          per utterance (one small launch), then out = x * gate + residual.
//   wavlm_spk_asp          AttentiveStatsPool (:156-160) after the two 1x1 projections: online softmax over time per
//                          (utterance, channel) with the weighted first and second moments carried along -- one pass over x
//                          and the logits, alpha is never written -- then BatchNorm's affine (:283).
// Arithmetic is fp32 everywhere (loads convert bf16) but for the bf16 MFMA operands of the Res2 chain; nothing is reduced
// across workgroups, so results are bitwise reproducible.
#include "common.hpp"
#include "tile_loaders.hpp"
#include "../../include/wavlm_hip.h"

#include <math.h>

namespace {

constexpr int SPK_MAX_STATES = 32;
constexpr int MIX_CS = 32;          // channels per workgroup
constexpr int MIX_NT = 512;
constexpr int MIX_SLAB_T = 1024;    // frames of the mixed slab kept in LDS (128 KiB)

struct SpkStates {
  const void* p[SPK_MAX_STATES];
  int64_t sb[SPK_MAX_STATES];
  int64_t st[SPK_MAX_STATES];
};

__device__ __forceinline__ int spk_len(const int* lengths, int b, int T) {
  if (!lengths) return T;
  const int l = lengths[b];
  return l < 0 ? 0 : (l > T ? T : l);
}

// ------------------------------------------------------------------------------------------- layer mix + instance norm
template <int V>
__device__ __forceinline__ void mix_at(const SpkStates& S, int n, int dt, const float* ws, int64_t b, int64_t t, int c,
                                       float add, float (&m)[V]) {
#pragma unroll
  for (int j = 0; j < V; ++j) m[j] = 0.f;
  for (int l = 0; l < n; ++l) {
    const int64_t off = b * S.sb[l] + t * S.st[l] + c;
    const float w = ws[l];
    if (V == 2) {
      if (dt == WL_F32) {
        const float2 v = *(const float2*)((const float*)S.p[l] + off);
        m[0] = fmaf(w, v.x, m[0]); m[V - 1] = fmaf(w, v.y, m[V - 1]);
      } else {
        const unsigned u = *(const unsigned*)((const bf16_t*)S.p[l] + off);
        m[0] = fmaf(w, __uint_as_float(u << 16), m[0]); m[V - 1] = fmaf(w, __uint_as_float(u & 0xffff0000u), m[V - 1]);
      }
    } else {
      m[0] = fmaf(w, ld_elem(S.p[l], off, dt), m[0]);
    }
  }
#pragma unroll
  for (int j = 0; j < V; ++j) m[j] += add;
}

// sum over the phases of one channel, in phase order, by every thread of that channel (identical in all of them)
template <int V, int PH>
__device__ __forceinline__ void mix_reduce(float* red, int cl, int ph, float (&v)[V]) {
  __syncthreads();
#pragma unroll
  for (int j = 0; j < V; ++j) red[ph * MIX_CS + cl + j] = v[j];
  __syncthreads();
#pragma unroll
  for (int j = 0; j < V; ++j) {
    float s = 0.f;
    for (int p = 0; p < PH; ++p) s += red[p * MIX_CS + cl + j];
    v[j] = s;
  }
}

template <int V>
__global__ __launch_bounds__(MIX_NT) void spk_mix_norm_kernel(SpkStates S, int n, int dt, const float* __restrict__ w,
                                                              const int* __restrict__ lengths, int T, int D, void* out,
                                                              int odt, int64_t osb, int64_t ost, int pad, float add,
                                                              float eps, int slab_T) {
  extern __shared__ float slab[];  // [slab_T][MIX_CS]
  constexpr int LPR = MIX_CS / V, PH = MIX_NT / LPR;
  __shared__ float red[PH * MIX_CS];
  __shared__ float ws[SPK_MAX_STATES];
  const int tid = threadIdx.x, cl = (tid % LPR) * V, ph = tid / LPR;
  const int b = blockIdx.y, c = blockIdx.x * MIX_CS + cl;
  const bool cin = c < D;  // V == 2: D is even, so a pair is inside or outside as a whole
  const int len = spk_len(lengths, b, T);
  if (tid < n) ws[tid] = w[tid];
  __syncthreads();

  // One state (a feature front end: log-mel columns) is summed about the column's first frame, so a constant column -- digital
  // silence, an empty mel filter -- has mean = its value and normalises to exactly 0.  Several states: the pivot is 0 and the
  // sums are the plain ones, bit for bit.
  float sum[V], m[V], piv[V];
#pragma unroll
  for (int j = 0; j < V; ++j) { sum[j] = 0.f; piv[j] = 0.f; }
  if (n == 1 && cin && len > 0) mix_at<V>(S, n, dt, ws, b, 0, c, add, piv);
  if (cin)
    for (int t = ph; t < len; t += PH) {
      mix_at<V>(S, n, dt, ws, b, t, c, add, m);
#pragma unroll
      for (int j = 0; j < V; ++j) {
        if (t < slab_T) slab[t * MIX_CS + cl + j] = m[j];
        sum[j] += m[j] - piv[j];
      }
    }
  mix_reduce<V, PH>(red, cl, ph, sum);
  const float inv_n = len > 0 ? 1.f / (float)len : 0.f;
  float mean[V], sq[V];
#pragma unroll
  for (int j = 0; j < V; ++j) { mean[j] = piv[j] + sum[j] * inv_n; sq[j] = 0.f; }
  if (cin)
    for (int t = ph; t < len; t += PH) {
      if (t < slab_T) {
#pragma unroll
        for (int j = 0; j < V; ++j) m[j] = slab[t * MIX_CS + cl + j];
      } else {
        mix_at<V>(S, n, dt, ws, b, t, c, add, m);
      }
#pragma unroll
      for (int j = 0; j < V; ++j) { const float d = m[j] - mean[j]; sq[j] = fmaf(d, d, sq[j]); }
    }
  mix_reduce<V, PH>(red, cl, ph, sq);
  float rstd[V];
#pragma unroll
  for (int j = 0; j < V; ++j) rstd[j] = 1.f / sqrtf(sq[j] * inv_n + eps);
  if (!cin) return;
  for (int t = ph - pad; t < T + pad; t += PH) {
    float y[V];
    if (t >= 0 && t < len) {
      if (t < slab_T) {
#pragma unroll
        for (int j = 0; j < V; ++j) m[j] = slab[t * MIX_CS + cl + j];
      } else {
        mix_at<V>(S, n, dt, ws, b, t, c, add, m);
      }
#pragma unroll
      for (int j = 0; j < V; ++j) y[j] = (m[j] - mean[j]) * rstd[j];
    } else {
#pragma unroll
      for (int j = 0; j < V; ++j) y[j] = 0.f;
    }
    const int64_t o = (int64_t)b * osb + (int64_t)t * ost + c;
#pragma unroll
    for (int j = 0; j < V; ++j) st_elem(out, o + j, odt, y[j]);
  }
}

// ------------------------------------------------------------------------------------------------------- row activation
__device__ __forceinline__ float spk_act(float v, int act) {
  if (act == 0) return fmaxf(v, 0.f);
  if (act == 1) return tanhf(v);
  return v;
}

// grid (ceil(C / 64), B, Z): thread (channel, phase of 4); Z > 1 (time chunks) only without mean_out
__global__ __launch_bounds__(256) void spk_rowact_kernel(const void* x, int xdt, int64_t sbx, int64_t ldx, void* y, int ydt,
                                                         int64_t sby, int64_t ldy, int T, int C, int act,
                                                         const float* __restrict__ scale, const float* __restrict__ shift,
                                                         const int* __restrict__ lengths, float* __restrict__ mean_out) {
  __shared__ float red[256];
  const int tid = threadIdx.x, cl = tid & 63, ph = tid >> 6;
  const int b = blockIdx.y, c = blockIdx.x * 64 + cl;
  const int len = spk_len(lengths, b, T);
  const int chunk = (T + gridDim.z - 1) / gridDim.z;
  const int tb = blockIdx.z * chunk, te = min(T, tb + chunk);
  float sum = 0.f;
  if (c < C) {
    const float sc = scale ? scale[c] : 1.f, sh = shift ? shift[c] : 0.f;
    for (int t = tb + ph; t < te; t += 4) {
      float v = 0.f;
      if (t < len) {
        v = fmaf(spk_act(ld_elem(x, (int64_t)b * sbx + (int64_t)t * ldx + c, xdt), act), sc, sh);
        sum += v;
      }
      st_elem(y, (int64_t)b * sby + (int64_t)t * ldy + c, ydt, v);
    }
  }
  if (!mean_out) return;
  red[tid] = sum;
  __syncthreads();
  if (ph == 0 && c < C) {
    const float s = (red[cl] + red[64 + cl]) + (red[128 + cl] + red[192 + cl]);
    mean_out[(int64_t)b * C + c] = len > 0 ? s / (float)len : 0.f;
  }
}

// ------------------------------------------------------------------------------------------------------------ Res2 chain
constexpr int R2_W = 64;      // channels per split (512 / scale 8)
constexpr int R2_NUMS = 7;    // convolutions in the chain
constexpr int R2_TT = 128;    // output frames per workgroup
constexpr int R2_NT = 512;    // 8 waves: wave g owns frames, lane owns the output channel
constexpr int R2_FR = 8;      // frames per thread and round
constexpr int R2_SLD = 68;    // LDS row stride in floats (16-byte aligned rows)
constexpr int R2_PADR = 4;    // zero rows on each side of the region (largest dilation)

__host__ __device__ inline int r2_rows(int dil) { return (R2_TT + 2 * R2_NUMS * dil + R2_FR - 1) / R2_FR * R2_FR; }
__host__ inline size_t r2_smem(int dil) {
  return ((size_t)2 * (r2_rows(dil) + 2 * R2_PADR) * R2_SLD + (size_t)3 * R2_W * R2_W) * sizeof(float);
}

// Wimg fp32 [7][3 taps][64 in][64 out]; bias / scale / shift fp32 [7][64]
__global__ __launch_bounds__(R2_NT) void spk_res2_kernel(const void* X, int xdt, int64_t sbx, int64_t ldx, void* Y, int ydt,
                                                         int64_t sby, int64_t ldy, int T, int dil,
                                                         const float* __restrict__ Wimg, const float* __restrict__ bias,
                                                         const float* __restrict__ scale, const float* __restrict__ shift,
                                                         const int* __restrict__ lengths) {
  extern __shared__ float smem[];
  const int H = R2_NUMS * dil, R = R2_TT + 2 * H, Rp = r2_rows(dil), rows = Rp + 2 * R2_PADR;
  float* Sa = smem + R2_PADR * R2_SLD;                 // row r of the region at Sa[r * R2_SLD], r in [-4, Rp + 4)
  float* Sb = Sa + (size_t)rows * R2_SLD;
  float* Wl = smem + (size_t)2 * rows * R2_SLD;
  const int tid = threadIdx.x, co = tid & 63, g = tid >> 6;
  const int b = blockIdx.y;
  const int t0 = blockIdx.x * R2_TT - H;               // frame of region row 0
  const int len = spk_len(lengths, b, T);
  const int64_t xb = (int64_t)b * sbx, yb = (int64_t)b * sby;

  for (int e = tid; e < 2 * rows * R2_SLD; e += R2_NT) smem[e] = 0.f;
  __syncthreads();
  for (int r = g; r < R; r += R2_NT / 64) {
    const int t = t0 + r;
    if (t >= 0 && t < len) Sa[r * R2_SLD + co] = ld_elem(X, xb + (int64_t)t * ldx + co, xdt);
  }
  // eighth split: passed through
  for (int r = H + g; r < H + R2_TT; r += R2_NT / 64) {
    const int t = t0 + r;
    if (t < T)
      st_elem(Y, yb + (int64_t)t * ldy + R2_NUMS * R2_W + co, ydt,
              t < len ? ld_elem(X, xb + (int64_t)t * ldx + R2_NUMS * R2_W + co, xdt) : 0.f);
  }

  float* Sin = Sa;
  float* Sout = Sb;
  for (int i = 0; i < R2_NUMS; ++i) {
    __syncthreads();  // the previous step's reads of Wl and Sout are done
    for (int e = tid; e < 3 * R2_W * R2_W; e += R2_NT) Wl[e] = Wimg[(size_t)i * 3 * R2_W * R2_W + e];
    __syncthreads();
    const float bi = bias[i * R2_W + co], sc = scale[i * R2_W + co], sh = shift[i * R2_W + co];
    for (int f0 = g * R2_FR; f0 < Rp; f0 += (R2_NT / 64) * R2_FR) {
      float acc[R2_FR];
#pragma unroll
      for (int q = 0; q < R2_FR; ++q) acc[q] = bi;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const float* sp = Sin + (f0 + (k - 1) * dil) * R2_SLD;   // rows -4 .. Rp + 3: inside the zero-padded buffer
        const float* wp = Wl + k * R2_W * R2_W + co;
#pragma unroll 4
        for (int ci = 0; ci < R2_W; ci += 4) {
          const float w0 = wp[(ci + 0) * R2_W], w1 = wp[(ci + 1) * R2_W], w2 = wp[(ci + 2) * R2_W], w3 = wp[(ci + 3) * R2_W];
#pragma unroll
          for (int q = 0; q < R2_FR; ++q) {
            const float4 xv = *(const float4*)(sp + q * R2_SLD + ci);
            acc[q] = fmaf(w0, xv.x, acc[q]);
            acc[q] = fmaf(w1, xv.y, acc[q]);
            acc[q] = fmaf(w2, xv.z, acc[q]);
            acc[q] = fmaf(w3, xv.w, acc[q]);
          }
        }
      }
#pragma unroll
      for (int q = 0; q < R2_FR; ++q) {
        const int f = f0 + q, t = t0 + f;
        const bool valid = f < R && t >= 0 && t < len;
        const float v = valid ? fmaf(fmaxf(acc[q], 0.f), sc, sh) : 0.f;
        if (f >= H && f < H + R2_TT && t < T) st_elem(Y, yb + (int64_t)t * ldy + i * R2_W + co, ydt, v);
        if (i + 1 < R2_NUMS)
          Sout[f * R2_SLD + co] = valid ? v + ld_elem(X, xb + (int64_t)t * ldx + (i + 1) * R2_W + co, xdt) : 0.f;
      }
    }
    float* tmp = Sin; Sin = Sout; Sout = tmp;
  }
}

// ---- bf16 mode: the same tiling, each step on v_mfma_f32_32x32x16_bf16.  Six waves; wave w owns region frames [32 w, 32 w + 32)
// and all 64 output channels (two accumulators).  A operand: lane (row = l & 31, half = l >> 5) reads 8 consecutive input
// channels of frame row + (tap - 1) * dilation from the fp32 running tensor (two 16-byte LDS reads) and rounds them to bf16;
// B operand: 8 consecutive input channels of output channel l & 31 (+ 32) from the step's weights, kept in LDS as bf16
// [tap][out][72] (one 16-byte read).  Accumulator register r of a lane: frame (r & 3) + 8 (r >> 2) + 4 half, channel l & 31.
constexpr int R2M_NT = 384;
constexpr int R2M_WLD = 72;   // bf16 per weight row: 144 bytes, 16-byte aligned

typedef __attribute__((ext_vector_type(16))) float r2_f32x16;
typedef __attribute__((ext_vector_type(4))) unsigned r2_u32x4;

__host__ __device__ inline int r2m_rows(int dil) { return (R2_TT + 2 * R2_NUMS * dil + 31) / 32 * 32; }
__host__ inline size_t r2m_smem(int dil) {
  return (size_t)2 * (r2m_rows(dil) + 2 * R2_PADR) * R2_SLD * sizeof(float) + (size_t)3 * R2_W * R2M_WLD * sizeof(bf16_t);
}

__global__ __launch_bounds__(R2M_NT) void spk_res2_mfma_kernel(const void* X, int xdt, int64_t sbx, int64_t ldx, void* Y, int ydt,
                                                               int64_t sby, int64_t ldy, int T, int dil,
                                                               const float* __restrict__ Wimg, const float* __restrict__ bias,
                                                               const float* __restrict__ scale, const float* __restrict__ shift,
                                                               const int* __restrict__ lengths) {
  extern __shared__ float smem[];
  const int H = R2_NUMS * dil, R = R2_TT + 2 * H, Rm = r2m_rows(dil), rows = Rm + 2 * R2_PADR;
  float* Sa = smem + R2_PADR * R2_SLD;
  float* Sb = Sa + (size_t)rows * R2_SLD;
  bf16_t* Wl = (bf16_t*)(smem + (size_t)2 * rows * R2_SLD);
  const int tid = threadIdx.x, co = tid & 63, g = tid >> 6;   // loads / stores outside the MFMA steps: lane = channel
  const int lane = tid & 63, col = lane & 31, half = lane >> 5;
  const int b = blockIdx.y;
  const int t0 = blockIdx.x * R2_TT - H;
  const int len = spk_len(lengths, b, T);
  const int64_t xb = (int64_t)b * sbx, yb = (int64_t)b * sby;

  for (int e = tid; e < 2 * rows * R2_SLD; e += R2M_NT) smem[e] = 0.f;
  __syncthreads();
  for (int r = g; r < R; r += R2M_NT / 64) {
    const int t = t0 + r;
    if (t >= 0 && t < len) Sa[r * R2_SLD + co] = ld_elem(X, xb + (int64_t)t * ldx + co, xdt);
  }
  for (int r = H + g; r < H + R2_TT; r += R2M_NT / 64) {
    const int t = t0 + r;
    if (t < T)
      st_elem(Y, yb + (int64_t)t * ldy + R2_NUMS * R2_W + co, ydt,
              t < len ? ld_elem(X, xb + (int64_t)t * ldx + R2_NUMS * R2_W + co, xdt) : 0.f);
  }

  float* Sin = Sa;
  float* Sout = Sb;
  for (int i = 0; i < R2_NUMS; ++i) {
    __syncthreads();
    // fp32 image [tap][in][out] -> bf16 [tap][out][in] (the weights of a bf16 model are bf16 values: the conversion is exact)
    for (int e = tid; e < 3 * R2_W * R2_W; e += R2M_NT) {
      const int tap = e >> 12, ci = (e >> 6) & 63, o = e & 63;
      Wl[(tap * R2_W + o) * R2M_WLD + ci] = f2bf(Wimg[(size_t)i * 3 * R2_W * R2_W + e]);
    }
    __syncthreads();
    for (int f0 = g * 32; f0 < Rm; f0 += (R2M_NT / 64) * 32) {
      r2_f32x16 acc0 = {}, acc1 = {};
#pragma unroll
      for (int tap = 0; tap < 3; ++tap) {
        const float* sp = Sin + (f0 + col + (tap - 1) * dil) * R2_SLD + 8 * half;   // rows -4 .. Rm + 3
        const bf16_t* w0 = Wl + (tap * R2_W + col) * R2M_WLD + 8 * half;
        const bf16_t* w1 = w0 + 32 * R2M_WLD;
#pragma unroll
        for (int c = 0; c < R2_W; c += 16) {
          const float4 a0 = *(const float4*)(sp + c), a1 = *(const float4*)(sp + c + 4);
          const r2_u32x4 pa = {pack_bf16x2(a0.x, a0.y), pack_bf16x2(a0.z, a0.w), pack_bf16x2(a1.x, a1.y), pack_bf16x2(a1.z, a1.w)};
          const bf16x8_t A = __builtin_bit_cast(bf16x8_t, pa);
          const bf16x8_t B0 = *(const bf16x8_t*)(w0 + c), B1 = *(const bf16x8_t*)(w1 + c);
          acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A, B0, acc0, 0, 0, 0);
          acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A, B1, acc1, 0, 0, 0);
        }
      }
#pragma unroll
      for (int nb = 0; nb < 2; ++nb) {
        const int oc = nb * 32 + col;
        const float bi = bias[i * R2_W + oc], sc = scale[i * R2_W + oc], sh = shift[i * R2_W + oc];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int f = f0 + (r & 3) + 8 * (r >> 2) + 4 * half, t = t0 + f;
          const bool valid = f < R && t >= 0 && t < len;
          const float a = nb == 0 ? acc0[r] : acc1[r];
          const float v = valid ? fmaf(fmaxf(a + bi, 0.f), sc, sh) : 0.f;
          if (f >= H && f < H + R2_TT && t < T) st_elem(Y, yb + (int64_t)t * ldy + i * R2_W + oc, ydt, v);
          if (i + 1 < R2_NUMS)
            Sout[f * R2_SLD + oc] = valid ? v + ld_elem(X, xb + (int64_t)t * ldx + (i + 1) * R2_W + oc, xdt) : 0.f;
        }
      }
    }
    float* tmp = Sin; Sin = Sout; Sout = tmp;
  }
}

// ------------------------------------------------------------------------------------------------ squeeze-excite + residual
// one workgroup per utterance: hid = relu(W1 mean + b1) [Cb], gate = sigmoid(W2 hid + b2) [C]
__global__ __launch_bounds__(256) void spk_se_gate_kernel(const float* __restrict__ mean, const void* W1, const void* b1,
                                                          const void* W2, const void* b2, int wdt, int C, int Cb,
                                                          float* __restrict__ gate) {
  extern __shared__ float sh[];  // mean [C] + hid [Cb]
  float* mv = sh;
  float* hid = sh + C;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x;
  for (int c = tid; c < C; c += 256) mv[c] = mean[(int64_t)b * C + c];
  __syncthreads();
  for (int j = wave; j < Cb; j += 4) {
    float s = 0.f;
    for (int c = lane; c < C; c += 64) s = fmaf(ld_elem(W1, (int64_t)j * C + c, wdt), mv[c], s);
    s = wave_sum(s);
    if (lane == 0) hid[j] = fmaxf(s + ld_elem(b1, j, wdt), 0.f);
  }
  __syncthreads();
  for (int c = tid; c < C; c += 256) {
    float s = ld_elem(b2, c, wdt);
    for (int j = 0; j < Cb; ++j) s = fmaf(ld_elem(W2, (int64_t)c * Cb + j, wdt), hid[j], s);
    gate[(int64_t)b * C + c] = 1.f / (1.f + expf(-s));
  }
}

// grid (ceil(C / 64), B, Z time chunks)
__global__ __launch_bounds__(256) void spk_se_apply_kernel(const void* x, int xdt, int64_t sbx, int64_t ldx, const void* res,
                                                           int rdt, int64_t sbr, int64_t ldr, void* out, int odt, int64_t sbo,
                                                           int64_t ldo, int T, int C, const float* __restrict__ gate,
                                                           const int* __restrict__ lengths) {
  const int tid = threadIdx.x, cl = tid & 63, ph = tid >> 6;
  const int b = blockIdx.y, c = blockIdx.x * 64 + cl;
  if (c >= C) return;
  const int len = spk_len(lengths, b, T);
  const int chunk = (T + gridDim.z - 1) / gridDim.z;
  const int tb = blockIdx.z * chunk, te = min(T, tb + chunk);
  const float gt = gate[(int64_t)b * C + c];
  for (int t = tb + ph; t < te; t += 4) {
    float v = 0.f;
    if (t < len)
      v = fmaf(ld_elem(x, (int64_t)b * sbx + (int64_t)t * ldx + c, xdt), gt,
               ld_elem(res, (int64_t)b * sbr + (int64_t)t * ldr + c, rdt));
    st_elem(out, (int64_t)b * sbo + (int64_t)t * ldo + c, odt, v);
  }
}

// ------------------------------------------------------------------------------------------- attentive statistics pooling
// grid (ceil(C / 64), B): thread (channel, phase of 4) carries (max, sum e, sum e x, sum e x^2) of its frames
__global__ __launch_bounds__(256) void spk_asp_kernel(const void* x, int xdt, int64_t sbx, int64_t ldx, const void* lg, int ldt,
                                                      int64_t sbl, int64_t ldl, int T, int C,
                                                      const int* __restrict__ lengths, const float* __restrict__ scale,
                                                      const float* __restrict__ shift, float* __restrict__ raw, void* out,
                                                      int odt) {
  __shared__ float rm[256], rs[256], rx[256], rxx[256];
  const int tid = threadIdx.x, cl = tid & 63, ph = tid >> 6;
  const int b = blockIdx.y, c = blockIdx.x * 64 + cl;
  const int len = spk_len(lengths, b, T);
  float m = -INFINITY, s = 0.f, sx = 0.f, sxx = 0.f;
  if (c < C)
    for (int t = ph; t < len; t += 4) {
      const float l = ld_elem(lg, (int64_t)b * sbl + (int64_t)t * ldl + c, ldt);
      const float v = ld_elem(x, (int64_t)b * sbx + (int64_t)t * ldx + c, xdt);
      if (l > m) {
        const float r = expf(m - l);  // exp(-inf) = 0 at the first frame
        s *= r; sx *= r; sxx *= r; m = l;
      }
      const float e = expf(l - m);
      s += e; sx = fmaf(e, v, sx); sxx = fmaf(e * v, v, sxx);
    }
  rm[tid] = m; rs[tid] = s; rx[tid] = sx; rxx[tid] = sxx;
  __syncthreads();
  if (ph != 0 || c >= C) return;
  float M = fmaxf(fmaxf(rm[cl], rm[64 + cl]), fmaxf(rm[128 + cl], rm[192 + cl]));
  float S = 0.f, SX = 0.f, SXX = 0.f;
  for (int p = 0; p < 4; ++p) {
    const float pm = rm[p * 64 + cl];
    const float r = pm == -INFINITY ? 0.f : expf(pm - M);
    S = fmaf(rs[p * 64 + cl], r, S); SX = fmaf(rx[p * 64 + cl], r, SX); SXX = fmaf(rxx[p * 64 + cl], r, SXX);
  }
  const float mean = S > 0.f ? SX / S : 0.f;
  const float ex2 = S > 0.f ? SXX / S : 0.f;
  const float sd = sqrtf(fmaxf(ex2 - mean * mean, 1e-9f));
  const int64_t o = (int64_t)b * 2 * C;
  if (raw) { raw[o + c] = mean; raw[o + C + c] = sd; }
  if (out) {
    st_elem(out, o + c, odt, fmaf(mean, scale ? scale[c] : 1.f, shift ? shift[c] : 0.f));
    st_elem(out, o + C + c, odt, fmaf(sd, scale ? scale[C + c] : 1.f, shift ? shift[C + c] : 0.f));
  }
}

inline bool spk_dt_ok(int dt) { return dt == WL_F32 || dt == WL_BF16; }
inline int spk_zchunks(int T, int wgs) {  // time chunks for the element-wise kernels: aim at ~1024 workgroups
  int z = (1024 + wgs - 1) / wgs, zt = (T + 63) / 64;
  if (z > zt) z = zt;
  return z < 1 ? 1 : (z > 64 ? 64 : z);
}

}  // namespace

extern "C" {

int wavlm_spk_mix_norm(const void* const* states, const int64_t* stride_b, const int64_t* stride_t, int32_t n_states,
                       int32_t dtype, const float* weights, const int32_t* lengths, int32_t B, int32_t T, int32_t D,
                       void* out, int32_t out_dtype, int64_t out_stride_b, int64_t out_stride_t, int32_t pad, float add,
                       float eps, void* stream) {
  if (!states || !stride_b || !stride_t || !weights || !out || n_states < 1 || n_states > SPK_MAX_STATES || B < 1 ||
      B > 65535 || T < 1 || D < 1 || pad < 0 || !spk_dt_ok(dtype) || !spk_dt_ok(out_dtype) || out_stride_t < D)
    return WL_EINVAL;
  SpkStates S;
  const uint64_t es = wl_esize(dtype);
  bool pairs = (D % 2) == 0;
  for (int l = 0; l < n_states; ++l) {
    if (!states[l] || stride_t[l] < D) return WL_EINVAL;
    S.p[l] = states[l]; S.sb[l] = stride_b[l]; S.st[l] = stride_t[l];
    pairs = pairs && ((uintptr_t)states[l] % (2 * es)) == 0 && (stride_b[l] % 2) == 0 && (stride_t[l] % 2) == 0;
  }
  for (int l = n_states; l < SPK_MAX_STATES; ++l) { S.p[l] = nullptr; S.sb[l] = 0; S.st[l] = 0; }
  hipStream_t st = (hipStream_t)stream;
  const int slab_T = T < MIX_SLAB_T ? T : MIX_SLAB_T;
  const size_t smem = (size_t)slab_T * MIX_CS * sizeof(float);
  const dim3 grid((D + MIX_CS - 1) / MIX_CS, B);
  static size_t allowed[2] = {0, 0};
  const void* fn = pairs ? (const void*)spk_mix_norm_kernel<2> : (const void*)spk_mix_norm_kernel<1>;
  if (smem > 48 * 1024 && smem > allowed[pairs]) {
    if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(MIX_SLAB_T * MIX_CS * sizeof(float))) != hipSuccess)
      return WL_ELAUNCH;
    allowed[pairs] = (size_t)MIX_SLAB_T * MIX_CS * sizeof(float);
  }
  if (pairs)
    WL_LAUNCH(spk_mix_norm_kernel<2>, grid, dim3(MIX_NT), smem, st, S, (int)n_states, (int)dtype, weights, (const int*)lengths,
              (int)T, (int)D, out, (int)out_dtype, out_stride_b, out_stride_t, (int)pad, add, eps, slab_T);
  else
    WL_LAUNCH(spk_mix_norm_kernel<1>, grid, dim3(MIX_NT), smem, st, S, (int)n_states, (int)dtype, weights, (const int*)lengths,
              (int)T, (int)D, out, (int)out_dtype, out_stride_b, out_stride_t, (int)pad, add, eps, slab_T);
  return wl_check_launch();
}

int wavlm_spk_rowact(const void* x, int32_t x_dtype, int64_t x_stride_b, int64_t ldx, void* y, int32_t y_dtype,
                     int64_t y_stride_b, int64_t ldy, int32_t B, int32_t T, int32_t C, int32_t act, const float* scale,
                     const float* shift, const int32_t* lengths, float* mean_out, void* stream) {
  if (!x || !y || B < 1 || B > 65535 || T < 1 || C < 1 || ldx < C || ldy < C || act < 0 || act > 2 || !spk_dt_ok(x_dtype) ||
      !spk_dt_ok(y_dtype))
    return WL_EINVAL;
  const int cb = (C + 63) / 64;
  const int z = mean_out ? 1 : spk_zchunks(T, cb * B);
  WL_LAUNCH(spk_rowact_kernel, dim3(cb, B, z), dim3(256), 0, (hipStream_t)stream, x, (int)x_dtype, x_stride_b, ldx, y,
            (int)y_dtype, y_stride_b, ldy, (int)T, (int)C, (int)act, scale, shift, (const int*)lengths, mean_out);
  return wl_check_launch();
}

int wavlm_spk_res2(const void* x, int32_t x_dtype, int64_t x_stride_b, int64_t ldx, void* y, int32_t y_dtype,
                   int64_t y_stride_b, int64_t ldy, int32_t B, int32_t T, int32_t C, int32_t dilation, const float* w_image,
                   const float* bias, const float* scale, const float* shift, const int32_t* lengths, void* stream) {
  if (!x || !y || x == y || !w_image || !bias || !scale || !shift || B < 1 || B > 65535 || T < 1 || C != (R2_NUMS + 1) * R2_W ||
      dilation < 1 || dilation > R2_PADR || ldx < C || ldy < C || !spk_dt_ok(x_dtype) || !spk_dt_ok(y_dtype))
    return WL_EINVAL;
  if (x_dtype == WL_BF16) {   // bf16 mode: the MFMA form
    const size_t smem = r2m_smem(dilation);
    static size_t allowed_m = 0;
    if (smem > allowed_m) {
      if (hipFuncSetAttribute((const void*)spk_res2_mfma_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)r2m_smem(R2_PADR)) != hipSuccess)
        return WL_ELAUNCH;
      allowed_m = r2m_smem(R2_PADR);
    }
    WL_LAUNCH(spk_res2_mfma_kernel, dim3((T + R2_TT - 1) / R2_TT, B), dim3(R2M_NT), smem, (hipStream_t)stream, x, (int)x_dtype,
              x_stride_b, ldx, y, (int)y_dtype, y_stride_b, ldy, (int)T, (int)dilation, w_image, bias, scale, shift,
              (const int*)lengths);
    return wl_check_launch();
  }
  const size_t smem = r2_smem(dilation);
  static size_t allowed = 0;
  if (smem > allowed) {
    if (hipFuncSetAttribute((const void*)spk_res2_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)r2_smem(R2_PADR)) !=
        hipSuccess)
      return WL_ELAUNCH;
    allowed = r2_smem(R2_PADR);
  }
  WL_LAUNCH(spk_res2_kernel, dim3((T + R2_TT - 1) / R2_TT, B), dim3(R2_NT), smem, (hipStream_t)stream, x, (int)x_dtype,
            x_stride_b, ldx, y, (int)y_dtype, y_stride_b, ldy, (int)T, (int)dilation, w_image, bias, scale, shift,
            (const int*)lengths);
  return wl_check_launch();
}

uint64_t wavlm_spk_se_workspace_bytes(int32_t B, int32_t C) {
  if (B < 1 || C < 1) return 0;
  return (uint64_t)B * C * sizeof(float);
}

int wavlm_spk_se_residual(const void* x, int32_t x_dtype, int64_t x_stride_b, int64_t ldx, const float* mean, const void* w1,
                          const void* b1, const void* w2, const void* b2, int32_t w_dtype, const void* res, int32_t res_dtype,
                          int64_t res_stride_b, int64_t ld_res, void* out, int32_t out_dtype, int64_t out_stride_b,
                          int64_t ld_out, int32_t B, int32_t T, int32_t C, int32_t Cb, const int32_t* lengths,
                          void* workspace, uint64_t ws_bytes, void* stream) {
  if (!x || !mean || !w1 || !b1 || !w2 || !b2 || !res || !out || !workspace || B < 1 || B > 65535 || T < 1 || C < 1 ||
      Cb < 1 || ldx < C || ld_res < C || ld_out < C || ws_bytes < wavlm_spk_se_workspace_bytes(B, C) ||
      (size_t)(C + Cb) * sizeof(float) > 48 * 1024 || !spk_dt_ok(x_dtype) || !spk_dt_ok(w_dtype) || !spk_dt_ok(res_dtype) ||
      !spk_dt_ok(out_dtype))
    return WL_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  float* gate = (float*)workspace;
  WL_LAUNCH(spk_se_gate_kernel, dim3(B), dim3(256), (size_t)(C + Cb) * sizeof(float), st, mean, w1, b1, w2, b2, (int)w_dtype,
            (int)C, (int)Cb, gate);
  const int cb = (C + 63) / 64;
  WL_LAUNCH(spk_se_apply_kernel, dim3(cb, B, spk_zchunks(T, cb * B)), dim3(256), 0, st, x, (int)x_dtype, x_stride_b, ldx, res,
            (int)res_dtype, res_stride_b, ld_res, out, (int)out_dtype, out_stride_b, ld_out, (int)T, (int)C, (const float*)gate,
            (const int*)lengths);
  return wl_check_launch();
}

int wavlm_spk_asp(const void* x, int32_t x_dtype, int64_t x_stride_b, int64_t ldx, const void* logits, int32_t l_dtype,
                  int64_t l_stride_b, int64_t ldl, int32_t B, int32_t T, int32_t C, const int32_t* lengths, const float* scale,
                  const float* shift, float* pooled_raw, void* out, int32_t out_dtype, void* stream) {
  if (!x || !logits || (!pooled_raw && !out) || B < 1 || B > 65535 || T < 1 || C < 1 || ldx < C || ldl < C ||
      !spk_dt_ok(x_dtype) || !spk_dt_ok(l_dtype) || (out && !spk_dt_ok(out_dtype)))
    return WL_EINVAL;
  WL_LAUNCH(spk_asp_kernel, dim3((C + 63) / 64, B), dim3(256), 0, (hipStream_t)stream, x, (int)x_dtype, x_stride_b, ldx, logits,
            (int)l_dtype, l_stride_b, ldl, (int)T, (int)C, (const int*)lengths, scale, shift, pooled_raw, out, (int)out_dtype);
  return wl_check_launch();
}

}  // extern "C"
