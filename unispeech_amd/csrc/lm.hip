// Transformer language model on the device: the two steps of an inference pass that had no kernel (the rest of a layer is
// wavlm_gemm / wavlm_layernorm_fwd / wavlm_act_fwd calls, unispeech_amd/transformer_lm.py).
//
// Entry points (include/wavlm_hip.h, "Transformer LM"):
//   wavlm_lm_logprob       the output layer of the reference's TransformerDecoder (src/fairseq/models/transformer.py:965-971,
//                          one bias-free Linear onto the vocabulary) fused with log_softmax and the gather of the target's
//                          entry (examples/speech_recognition/w2l_decoder.py:366-383): z[r, :] = W x_r is never stored.  A
//                          workgroup owns 128 rows and one slab of LM_SLAB vocabulary entries, walks the slab in tiles of 128
//                          entries, and keeps per row a running maximum, a running sum of exp and the target's logit -- an
//                          online softmax over the vocabulary.  bf16: z^T = W X^T on v_mfma_f32_32x32x16_bf16, so a row of X
//                          sits on the lane, its 128 logits of a tile in that lane's accumulators (two half-waves share a row),
//                          and the softmax state is per lane; the target's logit is read from that same accumulator.  fp32
//                          (parity mode): one thread per row, fp32 FMA in k order.  Each (slab, row) leaves (max, sum, target
//                          logit) in the workspace; a second launch folds a row's slabs in slab order.  The slab boundaries
//                          depend on V alone, nothing is reduced with atomics, and the columns of an MFMA do not mix: results
//                          are bitwise reproducible and a row's result depends neither on R nor on the row's position.
//   wavlm_attn_causal_fwd  the decoder's self-attention (src/fairseq/modules/transformer_layer.py:349-357 under
//                          buffered_future_mask, transformer.py:979-991) from the packed q|k|v layout of wavlm_attn_plain_fwd:
//                          query t attends keys 0..t of its own sequence, rows at or beyond lengths[b] are written as zeros and
//                          never read.  The structure is csrc/diar.hip's plain attention (S^T = K Q^T, O^T = V^T P^T, the query
//                          on the lane, P from accumulator to operand in registers) with heads 32 or 64 wide; key tiles above a
//                          workgroup's last query, and 32-key steps above a wave's last query, are skipped, not masked.
#include "common.hpp"
#include "tile_loaders.hpp"
#include "../../include/wavlm_hip.h"

#include <math.h>

namespace {

typedef __attribute__((ext_vector_type(16))) float lm_f32x16;

inline bool lm_dt_ok(int dt) { return dt == WL_F32 || dt == WL_BF16; }

// ------------------------------------------------------------------------------------------------ vocabulary log-probs
constexpr int LM_SLAB = 2048;          // vocabulary entries per slab: a function of nothing, so slabs depend on V alone
constexpr int LM_BM = 128;             // rows per workgroup
constexpr int LM_NT = 256;             // bf16: 4 waves, wave w owns rows [32 w, 32 w + 32) of the workgroup's 128
constexpr int LM_BN = 128;             // bf16: vocabulary entries per tile (four 32-entry MFMA tiles per wave)
constexpr int LM_BK = 64;              // bf16: k per LDS stage
constexpr int LM_LD = LM_BK + 8;       // bf16 per LDS row: 144 bytes, 16-byte aligned
constexpr int LMF_NT = 128;            // fp32: one thread per row
constexpr int LMF_BN = 32;             // fp32: vocabulary entries per tile
constexpr int LMF_BK = 32;
constexpr int LMF_XLD = LM_BM + 1;     // Xs[k][row]
constexpr int LMF_WLD = LMF_BN + 4;    // Ws[k][entry], rows 16-byte aligned

inline int64_t lm_slabs(int64_t V) { return (V + LM_SLAB - 1) / LM_SLAB; }
inline int64_t lm_row_blocks(int64_t R) { return (R + LM_BM - 1) / LM_BM; }

// grid: slab * row_blocks + row_block (the row blocks of one slab run together: its 2048 x D weights stay in L2)
__global__ __launch_bounds__(LM_NT) void lm_logprob_bf16_kernel(const bf16_t* __restrict__ X, int64_t ldx,
                                                                const bf16_t* __restrict__ W, int64_t ldw,
                                                                const int* __restrict__ target, int64_t R, int D, int V,
                                                                int nrb, float* __restrict__ ws_m, float* __restrict__ ws_l,
                                                                float* __restrict__ ws_t) {
  __shared__ __attribute__((aligned(16))) bf16_t Xs[LM_BM * LM_LD];
  __shared__ __attribute__((aligned(16))) bf16_t Ws[LM_BN * LM_LD];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int r = lane & 31, hi = lane >> 5;
  const int slab = blockIdx.x / nrb;
  const int64_t row0 = (int64_t)(blockIdx.x % nrb) * LM_BM;
  const int v_begin = slab * LM_SLAB;
  const int v_end = V - v_begin < LM_SLAB ? V : v_begin + LM_SLAB;
  const int64_t myrow = row0 + wv * 32 + r;
  const int tgt = myrow < R ? target[myrow] : -1;
  const int nk = (D + LM_BK - 1) / LM_BK;
  const int total = ((v_end - v_begin + LM_BN - 1) / LM_BN) * nk;

  // stage `it` = (tile it / nk, k step it % nk): thread tid moves 16-byte chunks tid + 256 i of the X and of the W tile
  uint4 xg[4], wg[4];
  auto gload = [&](int it) {
    const int v0 = v_begin + (it / nk) * LM_BN, k0 = (it % nk) * LM_BK;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int e = tid + LM_NT * i, rr = e >> 3, c = (e & 7) * 8;
      xg[i] = make_uint4(0u, 0u, 0u, 0u);
      wg[i] = xg[i];
      if (k0 + c < D) {                       // D % 8 == 0: a chunk is inside the row or beyond it
        if (row0 + rr < R) xg[i] = *(const uint4*)(X + (row0 + rr) * ldx + k0 + c);
        if ((int64_t)v0 + rr < v_end) wg[i] = *(const uint4*)(W + ((int64_t)v0 + rr) * ldw + k0 + c);
      }
    }
  };

  lm_f32x16 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[j][i] = 0.f;
  float m = -INFINITY, l = 0.f, tz = -INFINITY;   // l: this half-wave's part of the row's sum

  gload(0);
  for (int it = 0; it < total; ++it) {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int e = tid + LM_NT * i, rr = e >> 3, c = (e & 7) * 8;
      *(uint4*)(Xs + rr * LM_LD + c) = xg[i];
      *(uint4*)(Ws + rr * LM_LD + c) = wg[i];
    }
    __syncthreads();
    if (it + 1 < total) gload(it + 1);        // in flight under this stage's MFMAs
    const int k0 = (it % nk) * LM_BK;
#pragma unroll
    for (int s = 0; s < LM_BK / 16; ++s) {
      if (k0 + 16 * s >= D) break;            // uniform; a partial step reads the zero fill
      U4 xb; xb.v = *(const uint4*)(Xs + (wv * 32 + r) * LM_LD + 16 * s + 8 * hi);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        U4 a; a.v = *(const uint4*)(Ws + (j * 32 + r) * LM_LD + 16 * s + 8 * hi);
        acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.b, xb.b, acc[j], 0, 0, 0);
      }
    }
    if (it % nk != nk - 1) continue;
    // acc[j][i]: entry v0 + 32 j + (i & 3) + 8 (i >> 2) + 4 hi of row wv * 32 + r
    const int v0 = v_begin + (it / nk) * LM_BN;
    float cm = -INFINITY;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const unsigned v = (unsigned)v0 + 32 * j + (i & 3) + 8 * (i >> 2) + 4 * hi;   // unsigned: V may be close to 2^31
        const float z = v < (unsigned)v_end ? acc[j][i] : -INFINITY;
        if (v == (unsigned)tgt) tz = z;
        acc[j][i] = z;
        cm = fmaxf(cm, z);
      }
    cm = wl_max_xor32(cm);                    // entry v0 exists: finite
    const float mn = fmaxf(m, cm);
    l *= __expf(m - mn);                      // exp(-inf) = 0 at the first tile
    m = mn;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        l += __expf(acc[j][i] - mn);
        acc[j][i] = 0.f;
      }
  }
  l = wl_sum_xor32(l);
  tz = wl_max_xor32(tz);                      // at most one half holds it
  if (hi == 0 && myrow < R) {
    const int64_t o = (int64_t)slab * R + myrow;
    ws_m[o] = m; ws_l[o] = l; ws_t[o] = tz;
  }
}

__global__ __launch_bounds__(LMF_NT) void lm_logprob_f32_kernel(const float* __restrict__ X, int64_t ldx,
                                                                const float* __restrict__ W, int64_t ldw,
                                                                const int* __restrict__ target, int64_t R, int D, int V,
                                                                int nrb, float* __restrict__ ws_m, float* __restrict__ ws_l,
                                                                float* __restrict__ ws_t) {
  __shared__ float Xs[LMF_BK * LMF_XLD];
  __shared__ __attribute__((aligned(16))) float Ws[LMF_BK * LMF_WLD];
  const int tid = threadIdx.x;
  const int slab = blockIdx.x / nrb;
  const int64_t row0 = (int64_t)(blockIdx.x % nrb) * LM_BM;
  const int v_begin = slab * LM_SLAB;
  const int v_end = V - v_begin < LM_SLAB ? V : v_begin + LM_SLAB;
  const int64_t myrow = row0 + tid;
  const int tgt = myrow < R ? target[myrow] : -1;
  float m = -INFINITY, l = 0.f, tz = -INFINITY;
  for (int64_t v0 = v_begin; v0 < v_end; v0 += LMF_BN) {
    float acc[LMF_BN];
#pragma unroll
    for (int v = 0; v < LMF_BN; ++v) acc[v] = 0.f;
    for (int k0 = 0; k0 < D; k0 += LMF_BK) {
      const int kn = D - k0 < LMF_BK ? D - k0 : LMF_BK;
      __syncthreads();
      for (int e = tid; e < LM_BM * LMF_BK; e += LMF_NT) {
        const int rr = e / LMF_BK, kk = e % LMF_BK;
        Xs[kk * LMF_XLD + rr] = (kk < kn && row0 + rr < R) ? X[(row0 + rr) * ldx + k0 + kk] : 0.f;
      }
      for (int e = tid; e < LMF_BN * LMF_BK; e += LMF_NT) {
        const int vv = e / LMF_BK, kk = e % LMF_BK;
        Ws[kk * LMF_WLD + vv] = (kk < kn && v0 + vv < v_end) ? W[(v0 + vv) * ldw + k0 + kk] : 0.f;
      }
      __syncthreads();
      for (int kk = 0; kk < kn; ++kk) {
        const float x = Xs[kk * LMF_XLD + tid];
#pragma unroll
        for (int v4 = 0; v4 < LMF_BN / 4; ++v4) {
          const float4 w = *(const float4*)(Ws + kk * LMF_WLD + 4 * v4);
          acc[4 * v4] = fmaf(x, w.x, acc[4 * v4]);
          acc[4 * v4 + 1] = fmaf(x, w.y, acc[4 * v4 + 1]);
          acc[4 * v4 + 2] = fmaf(x, w.z, acc[4 * v4 + 2]);
          acc[4 * v4 + 3] = fmaf(x, w.w, acc[4 * v4 + 3]);
        }
      }
    }
    float cm = -INFINITY;
#pragma unroll
    for (int v = 0; v < LMF_BN; ++v) {
      const float z = v0 + v < v_end ? acc[v] : -INFINITY;
      if (v0 + v == tgt) tz = z;
      acc[v] = z;
      cm = fmaxf(cm, z);
    }
    const float mn = fmaxf(m, cm);
    l *= expf(m - mn);
    m = mn;
#pragma unroll
    for (int v = 0; v < LMF_BN; ++v) l += expf(acc[v] - mn);
  }
  if (myrow < R) {
    const int64_t o = (int64_t)slab * R + myrow;
    ws_m[o] = m; ws_l[o] = l; ws_t[o] = tz;
  }
}

// one thread per row: its slabs in slab order
__global__ __launch_bounds__(256) void lm_logprob_combine_kernel(const float* __restrict__ ws_m, const float* __restrict__ ws_l,
                                                                 const float* __restrict__ ws_t,
                                                                 const int* __restrict__ target, int64_t R, int V, int nslab,
                                                                 float* __restrict__ logprob, float* __restrict__ lse) {
  const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (row >= R) return;
  float M = -INFINITY;
  for (int s = 0; s < nslab; ++s) M = fmaxf(M, ws_m[(int64_t)s * R + row]);
  float L = 0.f;
  for (int s = 0; s < nslab; ++s) L += ws_l[(int64_t)s * R + row] * expf(ws_m[(int64_t)s * R + row] - M);
  const float ls = M + logf(L);
  if (lse) lse[row] = ls;
  const int tgt = target[row];
  float lp;
  if (tgt < 0) lp = 0.f;
  else if (tgt >= V) lp = __builtin_nanf("");
  else lp = ws_t[(int64_t)(tgt / LM_SLAB) * R + row] - ls;
  logprob[row] = lp;
}

// ---------------------------------------------------------------------------------------------------- causal attention
// fp32: grid (ceil(T / 128), B * H); one thread per query, K / V tiles of 64 keys in LDS (broadcast reads)
constexpr int ACF_Q = 128;
constexpr int ACF_KT = 64;

template <int DK>
__global__ __launch_bounds__(ACF_Q) void attn_causal_f32_kernel(const float* __restrict__ qkv, float* __restrict__ O,
                                                                const int* __restrict__ lengths, int T, int H, float scale) {
  __shared__ float4 Ks[ACF_KT][DK / 4];
  __shared__ float4 Vs[ACF_KT][DK / 4];
  const int tid = threadIdx.x;
  const int b = blockIdx.y / H, h = blockIdx.y % H;
  int L = lengths ? lengths[b] : T;
  L = L < 0 ? 0 : (L > T ? T : L);
  const int64_t ld = (int64_t)3 * H * DK;
  const float* base = qkv + (int64_t)b * T * ld + h * DK;
  const int q0 = blockIdx.x * ACF_Q;
  const int q = q0 + tid;
  const int qr = q < T ? q : T - 1;
  float4 qv[DK / 4], o[DK / 4];
#pragma unroll
  for (int i = 0; i < DK / 4; ++i) {
    qv[i] = *(const float4*)(base + (int64_t)qr * ld + 4 * i);
    o[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  float m = -INFINITY, l = 0.f;
  const int kend = q0 + ACF_Q < L ? q0 + ACF_Q : L;      // keys beyond the workgroup's last query are not visited
  for (int k0 = 0; k0 < kend; k0 += ACF_KT) {
    const int kn = kend - k0 < ACF_KT ? kend - k0 : ACF_KT;
    __syncthreads();
    for (int e = tid; e < ACF_KT * (DK / 4); e += ACF_Q) {
      const int r = e / (DK / 4), c4 = e % (DK / 4);
      float4 kv = make_float4(0.f, 0.f, 0.f, 0.f), vv = kv;
      if (r < kn) {
        const float* row = base + (int64_t)(k0 + r) * ld + 4 * c4;
        kv = *(const float4*)(row + H * DK);
        vv = *(const float4*)(row + 2 * H * DK);
      }
      Ks[r][c4] = kv; Vs[r][c4] = vv;
    }
    __syncthreads();
    for (int kk = 0; kk < kn; kk += 8) {
      if (k0 + kk > qr) break;                // every key of this and the later chunks is above the diagonal
      float s[8];
      float cm = -INFINITY;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float d = 0.f;
#pragma unroll
        for (int i = 0; i < DK / 4; ++i) {
          const float4 kv = Ks[kk + j][i];
          d = fmaf(qv[i].x, kv.x, d); d = fmaf(qv[i].y, kv.y, d); d = fmaf(qv[i].z, kv.z, d); d = fmaf(qv[i].w, kv.w, d);
        }
        s[j] = (kk + j < kn && k0 + kk + j <= qr) ? d * scale : -INFINITY;
        cm = fmaxf(cm, s[j]);
      }
      const float mn = fmaxf(m, cm);          // finite: key k0 + kk <= qr exists
      const float r = expf(m - mn);           // exp(-inf) = 0 at the first chunk
      l *= r;
#pragma unroll
      for (int i = 0; i < DK / 4; ++i) { o[i].x *= r; o[i].y *= r; o[i].z *= r; o[i].w *= r; }
      m = mn;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float p = expf(s[j] - mn);
        l += p;
#pragma unroll
        for (int i = 0; i < DK / 4; ++i) {
          const float4 vv = Vs[kk + j][i];
          o[i].x = fmaf(p, vv.x, o[i].x); o[i].y = fmaf(p, vv.y, o[i].y); o[i].z = fmaf(p, vv.z, o[i].z);
          o[i].w = fmaf(p, vv.w, o[i].w);
        }
      }
    }
  }
  if (q >= T) return;
  const float inv = q < L ? 1.f / l : 0.f;
  float* orow = O + ((int64_t)b * T + q) * (H * DK) + h * DK;
#pragma unroll
  for (int i = 0; i < DK / 4; ++i)
    *(float4*)(orow + 4 * i) = q < L ? make_float4(o[i].x * inv, o[i].y * inv, o[i].z * inv, o[i].w * inv)
                                     : make_float4(0.f, 0.f, 0.f, 0.f);
}

// bf16: grid (ceil(T / 128), B * H); 4 waves, wave w owns queries [32 w, 32 w + 32) of the workgroup's 128; key tiles of 64
// in LDS: K row-major (A operand of S^T = K Q^T), V transposed (A operand of O^T = V^T P^T).
constexpr int ACM_NT = 256;
constexpr int ACM_Q = 128;
constexpr int ACM_KT = 64;
constexpr int ACM_VLD = ACM_KT + 4;    // bf16 per V^T row: 136 bytes, 8-byte aligned

template <int DK>
__global__ __launch_bounds__(ACM_NT) void attn_causal_bf16_kernel(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ O,
                                                                  const int* __restrict__ lengths, int T, int H, float scale) {
  constexpr int KLD = DK + 8;            // bf16 per K row: 16-byte aligned
  __shared__ __attribute__((aligned(16))) bf16_t Ks[ACM_KT * KLD];
  __shared__ __attribute__((aligned(16))) bf16_t Vt[DK * ACM_VLD];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int r = lane & 31, hi = lane >> 5;
  const int b = blockIdx.y / H, h = blockIdx.y % H;
  int L = lengths ? lengths[b] : T;
  L = L < 0 ? 0 : (L > T ? T : L);
  const int64_t ld = (int64_t)3 * H * DK;
  const bf16_t* base = qkv + (int64_t)b * T * ld + h * DK;
  const int q0 = blockIdx.x * ACM_Q;
  const int q = q0 + wv * 32 + r;
  const int qr = q < T ? q : T - 1;
  const int qw_last = q0 + wv * 32 + 31;  // the wave's last query
  // B operand of S^T: Q[query r][d = 16 s + 8 hi + j]
  bf16x8_t qf[DK / 16];
#pragma unroll
  for (int s = 0; s < DK / 16; ++s) {
    U4 u; u.v = *(const uint4*)(base + (int64_t)qr * ld + 16 * s + 8 * hi);
    qf[s] = u.b;
  }
  lm_f32x16 oacc[DK / 32];
#pragma unroll
  for (int c = 0; c < DK / 32; ++c)
#pragma unroll
    for (int i = 0; i < 16; ++i) oacc[c][i] = 0.f;
  float m = -INFINITY, l = 0.f;   // l: this half-wave's part of the row sum

  const int kend = q0 + ACM_Q < L ? q0 + ACM_Q : L;      // key tiles beyond the workgroup's last query are not visited
  for (int k0 = 0; k0 < kend; k0 += ACM_KT) {
    __syncthreads();
#pragma unroll
    for (int it = 0; it < DK / 32; ++it) {  // chunk e: key e / (DK / 8), 8 channels of K and of V
      const int e = tid + ACM_NT * it;
      const int kr = e / (DK / 8), c8 = (e % (DK / 8)) * 8;
      U4 ku, vu;
      ku.v = make_uint4(0u, 0u, 0u, 0u); vu.v = ku.v;
      if (k0 + kr < kend) {
        const bf16_t* row = base + (int64_t)(k0 + kr) * ld + c8;
        ku.v = *(const uint4*)(row + H * DK);
        vu.v = *(const uint4*)(row + 2 * H * DK);
      }
      *(uint4*)(Ks + kr * KLD + c8) = ku.v;
#pragma unroll
      for (int j = 0; j < 8; ++j)
        Vt[(c8 + j) * ACM_VLD + kr] = (bf16_t)((vu.u[j >> 1] >> ((j & 1) * 16)) & 0xffffu);
    }
    __syncthreads();
#pragma unroll
    for (int kt = 0; kt < ACM_KT / 32; ++kt) {
      const int kb = k0 + kt * 32;
      if (kb >= kend || kb > qw_last) break;  // uniform over the wave: nothing below synchronises the workgroup
      lm_f32x16 sacc;
#pragma unroll
      for (int i = 0; i < 16; ++i) sacc[i] = 0.f;
#pragma unroll
      for (int s = 0; s < DK / 16; ++s) {
        U4 a; a.v = *(const uint4*)(Ks + (kt * 32 + r) * KLD + 16 * s + 8 * hi);
        sacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.b, qf[s], sacc, 0, 0, 0);
      }
      // sacc[i]: key kb + (i & 3) + 8 (i >> 2) + 4 hi, query r
      float cm = -INFINITY;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int key = kb + (i & 3) + 8 * (i >> 2) + 4 * hi;
        const float v = (key <= qr && key < kend) ? sacc[i] * scale : -INFINITY;
        sacc[i] = v;
        cm = fmaxf(cm, v);
      }
      cm = wl_max_xor32(cm);
      // key 0 is at or below every query, and its step comes first: m is finite from there on, whatever cm is
      const float mn = fmaxf(m, cm);
      const float rs = __expf(m - mn);
      m = mn;
      l *= rs;
#pragma unroll
      for (int c = 0; c < DK / 32; ++c)
#pragma unroll
        for (int i = 0; i < 16; ++i) oacc[c][i] *= rs;
      float p[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) { p[i] = __expf(sacc[i] - mn); l += p[i]; }
      // O^T += V^T P^T over this step's keys in two steps of 16; step s, slot e of half hi is accumulator register 8 s + e,
      // i.e. key kb + 16 s + 8 (e >> 2) + 4 hi + (e & 3): V^T is read in that order
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        U4 pb;
#pragma unroll
        for (int e = 0; e < 4; ++e) pb.u[e] = pack_bf16x2(p[8 * s + 2 * e], p[8 * s + 2 * e + 1]);
#pragma unroll
        for (int c = 0; c < DK / 32; ++c) {
          const bf16_t* vrow = Vt + (32 * c + r) * ACM_VLD + kt * 32 + 16 * s + 4 * hi;
          const uint2 v0 = *(const uint2*)vrow, v1 = *(const uint2*)(vrow + 8);
          U4 va; va.u[0] = v0.x; va.u[1] = v0.y; va.u[2] = v1.x; va.u[3] = v1.y;
          oacc[c] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(va.b, pb.b, oacc[c], 0, 0, 0);
        }
      }
    }
  }
  l = wl_sum_xor32(l);
  if (q >= T) return;
  const float inv = q < L ? 1.f / l : 0.f;
  // oacc[c][i]: channel 32 c + (i & 3) + 8 (i >> 2) + 4 hi of query r
  bf16_t* orow = O + ((int64_t)b * T + q) * (H * DK) + h * DK + 4 * hi;
#pragma unroll
  for (int c = 0; c < DK / 32; ++c)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      uint2 v = make_uint2(0u, 0u);
      if (q < L) {
        v.x = pack_bf16x2(oacc[c][4 * g] * inv, oacc[c][4 * g + 1] * inv);
        v.y = pack_bf16x2(oacc[c][4 * g + 2] * inv, oacc[c][4 * g + 3] * inv);
      }
      *(uint2*)(orow + 32 * c + 8 * g) = v;
    }
}

}  // namespace

extern "C" {

int wavlm_lm_logprob_supported(int32_t D, int32_t V, int32_t dtype) {
  return D >= 8 && D <= 8192 && D % 8 == 0 && V >= 1 && lm_dt_ok(dtype) ? 1 : 0;
}

uint64_t wavlm_lm_logprob_workspace_bytes(int64_t R, int32_t V) {
  if (R < 1 || V < 1) return 0;
  const uint64_t b = 3ull * (uint64_t)lm_slabs(V) * (uint64_t)R * sizeof(float);
  return (b + 255) / 256 * 256;
}

int wavlm_lm_logprob(const void* X, int64_t ldx, const void* W, int64_t ldw, int32_t dtype, const int32_t* target, int64_t R,
                     int32_t D, int32_t V, float* logprob, float* lse, void* workspace, uint64_t ws_bytes, void* stream) {
  if (R == 0) return WL_OK;
  if (!X || !W || !target || !logprob || !workspace || R < 0 || !wavlm_lm_logprob_supported(D, V, dtype) || ldx < D || ldw < D)
    return WL_EINVAL;
  const int64_t es = (int64_t)wl_esize(dtype);
  if (((uintptr_t)X & 15) || ((uintptr_t)W & 15) || (ldx * es) % 16 || (ldw * es) % 16 || ((uintptr_t)target & 3) ||
      ((uintptr_t)logprob & 3) || ((uintptr_t)lse & 3) || ((uintptr_t)workspace & 15))
    return WL_EINVAL;
  if (ws_bytes < wavlm_lm_logprob_workspace_bytes(R, V)) return WL_EINVAL;
  const int64_t nslab = lm_slabs(V), nrb = lm_row_blocks(R);
  if (nrb > 0x7fffffffll / nslab) return WL_EINVAL;    // beyond one grid dimension
  float* ws_m = (float*)workspace;
  float* ws_l = ws_m + nslab * R;
  float* ws_t = ws_l + nslab * R;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == WL_BF16)
    WL_LAUNCH(lm_logprob_bf16_kernel, dim3((unsigned)(nslab * nrb)), dim3(LM_NT), 0, st, (const bf16_t*)X, ldx, (const bf16_t*)W,
              ldw, target, R, (int)D, (int)V, (int)nrb, ws_m, ws_l, ws_t);
  else
    WL_LAUNCH(lm_logprob_f32_kernel, dim3((unsigned)(nslab * nrb)), dim3(LMF_NT), 0, st, (const float*)X, ldx, (const float*)W,
              ldw, target, R, (int)D, (int)V, (int)nrb, ws_m, ws_l, ws_t);
  WL_LAUNCH(lm_logprob_combine_kernel, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, st, ws_m, ws_l, ws_t, target, R, (int)V,
            (int)nslab, logprob, lse);
  return wl_check_launch();
}

int wavlm_attn_causal_fwd_supported(int32_t head_dim, int32_t dtype) {
  return (head_dim == 32 || head_dim == 64) && lm_dt_ok(dtype) ? 1 : 0;
}

int wavlm_attn_causal_fwd(const void* qkv, void* O, const int32_t* lengths, int32_t B, int32_t H, int32_t T, int32_t head_dim,
                          int32_t dtype, float scale, void* stream) {
  if (!qkv || !O || qkv == O || B < 1 || H < 1 || T < 1 || !wavlm_attn_causal_fwd_supported(head_dim, dtype) ||
      (int64_t)B * H > 65535 || ((uintptr_t)qkv & 15) || ((uintptr_t)O & 15) || ((uintptr_t)lengths & 3))
    return WL_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const dim3 gm((T + ACM_Q - 1) / ACM_Q, B * H), gf((T + ACF_Q - 1) / ACF_Q, B * H);
  if (dtype == WL_BF16) {
    if (head_dim == 32)
      WL_LAUNCH(attn_causal_bf16_kernel<32>, gm, dim3(ACM_NT), 0, st, (const bf16_t*)qkv, (bf16_t*)O, lengths, (int)T, (int)H, scale);
    else
      WL_LAUNCH(attn_causal_bf16_kernel<64>, gm, dim3(ACM_NT), 0, st, (const bf16_t*)qkv, (bf16_t*)O, lengths, (int)T, (int)H, scale);
  } else {
    if (head_dim == 32)
      WL_LAUNCH(attn_causal_f32_kernel<32>, gf, dim3(ACF_Q), 0, st, (const float*)qkv, (float*)O, lengths, (int)T, (int)H, scale);
    else
      WL_LAUNCH(attn_causal_f32_kernel<64>, gf, dim3(ACF_Q), 0, st, (const float*)qkv, (float*)O, lengths, (int)T, (int)H, scale);
  }
  return wl_check_launch();
}

}  // extern "C"
