// Seq2seq ASR decoding (additive to ABI 30): the two kernels an autoregressive decoder over encoder frames needs besides
// what the Transformer LM already has (lm.hip, lm_step.hip).
//
//   wavlm_attn_cross_fwd   encoder-decoder attention (src/fairseq/modules/multihead_attention.py with static encoder keys,
//                          modules/transformer_layer.py:392-411): a few query rows per sentence over its many encoder frames.
//                          The rows of a sentence (the live hypotheses of a beam, or the target positions of a teacher-forced
//                          pass) are one group, row_offsets[b] .. row_offsets[b + 1] - 1; a workgroup owns (sentence, head,
//                          tile of up to 32 rows) and walks the sentence's K and V once for all of them -- group-size times less
//                          traffic than a wave per row.  Keys are staged in LDS 128 (bf16) or 64 (fp32) at a time; the four
//                          waves split the keys by a rule that looks at the key index alone, each keeps an online softmax
//                          (running maximum, sum, output) per query in fp32, and the four states are folded through LDS in
//                          wave order.  bf16: S^T = K Q^T and O^T = V^T P^T on v_mfma_f32_32x32x16_bf16, so a query is a
//                          column of both products and its state sits on a lane (the layout of wavlm_attn_causal_fwd); a
//                          column's result does not depend on the other columns.  fp32: FMA in channel order.  Keys at or
//                          beyond src_lengths[b] are never read.  No atomics: bitwise reproducible; a row's bits depend
//                          neither on the other rows of its group, nor on the group's size, nor on B, nor on its place.
//   wavlm_beam_step        one search step of SequenceGenerator._generate (src/fairseq/sequence_generator.py:326-560) with
//                          BeamSearch.step (src/fairseq/search.py:103-147) for every sentence, one workgroup per sentence:
//                          log-softmax of the live rows in fp32 (a wave per row, lanes in a fixed order), the rules on pad, unk,
//                          eos, max_len and min_len, + the rows' cumulative scores, the best min(2 beam, n_live V - 1) of the
//                          sentence by (score descending, k V + token ascending) -- every wave keeps its best in registers, one
//                          entry per lane, sorted, and the four lists are merged in wave order -- and the walk over them:
//                          eos among the first `beam` ranks into the finished list, the first `beam` others into the next
//                          step's rows.  Hypotheses are a tree of slots (parent, token, step score); nothing is reordered.
//   wavlm_beam_step_fused  the same step with shallow fusion of a language model's logits (a second log-softmax state per row,
//                          lp += lm_weight * lm before the NaN rule, sequence_generator.py:338-346) and the n-gram blocker
//                          (ngram_repeat_block.py:96-143): after the log-softmax states are taken from the untouched logits, the
//                          workgroup reads every row's history out of the tree (position i of row k to one thread: about
//                          history x n reads per row, nothing of it in LDS) and overwrites the banned entries of the model's
//                          logits with -inf; the scan behind the barrier reads -inf.  The logits buffer is consumed.  One
//                          kernel template: without LM and blocker every float operation is wavlm_beam_step's.
#include "common.hpp"
#include "tile_loaders.hpp"
#include "../../include/wavlm_hip.h"

#include <math.h>

namespace {

typedef __attribute__((ext_vector_type(16))) float s2s_f32x16;

inline bool s2s_dt_ok(int dt) { return dt == WL_F32 || dt == WL_BF16; }

// ---------------------------------------------------------------------------------------------------- cross attention
constexpr int XA_NT = 256;             // four waves
constexpr int XA_Q = 32;               // query rows per tile
constexpr int XA_KT = 128;             // bf16: keys per stage, 32 per wave
constexpr int XA_VLD = XA_KT + 4;      // bf16 per V^T row: 264 bytes, 8-byte aligned
constexpr int XA_KF = 64;              // fp32: keys per stage, key j of a stage goes to wave j % 4

template <int DK> struct XaSmem {
  static constexpr int KLD = DK + 8;   // bf16 per K row: 16-byte aligned
  static constexpr int STAGE_BF = XA_KT * KLD * 2 + DK * XA_VLD * 2;
  static constexpr int STAGE_F32 = 2 * XA_KF * DK * 4;
  static constexpr int FOLD = 4 * XA_Q * (DK + 1) * 4 + 2 * 4 * XA_Q * 4;
  static constexpr int BF = STAGE_BF > FOLD ? STAGE_BF : FOLD;
  static constexpr int F32 = STAGE_F32 > FOLD ? STAGE_F32 : FOLD;
};

struct XaGroup { int first, end, len; bool bad; };

// the rows of sentence b; offsets that are not non-decreasing or leave [0, R] form no address: the rows they span are NaN,
// except that a row a sound group names as well holds either that group's result or NaN (two workgroups write it)
__device__ __forceinline__ XaGroup xa_group(const int* row_offsets, const int* src_lengths, int b, int R, int Ts) {
  XaGroup g;
  const int lo = row_offsets[b], hi = row_offsets[b + 1];
  g.bad = lo < 0 || hi < lo || hi > R;
  int a = lo < hi ? lo : hi, e = lo < hi ? hi : lo;
  a = a < 0 ? 0 : (a > R ? R : a);
  e = e < 0 ? 0 : (e > R ? R : e);
  g.first = a; g.end = e;
  int L = src_lengths ? src_lengths[b] : Ts;
  g.len = L < 0 ? 0 : (L > Ts ? Ts : L);
  return g;
}

// the four wave states of a tile -> O: thread t owns query t % 32 and DK / 8 channels; sums in wave order
template <typename T, int DK>
__device__ __forceinline__ void xa_fold_store(const float* fo, const float* fm, const float* fl, int tid, int row0, int end,
                                              const int* live, bool bad, int len, T* O, int64_t ld_o, int h) {
  constexpr int CH = DK / 8;
  const int r = tid & 31, c0 = (tid >> 5) * CH;
  const int row = row0 + r;
  if (row >= end) return;
  float y[CH];
  const bool dead = live && live[row] <= 0;
  if (bad) {
#pragma unroll
    for (int c = 0; c < CH; ++c) y[c] = __builtin_nanf("");
  } else if (dead || len <= 0) {
#pragma unroll
    for (int c = 0; c < CH; ++c) y[c] = 0.f;
  } else {
    float M = fm[r];
#pragma unroll
    for (int w = 1; w < 4; ++w) M = fmaxf(M, fm[w * XA_Q + r]);
    float wt[4], L = 0.f;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      wt[w] = expf(fm[w * XA_Q + r] - M);          // 0 for a wave that met no key
      L += fl[w * XA_Q + r] * wt[w];
    }
    const float inv = 1.f / L;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      float s = 0.f;
#pragma unroll
      for (int w = 0; w < 4; ++w) s += fo[(w * XA_Q + r) * (DK + 1) + c0 + c] * wt[w];
      y[c] = s * inv;
    }
  }
  T* orow = O + (int64_t)row * ld_o + h * DK + c0;
  if (sizeof(T) == 4) {
#pragma unroll
    for (int c = 0; c < CH; c += 4) *(float4*)((float*)orow + c) = make_float4(y[c], y[c + 1], y[c + 2], y[c + 3]);
  } else {
    if (CH == 8) {
      *(uint4*)orow = make_uint4(pack_bf16x2(y[0], y[1]), pack_bf16x2(y[2], y[3]), pack_bf16x2(y[CH - 4], y[CH - 3]),
                                 pack_bf16x2(y[CH - 2], y[CH - 1]));
    } else {
      *(uint2*)orow = make_uint2(pack_bf16x2(y[0], y[1]), pack_bf16x2(y[2], y[3]));
    }
  }
}

// grid: ((b * H + h) * tiles + tile); a workgroup takes the tiles tile, tile + tiles, ... of its group
template <int DK>
__global__ __launch_bounds__(XA_NT) void attn_cross_bf16_kernel(const bf16_t* __restrict__ Q, int64_t ld_q,
                                                                const bf16_t* __restrict__ KV, int64_t s_kv, int64_t ld_kv,
                                                                const int* __restrict__ src_lengths,
                                                                const int* __restrict__ row_offsets,
                                                                const int* __restrict__ live, bf16_t* __restrict__ O,
                                                                int64_t ld_o, int R, int Ts, int H, int tiles, float scale) {
  typedef XaSmem<DK> SM;
  constexpr int KLD = SM::KLD;
  __shared__ __attribute__((aligned(16))) unsigned char smem[SM::BF];
  bf16_t* Ks = (bf16_t*)smem;
  bf16_t* Vt = (bf16_t*)(smem + XA_KT * KLD * 2);
  float* fo = (float*)smem;
  float* fm = fo + 4 * XA_Q * (DK + 1);
  float* fl = fm + 4 * XA_Q;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int r = lane & 31, hi = lane >> 5;
  const int tile0 = blockIdx.x % tiles, bh = blockIdx.x / tiles;
  const int b = bh / H, h = bh % H;
  const XaGroup g = xa_group(row_offsets, src_lengths, b, R, Ts);
  const int len = g.bad ? 0 : g.len;
  const bf16_t* kbase = KV + (int64_t)b * s_kv + h * DK;

  for (int row0 = g.first + tile0 * XA_Q; row0 < g.end; row0 += tiles * XA_Q) {
    const int row = row0 + r;
    const bool on = !g.bad && row < g.end && (!live || live[row] > 0);
    // a tile without a live row (a finished sentence of the search) walks no key: K and V are not read for it (uniform over the
    // workgroup; the barrier also orders the previous tile's fold reads before this tile's first stage)
    const int klen = __syncthreads_or((int)on) ? len : 0;
    // B operand of S^T: Q[query r][d = 16 s + 8 hi + j]; a row that is not live reads nothing
    bf16x8_t qf[DK / 16];
#pragma unroll
    for (int s = 0; s < DK / 16; ++s) {
      U4 u; u.v = make_uint4(0u, 0u, 0u, 0u);
      if (on) u.v = *(const uint4*)(Q + (int64_t)row * ld_q + h * DK + 16 * s + 8 * hi);
      qf[s] = u.b;
    }
    s2s_f32x16 oacc[DK / 32];
#pragma unroll
    for (int c = 0; c < DK / 32; ++c)
#pragma unroll
      for (int i = 0; i < 16; ++i) oacc[c][i] = 0.f;
    float m = -INFINITY, l = 0.f;      // l: this half-wave's part of the row sum

    for (int k0 = 0; k0 < klen; k0 += XA_KT) {
      __syncthreads();
#pragma unroll
      for (int it = 0; it < DK / 16; ++it) {   // chunk e: key e / (DK / 8), 8 channels of K and of V
        const int e = tid + XA_NT * it;
        const int kr = e / (DK / 8), c8 = (e % (DK / 8)) * 8;
        U4 ku, vu;
        ku.v = make_uint4(0u, 0u, 0u, 0u); vu.v = ku.v;
        if (k0 + kr < len) {
          const bf16_t* krow = kbase + (int64_t)(k0 + kr) * ld_kv + c8;
          ku.v = *(const uint4*)krow;
          vu.v = *(const uint4*)(krow + H * DK);
        }
        *(uint4*)(Ks + kr * KLD + c8) = ku.v;
#pragma unroll
        for (int j = 0; j < 8; ++j)
          Vt[(c8 + j) * XA_VLD + kr] = (bf16_t)((vu.u[j >> 1] >> ((j & 1) * 16)) & 0xffffu);
      }
      __syncthreads();
      const int kb = k0 + wv * 32;     // this wave's 32 keys of the stage
      if (kb >= len) continue;         // uniform over the wave; the barriers above are met by every wave
      s2s_f32x16 sacc;
#pragma unroll
      for (int i = 0; i < 16; ++i) sacc[i] = 0.f;
#pragma unroll
      for (int s = 0; s < DK / 16; ++s) {
        U4 a; a.v = *(const uint4*)(Ks + (wv * 32 + r) * KLD + 16 * s + 8 * hi);
        sacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.b, qf[s], sacc, 0, 0, 0);
      }
      // sacc[i]: key kb + (i & 3) + 8 (i >> 2) + 4 hi, query r
      float cm = -INFINITY;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int key = kb + (i & 3) + 8 * (i >> 2) + 4 * hi;
        const float v = key < len ? sacc[i] * scale : -INFINITY;
        sacc[i] = v;
        cm = fmaxf(cm, v);
      }
      cm = wl_max_xor32(cm);           // key kb < len: finite
      const float mn = fmaxf(m, cm);
      const float rs = expf(m - mn);   // exp(-inf) = 0 at the wave's first keys
      m = mn;
      l *= rs;
#pragma unroll
      for (int c = 0; c < DK / 32; ++c)
#pragma unroll
        for (int i = 0; i < 16; ++i) oacc[c][i] *= rs;
      float p[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) { p[i] = expf(sacc[i] - mn); l += p[i]; }
      // O^T += V^T P^T over the 32 keys in two steps of 16; step s, slot e of half hi is accumulator register 8 s + e, i.e.
      // key kb + 16 s + 8 (e >> 2) + 4 hi + (e & 3): V^T is read in that order
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        U4 pb;
#pragma unroll
        for (int e = 0; e < 4; ++e) pb.u[e] = pack_bf16x2(p[8 * s + 2 * e], p[8 * s + 2 * e + 1]);
#pragma unroll
        for (int c = 0; c < DK / 32; ++c) {
          const bf16_t* vrow = Vt + (32 * c + r) * XA_VLD + wv * 32 + 16 * s + 4 * hi;
          const uint2 v0 = *(const uint2*)vrow, v1 = *(const uint2*)(vrow + 8);
          U4 va; va.u[0] = v0.x; va.u[1] = v0.y; va.u[2] = v1.x; va.u[3] = v1.y;
          oacc[c] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(va.b, pb.b, oacc[c], 0, 0, 0);
        }
      }
    }
    l = wl_sum_xor32(l);
    __syncthreads();                   // the stage is read no more: its bytes become the fold
    // oacc[c][i]: channel 32 c + (i & 3) + 8 (i >> 2) + 4 hi of query r
#pragma unroll
    for (int c = 0; c < DK / 32; ++c)
#pragma unroll
      for (int i = 0; i < 16; ++i)
        fo[(wv * XA_Q + r) * (DK + 1) + 32 * c + (i & 3) + 8 * (i >> 2) + 4 * hi] = oacc[c][i];
    if (hi == 0) { fm[wv * XA_Q + r] = m; fl[wv * XA_Q + r] = l; }
    __syncthreads();
    xa_fold_store<bf16_t, DK>(fo, fm, fl, tid, row0, g.end, live, g.bad, len, O, ld_o, h);
  }
}

// fp32: lane (r, hi) of wave w owns query r and channels [hi DK / 2, (hi + 1) DK / 2); the two halves of a dot product meet in
// one add (lo + hi); wave w takes keys j % 4 == w of every stage
template <int DK>
__global__ __launch_bounds__(XA_NT) void attn_cross_f32_kernel(const float* __restrict__ Q, int64_t ld_q,
                                                               const float* __restrict__ KV, int64_t s_kv, int64_t ld_kv,
                                                               const int* __restrict__ src_lengths,
                                                               const int* __restrict__ row_offsets,
                                                               const int* __restrict__ live, float* __restrict__ O,
                                                               int64_t ld_o, int R, int Ts, int H, int tiles, float scale) {
  typedef XaSmem<DK> SM;
  constexpr int HC = DK / 2;
  __shared__ __attribute__((aligned(16))) unsigned char smem[SM::F32];
  float* Ks = (float*)smem;
  float* Vs = Ks + XA_KF * DK;
  float* fo = (float*)smem;
  float* fm = fo + 4 * XA_Q * (DK + 1);
  float* fl = fm + 4 * XA_Q;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int r = lane & 31, hi = lane >> 5;
  const int tile0 = blockIdx.x % tiles, bh = blockIdx.x / tiles;
  const int b = bh / H, h = bh % H;
  const XaGroup g = xa_group(row_offsets, src_lengths, b, R, Ts);
  const int len = g.bad ? 0 : g.len;
  const float* kbase = KV + (int64_t)b * s_kv + h * DK;

  for (int row0 = g.first + tile0 * XA_Q; row0 < g.end; row0 += tiles * XA_Q) {
    const int row = row0 + r;
    const bool on = !g.bad && row < g.end && (!live || live[row] > 0);
    // a tile without a live row (a finished sentence of the search) walks no key: K and V are not read for it (uniform over the
    // workgroup; the barrier also orders the previous tile's fold reads before this tile's first stage)
    const int klen = __syncthreads_or((int)on) ? len : 0;
    float q[HC], o[HC];
#pragma unroll
    for (int c = 0; c < HC; c += 4) {
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (on) v = *(const float4*)(Q + (int64_t)row * ld_q + h * DK + hi * HC + c);
      q[c] = v.x; q[c + 1] = v.y; q[c + 2] = v.z; q[c + 3] = v.w;
    }
#pragma unroll
    for (int c = 0; c < HC; ++c) o[c] = 0.f;
    float m = -INFINITY, l = 0.f;

    for (int k0 = 0; k0 < klen; k0 += XA_KF) {
      __syncthreads();
#pragma unroll
      for (int it = 0; it < XA_KF * DK / 4 / XA_NT; ++it) {
        const int e = tid + XA_NT * it;
        const int kr = e / (DK / 4), c4 = (e % (DK / 4)) * 4;
        float4 kv = make_float4(0.f, 0.f, 0.f, 0.f), vv = kv;
        if (k0 + kr < len) {
          const float* krow = kbase + (int64_t)(k0 + kr) * ld_kv + c4;
          kv = *(const float4*)krow;
          vv = *(const float4*)(krow + H * DK);
        }
        *(float4*)(Ks + kr * DK + c4) = kv;
        *(float4*)(Vs + kr * DK + c4) = vv;
      }
      __syncthreads();
      const int kn = len - k0 < XA_KF ? len - k0 : XA_KF;
      for (int j = wv; j < kn; j += 4) {           // uniform over the wave
        const float* kr = Ks + j * DK + hi * HC;
        float d = 0.f;
#pragma unroll
        for (int c = 0; c < HC; c += 4) {
          const float4 kv = *(const float4*)(kr + c);
          d = fmaf(q[c], kv.x, d); d = fmaf(q[c + 1], kv.y, d); d = fmaf(q[c + 2], kv.z, d); d = fmaf(q[c + 3], kv.w, d);
        }
        float s, mn, rs, p;
        {
#pragma clang fp contract(off)
          s = wl_sum_xor32(d) * scale;             // rounds before the maximum is subtracted (see lm_step.hip)
          mn = fmaxf(m, s);
          rs = expf(m - mn);
          p = expf(s - mn);
        }
        m = mn;
        l = l * rs + p;
        const float* vr = Vs + j * DK + hi * HC;
#pragma unroll
        for (int c = 0; c < HC; c += 4) {
          const float4 vv = *(const float4*)(vr + c);
          o[c] = fmaf(p, vv.x, o[c] * rs); o[c + 1] = fmaf(p, vv.y, o[c + 1] * rs);
          o[c + 2] = fmaf(p, vv.z, o[c + 2] * rs); o[c + 3] = fmaf(p, vv.w, o[c + 3] * rs);
        }
      }
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < HC; ++c) fo[(wv * XA_Q + r) * (DK + 1) + hi * HC + c] = o[c];
    if (hi == 0) { fm[wv * XA_Q + r] = m; fl[wv * XA_Q + r] = l; }
    __syncthreads();
    xa_fold_store<float, DK>(fo, fm, fl, tid, row0, g.end, live, g.bad, len, O, ld_o, h);
  }
}

// ---------------------------------------------------------------------------------------------------------- beam step
constexpr int BS_NT = 256;
constexpr int BS_MAXBEAM = 32;
constexpr int BS_NONE = 0x7fffffff;    // the flat index of an empty list entry: loses against every candidate

__device__ __forceinline__ bool bs_better(float s, int i, float s2, int i2) { return s > s2 || (s == s2 && i < i2); }

// the wave's sorted list, entry `lane` on lane `lane` (lanes >= K2 stay empty): put (cs, ci) in, drop the last
__device__ __forceinline__ void bs_insert(float& ls, int& li, float cs, int ci, int lane, int K2) {
  const bool beats = lane < K2 && bs_better(cs, ci, ls, li);
  const float us = __shfl_up(ls, 1, 64);
  const int ui = __shfl_up(li, 1, 64);
  const int ub = __shfl_up((int)beats, 1, 64);
  if (beats) {
    if (lane > 0 && ub) { ls = us; li = ui; }
    else { ls = cs; li = ci; }
  }
}

// every lane offers one candidate (ok = false: none); those that beat the list's last entry go in, in lane order
__device__ __forceinline__ void bs_offer(float& ls, int& li, float s, int idx, bool ok, int lane, int K2) {
  const float ts = __shfl(ls, K2 - 1, 64);
  const int ti = __shfl(li, K2 - 1, 64);
  unsigned long long mask = __ballot(ok && bs_better(s, idx, ts, ti));
  while (mask) {
    const int src = __ffsll((long long)mask) - 1;
    mask &= mask - 1;
    const float cs = __shfl(s, src, 64);
    const int ci = __shfl(idx, src, 64);
    bs_insert(ls, li, cs, ci, lane, K2);           // one that no longer beats the last entry changes nothing
  }
}

// the logits argument: read-only in wavlm_beam_step, written between two barriers by the blocker of the fused step
template <typename T, bool FUSED> struct BsLogits { typedef const T* __restrict__ type; };
template <typename T> struct BsLogits<T, true> { typedef T* type; };

template <typename T, typename TL, bool FUSED>
__global__ __launch_bounds__(BS_NT) void beam_step_kernel(typename BsLogits<T, FUSED>::type logits, int64_t ld_logits,
                                                          const TL* __restrict__ lm, int64_t ld_lm, float lm_weight, int ngram,
                                                          int tree_lim, float* __restrict__ cum,
                                                          int* __restrict__ n_live, int* __restrict__ tokens,
                                                          int* __restrict__ lengths, int* __restrict__ slots,
                                                          const int* __restrict__ anc_in, int* __restrict__ anc_out,
                                                          int64_t ld_anc, int* __restrict__ tree_parent,
                                                          int* __restrict__ tree_token, float* __restrict__ tree_score,
                                                          float* __restrict__ fin_f, int* __restrict__ fin_i,
                                                          int* __restrict__ n_fin, int* __restrict__ finished,
                                                          float* __restrict__ cand_s, int* __restrict__ cand_i,
                                                          int* __restrict__ n_cand, int B, int beam, int V, int step, int max_len,
                                                          int min_len, int pad, int unk, int eos, float unk_penalty,
                                                          float temperature, float len_penalty, int normalize) {
  __shared__ float lm_max[FUSED ? BS_MAXBEAM : 1], lm_logsum[FUSED ? BS_MAXBEAM : 1];
  __shared__ float row_max[BS_MAXBEAM], row_logsum[BS_MAXBEAM], row_cum[BS_MAXBEAM];
  __shared__ float ws_s[4][64];
  __shared__ int ws_i[4][64];
  __shared__ int new_c[BS_MAXBEAM];
  __shared__ int sh_nnew;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int b = blockIdx.x;
  int n = n_live[b];
  n = n < 0 ? 0 : (n > beam ? beam : n);
  const int64_t row0 = (int64_t)b * beam;
  if (n == 0) {                                    // finished earlier: nothing lives, nothing is read
    for (int k = tid; k < beam; k += BS_NT) lengths[row0 + k] = 0;
    if (tid == 0) n_cand[b] = 0;
    return;
  }
  // log-softmax state of the live rows: wave w takes rows w, w + 4, ...; lane i entries i, i + 64, ... in order
  for (int k = wv; k < n; k += 4) {
    const T* row = logits + (row0 + k) * ld_logits;
    float m = -INFINITY, s = 0.f;
    for (int v = lane; v < V; v += 64) {
      const float x = Elem<T>::ld(row + v) / temperature;
      if (x == -INFINITY) continue;                // adds exp(-inf) = 0; with m still -inf the rescale would be exp(-inf + inf)
      const float mn = fmaxf(m, x);                // fmaxf skips a NaN; the sum does not
      s = s * expf(m - mn) + expf(x - mn);
      m = mn;
    }
    const float M = wave_max(m);
    const float S = wave_sum(s * expf(m - M));     // a row of -inf alone: NaN, and every entry becomes -inf below
    if (lane == 0) { row_max[k] = M; row_logsum[k] = logf(S); row_cum[k] = cum[row0 + k]; }
    if constexpr (FUSED) {
      if (lm) {                                    // the LM's row the same way; it takes no temperature
        const TL* lrow = lm + (row0 + k) * ld_lm;
        float ml = -INFINITY, sl = 0.f;
        for (int v = lane; v < V; v += 64) {
          const float y = Elem<TL>::ld(lrow + v);
          if (y == -INFINITY) continue;
          const float mn = fmaxf(ml, y);
          sl = sl * expf(ml - mn) + expf(y - mn);
          ml = mn;
        }
        const float Ml = wave_max(ml);
        const float Sl = wave_sum(sl * expf(ml - Ml));
        if (lane == 0) { lm_max[k] = Ml; lm_logsum[k] = logf(Sl); }
      }
    }
  }
  __syncthreads();
  if constexpr (FUSED) {
    // the blocker (ngram_repeat_block.py:96-143): h[j] = tree_token[anc_in[k][j]] for j < step, h[step] = tokens[row].  For
    // every i < cnt = step + 2 - ngram with h[i .. i + ngram - 2] == h[cnt .. step], token h[i + ngram - 1] is banned: its
    // logit becomes -inf now that both log-softmax states are taken (a banned token still counts in the normaliser), and
    // -inf stays -inf through every rule of the scan.  Several threads may write the same entry; they write the same value.
    const int cnt = step + 2 - ngram;
    if (ngram > 0 && cnt > 0) {                    // uniform over the workgroup
      for (int e = tid; e < n * cnt; e += BS_NT) {
        const int k = e / cnt, i = e - k * cnt;
        const int* anc = anc_in + (row0 + k) * ld_anc;
        const int last = tokens[row0 + k];
        auto hist = [&](int j) -> int {
          if (j >= step) return last;
          const int sl = anc[j];
          return (unsigned)sl < (unsigned)tree_lim ? tree_token[sl] : -1;
        };
        bool eq = true;
        for (int j = 0; j < ngram - 1 && eq; ++j) eq = hist(i + j) == hist(cnt + j);
        if (eq) {
          const int t = hist(i + ngram - 1);
          if ((unsigned)t < (unsigned)V) Elem<T>::st(logits + (row0 + k) * ld_logits + t, -INFINITY);
        }
      }
      __syncthreads();
    }
  }
  const int total = n * V;
  const int K2 = 2 * beam < total - 1 ? 2 * beam : total - 1;     // search.py:131-135; >= 1 since V >= 2
  float ls = -INFINITY;
  int li = BS_NONE;
  for (int i0 = wv * 64; i0 < total; i0 += BS_NT) {
    const int idx = i0 + lane;
    const bool ok = idx < total;
    float sc = -INFINITY;
    if (ok) {
      const int k = idx / V, v = idx - k * V;
      const float x = Elem<T>::ld(logits + (row0 + k) * ld_logits + v) / temperature;
      float lp = (x - row_max[k]) - row_logsum[k];
      if constexpr (FUSED) {
        if (lm) {                                                  // 338-344: 0 * -inf is NaN, and a NaN is -inf below
#pragma clang fp contract(off)
          const float l = (Elem<TL>::ld(lm + (row0 + k) * ld_lm + v) - lm_max[k]) - lm_logsum[k];
          const float wl = lm_weight * l;
          lp = lp + wl;
        }
      }
      if (lp != lp) lp = -INFINITY;                                // sequence_generator.py:346
      if (v == pad) lp = -INFINITY;                                // 348
      if (v == unk) lp -= unk_penalty;                             // 349
      if (step >= max_len && v != eos) lp = -INFINITY;             // 352-354
      if (step < min_len && v == eos) lp = -INFINITY;              // 365-367
      sc = lp + row_cum[k];                                        // search.py:119-126
      if (sc != sc) sc = -INFINITY;                                // -inf rows against +inf never arise; keep the order total
    }
    bs_offer(ls, li, sc, idx, ok, lane, K2);
  }
  ws_s[wv][lane] = ls; ws_i[wv][lane] = li;
  __syncthreads();
  if (wv == 0) {
    for (int w = 1; w < 4; ++w) bs_offer(ls, li, ws_s[w][lane], ws_i[w][lane], ws_i[w][lane] != BS_NONE, lane, K2);
    ws_s[0][lane] = ls; ws_i[0][lane] = li;
    if (lane < K2) { cand_s[(int64_t)b * 2 * beam + lane] = ls; cand_i[(int64_t)b * 2 * beam + lane] = li; }
    if (lane == 0) n_cand[b] = K2;
  }
  __syncthreads();
  // the walk (sequence_generator.py:405-520)
  const int64_t here = ((int64_t)step * B + b) * beam;             // the slots of this step's rows
  if (tid == 0) {
    int nf = n_fin[b];
    int nnew = 0;
    for (int c = 0; c < K2; ++c) {
      const float s = ws_s[0][c];
      const int idx = ws_i[0][c];
      const int k = idx / V, tok = idx - k * V;
      if (tok == eos && s > -INFINITY) {                           // an eos at -inf is no eos (line 414)
        if (c < beam && nf < beam) {
          const int64_t f = (int64_t)b * beam + nf;
          fin_f[3 * f] = normalize ? s / powf((float)(step + 1), len_penalty) : s;
          fin_f[3 * f + 1] = s;
          fin_f[3 * f + 2] = s - row_cum[k];
          fin_i[2 * f] = (int)(here + k);
          fin_i[2 * f + 1] = step + 1;
          ++nf;
        }
      } else if (nnew < beam) {
        new_c[nnew++] = c;
      }
    }
    n_fin[b] = nf;
    const int done = nf >= beam || step >= max_len || nnew == 0;
    if (done) { atomicAdd(finished, 1); nnew = 0; }
    n_live[b] = nnew;
    sh_nnew = nnew;
  }
  __syncthreads();
  const int nnew = sh_nnew;
  const int64_t next = ((int64_t)(step + 1) * B + b) * beam;
  for (int k = tid; k < beam; k += BS_NT) {
    if (k < nnew) {
      const int c = new_c[k];
      const float s = ws_s[0][c];
      const int idx = ws_i[0][c];
      const int kp = idx / V, tok = idx - kp * V;
      tokens[row0 + k] = tok;
      lengths[row0 + k] = step + 2;
      slots[row0 + k] = (int)(next + k);
      tree_parent[next + k] = (int)(here + kp);
      tree_token[next + k] = tok;
      tree_score[next + k] = s - row_cum[kp];
    } else {
      tokens[row0 + k] = pad;
      lengths[row0 + k] = 0;
      slots[row0 + k] = 0;
    }
  }
  __syncthreads();                                                 // row_cum was read above by other threads
  for (int k = tid; k < beam; k += BS_NT) cum[row0 + k] = k < nnew ? ws_s[0][new_c[k]] : -INFINITY;
  // the ancestors of a new row: its parent's, then the parent's slot
  for (int e = tid; e < nnew * (step + 1); e += BS_NT) {
    const int k = e / (step + 1), j = e - k * (step + 1);
    const int kp = ws_i[0][new_c[k]] / V;
    anc_out[(row0 + k) * ld_anc + j] = j < step ? anc_in[(row0 + kp) * ld_anc + j] : (int)(here + kp);
  }
}

}  // namespace

extern "C" {

int wavlm_attn_cross_fwd_supported(int32_t head_dim, int32_t dtype) {
  return (head_dim == 32 || head_dim == 64) && s2s_dt_ok(dtype) ? 1 : 0;
}

int wavlm_attn_cross_fwd(const void* Q, int64_t ld_q, const void* KV, int64_t s_kv, int64_t ld_kv, const int32_t* src_lengths,
                         const int32_t* row_offsets, const int32_t* live, void* O, int64_t ld_o, int32_t R, int32_t B, int32_t Ts,
                         int32_t H, int32_t head_dim, int32_t dtype, float scale, int32_t max_group, void* stream) {
  if (!Q || !KV || !row_offsets || !O || R < 1 || B < 1 || Ts < 1 || H < 1 || max_group < 1 ||
      !wavlm_attn_cross_fwd_supported(head_dim, dtype))
    return WL_EINVAL;
  const int64_t es = (int64_t)wl_esize(dtype), D = (int64_t)H * head_dim;
  if (ld_q < D || ld_o < D || ld_kv < 2 * D || s_kv < ((int64_t)Ts - 1) * ld_kv + 2 * D) return WL_EINVAL;
  if (((uintptr_t)Q & 15) || ((uintptr_t)KV & 15) || ((uintptr_t)O & 15) || (ld_q * es) % 16 || (ld_o * es) % 16 ||
      (ld_kv * es) % 16 || (s_kv * es) % 16 || ((uintptr_t)src_lengths & 3) || ((uintptr_t)row_offsets & 3) || ((uintptr_t)live & 3))
    return WL_EINVAL;
  // Q, KV and O must not overlap: byte ranges [first row, end of the last row)
  const uintptr_t p[3] = {(uintptr_t)Q, (uintptr_t)KV, (uintptr_t)O};
  const uint64_t n[3] = {(uint64_t)(((int64_t)R - 1) * ld_q + D) * es,
                         (uint64_t)(((int64_t)B - 1) * s_kv + ((int64_t)Ts - 1) * ld_kv + 2 * D) * es,
                         (uint64_t)(((int64_t)R - 1) * ld_o + D) * es};
  for (int i = 0; i < 3; ++i)
    for (int j = i + 1; j < 3; ++j)
      if (p[i] < p[j] + n[j] && p[j] < p[i] + n[i]) return WL_EINVAL;
  const int64_t cap = ((int64_t)(max_group < R ? max_group : R) + XA_Q - 1) / XA_Q;
  const int64_t blocks = (int64_t)B * H * cap;
  if (blocks > 0x7fffffffll) return WL_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)blocks), block(XA_NT);
#define XA_GO(KERNEL, T, DK)                                                                                                \
  WL_LAUNCH((KERNEL<DK>), grid, block, 0, st, (const T*)Q, ld_q, (const T*)KV, s_kv, ld_kv, src_lengths, row_offsets, live, \
            (T*)O, ld_o, (int)R, (int)Ts, (int)H, (int)cap, scale)
  if (dtype == WL_BF16) {
    if (head_dim == 32) XA_GO(attn_cross_bf16_kernel, bf16_t, 32); else XA_GO(attn_cross_bf16_kernel, bf16_t, 64);
  } else {
    if (head_dim == 32) XA_GO(attn_cross_f32_kernel, float, 32); else XA_GO(attn_cross_f32_kernel, float, 64);
  }
#undef XA_GO
  return wl_check_launch();
}

int wavlm_beam_step_supported(int32_t beam, int32_t V, int32_t B, int32_t dtype) {
  return beam >= 1 && beam <= BS_MAXBEAM && V >= 2 && V <= 65536 && B >= 1 && B <= 65535 && s2s_dt_ok(dtype) ? 1 : 0;
}

uint64_t wavlm_beam_step_workspace_bytes(int32_t B, int32_t beam) {
  if (B < 1 || beam < 1) return 0;
  const uint64_t b = (uint64_t)B * (2ull * beam * 8 + 4);
  return (b + 255) / 256 * 256;
}

int wavlm_beam_step(const void* logits, int64_t ld_logits, int32_t dtype, float* cum, int32_t* n_live, int32_t* tokens,
                    int32_t* lengths, int32_t* slots, const int32_t* anc_in, int32_t* anc_out, int64_t ld_anc,
                    int32_t* tree_parent, int32_t* tree_token, float* tree_score, int64_t tree_slots, float* fin_f, int32_t* fin_i,
                    int32_t* n_fin, int32_t* finished, int32_t B, int32_t beam, int32_t V, int32_t step, int32_t max_len,
                    int32_t min_len, int32_t pad, int32_t unk, int32_t eos, float unk_penalty, float temperature,
                    float len_penalty, int32_t normalize_scores, void* workspace, uint64_t ws_bytes, void* stream) {
  if (!logits || !cum || !n_live || !tokens || !lengths || !slots || !anc_in || !anc_out || anc_in == anc_out || !tree_parent ||
      !tree_token || !tree_score || !fin_f || !fin_i || !n_fin || !finished || !workspace ||
      !wavlm_beam_step_supported(beam, V, B, dtype))
    return WL_EINVAL;
  if (step < 0 || max_len < 0 || ld_logits < V || ld_anc < (int64_t)step + 1 || !(temperature > 0.f) ||
      tree_slots < ((int64_t)step + 2) * B * beam || ((int64_t)step + 2) * B * beam > 0x7fffffffll ||
      ws_bytes < wavlm_beam_step_workspace_bytes(B, beam) || ((uintptr_t)workspace & 15))
    return WL_EINVAL;
  if (((uintptr_t)logits & 3) || (dtype == WL_BF16 && ((uintptr_t)logits & 1))) return WL_EINVAL;
  float* cand_s = (float*)workspace;
  int* cand_i = (int*)(cand_s + (int64_t)B * 2 * beam);
  int* n_cand = cand_i + (int64_t)B * 2 * beam;
  hipStream_t st = (hipStream_t)stream;
#define BS_GO(T)                                                                                                              \
  WL_LAUNCH((beam_step_kernel<T, float, false>), dim3((unsigned)B), dim3(BS_NT), 0, st, (const T*)logits, ld_logits,          \
            (const float*)nullptr, (int64_t)0, 0.f, 0, 0, cum, n_live, tokens,                                                \
            lengths, slots, anc_in, anc_out, ld_anc, tree_parent, tree_token, tree_score, fin_f, fin_i, n_fin, finished,      \
            cand_s, cand_i, n_cand, (int)B, (int)beam, (int)V, (int)step, (int)max_len, (int)min_len, (int)pad, (int)unk,     \
            (int)eos, unk_penalty, temperature, len_penalty, (int)normalize_scores)
  if (dtype == WL_BF16) BS_GO(bf16_t); else BS_GO(float);
#undef BS_GO
  return wl_check_launch();
}

int wavlm_beam_step_fused_supported(int32_t beam, int32_t V, int32_t B, int32_t dtype, int32_t lm_dtype) {
  return wavlm_beam_step_supported(beam, V, B, dtype) && s2s_dt_ok(lm_dtype) ? 1 : 0;
}

int wavlm_beam_step_fused(void* logits, int64_t ld_logits, int32_t dtype, const void* lm_logits, int64_t ld_lm, int32_t lm_dtype,
                          float lm_weight, int32_t no_repeat_ngram_size, float* cum, int32_t* n_live, int32_t* tokens,
                          int32_t* lengths, int32_t* slots, const int32_t* anc_in, int32_t* anc_out, int64_t ld_anc,
                          int32_t* tree_parent, int32_t* tree_token, float* tree_score, int64_t tree_slots, float* fin_f,
                          int32_t* fin_i, int32_t* n_fin, int32_t* finished, int32_t B, int32_t beam, int32_t V, int32_t step,
                          int32_t max_len, int32_t min_len, int32_t pad, int32_t unk, int32_t eos, float unk_penalty,
                          float temperature, float len_penalty, int32_t normalize_scores, void* workspace, uint64_t ws_bytes,
                          void* stream) {
  if (!logits || !cum || !n_live || !tokens || !lengths || !slots || !anc_in || !anc_out || anc_in == anc_out || !tree_parent ||
      !tree_token || !tree_score || !fin_f || !fin_i || !n_fin || !finished || !workspace ||
      !wavlm_beam_step_fused_supported(beam, V, B, dtype, lm_logits ? lm_dtype : WL_F32))
    return WL_EINVAL;
  if (step < 0 || max_len < 0 || ld_logits < V || ld_anc < (int64_t)step + 1 || !(temperature > 0.f) ||
      tree_slots < ((int64_t)step + 2) * B * beam || ((int64_t)step + 2) * B * beam > 0x7fffffffll ||
      ws_bytes < wavlm_beam_step_workspace_bytes(B, beam) || ((uintptr_t)workspace & 15))
    return WL_EINVAL;
  if (((uintptr_t)logits & 3) || (dtype == WL_BF16 && ((uintptr_t)logits & 1))) return WL_EINVAL;
  if (no_repeat_ngram_size < 0 || !isfinite(lm_weight)) return WL_EINVAL;
  if (lm_logits) {
    if (ld_lm < V || ((uintptr_t)lm_logits & (lm_dtype == WL_BF16 ? 1 : 3))) return WL_EINVAL;
    // the blocker writes into `logits`: the two must not overlap
    const uintptr_t a = (uintptr_t)logits, c = (uintptr_t)lm_logits;
    const uint64_t na = (uint64_t)(((int64_t)B * beam - 1) * ld_logits + V) * (uint64_t)wl_esize(dtype);
    const uint64_t nc = (uint64_t)(((int64_t)B * beam - 1) * ld_lm + V) * (uint64_t)wl_esize(lm_dtype);
    if (a < c + nc && c < a + na) return WL_EINVAL;
  }
  float* cand_s = (float*)workspace;
  int* cand_i = (int*)(cand_s + (int64_t)B * 2 * beam);
  int* n_cand = cand_i + (int64_t)B * 2 * beam;
  const int tree_lim = (int)(tree_slots < 0x7fffffffll ? tree_slots : 0x7fffffffll);
  hipStream_t st = (hipStream_t)stream;
#define BS_GO(T, TL)                                                                                                          \
  WL_LAUNCH((beam_step_kernel<T, TL, true>), dim3((unsigned)B), dim3(BS_NT), 0, st, (T*)logits, ld_logits,                    \
            (const TL*)lm_logits, ld_lm, lm_weight, (int)no_repeat_ngram_size, tree_lim, cum, n_live, tokens,                 \
            lengths, slots, anc_in, anc_out, ld_anc, tree_parent, tree_token, tree_score, fin_f, fin_i, n_fin, finished,      \
            cand_s, cand_i, n_cand, (int)B, (int)beam, (int)V, (int)step, (int)max_len, (int)min_len, (int)pad, (int)unk,     \
            (int)eos, unk_penalty, temperature, len_penalty, (int)normalize_scores)
  const bool lb = lm_logits && lm_dtype == WL_BF16;
  if (dtype == WL_BF16) { if (lb) BS_GO(bf16_t, bf16_t); else BS_GO(bf16_t, float); }
  else { if (lb) BS_GO(float, bf16_t); else BS_GO(float, float); }
#undef BS_GO
  return wl_check_launch();
}

}  // extern "C"
