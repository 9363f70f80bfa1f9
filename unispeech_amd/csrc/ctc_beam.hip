// Lexicon-free CTC beam search with an n-gram unit LM (additive to ABI 30): the decoder of the reference's
// examples/speech_recognition/w2l_decoder.py in its --unit-lm, no-lexicon mode (flashlight's LexiconFreeDecoder, CTC criterion,
// log_add = false), by the rules written out at ctc.beam_search_reference, which is this kernel's specification.
//
// One workgroup of 1024 lanes per utterance; frames are sequential.  R = beam, K = min(beam_tokens, C), N = R x K <= 16384.
// LDS (dynamic, 8 N + 16 R + 4 C + 8 K bytes: 140.3 KiB at the envelope's corner, under 1 KiB at beam 1):
//   cscore fp32 [N], cstate int32 [N]   the frame's candidates; candidate i = r * K + j is beam entry r with the j-th considered
//                                       class.  The considered classes are kept in ascending order, so "parent rank ascending,
//                                       token ascending" is "i ascending", and prev_blank is (token == blank): a candidate's
//                                       merge key (state, token, prev_blank) is (cstate[i], column j)
//   bscore, bstate, btok [R]            the beam in rank order (btok: last token, 0xffff = none, bit 16 = prev_blank)
//   sel [R], em [C], ktok / kem [K]     the selected candidates; the frame's emissions; the considered classes and their scores
// Per frame:
//   1. the frame's C logits to LDS; unless `normalized` their log-sum-exp (block max, block sum in a fixed order) is subtracted
//   2. lane c ranks class c by counting the classes that beat it (ties to the lower class); the K best are compacted in class
//      order by ballot and popcount
//   3. every candidate is scored from the beam in LDS; a new token walks the LM tables in HBM: a bounded binary search in the
//      node's children, on a miss the node's backoff and its suffix link, at most 8 levels
//   4. the block maximum gives the threshold cut; a surviving candidate is dropped if another parent's candidate of the same
//      column has the same state and comes first in the total order (R compares per candidate, all in LDS)
//   5. if more than R are left, the R-th largest of the 46-bit keys (score bits made monotonic, then 16383 - i) is found bit by
//      bit, each step a block count (cb_kth of ctc_beam_common.hpp, which csrc/ctc_lexbeam.hip shares).  Keys are unique, so the cut takes exactly R
//   6. the selected candidates are compacted through an LDS counter (their slots are arbitrary) and 7. ranked by counting among
//      themselves (their ranks are not); lane p writes beam entry rank(p) and its back-pointer (parent | token << 16) to the workspace
// At the end lm_weight * lm(state, </s>) is added, the survivors are ranked again (ties keep their rank), and lane h < nbest walks
// hypothesis h's back-pointers into tokens[b, h, :], then collapses them in place.
// No global atomics (the two LDS counters only count); nothing depends on B or on the sample's place in the batch.  Every
// address is formed from a range-checked id: classes are lane ids below C, states and child ranges are clamped to the table
// sizes the caller states, back-pointers are clamped to the beam.  Emissions must be finite (a NaN score never survives a frame).
#include "ctc_beam_common.hpp"
#include "../../include/wavlm_hip.h"

#define CB_MAXCAND 16384
#define CB_KEYBITS 14   // CB_MAXCAND = 2^14 candidate indices

static inline int cb_ktok(int64_t C, int64_t beam_tokens) { return (int)(beam_tokens < C ? beam_tokens : C); }
static inline int cb_supported(int64_t C, int64_t beam, int64_t beam_tokens, int64_t lm_order) {
  if (C < 1 || C > CB_MAXC || beam < 1 || beam > CB_MAXBEAM || beam_tokens < 1 || lm_order < 0 || lm_order > CB_MAXORDER) return 0;
  return beam * cb_ktok(C, beam_tokens) <= CB_MAXCAND;
}
static inline size_t cb_lds_bytes(int R, int K, int C) { return 8 * (size_t)R * K + 16 * (size_t)R + 4 * (size_t)C + 8 * (size_t)K; }

__global__ __launch_bounds__(CB_NT) void ctc_beam_kernel(const void* __restrict__ x, int dt, long sb, long st, int T, int C,
    const int* __restrict__ in_len, int blank, int sil, int normalized, CbLm lm, int R, int K, float thr, float lmw, float silw,
    int nbest, int* tokens, int* counts, float* scores, int* n_hyp, int* ws) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __shared__ float s_red[CB_NT / 64];
  __shared__ unsigned long long s_mask[CB_NT / 64];
  __shared__ int s_cnt[64];   // 0: alive, 1: selected, 2 + k: step k of the bit search
  float* cscore = (float*)smem;
  int* cstate = (int*)(cscore + (size_t)R * K);
  float* bscore = (float*)(cstate + (size_t)R * K);
  int* bstate = (int*)(bscore + R);
  int* btok = bstate + R;
  int* sel = btok + R;
  float* em = (float*)(sel + R);
  int* ktok = (int*)(em + C);
  float* kem = (float*)(ktok + K);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x;
  const int Tb = ct_len(in_len, b, T);
  const bool has_lm = lm.n_nodes > 0;
  int* bp = ws + (size_t)b * T * R;

  for (int j = tid; j < K; j += CB_NT) { ktok[j] = 0; kem[j] = 0.0f; }
  if (tid == 0) {
    bscore[0] = 0.0f;
    bstate[0] = has_lm ? lm.start : 0;
    btok[0] = CB_NONE;
  }
  int nb = 1;   // entries in the beam (uniform)
  __syncthreads();

  for (int t = 0; t < Tb; ++t) {
    // 1. emissions
    const long xt = (long)b * sb + (long)t * st;
    float v = -INFINITY;
    if (tid < C) { v = ld_elem(x, xt + tid, dt); em[tid] = v; }
    if (tid < 64) s_cnt[tid] = 0;
    float lse = 0.0f;
    if (!normalized) {
      const float m = cb_block<true>(v, s_red);
      const float sum = cb_block<false>(tid < C ? expf(v - m) : 0.0f, s_red);
      lse = m + logf(sum);
    } else {
      __syncthreads();
    }
    // 2. the K best classes, in class order
    bool take = false;
    if (tid < C) {
      int rank = 0;
      for (int c = 0; c < C; ++c) {
        const float u = em[c];
        rank += (u > v || (u == v && c < tid)) ? 1 : 0;
      }
      take = rank < K;
    }
    const unsigned long long m = __ballot(take);
    if (lane == 0) s_mask[wave] = m;
    __syncthreads();
    if (take) {
      int p = __popcll(m & ((1ull << lane) - 1));
      for (int w = 0; w < wave; ++w) p += __popcll(s_mask[w]);
      if (p < K) { ktok[p] = tid; kem[p] = v - lse; }
    }
    __syncthreads();
    // 3. candidates
    const int N = nb * K;
    float best = -INFINITY;
    for (int i = tid; i < N; i += CB_NT) {
      const int r = i / K, j = i - r * K;
      const int n = ktok[j];
      float s = bscore[r] + kem[j];
      if (n == sil) s += silw;
      int state = bstate[r];
      const int tp = btok[r], last = tp & 0xffff, pb = tp >> 16;
      if (has_lm && n != blank && (n != last || pb)) {
        const float l = cb_lm(lm, state, lm.tok_word[n], &state);
        s += lmw * l;
      }
      cscore[i] = s;
      cstate[i] = state;
      best = fmaxf(best, s);
    }
    best = cb_block<true>(best, s_red);   // (its barriers publish the candidates)
    // 4. threshold and merge
    const float cut = best - thr;
    unsigned dead = 0;
    {
      int k = 0;
      for (int i = tid; i < N; i += CB_NT, ++k) {
        const float s = cscore[i];
        bool d = !(s >= cut);
        if (!d) {
          const int r = i / K, j = i - r * K, state = cstate[i];
          const int* cs = cstate + j;
          const float* sc = cscore + j;
          // eight independent reads of the column's states a step (they pipeline); equal states are rare and take the slow path
          for (int r0 = 0; r0 < nb && !d; r0 += 8) {
            unsigned hit = 0;
#pragma unroll
            for (int u = 0; u < 8; ++u) {
              const int rr = r0 + u < nb ? r0 + u : nb - 1;
              hit |= cs[rr * K] == state ? (1u << u) : 0u;
            }
            for (int u = 0; hit != 0u && u < 8; ++u) {
              const int r2 = r0 + u;
              if (((hit >> u) & 1u) && r2 < nb && r2 != r) {
                const float s2 = sc[r2 * K];
                if (s2 > s || (s2 == s && r2 < r)) d = true;
              }
            }
          }
        }
        dead |= d ? (1u << k) : 0u;
      }
    }
    __syncthreads();
    {
      int k = 0, alive = 0;
      for (int i = tid; i < N; i += CB_NT, ++k) {
        if ((dead >> k) & 1u) cscore[i] = -INFINITY; else ++alive;
      }
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) alive += __shfl_xor(alive, o, 64);
      if (lane == 0 && alive) atomicAdd(&s_cnt[0], alive);
    }
    __syncthreads();
    // 5. the R-th largest key
    unsigned long long kth = 1ull;
    if (s_cnt[0] > R) kth = cb_kth<CB_KEYBITS>(cscore, N, R, s_cnt + 2);
    // 6. compaction
    for (int i = tid; i < N; i += CB_NT) {
      const unsigned long long key = cb_key<CB_KEYBITS>(cscore[i], i);
      if (key != 0ull && key >= kth) {
        const int slot = atomicAdd(&s_cnt[1], 1);
        if (slot < R) sel[slot] = i;
      }
    }
    __syncthreads();
    const int nsel = s_cnt[1] < R ? s_cnt[1] : R;
    // 7. rank, the new beam and its back-pointers
    if (tid < nsel) {
      const int i = sel[tid];
      const unsigned long long key = cb_key<CB_KEYBITS>(cscore[i], i);
      int rank = 0;
      for (int q = 0; q < nsel; ++q) {
        const int iq = sel[q];
        rank += cb_key<CB_KEYBITS>(cscore[iq], iq) > key ? 1 : 0;
      }
      const int r = i / K, n = ktok[i - r * K];
      bscore[rank] = cscore[i];
      bstate[rank] = cstate[i];
      btok[rank] = n | (n == blank ? 0x10000 : 0);
      bp[(size_t)t * R + rank] = r | (n << 16);
    }
    nb = nsel;
    __syncthreads();
  }

  // the end score, the final order and the n-best
  if (tid < nb) {
    float s = bscore[tid];
    if (has_lm) {
      int unused;
      s += lmw * cb_lm(lm, bstate[tid], lm.eos_word, &unused);
    }
    cscore[tid] = s;
  }
  __syncthreads();
  if (tid < nb) {
    const float s = cscore[tid];
    int rank = 0;
    for (int q = 0; q < nb; ++q) {
      const float u = cscore[q];
      rank += (u > s || (u == s && q < tid)) ? 1 : 0;
    }
    if (rank < nbest) sel[rank] = tid;
  }
  __syncthreads();
  const int nh = nb < nbest ? nb : nbest;
  if (tid == 0) n_hyp[b] = nh;
  if (tid < nbest) {
    int* tk = tokens + ((size_t)b * nbest + tid) * T;
    int cnt = 0;
    float score = -INFINITY;
    if (tid < nh) {
      int cur = sel[tid];
      score = cscore[cur];
      for (int t = Tb - 1; t >= 0; --t) {
        if (cur >= R) cur = R - 1;
        const int w = bp[(size_t)t * R + cur];
        tk[t] = (w >> 16) & 0xffff;
        cur = w & 0xffff;
      }
      int last = -1;
      for (int t = 0; t < Tb; ++t) {
        const int a = tk[t];
        if (a != last && a != blank) tk[cnt++] = a;
        last = a;
      }
    }
    for (int t = cnt; t < T; ++t) tk[t] = -1;
    counts[(size_t)b * nbest + tid] = cnt;
    scores[(size_t)b * nbest + tid] = score;
  }
}

extern "C" {

int wavlm_ctc_beam_supported(int32_t C, int32_t beam, int32_t beam_tokens, int32_t lm_order) {
  return cb_supported(C, beam, beam_tokens, lm_order);
}

uint64_t wavlm_ctc_beam_workspace_bytes(int32_t B, int32_t T, int32_t beam) {
  if (B < 0 || T < 0 || beam < 0) return 0;
  return ((uint64_t)B * (uint64_t)T * (uint64_t)beam * 4 + 255) & ~(uint64_t)255;
}

int wavlm_ctc_beam(const void* logits, int32_t dtype, int64_t stride_b, int64_t stride_t, int32_t B, int32_t T, int32_t C,
                   const int32_t* input_lengths, int32_t blank, int32_t sil, int32_t normalized, const int32_t* lm_child_off,
                   const int32_t* lm_child_word, const float* lm_child_logp, const int32_t* lm_child_next,
                   const float* lm_node_backoff, const int32_t* lm_node_suffix, const int32_t* lm_tok_word, int32_t lm_nodes,
                   int32_t lm_children, int32_t lm_start, int32_t lm_eos_word, int32_t lm_order, int32_t beam,
                   int32_t beam_tokens, float beam_threshold, float lm_weight, float sil_weight, int32_t nbest, int32_t* tokens,
                   int32_t* counts, float* scores, int32_t* n_hyp, void* workspace, uint64_t ws_bytes, void* stream) {
  if (dtype != WL_F32 && dtype != WL_BF16) return WL_EINVAL;
  if (B < 0 || T < 1 || T > 0x3fffffff || blank < 0 || blank >= C || !cb_supported(C, beam, beam_tokens, lm_order)) return WL_EINVAL;
  if (nbest < 1 || nbest > beam || !(beam_threshold >= 0.0f) || !isfinite(lm_weight) || !isfinite(sil_weight)) return WL_EINVAL;
  if (lm_nodes < 0 || lm_children < 0 || (lm_nodes > 0) != (lm_order > 0)) return WL_EINVAL;
  if (lm_nodes > 0) {
    if (!lm_child_off || !lm_child_word || !lm_child_logp || !lm_child_next || !lm_node_backoff || !lm_node_suffix || !lm_tok_word)
      return WL_EINVAL;
    if (lm_start < 0 || lm_start >= lm_nodes || lm_eos_word < 0) return WL_EINVAL;
  }
  if (B == 0) return WL_OK;
  if (!logits || !input_lengths || !tokens || !counts || !scores || !n_hyp) return WL_EINVAL;
  if (!ct_view_ok(B, T, C, stride_b, stride_t)) return WL_EINVAL;
  if (!workspace || ws_bytes < wavlm_ctc_beam_workspace_bytes(B, T, beam) || ((uintptr_t)workspace & 3)) return WL_EINVAL;
  const int K = cb_ktok(C, beam_tokens);
  const size_t lds = cb_lds_bytes(beam, K, C);
  if (hipFuncSetAttribute((const void*)ctc_beam_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return WL_ELAUNCH;
  CbLm lm = {lm_child_off, lm_child_word, lm_child_logp, lm_child_next, lm_node_backoff, lm_node_suffix, lm_tok_word,
             (int)lm_nodes, (int)lm_children, (int)lm_start, (int)lm_eos_word};
  WL_LAUNCH(ctc_beam_kernel, dim3((unsigned)B), dim3(CB_NT), lds, (hipStream_t)stream, logits, (int)dtype, (long)stride_b,
            (long)stride_t, (int)T, (int)C, input_lengths, (int)blank, (int)sil, normalized ? 1 : 0, lm, (int)beam, K,
            beam_threshold, lm_weight, sil_weight, (int)nbest, tokens, counts, scores, n_hyp, (int*)workspace);
  return wl_check_launch();
}

}  // extern "C"
