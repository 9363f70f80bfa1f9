// CTC validation scoring in one launch (additive to ABI 30): the greedy decode of csrc/ctc.hip followed, in the same workgroup, by
// the unit and word edit distances of the reference's criterions/ctc.py:161-226 -- so that of a validation batch nothing but
// [B, 4] integers (c_err, c_len, w_err, w_len) has to leave the device.
//
// One workgroup of 4 waves per sample.
//  1. ct_greedy_sample (ctc_decode.hpp, the code of wavlm_ctc_greedy): tokens[b, :], counts[b].
//  2. Three waves compact, 64 elements a step by ballot and popcount (order kept, no atomics):
//       wave 0  targ units  tu = t[(t != pad) & (t != eos)], anywhere in the row
//       wave 1  pred stream pw = the decode without its DROP tokens
//       wave 2  targ stream tw = tu without its DROP tokens
//  3. Waves 1 and 2 cut their stream into words: a word starts at a non-SEP token whose left neighbour is a SEP (or the stream's
//     edge) and ends at one whose right neighbour is; the k-th start and the k-th end are the k-th word's, so both are ranked by
//     ballot as well.  With each_token_a_word every token is a word (post_process = None: `|` is an ordinary token).
//  4. Waves 1 and 2 give each word its length and a 32-bit hash of its tokens.
//  5. Wave 0 runs the unit DP (decode against tu), wave 1 the word DP (pred words against targ words).
// A class outside [0, C) never indexes the table: it is a LETTER, compared by value.
//
// The DP.  Columns are the target, rows stream over the hypothesis; a lane holds PER consecutive columns in registers (PER = 4 up
// to Lt = 256, 16 up to 1024).  With D the row above:  e[j] = min(D[j] + 1, D[j - 1] + neq(i, j)),  cur[j] = min_k<=j (e[k] + j - k)
// = j + prefix_min(e[k] - k), e[0] = i: the insertion chain becomes a running minimum inside the lane and one 6-step shuffle scan
// across lanes; no LDS, no barrier per row.  Rows are fetched 64 at a time, one per lane, and broadcast by v_readlane.
// Word equality: same length, same hash, and then the tokens themselves are compared -- the hash only saves the walk, the
// result is exact.  All arithmetic is integer; nothing depends on B or on the sample's place in the batch.
#include "ctc_decode.hpp"
#include "../../include/wavlm_hip.h"

#define CS_DROP 0
#define CS_SEP 1
#define CS_LETTER 2
#define CS_MAXLT 1024   // 64 lanes x 16 columns

static inline int cs_supported(int64_t T, int64_t Lt) { return T >= 1 && T <= 0x3fffffff && Lt >= 0 && Lt <= CS_MAXLT; }
// ints of workspace per sample: tu | tw | tS | tL | tH (Lt each), pw | pS | pL | pH (T each)
static inline uint64_t cs_sample_ints(int64_t T, int64_t Lt) { return 5 * (uint64_t)Lt + 4 * (uint64_t)T; }

__device__ __forceinline__ int cs_cls(const uint8_t* __restrict__ cls, int C, int v) {
  return (unsigned)v < (unsigned)C ? (int)cls[v] : CS_LETTER;
}

struct cs_keep_units {
  int pad, eos;
  __device__ __forceinline__ bool operator()(int v) const { return v != pad && v != eos; }
};
struct cs_keep_stream {
  const uint8_t* cls; int C, pad, eos;   // pad = eos = -1 for the decode, which keeps them
  __device__ __forceinline__ bool operator()(int v) const { return v != pad && v != eos && cs_cls(cls, C, v) != CS_DROP; }
};

// one wave: dst = the elements of src[0 .. n) that `keep` takes, in order; returns their number (to every lane)
template <class Keep>
__device__ __forceinline__ int cs_compact(const int* src, int n, int* dst, const Keep keep, int lane) {
  int base = 0;
  for (int i0 = 0; i0 < n; i0 += 64) {
    const int i = i0 + lane;
    const int v = i < n ? src[i] : 0;
    const bool k = i < n && keep(v);
    const unsigned long long m = __ballot(k);
    if (k) dst[base + __popcll(m & ((1ull << lane) - 1))] = v;
    base += __popcll(m);
  }
  return base;
}

// one wave: the words of the stream w[0 .. n): S[k] = first token, E[k] = one past the last; returns the number of words
__device__ __forceinline__ int cs_spans(const int* w, int n, const uint8_t* __restrict__ cls, int C, int each, int* S, int* E,
                                        int lane) {
  int nb = 0, ne = 0;
  for (int i0 = 0; i0 < n; i0 += 64) {
    const int i = i0 + lane;
    const bool in = i < n;
    const bool let = in && cs_cls(cls, C, w[i]) != CS_SEP;
    const bool first = let && (each || i == 0 || cs_cls(cls, C, w[i - 1]) == CS_SEP);
    const bool last = let && (each || i == n - 1 || cs_cls(cls, C, w[i + 1]) == CS_SEP);
    const unsigned long long mb = __ballot(first), me = __ballot(last), below = (1ull << lane) - 1;
    if (first) S[nb + __popcll(mb & below)] = i;
    if (last) E[ne + __popcll(me & below)] = i + 1;
    nb += __popcll(mb);
    ne += __popcll(me);
  }
  return nb;
}

// one wave: L[k] (the end on entry) becomes the word's length, H[k] its hash (FNV-1a over the token ids)
__device__ __forceinline__ void cs_finish(const int* w, const int* S, int* L, int* H, int nw, int lane) {
  for (int k = lane; k < nw; k += 64) {
    const int s = S[k], len = L[k] - s;
    unsigned h = 2166136261u;
    for (int q = 0; q < len; ++q) h = (h ^ (unsigned)w[s + q]) * 16777619u;
    L[k] = len;
    H[k] = (int)h;
  }
}

// one wave: Levenshtein distance of the m rows against the n <= 64 * PER columns.  Units: r0 / c0 are the token ids.  Words:
// r0 / c0 are the words' first tokens in rW / cW, r1 / c1 their lengths, r2 / c2 their hashes.
template <int PER, bool WORDS>
__device__ __forceinline__ int cs_dp(const int* r0p, const int* r1p, const int* r2p, const int* rW, int m, const int* c0p,
                                     const int* c1p, const int* c2p, const int* cW, int n, int lane) {
  m = __builtin_amdgcn_readfirstlane(m);
  n = __builtin_amdgcn_readfirstlane(n);
  int prev[PER], c0[PER], c1[PER], c2[PER];
  const int j0 = lane * PER;   // this lane's first column (0-based element; DP column j0 + 1)
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    const int j = j0 + k;
    const bool in = j < n;
    c0[k] = in ? c0p[j] : 0;
    c1[k] = (WORDS && in) ? c1p[j] : -1;   // a column beyond the target equals no word (its cells are never read)
    c2[k] = (WORDS && in) ? c2p[j] : 0;
    prev[k] = j + 1;
  }
  for (int i0 = 0; i0 < m; i0 += 64) {
    const int ri = i0 + lane;
    const int r0 = ri < m ? r0p[ri] : 0;
    const int r1 = (WORDS && ri < m) ? r1p[ri] : 0;
    const int r2 = (WORDS && ri < m) ? r2p[ri] : 0;
    const int nr = m - i0 < 64 ? m - i0 : 64;
    for (int r = 0; r < nr; ++r) {
      const int i = i0 + r + 1;   // DP row
      const int a0 = __builtin_amdgcn_readlane(r0, r);
      const int a1 = WORDS ? __builtin_amdgcn_readlane(r1, r) : 0;
      const int a2 = WORDS ? __builtin_amdgcn_readlane(r2, r) : 0;
      int d = __shfl_up(prev[PER - 1], 1, 64);   // D[i - 1][j0]
      if (lane == 0) d = i - 1;
      int e[PER];
#pragma unroll
      for (int k = 0; k < PER; ++k) {
        bool eq;
        if (WORDS) {
          eq = c1[k] == a1 && c2[k] == a2;
          if (eq)
            for (int q = 0; q < a1; ++q)
              if (rW[a0 + q] != cW[c0[k] + q]) { eq = false; break; }
        } else {
          eq = c0[k] == a0;
        }
        const int up = prev[k] + 1, dg = d + (eq ? 0 : 1);
        d = prev[k];
        e[k] = (up < dg ? up : dg) - (j0 + k + 1);
      }
#pragma unroll
      for (int k = 1; k < PER; ++k) e[k] = e[k] < e[k - 1] ? e[k] : e[k - 1];
      int t = e[PER - 1];   // inclusive prefix minimum over the lanes
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(t, o, 64);
        if (lane >= o && u < t) t = u;
      }
      int ex = __shfl_up(t, 1, 64);   // everything left of this lane, and column 0 (e[0] - 0 = i)
      ex = (lane == 0 || i < ex) ? i : ex;
#pragma unroll
      for (int k = 0; k < PER; ++k) prev[k] = (j0 + k + 1) + (e[k] < ex ? e[k] : ex);
    }
  }
  if (n == 0) return m;
  int res = 0;
#pragma unroll
  for (int k = 0; k < PER; ++k) res = (j0 + k + 1 == n) ? prev[k] : res;
  return __shfl(res, (n - 1) / PER, 64);
}

template <int PER>
__global__ __launch_bounds__(CT_NT) void ctc_score_kernel(const void* __restrict__ x, int dt, long sb, long st, int T, int C,
    const int* __restrict__ in_len, int blank, const int* __restrict__ targets, int Lt, int pad, int eos,
    const uint8_t* __restrict__ cls, int each, int* tokens, int* counts, int* ws, int* __restrict__ out) {
  __shared__ int s_arg[CT_NT];
  __shared__ int s_state[2];
  __shared__ int s_n[5];   // units of the target, pred stream, targ stream, pred words, targ words
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x;
  const int cnt = ct_greedy_sample(x, dt, sb, st, T, C, in_len, blank, tokens, counts, b, s_arg, s_state);
  const int* tok = tokens + (long)b * T;
  const int* trow = targets + (long)b * Lt;
  int* tu = ws + (size_t)b * (5 * (size_t)Lt + 4 * (size_t)T);
  int *tw = tu + Lt, *tS = tw + Lt, *tL = tS + Lt, *tH = tL + Lt;
  int *pw = tH + Lt, *pS = pw + T, *pL = pS + T, *pH = pL + T;

  if (wave == 0) {
    const int n = cs_compact(trow, Lt, tu, cs_keep_units{pad, eos}, lane);
    if (lane == 0) s_n[0] = n;
  } else if (wave == 1) {
    const int n = cs_compact(tok, cnt, pw, cs_keep_stream{cls, C, -1, -1}, lane);
    if (lane == 0) s_n[1] = n;
  } else if (wave == 2) {
    const int n = cs_compact(trow, Lt, tw, cs_keep_stream{cls, C, pad, eos}, lane);
    if (lane == 0) s_n[2] = n;
  }
  __syncthreads();
  if (wave == 1) {
    const int n = cs_spans(pw, s_n[1], cls, C, each, pS, pL, lane);
    if (lane == 0) s_n[3] = n;
  } else if (wave == 2) {
    const int n = cs_spans(tw, s_n[2], cls, C, each, tS, tL, lane);
    if (lane == 0) s_n[4] = n;
  }
  __syncthreads();
  if (wave == 1) cs_finish(pw, pS, pL, pH, s_n[3], lane);
  else if (wave == 2) cs_finish(tw, tS, tL, tH, s_n[4], lane);
  __syncthreads();
  if (wave == 0) {
    const int nt = s_n[0];
    const int c_err = cs_dp<PER, false>(tok, nullptr, nullptr, nullptr, cnt, tu, nullptr, nullptr, nullptr, nt, lane);
    if (lane == 0) { out[4 * b + 0] = c_err; out[4 * b + 1] = nt; }
  } else if (wave == 1) {
    const int nw = s_n[4];
    const int w_err = cs_dp<PER, true>(pS, pL, pH, pw, s_n[3], tS, tL, tH, tw, nw, lane);
    if (lane == 0) { out[4 * b + 2] = w_err; out[4 * b + 3] = nw; }
  }
}

extern "C" {

int wavlm_ctc_score_supported(int32_t T, int32_t Lt) { return cs_supported(T, Lt); }

uint64_t wavlm_ctc_score_workspace_bytes(int32_t B, int32_t T, int32_t Lt) {
  if (B < 0 || T < 0 || Lt < 0) return 0;
  return ((uint64_t)B * cs_sample_ints(T, Lt) * 4 + 255) & ~(uint64_t)255;
}

int wavlm_ctc_score(const void* logits, int32_t dtype, int64_t stride_b, int64_t stride_t, int32_t B, int32_t T, int32_t C,
                    const int32_t* input_lengths, int32_t blank, const int32_t* targets, int32_t Lt, int32_t pad, int32_t eos,
                    const uint8_t* cls, int32_t each_token_a_word, int32_t* tokens, int32_t* counts, int32_t* out,
                    void* workspace, uint64_t ws_bytes, void* stream) {
  if (dtype != WL_F32 && dtype != WL_BF16) return WL_EINVAL;
  if (B < 0 || C < 1 || blank < 0 || blank >= C || !cs_supported(T, Lt)) return WL_EINVAL;
  if (B == 0) return WL_OK;
  if (!logits || !input_lengths || !tokens || !counts || !out || !cls || (Lt > 0 && !targets)) return WL_EINVAL;
  if (!ct_view_ok(B, T, C, stride_b, stride_t)) return WL_EINVAL;
  if (!workspace || ws_bytes < wavlm_ctc_score_workspace_bytes(B, T, Lt) || ((uintptr_t)workspace & 3)) return WL_EINVAL;
  hipStream_t s = (hipStream_t)stream;
#define CS_GO(PER)                                                                                                         \
  WL_LAUNCH((ctc_score_kernel<PER>), dim3((unsigned)B), dim3(CT_NT), 0, s, logits, (int)dtype, (long)stride_b, (long)stride_t, \
            (int)T, (int)C, input_lengths, (int)blank, targets, (int)Lt, (int)pad, (int)eos, cls, each_token_a_word ? 1 : 0, \
            tokens, counts, (int*)workspace, out)
  if (Lt <= 64 * 4) CS_GO(4);
  else CS_GO(16);
#undef CS_GO
  return wl_check_launch();
}

}  // extern "C"
