// What csrc/ctc_beam.hip (wavlm_ctc_beam) and csrc/ctc_lexbeam.hip (wavlm_ctc_lexbeam) share: the walk of the n-gram tables, the
// block reductions in a fixed order, the monotonic key of the total order and the bit-by-bit search of the R-th largest key.
// A workgroup is CB_NT = 1024 lanes in both.
#pragma once
#include "ctc_decode.hpp"

#define CB_NT 1024
#define CB_MAXC 1024
#define CB_MAXBEAM 512
#define CB_MAXORDER 6
#define CB_NONE 0xffff

struct CbLm {
  const int* child_off; const int* child_word; const float* child_logp; const int* child_next;
  const float* node_backoff; const int* node_suffix; const int* tok_word;
  int n_nodes, n_children, start, eos_word;
};

// log10 p(word | node) and the state after it
__device__ __forceinline__ float cb_lm(const CbLm& lm, int node, int word, int* next) {
  float acc = 0.0f;
  for (int level = 0; level < 8; ++level) {
    if ((unsigned)node >= (unsigned)lm.n_nodes) node = 0;
    int lo = lm.child_off[node], hi = lm.child_off[node + 1];
    lo = lo < 0 ? 0 : (lo > lm.n_children ? lm.n_children : lo);
    hi = hi < lo ? lo : (hi > lm.n_children ? lm.n_children : hi);
    const int end = hi;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (lm.child_word[mid] < word) lo = mid + 1; else hi = mid;
    }
    if (lo < end && lm.child_word[lo] == word) {
      const int nx = lm.child_next[lo];
      *next = (unsigned)nx < (unsigned)lm.n_nodes ? nx : 0;
      return acc + lm.child_logp[lo];
    }
    if (node == 0) break;
    acc += lm.node_backoff[node];
    node = lm.node_suffix[node];
  }
  *next = 0;
  return acc;
}

// the value of every lane's v combined over the workgroup, the 16 wave results in a fixed order; s_red: 16 floats
template <bool MAX>
__device__ __forceinline__ float cb_block(float v, float* s_red) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const float u = __shfl_xor(v, o, 64);
    v = MAX ? fmaxf(v, u) : v + u;
  }
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
  __syncthreads();
  float r = s_red[0];
#pragma unroll
  for (int k = 1; k < CB_NT / 64; ++k) r = MAX ? fmaxf(r, s_red[k]) : r + s_red[k];
  __syncthreads();
  return r;
}

// 32 + BITS bits: larger = earlier in the total order (score descending, candidate index ascending, i < 2^BITS); 0 = dead
template <int BITS>
__device__ __forceinline__ unsigned long long cb_key(float s, int i) {
  if (!(s > -INFINITY)) return 0ull;
  unsigned u = s == 0.0f ? 0u : __float_as_uint(s);
  u = (u >> 31) ? ~u : (u | 0x80000000u);
  return ((unsigned long long)u << BITS) | (unsigned)((1 << BITS) - 1 - i);
}

// The R-th largest key of the N candidates whose scores are in LDS (dead ones at -inf), found bit by bit, each step a block
// count.  Keys are unique, so `key >= result` takes exactly R.  Called by every lane when more than R candidates are alive;
// s_cnt: 32 + BITS ints of LDS, zero on entry
template <int BITS>
__device__ __forceinline__ unsigned long long cb_kth(const float* cscore, int N, int R, int* s_cnt) {
  const int tid = threadIdx.x, lane = tid & 63;
  unsigned long long kth = 0ull;
  for (int bit = 31 + BITS; bit >= 0; --bit) {
    const unsigned long long trial = kth | (1ull << bit);
    int c = 0;
    for (int i = tid; i < N; i += CB_NT) c += cb_key<BITS>(cscore[i], i) >= trial ? 1 : 0;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) c += __shfl_xor(c, o, 64);
    if (lane == 0 && c) atomicAdd(&s_cnt[31 + BITS - bit], c);
    __syncthreads();
    if (s_cnt[31 + BITS - bit] >= R) kth = trial;
  }
  return kth;
}
