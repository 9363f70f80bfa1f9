// Lexicon-constrained CTC beam search with a word n-gram LM (additive to ABI 30): the decoder of the reference's
// examples/speech_recognition/w2l_decoder.py with --lexicon (flashlight's LexiconDecoder, CTC criterion, log_add = false,
// SmearingMode::MAX), by the rules written out at ctc_lexicon.lexicon_beam_search_reference, which is this kernel's specification.
//
// One workgroup of 1024 lanes per utterance; frames are sequential.  R = beam, K = min(beam_tokens, C), `width` the caller's bound
// on one parent's candidates, cap = R x width <= 16384 the candidate capacity, tsize the power of two >= cap.
// LDS (dynamic, 12 cap + 4 tsize + 24 R + 4 + 8 C bytes up to cap = 8192: 148.0 KiB at cap = 8192, R = 512, C = 1024; above that
// -- the kernel's BIG instantiation -- cstate and cnt move to the HBM workspace and it is 4 cap + 4 tsize + ..., 148.0 KiB at cap
// = 16384.  Nothing is packed or truncated in either):
//   cscore fp32, cstate int32, cnt int32 [cap]   the frame's candidates: score, LM state, trie node | token << 21 (prev_blank is
//                                       token == blank, so (cstate, cnt) is the whole merge key).  Parent r's candidates stand at
//                                       poff[r] .. poff[r + 1) in (token, slot) order, so "parent rank ascending, token ascending,
//                                       slot ascending" is "index ascending"
//   table int32 [tsize]                 open-addressing hash table of the merge: a slot holds the best candidate of its key
//   bscore, bstate, bnode, btok [R]     the beam in rank order (btok: last token, 0xffff = none, bit 16 = prev_blank)
//   sel [R], poff [R + 1], em [C], isk [C]   selected candidates; candidate offsets; the frame's log-probabilities; considered?
// HBM workspace: the back-pointers, two ints per beam entry and frame (parent | token << 16, word or -1), and per candidate its word
// -- the one field of a candidate that only the back-pointer needs -- and, in BIG, cstate and cnt: one or three ints.  A
// workgroup reads there only what it wrote itself, behind a barrier.
// Per frame:
//   1. the frame's C logits to LDS; unless `normalized` their log-sum-exp is subtracted
//   2. lane c ranks class c by counting the classes that beat it (ties to the lower class): isk[c] = among the K best
//   3. lane r < beam entries counts parent r's candidates (lb_expand<false>: blank, repeat, root silence, and per considered
//      child of its node one descent if the child has children and one word per label, or <unk>); a block prefix sum gives poff;
//      the same walk writes them (lb_expand<true>), a word candidate walking the LM tables as the lexicon-free kernel does
//   4. the block maximum gives the threshold cut; every survivor is put into the hash table: an empty slot is claimed by
//      compare-and-swap, a slot of the same key keeps the better of the two in the total order (the outcome is the maximum,
//      whatever the order of arrival); after a barrier a candidate is alive if its key's slot holds it
//   5. - 7. as csrc/ctc_beam.hip: the R-th largest of the 46-bit keys bit by bit, compaction through an LDS counter, ranking by
//      counting; the parent of a selected candidate is found by binary search in poff
// At the end only the entries at the root finish if there is one (else all); lm_weight * lm(state, </s>) is added, they are
// ranked again (ties keep their rank), and lane h < nbest walks hypothesis h's back-pointers into tokens[b, h, :] and
// words[b, h, :], collapses the tokens and compacts the words.
// No global atomics (the LDS atomics count or take a maximum); nothing depends on B or on the sample's place in the batch.
// Every address is formed from a range-checked id: classes are below C, trie nodes, child and label ranges, words and LM states
// are clamped to the table sizes the caller states, candidate writes are checked against cap (reached only if `width` was not a
// bound: the host computes it from the lexicon), back-pointers are clamped to the beam.  Emissions must be finite.
#include "ctc_beam_common.hpp"
#include "../../include/wavlm_hip.h"

#define LB_MAXCAND 16384
#define LB_LDSCAND 8192        // up to here a candidate's state and node | token are kept in LDS, above in the workspace
#define LB_KEYBITS 14          // LB_MAXCAND = 2^14 candidate indices
#define LB_NODEBITS 21         // cnt = node | token << 21: nodes <= 2^21, tokens < 2^10
#define LB_MAXNODES (1 << LB_NODEBITS)
#define LB_NODEMASK (LB_MAXNODES - 1)

struct LbLex {
  const int* child_off; const int* child_tok; const int* child_node; const float* node_max;
  const int* label_off; const int* label_word;
  int n_nodes, n_children, n_labels, n_words, unk_word;
};

struct LbOpt {
  int C, blank, sil, has_lm, unk_on;
  float lmw, silw, wsc, usc;
};

static inline int lb_supported(int64_t C, int64_t beam, int64_t width, int64_t lm_order, int64_t nodes) {
  if (C < 1 || C > CB_MAXC || beam < 1 || beam > CB_MAXBEAM || width < 1 || lm_order < 0 || lm_order > CB_MAXORDER) return 0;
  if (nodes < 1 || nodes > LB_MAXNODES) return 0;
  return beam * width <= LB_MAXCAND;
}
static inline int lb_tsize(int cap) { int t = 2; while (t < cap) t <<= 1; return t; }
static inline size_t lb_lds_bytes(int R, int cap, int C) {
  return (cap > LB_LDSCAND ? 4 : 12) * (size_t)cap + 4 * (size_t)lb_tsize(cap) + 24 * (size_t)R + 4 + 8 * (size_t)C;
}
// ints per candidate in the workspace: its word, and above LB_LDSCAND its state and node | token
static inline int lb_cand_ints(int64_t cap) { return cap > LB_LDSCAND ? 3 : 1; }
static inline uint64_t lb_cand_bytes(int64_t B, int64_t cap) {
  return ((uint64_t)B * cap * 4 * lb_cand_ints(cap) + 255) & ~(uint64_t)255;
}
static inline uint64_t lb_bp_bytes(int64_t B, int64_t T, int64_t beam) { return ((uint64_t)B * T * beam * 8 + 255) & ~(uint64_t)255; }
// B x T frames up to 2^40 with beam <= 512 and cap <= 16384: every product above stays far below 2^64
static inline int lb_sizes_ok(int64_t B, int64_t T, int64_t beam, int64_t width) {
  return B >= 0 && T >= 0 && beam >= 1 && beam <= CB_MAXBEAM && width >= 1 && beam * width <= LB_MAXCAND && B * T <= ((int64_t)1 << 40);
}

__device__ __forceinline__ int lb_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__device__ __forceinline__ unsigned lb_hash(int state, int nt) {
  unsigned h = (unsigned)state * 0x9E3779B1u ^ ((unsigned)nt * 0x85EBCA77u);
  h ^= h >> 15; h *= 0x2C1B3C6Du; h ^= h >> 13;
  return h;
}

// The candidates of one beam entry (score sc, LM state st, trie node nd, last token, prev_blank) in (token, slot) order: their
// number; WRITE puts them at base .. (below cap) and keeps the maximum score in *best.
template <bool WRITE>
__device__ __forceinline__ int lb_expand(const LbLex& lx, const CbLm& lm, const LbOpt& o, const float* em, const int* isk, float sc,
    int st, int nd, int last, int pb, int base, int cap, float* cscore, int* cstate, int* cnt, int* cword, float* best) {
  int k = 0;
  auto emit = [&](float s, int state, int node, int n, int word) {
    if (WRITE) {
      const int i = base + k;
      if (i < cap) {
        cscore[i] = s; cstate[i] = state; cnt[i] = node | (n << LB_NODEBITS); cword[i] = word;
        *best = fmaxf(*best, s);
      }
    }
    ++k;
  };
  if ((unsigned)nd >= (unsigned)lx.n_nodes) nd = 0;
  const float lexmax = nd == 0 ? 0.0f : lx.node_max[nd];
  const int rep = (last != CB_NONE && !pb && last < o.C) ? last : -1;
  const int silr = (nd == 0 && o.sil >= 0 && o.sil < o.C && o.sil != o.blank && o.sil != rep) ? o.sil : -1;
  int done = -1;   // the largest special token (blank, repeat, root silence) emitted so far
  auto flush = [&](int limit) {
    for (int it = 0; it < 3; ++it) {
      int m = 0x7fffffff;
      if (o.blank > done && o.blank < m) m = o.blank;
      if (rep > done && rep < m) m = rep;
      if (silr > done && silr < m) m = silr;
      if (m >= limit) break;
      emit(sc + em[m] + (m == o.sil ? o.silw : 0.0f), st, nd, m, -1);   // same state and node
      done = m;
    }
  };
  const int lo = lb_clamp(lx.child_off[nd], 0, lx.n_children), hi = lb_clamp(lx.child_off[nd + 1], lo, lx.n_children);
  for (int e = lo; e < hi; ++e) {
    const int n = lx.child_tok[e];
    if ((unsigned)n >= (unsigned)o.C) continue;
    flush(n);
    if (n == o.blank || n == rep || n == silr || !isk[n]) continue;
    const int c = lx.child_node[e];
    if (c < 1 || c >= lx.n_nodes) continue;
    const float s = sc + em[n] + (n == o.sil ? o.silw : 0.0f);
    const int clo = lb_clamp(lx.child_off[c], 0, lx.n_children), chi = lb_clamp(lx.child_off[c + 1], clo, lx.n_children);
    if (chi > clo) emit(s + o.lmw * (lx.node_max[c] - lexmax), st, c, n, -1);
    const int llo = lb_clamp(lx.label_off[c], 0, lx.n_labels), lhi = lb_clamp(lx.label_off[c + 1], llo, lx.n_labels);
    const int nl = lhi > llo ? lhi - llo : (o.unk_on ? 1 : 0);
    for (int q = 0; q < nl; ++q) {
      int w = lhi > llo ? lx.label_word[llo + q] : lx.unk_word;
      if ((unsigned)w >= (unsigned)lx.n_words) w = lx.unk_word;
      float l = 0.0f;
      int st2 = st;
      if (WRITE && o.has_lm) l = cb_lm(lm, st, lm.tok_word[w], &st2);
      emit(s + o.lmw * (l - lexmax) + (lhi > llo ? o.wsc : o.usc), st2, 0, n, w);
    }
  }
  flush(0x7fffffff);
  return k;
}

template <bool BIG>
__global__ __launch_bounds__(CB_NT) void ctc_lexbeam_kernel(const void* __restrict__ x, int dt, long sb, long st, int T,
    const int* __restrict__ in_len, int normalized, CbLm lm, LbLex lx, LbOpt o, int R, int K, int cap, int tsize, float thr,
    int nbest, int* tokens, int* counts, float* scores, int* n_hyp, int* words, int* word_counts, int* ws_bp, int* ws_cand) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __shared__ float s_red[CB_NT / 64];
  __shared__ int s_wsum[CB_NT / 64];
  __shared__ int s_cnt[64];   // 0: alive, 1: selected, 2 + k: step k of the bit search
  const int C = o.C, blank = o.blank;
  float* cscore = (float*)smem;
  int* const cword = ws_cand + (size_t)blockIdx.x * (BIG ? 3 : 1) * cap;
  int* const cstate = BIG ? cword + cap : (int*)(cscore + cap);
  int* const cnt = cstate + cap;
  int* table = BIG ? (int*)(cscore + cap) : cnt + cap;
  float* bscore = (float*)(table + tsize);
  int* bstate = (int*)(bscore + R);
  int* bnode = bstate + R;
  int* btok = bnode + R;
  int* sel = btok + R;
  int* poff = sel + R;
  float* em = (float*)(poff + R + 1);
  int* isk = (int*)(em + C);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x;
  const int Tb = ct_len(in_len, b, T);
  int* bp = ws_bp + (size_t)b * T * R * 2;

  if (tid == 0) {
    bscore[0] = 0.0f;
    bstate[0] = o.has_lm ? lm.start : 0;
    bnode[0] = 0;
    btok[0] = CB_NONE;
  }
  int nb = 1;   // entries in the beam (uniform)
  __syncthreads();

  for (int t = 0; t < Tb; ++t) {
    // 1. emissions
    const long xt = (long)b * sb + (long)t * st;
    float v = -INFINITY;
    if (tid < C) v = ld_elem(x, xt + tid, dt);
    if (tid < 64) s_cnt[tid] = 0;
    for (int i = tid; i < tsize; i += CB_NT) table[i] = -1;
    if (!normalized) {
      const float m = cb_block<true>(v, s_red);
      const float sum = cb_block<false>(tid < C ? expf(v - m) : 0.0f, s_red);
      v -= m + logf(sum);
    }
    if (tid < C) em[tid] = v;
    __syncthreads();
    // 2. the K best classes
    if (tid < C) {
      int rank = 0;
      for (int c = 0; c < C; ++c) {
        const float u = em[c];
        rank += (u > v || (u == v && c < tid)) ? 1 : 0;
      }
      isk[tid] = rank < K ? 1 : 0;
    }
    __syncthreads();
    // 3. candidates: count, prefix sum, write
    float sc = 0.0f;
    int hst = 0, hnd = 0, hlast = CB_NONE, hpb = 0, mine = 0;
    if (tid < nb) {
      sc = bscore[tid]; hst = bstate[tid]; hnd = bnode[tid];
      const int tp = btok[tid];
      hlast = tp & 0xffff; hpb = tp >> 16;
      mine = lb_expand<false>(lx, lm, o, em, isk, sc, hst, hnd, hlast, hpb, 0, 0, cscore, cstate, cnt, cword, nullptr);
    }
    int incl = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int u = __shfl_up(incl, d, 64);
      if (lane >= d) incl += u;
    }
    if (lane == 63) s_wsum[wave] = incl;
    __syncthreads();
    int base = incl - mine, total = 0;
    for (int w = 0; w < CB_NT / 64; ++w) {
      const int u = s_wsum[w];
      if (w < wave) base += u;
      total += u;
    }
    if (tid < nb) poff[tid] = base < cap ? base : cap;
    const int N = total < cap ? total : cap;
    if (tid == 0) poff[nb] = N;
    float best = -INFINITY;
    if (tid < nb) lb_expand<true>(lx, lm, o, em, isk, sc, hst, hnd, hlast, hpb, base, cap, cscore, cstate, cnt, cword, &best);
    best = cb_block<true>(best, s_red);   // (its barriers publish the candidates and poff)
    // 4. threshold and merge
    const float cut = best - thr;
    for (int i = tid; i < N; i += CB_NT) {
      const float s = cscore[i];
      if (!(s >= cut)) continue;
      const int state = cstate[i], nt = cnt[i];
      unsigned h = lb_hash(state, nt) & (unsigned)(tsize - 1);
      for (int probe = 0; probe < tsize; ++probe) {
        int j = __atomic_load_n(&table[h], __ATOMIC_RELAXED);
        if (j < 0) {
          j = atomicCAS(&table[h], -1, i);
          if (j < 0) break;                       // claimed
        }
        j = lb_clamp(j, 0, N - 1);
        if (cstate[j] == state && cnt[j] == nt) {   // the key's slot: the better of its holder and i stays
          for (int guard = 0; guard < LB_MAXCAND; ++guard) {
            const float sj = cscore[j];
            if (sj > s || (sj == s && j < i)) break;
            const int old = atomicCAS(&table[h], j, i);
            if (old == j) break;
            j = lb_clamp(old, 0, N - 1);
          }
          break;
        }
        h = (h + 1) & (unsigned)(tsize - 1);
      }
    }
    __syncthreads();
    {
      int alive = 0;
      for (int i = tid; i < N; i += CB_NT) {
        const float s = cscore[i];
        bool keep = false;
        if (s >= cut) {
          const int state = cstate[i], nt = cnt[i];
          unsigned h = lb_hash(state, nt) & (unsigned)(tsize - 1);
          for (int probe = 0; probe < tsize; ++probe) {
            const int j = table[h];
            if (j < 0) break;
            if (j == i) { keep = true; break; }
            const int jj = lb_clamp(j, 0, N - 1);
            if (cstate[jj] == state && cnt[jj] == nt) break;
            h = (h + 1) & (unsigned)(tsize - 1);
          }
        }
        if (keep) ++alive; else cscore[i] = -INFINITY;   // (only lane i's owner reads or writes cscore[i] in this pass)
      }
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) alive += __shfl_xor(alive, d, 64);
      if (lane == 0 && alive) atomicAdd(&s_cnt[0], alive);
    }
    __syncthreads();
    // 5. the R-th largest key
    unsigned long long kth = 1ull;
    if (s_cnt[0] > R) kth = cb_kth<LB_KEYBITS>(cscore, N, R, s_cnt + 2);
    // 6. compaction
    for (int i = tid; i < N; i += CB_NT) {
      const unsigned long long key = cb_key<LB_KEYBITS>(cscore[i], i);
      if (key != 0ull && key >= kth) {
        const int slot = atomicAdd(&s_cnt[1], 1);
        if (slot < R) sel[slot] = i;
      }
    }
    __syncthreads();
    const int nsel = s_cnt[1] < R ? s_cnt[1] : R;
    // 7. rank, the new beam and its back-pointers
    int rank = 0, par = 0, i7 = 0;
    if (tid < nsel) {
      i7 = sel[tid];
      const unsigned long long key = cb_key<LB_KEYBITS>(cscore[i7], i7);
      for (int q = 0; q < nsel; ++q) {
        const int iq = sel[q];
        rank += cb_key<LB_KEYBITS>(cscore[iq], iq) > key ? 1 : 0;
      }
      int lo = 0, hi = nb;                         // the last r with poff[r] <= i7
      while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (poff[mid] <= i7) lo = mid; else hi = mid;
      }
      par = lo;
    }
    __syncthreads();                               // the old beam and poff have been read
    if (tid < nsel) {
      const int nt = cnt[i7], n = (nt >> LB_NODEBITS) & 0x3ff;
      bscore[rank] = cscore[i7];
      bstate[rank] = cstate[i7];
      bnode[rank] = nt & LB_NODEMASK;
      btok[rank] = n | (n == blank ? 0x10000 : 0);
      bp[((size_t)t * R + rank) * 2] = par | (n << 16);
      bp[((size_t)t * R + rank) * 2 + 1] = cword[i7];
    }
    nb = nsel;
    __syncthreads();
  }

  // the end: the entries at the root if there is one, the end score, the final order and the n-best
  const int at_root = __syncthreads_or(tid < nb && bnode[tid] == 0 ? 1 : 0);
  const bool fin = tid < nb && (!at_root || bnode[tid] == 0);
  if (tid < nb) {
    float s = -INFINITY;
    if (fin) {
      s = bscore[tid];
      if (o.has_lm) {
        int unused;
        s += o.lmw * cb_lm(lm, bstate[tid], lm.eos_word, &unused);
      }
    }
    cscore[tid] = s;
  }
  const int nfin = __syncthreads_count(fin ? 1 : 0);
  if (fin) {
    const float s = cscore[tid];
    int rank = 0;
    for (int q = 0; q < nb; ++q) {
      const float u = cscore[q];
      rank += (u > s || (u == s && q < tid)) ? 1 : 0;
    }
    if (rank < nbest) sel[rank] = tid;
  }
  __syncthreads();
  const int nh = nfin < nbest ? nfin : nbest;
  if (tid == 0) n_hyp[b] = nh;
  if (tid < nbest) {
    int* tk = tokens + ((size_t)b * nbest + tid) * T;
    int* wd = words + ((size_t)b * nbest + tid) * T;
    int cn = 0, wn = 0;
    float score = -INFINITY;
    if (tid < nh) {
      int cur = sel[tid];
      score = cscore[cur];
      for (int t = Tb - 1; t >= 0; --t) {
        if (cur >= R) cur = R - 1;
        const int w = bp[((size_t)t * R + cur) * 2];
        tk[t] = (w >> 16) & 0xffff;
        wd[t] = bp[((size_t)t * R + cur) * 2 + 1];
        cur = w & 0xffff;
      }
      int last = -1;
      for (int t = 0; t < Tb; ++t) {
        const int a = tk[t], w = wd[t];
        if (a != last && a != blank) tk[cn++] = a;
        if (w >= 0) wd[wn++] = w;
        last = a;
      }
    }
    for (int t = cn; t < T; ++t) tk[t] = -1;
    for (int t = wn; t < T; ++t) wd[t] = -1;
    counts[(size_t)b * nbest + tid] = cn;
    word_counts[(size_t)b * nbest + tid] = wn;
    scores[(size_t)b * nbest + tid] = score;
  }
}

extern "C" {

int wavlm_ctc_lexbeam_supported(int32_t C, int32_t beam, int32_t width, int32_t lm_order, int32_t lex_nodes) {
  return lb_supported(C, beam, width, lm_order, lex_nodes);
}

uint64_t wavlm_ctc_lexbeam_workspace_bytes(int32_t B, int32_t T, int32_t beam, int32_t width) {
  if (!lb_sizes_ok(B, T, beam, width)) return 0;   // also what wavlm_ctc_lexbeam refuses
  return lb_bp_bytes(B, T, beam) + lb_cand_bytes(B, (int64_t)beam * width);
}

int wavlm_ctc_lexbeam(const void* logits, int32_t dtype, int64_t stride_b, int64_t stride_t, int32_t B, int32_t T, int32_t C,
                      const int32_t* input_lengths, int32_t blank, int32_t sil, int32_t normalized, const int32_t* lm_child_off,
                      const int32_t* lm_child_word, const float* lm_child_logp, const int32_t* lm_child_next,
                      const float* lm_node_backoff, const int32_t* lm_node_suffix, const int32_t* lm_tok_word, int32_t lm_nodes,
                      int32_t lm_children, int32_t lm_start, int32_t lm_eos_word, int32_t lm_order,
                      const int32_t* lex_child_off, const int32_t* lex_child_tok, const int32_t* lex_child_node,
                      const float* lex_node_max, const int32_t* lex_label_off, const int32_t* lex_label_word, int32_t lex_nodes,
                      int32_t lex_children, int32_t lex_labels, int32_t lex_words, int32_t lex_width, int32_t unk_word,
                      int32_t beam, int32_t beam_tokens, float beam_threshold, float lm_weight, float word_score, float unk_score,
                      float sil_weight, int32_t nbest, int32_t* tokens, int32_t* counts, float* scores, int32_t* n_hyp,
                      int32_t* words, int32_t* word_counts, void* workspace, uint64_t ws_bytes, void* stream) {
  if (dtype != WL_F32 && dtype != WL_BF16) return WL_EINVAL;
  if (B < 0 || T < 1 || T > 0x0fffffff || blank < 0 || blank >= C || beam_tokens < 1) return WL_EINVAL;
  if (!lb_supported(C, beam, lex_width, lm_order, lex_nodes) || !lb_sizes_ok(B, T, beam, lex_width)) return WL_EINVAL;
  if (nbest < 1 || nbest > beam || !(beam_threshold >= 0.0f) || !isfinite(lm_weight) || !isfinite(sil_weight)) return WL_EINVAL;
  if (!isfinite(word_score) || !(isfinite(unk_score) || unk_score == -INFINITY)) return WL_EINVAL;
  if (lm_nodes < 0 || lm_children < 0 || (lm_nodes > 0) != (lm_order > 0)) return WL_EINVAL;
  if (lex_children < 0 || lex_labels < 0 || lex_words < 1 || unk_word < 0 || unk_word >= lex_words) return WL_EINVAL;
  if (!lex_child_off || !lex_child_tok || !lex_child_node || !lex_node_max || !lex_label_off || !lex_label_word) return WL_EINVAL;
  if (lm_nodes > 0) {
    if (!lm_child_off || !lm_child_word || !lm_child_logp || !lm_child_next || !lm_node_backoff || !lm_node_suffix || !lm_tok_word)
      return WL_EINVAL;
    if (lm_start < 0 || lm_start >= lm_nodes || lm_eos_word < 0) return WL_EINVAL;
  }
  if (B == 0) return WL_OK;
  if (!logits || !input_lengths || !tokens || !counts || !scores || !n_hyp || !words || !word_counts) return WL_EINVAL;
  if (!ct_view_ok(B, T, C, stride_b, stride_t)) return WL_EINVAL;
  if (!workspace || ws_bytes < wavlm_ctc_lexbeam_workspace_bytes(B, T, beam, lex_width) || ((uintptr_t)workspace & 3))
    return WL_EINVAL;
  const int K = (int)(beam_tokens < C ? beam_tokens : C);
  const int cap = (int)beam * (int)lex_width, tsize = lb_tsize(cap);
  const size_t lds = lb_lds_bytes(beam, cap, C);
  const bool big = cap > LB_LDSCAND;
  const void* fn = big ? (const void*)ctc_lexbeam_kernel<true> : (const void*)ctc_lexbeam_kernel<false>;
  if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) return WL_ELAUNCH;
  CbLm lm = {lm_child_off, lm_child_word, lm_child_logp, lm_child_next, lm_node_backoff, lm_node_suffix, lm_tok_word,
             (int)lm_nodes, (int)lm_children, (int)lm_start, (int)lm_eos_word};
  LbLex lx = {lex_child_off, lex_child_tok, lex_child_node, lex_node_max, lex_label_off, lex_label_word,
              (int)lex_nodes, (int)lex_children, (int)lex_labels, (int)lex_words, (int)unk_word};
  LbOpt o = {(int)C, (int)blank, (int)sil, lm_nodes > 0 ? 1 : 0, unk_score > -INFINITY ? 1 : 0,
             lm_weight, sil_weight, word_score, unk_score > -INFINITY ? unk_score : 0.0f};
  int* bp = (int*)workspace;
  int* cw = (int*)((char*)workspace + lb_bp_bytes(B, T, beam));
#define LB_GO(BIG)                                                                                                          \
  WL_LAUNCH(ctc_lexbeam_kernel<BIG>, dim3((unsigned)B), dim3(CB_NT), lds, (hipStream_t)stream, logits, (int)dtype,             \
            (long)stride_b, (long)stride_t, (int)T, input_lengths, normalized ? 1 : 0, lm, lx, o, (int)beam, K, cap, tsize,    \
            beam_threshold, (int)nbest, tokens, counts, scores, n_hyp, words, word_counts, bp, cw)
  if (big) LB_GO(true); else LB_GO(false);
#undef LB_GO
  return wl_check_launch();
}

}  // extern "C"
