// What csrc/ctc.hip (wavlm_ctc_greedy) and csrc/ctc_score.hip (wavlm_ctc_score) share: the greedy decode of one sample by one
// workgroup, the clamp of an input length and the check of the logits view.
#pragma once
#include "common.hpp"
#include <math.h>

#define CT_NT 256

__device__ __forceinline__ int ct_len(const int* __restrict__ in_len, int b, int T) {
  const int v = in_len[b];
  return v < 0 ? 0 : (v > T ? T : v);
}

// the B x T x C view with unit class stride must not overlap itself: rows apart by at least C along one axis, samples (or frames)
// apart by at least the other axis's whole extent
static inline int ct_view_ok(int64_t B, int64_t T, int64_t C, int64_t sb, int64_t st) {
  if (sb < 0 || st < 0) return 0;
  if (B > 1 && T > 1) return (st >= C && sb >= T * st) || (sb >= C && st >= B * sb);
  if (T > 1) return st >= C;
  if (B > 1) return sb >= C;
  return 1;
}

// Sample b by the whole workgroup of CT_NT lanes: argmax per frame (ties to the lowest class), repeats collapsed, blanks dropped.
// tokens[b, 0 .. cnt) is the decode, -1 behind it; counts[b] = cnt, which is returned to every lane.  s_arg: CT_NT ints of LDS,
// s_state: 2.  The decode is visible to the whole workgroup on return (the last write of it is followed by a barrier); the -1 fill
// is not.
__device__ __forceinline__ int ct_greedy_sample(const void* __restrict__ x, int dt, long sb, long st, int T, int C,
    const int* __restrict__ in_len, int blank, int* tokens, int* counts, int b, int* s_arg, int* s_state) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int Tb = ct_len(in_len, b, T);
  const long xb = (long)b * sb;
  int* tok = tokens + (long)b * T;
  if (tid == 0) { s_state[0] = 0; s_state[1] = -1; }   // tokens written so far, the last frame's class
  __syncthreads();
  for (int t0 = 0; t0 < Tb; t0 += CT_NT) {   // a chunk of CT_NT frames: a wave takes a frame at a time
    const int n = Tb - t0 < CT_NT ? Tb - t0 : CT_NT;
    for (int f = wave; f < n; f += CT_NT / 64) {
      const long xt = xb + (long)(t0 + f) * st;
      float best = -INFINITY;
      int arg = -1;                          // a lane without a class (C < 64) stays at -1
      for (int c = lane; c < C; c += 64) {   // ascending c per lane: the first maximum stays
        const float v = ld_elem(x, xt + c, dt);
        if (arg < 0 || v > best) { best = v; arg = c; }
      }
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) {
        const float ob = __shfl_xor(best, o, 64);
        const int oa = __shfl_xor(arg, o, 64);
        if (oa >= 0 && (arg < 0 || ob > best || (ob == best && oa < arg))) { best = ob; arg = oa; }
      }
      if (lane == 0) s_arg[f] = arg;
    }
    __syncthreads();
    if (tid == 0) {   // the collapse is sequential in t: at most CT_NT steps per chunk on one lane
      int base = s_state[0], last = s_state[1];
      for (int f = 0; f < n; ++f) {
        const int a = s_arg[f];
        if (a != last && a != blank) tok[base++] = a;
        last = a;
      }
      s_state[0] = base; s_state[1] = last;
    }
    __syncthreads();
  }
  const int cnt = s_state[0];
  for (int t = cnt + tid; t < T; t += CT_NT) tok[t] = -1;
  if (tid == 0) counts[b] = cnt;
  return cnt;
}
