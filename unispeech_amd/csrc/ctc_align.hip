// CTC forced alignment (additive to ABI 30): the best path of a transcript through the emissions, its frames, the span and the
// score of every label.  The max-plus twin of csrc/ctc.hip's alpha recursion, with back-pointers and a back-trace.
//
// With l' the extended target (blank, l_0, blank, ..., l_(L-1), blank: S = 2 L + 1 positions), x the RAW logits and
// skip(s) = s odd and l'_s != l'_(s-2), in float64:
//   v_0(s) = x[0, l'_s] for s < 2, else -inf
//   v_t(s) = max(v_(t-1)(s), v_(t-1)(s-1), skip(s) ? v_(t-1)(s-2) : -inf) + x[t, l'_s]
//   end    = the better of v_(Tb-1)(S-1) and v_(Tb-1)(S-2)                            Tb = the sample's input length
// The log-softmax is not needed to find the path (every path takes one class per frame, so lse[t] shifts all of them alike); it
// enters only the reported scores, lp[t, c] = x[t, c] - lse[t].  max is exact and every v is ONE float64 addition of two
// operands that the host restatement (unispeech_amd.ctc_align.forced_align_reference) adds too, so the path is the
// reference's bit for bit, ties included.  Ties: the predecessor with the larger s wins (stay over s - 1 over s - 2), and at the
// end S - 1 wins over S - 2.
//
// Two launches, no global atomics.
//  (a) al_lse_kernel: one wave per (b, t) row, float64 -- the arithmetic of ctc.hip's ctc_lse_kernel (that file's helpers are
//      local to it and it is left as it stands, hence the copy of its exponential here).
//  (b) ctc_align_kernel: one workgroup per sample.
//      forward     lanes over the extended positions, PER = 1, 2, 4 or 8 per lane, the previous column twice in LDS (frame
//                  parity picks the buffer): one barrier per frame, the next frame's logits loaded a frame ahead -- the layout of
//                  ctc_alpha_kernel; a lane's reads of the old column are all issued before the first is used.
//                  The choice of predecessor is 2 bits per (t, s): a wave's 64 positions give two ballots, low
//                  bits and high bits, which lane 0 stores as one 16-byte group of the frame's row in the workspace.
//      back-trace  a chain of Tb dependent steps on one lane.  The rows are staged into LDS AL_BLK frames at a time -- every
//                  lane loads its part of the NEXT block into registers before the walk of the current one starts -- so the walk
//                  reads LDS, not HBM.  It writes frames[] and, into LDS, each label's first and one-past-last frame.
//      sums        256 frames at a time: every lane computes lp[t, path_t] of one frame into LDS; then lanes over the labels add
//                  their span's part of the chunk, and one lane adds the whole chunk to the score: ascending t throughout,
//                  float64, one rounding to fp32 at the end.
// Nothing depends on B, on the sample's place in the batch or on the other samples.
#include "ctc_decode.hpp"
#include "../../include/wavlm_hip.h"

#define AL_MAXL 1023                 // labels per sample
#define AL_SP 2048                   // extended positions, padded (2 * AL_MAXL + 1 = 2047)
#define AL_MAXG (AL_SP / 64)         // 16-byte groups (64 positions x 2 bits) in a row of back-pointers
#define AL_BLK WAVLM_CTC_ALIGN_BLOCK // frames of back-pointers staged into LDS at a time

static inline int al_supported(int64_t Lmax) { return Lmax >= 0 && Lmax <= AL_MAXL; }
static inline uint64_t al_align(uint64_t v) { return (v + 255) & ~(uint64_t)255; }
static inline int al_groups(int64_t Lmax) { return (int)((2 * Lmax + 1 + 63) / 64); }
// workspace: ticks uint64 [B, 4] | lse double [B, T] | back-pointers uint4 [B, T, groups(Lmax)]
struct al_ws { uint64_t ticks, lse, bp, total; };
static inline al_ws al_carve(int64_t B, int64_t T, int64_t Lmax) {
  al_ws w;
  w.ticks = 0;
  w.lse = al_align((uint64_t)B * 32);
  w.bp = w.lse + al_align((uint64_t)B * (uint64_t)T * 8);
  w.total = w.bp + al_align((uint64_t)B * (uint64_t)T * (uint64_t)al_groups(Lmax) * 16);
  return w;
}

// ctc.hip's ct_exp: exp(x) for x <= 1 or so to 1e-14 relative (0 below -60)
__device__ __forceinline__ double al_exp(double x) {
  if (!(x > -60.0)) return x != x ? x : 0.0;
  const double n = rint(x * 1.4426950408889634074);
  const double u = fma(-n, 0.69314718055994530942, x);
  double p = 1.0 / 39916800.0;
  p = fma(p, u, 1.0 / 3628800.0);
  p = fma(p, u, 1.0 / 362880.0);
  p = fma(p, u, 1.0 / 40320.0);
  p = fma(p, u, 1.0 / 5040.0);
  p = fma(p, u, 1.0 / 720.0);
  p = fma(p, u, 1.0 / 120.0);
  p = fma(p, u, 1.0 / 24.0);
  p = fma(p, u, 1.0 / 6.0);
  p = fma(p, u, 0.5);
  p = fma(p, u, 1.0);
  p = fma(p, u, 1.0);
  return ldexp(p, (int)n);
}

template <int DT> __device__ __forceinline__ float al_ld(const void* p, long i) {
  return DT == WL_F32 ? ((const float*)p)[i] : bf2f(((const bf16_t*)p)[i]);
}

// ---- (a) lse[b, t] = log sum_c exp x[b, t, c]; rows at or beyond the input length are skipped (never read) ----
__global__ __launch_bounds__(CT_NT) void al_lse_kernel(const void* __restrict__ x, int dt, long sb, long st, long rows, int T,
    int C, const int* __restrict__ in_len, double* __restrict__ lse) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * (CT_NT / 64) + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int b = (int)(row / T), t = (int)(row - (long)b * T);
  if (t >= ct_len(in_len, b, T)) return;
  const long base = (long)b * sb + (long)t * st;
  float m = -INFINITY;
  for (int c = lane; c < C; c += 64) m = fmaxf(m, ld_elem(x, base + c, dt));
  m = wave_max(m);
  double s = 0.0;
  for (int c = lane; c < C; c += 64) s += al_exp((double)ld_elem(x, base + c, dt) - (double)m);
  s = wave_sum_d(s);
  if (lane == 0) lse[row] = (double)m + log(s);
}

// ---- (b) forward with back-pointers, back-trace, per-label and total sums ----
template <int PER, int DT>
__global__ __launch_bounds__(CT_NT) void ctc_align_kernel(const void* __restrict__ x, long sb, long st, int T, int C,
    const int* __restrict__ targets, const int* __restrict__ toff, int ntgt, const int* __restrict__ in_len, int blank, int Lmax,
    const double* __restrict__ lse, uint4* bp, int* frames, int* __restrict__ spans, float* __restrict__ tscores,
    float* __restrict__ score, unsigned long long* __restrict__ ticks) {
  constexpr int LPER = PER >= 2 ? PER / 2 : 1;   // labels per lane in the sums, and 16-byte groups per lane of a staged block
  __shared__ double s_v[2][AL_SP];
  __shared__ uint4 s_bp[AL_BLK * AL_MAXG];
  __shared__ double s_lp[CT_NT];
  __shared__ int s_span[2][AL_MAXL + 1];
  __shared__ int s_bad, s_end;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x;
  int* fr = frames + (long)b * T;
  int* sp = spans + (long)b * Lmax * 2;
  float* ts = tscores + (long)b * Lmax;
  unsigned long long* tk = ticks + (long)b * 4;
  const unsigned long long tick0 = wall_clock64();

  // the sample's labels: offsets and classes in range, or the sample is refused (NaN)
  const int o0 = toff[b], o1 = toff[b + 1];
  const bool ok = o0 >= 0 && o1 >= o0 && o1 <= ntgt && o1 - o0 <= Lmax;
  const int L = ok ? o1 - o0 : 0;
  if (tid == 0) { s_bad = ok ? 0 : 1; s_end = -1; }
  for (int j = tid; j <= AL_MAXL; j += CT_NT) { s_span[0][j] = -1; s_span[1][j] = -1; }
  __syncthreads();
  for (int j = tid; j < L; j += CT_NT) {
    const int lab = targets[o0 + j];
    if (lab < 0 || lab >= C) s_bad = 1;
  }
  __syncthreads();
  const bool good = s_bad == 0;
  const int S = 2 * L + 1;
  const int Tb = good ? ct_len(in_len, b, T) : 0;
  const int G = (2 * Lmax + 1 + 63) >> 6;
  const long xb = (long)b * sb;
  const double* lse_b = lse + (long)b * T;
  uint4* bpb = bp + (size_t)b * T * G;

  if (Tb > 0) {
    int lab[PER];
    bool skip[PER];
    float nxt[PER];   // x[t + 1, l'_s], loaded a frame ahead
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const int s = tid + k * CT_NT;
      lab[k] = 0; skip[k] = false; nxt[k] = 0.f;
      if (s < S) {
        lab[k] = (s & 1) ? targets[o0 + (s >> 1)] : blank;
        skip[k] = (s & 1) && s >= 2 && lab[k] != targets[o0 + (s >> 1) - 1];
        s_v[0][s] = s < 2 ? (double)al_ld<DT>(x, xb + lab[k]) : -INFINITY;
        if (Tb > 1) nxt[k] = al_ld<DT>(x, xb + st + lab[k]);
      }
    }
    __syncthreads();
    for (int t = 1; t < Tb; ++t) {
      const double* prv = s_v[(t & 1) ^ 1];
      double* cur = s_v[t & 1];
      // the next frame's loads: every lane, no branch (an idle lane reads class 0, the last frame reads itself again)
      float raw[PER];
      const long xn = xb + (long)(t + 1 < Tb ? t + 1 : t) * st;
#pragma unroll
      for (int k = 0; k < PER; ++k) { raw[k] = nxt[k]; nxt[k] = al_ld<DT>(x, xn + lab[k]); }
      // all reads of the old column first, none under a condition: one LDS round trip per frame, not one per position
      double p0[PER], p1[PER], p2[PER];
#pragma unroll
      for (int k = 0; k < PER; ++k) {
        const int s = tid + k * CT_NT;   // below AL_SP: the reads stay inside the column, what lies beyond S is not used
        p0[k] = prv[s];
        p1[k] = prv[s >= 1 ? s - 1 : 0];
        p2[k] = prv[s >= 2 ? s - 2 : 0];
      }
#pragma unroll
      for (int k = 0; k < PER; ++k) {
        const int s = tid + k * CT_NT;
        const bool in = s < S;
        const double a0 = p0[k];
        const double a1 = s >= 1 ? p1[k] : -INFINITY;
        const double a2 = skip[k] ? p2[k] : -INFINITY;
        double best = a0;
        int code = 0;                    // ties: stay over s - 1 over s - 2
        if (a1 > best) { best = a1; code = 1; }
        if (a2 > best) { best = a2; code = 2; }
        if (!in) code = 0;
        if (in) cur[s] = best + (double)raw[k];
        const unsigned long long lo = __ballot(code & 1), hi = __ballot(code & 2);
        const int g = k * (CT_NT / 64) + wave;   // positions 64 g .. 64 g + 63
        if (lane == 0 && g < G)
          bpb[(size_t)t * G + g] = make_uint4((unsigned)lo, (unsigned)(lo >> 32), (unsigned)hi, (unsigned)(hi >> 32));
      }
      __syncthreads();
    }
    if (tid == 0) {
      const double* fin = s_v[(Tb - 1) & 1];
      int e = S - 1;                     // ties: S - 1 over S - 2
      if (S > 1 && fin[S - 2] > fin[S - 1]) e = S - 2;
      s_end = fin[e] > -INFINITY ? e : -1;
    }
    __syncthreads();
  }

  if (s_end < 0) {
    // no alignment (-inf), no frame (0 for the empty target, else -inf) or a sample that was refused (NaN)
    for (int t = tid; t < T; t += CT_NT) fr[t] = -2;
    for (int j = tid; j < Lmax; j += CT_NT) { sp[2 * j] = -1; sp[2 * j + 1] = -1; ts[j] = 0.f; }
    if (tid == 0) {
      score[b] = !good ? NAN : ((Tb == 0 && L == 0) ? 0.f : -INFINITY);
      tk[0] = tick0; tk[1] = tick0; tk[2] = tick0; tk[3] = tick0;
    }
    return;
  }
  const unsigned long long tick1 = wall_clock64();

  // back-trace.  Row t holds the step from frame t to frame t - 1; row 0 does not exist and is staged as zeros ("stay").
  {
    const int nq = (Tb + AL_BLK - 1) / AL_BLK;
    const int nblk = AL_BLK * G;         // 16-byte groups in a block, at most LPER * CT_NT
    const long nrow = (long)Tb * G;
    uint4 pre[LPER];
#pragma unroll
    for (int i = 0; i < LPER; ++i) {
      const int idx = tid + i * CT_NT;
      const long e = (long)(nq - 1) * nblk + idx;
      pre[i] = (idx < nblk && e >= G && e < nrow) ? bpb[e] : make_uint4(0, 0, 0, 0);
    }
    int s = s_end, prev = -1;
    for (int q = nq - 1; q >= 0; --q) {
#pragma unroll
      for (int i = 0; i < LPER; ++i) {
        const int idx = tid + i * CT_NT;
        if (idx < nblk) s_bp[idx] = pre[i];
      }
      __syncthreads();
      if (q > 0) {
#pragma unroll
        for (int i = 0; i < LPER; ++i) {
          const int idx = tid + i * CT_NT;
          const long e = (long)(q - 1) * nblk + idx;
          pre[i] = (idx < nblk && e >= G && e < nrow) ? bpb[e] : make_uint4(0, 0, 0, 0);
        }
      }
      if (tid == 0) {
        const unsigned* w = (const unsigned*)s_bp;
        const int t0 = q * AL_BLK;
        const int t1 = Tb - 1 < t0 + AL_BLK - 1 ? Tb - 1 : t0 + AL_BLK - 1;
        for (int t = t1; t >= t0; --t) {
          const int j = s >> 1;
          fr[t] = (s & 1) ? j : -1;
          if (s & 1) {
            if (s != prev) s_span[1][j] = t + 1;
            s_span[0][j] = t;
          }
          prev = s;
          const int wi = (((t - t0) * G + (s >> 6)) << 2) + ((s >> 5) & 1);
          const unsigned lo = w[wi], hi = w[wi + 2];
          s -= (int)(((lo >> (s & 31)) & 1u) | (((hi >> (s & 31)) & 1u) << 1));
        }
      }
      __syncthreads();
    }
  }
  const unsigned long long tick2 = wall_clock64();

  // sums over the path, a chunk of CT_NT frames at a time
  double acc[LPER];
  int s0[LPER], s1[LPER];
#pragma unroll
  for (int k = 0; k < LPER; ++k) {
    const int j = tid + k * CT_NT;
    acc[k] = 0.0;
    s0[k] = j < L ? s_span[0][j] : 0;
    s1[k] = j < L ? s_span[1][j] : 0;
  }
  double total = 0.0;
  for (int c0 = 0; c0 < Tb; c0 += CT_NT) {
    const int n = Tb - c0 < CT_NT ? Tb - c0 : CT_NT;
    if (tid < n) {
      const int t = c0 + tid;
      const int f = fr[t];
      const int cls = f >= 0 ? targets[o0 + f] : blank;
      s_lp[tid] = (double)al_ld<DT>(x, xb + (long)t * st + cls) - lse_b[t];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < LPER; ++k) {
      const int lo = (s0[k] > c0 ? s0[k] : c0) - c0, hi = (s1[k] < c0 + n ? s1[k] : c0 + n) - c0;
      for (int i = lo; i < hi; ++i) acc[k] += s_lp[i];
    }
    if (tid == CT_NT - 1)
      for (int i = 0; i < n; ++i) total += s_lp[i];
    __syncthreads();
  }
#pragma unroll
  for (int k = 0; k < LPER; ++k) {
    const int j = tid + k * CT_NT;
    if (j < Lmax) {
      sp[2 * j] = j < L ? s0[k] : -1;
      sp[2 * j + 1] = j < L ? s1[k] : -1;
      ts[j] = j < L ? (float)acc[k] : 0.f;
    }
  }
  for (int t = Tb + tid; t < T; t += CT_NT) fr[t] = -2;
  if (tid == CT_NT - 1) score[b] = (float)total;
  if (tid == 0) { tk[0] = tick0; tk[1] = tick1; tk[2] = tick2; tk[3] = wall_clock64(); }
}

extern "C" {

int wavlm_ctc_align_supported(int32_t Lmax) { return al_supported(Lmax); }

uint64_t wavlm_ctc_align_workspace_bytes(int32_t B, int32_t T, int32_t Lmax) {
  if (B < 0 || T < 0 || Lmax < 0) return 0;
  return al_carve(B, T, Lmax).total;
}

int wavlm_ctc_align(const void* logits, int32_t dtype, int64_t stride_b, int64_t stride_t, int32_t B, int32_t T, int32_t C,
                    const int32_t* targets, const int32_t* target_offsets, int32_t n_targets, int32_t Lmax,
                    const int32_t* input_lengths, int32_t blank, int32_t* frames, int32_t* spans, float* token_scores,
                    float* score, void* workspace, uint64_t ws_bytes, void* stream) {
  if (dtype != WL_F32 && dtype != WL_BF16) return WL_EINVAL;
  if (B < 0 || T < 0 || C < 1 || n_targets < 0 || !al_supported(Lmax) || blank < 0 || blank >= C) return WL_EINVAL;
  if (B == 0) return WL_OK;
  if (!target_offsets || !input_lengths || !score || (n_targets > 0 && !targets)) return WL_EINVAL;
  if (T > 0 && (!logits || !frames)) return WL_EINVAL;
  if (Lmax > 0 && (!spans || !token_scores)) return WL_EINVAL;
  if (!ct_view_ok(B, T, C, stride_b, stride_t)) return WL_EINVAL;
  const al_ws w = al_carve(B, T, Lmax);
  if (!workspace || ws_bytes < w.total || ((uintptr_t)workspace & 15)) return WL_EINVAL;
  const int64_t rows = (int64_t)B * T;
  if (rows / (CT_NT / 64) >= 0x7fffffffLL) return WL_EINVAL;
  char* ws = (char*)workspace;
  unsigned long long* ticks = (unsigned long long*)(ws + w.ticks);
  double* lse = (double*)(ws + w.lse);
  uint4* bp = (uint4*)(ws + w.bp);
  hipStream_t s = (hipStream_t)stream;
  if (rows > 0)
    WL_LAUNCH(al_lse_kernel, dim3((unsigned)((rows + CT_NT / 64 - 1) / (CT_NT / 64))), dim3(CT_NT), 0, s, logits, (int)dtype,
              (long)stride_b, (long)stride_t, (long)rows, (int)T, (int)C, input_lengths, lse);
  const int S = 2 * Lmax + 1;
#define AL_GO2(PER, DT)                                                                                                     \
  WL_LAUNCH((ctc_align_kernel<PER, DT>), dim3((unsigned)B), dim3(CT_NT), 0, s, logits, (long)stride_b, (long)stride_t, (int)T, \
            (int)C, targets, target_offsets, (int)n_targets, input_lengths, (int)blank, (int)Lmax, (const double*)lse, bp,   \
            frames, spans, token_scores, score, ticks)
#define AL_GO(PER)                                             \
  do {                                                         \
    if (dtype == WL_F32) AL_GO2(PER, WL_F32); else AL_GO2(PER, WL_BF16); \
  } while (0)
  if (S <= CT_NT) AL_GO(1);
  else if (S <= 2 * CT_NT) AL_GO(2);
  else if (S <= 4 * CT_NT) AL_GO(4);
  else AL_GO(8);
#undef AL_GO
#undef AL_GO2
  return wl_check_launch();
}

}  // extern "C"
