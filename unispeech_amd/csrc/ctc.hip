// CTC loss and its gradient with respect to the logits, and the greedy decode (ABI 30): the loss of the reference's ASR
// fine-tuning, criterions/ctc.py:113-147 -- F.ctc_loss(log_softmax(logits.float(), -1), targets_flat, input_lengths,
// target_lengths, blank, reduction="none", zero_infinity) with the log-softmax fused (models/hubert/hubert_asr.py:155-162
// get_normalized_probs(log_probs=True) is exactly that) -- and criterions/ctc.py:200-201 argmax / unique_consecutive / != blank.
//
// With l' the extended target (blank, l_0, blank, l_1, ..., blank: S = 2 L + 1 positions), lp[t, c] = x[t, c] - lse[t] and
// skip(s) = s odd and l'_s != l'_(s-2):
//   alpha_0(s) = lp[0, l'_s] for s < 2, else -inf
//   alpha_t(s) = lae(alpha_(t-1)(s), alpha_(t-1)(s-1), skip(s) ? alpha_(t-1)(s-2) : -inf) + lp[t, l'_s]
//   nll        = -lae(alpha_(Tb-1)(S-1), alpha_(Tb-1)(S-2))                         Tb = the sample's input length
//   beta the mirror image from t = Tb - 1 down (it includes lp[t, l'_s] as alpha does, hence the "- lp" below)
//   dx[t, c]   = g (exp(lp[t, c]) - sum_{s: l'_s = c} exp(alpha_t(s) + beta_t(s) + nll - lp[t, c]))
// which is torch's exp(lp) - exp(logsumexp_s(alpha + beta) + nll - lp) with the sum taken over its terms: each term is the
// posterior probability of position s at frame t, in [0, 1], so nothing overflows and no running maximum is needed.
//
// Three launches per call, none per sample or frame.
//  (a) ctc_lse_kernel: one wave per (b, t) row, two passes over the row (maximum, sum of exponentials).
//  (b) ctc_alpha_kernel: one workgroup per sample, lanes over the extended positions (PER = 1, 2, 4 or 8 per lane for S up to
//      256, 512, 1024, 2047).  The previous column lives in LDS twice (frame parity picks the buffer), so a frame costs one
//      barrier: a lane reads s, s - 1, s - 2 of the old buffer and writes s of the new one.  lp[t + 1, l'_s] is loaded before
//      frame t is combined, so the gather's latency hides under the three exponentials and the logarithm.
//  (c) ctc_beta_grad_kernel: the same walk backwards; after the frame's barrier the lanes turn to the classes (c = tid,
//      tid + 256, ...) and sum the posteriors of their class's positions.
// The running columns, lse and nll are float64: a float32 column re-rounds at the magnitude of alpha (hundreds to thousands)
// in every one of several hundred dependent steps, float64 leaves one rounding of alpha to float32 where it is stored for (c).
// exp and log are this file's own (ct_exp, ct_log13: 1e-14 relative against libm, checked on the host).
// The kernels are bound by the latency of that dependent chain, not by throughput.
//
// Fixed order.  The label indices are ranked by (class, index) once per sample -- by counting, no atomics -- so a class's
// occurrences are walked in ascending s; the blank's up to L + 1 positions are summed by one wave, each lane its own positions
// in ascending s, then one xor butterfly.  Nothing depends on B, on the sample's place in the batch or on the other samples:
// results are bitwise reproducible and a sample's loss and gradient are the same bits alone and in any batch.
#include "ctc_decode.hpp"
#include "../../include/wavlm_hip.h"

#define CT_MAXL 1023                 // labels per sample
#define CT_SP 2048                   // extended positions, padded (2 * CT_MAXL + 1 = 2047)
#define CT_MAXC 1024                 // classes
#define CT_CPER (CT_MAXC / CT_NT)    // classes per lane in (c)

static inline int ct_supported(int64_t C, int64_t Lmax) { return C >= 1 && C <= CT_MAXC && Lmax >= 0 && Lmax <= CT_MAXL; }
static inline uint64_t ct_align(uint64_t v) { return (v + 255) & ~(uint64_t)255; }
// workspace: nll64 double [B] | lse double [B, T] | alpha float [B, T, 2 Lmax + 1]
struct ct_ws { uint64_t nll, lse, alpha, total; };
static inline ct_ws ct_carve(int64_t B, int64_t T, int64_t Lmax) {
  ct_ws w;
  w.nll = 0;
  w.lse = ct_align((uint64_t)B * 8);
  w.alpha = w.lse + ct_align((uint64_t)B * (uint64_t)T * 8);
  w.total = w.alpha + ct_align((uint64_t)B * (uint64_t)T * (uint64_t)(2 * Lmax + 1) * 4);
  return w;
}

// exp(x) for x <= 1 or so to 1e-14 relative (0 below -60, where it is below 1e-26 of the term it is added to): 2^n by v_ldexp_f64,
// exp of the remainder |u| <= ln 2 / 2 by the degree-11 Taylor polynomial (u^12 / 12! < 7e-15): a dozen dependent FMAs.
// (Against the library's exp the whole call measured 4.01 ms instead of 4.19 ms at the shape of tools/ctc_bench.py.)
__device__ __forceinline__ double ct_exp(double x) {
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
// log(s) for s in [1, 3] to 1e-14: the fp32 hardware logarithm y0, then log(s) = y0 + log1p(d) with d = s exp(-y0) - 1 ~ 1e-6
__device__ __forceinline__ double ct_log13(double s) {
  const double y0 = (double)__logf((float)s);
  const double d = fma(s, ct_exp(-y0), -1.0);
  return y0 + (d - 0.5 * d * d);
}
// log(e^a + e^b + e^c): the largest term is exp(0) = 1 and is not evaluated
__device__ __forceinline__ double ct_lae3(double a, double b, double c) {
  const double m = fmax(a, fmax(b, c));
  if (m == -INFINITY) return -INFINITY;
  const double o1 = a == m ? b : a, o2 = (a == m || b == m) ? c : b;
  return m + ct_log13(1.0 + ct_exp(o1 - m) + ct_exp(o2 - m));
}

// element type as a template argument in (b) and (c): with a run-time type every load sat in a branch of its own and the
// compiler placed its s_waitcnt vmcnt(0) right behind it (seen in the ISA), one full load latency per position and frame
template <int DT> __device__ __forceinline__ float ct_ld(const void* p, long i) {
  return DT == WL_F32 ? ((const float*)p)[i] : bf2f(((const bf16_t*)p)[i]);
}
template <int DT> __device__ __forceinline__ void ct_st(void* p, long i, float v) {
  if (DT == WL_F32) ((float*)p)[i] = v; else ((bf16_t*)p)[i] = f2bf(v);
}

// ---- (a) lse[b, t] = log sum_c exp x[b, t, c], rows at or beyond the input length are skipped (never read) ----
__global__ __launch_bounds__(CT_NT) void ctc_lse_kernel(const void* __restrict__ x, int dt, long sb, long st, long rows, int T,
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
  for (int c = lane; c < C; c += 64) s += ct_exp((double)ld_elem(x, base + c, dt) - (double)m);
  s = wave_sum_d(s);
  if (lane == 0) lse[row] = (double)m + log(s);
}

// the sample's labels into LDS as the extended target; returns (uniformly) 0 if an offset or a label is out of range
__device__ __forceinline__ int ct_stage_labels(short* s_lab, int* s_bad, const int* __restrict__ targets,
    const int* __restrict__ toff, int b, int ntgt, int Lmax, int C, int blank, int& L) {
  const int tid = threadIdx.x;
  const int o0 = toff[b], o1 = toff[b + 1];
  const bool ok = o0 >= 0 && o1 >= o0 && o1 <= ntgt && o1 - o0 <= Lmax;
  L = ok ? o1 - o0 : 0;
  if (tid == 0) *s_bad = ok ? 0 : 1;
  __syncthreads();
  const int S = 2 * L + 1;
  for (int s = tid; s < S; s += CT_NT) {
    int lab = (s & 1) ? targets[o0 + (s >> 1)] : blank;
    if (lab < 0 || lab >= C) { *s_bad = 1; lab = blank; }
    s_lab[s] = (short)lab;
  }
  __syncthreads();
  return *s_bad == 0;
}

// ---- (b) alpha [b, t, s] for t < Tb, and nll64[b] ----
template <int PER, int DT>
__global__ __launch_bounds__(CT_NT) void ctc_alpha_kernel(const void* __restrict__ x, long sb, long st, int T, int C,
    const int* __restrict__ targets, const int* __restrict__ toff, int ntgt, const int* __restrict__ in_len, int blank, int Lmax,
    const double* __restrict__ lse, float* __restrict__ alpha, double* __restrict__ nll64) {
  __shared__ double s_a[2][CT_SP];
  __shared__ short s_lab[CT_SP];
  __shared__ int s_bad;
  const int tid = threadIdx.x, b = blockIdx.x;
  int L;
  if (!ct_stage_labels(s_lab, &s_bad, targets, toff, b, ntgt, Lmax, C, blank, L)) {
    if (tid == 0) nll64[b] = (double)NAN;
    return;
  }
  const int S = 2 * L + 1, Smax = 2 * Lmax + 1;
  const int Tb = ct_len(in_len, b, T);
  if (Tb == 0) {   // no frame: the empty target has probability one, every other none
    if (tid == 0) nll64[b] = L == 0 ? 0.0 : (double)INFINITY;
    return;
  }
  const long xb = (long)b * sb;
  const double* lse_b = lse + (long)b * T;
  float* al = alpha + (size_t)b * T * Smax;
  int lab[PER];
  bool skip[PER];
  float nxt[PER];   // x[t + 1, l'_s], loaded a frame ahead and not touched until then
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    const int s = tid + k * CT_NT;
    lab[k] = 0; skip[k] = false; nxt[k] = 0.f;
    if (s < S) {
      lab[k] = s_lab[s];
      skip[k] = (s & 1) && s >= 2 && s_lab[s] != s_lab[s - 2];
      const double v = s < 2 ? (double)ct_ld<DT>(x, xb + lab[k]) - lse_b[0] : -INFINITY;
      s_a[0][s] = v;
      al[s] = (float)v;
      if (Tb > 1) nxt[k] = ct_ld<DT>(x, xb + st + lab[k]);
    }
  }
  __syncthreads();
  for (int t = 1; t < Tb; ++t) {
    const double* prv = s_a[(t & 1) ^ 1];
    double* cur = s_a[t & 1];
    const double lse_t = lse_b[t];
    // the next frame's loads: every lane, no branch (an idle lane reads class 0, the last frame reads itself again), so that
    // nothing waits for them before the next trip
    float raw[PER];
    const long xn = xb + (long)(t + 1 < Tb ? t + 1 : t) * st;
#pragma unroll
    for (int k = 0; k < PER; ++k) { raw[k] = nxt[k]; nxt[k] = ct_ld<DT>(x, xn + lab[k]); }
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const int s = tid + k * CT_NT;
      if (s < S) {
        const double lp = (double)raw[k] - lse_t;
        const double a0 = prv[s], a1 = s >= 1 ? prv[s - 1] : -INFINITY, a2 = skip[k] ? prv[s - 2] : -INFINITY;
        const double v = ct_lae3(a0, a1, a2) + lp;
        cur[s] = v;
        al[(size_t)t * Smax + s] = (float)v;
      }
    }
    __syncthreads();
  }
  if (tid == 0) {
    const double* fin = s_a[(Tb - 1) & 1];
    nll64[b] = -ct_lae3(fin[S - 1], S > 1 ? fin[S - 2] : -INFINITY, -INFINITY);
  }
}

// ---- (c) beta, the class sums and dx; nll[b] out ----
template <int PER, int DT>
__global__ __launch_bounds__(CT_NT) void ctc_beta_grad_kernel(const void* __restrict__ x, long sb, long st, int T, int C,
    const int* __restrict__ targets, const int* __restrict__ toff, int ntgt, const int* __restrict__ in_len, int blank, int Lmax,
    const double* __restrict__ lse, const float* __restrict__ alpha, const double* __restrict__ nll64,
    const float* __restrict__ grad_out, int zero_infinity, float* __restrict__ nll_out, void* __restrict__ dx) {
  __shared__ double s_b[2][CT_SP];
  __shared__ float s_g[2][CT_SP];
  __shared__ short s_lab[CT_SP];
  __shared__ unsigned short s_ord[CT_MAXL + 1];
  __shared__ int s_bad;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x;
  const long xb = (long)b * sb;
  int L;
  const bool ok = ct_stage_labels(s_lab, &s_bad, targets, toff, b, ntgt, Lmax, C, blank, L);
  const int S = 2 * L + 1, Smax = 2 * Lmax + 1;
  const int Tb = ok ? ct_len(in_len, b, T) : 0;
  const double nll = nll64[b];
  const bool feasible = nll < (double)INFINITY;   // false for NaN (labels out of range) too
  if (tid == 0) nll_out[b] = (zero_infinity && nll == (double)INFINITY) ? 0.f : (float)nll;
  // rows the sample does not reach are zero; so is everything of a sample without an alignment under zero_infinity (and of one
  // with labels out of range, whose loss is NaN).  Without zero_infinity the formula gives NaN there, as it does in torch.
  const int t_fill = (feasible && Tb > 0) ? Tb : 0;
  const float fill = (!feasible && ok && !zero_infinity) ? NAN : 0.f;
  for (int t = t_fill; t < T; ++t)
    for (int c = tid; c < C; c += CT_NT) ct_st<DT>(dx, xb + (long)t * st + c, (t_fill == 0 && t < Tb) ? fill : 0.f);
  if (t_fill == 0) return;

  // label indices ranked by (class, index); a lane's classes: where their run starts and how long it is
  for (int i = tid; i < L; i += CT_NT) {
    const int c = s_lab[2 * i + 1];
    int r = 0;
    for (int j = 0; j < L; ++j) {
      const int cj = s_lab[2 * j + 1];
      r += (cj < c || (cj == c && j < i)) ? 1 : 0;
    }
    s_ord[r] = (unsigned short)i;
  }
  int cstart[CT_CPER], ccnt[CT_CPER];
#pragma unroll
  for (int q = 0; q < CT_CPER; ++q) {
    const int c = tid + q * CT_NT;
    cstart[q] = 0; ccnt[q] = 0;
    if (c < C && c != blank)
      for (int j = 0; j < L; ++j) {
        const int cj = s_lab[2 * j + 1];
        cstart[q] += cj < c ? 1 : 0;
        ccnt[q] += cj == c ? 1 : 0;
      }
  }
  int lab[PER];
  bool skip[PER];
  float lpn[PER];   // x[t - 1, l'_s] and alpha_(t-1)(s), loaded a frame ahead
  float aln[PER];
  const double* lse_b = lse + (long)b * T;
  const float* al = alpha + (size_t)b * T * Smax;
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    const int s = tid + k * CT_NT;
    lab[k] = 0; skip[k] = false; lpn[k] = 0.f; aln[k] = 0.f;
    if (s < S) {
      lab[k] = s_lab[s];
      skip[k] = (s & 1) && s + 2 < S && s_lab[s] != s_lab[s + 2];
      lpn[k] = ct_ld<DT>(x, xb + (long)(Tb - 1) * st + lab[k]);
      aln[k] = al[(size_t)(Tb - 1) * Smax + s];
    }
  }
  const double g = (double)grad_out[b];
  __syncthreads();

  for (int t = Tb - 1; t >= 0; --t) {
    const long xt = xb + (long)t * st;
    const double lse_t = lse_b[t];
    float xc[CT_CPER];
#pragma unroll
    for (int q = 0; q < CT_CPER; ++q) {
      const int c = tid + q * CT_NT;
      xc[q] = c < C ? ct_ld<DT>(x, xt + c) : 0.f;
    }
    const double* nx = s_b[(t & 1) ^ 1];
    double* cur = s_b[t & 1];
    float* gam = s_g[t & 1];
    // the previous frame's loads: every lane, no branch (an idle lane reads class 0 and position 0, frame 0 reads itself again)
    float rawx[PER], rawa[PER];
    const int tp = t > 0 ? t - 1 : 0;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const int s = tid + k * CT_NT;
      rawx[k] = lpn[k]; rawa[k] = aln[k];
      lpn[k] = ct_ld<DT>(x, xb + (long)tp * st + lab[k]);
      aln[k] = al[(size_t)tp * Smax + (s < S ? s : 0)];
    }
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const int s = tid + k * CT_NT;
      if (s < S) {
        const double lp = (double)rawx[k] - lse_t, av = (double)rawa[k];
        double bv;
        if (t == Tb - 1) {
          bv = s >= S - 2 ? lp : -INFINITY;
        } else {
          const double b0 = nx[s], b1 = s + 1 < S ? nx[s + 1] : -INFINITY, b2 = skip[k] ? nx[s + 2] : -INFINITY;
          bv = ct_lae3(b0, b1, b2) + lp;
        }
        cur[s] = bv;
        gam[s] = (float)ct_exp(av + bv + nll - lp);   // -inf on either side: 0
      }
    }
    __syncthreads();
    // gam[] of this parity is next written two frames on, after the next frame's barrier: no second barrier is needed
    if (wave == CT_NT / 64 - 1) {   // the blank's positions (every even s, and a label that names the blank)
      double part = 0.0;
      for (int s = lane; s < S; s += 64) part += s_lab[s] == blank ? (double)gam[s] : 0.0;
      part = wave_sum_d(part);
      if (lane == 0) {
        const float xblank = ct_ld<DT>(x, xt + blank);
        ct_st<DT>(dx, xt + blank, (float)(g * (ct_exp((double)xblank - lse_t) - part)));
      }
    }
#pragma unroll
    for (int q = 0; q < CT_CPER; ++q) {
      const int c = tid + q * CT_NT;
      if (c < C && c != blank) {
        double sum = 0.0;
        for (int i = 0; i < ccnt[q]; ++i) sum += (double)gam[2 * (int)s_ord[cstart[q] + i] + 1];
        ct_st<DT>(dx, xt + c, (float)(g * (ct_exp((double)xc[q] - lse_t) - sum)));
      }
    }
  }
}

// ---- greedy decode: argmax per frame (ties to the lowest class), repeats collapsed, blanks dropped (ctc_decode.hpp) ----
__global__ __launch_bounds__(CT_NT) void ctc_greedy_kernel(const void* __restrict__ x, int dt, long sb, long st, int T, int C,
    const int* __restrict__ in_len, int blank, int* __restrict__ tokens, int* __restrict__ counts) {
  __shared__ int s_arg[CT_NT];
  __shared__ int s_state[2];
  ct_greedy_sample(x, dt, sb, st, T, C, in_len, blank, tokens, counts, blockIdx.x, s_arg, s_state);
}

template <int PER, int DT>
static void ct_launch(int B, hipStream_t s, const void* x, long sb, long st, int T, int C, const int* targets, const int* toff,
                      int ntgt, const int* in_len, int blank, int Lmax, const double* lse, float* alpha, double* nll64,
                      const float* grad_out, int zero_infinity, float* nll, void* dx) {
  WL_LAUNCH((ctc_alpha_kernel<PER, DT>), dim3((unsigned)B), dim3(CT_NT), 0, s, x, sb, st, T, C, targets, toff, ntgt, in_len, blank,
            Lmax, lse, alpha, nll64);
  WL_LAUNCH((ctc_beta_grad_kernel<PER, DT>), dim3((unsigned)B), dim3(CT_NT), 0, s, x, sb, st, T, C, targets, toff, ntgt, in_len,
            blank, Lmax, lse, (const float*)alpha, (const double*)nll64, grad_out, zero_infinity, nll, dx);
}

extern "C" {

int wavlm_ctc_supported(int32_t C, int32_t Lmax) { return ct_supported(C, Lmax); }

uint64_t wavlm_ctc_workspace_bytes(int32_t B, int32_t T, int32_t Lmax) {
  if (B < 0 || T < 0 || Lmax < 0) return 0;
  return ct_carve(B, T, Lmax).total;
}

int wavlm_ctc_loss(const void* logits, int32_t dtype, int64_t stride_b, int64_t stride_t, int32_t B, int32_t T, int32_t C,
                   const int32_t* targets, const int32_t* target_offsets, int32_t n_targets, int32_t Lmax,
                   const int32_t* input_lengths, int32_t blank, int32_t zero_infinity, const float* grad_out, float* nll,
                   void* dlogits, void* workspace, uint64_t ws_bytes, void* stream) {
  if (dtype != WL_F32 && dtype != WL_BF16) return WL_EINVAL;
  if (B < 0 || T < 0 || n_targets < 0 || !ct_supported(C, Lmax) || blank < 0 || blank >= C) return WL_EINVAL;
  if (B == 0) return WL_OK;
  if (!target_offsets || !input_lengths || !grad_out || !nll || (n_targets > 0 && !targets)) return WL_EINVAL;
  if (T > 0 && (!logits || !dlogits)) return WL_EINVAL;
  if (!ct_view_ok(B, T, C, stride_b, stride_t)) return WL_EINVAL;
  const ct_ws w = ct_carve(B, T, Lmax);
  if (!workspace || ws_bytes < w.total || ((uintptr_t)workspace & 7)) return WL_EINVAL;
  const int64_t rows = (int64_t)B * T;
  if (rows / (CT_NT / 64) >= 0x7fffffffLL) return WL_EINVAL;
  char* ws = (char*)workspace;
  double* nll64 = (double*)(ws + w.nll);
  double* lse = (double*)(ws + w.lse);
  float* alpha = (float*)(ws + w.alpha);
  hipStream_t s = (hipStream_t)stream;
  if (rows > 0)
    WL_LAUNCH(ctc_lse_kernel, dim3((unsigned)((rows + CT_NT / 64 - 1) / (CT_NT / 64))), dim3(CT_NT), 0, s, logits, (int)dtype,
              (long)stride_b, (long)stride_t, (long)rows, (int)T, (int)C, input_lengths, lse);
  const int S = 2 * Lmax + 1;
#define CT_GO(PER)                                                                                                        \
  do {                                                                                                                    \
    if (dtype == WL_F32)                                                                                                  \
      ct_launch<PER, WL_F32>(B, s, logits, (long)stride_b, (long)stride_t, (int)T, (int)C, targets, target_offsets,       \
                             (int)n_targets, input_lengths, (int)blank, (int)Lmax, lse, alpha, nll64, grad_out,           \
                             (int)zero_infinity, nll, dlogits);                                                           \
    else                                                                                                                  \
      ct_launch<PER, WL_BF16>(B, s, logits, (long)stride_b, (long)stride_t, (int)T, (int)C, targets, target_offsets,      \
                              (int)n_targets, input_lengths, (int)blank, (int)Lmax, lse, alpha, nll64, grad_out,          \
                              (int)zero_infinity, nll, dlogits);                                                          \
  } while (0)
  if (S <= CT_NT) CT_GO(1);
  else if (S <= 2 * CT_NT) CT_GO(2);
  else if (S <= 4 * CT_NT) CT_GO(4);
  else CT_GO(8);
#undef CT_GO
  return wl_check_launch();
}

int wavlm_ctc_greedy(const void* logits, int32_t dtype, int64_t stride_b, int64_t stride_t, int32_t B, int32_t T, int32_t C,
                     const int32_t* input_lengths, int32_t blank, int32_t* tokens, int32_t* counts, void* stream) {
  if (dtype != WL_F32 && dtype != WL_BF16) return WL_EINVAL;
  if (B < 0 || T < 0 || C < 1 || blank < 0 || blank >= C) return WL_EINVAL;
  if (B == 0) return WL_OK;
  if (!input_lengths || !counts || (T > 0 && (!logits || !tokens))) return WL_EINVAL;
  if (!ct_view_ok(B, T, C, stride_b, stride_t)) return WL_EINVAL;
  WL_LAUNCH(ctc_greedy_kernel, dim3((unsigned)B), dim3(CT_NT), 0, (hipStream_t)stream, logits, (int)dtype, (long)stride_b,
            (long)stride_t, (int)T, (int)C, input_lengths, (int)blank, tokens, counts);
  return wl_check_launch();
}

}  // extern "C"
