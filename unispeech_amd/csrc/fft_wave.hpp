// The table staging (mf_stage_tables) and the wave-per-frame real transform shared by csrc/mfcc.hip and csrc/fbank.hip: the
// real P-point transform of a frame y is the complex H = P / 2-point transform of z[n] = y[2n] + i y[2n + 1] -- Stockham
// radix-4 passes (one radix-2 pass when log2 H is odd) between two wave-private LDS buffers, one butterfly per lane and pass at
// P = 512 -- and the split
//   X[k] = (Z[k] + conj Z[H - k]) / 2 + w_P^k (Z[k] - conj Z[H - k]) / 2i,      k < H
// so an all-zero frame has an all-zero spectrum exactly.  Twiddles tw[t] = exp(-2 pi i t / P), t < P, come from the host (float64
// rounded to fp32 once); no sine or cosine is evaluated here.  Every wave of the workgroup must make the same number of calls:
// the stages end in workgroup barriers.
#pragma once
#include "common.hpp"

// Butterflies are evaluated in fp64 registers on fp32 operands (samples, twiddles) and, with float2 storage, stored to LDS as
// fp32: a value is rounded once per pass instead of once per multiply and add, which is what keeps the transform's error near that of a transform
// evaluated exactly and rounded at the end (numpy's single-precision rfft, the tests' fp32 oracle, behaves like that)
struct mf_c64 { double x, y; };
__device__ __forceinline__ mf_c64 mf_wide(float2 a) { return {(double)a.x, (double)a.y}; }
__device__ __forceinline__ float2 mf_narrow(double x, double y) { return make_float2((float)x, (float)y); }
// storage between the passes: float2 (mfcc.hip: one rounding per value and pass) or double2 (fbank.hip: none before the power
// spectrum; its bound, DESIGN 4.9, leaves no room for four)
__device__ __forceinline__ mf_c64 mf_wide(double2 a) { return {a.x, a.y}; }
__device__ __forceinline__ void mf_put(float2& o, double x, double y) { o = mf_narrow(x, y); }
__device__ __forceinline__ void mf_put(double2& o, double x, double y) { o = make_double2(x, y); }
__device__ __forceinline__ mf_c64 mf_cmul(mf_c64 a, float2 w) {
  return {a.x * (double)w.x - a.y * (double)w.y, a.x * (double)w.y + a.y * (double)w.x};
}

// the tables a workgroup of nt threads stages once: twiddles as float2 [P], the window [W], the mel weights padded with zeros to
// [P], and per filter (first bin, count, offset into the weights) [nfilt][3], clamped so that a filter stays inside the H = P / 2
// bins and the nw weights whatever the host's table holds
__device__ __forceinline__ void mf_stage_tables(float2* s_tw, float* s_win, float* s_melw, int* s_meli,
                                                const float* __restrict__ twiddle, const float* __restrict__ window,
                                                const int* __restrict__ mel_idx, const float* __restrict__ mel_w, int n_mel_w,
                                                int nfilt, int W, int P, int tid, int nt) {
  const int H = P / 2;
  for (int k = tid; k < P; k += nt) s_tw[k] = make_float2(twiddle[2 * k], twiddle[2 * k + 1]);
  for (int k = tid; k < W; k += nt) s_win[k] = window[k];
  const int nw = n_mel_w < P ? n_mel_w : P;
  for (int k = tid; k < P; k += nt) s_melw[k] = k < nw ? mel_w[k] : 0.f;
  for (int f = tid; f < nfilt; f += nt) {
    int first = mel_idx[3 * f], count = mel_idx[3 * f + 1], off = mel_idx[3 * f + 2];
    first = first < 0 ? 0 : (first > H ? H : first);
    off = off < 0 ? 0 : (off > nw ? nw : off);
    if (count > H - first) count = H - first;
    if (count > nw - off) count = nw - off;
    if (count < 0) count = 0;
    s_meli[3 * f] = first; s_meli[3 * f + 1] = count; s_meli[3 * f + 2] = off;
  }
}

// one Stockham pass of radix R over H points: Ns = product of the radices before it; twiddles w_H^t = tw[2 t]
template <int R, typename C2>
__device__ __forceinline__ void mf_pass(const C2* __restrict__ in, C2* __restrict__ out, const float2* __restrict__ tw,
                                        int H, int Ns, int lane) {
  const int T = H / R;
  for (int j = lane; j < T; j += 64) {
    const int k = j & (Ns - 1);
    const int step = 2 * k * (H / (Ns * R));
    mf_c64 v[R];
#pragma unroll
    for (int r = 0; r < R; ++r) v[r] = mf_wide(in[j + r * T]);
#pragma unroll
    for (int r = 1; r < R; ++r) v[r] = mf_cmul(v[r], tw[r * step]);
    C2* o = out + (j - k) * R + k;
    if (R == 2) {
      mf_put(o[0], v[0].x + v[1].x, v[0].y + v[1].y);
      mf_put(o[Ns], v[0].x - v[1].x, v[0].y - v[1].y);
    } else {
      const mf_c64 a0 = {v[0].x + v[2].x, v[0].y + v[2].y}, a1 = {v[0].x - v[2].x, v[0].y - v[2].y};
      const mf_c64 a2 = {v[1].x + v[3].x, v[1].y + v[3].y};
      const mf_c64 a3 = {v[1].y - v[3].y, v[3].x - v[1].x};                     // -i (v1 - v3)
      mf_put(o[0], a0.x + a2.x, a0.y + a2.y);
      mf_put(o[Ns], a1.x + a3.x, a1.y + a3.y);
      mf_put(o[2 * Ns], a0.x - a2.x, a0.y - a2.y);
      mf_put(o[3 * Ns], a1.x - a3.x, a1.y - a3.y);
    }
  }
}

// the complex H-point transform of z, which the wave's lanes have just written to src (not yet synchronised): on return src
// holds Z and dst is the wave's other buffer
template <typename C2>
__device__ __forceinline__ void mf_transform(C2*& src, C2*& dst, const float2* tw, int H, int lane) {
  __syncthreads();
  int Ns = 1;
  for (; Ns * 4 <= H; Ns *= 4) {
    mf_pass<4>(src, dst, tw, H, Ns, lane);
    __syncthreads();
    C2* t = src; src = dst; dst = t;
  }
  if (Ns < H) {
    mf_pass<2>(src, dst, tw, H, Ns, lane);
    __syncthreads();
    C2* t = src; src = dst; dst = t;
  }
}

// power spectrum of the real transform, bins 0 .. H - 1 (not the Nyquist bin), from Z = src into pw
template <typename C2>
__device__ __forceinline__ void mf_power(const C2* src, float* pw, const float2* tw, int H, int lane) {
  for (int k = lane; k < H; k += 64) {
    const mf_c64 zk = mf_wide(src[k]), zn = mf_wide(src[(H - k) & (H - 1)]);
    const mf_c64 ev = {0.5 * (zk.x + zn.x), 0.5 * (zk.y - zn.y)};             // (Z[k] + conj Z[H - k]) / 2
    const mf_c64 od = {0.5 * (zk.y + zn.y), -0.5 * (zk.x - zn.x)};            // (Z[k] - conj Z[H - k]) / 2i
    const mf_c64 t = mf_cmul(od, tw[k]);
    const double re = ev.x + t.x, im = ev.y + t.y;
    pw[k] = (float)(re * re + im * im);
  }
  __syncthreads();
}
