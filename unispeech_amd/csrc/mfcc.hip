// Kaldi MFCC + deltas (ABI 28): the features of HuBERT's first k-means iteration, what the reference computes per utterance on
// the CPU in src/examples/hubert/simple_kmeans/dump_mfcc_feature.py:46-55 -- torchaudio.compliance.kaldi.mfcc(use_energy=False)
// at its defaults, compute_deltas twice, [c | d | dd] = 39 columns.  With W = int(0.025 sr), S = int(0.010 sr), P = 2^ceil(log2 W):
//   frame i = x[i S : i S + W], m = 1 + (len - W) / S frames;  minus its mean;  y[j] = x[j] - 0.97 x[max(j - 1, 0)];  times the
//   Povey window;  zero-padded to P;  |rfft|^2;  23 mel filters (bins < P / 2);  log(max(E, 2^-23));  13 rows of DCT x lifter;
//   d[t] = sum_{k = -2..2} k c[clamp(t + k, 0, m - 1)] / 10, applied twice.
// Every table (window, twiddles exp(-2 pi i t / P), mel weights by filter, DCT x lifter) comes from the host, float64 rounded to
// fp32 once (unispeech_amd/mfcc.py); no sine or cosine is evaluated here.
//
// One launch.  A workgroup of 4 waves owns MF_FT = 56 output frames of one row and computes the cepstra of MF_NF = 64 frames:
// its own and 4 on either side, which is what the second-order delta reaches, so no cepstrum, spectrum or log-mel value ever
// goes to HBM and nothing is exchanged between workgroups.  The (MF_NF - 1) S + W samples of the tile go to LDS once (wave_input.hpp:
// the input layer shared with resample.hip and fbank.hip).  A wave takes one frame at a time (fft_wave.hpp, shared with
// fbank.hip, holds the table staging and the transform): the real P-point transform is the
// complex P / 2-point transform of z[n] = y[2n] + i y[2n + 1] -- Stockham radix-4 passes (one radix-2 pass when log2(P / 2) is
// odd) between two wave-private LDS buffers, one butterfly per lane and pass at P = 512 -- and the split
//   X[k] = (Z[k] + conj Z[H - k]) / 2 + w_P^k (Z[k] - conj Z[H - k]) / 2i,      H = P / 2, k < H
// so an all-zero frame has an all-zero spectrum exactly and reaches the floor exactly.  Mel: one lane per filter runs over the
// filter's own bins in order (480 weights at 16 kHz, not 23 x 257); DCT: one lane per coefficient, 23 fmaf's.
// Arithmetic order is fixed and depends on nothing but the row's samples and the frame's index in the row (tiles start at frame
// 0 of every row): a row's features are bit-identical wherever the row sits in the batch and whatever the other rows hold.
#include "common.hpp"
#include "fft_wave.hpp"
#include "wave_input.hpp"
#include "../../include/wavlm_hip.h"

#define MF_NT 256
#define MF_WAVES 4
#define MF_FT 56                       // output frames per workgroup
#define MF_HALO 4                      // frames on either side the second-order delta reaches
#define MF_NF (MF_FT + 2 * MF_HALO)    // frames whose cepstra a workgroup computes
#define MF_ND (MF_FT + MF_HALO)        // frames whose first-order delta it computes
#define MF_NMEL 23
#define MF_NCEP 13
#define MF_LDS_BYTES (80 * 1024)

// LDS carve-up in floats; the two float2 regions come first (8-byte alignment)
struct mf_layout { int tw, fft, win, melw, meli, dct, x, c, d, total; };
static inline __host__ __device__ mf_layout mf_carve(int W, int S, int P) {
  mf_layout l;
  l.tw = 0;                                  // float2 [P]
  l.fft = l.tw + 2 * P;                      // per wave two buffers of float2 [P / 2]
  l.win = l.fft + MF_WAVES * 2 * P;          // [W]
  l.melw = l.win + W;                        // [P]: at most two filters per bin
  l.meli = l.melw + P;                       // int [23][3]
  l.dct = l.meli + 3 * MF_NMEL;              // [13][23]
  l.x = l.dct + MF_NCEP * MF_NMEL;           // [(MF_NF - 1) S + W]
  l.c = l.x + (MF_NF - 1) * S + W;           // [MF_NF][13]
  l.d = l.c + MF_NF * MF_NCEP;               // [MF_ND][13]
  l.total = l.d + MF_ND * MF_NCEP;
  return l;
}

static inline int mf_supported(int64_t W, int64_t S, int64_t P) {
  if (P < 64 || P > 512 || (P & (P - 1))) return 0;
  if (W > P || 2 * W <= P || S < 1 || S > W) return 0;          // P is the next power of two at or above W
  return (int64_t)mf_carve((int)W, (int)S, (int)P).total * 4 <= MF_LDS_BYTES;
}

static inline int64_t mf_frames(int64_t len, int64_t W, int64_t S) { return len < W ? 0 : 1 + (len - W) / S; }

// sum_k k v[k + 2] / 10 as differences of the mirrored pairs: a constant stretch (digital silence at the floor) gives exactly 0
__device__ __forceinline__ float mf_delta(const float* v) { return ((v[3] - v[1]) + 2.0f * (v[4] - v[0])) / 10.0f; }

__global__ __launch_bounds__(MF_NT) void mfcc_kernel(const void* __restrict__ x, int x_dt, long x_stride, long L,
    const int* __restrict__ lengths, int W, int S, int P, const float* __restrict__ window, const float* __restrict__ twiddle,
    const int* __restrict__ mel_idx, const float* __restrict__ mel_w, int n_mel_w, const float* __restrict__ dct,
    float* __restrict__ y, long y_stride, long Mmax, int ncol) {
  extern __shared__ __attribute__((aligned(16))) float mf_lds[];
  const mf_layout lo = mf_carve(W, S, P);
  const int H = P / 2;
  float2* s_tw = (float2*)(mf_lds + lo.tw);
  float* s_win = mf_lds + lo.win;
  float* s_melw = mf_lds + lo.melw;
  int* s_meli = (int*)(mf_lds + lo.meli);
  float* s_dct = mf_lds + lo.dct;
  float* s_x = mf_lds + lo.x;
  float* s_c = mf_lds + lo.c;
  float* s_d = mf_lds + lo.d;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.y;
  const long t0 = (long)blockIdx.x * MF_FT;                 // first output frame of the tile
  long t1 = t0 + MF_FT;
  if (t1 > Mmax) t1 = Mmax;
  const long len = wave_row_len(lengths, b, L);
  const long m = len < W ? 0 : 1 + (len - W) / S;           // this row's frames; [m, Mmax) is written as zero
  float* yrow = y + (size_t)b * y_stride;
  if (t0 >= m) {                                            // nothing of the row reaches this tile
    for (long q = t0 * ncol + tid; q < t1 * ncol; q += MF_NT) yrow[q] = 0.f;
    return;
  }
  mf_stage_tables(s_tw, s_win, s_melw, s_meli, twiddle, window, mel_idx, mel_w, n_mel_w, MF_NMEL, W, P, tid, MF_NT);
  for (int k = tid; k < MF_NCEP * MF_NMEL; k += MF_NT) s_dct[k] = dct[k];
  // samples: s_x[k] = x[(t0 - MF_HALO) S + k]
  wave_stage(s_x, wave_row(x, b, x_stride, x_dt), x_dt, (t0 - MF_HALO) * S, (MF_NF - 1) * S + W, len, tid, MF_NT);
  __syncthreads();

  float2* bufA = (float2*)(mf_lds + lo.fft) + (size_t)wave * 2 * H;
  float2* bufB = bufA + H;
  // frames outside [0, m) are computed on whatever the tile holds there (zeros beyond the row) and never read: every wave makes
  // the same number of trips, so the barriers below are uniform
  for (int fr = wave; fr < MF_NF; fr += MF_WAVES) {
    const float* xf = s_x + fr * S;
    float part = 0.f;
    for (int n = lane; n < W; n += 64) part += xf[n];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) part += __shfl_xor(part, o, 64);
    const float mean = part / (float)W;
    for (int h = lane; h < H; h += 64) {
      float2 z = make_float2(0.f, 0.f);
      const int n = 2 * h;
      if (n < W) {
        const float cur = xf[n] - mean, prev = xf[n > 0 ? n - 1 : 0] - mean;
        z.x = (cur - 0.97f * prev) * s_win[n];
        if (n + 1 < W) z.y = ((xf[n + 1] - mean) - 0.97f * cur) * s_win[n + 1];
      }
      bufA[h] = z;
    }
    float2* src = bufA;
    float2* dst = bufB;
    mf_transform(src, dst, s_tw, H, lane);
    // power spectrum of the real transform, bins 0 .. H - 1 (the Nyquist bin has weight zero)
    float* pw = (float*)dst;
    mf_power(src, pw, s_tw, H, lane);
    float* lg = (float*)src;
    if (lane < MF_NMEL) {
      const int first = s_meli[3 * lane], count = s_meli[3 * lane + 1], off = s_meli[3 * lane + 2];
      float e = 0.f;
      for (int i = 0; i < count; ++i) e = fmaf(s_melw[off + i], pw[first + i], e);
      lg[lane] = logf(fmaxf(e, 1.1920928955078125e-07f));
    }
    __syncthreads();
    if (lane < MF_NCEP) {
      float c = 0.f;
#pragma unroll
      for (int q = 0; q < MF_NMEL; ++q) c = fmaf(s_dct[lane * MF_NMEL + q], lg[q], c);
      s_c[fr * MF_NCEP + lane] = c;
    }
    __syncthreads();
  }

  const long base = t0 - MF_HALO;                           // frame of s_c row 0
  const long last = m - 1;
  if (ncol > MF_NCEP) {
    for (int q = tid; q < MF_ND * MF_NCEP; q += MF_NT) {    // d of frames t0 - 2 .. t0 + MF_FT + 1
      const int ui = q / MF_NCEP, i = q - ui * MF_NCEP;
      const long u = t0 - 2 + ui;
      float d = 0.f;
      if (u >= 0 && u <= last) {
        float cv[5];
#pragma unroll
        for (int k = -2; k <= 2; ++k) {
          long v = u + k;
          v = v < 0 ? 0 : (v > last ? last : v);
          cv[k + 2] = s_c[(int)(v - base) * MF_NCEP + i];
        }
        d = mf_delta(cv);
      }
      s_d[q] = d;
    }
    __syncthreads();
  }
  const int rows = (int)(t1 - t0);
  for (int q = tid; q < rows * ncol; q += MF_NT) {
    const int ti = q / ncol, col = q - ti * ncol;
    const long t = t0 + ti;
    float v = 0.f;
    if (t <= last) {
      if (col < MF_NCEP) {
        v = s_c[(ti + MF_HALO) * MF_NCEP + col];
      } else if (col < 2 * MF_NCEP) {
        v = s_d[(ti + 2) * MF_NCEP + col - MF_NCEP];
      } else {
        const int i = col - 2 * MF_NCEP;
        float dv[5];
#pragma unroll
        for (int k = -2; k <= 2; ++k) {
          long u = t + k;
          u = u < 0 ? 0 : (u > last ? last : u);
          dv[k + 2] = s_d[(int)(u - (t0 - 2)) * MF_NCEP + i];
        }
        v = mf_delta(dv);
      }
    }
    yrow[t0 * ncol + q] = v;
  }
}

extern "C" {

// 1 if wavlm_mfcc_rows takes this window / shift / transform size: P a power of two in [64, 512] and the next one at or above
// W, 1 <= S <= W, and the tile fits the kernel's LDS budget
int wavlm_mfcc_supported(int32_t W, int32_t S, int32_t P) { return mf_supported(W, S, P); }

// frames of a row of `len` samples (snip_edges): 0 below W, else 1 + (len - W) / S; -1 for a window or shift below 1
int64_t wavlm_mfcc_frames(int64_t len, int32_t W, int32_t S) {
  if (W < 1 || S < 1) return -1;
  return mf_frames(len < 0 ? 0 : len, W, S);
}

int wavlm_mfcc_rows(const void* x, int32_t x_dtype, int64_t x_stride, int32_t B, int64_t L, const int32_t* lengths, int32_t W,
                    int32_t S, int32_t P, const float* window, const float* twiddle, const int32_t* mel_idx, const float* mel_w,
                    int32_t n_mel_w, const float* dct, float* y, int64_t y_stride, int64_t Mmax, int32_t ncol, void* stream) {
  if (wave_check_input(x, x_dtype, x_stride, B, L, INT64_MAX >> 8) != WL_OK) return WL_EINVAL;
  if (!y || !window || !twiddle || !mel_idx || !mel_w || !dct) return WL_EINVAL;
  if (ncol != MF_NCEP && ncol != 3 * MF_NCEP) return WL_EINVAL;
  if (!mf_supported(W, S, P) || n_mel_w < 0) return WL_EINVAL;
  if (Mmax < mf_frames(L, W, S) || Mmax > (INT64_MAX >> 8) || y_stride < Mmax * ncol) return WL_EINVAL;   // no row is cut short
  if (Mmax == 0) return WL_OK;
  const int64_t tiles = (Mmax + MF_FT - 1) / MF_FT;
  if (tiles > 0x7fffffffLL) return WL_EINVAL;
  const size_t smem = (size_t)mf_carve(W, S, P).total * sizeof(float);
  if (wl_dynamic_lds(mfcc_kernel, smem, MF_LDS_BYTES) != WL_OK) return WL_ELAUNCH;
  WL_LAUNCH(mfcc_kernel, dim3((unsigned)tiles, (unsigned)B), dim3(MF_NT), smem, (hipStream_t)stream, x, (int)x_dtype,
            (long)x_stride, (long)L, lengths, (int)W, (int)S, (int)P, window, twiddle, mel_idx, mel_w, (int)n_mel_w, dct, y,
            (long)y_stride, (long)Mmax, (int)ncol);
  return wl_check_launch();
}

}  // extern "C"
