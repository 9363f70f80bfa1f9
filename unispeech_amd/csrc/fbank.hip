// Log-mel filter bank (ABI 29): the front end of the reference's ECAPA-TDNN baseline, downstreams/speaker_verification/models/
// ecapa_tdnn.py:179-182, 253, 257 with feat_type='fbank' -- torchaudio.transforms.MelSpectrogram(sample_rate=sr, n_fft=P,
// win_length=W, hop_length=S, f_min=0, f_max=sr // 2, pad=0, n_mels=M) at its defaults otherwise, + 1e-6, log:
//   T = 1 + len / S frames;  frame t = the P samples around t S (centre=True), reflected at both ends of the row without
//   repeating the edge sample (i < 0 -> -i;  i >= len -> 2 (len - 1) - i; needs len > P / 2);  times the periodic Hann window of
//   W points placed at offset (P - W) / 2;  |rfft_P|^2;  M triangular HTK mel filters over 0 .. sr / 2 (bin 0 and the Nyquist bin
//   weigh 0);  log(E + 1e-6).
// Every table (window, twiddles exp(-2 pi i t / P), mel weights by filter) comes from the host, float64 rounded to fp32 once
// (unispeech_amd/fbank.py); no sine or cosine is evaluated here.
//
// One launch.  A workgroup of 4 waves owns FB_NF = 56 frames of one row.  The (FB_NF - 1) S + W samples under the tile's windows
// go to LDS once, the reflection resolved while staging (wave_input.hpp: the input layer shared with resample.hip and mfcc.hip;
// the P - W samples of a frame the window zeroes are never read).  The tables are staged and a wave takes one frame at a time
// through fft_wave.hpp -- the real P-point transform as
// the complex P / 2-point one and the split, shared with mfcc.hip; here the values stay fp64 in LDS between the passes (the
// products sample x window and the twiddles are fp32, the power spectrum is rounded to fp32 once) -- so an all-zero frame has
// an all-zero spectrum and gives log(1e-6f) rounded to fp32.  Mel: lane m, m + 64 runs over its filter's own bins in order, the
// sum and the log in fp64; the M
// columns of a frame are the only thing written to HBM.
// Arithmetic order is fixed and depends on nothing but the row's samples and length and the frame's index in the row (tiles
// start at frame 0 of every row): a row's features are bit-identical wherever the row sits in the batch.
#include "common.hpp"
#include "fft_wave.hpp"
#include "wave_input.hpp"
#include "../../include/wavlm_hip.h"

#define FB_NT 256
#define FB_WAVES 4
#define FB_NF 56                       // frames per workgroup (a multiple of FB_WAVES)
#define FB_MAX_MEL 128
#define FB_LDS_BYTES (80 * 1024)       // two workgroups per CU

// LDS carve-up in floats; the float2 and double2 regions come first (16-byte alignment)
struct fb_layout { int tw, fft, win, melw, meli, x, total; };
static inline __host__ __device__ fb_layout fb_carve(int W, int S, int P) {
  fb_layout l;
  l.tw = 0;                                  // float2 [P]
  l.fft = l.tw + 2 * P;                      // per wave two buffers of double2 [P / 2] (16-byte aligned: 2 P floats in)
  l.win = l.fft + FB_WAVES * 4 * P;          // [W]
  l.melw = l.win + W;                        // [P]: at most two filters per bin, none on bin 0
  l.meli = l.melw + P;                       // int [FB_MAX_MEL][3]
  l.x = l.meli + 3 * FB_MAX_MEL;             // [(FB_NF - 1) S + W]
  l.total = l.x + (FB_NF - 1) * S + W;
  return l;
}

static inline int fb_supported(int64_t W, int64_t S, int64_t P, int64_t M) {
  if (P < 64 || P > 512 || (P & (P - 1))) return 0;
  if (W > P || 2 * W <= P || S < 1 || S > W || M < 1 || M > FB_MAX_MEL) return 0;
  return (int64_t)fb_carve((int)W, (int)S, (int)P).total * 4 <= FB_LDS_BYTES;
}

static inline __host__ __device__ int64_t fb_frames(int64_t len, int64_t S, int64_t P) { return len <= P / 2 ? 0 : 1 + len / S; }

__global__ __launch_bounds__(FB_NT) void fbank_kernel(const void* __restrict__ x, int x_dt, long x_stride, long L,
    const int* __restrict__ lengths, int W, int S, int P, int M, const float* __restrict__ window,
    const float* __restrict__ twiddle, const int* __restrict__ mel_idx, const float* __restrict__ mel_w, int n_mel_w,
    float* __restrict__ y, long y_stride, long Tmax) {
  extern __shared__ __attribute__((aligned(16))) float fb_lds[];
  const fb_layout lo = fb_carve(W, S, P);
  const int H = P / 2;
  float2* s_tw = (float2*)(fb_lds + lo.tw);
  float* s_win = fb_lds + lo.win;
  float* s_melw = fb_lds + lo.melw;
  int* s_meli = (int*)(fb_lds + lo.meli);
  float* s_x = fb_lds + lo.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.y;
  const long t0 = (long)blockIdx.x * FB_NF;                 // first frame of the tile
  long t1 = t0 + FB_NF;
  if (t1 > Tmax) t1 = Tmax;
  const long len = wave_row_len(lengths, b, L);
  const long m = fb_frames(len, S, P);                      // this row's frames; [m, Tmax) is written as zero
  float* yrow = y + (size_t)b * y_stride;
  const long tv = m < t0 ? t0 : (m < t1 ? m : t1);          // the tile's frames [tv, t1) do not exist in this row
  for (long q = tv * M + tid; q < t1 * M; q += FB_NT) yrow[q] = 0.f;
  if (tv == t0) return;                                     // nothing of the row reaches this tile
  mf_stage_tables(s_tw, s_win, s_melw, s_meli, twiddle, window, mel_idx, mel_w, n_mel_w, M, W, P, tid, FB_NT);
  // samples under the windows of the tile's frames: s_x[k] = x[reflect(t0 S - P / 2 + w0 + k)], w0 the window's offset in the
  // frame.  Every index a frame of the row reaches lands in [0, len) after one reflection (len > P / 2, t S <= len); the trips
  // that round the frame count up to the waves read past that and take zero.
  const int w0 = (P - W) / 2;
  const int nfr = (int)(((tv - t0) + FB_WAVES - 1) / FB_WAVES) * FB_WAVES;   // <= FB_NF
  wave_stage<true>(s_x, wave_row(x, b, x_stride, x_dt), x_dt, t0 * S - H + w0, (nfr - 1) * S + W, len, tid, FB_NT);
  __syncthreads();

  double2* bufA = (double2*)(fb_lds + lo.fft) + (size_t)wave * 2 * H;
  double2* bufB = bufA + H;
  // every wave makes the same number of trips, so the barriers are uniform; a trip beyond the row's frames is not stored
  for (int fr = wave; fr < nfr; fr += FB_WAVES) {
    const float* xf = s_x + fr * S - w0;                    // xf[n]: sample n of the P-point frame, read for w0 <= n < w0 + W
    const float* wf = s_win - w0;
    for (int h = lane; h < H; h += 64) {
      float2 z = make_float2(0.f, 0.f);
      const int n = 2 * h;
      if (n >= w0 && n < w0 + W) z.x = xf[n] * wf[n];
      if (n + 1 >= w0 && n + 1 < w0 + W) z.y = xf[n + 1] * wf[n + 1];
      bufA[h] = make_double2((double)z.x, (double)z.y);
    }
    double2* src = bufA;
    double2* dst = bufB;
    mf_transform(src, dst, s_tw, H, lane);
    float* pw = (float*)dst;
    mf_power(src, pw, s_tw, H, lane);
    const long t = t0 + fr;
    for (int f = lane; f < M; f += 64) {
      const int first = s_meli[3 * f], count = s_meli[3 * f + 1], off = s_meli[3 * f + 2];
      // fp64 sum and log of fp32 weights and powers: logf alone is an ulp off, which is 2 x E32 where the log is near -2.5
      double e = 0.0;
      for (int i = 0; i < count; ++i) e = fma((double)s_melw[off + i], (double)pw[first + i], e);
      if (t < tv) yrow[t * M + f] = (float)log(e + (double)1e-6f);
    }
    __syncthreads();                                        // pw is read before the next frame overwrites the buffers
  }
}

extern "C" {

// 1 if wavlm_fbank_rows takes this window / hop / transform size / filter count: P a power of two in [64, 512], P / 2 < W <= P,
// 1 <= S <= W, 1 <= M <= 128, and the tile fits the kernel's LDS budget
int wavlm_fbank_supported(int32_t W, int32_t S, int32_t P, int32_t M) { return fb_supported(W, S, P, M); }

// frames of a row of `len` samples (centre=True): 0 for len <= P / 2 (the reflection needs more), else 1 + len / S; -1 for a
// hop or transform size below 1
int64_t wavlm_fbank_frames(int64_t len, int32_t S, int32_t P) {
  if (S < 1 || P < 1) return -1;
  return fb_frames(len < 0 ? 0 : len, S, P);
}

int wavlm_fbank_rows(const void* x, int32_t x_dtype, int64_t x_stride, int32_t B, int64_t L, const int32_t* lengths, int32_t W,
                     int32_t S, int32_t P, int32_t M, const float* window, const float* twiddle, const int32_t* mel_idx,
                     const float* mel_w, int32_t n_mel_w, float* y, int64_t y_stride, int64_t Tmax, void* stream) {
  if (wave_check_input(x, x_dtype, x_stride, B, L, INT64_MAX >> 8) != WL_OK) return WL_EINVAL;
  if (!y || !window || !twiddle || !mel_idx || !mel_w) return WL_EINVAL;
  if (!fb_supported(W, S, P, M) || n_mel_w < 0) return WL_EINVAL;
  if (Tmax < fb_frames(L, S, P) || Tmax > (INT64_MAX >> 8) / M || y_stride < Tmax * M) return WL_EINVAL;   // no row is cut short
  if (Tmax == 0) return WL_OK;
  const int64_t tiles = (Tmax + FB_NF - 1) / FB_NF;
  if (tiles > 0x7fffffffLL) return WL_EINVAL;
  const size_t smem = (size_t)fb_carve(W, S, P).total * sizeof(float);
  if (wl_dynamic_lds(fbank_kernel, smem, FB_LDS_BYTES) != WL_OK) return WL_ELAUNCH;
  WL_LAUNCH(fbank_kernel, dim3((unsigned)tiles, (unsigned)B), dim3(FB_NT), smem, (hipStream_t)stream, x, (int)x_dtype,
            (long)x_stride, (long)L, lengths, (int)W, (int)S, (int)P, (int)M, window, twiddle, mel_idx, mel_w, (int)n_mel_w, y,
            (long)y_stride, (long)Tmax);
  return wl_check_launch();
}

}  // extern "C"
