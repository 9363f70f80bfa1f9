// Polyphase windowed-sinc resampler (ABI 27): torchaudio.functional.resample with sinc_interpolation, the step the reference's
// speaker and diarization recipes put in front of the upstream (downstreams/speaker_diarization/models/models.py:138,207
// `torchaudio.transforms.Resample(sr, 16000)`, downstreams/speaker_verification/verification.py:46-49).
//
//   o = orig / gcd, n = new / gcd;   y[f * n + i] = sum_k h_i[k] * xpad[f * o + k],   k < 2 * width + o
// with xpad = x behind `width` zeros.  Outside |t| < 6 the Hann window is zero, so phase i has at most 2 * width + 1 taps that
// matter; the host hands over exactly TC = 2 * width + 1 taps per phase (unispeech_amd/resample.py: float64, rounded to fp32,
// zero where the window is) and the index `first[i]` of the first of them:
//   y[f * n + i] = sum_{j < TC} tab[i][j] * x[f * o + first[i] + j - width]          (x = 0 outside [0, len))
// One launch; a workgroup owns FT frames (FT * n consecutive outputs) of one row.  The table, `first` and the FT * o + 2 * width
// input samples the tile touches go to LDS once (wave_input.hpp: the input layer shared with mfcc.hip and fbank.hip), so HBM
// sees every input sample once per tile (+ 2 * width of overlap) and every output once.
// A thread computes RS outputs of ONE phase, FT / RS frames apart: each tap is read from LDS once for RS multiply-adds, and
// consecutive lanes hold consecutive outputs (coalesced stores; tap rows TC dwords apart with TC odd: no bank conflicts).
// Arithmetic: fp32 fmaf over j = 0 .. TC - 1 in that order, one thread per output: a row's result depends on nothing but the
// row -- bit-identical wherever it sits in the batch.
#include "common.hpp"
#include "wave_input.hpp"
#include "../../include/wavlm_hip.h"

#define RS_NT 256
#define RS_RS 4                     // outputs per thread and pass (same phase)
#define RS_TILE_OUT 4096            // outputs per workgroup aimed at
#define RS_X_FLOATS 8192            // input tile budget (32 KiB)
#define RS_TAB_BYTES (48 * 1024)    // compact table + first-index budget

// frames per tile, 0 if the ratio does not fit the LDS budgets
static inline int rs_tile_frames(int64_t o, int64_t n, int64_t width) {
  if (o < 1 || n < 1 || width < 1 || o > (1 << 20) || n > (1 << 20) || width > (1 << 20)) return 0;
  const int64_t tc = 2 * width + 1;
  if (n * (tc + 1) * 4 > RS_TAB_BYTES) return 0;
  // every tile reads the whole table (from L2): a large table asks for a tile of at least twice as many outputs
  const int64_t want = 2 * n * tc > RS_TILE_OUT ? 2 * n * tc : RS_TILE_OUT;
  int64_t ft = (want + n - 1) / n;
  ft = (ft + RS_RS - 1) / RS_RS * RS_RS;
  const int64_t fit = (RS_X_FLOATS - 2 * width) / o / RS_RS * RS_RS;
  if (RS_X_FLOATS < 2 * width || fit < RS_RS) return 0;
  return (int)(ft < fit ? ft : fit);
}

__global__ __launch_bounds__(RS_NT) void resample_kernel(const void* __restrict__ x, int x_dt, long x_stride, long L,
    const int* __restrict__ lengths, const float* __restrict__ tab, const int* __restrict__ first, int o, int n, int width,
    int FT, void* __restrict__ y, int y_dt, long y_stride, long L_out) {
  extern __shared__ __attribute__((aligned(16))) float rs_lds[];
  const int TC = 2 * width + 1;
  float* s_tab = rs_lds;                     // [n][TC]
  int* s_first = (int*)(s_tab + n * TC);     // [n]
  float* s_x = (float*)(s_first + n);        // [FT * o + 2 * width]: s_x[k] = x[f0 * o - width + k]
  const int b = blockIdx.y;
  const long f0 = (long)blockIdx.x * FT;
  const long len = wave_row_len(lengths, b, L);
  const long len_out = (len * n + o - 1) / o;              // this row's samples; [len_out, L_out) is written as zero
  const long m0 = f0 * n;
  long m1 = m0 + (long)FT * n;
  if (m1 > L_out) m1 = L_out;
  void* yrow = (char*)y + (size_t)b * y_stride * (y_dt == WL_BF16 ? 2 : 4);
  if (m0 >= len_out) {                                     // nothing of the row reaches this tile
    for (long m = m0 + threadIdx.x; m < m1; m += RS_NT) st_elem(yrow, m, y_dt, 0.f);
    return;
  }
  const void* xrow = wave_row(x, b, x_stride, x_dt);
  for (int k = threadIdx.x; k < n * TC; k += RS_NT) s_tab[k] = tab[k];
  const int first_max = 2 * width + o - TC;                // keeps first[i] + TC - 1 inside the dense 2 * width + o taps
  for (int k = threadIdx.x; k < n; k += RS_NT) { const int s = first[k]; s_first[k] = s < 0 ? 0 : (s > first_max ? first_max : s); }
  wave_stage(s_x, xrow, x_dt, f0 * o - width, FT * o + 2 * width, len, threadIdx.x, RS_NT);
  __syncthreads();
  const int FQ = FT / RS_RS;                               // frames between a thread's outputs
  for (int q = threadIdx.x; q < FQ * n; q += RS_NT) {
    const int fg = q / n, i = q - fg * n;
    const float* h = s_tab + i * TC;
    const float* xs = s_x + fg * o + s_first[i];
    float acc[RS_RS];
#pragma unroll
    for (int r = 0; r < RS_RS; ++r) acc[r] = 0.f;
    for (int j = 0; j < TC; ++j) {
      const float hj = h[j];
#pragma unroll
      for (int r = 0; r < RS_RS; ++r) acc[r] = fmaf(hj, xs[r * FQ * o + j], acc[r]);
    }
#pragma unroll
    for (int r = 0; r < RS_RS; ++r) {
      const long m = m0 + (long)(fg + r * FQ) * n + i;
      if (m < m1) st_elem(yrow, m, y_dt, m < len_out ? acc[r] : 0.f);
    }
  }
}

extern "C" {

// 1 if wavlm_resample_rows takes the reduced ratio o : n with this filter half-width (table and tile fit the LDS budget)
int wavlm_resample_supported(int32_t o, int32_t n, int32_t width) { return rs_tile_frames(o, n, width) > 0 ? 1 : 0; }

int wavlm_resample_rows(const void* x, int32_t x_dtype, int64_t x_stride, int32_t B, int64_t L, const int32_t* lengths,
                        const float* table, const int32_t* first, int32_t o, int32_t n, int32_t width, void* y,
                        int32_t y_dtype, int64_t y_stride, void* stream) {
  if (wave_check_input(x, x_dtype, x_stride, B, L, INT64_MAX >> 22) != WL_OK) return WL_EINVAL;   // n * L stays far inside int64
  if (!y || !table || !first || (y_dtype != WL_F32 && y_dtype != WL_BF16)) return WL_EINVAL;
  const int FT = rs_tile_frames(o, n, width);
  if (FT <= 0) return WL_EINVAL;
  const int64_t L_out = (L * n + o - 1) / o;
  if (y_stride < L_out) return WL_EINVAL;
  const int64_t frames = (L_out + n - 1) / n;
  const int64_t tiles = (frames + FT - 1) / FT;
  if (tiles > 0x7fffffffLL) return WL_EINVAL;
  const int64_t tc = 2 * (int64_t)width + 1;
  const size_t smem = (size_t)((int64_t)n * (tc + 1) + (int64_t)FT * o + 2 * (int64_t)width) * sizeof(float);
  if (wl_dynamic_lds(resample_kernel, smem, (int)(RS_TAB_BYTES + RS_X_FLOATS * sizeof(float))) != WL_OK) return WL_ELAUNCH;
  WL_LAUNCH(resample_kernel, dim3((unsigned)tiles, (unsigned)B), dim3(RS_NT), smem, (hipStream_t)stream, x, (int)x_dtype,
            (long)x_stride, (long)L, lengths, table, first, (int)o, (int)n, (int)width, FT, y, (int)y_dtype, (long)y_stride,
            (long)L_out);
  return wl_check_launch();
}

}  // extern "C"
