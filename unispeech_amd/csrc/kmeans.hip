// k-means on the device for HuBERT / WavLM training targets (replaces the CPU work of the reference's
// src/examples/hubert/simple_kmeans/learn_kmeans.py (sklearn MiniBatchKMeans) and dump_km_label.py (ApplyKmeans)).
//
// Four entry points (include/wavlm_hip.h, "k-means"):
//   wavlm_kmeans_prepare     fp32 centres C [K, D] -> image: zero-padded [Kp, Dp] fp32 rows (Kp = K rounded up to 64,
//                            Dp = D rounded up to 32) followed by Cnorm [Kp] (sum_d c_d^2, one fmaf chain in d order)
//   wavlm_kmeans_assign      labels[n] = argmin_j (Cnorm_j - 2 x_n . c_j), min_dist[n] = sum_d (x_nd - c_{label,d})^2.
//                            The dot products run on v_mfma_f32_32x32x2_f32: an exact k-ordered fmaf chain per output,
//                            so the comparison is fp32-grade and identical centres give bit-identical scores.  A running
//                            (min, argmin) per accumulator register is kept across the centre tiles (scanned in
//                            increasing index order with strict <), then merged across the 32 lanes that share a row
//                            (equal values: the lower index wins).  No distance matrix, no cross-workgroup reduction.
//   wavlm_kmeans_accumulate  per-cluster sums [K, D] and counts [K] through a stable inverted index; bitwise
//                            reproducible, no float atomics (see the kernel comments)
//   wavlm_kmeans_update      Lloyd (c = sums / n) or sklearn's mini-batch rule (c = (c w + sums) / (w + n), w += n)
#include "common.hpp"
#include "../../include/wavlm_hip.h"

#include <math.h>

namespace {

constexpr int KM_BM = 128;    // rows of X per workgroup (4 waves x 32 rows)
constexpr int KM_BN = 64;     // centres per tile (two 32-wide MFMA column blocks per wave)
constexpr int KM_BK = 32;     // feature chunk staged through LDS
constexpr int KM_LDS = KM_BK + 1;  // padded row: lanes reading one column of 32 rows hit 32 different banks

constexpr int ACC_SEG_MAX = 2048;  // inverted-index segments (one thread each, rows in order)
constexpr int ACC_SEG_MIN_ROWS = 256;
constexpr int ACC_CHUNK = 256;     // longest run of rows one workgroup sums before the chunk partials are added

typedef __attribute__((ext_vector_type(16))) float f32x16;

__host__ __device__ inline int64_t round_up(int64_t a, int64_t b) { return (a + b - 1) / b * b; }

__device__ __forceinline__ float ld_x(const void* X, int dt, int64_t i) {
  return dt == WL_F32 ? ((const float*)X)[i] : bf2f(((const bf16_t*)X)[i]);
}

// ---------------------------------------------------------------- centre image
__global__ void km_prepare_kernel(const float* __restrict__ C, int K, int D, int Kp, int Dp, float* __restrict__ img) {
  const int64_t total = (int64_t)Kp * Dp;
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int j = (int)(e / Dp), d = (int)(e % Dp);
    img[e] = (j < K && d < D) ? C[(int64_t)j * D + d] : 0.f;
  }
}

__global__ void km_cnorm_kernel(const float* __restrict__ C, int K, int D, int Kp, float* __restrict__ cnorm) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= Kp) return;
  float s = 0.f;
  if (j < K)
    for (int d = 0; d < D; ++d) { const float v = C[(int64_t)j * D + d]; s = fmaf(v, v, s); }
  cnorm[j] = s;
}

// ---------------------------------------------------------------- assignment
// (v, i) better than (bv, bi): smaller value, equal value and lower index; bi < 0 = nothing yet
__device__ __forceinline__ bool km_better(float v, int i, float bv, int bi) {
  if (i < 0) return false;
  if (bi < 0) return true;
  return v < bv || (v == bv && i < bi);
}

__global__ __launch_bounds__(256) void km_assign_kernel(const void* __restrict__ X, int dt, int64_t N, int D, int64_t ldx,
                                                        const float* __restrict__ img, int K, int Kp, int Dp,
                                                        int* __restrict__ labels, float* __restrict__ min_dist) {
  __shared__ float Xs[KM_BM * KM_LDS];
  __shared__ float Cs[KM_BN * KM_LDS];
  __shared__ int row_label[KM_BM];
  const float* __restrict__ cnorm = img + (int64_t)Kp * Dp;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = lane & 31, half = lane >> 5;
  const int64_t m0 = (int64_t)blockIdx.x * KM_BM;

  float best[16];
  int bidx[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) { best[r] = INFINITY; bidx[r] = -1; }

  for (int n0 = 0; n0 < Kp; n0 += KM_BN) {
    f32x16 acc0 = {}, acc1 = {};
    for (int k0 = 0; k0 < Dp; k0 += KM_BK) {
      __syncthreads();
      // thread t stages column k0 + (t & 31) of rows (t >> 5) + 8 i: 32 lanes read 32 consecutive elements of one row
      {
        const int k = tid & 31, r0 = tid >> 5, c = k0 + k;
        const bool cin = c < D;
        int64_t off = (m0 + r0) * ldx + c;
#pragma unroll 4
        for (int i = 0; i < KM_BM / 8; ++i, off += 8 * ldx)
          Xs[(r0 + 8 * i) * KM_LDS + k] = (cin && m0 + r0 + 8 * i < N) ? ld_x(X, dt, off) : 0.f;
        const float* cp = img + (int64_t)(n0 + r0) * Dp + c;
#pragma unroll
        for (int i = 0; i < KM_BN / 8; ++i) Cs[(r0 + 8 * i) * KM_LDS + k] = cp[(int64_t)8 * i * Dp];
      }
      __syncthreads();
      const float* xa = Xs + (wave * 32 + col) * KM_LDS + half;
      const float* cb0 = Cs + col * KM_LDS + half;
      const float* cb1 = Cs + (32 + col) * KM_LDS + half;
#pragma unroll
      for (int kk = 0; kk < KM_BK; kk += 2) {
        const float a = xa[kk];
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, cb0[kk], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, cb1[kk], acc1, 0, 0, 0);
      }
    }
    // accumulator register r of this lane: row (r&3) + 8 (r>>2) + 4 half of the wave's 32 rows, centre n0 + col (+32)
    const int j0 = n0 + col, j1 = n0 + 32 + col;
    const float cn0 = cnorm[j0], cn1 = cnorm[j1];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      if (j0 < K) {
        const float v = fmaf(-2.f, acc0[r], cn0);
        if (v < best[r] || bidx[r] < 0) { best[r] = v; bidx[r] = j0; }
      }
      if (j1 < K) {
        const float v = fmaf(-2.f, acc1[r], cn1);
        if (v < best[r] || bidx[r] < 0) { best[r] = v; bidx[r] = j1; }
      }
    }
  }
  // merge the 32 lanes of each half (they hold the same rows, different centres)
#pragma unroll
  for (int r = 0; r < 16; ++r) {
#pragma unroll
    for (int m = 1; m < 32; m <<= 1) {
      const float ov = __shfl_xor(best[r], m);
      const int oi = __shfl_xor(bidx[r], m);
      if (km_better(ov, oi, best[r], bidx[r])) { best[r] = ov; bidx[r] = oi; }
    }
  }
  if (col == 0) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int rl = wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
      const int lab = bidx[r] < 0 ? 0 : bidx[r];
      row_label[rl] = lab;
      if (m0 + rl < N) labels[m0 + rl] = lab;
    }
  }
  if (!min_dist) return;
  __syncthreads();
  // distance to the chosen centre, summed as (x - c)^2 (no cancellation): lane-strided partials, then a fixed tree
  for (int rr = 0; rr < 32; ++rr) {
    const int rl = wave * 32 + rr;
    const int64_t row = m0 + rl;
    if (row >= N) break;
    const float* c = img + (int64_t)row_label[rl] * Dp;
    float s = 0.f;
    for (int d = lane; d < D; d += 64) { const float t = ld_x(X, dt, row * ldx + d) - c[d]; s = fmaf(t, t, s); }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m);
    if (lane == 0) min_dist[row] = s;
  }
}

// ---------------------------------------------------------------- accumulation
// Stable inverted index: the rows are cut into S contiguous segments, one thread each walks its segment in row order.
//   1 km_hist_kernel     hist[j][s] = rows of segment s with label j
//   2 km_scan_kernel     (one workgroup) counts[j]; start[j] = exclusive prefix of counts; hist[j][s] becomes the first
//                        slot of segment s in cluster j's list; chunk offsets cst[j] (ceil(n_j / ACC_CHUNK) chunks each)
//   3 km_scatter_kernel  idx[start + ...] = row ids, in increasing row order inside each cluster (stable)
//   4 km_chunk_kernel    one workgroup per chunk of <= ACC_CHUNK rows of one cluster, summed in list (= row) order; a
//                        cluster of any size is split into bounded chunks, so skewed cluster sizes do not serialise
//   5 km_finish_kernel   sums[j] = chunk partials added in chunk order
// Rows whose label is outside [0, K) are ignored.
__global__ void km_hist_kernel(const int* __restrict__ labels, int64_t N, int K, int S, int64_t R, int* __restrict__ hist) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S) return;
  for (int j = 0; j < K; ++j) hist[(int64_t)j * S + s] = 0;
  const int64_t r1 = min(N, (s + 1) * R);
  for (int64_t r = s * R; r < r1; ++r) {
    const int j = labels[r];
    if (j >= 0 && j < K) hist[(int64_t)j * S + s] += 1;
  }
}

__global__ __launch_bounds__(1024) void km_scan_kernel(int* __restrict__ hist, int K, int S, int* __restrict__ counts,
                                                       int* __restrict__ start, int* __restrict__ cst) {
  __shared__ int tot_n[1024], tot_c[1024];
  const int t = threadIdx.x;
  const int per = (K + 1023) / 1024;
  const int j0 = min(K, t * per), j1 = min(K, j0 + per);
  int sn = 0, sc = 0;
  for (int j = j0; j < j1; ++j) {
    int run = 0;
    for (int s = 0; s < S; ++s) { const int c = hist[(int64_t)j * S + s]; hist[(int64_t)j * S + s] = run; run += c; }
    counts[j] = run;
    sn += run;
    sc += (run + ACC_CHUNK - 1) / ACC_CHUNK;
  }
  tot_n[t] = sn;
  tot_c[t] = sc;
  __syncthreads();
  if (t == 0) {  // 1024 partial totals, serial: fixed order, negligible next to the passes over the rows
    int a = 0, b = 0;
    for (int i = 0; i < 1024; ++i) { const int x = tot_n[i], y = tot_c[i]; tot_n[i] = a; tot_c[i] = b; a += x; b += y; }
    start[K] = a;
    cst[K] = b;
  }
  __syncthreads();
  int a = tot_n[t], b = tot_c[t];
  for (int j = j0; j < j1; ++j) {
    start[j] = a;
    cst[j] = b;
    const int n = counts[j];
    for (int s = 0; s < S; ++s) hist[(int64_t)j * S + s] += a;
    a += n;
    b += (n + ACC_CHUNK - 1) / ACC_CHUNK;
  }
}

__global__ void km_scatter_kernel(const int* __restrict__ labels, int64_t N, int K, int S, int64_t R, int* __restrict__ hist,
                                  int* __restrict__ idx) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S) return;
  const int64_t r1 = min(N, (s + 1) * R);
  for (int64_t r = s * R; r < r1; ++r) {
    const int j = labels[r];
    if (j >= 0 && j < K) {
      const int64_t p = (int64_t)j * S + s;
      const int pos = hist[p];
      hist[p] = pos + 1;
      idx[pos] = (int)r;
    }
  }
}

__global__ __launch_bounds__(256) void km_chunk_kernel(const void* __restrict__ X, int dt, int D, int64_t ldx, int K,
                                                       const int* __restrict__ idx, const int* __restrict__ start,
                                                       const int* __restrict__ cst, float* __restrict__ partial) {
  __shared__ int rows[ACC_CHUNK];
  const int c = blockIdx.x;
  if (c >= cst[K]) return;
  int lo = 0, hi = K;  // largest j with cst[j] <= c (then c < cst[j + 1])
  while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (cst[mid] <= c) lo = mid; else hi = mid; }
  const int j = lo;
  const int p0 = start[j] + (c - cst[j]) * ACC_CHUNK;
  const int n = min(ACC_CHUNK, start[j + 1] - p0);
  if ((int)threadIdx.x < n) rows[threadIdx.x] = idx[p0 + threadIdx.x];
  __syncthreads();
  for (int d = threadIdx.x; d < D; d += 256) {
    float s = 0.f;
    for (int p = 0; p < n; ++p) s += ld_x(X, dt, (int64_t)rows[p] * ldx + d);
    partial[(int64_t)c * D + d] = s;
  }
}

__global__ __launch_bounds__(256) void km_finish_kernel(const float* __restrict__ partial, const int* __restrict__ cst, int D,
                                                        float* __restrict__ sums) {
  const int j = blockIdx.x;
  const int c0 = cst[j], c1 = cst[j + 1];
  for (int d = threadIdx.x; d < D; d += 256) {
    float s = 0.f;
    for (int c = c0; c < c1; ++c) s += partial[(int64_t)c * D + d];
    sums[(int64_t)j * D + d] = s;
  }
}

struct AccLayout {
  int S;
  int64_t R, max_chunks;
  uint64_t hist, idx, start, cst, partial, total;
};

AccLayout acc_layout(int64_t N, int K, int D) {
  AccLayout L;
  int64_t S = (N + ACC_SEG_MIN_ROWS - 1) / ACC_SEG_MIN_ROWS;
  if (S > ACC_SEG_MAX) S = ACC_SEG_MAX;
  if (S < 1) S = 1;
  L.R = (N + S - 1) / S;
  L.S = (int)((N + L.R - 1) / L.R);
  if (L.S < 1) L.S = 1;
  L.max_chunks = (N + ACC_CHUNK - 1) / ACC_CHUNK + K;
  uint64_t o = 0;
  auto take = [&](uint64_t b) { const uint64_t at = o; o += (uint64_t)round_up((int64_t)b, 256); return at; };
  L.hist = take((uint64_t)K * L.S * 4);
  L.idx = take((uint64_t)N * 4);
  L.start = take((uint64_t)(K + 1) * 4);
  L.cst = take((uint64_t)(K + 1) * 4);
  L.partial = take((uint64_t)L.max_chunks * D * 4);
  L.total = o;
  return L;
}

// ---------------------------------------------------------------- centre update
__global__ __launch_bounds__(256) void km_update_kernel(float* __restrict__ C, float* __restrict__ w,
                                                        const float* __restrict__ sums, const int* __restrict__ counts,
                                                        int D, int mode) {
  const int j = blockIdx.x;
  const int n = counts[j];
  if (n <= 0) return;  // empty in this batch / pass: the centre stays where it is
  float* c = C + (int64_t)j * D;
  const float* s = sums + (int64_t)j * D;
  if (mode == 0) {
    const float fn = (float)n;
    for (int d = threadIdx.x; d < D; d += 256) c[d] = s[d] / fn;
    return;
  }
  const float wo = w[j];
  const float wn = wo + (float)n;
  const float alpha = 1.f / wn;
  for (int d = threadIdx.x; d < D; d += 256) c[d] = __fmul_rn(__fadd_rn(__fmul_rn(c[d], wo), s[d]), alpha);
  __syncthreads();
  if (threadIdx.x == 0) w[j] = wn;
}

}  // namespace

extern "C" {

uint64_t wavlm_kmeans_centres_bytes(int32_t K, int32_t D) {
  if (K <= 0 || D <= 0) return 0;
  const int64_t Kp = round_up(K, KM_BN), Dp = round_up(D, KM_BK);
  return (uint64_t)(Kp * Dp + Kp) * sizeof(float);
}

int wavlm_kmeans_prepare(const float* C, int32_t K, int32_t D, void* image, uint64_t image_bytes, void* stream) {
  if (!C || !image || K <= 0 || D <= 0 || image_bytes < wavlm_kmeans_centres_bytes(K, D)) return WL_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const int Kp = (int)round_up(K, KM_BN), Dp = (int)round_up(D, KM_BK);
  float* img = (float*)image;
  const int64_t total = (int64_t)Kp * Dp;
  const int blocks = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
  WL_LAUNCH(km_prepare_kernel, dim3(blocks), dim3(256), 0, st, C, (int)K, (int)D, Kp, Dp, img);
  WL_LAUNCH(km_cnorm_kernel, dim3((Kp + 255) / 256), dim3(256), 0, st, C, (int)K, (int)D, Kp, img + total);
  return wl_check_launch();
}

int wavlm_kmeans_assign(const void* X, int32_t x_dtype, int64_t N, int32_t D, int64_t ldx, const void* image, int32_t K,
                        int32_t* labels, float* min_dist, void* stream) {
  if (!X || !image || !labels || N <= 0 || D <= 0 || K <= 0 || ldx < D || (x_dtype != WL_F32 && x_dtype != WL_BF16))
    return WL_EINVAL;
  if ((N + KM_BM - 1) / KM_BM > 0x7fffffff) return WL_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const int Kp = (int)round_up(K, KM_BN), Dp = (int)round_up(D, KM_BK);
  WL_LAUNCH(km_assign_kernel, dim3((unsigned)((N + KM_BM - 1) / KM_BM)), dim3(256), 0, st, X, (int)x_dtype, N, (int)D, ldx,
            (const float*)image, (int)K, Kp, Dp, (int*)labels, min_dist);
  return wl_check_launch();
}

uint64_t wavlm_kmeans_accumulate_workspace_bytes(int64_t N, int32_t K, int32_t D) {
  if (N <= 0 || K <= 0 || D <= 0 || N > 0x7fffffff) return 0;
  return acc_layout(N, K, D).total;
}

int wavlm_kmeans_accumulate(const void* X, int32_t x_dtype, int64_t N, int32_t D, int64_t ldx, const int32_t* labels,
                            int32_t K, float* sums, int32_t* counts, void* workspace, uint64_t ws_bytes, void* stream) {
  if (!X || !labels || !sums || !counts || !workspace || N <= 0 || N > 0x7fffffff || D <= 0 || K <= 0 || ldx < D ||
      (x_dtype != WL_F32 && x_dtype != WL_BF16))
    return WL_EINVAL;
  const AccLayout L = acc_layout(N, K, D);
  if (ws_bytes < L.total || L.max_chunks > 0x7fffffff) return WL_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  int* hist = (int*)(ws + L.hist);
  int* idx = (int*)(ws + L.idx);
  int* start = (int*)(ws + L.start);
  int* cst = (int*)(ws + L.cst);
  float* partial = (float*)(ws + L.partial);
  const int sb = (L.S + 255) / 256;
  WL_LAUNCH(km_hist_kernel, dim3(sb), dim3(256), 0, st, (const int*)labels, N, (int)K, L.S, L.R, hist);
  WL_LAUNCH(km_scan_kernel, dim3(1), dim3(1024), 0, st, hist, (int)K, L.S, (int*)counts, start, cst);
  WL_LAUNCH(km_scatter_kernel, dim3(sb), dim3(256), 0, st, (const int*)labels, N, (int)K, L.S, L.R, hist, idx);
  WL_LAUNCH(km_chunk_kernel, dim3((unsigned)L.max_chunks), dim3(256), 0, st, X, (int)x_dtype, (int)D, ldx, (int)K, idx,
            start, cst, partial);
  WL_LAUNCH(km_finish_kernel, dim3(K), dim3(256), 0, st, partial, cst, (int)D, sums);
  return wl_check_launch();
}

int wavlm_kmeans_update(float* C, float* weights, const float* sums, const int32_t* counts, int32_t K, int32_t D,
                        int32_t mode, void* stream) {
  if (!C || !sums || !counts || K <= 0 || D <= 0 || (mode != 0 && mode != 1) || (mode == 1 && !weights)) return WL_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  WL_LAUNCH(km_update_kernel, dim3(K), dim3(256), 0, st, C, weights, sums, (const int*)counts, (int)D, (int)mode);
  return wl_check_launch();
}

}  // extern "C"
