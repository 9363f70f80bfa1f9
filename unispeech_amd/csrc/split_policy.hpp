// Launch policy of the weight-gradient GEMMs (dW[N, K] += dy[n, N]^T x[n, K]), host code only: the ONE statement of these
// rules.  The fused block (layer.hip), the grouped launch (gemm_bf16.hip) and, through the wavlm_split_* / wavlm_linear_wgrads
// entry points, the Python autograd path and the CPU tests evaluate the functions below.  The arithmetic takes the grid, the
// forced split and the balanced flag as arguments; the settings underneath say what those are in this process.
#pragma once
#include <stdlib.h>

#include <algorithm>

#include "wavlm_hip.h"

#if defined(WAVLM_EXPERIMENTAL)   // the lab build (tools/probe/build_probe.py lab): the only one with the balanced launch
constexpr bool kLabLibrary = true;
#else
constexpr bool kLabLibrary = false;
#endif

namespace wl_policy {

// ------------------------------------------------------------------------------------------------ arithmetic
// split-K factor of a grouped launch, or 0 when the members should run as single launches.  Measured
// (profiles/r03/envab_wg.txt, Base: 108 tiles x 375 K-steps per layer, same box): ONE round of tiles * split work items is
// what pays -- split 2 (216 items) 335 us per layer against 349 us for the four single launches + 28 us less slab reduction;
// split 7 (2.95 rounds) 371 us and split 14 423 us although they balance the K-steps better: every extra round costs a slab
// store and a pipeline refill per CU.  So: the largest split that still fits one round of `grid` blocks, and no grouping when
// even split 2 does not (Large: 192 tiles).  forced > 0 overrides (A/B measurements).
inline long one_round(long tiles, long ktiles, long grid) {   // ... with at least 8 K-steps per slab, at most 64 slabs
  return std::min({grid / std::max(tiles, 1L), ktiles / 8, 64L});
}
inline int split_grouped(long tiles, long ktiles, long grid, int forced) {
  if (forced > 0) return forced < 2 ? 2 : forced;
  const int s = (int)one_round(tiles, ktiles, grid);
  return s >= 2 ? s : 0;
}

// `split_k` of a grouped launch's members = fp32 slabs each member's workspace holds: the one-round split.  balanced (lab
// library, gemm_common.hpp: gemm_sk_plan): one more, so that the CUs that split leaves idle (Base: 108 tiles x 2 = 216 of 256)
// take the K tail of every tile -- measured neutral (profiles/r04/ab_wgrad_balanced_*.txt: the launch is not bound by how many
// CUs take part), so libwavlm_hip.so does not carry that path.
inline int slabs_grouped(long tiles, long ktiles, long grid, int forced, bool balanced) {
  const int split = std::max(2, split_grouped(tiles, ktiles, grid, forced));
  if (balanced && forced <= 0 && tiles < grid && tiles * ktiles >= 8 * grid) return std::max(split, (int)(grid / tiles) + 1);
  return split;
}

// split-K factor of a single launch, so that a small-output / long-reduction GEMM still fills the chip.  Problems the
// 256 x 256 kernels take (one block per CU) aim at one full round of `grid` blocks; the 128-wide kernel (two to three blocks
// per CU) at 768 blocks.
inline int split_single(int M, int N, long ktiles, long grid) {
  if (M >= 256 && N >= 256) return (int)std::max(1L, one_round((long)((M + 255) / 256) * ((N + 255) / 256), ktiles, grid));
  const long tiles = (long)((M + 127) / 128) * ((N + 127) / 128);
  return (int)std::min(std::max(1L, std::min(ktiles, (768 + tiles - 1) / tiles)), 64L);
}

// -------------------------------------------------------------------------------------------------- settings
// (each variable is read once per process; empty or 0 = unset)
inline int env_int(const char* name) { const char* e = getenv(name); return e && *e ? atoi(e) : 0; }

// blocks of a persistent GEMM grid: one per CU minus what the data-parallel reducer keeps free for the RCCL kernels
// (wavlm_set_reserved_cus).  Every split-K choice aims at ONE round of THIS many blocks: with 8 CUs reserved, the 252 work
// items a 256-CU split produces run as a full round plus a round of four (measured: +17 % step time,
// profiles/r04/reserved_cus_base_before.txt).
constexpr int kFullGrid = 256;
inline int grid_blocks() { return kFullGrid - wavlm_get_reserved_cus(); }

inline int forced_split() { static const int f = env_int("WAVLM_WGRAD_SPLIT"); return f > 0 ? f : 0; }

// the balanced grouped launch is in this library and switched on
inline bool streamk() { static const bool on = kLabLibrary && env_int("WAVLM_WGRAD_STREAMK") > 0; return on; }

// the weight gradients of a block go out as grouped launches: anything but the literal "0" is on (atoi("auto") would be 0)
inline bool grouping() {
  static const bool on = [] { const char* e = getenv("WAVLM_WGRAD_GROUPING"); return !(e && e[0] == '0' && !e[1]); }();
  return on;
}

}  // namespace wl_policy
