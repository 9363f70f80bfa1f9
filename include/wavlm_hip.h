/*
 * wavlm_hip.h -- C ABI of libwavlm_hip.so: the MI355X (gfx950) kernels of the WavLM / UniSpeech
 * pre-training hot path.
 *
 * The reference (microsoft/UniSpeech) has NO native interface on this path: every FLOP is a stock
 * PyTorch op called from Python.  Each entry point below therefore cites the reference *Python*
 * call site whose arithmetic it replaces (paths relative to the reference root).  A maintainer
 * binds the library with ctypes (INTEGRATION.md shows the stub); unispeech_amd/_lib.py is that
 * binding.
 *
 * Conventions (all entry points):
 *   - plain device pointers + sizes; no torch types; `stream` is a hipStream_t passed as void*
 *   - returns 0 on success, <0 on error (-1 bad argument, -2 launch failure); never throws,
 *     never allocates, never synchronises -- with ONE exception: the first GELU-epilogue launch on a device fills a
 *     32 KiB chord table and waits for it (once per device and process; every later launch reads one atomic pointer)
 *   - dtype codes: 0 = float32, 1 = bfloat16 (raw 16-bit)
 *   - activations are channel-last: [B, T, C] row-major ("rows" = frames, contiguous channels)
 */
#ifndef WAVLM_HIP_H
#define WAVLM_HIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define WAVLM_HIP_ABI_VERSION 30
int wavlm_abi_version(void);

/* ------------------------------------------------------------------------------------------
 * Dense contraction (MFMA for bf16, exact-f32 VALU tile for the parity mode).
 *   C[zo,zi][m,n] = epi( alpha * sum_{kb<KB} sum_{k<K} A[zo,zi,kb](m,k) * B[zo,zi,kb](n,k) + bias[n] )
 * A(m,k) lives at A + zo*sA_o + zi*sA_i + kb*sA_kb + (transA ? k*lda + m : m*lda + k); same for B.
 * lda may be SMALLER than K (overlapping rows): that is how a strided Conv1d over a channel-last
 * activation becomes a GEMM with no im2col.
 * Replaces: F.linear (WavLM/WavLM.py:348, modules.py:540-563 q/k/v/out, WavLM.py:671-672 fc1/fc2),
 * nn.Conv1d of the feature extractor (WavLM/WavLM.py:401,499-500), the grouped pos_conv
 * (WavLM/WavLM.py:514-527), torch.bmm inside F.multi_head_attention_forward, the cosine-logit
 * product (src/fairseq/models/wavlm/wavlm.py:431) and all their autograd backward contractions.
 * epi: 0 none | 1 gelu (pre-activation stored to aux if aux != NULL) | 2 multiply by gelu'(aux)
 *      | 3 gelu (gelu'(pre-activation) stored to aux if aux != NULL) | 4 multiply by aux
 *      (3 / 4 are the training pair: forward pays three extra VALU ops per element, backward saves an erf + exp)
 * then: + res (if res != NULL), + old C (if accumulate).
 * split_k > 1: the KB range is cut into split_k slabs written to `workspace` (f32) and summed by a
 * second kernel (deterministic, no atomics).  workspace bytes >= wavlm_gemm_workspace_bytes().
 * ------------------------------------------------------------------------------------------ */
typedef struct wavlm_gemm_desc {
  int32_t dtype;      /* element type of A and B */
  int32_t c_dtype;    /* element type of C */
  int32_t M, N, K, KB;
  int32_t transA, transB;
  int64_t lda, ldb, ldc;
  int64_t sA_kb, sB_kb;
  int32_t batch_o, batch_i;
  int64_t sA_o, sA_i, sB_o, sB_i, sC_o, sC_i;
  const void* A;
  const void* B;
  void* C;
  float alpha;
  int32_t epi;
  const void* bias; int32_t bias_dtype; int64_t sBias_o, sBias_i;
  void* aux; int32_t aux_dtype; int64_t ld_aux, sAux_o, sAux_i;
  const void* res; int32_t res_dtype; int64_t ld_res, sRes_o, sRes_i;
  int32_t accumulate;
  int32_t split_k;
  void* workspace; uint64_t ws_bytes;
  /* optional: colsum[n] (+)= sum_m C[m][n] over the rows of the (un-batched, un-split) result, in colsum_dtype -- the bias
   * gradient of the linear whose output gradient C is (fc1's from fc2's GELU'-multiplying dX GEMM, WavLM/WavLM.py:732-737).
   * Computed inside the GEMM's epilogue where the kernel supports it (per-tile partial rows in `workspace` + one finishing
   * launch), otherwise by a column-sum pass over C; either way `workspace` must hold wavlm_gemm_workspace_bytes(). */
  void* colsum; int32_t colsum_dtype; int32_t colsum_accumulate;
} wavlm_gemm_desc;

uint64_t wavlm_gemm_workspace_bytes(const wavlm_gemm_desc* d);
int wavlm_gemm(const wavlm_gemm_desc* d, void* stream);
/* n descriptors in one call.  Weight-gradient-shaped problems (transA && transB, same K and split_k >= 2, no epilogue
 * extras, each with its own workspace) run as ONE grouped split-K launch + one slab reduction each -- the four dW of an
 * encoder layer (modules.py q/k/v/out_proj, WavLM.py:732-737 fc1/fc2) share the reduction length B*T; anything else is
 * executed as n wavlm_gemm calls.  Results are identical either way.  Callers should pick `split_k` so that all members' tiles x
 * split_k fit ONE round of the persistent grid (256 CUs minus wavlm_set_reserved_cus): wavlm_slabs_grouped below says how many,
 * and wavlm_linear_wgrads does all of it.  In the lab build under WAVLM_WGRAD_STREAMK=1 `split_k` may be one larger than that
 * (= the fp32 slabs the workspace holds): the library then runs a balanced partition in which the CUs the one-round split
 * leaves idle take the K tail of every tile (measured neutral: off by default). */
int wavlm_gemm_grouped(const wavlm_gemm_desc* d, int32_t n, void* stream);

/* Launch policy of the weight-gradient GEMMs (csrc/split_policy.hpp; host functions, no GPU needed).  tiles = 256 x 256
 * output tiles, ktiles = 64-row steps of the reduction.  grid = 0, forced < 0, balanced < 0 ask for the process's own
 * settings: 256 minus wavlm_set_reserved_cus, WAVLM_WGRAD_SPLIT, and "lab build with WAVLM_WGRAD_STREAMK" (both variables
 * are read once per process; empty or 0 = unset).  Explicit values evaluate the same arithmetic anywhere.
 *   wavlm_grid_blocks     blocks of a persistent GEMM grid
 *   wavlm_split_single    split_k of one dW[M, N] launch
 *   wavlm_split_grouped   split_k that keeps a grouped launch within ONE round of the grid; 0 = run the members singly
 *   wavlm_slabs_grouped   `split_k` of a grouped launch's members = fp32 slabs per member (one more for the balanced launch)
 *   wavlm_wgrad_grouping  0 iff WAVLM_WGRAD_GROUPING=0: every weight gradient goes out as a single launch */
int32_t wavlm_grid_blocks(void);
int32_t wavlm_split_single(int32_t M, int32_t N, int64_t ktiles, int32_t grid);
int32_t wavlm_split_grouped(int64_t tiles, int64_t ktiles, int32_t grid, int32_t forced);
int32_t wavlm_slabs_grouped(int64_t tiles, int64_t ktiles, int32_t grid, int32_t forced, int32_t balanced);
int32_t wavlm_wgrad_grouping(void);

/* dW_i[N_i, K_i] += dy_i[rows, N_i]^T x_i[rows, K_i] for the linears of one block (bf16 operands, dW in c_dtype; F.linear's
 * weight gradient: modules.py q/k/v/out_proj, WavLM.py:732-737 fc1/fc2), issued under the policy above: consecutive items are
 * packed into grouped launches of at most four while their tiles fit one round with a split >= 2, the rest run singly.
 * wavlm_encoder_layer_bwd issues its four weight gradients through this call.  The workspace size is an upper bound over
 * every packing and every CU reservation, so it stays valid if wavlm_set_reserved_cus is called between query and launch. */
typedef struct wavlm_wgrad_item {
  const void* dy;
  const void* x;
  void* dW;
  int32_t N, K;
} wavlm_wgrad_item;
uint64_t wavlm_linear_wgrads_workspace_bytes(const wavlm_wgrad_item* items, int32_t n_items, int64_t rows);
int wavlm_linear_wgrads(const wavlm_wgrad_item* items, int32_t n_items, int64_t rows, int32_t c_dtype, void* workspace,
                        uint64_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Row kernels (one 64-lane wave per row, wave-shuffle reductions).
 * ------------------------------------------------------------------------------------------ */

/* y = dropout_out( act( LayerNorm( x + dropout_in(r) ) ) ).  r may be NULL.  s (optional) receives the
 * pre-norm sum, mean/rstd (optional) the row statistics -- backward needs all three.  act: 0 none, 1 gelu.
 * Replaces nn.LayerNorm / Fp32LayerNorm + the residual add + nn.Dropout around it
 * (WavLM/WavLM.py:342, 582-584, 702-703, 726-729, 739-740; WavLM/modules.py:30-42). D % 8 == 0, D <= 2048. */
int wavlm_layernorm_fwd(const void* x, const void* r, void* y, void* s, float* mean, float* rstd, const void* gamma,
                        const void* beta, int64_t rows, int32_t D, float eps, int32_t dtype, int32_t param_dtype,
                        int32_t act, float p_in, uint64_t seed_in, float p_out, uint64_t seed_out, void* stream);
uint64_t wavlm_layernorm_bwd_workspace_bytes(int32_t D);
/* dx: gradient of x (and of the sum s); dr (optional): gradient of r (dx through the input-dropout mask);
 * dgamma/dbeta in param dtype; dy is scaled by grad_scale first (GradMultiply, WavLM/modules.py:60-69).
 * dr_colsum (optional, [D], param dtype, same accumulate flag): column sums of the gradient of r, i.e. the bias
 * gradient of the nn.Linear whose output r is (out_proj / fc2 of a post-LN block, WavLM/WavLM.py:726-740) -- it falls
 * out of the pass that already reduces dgamma / dbeta over rows.
 * dx_add (optional, same shape / dtype as dx): added into dx -- the gradient that reaches x past the LayerNorm, i.e. the
 * residual stream of a layer_norm_first block (WavLM/WavLM.py:702-724: `residual = x; x = layer_norm(x); ...; x =
 * residual + x`), so the two contributions never meet in a separate add kernel.  dr / dr_colsum do not include it unless
 * dr_incl_add != 0: then the SUM s = x + dropout(r) is itself the residual stream (a pre-LN block whose residual add is
 * fused into the following LayerNorm) and the gradient arriving at s reaches r as well (through the dropout mask). */
int wavlm_layernorm_bwd(const void* dy, const void* s, const float* mean, const float* rstd, const void* gamma,
                        const void* beta, void* dx, void* dr, const void* dx_add, void* dgamma, void* dbeta,
                        void* dr_colsum, int64_t rows, int32_t D, int32_t dtype, int32_t param_dtype, int32_t act,
                        float p_in, uint64_t seed_in, float p_out, uint64_t seed_out, float grad_scale,
                        int32_t accumulate_params, int32_t dr_incl_add, void* workspace, uint64_t ws_bytes, void* stream);
/* The same with a segmented dx: row r of the b-th run of dx_seg_rows rows is written at row r + b * dx_seg_gap of dx (the
 * caller zero-fills the gaps) -- the zero-padded per-utterance layout that the data-gradient GEMMs of the conv layer in
 * front of this LayerNorm read (layer_norm extractor mode: WavLM/WavLM.py:403-418), so that no padded copy of the gradient is
 * made.  dx_seg_rows = 0: contiguous.  D in {512, 768, 1024} only (WL_EINVAL otherwise). */
int wavlm_layernorm_bwd_seg(const void* dy, const void* s, const float* mean, const float* rstd, const void* gamma,
                            const void* beta, void* dx, void* dr, const void* dx_add, void* dgamma, void* dbeta,
                            void* dr_colsum, int64_t rows, int32_t D, int32_t dtype, int32_t param_dtype, int32_t act,
                            float p_in, uint64_t seed_in, float p_out, uint64_t seed_out, float grad_scale,
                            int32_t accumulate_params, int32_t dr_incl_add, int32_t dx_seg_rows, int32_t dx_seg_gap,
                            void* workspace, uint64_t ws_bytes, void* stream);

/* out[c] (+)= sum over rows of x[row, c]; a row counts iff (!include || include[row]) && (!exclude || !exclude[row]).
 * Bias gradients of every nn.Linear / conv bias, and d(mask_emb) (src/fairseq/models/wavlm/wavlm.py:401). */
uint64_t wavlm_colsum_workspace_bytes(int32_t N);
int wavlm_colsum(const void* x, int64_t rows, int32_t N, int64_t ld, int32_t dtype, const uint8_t* include_mask,
                 const uint8_t* exclude_mask, void* out, int32_t out_dtype, int32_t accumulate, void* workspace,
                 uint64_t ws_bytes, void* stream);

/* y[row] = zero[row] ? 0 : (sel[row] ? emb (0 if emb == NULL) : x[row]).  apply_mask's x[mask] = mask_emb and the
 * encoder's x[padding_mask] = 0 in one pass (WavLM/WavLM.py:286, 574-575), and their backward. */
int wavlm_select_rows(const void* x, void* y, const uint8_t* sel, const void* emb, const uint8_t* zero, int64_t rows,
                      int32_t D, int32_t dtype, int32_t emb_dtype, void* stream);
/* dst[i] = idx[i] >= 0 ? src[idx[i]] : 0.  x[masked_indices] (wavlm.py:541,557) and its scatter-back. */
int wavlm_gather_rows(const void* src, const int32_t* idx, void* dst, int64_t n_out, int32_t D, int32_t dtype,
                      void* stream);
/* Operand images of the feature extractor's Conv1d weights (WavLM/WavLM.py:378-504: conv_layers.{i}.0.weight
 * [Cout, Cin, k]) for every layer of the stack in ONE launch: Wf[l] = [Cout][k * Cin] (forward GEMM over overlapping
 * rows) and, if Wb[l] != NULL, the s[l] stride-phase images of the data-gradient GEMMs back to back, phase r as
 * [Cin][J_r * Cout] with J_r = ceil((k - r) / s) taps newest first.  wavlm_conv_wgrad_scatter is the way back for the
 * weight gradients: W[l][co][ci][kk] (+)= Wf[l][co][kk * Cin + ci] (here W = the gradient tensors, Wf = the GEMM outputs). */
#define WL_CONV_RELAYOUT_MAX 8
typedef struct {
  const void* W[WL_CONV_RELAYOUT_MAX];
  void* Wf[WL_CONV_RELAYOUT_MAX];
  void* Wb[WL_CONV_RELAYOUT_MAX];
  int32_t Cout[WL_CONV_RELAYOUT_MAX], Cin[WL_CONV_RELAYOUT_MAX], k[WL_CONV_RELAYOUT_MAX], s[WL_CONV_RELAYOUT_MAX];
  int32_t n_layers, dtype;
} wavlm_conv_relayout_desc;
int wavlm_conv_weights_relayout(const wavlm_conv_relayout_desc* d, void* stream);
int wavlm_conv_wgrad_scatter(const wavlm_conv_relayout_desc* d, int32_t accumulate, void* stream);
/* y = a*x + b*y */
int wavlm_axpby(const void* x, int32_t x_dtype, void* y, int32_t y_dtype, int64_t n, float a, float b, void* stream);
/* y *= scalar[0] * extra, scalar on the device (upstream loss gradient without a host sync) */
int wavlm_scale_dev(void* y, int32_t dtype, int64_t n, const float* scalar, float extra, void* stream);
/* y = dropout(x; p, seed): counter-based (Philox4x32-10) mask, regenerated (not stored) for the backward. */
int wavlm_dropout(const void* x, void* y, int64_t n, float p, uint64_t seed, int32_t dtype, void* stream);
/* y = x + dropout(r, p, seed): residual add of a pre-LN block (unispeech_sat.py:1088-1111 `x = residual + dropout(x)`);
 * same mask as wavlm_dropout for the same seed (the backward of the dropped branch is wavlm_dropout(dy)) */
int wavlm_dropout_add(const void* x, const void* r, void* y, int64_t n, float p, uint64_t seed, int32_t dtype, void* stream);
/* UniSpeech's replace-mix (src/fairseq/models/unispeech/unispeech.py:107-112: x.masked_fill(r, 0) + q.masked_fill(~r, 0), then
 * final_dropout) in one launch: y[row, :] = dropout(sel[row] ? q[row, :] : x[row, :], p, seed).  x, q, y: [rows, D] row-major,
 * fp32 or bf16, 16-byte aligned, D % 8 == 0; sel: uint8 [rows].  Only the selected source row is read (one read and one write of
 * rows x D).  The keep decision of element row * D + c is wavlm_dropout's for the same seed and flat index; p = 0 is a plain
 * select.  _bwd: dx[row, :] = sel[row] ? 0 : dropout(g[row, :]), dq[row, :] = sel[row] ? dropout(g[row, :]) : 0, the mask
 * recomputed from the seed.  No workspace, no atomics.  -1 for a NULL pointer, D % 8 != 0 or p outside [0, 1); rows == 0 is 0.
 * Additive to ABI 30 (two new symbols, nothing else changes). */
int wavlm_replace_mix(const void* x, const void* q, const uint8_t* sel, void* y, int64_t rows, int32_t D, float p, uint64_t seed,
                      int32_t dtype, void* stream);
int wavlm_replace_mix_bwd(const void* g, const uint8_t* sel, void* dx, void* dq, int64_t rows, int32_t D, float p, uint64_t seed,
                          int32_t dtype, void* stream);
/* out[0] = scale * sum(x^2): features_pen (wavlm.py:486) and the global gradient norm (utils.py:338-388). */
uint64_t wavlm_sumsq_workspace_bytes(void);
int wavlm_sumsq(const void* x, int32_t dtype, int64_t n, float scale, float* out, void* workspace, uint64_t ws_bytes,
                void* stream);

/* ------------------------------------------------------------------------------------------
 * conv0: Conv1d(1->C, k=10, stride) + GroupNorm(C, C) + GELU, channel-last output [B, T0, C]
 * (WavLM/WavLM.py:401-428 block(is_group_norm=True); Fp32GroupNorm WavLM/modules.py:45-57).
 * stats[B, C, 2] = (mean, rstd) saved for backward.  kw must be 10, C <= 512.
 * ------------------------------------------------------------------------------------------ */
uint64_t wavlm_conv0_gn_workspace_bytes(int32_t B, int64_t T, int32_t C, int32_t stride);
int wavlm_conv0_gn_gelu_fwd(const void* wav, int32_t wav_dtype, const void* W, const void* gamma, const void* beta,
                            int32_t param_dtype, void* out, int32_t out_dtype, float* stats, int32_t B, int64_t T,
                            int32_t C, int32_t kw, int32_t stride, float eps, void* workspace, uint64_t ws_bytes,
                            void* stream);
uint64_t wavlm_conv0_gn_bwd_workspace_bytes(int32_t B, int64_t T, int32_t C, int32_t stride);
int wavlm_conv0_gn_gelu_bwd(const void* wav, int32_t wav_dtype, const void* W, const void* gamma, const void* beta,
                            int32_t param_dtype, const void* g, int32_t g_dtype, const float* stats, void* dW,
                            void* dgamma, void* dbeta, int32_t B, int64_t T, int32_t C, int32_t kw, int32_t stride,
                            float gscale, void* workspace, uint64_t ws_bytes, void* stream);

/* extractor_mode = "layer_norm" (WavLM-Large), block 0: Conv1d(1 -> C, k = 10) -> LayerNorm over the C channels of each
 * frame -> GELU, channel-last (WavLM/WavLM.py:403-418 with mode "layer_norm"; Fp32LayerNorm WavLM/modules.py:31-43).
 * One fused pass forward; backward (dW, dgamma, dbeta; no input gradient) recomputes conv and statistics.  With bf16
 * operands and C = 512 both run on the matrix cores; their frame statistics come from second moments of the parameters over
 * the channels, which the forward keeps in its (small) workspace: wavlm_conv0_ln_fwd_workspace_bytes() bytes. */
uint64_t wavlm_conv0_ln_fwd_workspace_bytes(void);
int wavlm_conv0_ln_gelu_fwd(const void* wav, int32_t wav_dtype, const void* W, const void* conv_bias, const void* gamma,
                            const void* beta, int32_t param_dtype, void* out, int32_t out_dtype, int32_t B, int64_t T,
                            int32_t C, int32_t kw, int32_t stride, float eps, void* workspace, uint64_t ws_bytes,
                            void* stream);
uint64_t wavlm_conv0_ln_bwd_workspace_bytes(int32_t B, int64_t T, int32_t C, int32_t stride);
/* conv_bias / dconv_bias: the Conv1d bias of conv_bias=True configurations and its gradient (both optional, [C]) */
int wavlm_conv0_ln_gelu_bwd(const void* wav, int32_t wav_dtype, const void* W, const void* conv_bias, const void* gamma,
                            const void* beta, int32_t param_dtype, const void* g, int32_t g_dtype, void* dW,
                            void* dconv_bias, void* dgamma, void* dbeta, int32_t B, int64_t T, int32_t C, int32_t kw,
                            int32_t stride, float eps, float gscale, void* workspace, uint64_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Gated relative-position-bias attention (WavLM/modules.py:417-455, 504-563).
 * ------------------------------------------------------------------------------------------ */
/* rel[h][d] = emb[bucket[d]][h], d = (j - i) + T - 1 in [0, 2T-2]; bucket[] is the host-computed int table */
int wavlm_relpos_gather(const void* emb, int32_t emb_dtype, const int32_t* bucket, float* tab, int32_t H, int32_t L,
                        void* stream);
int wavlm_relpos_scatter(const float* dtab, const int32_t* bucket, void* demb, int32_t emb_dtype, int32_t H, int32_t L,
                         int32_t num_buckets, void* stream);
/* gate[b,h,t] = ga*(gb*grep_a[h] - 1) + 2 from the un-projected layer input x[B,T,H*hd] (modules.py:523-533) */
int wavlm_gate_fwd(const void* x, const void* W, const void* bias, const void* grep_a, float* gate, float* ga, float* gb,
                   int32_t B, int32_t T, int32_t H, int32_t hd, int32_t dtype, int32_t param_dtype, void* stream);
uint64_t wavlm_gate_bwd_workspace_bytes(int32_t H, int32_t hd);
int wavlm_gate_bwd(const float* dgate, const void* x, const void* W, const void* grep_a, const float* ga,
                   const float* gb, void* dx, void* dW, void* dbias, void* dgrep_a, int32_t B, int32_t T, int32_t H,
                   int32_t hd, int32_t dtype, int32_t param_dtype, int32_t accumulate_params, void* workspace,
                   uint64_t ws_bytes, void* stream);  /* accumulate_params bit 0: dW / dbias / dgrep_a (+)= (gradient sinks);
                                           bit 1: dx (+)= (dx already holds the gradient another consumer of x produced) */
/* P = dropout(softmax_j(S + gate_i*rel[h, j-i] + keypad)); lse saved.  S: [B*H, T, ldS], P: [B*H, T, ldP]; T <= 1024 */
int wavlm_attn_softmax_fwd(const void* S, void* P, float* lse, const float* gate, const float* tab, const uint8_t* kpm,
                           int32_t B, int32_t H, int32_t T, int64_t ldS, int64_t ldP, int32_t s_dtype, int32_t p_dtype,
                           float p_drop, uint64_t seed, void* stream);
uint64_t wavlm_attn_softmax_bwd_workspace_bytes(int32_t B, int32_t H, int32_t T);
int wavlm_attn_softmax_bwd(const void* S, const void* dP, const float* lse, const float* gate, const float* tab,
                           const uint8_t* kpm, void* dS, float* dgate, float* dtab, int32_t dtab_accumulate, int32_t B,
                           int32_t H, int32_t T, int64_t ldS, int64_t ldP, int32_t s_dtype, int32_t p_dtype,
                           float p_drop, uint64_t seed, void* workspace, uint64_t ws_bytes, void* stream);

/* Fused attention (bf16, head_dim 64): scores, Toeplitz bias, key padding, online softmax, dropout and PV in one
 * kernel; nothing of size [B*H, T, T] is written.  qkv: packed [B, T, 3*H*64]; O: [B, T, H*64]; lse: [B*H, T].
 * Replaces F.multi_head_attention_forward + the materialised gated bias (WavLM/modules.py:504-563). */
int wavlm_attn_fused_fwd(const void* qkv, void* O, float* lse, const float* gate, const float* tab, const uint8_t* kpm,
                         int32_t B, int32_t H, int32_t T, int32_t head_dim, float scale, float p_drop, uint64_t seed,
                         void* stream);
uint64_t wavlm_attn_fused_bwd_workspace_bytes(int32_t B, int32_t H, int32_t T);
/* dqkv [B, T, 3*H*64], dgate [B, H, T], dtab [H, 2T-1] from dO and the forward's (qkv, O, lse).
 * dbias (optional, [3*H*64], dbias_dtype, (+)= if dbias_accumulate): column sums of dqkv over all B*T rows, i.e. the bias
 * gradient of the packed q|k|v projection (WavLM/modules.py:504-520 in_proj_bias) -- it falls out of the kernels that produce
 * dq / dk / dv (per-block column sums + one finishing launch) instead of a separate pass over dqkv. */
int wavlm_attn_fused_bwd(const void* qkv, const void* O, const void* dO, const float* lse, const float* gate,
                         const float* tab, const uint8_t* kpm, void* dqkv, float* dgate, float* dtab, void* dbias,
                         int32_t dbias_dtype, int32_t dbias_accumulate, int32_t B, int32_t H, int32_t T, int32_t head_dim,
                         float scale, float p_drop, uint64_t seed, void* workspace, uint64_t ws_bytes, void* stream);
/* The same pair with STORED PROBABILITIES (round 5): the forward additionally writes its softmax probabilities -- fp16,
 * relative to the running row maximum of their key tile, dropout decision in the sign bit -- and those maxima into the opaque
 * `pstore` (wavlm_attn_fused_pstore_bytes: 4 KiB per 32 query rows x 64 keys, 453 MB per layer at B = 32, H = 12, T = 749),
 * and the backward kernels read them instead of recomputing scores, bias, exponentials and dropout words from (q, k, lse,
 * seed): the element pass of both backward kernels shrinks to convert / scale / multiply and each loses its score MFMA.
 * The reference keeps the same tensor (`attn_output_weights` after dropout, F.multi_head_attention_forward under
 * WavLM/modules.py:504-563, fp32 / fp16 [B*H, T, T]) -- here it is a memory-for-VALU trade the 288 GB part can afford.
 * wavlm_attn_fused_pstore_bytes returns 0 for T > 1024: recompute only.
 * pstore == NULL: exactly wavlm_attn_fused_fwd / _bwd (recompute; the low-memory mode).  A backward with pstore must be
 * given the pstore its own forward wrote (same B, H, T, gate, tab, kpm, p_drop, seed).
 * BIT mode (ABI 21, round 6; opt-in, measured neutral): a pstore of exactly wavlm_attn_fused_dbits_bytes (one bit per (row, key) of
 * the padded grid: 27 MB per layer at B = 32, H = 12, T = 749; 256-byte aligned) makes the forward store only its dropout
 * DECISIONS -- it evaluates the hash anyway -- and both backward kernels select with the stored bits (two instructions per
 * element) instead of evaluating the hash twice more; scores, bias and exponentials are recomputed as without a pstore.  The
 * reference keeps the dropout mask inside F.dropout's autograd node (WavLM/modules.py:504-563 under
 * F.multi_head_attention_forward, one byte per element). */
uint64_t wavlm_attn_fused_pstore_bytes(int32_t B, int32_t H, int32_t T);
uint64_t wavlm_attn_fused_dbits_bytes(int32_t B, int32_t H, int32_t T);
int wavlm_attn_fused_fwd_p(const void* qkv, void* O, float* lse, const float* gate, const float* tab, const uint8_t* kpm,
                           void* pstore, uint64_t pstore_bytes, int32_t B, int32_t H, int32_t T, int32_t head_dim, float scale,
                           float p_drop, uint64_t seed, void* stream);
int wavlm_attn_fused_bwd_p(const void* qkv, const void* O, const void* dO, const float* lse, const float* gate,
                           const float* tab, const uint8_t* kpm, const void* pstore, uint64_t pstore_bytes, void* dqkv,
                           float* dgate, float* dtab, void* dbias, int32_t dbias_dtype, int32_t dbias_accumulate, int32_t B,
                           int32_t H, int32_t T, int32_t head_dim, float scale, float p_drop, uint64_t seed, void* workspace,
                           uint64_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * pos_conv weight side: weight_norm(dim=2) -> GEMM weight images, and its backward (WavLM/WavLM.py:514-527)
 * ------------------------------------------------------------------------------------------ */
uint64_t wavlm_posconv_weight_workspace_bytes(int32_t D, int32_t Cg, int32_t K);
/* w[co, ci, k] = g[k] * v[co, ci, k] / ||v[:, :, k]|| as the two operand images of the convolution (Wf: forward; Wb:
 * gradient of x, taps flipped, channels / columns swapped), G * Cg * K * Cg elements each.  layout 0: [g][column][tap][channel]
 * (B operand of the overlapping-row GEMM form); layout 1 (K % 16 == 0, Cg % 8 == 0): the image wavlm_posconv_direct
 * streams, [g][channel / 8][(tap % 16) / 4][tap / 16][tap % 4][column][channel % 8]. */
int wavlm_posconv_weight_fwd(const void* v, const void* g, int32_t param_dtype, void* Wf, void* Wb, int32_t out_dtype,
                             float* norm, int32_t D, int32_t Cg, int32_t K, int32_t layout, void* workspace,
                             uint64_t ws_bytes, void* stream);
/* dWf: fp32 gradient of the layout-0 forward image, as `nsplit` slabs of G*Cg*K*Cg elements that are summed first
 * (1 slab from the GEMM form, wavlm_posconv_dw_direct_splits() from the direct kernel) -> dv, dg in param dtype */
int wavlm_posconv_weight_bwd(const float* dWf, const void* v, const void* g, const float* norm, int32_t param_dtype,
                             void* dv, void* dg, int32_t D, int32_t Cg, int32_t K, int32_t nsplit, void* workspace,
                             uint64_t ws_bytes, void* stream);
/* x[B,T,D] (optionally * gelu'(aux)) -> group-major, time-padded out[B,G,Tp,D/G]; nat_out optional natural copy */
int wavlm_posconv_group_major(const void* x, const void* aux, void* out, void* nat_out, int32_t B, int32_t T, int32_t D,
                              int32_t G, int32_t left_pad, int32_t Tp, int32_t dtype, int32_t aux_is_grad, void* stream);

/* The grouped convolution itself as a direct convolution (bf16; Cg = 48 or 64; K = 128): one workgroup per (batch,
 * group, frame segment) keeps its input window in LDS, the group's weights stream through it.
 *   out[b, t, g*Cg + n] = res[b, t, g*Cg + n] + f( sum_{tap, ci} xg[b, g, t + tap, ci] * w[g, n, tap, ci] + bias[g*Cg + n] )
 * xg [B, G, Tp, Cg] is wavlm_posconv_group_major's output (Tp >= T + K - 1), W one of wavlm_posconv_weight_fwd's LAYOUT-1 images.
 * gelu != 0: f = GELU and aux (optional, [B, T, G*Cg]) receives the pre-activation for the backward pass -- the
 * forward, nn.Conv1d(groups=16, k=128) + SamePad + GELU + the residual add of WavLM/WavLM.py:577-579; gelu == 0 with
 * W = Wb over the group-major dy * gelu': the gradient of x.  bias / res / aux may be NULL.
 * wavlm_posconv_direct_supported tells whether the shape is covered (otherwise: wavlm_gemm, overlapping-row form). */
int wavlm_posconv_direct_supported(int32_t Cg, int32_t K, int32_t T);
int wavlm_posconv_direct(const void* xg, const void* W, const void* bias, const void* res, void* out, void* aux,
                         int32_t B, int32_t G, int32_t T, int32_t Tp, int32_t Cg, int32_t K, int32_t gelu, void* stream);
/* The weight gradient of the same convolution, directly from the two group-major copies (bf16; Cg = 48 / 64; K = 128):
 *   part[s][g][n][tap][ci] = sum over the s-th part of the batch and all t of xg[b, g, t + tap, ci] * dug[b, g, du_off + t, n]
 * fp32, wavlm_posconv_dw_direct_splits(Cg, G) slabs (0: shape not covered) for wavlm_posconv_weight_bwd to add up.
 * Replaces the weight-gradient pass of nn.Conv1d(groups=16, k=128) in WavLM/WavLM.py:514-527's backward. */
int wavlm_posconv_dw_direct_splits(int32_t Cg, int32_t G);
int wavlm_posconv_dw_direct(const void* xg, const void* dug, float* part, int32_t B, int32_t G, int32_t T, int32_t Tp,
                            int32_t du_off, int32_t Cg, int32_t K, void* stream);

/* ------------------------------------------------------------------------------------------
 * Masked-prediction loss (src/fairseq/models/wavlm/wavlm.py:426-438; criterions/wavlm_criterion.py:52-138)
 * ------------------------------------------------------------------------------------------ */
int wavlm_l2norm_fwd(const void* x, int32_t x_dtype, void* y, int32_t y_dtype, float* inv_norm, int64_t rows,
                     int32_t D, float eps, void* stream);
int wavlm_l2norm_bwd(const void* dy, const void* y, int32_t y_dtype, const float* inv_norm, void* dx, int32_t x_dtype,
                     int64_t rows, int32_t D, void* stream);
/* per row: loss = logsumexp(logits) - logits[target]; correct = (logits[target] is the row max);
 * dlogits (optional) = weight * (softmax - onehot), zero-filled up to ld_dlogits.
 * flat_wrong (ABI 25): a row whose V logits are all equal counts as not correct -- the wav2vec criterion's
 * (argmax == 0) minus (argmax == 0 and argmin == 0), criterions/wav2vec_criterion.py:105-113, with the target in column 0. */
int wavlm_ce_rows(const float* logits, const int32_t* target, float* loss_rows, float* correct_rows, void* dlogits,
                  int32_t d_dtype, int64_t S, int32_t V, int64_t ld_logits, int64_t ld_dlogits, float weight,
                  int32_t flat_wrong, void* stream);

/* Sampled-instance cosine logits + BCE: the utterance-contrastive head of UniSpeech-SAT
 * (src/fairseq/models/unispeech_sat/unispeech_sat.py:487-557 sample_instances / compute_nce, 701-737 compute_pred_spk;
 * the same gathered-cosine shape as wav2vec 2.0's sample_negatives, models/wav2vec/wav2vec2.py:474-553).
 * X, Y: L2-normalised rows (X = Y for UniSpeech-SAT); idx[s, n]: row of Y gathered for logit n of row s (the host draws
 * the indices with the reference's torch.randint calls); out[s, n] = scale * <X[s], Y[idx[s, n]]>; mask_raw (ABI 25; NULL = no
 * masking): the rows of Y before normalisation, same shape and dtype -- logits n >= 1 whose gathered row of mask_raw equals the
 * row of column 0 become -inf (wav2vec 2.0's neg_is_pos, wav2vec2.py:535-551, which compares the un-normalised targets: a
 * positive multiple of the positive is NOT masked).  rows_wsum is both halves of its backward:
 * out[j] (+)= sum_{e in [off[j], off[j+1])} w[e] * Y[src[e]]. */
int wavlm_gather_dot(const void* X, const void* Y, int32_t dtype, const int32_t* idx, float* out, int64_t S, int32_t N,
                     int32_t D, float scale, const void* mask_raw, void* stream);
int wavlm_rows_wsum(const void* Y, int32_t dtype, const int32_t* src, const float* w, const int32_t* off, void* out,
                    int32_t out_dtype, int64_t rows, int32_t D, int32_t accumulate, void* stream);
uint64_t wavlm_bce_workspace_bytes(void);
int wavlm_bce_logits(const float* logits, const uint8_t* targets, float* dlogits, float* out, int64_t n, float gscale,
                     void* workspace, uint64_t ws_bytes, void* stream);
/* Gated linear unit over the last dimension: y[rows, F] = x[:, :F] * g(x[:, F:]) and its backward dx[rows, 2F].
 * gate: 0 sigmoid = nn.GLU (target_glu, src/fairseq/models/wavlm/wavlm.py:322-327, 529-531: Linear(F, 2F) + GLU on the label
 * embeddings) | 1 swish (GLU_Linear(.., "swish"): the feed-forward fc1 under activation_fn = "glu", WavLM/modules.py:99-129,
 * WavLM/WavLM.py:668-669, 707-708) | 2 relu | 3 gelu | 4 bilinear. */
int wavlm_glu_fwd(const void* x, void* y, int64_t rows, int32_t F, int32_t dtype, int32_t gate, void* stream);
int wavlm_glu_bwd(const void* x, const void* dy, void* dx, int64_t rows, int32_t F, int32_t dtype, int32_t gate, void* stream);
/* Elementwise feed-forward activations other than the erf GELU of the GEMM epilogues (utils.get_activation_fn,
 * src/fairseq/utils.py:533-555; WavLM/modules.py:144-160): kind 1 relu | 2 gelu_accurate (tanh form,
 * src/fairseq/modules/gelu.py:14-19) | 3 tanh | 4 erf gelu.  The backward takes the pre-activation x: dx = dy * act'(x). */
int wavlm_act_fwd(const void* x, void* y, int64_t n, int32_t dtype, int32_t kind, void* stream);
int wavlm_act_bwd(const void* x, const void* dy, void* dx, int64_t n, int32_t dtype, int32_t kind, void* stream);
uint64_t wavlm_sum_workspace_bytes(void);
int wavlm_sum_f32(const float* x, int64_t n, float* out, void* workspace, uint64_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Fused optimizer step (src/fairseq/optim/adam.py:148-228, fp16_optimizer.py:106-218, utils.py:338-388)
 * ------------------------------------------------------------------------------------------ */
/* grad is scaled by grad_mult (* grad_mult_dev[0] when given: a device scalar such as 1 / global sample size) and
 * clipped to max_norm using the device scalar *gnorm_sq (sum of squares of the unscaled gradient) -- no host sync. */
int wavlm_adam_step(float* p, float* m, float* v, const void* grad, int32_t grad_dtype, void* p_lowp,
                    int32_t lowp_dtype, int64_t n, float lr, float beta1, float beta2, float eps, float weight_decay,
                    int64_t step, float grad_mult, const float* grad_mult_dev, const float* gnorm_sq, float max_norm,
                    void* stream);

/* ------------------------------------------------------------------------------------------
 * Utterance / noise mixing of a collated batch (replaces the per-sample numpy loop of
 * src/fairseq/data/audio/utterance_mixing_dataset.py:373-438 mixing_collated_audios; all random draws stay on the host).
 * dst[B, T] (fp32, != src) = src with `ops` applied in the reference's in-place row order; ops: n_ops x 8 int32
 * (row, kind 0 = batch row / 1 = noise segment, src row | noise offset, c_start, s_start, c_len, src length, float32
 * bits of 10^(snr/10)), sorted by row; op_begin[B + 1].  scale = sqrt(mean(dst_row^2) / (mean(src^2) * gain)), 0 if the
 * source power is 0.  normalize: rows that were mixed get (x - mean) / sqrt(var + eps) over the whole row (F.layer_norm).
 * dst_lowp (optional): bf16 copy of the result (the Trainer's waveform cast, trainer.py:1141-1152).
 * ------------------------------------------------------------------------------------------ */
uint64_t wavlm_mix_workspace_bytes(int32_t B, int64_t T);
int wavlm_mix_utterances(const float* src, float* dst, void* dst_lowp, int32_t B, int64_t T, const int32_t* ops,
                         int32_t n_ops, const int32_t* op_begin, const float* noise, int32_t normalize, float eps,
                         void* workspace, uint64_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Gumbel-softmax vector quantiser on projected logits [n, G*V] (replaces the per-row part of
 * src/fairseq/modules/gumbel_vector_quantizer.py:157-213; the weight projection is a wavlm_gemm, the codebook product a
 * wavlm_gather_rows with the returned indices).
 *   fwd: idx[n*G] = g*V + argmax (training: of (logits + gumbel)/tau, else of the raw logits); ysoft[n*G, V] =
 *        softmax((logits + gumbel)/tau) (training only); noise = the Gumbel draws [n*G, V] (fp32) or NULL for a device
 *        counter hash of `seed`; part[wavlm_gumbel_vq_partial_rows(n)][ld_part >= 2*G*V] = per-wave column sums of softmax(raw
 *        logits) and of the hard one-hot (sum the rows with wavlm_colsum; ld_part, ABI 25, lets the caller round the row up
 *        to wavlm_colsum's 8-column granule when G*V is not a multiple of 4 -- columns beyond 2*G*V are not written).
 *   perplexity: sums[2][G*V] -> out[0] = prob_perplexity, out[1] = code_perplexity, dA[G*V] = d prob_ppl / d avg_probs.
 *   bwd: dlogits = ysoft*(dret - <ysoft,dret>)/tau (if ysoft/dret given) + dppl[0] * softmax(raw)*(dA - <softmax,dA>)/n
 *        (if dppl given).  G <= 4, V <= 320.
 * ------------------------------------------------------------------------------------------ */
uint64_t wavlm_gumbel_vq_partial_rows(int64_t n);
int wavlm_gumbel_vq_fwd(const void* logits, int32_t dtype, const float* noise, uint64_t seed, float tau, int32_t training,
                        int64_t n, int32_t G, int32_t V, float* ysoft, int32_t* idx, float* part, int64_t ld_part,
                        void* stream);
int wavlm_vq_perplexity(const float* sums, int64_t n, int32_t G, int32_t V, float* out, float* dA, void* stream);
int wavlm_gumbel_vq_bwd(const void* logits, int32_t dtype, const float* ysoft, const float* dret, const float* dA,
                        const float* dppl, float tau, int64_t n, int32_t G, int32_t V, void* dlogits, void* stream);

/* ------------------------------------------------------------------------------------------
 * One transformer encoder block per call (WavLM/WavLM.py:615-742 TransformerSentenceEncoderLayer.forward + the
 * MultiheadAttention it owns, WavLM/modules.py:417-563; fairseq twin models/unispeech_sat/unispeech_sat.py:1040-1139).
 * The kernel sequence of a block is fixed, so the host issues it from C: one call (and one autograd node) per block and
 * direction instead of ~35 -- the reference's training loop calls the model once per micro-batch (trainer.py:697-760)
 * and the launch thread must stay ahead of a 35 ms step.
 *   forward, post-LN (pre_ln = 0):  a = out_proj(attn(x)); x1 = LN1(x + drop(a)); f = fc2(gelu(fc1 x1)); y = LN2(x1 + drop(f))
 *   forward, pre-LN (pre_ln = 1), residual adds fused into the LayerNorms: s1 = x + drop(r_in) (r_in = the previous
 *     block's feed-forward output, NULL for the first block: s1 = x); h1 = LN1(s1); a = out_proj(attn(h1));
 *     y = s1 + drop(a); h2 = LN2(y); r_out = fc2(gelu(fc1 h2))  -- the caller adds r_out in the next block / final LN.
 * attn = gate (gru_rel_pos, optional) -> packed q|k|v projection -> wavlm_attn_fused_fwd.  bf16, head_dim 64 only.
 * `saved` holds what backward needs (wavlm_layer_saved_bytes; forward with saved == NULL = inference: nothing kept, the
 * workspace must then hold wavlm_layer_fwd_workspace_bytes, which includes that region).  Backward accumulates EVERY
 * parameter gradient into the given gradient pointers ((+)=, the flat gradient arena of the optimizer), returns the input
 * gradient(s) and (+)= or = the gradient of the relative-position table.
 * All parameters share param_dtype; activations are bf16.  Dropout seeds: one per mask, regenerated in backward.
 * ------------------------------------------------------------------------------------------ */
typedef struct wavlm_layer_desc {
  int32_t B, T, D, H, F;           /* batch, frames, model width, heads (D / H == 64), feed-forward width */
  int32_t pre_ln;                  /* 0 post-LN (Base), 1 pre-LN with fused residual adds (Large) */
  int32_t param_dtype;             /* 0 f32 | 1 bf16 */
  int32_t dtab_accumulate;         /* backward: dtab (+)= instead of = */
  float eps1, eps2, scale;         /* LayerNorm epsilons, q scaling (head_dim^-0.5) */
  float p_drop, p_attn;            /* residual dropout, attention dropout (0 in eval) */
  int32_t attn_store_p;            /* 2: the attention keeps its dropout decisions (bit words) in `saved` for backward;
                                      1: its probabilities (wavlm_attn_fused_fwd_p); 0: backward recomputes everything
                                      (the default).  Same value in forward and backward. */
  uint64_t seed_r1, seed_r2, seed_attn;
  /* parameters (and, backward only, their gradient accumulators) */
  const void *Wqkv, *bqkv, *Wo, *bo, *W1, *b1, *W2, *b2, *ln1_g, *ln1_b, *ln2_g, *ln2_b;
  const void *Wgate, *bgate, *grep_a;           /* grep_linear [8, 64], [8]; grep_a [H]; all NULL: gate == 1 */
  void *dWqkv, *dbqkv, *dWo, *dbo, *dW1, *db1, *dW2, *db2, *dln1_g, *dln1_b, *dln2_g, *dln2_b, *dWgate, *dbgate, *dgrep_a;
  void* db2_prev;                  /* pre-LN backward: gradient of the bias of the linear that produced r_in (or NULL) */
  const float* tab;                /* [H, 2T-1] Toeplitz generator of the position bias, or NULL */
  const uint8_t* kpm;              /* [B, T] key padding (1 = padded) or NULL */
  /* activations */
  const void* x;                   /* [B, T, D] block input (pre-LN: the residual stream) */
  const void* r_in;                /* pre-LN: [B, T, D] pending feed-forward output of the previous block, or NULL */
  void* y;                         /* [B, T, D] block output (pre-LN: the residual stream after the attention branch) */
  void* r_out;                     /* pre-LN: [B, T, D] this block's feed-forward output */
  void* saved; uint64_t saved_bytes;
  void* workspace; uint64_t ws_bytes;
  /* backward */
  const void* dy;                  /* gradient of y */
  const void* dr_out;              /* pre-LN: gradient of r_out */
  void* dx;                        /* gradient of x */
  void* dr_in;                     /* pre-LN: gradient of r_in (if r_in != NULL) */
  float* dtab;                     /* [H, 2T-1] (if tab != NULL) */
} wavlm_layer_desc;
uint64_t wavlm_layer_saved_bytes(const wavlm_layer_desc* d);
uint64_t wavlm_layer_fwd_workspace_bytes(const wavlm_layer_desc* d);   /* for saved == NULL add wavlm_layer_saved_bytes */
uint64_t wavlm_layer_bwd_workspace_bytes(const wavlm_layer_desc* d);
int wavlm_encoder_layer_fwd(const wavlm_layer_desc* d, void* stream);
int wavlm_encoder_layer_bwd(const wavlm_layer_desc* d, void* stream);

/* ------------------------------------------------------------------------------------------
 * Data-parallel seam below Python.  The reference reduces gradients AFTER the whole backward, from one flat buffer
 * (src/fairseq/distributed/legacy_distributed_data_parallel.py:76-165); here backward kernels accumulate straight into
 * the caller's flat gradient arena, and a reducer that wants to start a bucket's all-reduce while backward is still running
 * has to learn which slice has just been written.  Every entry point that ACCUMULATES into a caller-designated parameter
 * gradient -- wavlm_gemm / wavlm_gemm_grouped with `accumulate` or an accumulating `colsum`, wavlm_layernorm_bwd with
 * accumulate_params (dgamma, dbeta, dr_colsum), wavlm_colsum with accumulate, wavlm_gate_bwd (bit 0), wavlm_attn_fused_bwd
 * (dbias), wavlm_conv_wgrad_scatter with accumulate, and through them wavlm_encoder_layer_bwd -- calls the listener with
 * (base, bytes, stream, user) right after it has ENQUEUED the kernels: the slice is complete in `stream` order (record an
 * event on `stream`, make the communication stream wait for it).  One call per accumulation: a parameter used twice in
 * one forward is reported twice.  The callback runs on the launch thread and must not block.  cb == NULL: none.
 * ------------------------------------------------------------------------------------------ */
typedef void (*wavlm_grad_listener)(const void* base, uint64_t bytes, void* stream, void* user);
void wavlm_dp_set_listener(wavlm_grad_listener cb, void* user);

/* The transport half (ABI v20, csrc/dp_rccl.hip): one RCCL communicator per process (one process per GPU), the reference's
 * all-reduce of the flat gradient buffer (src/fairseq/distributed/legacy_distributed_data_parallel.py:82-120,
 * src/fairseq/distributed/utils.py:273-288) bucket by bucket, overlapped with backward:
 *   wavlm_dp_unique_id(id128)             rank 0: a fresh ncclUniqueId (128 bytes) for the caller to hand to the other ranks
 *                                         (over whatever it bootstraps with: MPI, a TCP store, torch.distributed)
 *   wavlm_dp_init(rank, world, id128, average)   ncclCommInitRank on the CURRENT device + a high-priority communication
 *                                         stream; average != 0: ncclAvg (the reference divides by the world size), else ncclSum
 *   wavlm_dp_bucket_ready(base, count, dtype, compute_stream)   the `count` elements at `base` (WL_F32 / WL_BF16) are
 *                                         complete in compute_stream order: all-reduced in place on the communication stream
 *                                         behind an event on compute_stream.  Every rank reports the same buckets in the same
 *                                         order (RCCL matches collectives by issue order).  Call it from the gradient listener.
 *   wavlm_dp_finish(compute_stream)       compute_stream waits for every bucket reported since the last finish (before the
 *                                         optimizer reads the gradients); no host synchronisation
 *   wavlm_dp_destroy()
 * RCCL is resolved at the first of these calls (the copy the process already carries, else librccl.so): libwavlm_hip.so has no
 * link-time dependency on it.  WL_ELAUNCH (-2): RCCL missing or a HIP / RCCL call failed; WL_EINVAL (-1): bad argument, not
 * initialised, initialised twice. */
int wavlm_dp_unique_id(void* id128);
int wavlm_dp_init(int32_t rank, int32_t world, const void* id128, int32_t average);
int wavlm_dp_bucket_ready(void* base, uint64_t count, int32_t dtype, void* compute_stream);
int wavlm_dp_finish(void* compute_stream);
int wavlm_dp_destroy(void);

/* ------------------------------------------------------------------------------------------
 * k-means (ABI 22, csrc/kmeans.hip): HuBERT / WavLM pre-training targets on the device.  Replaces the CPU work of
 * src/examples/hubert/simple_kmeans/dump_km_label.py:25-47 (ApplyKmeans: argmin(|x|^2 - 2 x.C + |c|^2)) and
 * learn_kmeans.py:24-47 (sklearn MiniBatchKMeans: the assignment and centre-update steps; the loop is host code,
 * unispeech_amd/kmeans.py).
 *   wavlm_kmeans_centres_bytes(K, D)      bytes of the prepared centre image: fp32 [Kp, Dp] (K rounded up to 64, D to 32,
 *                                         zero padded) followed by Cnorm fp32 [Kp]
 *   wavlm_kmeans_prepare(C, K, D, ...)    fp32 centres C [K, D] -> image; Cnorm_j = one fmaf chain over d in order.  Once
 *                                         per set of centres.
 *   wavlm_kmeans_assign                   X [N, D] (x_dtype WL_F32 / WL_BF16, row stride ldx >= D) against the image:
 *                                         labels int32 [N] = argmin_j (Cnorm_j - 2 x.c_j) through fp32 MFMA (exact fmaf
 *                                         chains); ties go to the LOWEST index (numpy / torch argmin).  min_dist (fp32 [N],
 *                                         optional) = |x - c_label|^2 summed as squared differences.  No distance matrix is
 *                                         written.  Any N, K, D >= 1.
 *   wavlm_kmeans_accumulate               sums fp32 [K, D] and counts int32 [K] of the rows per label (labels outside
 *                                         [0, K) are ignored): stable inverted index + bounded chunks summed in row order,
 *                                         then chunk partials in chunk order -- bitwise reproducible, no float atomics.
 *                                         workspace >= wavlm_kmeans_accumulate_workspace_bytes(N, K, D); N < 2^31.
 *   wavlm_kmeans_update                   mode 0 (Lloyd): c_j = sums_j / n_j; mode 1 (mini-batch, sklearn
 *                                         _minibatch_update_dense): c_j = (c_j w_j + sums_j) * (1 / (w_j + n_j)),
 *                                         w_j += n_j.  Clusters with n_j == 0 keep their centre (and weight) in both modes.
 * ------------------------------------------------------------------------------------------ */
uint64_t wavlm_kmeans_centres_bytes(int32_t K, int32_t D);
int wavlm_kmeans_prepare(const float* C, int32_t K, int32_t D, void* image, uint64_t image_bytes, void* stream);
int wavlm_kmeans_assign(const void* X, int32_t x_dtype, int64_t N, int32_t D, int64_t ldx, const void* image, int32_t K,
                        int32_t* labels, float* min_dist, void* stream);
uint64_t wavlm_kmeans_accumulate_workspace_bytes(int64_t N, int32_t K, int32_t D);
int wavlm_kmeans_accumulate(const void* X, int32_t x_dtype, int64_t N, int32_t D, int64_t ldx, const int32_t* labels,
                            int32_t K, float* sums, int32_t* counts, void* workspace, uint64_t ws_bytes, void* stream);
int wavlm_kmeans_update(float* C, float* weights, const float* sums, const int32_t* counts, int32_t K, int32_t D,
                        int32_t mode, void* stream);

/* ------------------------------------------------------------------------------------------
 * speaker head (ABI 23, csrc/spkhead.hip): the inference path of the reference's ECAPA-TDNN over upstream layer states,
 * downstreams/speaker_verification/models/ecapa_tdnn.py.  Its k = 5 and 1x1 convolutions and its Linear are wavlm_gemm calls
 * (overlapping rows over a time-padded channel-last tensor for k = 5); these entry points are everything in between.
 * All tensors channel-last [B, T, C] with a batch stride and a row stride (in elements), WL_F32 or WL_BF16; arithmetic,
 * statistics and softmax in fp32.  `lengths` (int32 [B], device, optional): frames t >= lengths[b] do not exist for
 * utterance b -- they are written as zeros and left out of every mean / norm / pooling; NULL = all T frames.
 * Nothing is reduced across workgroups: results are bitwise reproducible.
 *   wavlm_spk_mix_norm     ecapa_tdnn.py:261-270 (torch.stack of the states, softmax-weighted sum, transpose, + 1e-6,
 *                          InstanceNorm1d): out[b, t, :] = ((sum_l weights[l] * state_l[b, t, :] + add) - mean) * rstd, mean
 *                          and biased variance per (b, channel) over the valid frames.  `states`, `stride_b`, `stride_t`
 *                          are HOST arrays of n_states <= 32 device pointers / element strides (unit channel stride; the
 *                          tensors are read where extract_features left them); `weights` fp32 [n_states] on the device (the
 *                          softmax already applied).  Every state is read once for T <= 1024 (the mixed slab stays in LDS);
 *                          later frames are mixed three times.  n_states == 1 (ABI 29: the log-mel features of csrc/fbank.hip,
 *                          fp32 in, the head's dtype out): sums are taken about the column's first frame, so a constant
 *                          column normalises to exactly 0; several states are summed as before, bit for bit.  Rows [-pad, 0) and [T, T + pad) of every utterance of `out`
 *                          are written as zeros (the k = 5 convolution's padding): `out` points at row 0.
 *   wavlm_spk_rowact       ecapa_tdnn.py:63-64 / :282 / :154: y = act(x) * scale[c] + shift[c], act 0 = ReLU, 1 = tanh,
 *                          2 = none; scale / shift fp32 [C] (BatchNorm folded: w / sqrt(var + eps), b - mean * scale) or
 *                          NULL.  mean_out (fp32 [B, C], optional) receives the time mean of y over the valid frames
 *                          (SE_Connect's x.mean(dim=2), :78) from the same pass.  x == y is allowed.
 *   wavlm_spk_res2         ecapa_tdnn.py:34-50 (Res2Conv1dReluBn, scale 8, width 64: C must be 512), one launch: y[:, :, 64 i
 *                          : 64 i + 64] = BN_i(relu(conv_i(sp_i))), sp_0 = x_0, sp_i = y_{i-1} + x_i, kernel 3, `dilation`
 *                          (1..4) with zero padding; the eighth split is copied.  w_image fp32 [7][3 taps][64 in][64 out],
 *                          bias / scale / shift fp32 [7][64].  Each workgroup recomputes a halo of 7 * dilation frames per
 *                          side.  bf16 x: the steps run on bf16 MFMA (the running tensor rounded to bf16 as the operand
 *                          only; accumulation, running add and affine in fp32); fp32 x: fp32 FMA throughout.  x != y.
 *   wavlm_spk_se_residual  ecapa_tdnn.py:77-83,125: out = x * sigmoid(W2 relu(W1 mean + b1) + b2) + res; W1 [Cb, C], W2
 *                          [C, Cb] and the biases in w_dtype; workspace >= wavlm_spk_se_workspace_bytes(B, C).
 *   wavlm_spk_asp          ecapa_tdnn.py:156-160,283: alpha = softmax over time of `logits` per channel; mean = sum alpha x,
 *                          std = sqrt(max(sum alpha x^2 - mean^2, 1e-9)); one pass, alpha is never written.  pooled_raw
 *                          (fp32 [B, 2 C], optional) = [mean | std]; out (optional) = the same times scale + shift (fp32
 *                          [2 C], the BatchNorm that follows; NULL = identity).
 * ------------------------------------------------------------------------------------------ */
int wavlm_spk_mix_norm(const void* const* states, const int64_t* stride_b, const int64_t* stride_t, int32_t n_states,
                       int32_t dtype, const float* weights, const int32_t* lengths, int32_t B, int32_t T, int32_t D,
                       void* out, int32_t out_dtype, int64_t out_stride_b, int64_t out_stride_t, int32_t pad, float add,
                       float eps, void* stream);
int wavlm_spk_rowact(const void* x, int32_t x_dtype, int64_t x_stride_b, int64_t ldx, void* y, int32_t y_dtype,
                     int64_t y_stride_b, int64_t ldy, int32_t B, int32_t T, int32_t C, int32_t act, const float* scale,
                     const float* shift, const int32_t* lengths, float* mean_out, void* stream);
int wavlm_spk_res2(const void* x, int32_t x_dtype, int64_t x_stride_b, int64_t ldx, void* y, int32_t y_dtype,
                   int64_t y_stride_b, int64_t ldy, int32_t B, int32_t T, int32_t C, int32_t dilation, const float* w_image,
                   const float* bias, const float* scale, const float* shift, const int32_t* lengths, void* stream);
uint64_t wavlm_spk_se_workspace_bytes(int32_t B, int32_t C);
int wavlm_spk_se_residual(const void* x, int32_t x_dtype, int64_t x_stride_b, int64_t ldx, const float* mean, const void* w1,
                          const void* b1, const void* w2, const void* b2, int32_t w_dtype, const void* res, int32_t res_dtype,
                          int64_t res_stride_b, int64_t ld_res, void* out, int32_t out_dtype, int64_t out_stride_b,
                          int64_t ld_out, int32_t B, int32_t T, int32_t C, int32_t Cb, const int32_t* lengths,
                          void* workspace, uint64_t ws_bytes, void* stream);
int wavlm_spk_asp(const void* x, int32_t x_dtype, int64_t x_stride_b, int64_t ldx, const void* logits, int32_t l_dtype,
                  int64_t l_stride_b, int64_t ldl, int32_t B, int32_t T, int32_t C, const int32_t* lengths, const float* scale,
                  const float* shift, float* pooled_raw, void* out, int32_t out_dtype, void* stream);

/* ------------------------------------------------------------------------------------------
 * diarization head (ABI 24, csrc/diar.hip): the inference path of the reference's EEND-vector-clustering model over upstream
 * layer states, downstreams/speaker_diarization/models/models.py and models/transformer.py.  Its Linear layers are wavlm_gemm
 * calls and its LayerNorms wavlm_layernorm_fwd calls (the residual operand carries `e + att(e)` / `e + ff(e)`); these entry
 * points are the three steps in between.  Tensors WL_F32 or WL_BF16; arithmetic, statistics and softmax in fp32.  Nothing is
 * reduced across workgroups: results are bitwise reproducible and no chunk depends on the batch it is in.
 *   wavlm_diar_front      models.py:210-225 with context_size 0.  mixed[b, t, c] = sum_l weights[l] * state_l[b, t, c] + add;
 *                         mean and biased variance per (b, c) over the T frames, `eps`, no affine; every `subsampling`-th
 *                         frame (T_in = ceil(T / subsampling)); then F.interpolate(mode="linear", align_corners=False) to T_out
 *                         frames: src = max(T_in / T_out * (j + 0.5) - 0.5, 0) in fp32, i0 = floor(src), i1 = min(i0 + 1,
 *                         T_in - 1), out = (1 - f) x[i0] + f x[i1].  out[b, j, c] channel-last with a batch and a row stride
 *                         (elements).  `states`, `stride_b`, `stride_t` are HOST arrays of n_states <= 32 device pointers /
 *                         element strides (unit channel stride), `weights` fp32 [n_states] on the device (softmax applied).
 *                         Every state element is read once for T <= 1536 (the mixed slab of 16 channels stays in LDS, 96 KiB);
 *                         a later frame is mixed again once for the variance and once per interpolation tap that uses it (up
 *                         to four reads of those frames when T_out <= T_in).
 *   wavlm_attn_plain_fwd  transformer.py:55-69: O[b, t, h * d + :] = softmax_j(scale * q[b, t, h] . k[b, j, h]) v[b, j, h] from
 *                         the packed qkv [B, T, 3 * H * d] (q | k | v, head h at h * d inside each), O [B, T, H * d], both of
 *                         `dtype`, 16-byte aligned.  head_dim must be 32; any T; online softmax, no [B H, T, T] tensor.  bf16:
 *                         both products on v_mfma_f32_32x32x16_bf16 with fp32 softmax state (P rounded to bf16 as the operand
 *                         only); fp32: fp32 FMA throughout.  No bias, mask or dropout: the reference has none in eval.
 *   wavlm_diar_estimate   models.py:232-250,325-344.  z [B, T, ldz] holds, per frame, S activity logits then S vectors of E
 *                         (the output of one GEMM over `linear` | `linear0` .. concatenated; ldz >= S + S * E, E <= 512).
 *                         activities fp32 [B, T, S] = sigmoid(logits); vectors [B, S, E] (v_dtype) = normalize(sum_t
 *                         activities[b, t, s] * z[b, t, s, :] / |z[b, t, s, :]|): per-frame normalisation, weight, sum over
 *                         time (inside one workgroup, fixed order), final normalisation -- estimate()'s order.
 * ------------------------------------------------------------------------------------------ */
int wavlm_diar_front(const void* const* states, const int64_t* stride_b, const int64_t* stride_t, int32_t n_states,
                     int32_t dtype, const float* weights, int32_t B, int32_t T, int32_t D, int32_t subsampling, int32_t T_out,
                     void* out, int32_t out_dtype, int64_t out_stride_b, int64_t out_stride_t, float add, float eps,
                     void* stream);
int wavlm_attn_plain_fwd(const void* qkv, void* O, int32_t B, int32_t H, int32_t T, int32_t head_dim, int32_t dtype,
                         float scale, void* stream);
int wavlm_diar_estimate(const void* z, int32_t z_dtype, int64_t z_stride_b, int64_t ldz, int32_t B, int32_t T, int32_t S,
                        int32_t E, float* activities, void* vectors, int32_t v_dtype, void* stream);

/* ------------------------------------------------------------------------------------------
 * sinc resampler (ABI 27, csrc/resample.hip): torchaudio.functional.resample with sinc_interpolation, the step in front of the
 * upstream in downstreams/speaker_diarization/models/models.py:138,207 (`torchaudio.transforms.Resample(sr, 16000)` per chunk
 * batch) and downstreams/speaker_verification/verification.py:46-49.  o = orig / gcd(orig, new), n = new / gcd, `width` the
 * filter half-width in input samples (ceil(lowpass_filter_width * o / (min(o, n) * rolloff))).
 *   y[b, f * n + i] = sum_{j < 2 width + 1} table[i][j] * x[b, f * o + first[i] + j - width],   x = 0 outside [0, len_b)
 * for f * n + i < ceil(n * len_b / o); the rest of the row up to L_out = ceil(n * L / o) is written as zero.  len_b =
 * lengths[b] clamped to [0, L] (int32 on the device), or L when lengths is NULL.
 *   table  fp32 [n][2 width + 1] on the device: per phase, the taps of the dense 2 width + o filter that lie inside the window
 *          (|t| < lowpass_filter_width), zero-filled; first int32 [n]: the dense index of table[i][0], at most o - 1.
 *   x      [B, L] WL_F32, or WL_I16 = 2: int16 PCM, input only (scaled by 1 / 32768 in the kernel); y [B, L_out] WL_F32 or
 *          WL_BF16; x_stride / y_stride: row strides in elements (>= L / >= L_out).  Bytes of y outside the B x L_out view are
 *          not touched.
 * fp32 fmaf in tap order, one thread per output and no reduction across threads: bitwise reproducible, and a row's result does
 * not depend on B or on its position in the batch.  wavlm_resample_supported: 1 if the table (n * (2 width + 2) * 4 bytes <= 48
 * KiB) and a tile of at least four frames (4 o + 2 width <= 8192 samples) fit the kernel's LDS budget; wavlm_resample_rows
 * returns -1 for a ratio that is not.
 * ------------------------------------------------------------------------------------------ */
int wavlm_resample_supported(int32_t o, int32_t n, int32_t width);
int wavlm_resample_rows(const void* x, int32_t x_dtype, int64_t x_stride, int32_t B, int64_t L, const int32_t* lengths,
                        const float* table, const int32_t* first, int32_t o, int32_t n, int32_t width, void* y,
                        int32_t y_dtype, int64_t y_stride, void* stream);

/* ------------------------------------------------------------------------------------------
 * Kaldi MFCC + deltas (ABI 28, csrc/mfcc.hip): the 39-wide features of HuBERT's first k-means iteration
 * (src/examples/hubert/simple_kmeans/dump_mfcc_feature.py:46-55: torchaudio.compliance.kaldi.mfcc(use_energy=False) at its
 * defaults, compute_deltas twice, [c | d | dd]).  W = int(0.025 sr), S = int(0.010 sr), P = the next power of two >= W.
 *   x        [B, L] fp32 in [-1, 1] or int16 PCM (x_dtype WL_F32 / WL_I16; int16 is scaled by 1 / 32768 on load), row stride x_stride >= L
 *   lengths  NULL or B sample counts (clamped to [0, L]): a row ends there
 *   window [W], twiddle [P][2] = (cos, -sin)(2 pi t / P), mel_idx [23][3] = (first bin, count, offset into mel_w), mel_w
 *   [n_mel_w <= P]: filter b = sum_i mel_w[offset + i] * power[first + i] over bins < P / 2; dct [13][23] with the lifter folded
 *   in -- computed by the host in float64 and rounded to fp32 once (unispeech_amd/mfcc.py); out-of-range mel_idx entries are
 *   clamped, never followed
 *   y        fp32 [B, Mmax, ncol], ncol 39 or 13 (no deltas), row stride y_stride >= Mmax * ncol in elements; Mmax >=
 *            wavlm_mfcc_frames(L, W, S); frames at or beyond a row's own count are written as zero; deltas replicate the row's
 *            own first and last frame
 * One launch, nothing staged in HBM.  Fixed arithmetic order: a row's features are bitwise the same wherever the row sits in the
 * batch.  wavlm_mfcc_supported (host): 1 if P is a power of two in [64, 512], P / 2 < W <= P, 1 <= S <= W and the tile fits 80
 * KiB of LDS (16000 Hz: 400 / 160 / 512 and 8000 Hz: 200 / 80 / 256 do); wavlm_mfcc_rows returns -1 otherwise.
 * wavlm_mfcc_frames (host): 0 for len < W, else 1 + (len - W) / S.
 * ------------------------------------------------------------------------------------------ */
int wavlm_mfcc_supported(int32_t W, int32_t S, int32_t P);
int64_t wavlm_mfcc_frames(int64_t len, int32_t W, int32_t S);
int wavlm_mfcc_rows(const void* x, int32_t x_dtype, int64_t x_stride, int32_t B, int64_t L, const int32_t* lengths, int32_t W,
                    int32_t S, int32_t P, const float* window, const float* twiddle, const int32_t* mel_idx, const float* mel_w,
                    int32_t n_mel_w, const float* dct, float* y, int64_t y_stride, int64_t Mmax, int32_t ncol, void* stream);

/* ------------------------------------------------------------------------------------------
 * Log-mel filter bank (ABI 29, csrc/fbank.hip): the front end of the ECAPA-TDNN baseline without an upstream,
 * downstreams/speaker_verification/models/ecapa_tdnn.py:179-182, 253, 257 (feat_type='fbank'):
 * torchaudio.transforms.MelSpectrogram(sample_rate=sr, n_fft=P, win_length=W, hop_length=S, f_min=0, f_max=sr // 2, pad=0,
 * n_mels=M) at its defaults otherwise (periodic Hann, power 2, centre, reflect, one-sided, HTK scale, no norm), + 1e-6, log.
 * The speaker model's geometry is W = 400, S = 160, P = 512, M = 40 at 16 kHz.
 *   x        [B, L] fp32 in [-1, 1] or int16 PCM (x_dtype WL_F32 / WL_I16; int16 is scaled by 1 / 32768 on load), row stride x_stride >= L
 *   lengths  NULL or B sample counts (clamped to [0, L]): a row ends there and is reflected at its own end
 *   window [W], twiddle [P][2] = (cos, -sin)(2 pi t / P), mel_idx [M][3] = (first bin, count, offset into mel_w), mel_w
 *   [n_mel_w <= P]: filter m = sum_i mel_w[offset + i] * power[first + i] over bins < P / 2 -- computed by the host in float64
 *   and rounded to fp32 once (unispeech_amd/fbank.py); out-of-range mel_idx entries are clamped, never followed
 *   y        fp32 [B, Tmax, M] channel-last, row stride y_stride >= Tmax * M in elements; Tmax >= wavlm_fbank_frames(L, S, P);
 *            y[b, t, m] = log(sum_k fb[k, m] |rfft_P(frame t)|^2[k] + 1e-6); frames at or beyond a row's own count are
 *            written as zero
 * One launch, nothing staged in HBM.  Fixed arithmetic order: a row's features are bitwise the same wherever the row sits in the
 * batch.  wavlm_fbank_supported (host): 1 if P is a power of two in [64, 512], P / 2 < W <= P, 1 <= S <= W, 1 <= M <= 128 and
 * the tile fits 80 KiB of LDS; wavlm_fbank_rows returns -1 otherwise.  wavlm_fbank_frames (host): 0 for len <= P / 2 (the
 * reflection needs more samples), else 1 + len / S.
 * ------------------------------------------------------------------------------------------ */
int wavlm_fbank_supported(int32_t W, int32_t S, int32_t P, int32_t M);
int64_t wavlm_fbank_frames(int64_t len, int32_t S, int32_t P);
int wavlm_fbank_rows(const void* x, int32_t x_dtype, int64_t x_stride, int32_t B, int64_t L, const int32_t* lengths, int32_t W,
                     int32_t S, int32_t P, int32_t M, const float* window, const float* twiddle, const int32_t* mel_idx,
                     const float* mel_w, int32_t n_mel_w, float* y, int64_t y_stride, int64_t Tmax, void* stream);

/* ------------------------------------------------------------------------------------------
 * CTC loss, its gradient and the greedy decode (ABI 30, csrc/ctc.hip): the loss of ASR fine-tuning,
 * src/fairseq/criterions/ctc.py:113-147 -- F.ctc_loss(log_softmax(logits.float(), -1), targets_flat, input_lengths,
 * target_lengths, blank, reduction="none", zero_infinity) and its gradient with respect to the LOGITS (the log-softmax is
 * src/fairseq/models/hubert/hubert_asr.py:155-162 get_normalized_probs(log_probs=True) and is fused) -- and the argmax /
 * unique_consecutive / != blank of ctc.py:200-201.
 *   logits   fp32 or bf16, element (b, t, c) at b * stride_b + t * stride_t + c (strides in elements, unit class stride): a
 *            batch-first [B, T, C] tensor and the T x B x C view of one are both read in place; the view must not overlap itself
 *   targets  int32 [n_targets] flat; sample b's labels are targets[target_offsets[b] .. target_offsets[b + 1]); at most Lmax each
 *   input_lengths int32 [B] on the device, clamped to [0, T]
 *   grad_out fp32 [B]: the gradient of whatever follows with respect to each sample's loss (ones for reduction="sum")
 *   nll      fp32 [B]: the loss per sample; +inf where no alignment exists -- with zero_infinity 0, and that sample's gradient 0;
 *            NaN (and a zero gradient) where an offset or a label of the sample is out of range
 *   dlogits  dtype and strides of logits: grad_out[b] * (softmax - posterior); rows t >= input_lengths[b] are zero, and without
 *            zero_infinity the rows of a sample without an alignment are NaN, as torch's are.  Nothing outside the B x T x C
 *            view is written.
 *   workspace  wavlm_ctc_workspace_bytes(B, T, Lmax) bytes, 8-byte aligned: nll and the row log-sum-exp in float64, and
 *            alpha [B, T, 2 Lmax + 1] in fp32
 * input_length 0: the loss is 0 for an empty target and +inf otherwise.  Three launches (row log-sum-exp; alpha; beta + gradient),
 * one workgroup per sample in the last two.  The per-class sums run in a fixed order, no atomics: results are bitwise
 * reproducible, and a sample's loss and gradient do not depend on B or on where it sits in the batch.
 * wavlm_ctc_supported (host): 1 for 1 <= C <= 1024 and 0 <= Lmax <= 1023; wavlm_ctc_loss returns -1 otherwise.
 * wavlm_ctc_greedy: tokens int32 [B, T] (sample b's decode in tokens[b, 0 .. counts[b]), -1 behind it), counts int32 [B]; the
 * argmax takes the lowest class among equal maxima; any C >= 1.
 * ------------------------------------------------------------------------------------------ */
int wavlm_ctc_supported(int32_t C, int32_t Lmax);
uint64_t wavlm_ctc_workspace_bytes(int32_t B, int32_t T, int32_t Lmax);
int wavlm_ctc_loss(const void* logits, int32_t dtype, int64_t stride_b, int64_t stride_t, int32_t B, int32_t T, int32_t C,
                   const int32_t* targets, const int32_t* target_offsets, int32_t n_targets, int32_t Lmax,
                   const int32_t* input_lengths, int32_t blank, int32_t zero_infinity, const float* grad_out, float* nll,
                   void* dlogits, void* workspace, uint64_t ws_bytes, void* stream);
int wavlm_ctc_greedy(const void* logits, int32_t dtype, int64_t stride_b, int64_t stride_t, int32_t B, int32_t T, int32_t C,
                     const int32_t* input_lengths, int32_t blank, int32_t* tokens, int32_t* counts, void* stream);

/* ------------------------------------------------------------------------------------------
 * CTC validation scoring (csrc/ctc_score.hip; additive to ABI 30: three new symbols, nothing else changes): the greedy decode of
 * wavlm_ctc_greedy and, in the same launch, the error counts of src/fairseq/criterions/ctc.py:161-226 -- unit and word edit
 * distances of every sample's decode against its target -- so that only [B, 4] integers have to leave the device.
 *   logits, dtype, strides, input_lengths, blank, tokens, counts   exactly as wavlm_ctc_greedy takes and writes them
 *   targets  int32 [B, Lt] row-major, padded (the criterion's sample["target"]); pad and eos are dropped wherever they stand
 *   cls      uint8 [C]: 0 = DROP (the dictionary's string() omits the token), 1 = SEP (the word boundary `|`), 2 = LETTER.  A
 *            target id outside [0, C) never indexes the table: it is a LETTER, compared by value
 *   each_token_a_word  0: DROP tokens are removed, then words are the maximal runs of LETTER tokens between SEPs (post_process =
 *            "letter": a dropped token inside a word does not split it; leading, trailing and repeated separators make no empty
 *            words).  1: every non-DROP token is a word of its own (post_process = None)
 *   out      int32 [B, 4]: c_err = Levenshtein(decode, target units), c_len = target units, w_err = Levenshtein(decode's words,
 *            target's words), w_len = target's words.  The decode keeps whatever pad / eos / unk the argmax produced.  Two words
 *            are equal when their token ids are (a hash only spares the comparison): all integer, exact
 *   workspace  wavlm_ctc_score_workspace_bytes(B, T, Lt) bytes, 4-byte aligned: per sample the target's units, both word streams
 *            and their span tables (first token, length, hash): 5 Lt + 4 T ints
 * One launch, one workgroup per sample; the two DPs run one wave each with the row in registers (no atomics, nothing that
 * depends on B or on the sample's place in the batch).  wavlm_ctc_score_supported (host): 1 for T >= 1 and 0 <= Lt <= 1024 (64
 * lanes x 16 columns); wavlm_ctc_score returns -1 otherwise, and for a NULL pointer, a bad view or a short workspace.
 * ------------------------------------------------------------------------------------------ */
int wavlm_ctc_score_supported(int32_t T, int32_t Lt);
uint64_t wavlm_ctc_score_workspace_bytes(int32_t B, int32_t T, int32_t Lt);
int wavlm_ctc_score(const void* logits, int32_t dtype, int64_t stride_b, int64_t stride_t, int32_t B, int32_t T, int32_t C,
                    const int32_t* input_lengths, int32_t blank, const int32_t* targets, int32_t Lt, int32_t pad, int32_t eos,
                    const uint8_t* cls, int32_t each_token_a_word, int32_t* tokens, int32_t* counts, int32_t* out,
                    void* workspace, uint64_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * CTC beam search with an n-gram unit LM (csrc/ctc_beam.hip; additive to ABI 30: three new symbols, nothing else changes): the
 * lexicon-free decoder of examples/speech_recognition/w2l_decoder.py (--unit-lm, no lexicon; flashlight's LexiconFreeDecoder with
 * the CTC criterion and log_add = false).  The rules are written out at unispeech_amd.ctc.beam_search_reference.
 *   logits, dtype, strides, input_lengths, blank   as wavlm_ctc_greedy takes them
 *   sil        the class that takes sil_weight (-1: none)
 *   normalized 0: each frame's log-sum-exp is subtracted from its logits (fp32); 1: the input holds log-probabilities
 *   lm_*       the tables of unispeech_amd.ctc_lm.NgramLM on the device: child_off int32 [lm_nodes + 1], child_word / child_logp /
 *              child_next [lm_children] (a node's children ascending by word), node_backoff / node_suffix [lm_nodes], tok_word
 *              int32 [C] (class -> word), lm_start the state of <s>, lm_eos_word the word </s>, lm_order 1 .. 6.  Without an LM:
 *              lm_nodes = lm_order = 0 and the pointers are not read (one state, every LM score 0)
 *   beam, beam_tokens, beam_threshold (>= 0, may be +inf), lm_weight, sil_weight, nbest (1 .. beam)   the decoder's options
 *   tokens     int32 [B, nbest, T]: hypothesis h of sample b in tokens[b, h, 0 .. counts[b, h]), -1 behind it
 *   counts     int32 [B, nbest]; scores fp32 [B, nbest] (-inf for h >= n_hyp[b]); n_hyp int32 [B]: the hypotheses returned
 *   workspace  wavlm_ctc_beam_workspace_bytes(B, T, beam) bytes, 4-byte aligned: the back-pointers, B x T x beam int32
 * One launch, one workgroup per sample, no global atomics; a sample's result does not depend on B or on its place in the batch.
 * Emissions must be finite.  wavlm_ctc_beam_supported (host): 1 for 1 <= C <= 1024, 1 <= beam <= 512, beam_tokens >= 1,
 * beam x min(beam_tokens, C) <= 16384 and 0 <= lm_order <= 6; wavlm_ctc_beam returns -1 otherwise, and for a NULL pointer, a bad
 * view or a short workspace.  Inside that envelope nothing is truncated: the result is the reference's.
 * ------------------------------------------------------------------------------------------ */
int wavlm_ctc_beam_supported(int32_t C, int32_t beam, int32_t beam_tokens, int32_t lm_order);
uint64_t wavlm_ctc_beam_workspace_bytes(int32_t B, int32_t T, int32_t beam);
int wavlm_ctc_beam(const void* logits, int32_t dtype, int64_t stride_b, int64_t stride_t, int32_t B, int32_t T, int32_t C,
                   const int32_t* input_lengths, int32_t blank, int32_t sil, int32_t normalized, const int32_t* lm_child_off,
                   const int32_t* lm_child_word, const float* lm_child_logp, const int32_t* lm_child_next,
                   const float* lm_node_backoff, const int32_t* lm_node_suffix, const int32_t* lm_tok_word, int32_t lm_nodes,
                   int32_t lm_children, int32_t lm_start, int32_t lm_eos_word, int32_t lm_order, int32_t beam,
                   int32_t beam_tokens, float beam_threshold, float lm_weight, float sil_weight, int32_t nbest, int32_t* tokens,
                   int32_t* counts, float* scores, int32_t* n_hyp, void* workspace, uint64_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Lexicon-constrained CTC beam search with a word n-gram LM (csrc/ctc_lexbeam.hip; additive to ABI 30: three new symbols): the
 * decoder of examples/speech_recognition/w2l_decoder.py with --lexicon (flashlight's LexiconDecoder, CTC criterion, log_add =
 * false, SmearingMode::MAX).  The rules are written out at unispeech_amd.ctc_lexicon.lexicon_beam_search_reference.
 *   logits .. lm_order   as wavlm_ctc_beam takes them, except that lm_tok_word is int32 [lex_words]: lexicon word id -> LM word
 *   lex_*      the trie of unispeech_amd.ctc_lexicon.Lexicon on the device (node 0 is the root): child_off int32 [lex_nodes + 1],
 *              child_tok / child_node int32 [lex_children] (a node's children ascending by token), node_max fp32 [lex_nodes] (the
 *              smeared maximum of the words' scores at and below a node), label_off int32 [lex_nodes + 1], label_word int32
 *              [lex_labels] (the words whose spelling ends at a node), lex_words the number of words, unk_word the word <unk>
 *   lex_width  an upper bound on the candidates of one hypothesis in one frame, computed by the host from the trie
 *   beam .. nbest   the decoder's options; word_score finite, unk_score finite or -inf (no <unk> words)
 *   tokens, counts, scores, n_hyp   as wavlm_ctc_beam writes them
 *   words      int32 [B, nbest, T]: the words of hypothesis h in words[b, h, 0 .. word_counts[b, h]), -1 behind them
 *   word_counts int32 [B, nbest]
 *   workspace  wavlm_ctc_lexbeam_workspace_bytes(B, T, beam, lex_width) bytes, 4-byte aligned
 * One launch, one workgroup per sample, no global atomics; a sample's result does not depend on B or on its place in the batch.
 * wavlm_ctc_lexbeam_supported (host): 1 for 1 <= C <= 1024, 1 <= beam <= 512, width >= 1, beam x width <= 16384, 0 <= lm_order
 * <= 6 and 1 <= lex_nodes <= 2^21; wavlm_ctc_lexbeam returns -1 otherwise, and for a NULL pointer, a bad view or a short
 * workspace.  Inside that envelope nothing is truncated: the result is the reference's.
 * ------------------------------------------------------------------------------------------ */
int wavlm_ctc_lexbeam_supported(int32_t C, int32_t beam, int32_t width, int32_t lm_order, int32_t lex_nodes);
uint64_t wavlm_ctc_lexbeam_workspace_bytes(int32_t B, int32_t T, int32_t beam, int32_t width);
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
                      int32_t* words, int32_t* word_counts, void* workspace, uint64_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * CTC forced alignment (csrc/ctc_align.hip; additive to ABI 30: three new symbols, nothing else changes): the best path of a
 * transcript through the emissions -- which frames belong to which label -- and from it the `timesteps` of
 * examples/speech_recognition/w2l_decoder.py:243-262.  The rules are written out at
 * unispeech_amd.ctc_align.forced_align_reference; the path is that float64 restatement's bit for bit (the recursion runs on the
 * raw logits in float64: max is exact and every value is one addition of the same two operands on both sides).
 *   logits, dtype, strides, targets, target_offsets, n_targets, Lmax, input_lengths, blank   exactly as wavlm_ctc_loss takes them;
 *            any C >= 1, and rows at or beyond a sample's input length are never read
 *   frames   int32 [B, T]: the index j in [0, L) of the label that frame t emits, -1 for a blank frame, -2 for t >= input length
 *   spans    int32 [B, Lmax, 2]: first frame and one-past-last frame of label j; -1 for j >= L
 *   token_scores fp32 [B, Lmax]: the sum of lp[t, l_j] over the label's frames, lp = logits - row log-sum-exp, added in
 *            ascending t in float64 and rounded once; 0 for j >= L
 *   score    fp32 [B]: the sum of lp over all frames of the path, in ascending t, float64, rounded once
 *   workspace  wavlm_ctc_align_workspace_bytes(B, T, Lmax) bytes, 16-byte aligned: uint64 [B, 4] clock stamps in front (100 MHz
 *            ticks at the sample's start, after the forward pass, after the back-trace and at its end -- tools/ctc_align_bench.py
 *            reads them), the row log-sum-exp in float64, and the back-pointers, 2 bits per (b, t, s) in 16-byte groups of 64
 *            positions
 * Ties: among equal predecessors the one with the larger s wins (stay over s - 1 over s - 2), and at the end S - 1 wins over
 * S - 2: of all best paths, the one whose state sequence read from the last frame to the first is lexicographically greatest.
 * Special cases: no alignment exists (the input length is below L + the number of adjacent equal labels): score -inf, frames -2
 * throughout, spans -1, token_scores 0.  Input length 0: score 0 for L = 0, -inf otherwise.  An offset or a label out of range:
 * score NaN, the rest as without an alignment (wavlm_ctc_loss treats such a sample the same way).
 * Two launches (row log-sum-exp; forward, back-trace and sums by one workgroup per sample), no global atomics; a sample's result
 * does not depend on B or on its place in the batch.  The back-trace reads the back-pointers from LDS, staged
 * WAVLM_CTC_ALIGN_BLOCK frames at a time.  wavlm_ctc_align_supported (host): 1 for 0 <= Lmax <= 1023; wavlm_ctc_align returns -1
 * otherwise, and for a NULL pointer, a bad view or a short workspace.
 * ------------------------------------------------------------------------------------------ */
#define WAVLM_CTC_ALIGN_BLOCK 32
int wavlm_ctc_align_supported(int32_t Lmax);
uint64_t wavlm_ctc_align_workspace_bytes(int32_t B, int32_t T, int32_t Lmax);
int wavlm_ctc_align(const void* logits, int32_t dtype, int64_t stride_b, int64_t stride_t, int32_t B, int32_t T, int32_t C,
                    const int32_t* targets, const int32_t* target_offsets, int32_t n_targets, int32_t Lmax,
                    const int32_t* input_lengths, int32_t blank, int32_t* frames, int32_t* spans, float* token_scores,
                    float* score, void* workspace, uint64_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Transformer LM (csrc/lm.hip; additive to ABI 30: five new symbols, nothing else changes): the two steps of an inference pass of
 * the reference's decoder-only TransformerDecoder (src/fairseq/models/transformer.py:636-991, as TransformerLanguageModel builds
 * it) that no other entry point covers.  Its Linear layers are wavlm_gemm calls, its LayerNorms wavlm_layernorm_fwd calls
 * (unispeech_amd/transformer_lm.py).  Tensors WL_F32 or WL_BF16; accumulation, softmax state and results in fp32.
 *   wavlm_lm_logprob      transformer.py:965-971 + get_normalized_probs(log_probs=True) + the target's entry, as FairseqLM reads
 *                         it (examples/speech_recognition/w2l_decoder.py:366-383).  X [R, D] (row stride ldx), W [V, D] (row
 *                         stride ldw; the output projection as the checkpoint stores it, no bias), target int32 [R]:
 *                           z[r, v] = sum_i X[r, i] * W[v, i]   (fp32 accumulation; never stored)
 *                           lse[r] = log sum_v exp z[r, v]      (optional: NULL = not wanted)
 *                           logprob[r] = z[r, target[r]] - lse[r]
 *                         target[r] < 0: a padding row, logprob[r] = 0.  target[r] >= V: logprob[r] = NaN (wavlm_ctc_loss treats
 *                         bad labels the same way).  V is cut into slabs of 2048 entries -- a function of V alone; a workgroup
 *                         owns 128 rows and one slab and keeps a running maximum, a running sum and the target's logit per row
 *                         (online softmax; bf16 on v_mfma_f32_32x32x16_bf16 with the row on the lane, the target's logit taken
 *                         from the same accumulator as the logits under the sum; fp32: fp32 FMA in k order).  Each (slab, row)
 *                         writes (max, sum, target logit) to `workspace`; a second launch folds them in slab order.  No global
 *                         atomics: bitwise reproducible, and a row's result depends neither on R nor on the row's position.
 *                         workspace: wavlm_lm_logprob_workspace_bytes(R, V) = 12 bytes x R x ceil(V / 2048), rounded up to 256 --
 *                         O(R x slabs), never O(R x V); 16-byte aligned.
 *                         wavlm_lm_logprob_supported (host): 1 for D % 8 == 0, 8 <= D <= 8192, 1 <= V < 2^31 and the two dtypes.
 *                         wavlm_lm_logprob returns -1 otherwise, and for a NULL pointer (lse excepted), ldx or ldw below D, X or W
 *                         or a row stride that is not 16-byte aligned, a short workspace, or R x slabs beyond one grid dimension.
 *   wavlm_attn_causal_fwd modules/transformer_layer.py:349-357 under the future mask (transformer.py:979-991): the packed qkv
 *                         [B, T, 3 * H * d] and O [B, T, H * d] of wavlm_attn_plain_fwd; query t of sequence b attends keys 0..t.
 *                         lengths int32 [B] on the device (NULL: every sequence is T long): rows t >= lengths[b] are written as
 *                         zeros and no result reads them (right padding).  head_dim 32 or 64, any T >= 1, B * H <= 65535; online
 *                         softmax, no [B H, T, T] tensor; key tiles entirely above the diagonal are skipped, not masked.  bf16:
 *                         both products on v_mfma_f32_32x32x16_bf16 with fp32 softmax state; fp32: fp32 FMA throughout.  A
 *                         sequence's result does not depend on B, on T beyond its length, or on its place in the batch.
 * ------------------------------------------------------------------------------------------ */
int wavlm_lm_logprob_supported(int32_t D, int32_t V, int32_t dtype);
uint64_t wavlm_lm_logprob_workspace_bytes(int64_t R, int32_t V);
int wavlm_lm_logprob(const void* X, int64_t ldx, const void* W, int64_t ldw, int32_t dtype, const int32_t* target, int64_t R,
                     int32_t D, int32_t V, float* logprob, float* lse, void* workspace, uint64_t ws_bytes, void* stream);
int wavlm_attn_causal_fwd_supported(int32_t head_dim, int32_t dtype);
int wavlm_attn_causal_fwd(const void* qkv, void* O, const int32_t* lengths, int32_t B, int32_t H, int32_t T, int32_t head_dim,
                          int32_t dtype, float scale, void* stream);

/* ------------------------------------------------------------------------------------------
 * Transformer LM, incremental decoding (csrc/lm_step.hip; additive to ABI 30: two new symbols, nothing else changes).
 *   wavlm_attn_step       single-query self-attention over a tree-shaped KV cache: one new token per row, the rows' prefixes
 *                         forming a tree (the word histories of a beam).  A cache entry ("slot") holds the K and the V of one
 *                         token of one layer: Kc, Vc [slots, H * d] (row stride ld_kv).  Row r brings its packed q | k | v
 *                         (qkv [R, 3 * H * d], row stride ld_qkv); slot[r] names the slot its own k and v are written to;
 *                         anc[r * ld_anc + 0 .. lengths[r] - 2] (int32) names the slots of its ancestors in position order;
 *                         lengths[r] counts the row itself.
 *                           O[r, h * d + :] = softmax(scale * q[r, h] . [K[anc[r, .], h] ; k[r, h]]) [V[anc[r, .], h] ; v[r, h]]
 *                         fp32 softmax state and accumulation, online softmax, no score tensor.  The own k and v are stored
 *                         from the registers the softmax uses, by the same launch; a row never reads a slot written in that
 *                         launch (the caller evaluates parents before children and names each slot once per launch).
 *                         lengths[r] <= 0: O[r] is zeros and nothing is stored.  Entries of anc at or beyond lengths[r] - 1
 *                         are never read; slots not named are never read.  What a caller must not pass is answered without
 *                         forming an address: lengths[r] > max_length, slot[r] outside [0, slots) or a read ancestor outside
 *                         [0, slots) gives a row of NaN and stores nothing.  One wave per (row, head), the 64 lane states
 *                         folded in lane order: no atomics, bitwise reproducible, a row's bits depend neither on R nor on its
 *                         place in the batch.  head_dim 32 or 64, WL_F32 or WL_BF16.
 *                         Returns -1 before any launch for a NULL pointer, qkv / Kc / Vc / O or a row stride of theirs that is
 *                         not 16-byte aligned, an int32 array that is not 4-byte aligned, two of qkv / Kc / Vc / O whose
 *                         byte ranges (first row to the end of the last) overlap, a row stride shorter than its row,
 *                         ld_anc < max_length - 1, an unsupported head width or dtype, R, H, slots or max_length below 1, or
 *                         R * H beyond one grid dimension.
 * ------------------------------------------------------------------------------------------ */
int wavlm_attn_step_supported(int32_t head_dim, int32_t dtype);
int wavlm_attn_step(const void* qkv, int64_t ld_qkv, void* Kc, void* Vc, int64_t ld_kv, int64_t slots, const int32_t* slot,
                    const int32_t* anc, int64_t ld_anc, const int32_t* lengths, int32_t max_length, void* O, int64_t ld_o,
                    int32_t R, int32_t H, int32_t head_dim, int32_t dtype, float scale, void* stream);

/* ------------------------------------------------------------------------------------------
 * Seq2seq ASR decoding (csrc/s2s.hip; additive to ABI 30: five new symbols, nothing else changes).
 *   wavlm_attn_cross_fwd  encoder-decoder attention: a few query rows per sentence over its encoder frames.  Q [R, H * d] (row
 *                         stride ld_q); KV [B, Ts, 2 * H * d], a frame's keys then its values (batch stride s_kv, row stride
 *                         ld_kv); src_lengths int32 [B] on the device (NULL: every sentence is Ts long; values are clamped to
 *                         [0, Ts]); row_offsets int32 [B + 1]: rows row_offsets[b] .. row_offsets[b + 1] - 1 attend sentence b
 *                         (a group may be empty; rows that no group names are not written); live int32 [R] or NULL: a row
 *                         with live[r] <= 0 is written as zeros and reads nothing; O [R, H * d] (row stride ld_o).
 *                           O[r, h] = softmax(scale * q[r, h] . K[b, 0 .. len_b - 1, h]) V[b, 0 .. len_b - 1, h]
 *                         fp32 softmax state and accumulation, online softmax, no score tensor; keys at or beyond
 *                         src_lengths[b] are never read; src_lengths[b] <= 0 gives rows of zeros.  One workgroup owns
 *                         (sentence, head, tile of up to 32 rows) and walks K and V once for the tile: the rows of a sentence
 *                         share the pass.  Its four waves split the keys by the key index alone and are folded through LDS in
 *                         wave order; bf16: both products on v_mfma_f32_32x32x16_bf16 (keys x queries: a query's softmax
 *                         state sits on a lane), fp32: FMA in channel order.  No atomics.  Bitwise reproducible; a row's bits
 *                         depend neither on the other rows of its group, nor on the group's size, nor on B, nor on its place
 *                         in the batch.  max_group >= 1 sizes the grid: the largest group the caller expects (B * H *
 *                         ceil(min(max_group, R) / 32) workgroups); a larger group is still computed in full, its workgroups
 *                         taking several tiles each, with the same bits.  head_dim 32 or 64, WL_F32 or WL_BF16, any Ts >= 1.
 *                         Offsets that are not non-decreasing or leave [0, R] form no address: the rows between the two
 *                         offending entries (clamped to [0, R)) come back as NaN -- except a row that a sound group names as
 *                         well: two workgroups write it, and it holds either that group's result or NaN (unspecified which).
 *                         A tile whose rows are all dead (live <= 0) reads neither Q nor K nor V.
 *                         Returns -1 before any launch for a NULL pointer (src_lengths and live excepted), Q / KV / O or a
 *                         stride of theirs that is not 16-byte aligned, an int32 array that is not 4-byte aligned, ld_q or ld_o
 *                         below H * d, ld_kv below 2 * H * d, s_kv shorter than a sentence, two of Q / KV / O whose byte ranges
 *                         overlap, an unsupported head width or dtype, R, B, Ts, H or max_group below 1, or a grid beyond one
 *                         dimension.
 *   wavlm_beam_step       one step of SequenceGenerator._generate (src/fairseq/sequence_generator.py:326-560) with
 *                         BeamSearch.step (src/fairseq/search.py:103-147) for every sentence; one workgroup per sentence.  Rows
 *                         are r = b * beam + k; sentence b has n_live[b] live rows k < n_live[b] (1 at step 0, up to beam
 *                         afterwards, 0 once finished).  logits [B * beam, V] (dtype, row stride ld_logits; rows that are not
 *                         live are not read; an entry of -inf is a token of probability 0, a NaN or +inf entry makes its whole
 *                         row -inf, as torch.log_softmax followed by line 346 does), cum fp32 [B * beam] the rows' cumulative scores (0 at step 0).  In order: the
 *                         logits over `temperature`, log-softmax in fp32 (811-815); NaN -> -inf (346); pad -> -inf, unk -=
 *                         unk_penalty (348-349); at step >= max_len everything but eos -> -inf (352-354); at step < min_len
 *                         eos -> -inf (365-367); + cum[row]; the best min(2 beam, n_live V - 1) of the sentence by (score
 *                         descending, k * V + token ascending) -- torch.topk leaves ties open, this does not.  The walk
 *                         (405-520): an eos (with a score above -inf) among the first `beam` ranks goes to the finished list
 *                         while that has fewer than `beam` entries: fin_f [B, beam, 3] = (score / (step + 1)^len_penalty if
 *                         normalize_scores else score, score, score - parent's cum), fin_i [B, beam, 2] = (parent slot,
 *                         length = step + 1), n_fin [B]; an eos at a later rank is dropped.  The first `beam` others become
 *                         the next step's rows k' = 0, 1, ..: tokens[r], cum[r], lengths[r] = step + 2, slots[r] = ((step + 1)
 *                         B + b) beam + k' (static: a row's slot in a KV cache of wavlm_attn_step and in the tree),
 *                         anc_out[r, 0 .. step] = anc_in[parent row, 0 .. step - 1] then the parent's slot (step B + b) beam +
 *                         k (two buffers, ping-pong, row stride ld_anc >= step + 1), tree_parent / tree_token / tree_score
 *                         [tree_slots] at the new slot (score: the step's own, new cum - parent's cum, as finalize_hypos
 *                         takes positional scores).  Rows beyond them get lengths 0, token pad, cum -inf.  A sentence with
 *                         `beam` finished entries, or at step >= max_len, or without a candidate left, gets n_live = 0 and
 *                         *finished (int32, device) goes up by one (715-735) -- the only global atomic.  workspace holds the
 *                         candidates for inspection: fp32 scores [B, 2 beam], int32 flat indices [B, 2 beam], int32 counts
 *                         [B] (wavlm_beam_step_workspace_bytes, 16-byte aligned).  Bitwise reproducible; a sentence's result
 *                         depends neither on B nor on its place in the batch.
 *                         wavlm_beam_step_supported (host): 1 for 1 <= beam <= 32, 2 <= V <= 65536, 1 <= B <= 65535 and the two
 *                         dtypes.  Returns -1 before the launch otherwise, and for a NULL pointer, anc_in == anc_out, ld_logits <
 *                         V, ld_anc < step + 1, tree_slots < (step + 2) B beam, temperature <= 0, a negative step or max_len, or
 *                         a short or misaligned workspace.
 *   wavlm_beam_step_fused the same step -- same state arrays, tie rule, walk, finished lists, tree and workspace -- with two
 *                         more rules.  Shallow fusion (338-344): lm_logits [B * beam, V] (lm_dtype, row stride ld_lm; NULL:
 *                         none) gets a log-softmax of its own, without temperature, and per entry, in fp32 and in this order,
 *                           lp = (x / temperature - M) - logS;  lm = (y - Ml) - logSl;  lp += lm_weight * lm
 *                         before NaN -> -inf (346) and the rules above.  Taken literally: 0 * -inf is NaN, hence -inf, and a
 *                         NaN anywhere in an LM row kills that row.  The n-gram blocker (no_repeat_ngram_size = n > 0,
 *                         388-389, ngram_repeat_block.py:96-143) comes after those rules: the history of row k is h[j] =
 *                         tree_token[anc_in[k][j]] for j < step and h[step] = tokens[row] (h[0] is the bos); for every i in
 *                         0 .. step + 1 - n with h[i .. i + n - 2] == h[step + 2 - n .. step], token h[i + n - 1] is -inf.
 *                         n = 1 bans every token of the history, eos included.  A banned token still counts in the normaliser.
 *                         THE LOGITS BUFFER IS CONSUMED: once both log-softmax states are taken the workgroup overwrites
 *                         the banned entries of `logits` with -inf -- those entries of live rows and nothing else; with n = 0
 *                         nothing is written.  About history x n reads per row, no LDS sized by beam x V or beam x history,
 *                         no atomics besides *finished.  With lm_logits == NULL and n == 0 every output equals
 *                         wavlm_beam_step's bit for bit.  Bitwise reproducible; a sentence's result depends neither on B nor
 *                         on its place in the batch.  Returns -1 before the launch, the state untouched, for everything
 *                         wavlm_beam_step refuses and for ld_lm < V, a misaligned lm_logits or one that overlaps logits, an
 *                         lm_dtype that is neither, n < 0 and an lm_weight that is not finite.  The workspace is
 *                         wavlm_beam_step_workspace_bytes.
 * ------------------------------------------------------------------------------------------ */
int wavlm_attn_cross_fwd_supported(int32_t head_dim, int32_t dtype);
int wavlm_attn_cross_fwd(const void* Q, int64_t ld_q, const void* KV, int64_t s_kv, int64_t ld_kv, const int32_t* src_lengths,
                         const int32_t* row_offsets, const int32_t* live, void* O, int64_t ld_o, int32_t R, int32_t B, int32_t Ts,
                         int32_t H, int32_t head_dim, int32_t dtype, float scale, int32_t max_group, void* stream);
int wavlm_beam_step_supported(int32_t beam, int32_t V, int32_t B, int32_t dtype);
uint64_t wavlm_beam_step_workspace_bytes(int32_t B, int32_t beam);
int wavlm_beam_step(const void* logits, int64_t ld_logits, int32_t dtype, float* cum, int32_t* n_live, int32_t* tokens,
                    int32_t* lengths, int32_t* slots, const int32_t* anc_in, int32_t* anc_out, int64_t ld_anc,
                    int32_t* tree_parent, int32_t* tree_token, float* tree_score, int64_t tree_slots, float* fin_f, int32_t* fin_i,
                    int32_t* n_fin, int32_t* finished, int32_t B, int32_t beam, int32_t V, int32_t step, int32_t max_len,
                    int32_t min_len, int32_t pad, int32_t unk, int32_t eos, float unk_penalty, float temperature,
                    float len_penalty, int32_t normalize_scores, void* workspace, uint64_t ws_bytes, void* stream);
int wavlm_beam_step_fused_supported(int32_t beam, int32_t V, int32_t B, int32_t dtype, int32_t lm_dtype);
int wavlm_beam_step_fused(void* logits, int64_t ld_logits, int32_t dtype, const void* lm_logits, int64_t ld_lm, int32_t lm_dtype,
                          float lm_weight, int32_t no_repeat_ngram_size, float* cum, int32_t* n_live, int32_t* tokens,
                          int32_t* lengths, int32_t* slots, const int32_t* anc_in, int32_t* anc_out, int64_t ld_anc,
                          int32_t* tree_parent, int32_t* tree_token, float* tree_score, int64_t tree_slots, float* fin_f,
                          int32_t* fin_i, int32_t* n_fin, int32_t* finished, int32_t B, int32_t beam, int32_t V, int32_t step,
                          int32_t max_len, int32_t min_len, int32_t pad, int32_t unk, int32_t eos, float unk_penalty,
                          float temperature, float len_penalty, int32_t normalize_scores, void* workspace, uint64_t ws_bytes,
                          void* stream);

/* ------------------------------------------------------------------------------------------
 * Measurement aid (bench.py roofline leg): HIP events around every wavlm_gemm launch while enabled.
 * ------------------------------------------------------------------------------------------ */
void wavlm_prof_enable(int on);
/* 0: automatic tile choice, 1: force the 128x128 tile (A/B measurements only) */
void wavlm_gemm_set_variant(int v);
/* Data-parallel runs: leave `n` of the 256 CUs out of every PERSISTENT GEMM launch (grid 256 - n), so that the RCCL
 * kernels of the gradient all-reduce (side stream; replaces the blocking all-reduce after backward of
 * src/fairseq/distributed/legacy_distributed_data_parallel.py:132-165) find free CUs while backward is still running.
 * 0 (default) = use the whole chip.  Values are clamped to [0, 64]. */
void wavlm_set_reserved_cus(int n);
int wavlm_get_reserved_cus(void);
int wavlm_prof_collect(int dtype, double* total_ms, double* total_flops);
/* algorithmic HBM bytes of the recorded launches: every operand, output and epilogue tensor counted once */
double wavlm_prof_collect_bytes(int dtype);
/* Kernel classes timed besides wavlm_gemm (class 0) while profiling is enabled: the fused attention forward / backward
 * (backward = dQ + dK/dV kernels + their finishing launches), the conv0 stage forward / backward (either norm mode) and
 * the LayerNorm row kernels.  Returns the number of recorded calls of class `cls`; totals: duration [ms], algorithmic
 * FLOPs (attention: 4 B H T^2 hd forward, 10 B H T^2 hd backward) and algorithmic HBM bytes (every input / output tensor
 * of the call once).  Blocks until the recorded launches have finished. */
#define WL_PROF_GEMM 0
#define WL_PROF_ATTN_FWD 1
#define WL_PROF_ATTN_BWD 2
#define WL_PROF_CONV0_FWD 3
#define WL_PROF_CONV0_BWD 4
#define WL_PROF_LN_FWD 5
#define WL_PROF_LN_BWD 6
int wavlm_prof_collect_class(int cls, double* total_ms, double* total_flops, double* total_bytes);
/* one text line per recorded wavlm_gemm launch into `path`: M N K KB trans epi split batches ms gflop (tools/gemm_step_table.py:
 * which shapes of a real step sit where against the MFMA peak).  Returns the number of lines, < 0 on error. */
int wavlm_prof_dump(const char* path);

#ifdef __cplusplus
}
#endif
#endif
