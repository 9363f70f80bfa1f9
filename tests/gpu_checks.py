"""Kernel-level parity checks: each HIP entry point / autograd function against a plain PyTorch fp32 (fp64 where
cheap) CPU reference of the same op on seeded inputs.  Used by tests/test_kernels_gpu.py (pytest -m gpu) and by
tools/gpu_report.py (crash-isolated report).  Every check returns a list of (name, error, tolerance).

Error metric: max |a - b| / max(|b|_max, tiny) -- "relative to the tensor scale" -- unless noted.
Tolerances: fp32 mode 1e-4 (BASELINE.json north_star) except long fp32 reductions (2e-4); bf16 mode 2e-2.

The row kernels (rowops.hip, optim.hip) are grid-stride kernels with a grid cap, and four groups run them where a wave or a
thread takes several items, against fp64 torch on the device.  Their shapes rest on the launch geometry -- 4 rows per block,
LayerNorm caps of 1024 blocks (forward: full-width kernels, and every forward with dropout), 512 (backward, LN_BWD_BLOCKS) and
8192 (general forward without dropout), rows / 128 and rows / 256 above 131 072 rows, CS_BLOCKS = 512 for colsum -- so a retuned
cap moves the shape named beside it:
  layernorm_rows         8195 rows (= 2 * 4096 + 3 = 4 * 2048 + 3: 2-3 rows per forward wave, 4-5 per backward wave, ragged last
                         sweeps), 1 / 5 / 8192 rows, 32 773 rows (general forward past 4 * 8192), 262 149 rows (past the cap change)
  layernorm_dropout_ref  8195 rows: forward (1024 blocks) and backward (512) regenerate one mask with different row assignments
  colsum_rows            799 / 1027 / 1795 / 2048 / 8195 rows = 200 / 257 / 449 / 512 / 512 partial rows (the finish kernel's unrolled
                         loop needs more than 192), the last one strided over CS_BLOCKS
  flat_strided           n just past 16384 x 256 (adam_step), 8192 x 256 (axpby, scale_dev; x 8 for dropout, dropout_add),
                         1024 x 4096 (sumsq), 4096 x 256 x 8 (select_rows, gather_rows)
tests/test_kernels_gpu.py runs the two LayerNorm groups once more in a fresh process under WAVLM_LN_FULL=0.

The kernels of loss.hip loop the same way -- 8192 blocks of 4 rows (l2norm_fwd, l2norm_bwd, ce_rows, gather_dot, rows_wsum), 8192
blocks of one row (glu_fwd, glu_bwd), 8192 x 256 elements (act_fwd, act_bwd), 1024 blocks x 2048 elements (sum_f32, bce_logits) --
and two groups run them there, against fp64 torch on the device:
  masked_pred_head       MaskedPredLossFn and its kernels one by one at (S, V, F) = (1029, 504, 256), (12 805, 504, 256), (32 773, 504,
                         256) -- the label-embedding gradient's split-K (ops.pick_split on S / 64 K tiles) at 2, 25 and its cap of 64
                         slabs; 32 773 = 4 x 8192 + 5 rows -- (2053, 504, 768), (1500, 100, 256), (1029, 500, 256), (1029, 1000, 256),
                         (5, 2, 8); skewed, out-of-range and zero-row inputs, need_grad=False, S = 0, target_glu at (1029, 504, 256)
  loss_rows_capped       32 773 rows (4 x 8192 + 5) for l2norm (D = 256, 100), ce_rows (V = 101, ld = 104), gather_dot (N = 3, D = 64)
                         and rows_wsum (D = 64); 8195 rows (8192 + 3) for glu (F = 48, 300); n = 8192 x 256 + 7 for act; n = 1024 x
                         2048 + 5 for sum_f32 and bce_logits

The convolutional position embedding (posconv.hip, posconv_direct.hip; PosConvFn) has three groups at its launch geometry, against
posconv_ref64 -- a loop over the K taps of a grouped matrix product in fp64 on the device, autograd for the gradients; tests/
test_posconv_ref.py holds its CPU side.  The constants a retune would move: posconv_dw_kernel's frame chunk TCH = 256 (Cg = 48) /
128 (Cg = 64) and batch splits BS = 4 / 2 (PDW_TCH, PDW_BS below); posconv_direct_kernel's candidate frame tiles 768, 512, 384 /
512, 384 (PCD_TILES); pc_group_major_kernel's grid cap of 8192 x 256 chunks of 8 elements (GM_CAP):
  posconv_batch          bf16, K = 128, G = 16; (B, T) = (5, 300) at Cg = 48: bchunk 2, splits of 2, 2, 1, 0 batches, two chunks with
                         a 44-frame tail; (8, 257): four full splits, a one-frame tail; (9, 64): bchunk 3, one chunk per batch; at
                         Cg = 64 (3, 200): splits of 2, 1, two chunks of 128; (5, 129): splits of 3, 2, a one-frame tail.  Where a
                         tail exists, once more with dy zero outside it.  At (5, 300) the inference forward, x without gradient, a
                         non-contiguous dy
  posconv_frames         bf16, K = 128, Cg = 48 as D = 96, G = 2 and Cg = 64 as D = 256, G = 4 (the smallest G with the direct dw
                         kernel), B = 1: T = 1, 16, 63, 127, 383, 384 (tile 384), 385, 512 (tile 512), 513 (768 against 2 x 384: the
                         tie goes to the larger tile), 768, 769 (2 x 512; also B = 2), 1153 (2 x 768 on a three-way tie), 1537
                         (5 x 384) at Cg = 48; T = 1, 65, 384, 385, 512, 513 (2 x 384; also B = 2), 1024 (2 x 512), 1025 (3 x 384),
                         1537 (5 x 384) at Cg = 64
  posconv_layouts        group_major at 5 x 16 x 3327 x 8 = 2 129 280 chunks (B = 5, T = 3200, D = 1024, G = 16, left_pad 64; the cap
                         is 2 097 152) into NaN-filled memory, and at B = T = 1; posconv_weight_fwd's norm and both images at (D, Cg,
                         K) = (96, 48, 128), (256, 64, 128) in layouts 0 and 1 and (64, 16, 15) in layout 0, placed by the index maps
                         of posconv.hip's comments, for fp32 -> bf16, bf16 -> bf16, fp32 -> fp32; posconv_weight_bwd on seeded slabs,
                         nsplit 1 and 4, at (96, 48, 128) and (1024, 64, 128); PosConvFn's GEMM form at (B, T, D, G) = (2, 49, 64, 4)
                         with K = 15, 3 (odd: the left pad of the gradient copy is K - 1 - K // 2) and 16; the refusals
Bounds: check_posconv's (tol_for(dtype) for y, x 2 for dx and dbias, x 3 for dv and dg; 1e-2 between the direct and the GEMM form).

The fused attention (attn_fused.hip, attn_fused_dkv.hip; ops.attn_fused_fwd / attn_fused_bwd, F.AttnCoreFn) has three groups at its
launch geometry, bf16 with head_dim 64, against _ref_attention / _ref_attention_masked in fp64 on the device; tests/
test_attention_ref.py holds their CPU side.  The constants a retune would move: 128 query rows per block of the forward and dQ
kernels and 128 key rows per block of the dK/dV kernel (FA_BQ), 4 partial rows per block -- one per wave of 32 rows -- for d(rel)
and for the q|k|v bias gradient (FA_PART), so ntot = B x 4 x ceil(T / 128) partial rows; fa_dtab_reduce_kernel's 64 row slices x 4
rows in flight, stepping by 256 (FA_RED_STRIDE): slice s adds the rows s + 64 u + 256 k; 64-key tiles of the online softmax;
FA_PSTORE_MAX_T = 1024 = FA_DKVP_ROWS, the last T with a probability store:
  attention_reduce       (B, H, T) = (17, 1, 100): ntot 68, the first use of u = 1; (33, 2, 130): 264, a second sweep with a ragged
                         end, 8 rows per item; (11, 1, 700): 264 with 24 rows per item, so item and row-in-item change in the
                         middle of a sweep; (32, 1, 749): 768, the training step's count.  Whole-batch parity of O, dqkv, dgate, dtab
                         and dbias (fp32 and bf16, written into NaN-filled memory and added onto a base) in the recompute and
                         stored-P modes; each of the partial rows 0, 63, 64, 65, 127, 128, 191, 192, 255, 256, ntot - 1 ALONE (dO zero
                         elsewhere) against a B = 1 reference of its item, the other items' dqkv and dgate exactly zero; gate = tab =
                         None at (33, 2, 130).  Every backward runs over a workspace of 0xFF bytes
  attention_ragged       B = 8, H = 2, T = 300: lengths 300, 257, 256, 129, 65, 2; keys [0, 70) and [128, 192) masked (a dead first
                         tile, a dead tile between live ones); length 1.  PER ITEM, each slice against its own reference maximum;
                         recompute, stored P and unfused without dropout, the three fused modes with dropout 0.25 under the kernels'
                         own mask (identical in forward, dQ, dK/dV); dk, dv of masked keys exactly zero; an item alone gives the bits
                         it gives in the batch
  attention_long         T = 1024 (store returned, LDS row arrays full), 1025 (no store: AttnCoreFn recomputes), (2, 2, 1153) with
                         item 1 at 1030, 1537; dropout 0.25 at 1025 in the recompute and stored-bits modes, bit-identical
Bounds: check_attention's (TOLBF for O, 2 x TOLBF for gradients), per slice where the metric is per item.
"""
import math
import sys

import numpy as np
import torch
import torch.nn.functional as TF

sys.path.insert(0, __file__.rsplit("/tests/", 1)[0])
from unispeech_amd import functional as F  # noqa: E402
from unispeech_amd import ops  # noqa: E402

DEV = "cuda"
ATTN_STORE_P_DEFAULT = F.ATTN_STORE_P   # restored after the checks that switch the attention backward mode
TOL32, TOLBF = 1e-4, 2e-2


def err(a, b):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    if a.shape != b.shape:
        return float("inf")
    if b.numel() == 0:
        return 0.0
    if not torch.isfinite(a).all():
        return float("inf")
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-12)).item()


def gen(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def tol_for(dtype):
    return TOL32 if dtype == torch.float32 else TOLBF


def q(t, dtype):
    """round a CPU fp32 tensor through `dtype` so that device and reference see identical inputs"""
    return t.to(dtype).float()


# ------------------------------------------------------------------------------------------------------ GEMM
def check_gemm():
    out = []
    # the 256x128 / 8-wave tile, forced, on ragged sizes in all four layouts (+ split-K)
    ops.gemm_set_variant(2)
    try:
        dtype, tol = torch.bfloat16, TOLBF
        for (M, N, K, tA, tB) in [(700, 200, 264, 0, 0), (513, 136, 749, 0, 1), (300, 260, 200, 1, 0), (258, 130, 333, 1, 1)]:
            Kp, Mp, Np = (K + 7) // 8 * 8, (M + 7) // 8 * 8, (N + 7) // 8 * 8
            A, B = q(gen(M, K, seed=21), dtype), q(gen(N, K, seed=22), dtype)
            ref = A.double() @ B.double().t()
            if tA:
                Ad = torch.zeros(K, Mp); Ad[:, :M] = A.t(); lda = Mp
            else:
                Ad = torch.full((M, Kp), float("nan")); Ad[:, :K] = A; lda = Kp
            if tB:
                Bd = torch.zeros(K, Np); Bd[:, :N] = B.t(); ldb = Np
            else:
                Bd = torch.full((N, Kp), float("nan")); Bd[:, :K] = B; ldb = Kp
            Ad, Bd = Ad.to(dtype).to(DEV), Bd.to(dtype).to(DEV)
            for split in (1, 3):
                C = torch.full((M, Np), float("nan"), dtype=dtype, device=DEV)
                ops.gemm(Ad, Bd, C, M, N, K, lda=lda, ldb=ldb, ldc=Np, transA=tA, transB=tB, split_k=split)
                out.append((f"gemm256[{dtype}] {M}x{N}x{K} tA={tA} tB={tB} split={split}", err(C[:, :N], ref), tol))
    finally:
        ops.gemm_set_variant(0)
    for dtype in (torch.float32, torch.bfloat16):
        tol = tol_for(dtype)
        for (M, N, K, tA, tB) in [(200, 136, 72, 0, 0), (129, 64, 264, 0, 1), (260, 130, 200, 1, 0), (77, 48, 333, 1, 1),
                                  (512, 256, 512, 0, 0), (48, 640, 749, 1, 1), (100, 72, 749, 0, 0), (100, 64, 749, 0, 1)]:
            Kp = (K + 7) // 8 * 8
            Mp = (M + 7) // 8 * 8
            Np = (N + 7) // 8 * 8
            A = q(gen(M, K, seed=1), dtype)
            B = q(gen(N, K, seed=2), dtype)
            ref = A.double() @ B.double().t()
            # storage: K-contiguous [rows, Kp] or K-strided [K, rows_p]
            if tA:
                Ad = torch.zeros(K, Mp); Ad[:, :M] = A.t(); lda = Mp
            else:
                Ad = torch.zeros(M, Kp); Ad[:, :K] = A; lda = Kp
            if tB:
                Bd = torch.zeros(K, Np); Bd[:, :N] = B.t(); ldb = Np
            else:
                Bd = torch.zeros(N, Kp); Bd[:, :K] = B; ldb = Kp
            # poison the padding with NaN where it must be ignored (K tail of K-contiguous operands)
            if not tA and Kp > K:
                Ad[:, K:] = float("nan")
            if not tB and Kp > K:
                Bd[:, K:] = float("nan")
            Ad = Ad.to(dtype).to(DEV); Bd = Bd.to(dtype).to(DEV)
            C = torch.full((M, N), float("nan"), dtype=torch.float32, device=DEV)
            ops.gemm(Ad, Bd, C, M, N, K, lda=lda, ldb=ldb, ldc=N, transA=tA, transB=tB)
            out.append((f"gemm[{dtype}] {M}x{N}x{K} tA={tA} tB={tB}", err(C, ref), tol))
            for split in (3,):
                C2 = torch.full((M, N), float("nan"), dtype=torch.float32, device=DEV)
                ops.gemm(Ad, Bd, C2, M, N, K, lda=lda, ldb=ldb, ldc=N, transA=tA, transB=tB, split_k=split)
                out.append((f"gemm[{dtype}] {M}x{N}x{K} tA={tA} tB={tB} split={split}", err(C2, ref), tol))
        # batched + K-batch + epilogues
        Bo, Bi, KB, M, N, K = 2, 3, 2, 70, 40, 64
        A = q(gen(Bo, Bi, KB, M, K, seed=3), dtype)
        B = q(gen(Bo, Bi, KB, N, K, seed=4), dtype)
        bias = q(gen(Bi, N, seed=5), dtype)
        res = q(gen(Bo, Bi, M, N, seed=6), dtype)
        pre = torch.einsum("oikmc,oiknc->oimn", A.double(), B.double()) * 0.5 + bias.double()[None, :, None, :]
        ref = TF.gelu(pre) + res.double()
        Ad, Bd = A.to(dtype).to(DEV), B.to(dtype).to(DEV)
        C = torch.empty(Bo, Bi, M, N, dtype=dtype, device=DEV)
        aux = torch.empty(Bo, Bi, M, N, dtype=dtype, device=DEV)
        ops.gemm(Ad, Bd, C, M, N, K, lda=K, ldb=K, ldc=N, KB=KB, sA_kb=M * K, sB_kb=N * K, batch=(Bo, Bi),
                 sA=(Bi * KB * M * K, KB * M * K), sB=(Bi * KB * N * K, KB * N * K), sC=(Bi * M * N, M * N), alpha=0.5,
                 bias=bias.to(dtype).to(DEV), sBias=(0, N), epi=1, aux=aux, ld_aux=N, sAux=(Bi * M * N, M * N),
                 res=res.to(dtype).to(DEV), ld_res=N, sRes=(Bi * M * N, M * N))
        out.append((f"gemm[{dtype}] batched+KB+bias+gelu+res", err(C, ref), tol))
        out.append((f"gemm[{dtype}] aux(pre-activation)", err(aux, pre), tol))
        # epi 2: multiply by gelu'(aux)
        u = q(gen(M, N, seed=7), dtype)
        A2, B2 = q(gen(M, K, seed=8), dtype), q(gen(N, K, seed=9), dtype)
        ud = u.double().requires_grad_(True)
        gp = torch.autograd.grad(TF.gelu(ud).sum(), ud)[0]
        ref2 = (A2.double() @ B2.double().t()) * gp
        C = torch.empty(M, N, dtype=dtype, device=DEV)
        ops.gemm(A2.to(dtype).to(DEV), B2.to(dtype).to(DEV), C, M, N, K, lda=K, ldb=K, ldc=N, epi=2,
                 aux=u.to(dtype).to(DEV), ld_aux=N)
        out.append((f"gemm[{dtype}] epi=gelu'", err(C, ref2), tol))
        # overlapping rows == strided conv1d over a channel-last activation
        Bb, Tin, Cin, Cout, k, s = 2, 41, 16, 24, 3, 2
        x = q(gen(Bb, Tin, Cin, seed=10), dtype)
        w = q(gen(Cout, Cin, k, seed=11, scale=0.2), dtype)
        refc = TF.conv1d(x.double().transpose(1, 2), w.double(), stride=s).transpose(1, 2)
        Tout = refc.shape[1]
        Wf = w.permute(0, 2, 1).reshape(Cout, k * Cin).contiguous()
        y = torch.empty(Bb, Tout, Cout, dtype=dtype, device=DEV)
        ops.gemm(x.to(dtype).to(DEV), Wf.to(dtype).to(DEV), y, Tout, Cout, k * Cin, lda=s * Cin, ldb=k * Cin, ldc=Cout,
                 batch=(Bb, 1), sA=(Tin * Cin, 0), sC=(Tout * Cout, 0))
        out.append((f"gemm[{dtype}] overlapping-row conv1d k3 s2", err(y, refc), tol))
    return out


def check_gemm_pp(variant=3, name="gemm_pp"):
    """256x256 (variant 3) / 192x384 (variant 4) ping-pong kernels: all four operand layouts, ragged M/N edges, K tails
    (zero-page path), K batches with a tail in every batch, split-K, and the fused epilogues."""
    out = []
    dtype, tol = torch.bfloat16, TOLBF
    ops.gemm_set_variant(variant)
    try:
        cases = [  # M, N, K, tA, tB, KB, split
            (600, 520, 256, 0, 0, 1, 1), (600, 520, 200, 0, 0, 1, 1), (1000, 296, 1000, 0, 1, 1, 1),
            (512, 256, 777, 1, 1, 1, 1), (264, 392, 333, 1, 0, 1, 1), (520, 264, 150, 1, 1, 3, 1),
            (768, 512, 1400, 1, 1, 2, 3), (300, 260, 128, 0, 0, 1, 2), (2000, 768, 64, 0, 0, 1, 1),
            (256, 128, 64, 0, 1, 1, 1), (776, 1032, 520, 0, 0, 2, 1),
        ]
        for (M, N, K, tA, tB, KB, split) in cases:
            A = q(gen(KB, M, K, seed=31), dtype)
            B = q(gen(KB, N, K, seed=32), dtype)
            ref = torch.einsum("kmc,knc->mn", A.double(), B.double())
            Kp, Mp, Np = (K + 7) // 8 * 8 + 8, (M + 7) // 8 * 8, (N + 7) // 8 * 8
            if tA:
                Ad = torch.full((KB, K, Mp), float("nan")); Ad[:, :, :M] = A.transpose(1, 2); lda, sa = Mp, K * Mp
            else:
                Ad = torch.full((KB, M, Kp), float("nan")); Ad[:, :, :K] = A; lda, sa = Kp, M * Kp
            if tB:
                Bd = torch.full((KB, K, Np), float("nan")); Bd[:, :, :N] = B.transpose(1, 2); ldb, sb = Np, K * Np
            else:
                Bd = torch.full((KB, N, Kp), float("nan")); Bd[:, :, :K] = B; ldb, sb = Kp, N * Kp
            Ad, Bd = Ad.to(dtype).to(DEV), Bd.to(dtype).to(DEV)
            C = torch.full((M, Np), float("nan"), dtype=dtype, device=DEV)
            ops.gemm(Ad, Bd, C, M, N, K, lda=lda, ldb=ldb, ldc=Np, transA=tA, transB=tB, KB=KB, sA_kb=sa, sB_kb=sb,
                     split_k=split)
            out.append((f"{name} {M}x{N}x{K} tA={tA} tB={tB} KB={KB} split={split}", err(C[:, :N], ref), tol))
        # batched + bias + gelu + aux + residual through the ping-pong kernel
        Bo, Bi, M, N, K = 2, 2, 300, 264, 192
        A = q(gen(Bo, Bi, M, K, seed=33), dtype)
        B = q(gen(Bo, Bi, N, K, seed=34), dtype)
        bias = q(gen(Bi, N, seed=35), dtype)
        res = q(gen(Bo, Bi, M, N, seed=36), dtype)
        pre = torch.einsum("oimc,oinc->oimn", A.double(), B.double()) * 0.5 + bias.double()[None, :, None, :]
        ref = TF.gelu(pre) + res.double()
        C = torch.empty(Bo, Bi, M, N, dtype=dtype, device=DEV)
        aux = torch.empty(Bo, Bi, M, N, dtype=dtype, device=DEV)
        ops.gemm(A.to(dtype).to(DEV), B.to(dtype).to(DEV), C, M, N, K, lda=K, ldb=K, ldc=N, batch=(Bo, Bi),
                 sA=(Bi * M * K, M * K), sB=(Bi * N * K, N * K), sC=(Bi * M * N, M * N), alpha=0.5,
                 bias=bias.to(dtype).to(DEV), sBias=(0, N), epi=1, aux=aux, ld_aux=N, sAux=(Bi * M * N, M * N),
                 res=res.to(dtype).to(DEV), ld_res=N, sRes=(Bi * M * N, M * N))
        out.append((f"{name} batched+bias+gelu+res", err(C, ref), tol))
        out.append((f"{name} aux(pre-activation)", err(aux, pre), tol))
        # overlapping rows (strided conv) through the ping-pong kernel
        Bb, Tin, Cin, Cout, k, s = 2, 701, 64, 256, 3, 2
        x = q(gen(Bb, Tin, Cin, seed=37), dtype)
        w = q(gen(Cout, Cin, k, seed=38, scale=0.2), dtype)
        refc = TF.conv1d(x.double().transpose(1, 2), w.double(), stride=s).transpose(1, 2)
        Tout = refc.shape[1]
        Wf = w.permute(0, 2, 1).reshape(Cout, k * Cin).contiguous()
        y = torch.empty(Bb, Tout, Cout, dtype=dtype, device=DEV)
        ops.gemm(x.to(dtype).to(DEV), Wf.to(dtype).to(DEV), y, Tout, Cout, k * Cin, lda=s * Cin, ldb=k * Cin, ldc=Cout,
                 batch=(Bb, 1), sA=(Tin * Cin, 0), sC=(Tout * Cout, 0))
        out.append((f"{name} overlapping-row conv1d k3 s2", err(y, refc), tol))
        out += _gemm_conv_forms(name)
    finally:
        ops.gemm_set_variant(0)
    return out


def _gemm_conv_forms(name):
    """The three launch kinds of ConvStackFn (forward, one stride phase of the data gradient, weight gradient), one launch
    each with the addressing the autograd function uses, at B = 2, Cin = Cout = 512, k = 3, s = 2, T_in = 549 (T_out = 274:
    one full 256-row tile plus a ragged one per utterance; fp = bp = 1).  The caller has forced the kernel variant."""
    out = []
    dtype, tol = torch.bfloat16, TOLBF
    Bb, Tin, Cc, k, s = 2, 549, 512, 3, 2
    Tout, J, fp, bp = F._conv_geometry(Tin, k, s)
    Tp = fp + Tout + bp
    x = q(gen(Bb, Tin, Cc, seed=41), dtype)
    w = q(gen(Cc, Cc, k, seed=42, scale=1.0 / math.sqrt(Cc * k)), dtype)
    bias = q(0.1 * gen(Cc, seed=43), dtype)
    du = q(gen(Bb, Tout, Cc, seed=44), dtype)
    gpv = q(0.5 + 0.3 * gen(Bb, Tin, Cc, seed=45), dtype)   # stands for the GELU' of the layer below (epilogue class 4)
    xd = x.to(dtype).to(DEV)
    edge = _edge_rows(Tout)
    nan = float("nan")
    # ---- forward form: overlapping A rows, one batch entry per utterance, bias, table GELU, GELU' to aux
    pre = TF.conv1d(x.double().transpose(1, 2), w.double(), bias.double(), stride=s).transpose(1, 2).contiguous().requires_grad_(True)
    act = TF.gelu(pre)
    gp, = torch.autograd.grad(act.sum(), pre)
    Wf = w.permute(0, 2, 1).reshape(Cc, k * Cc).contiguous()
    y = torch.full((Bb, Tout, Cc), nan, dtype=dtype, device=DEV)
    u = torch.full((Bb, Tout, Cc), nan, dtype=dtype, device=DEV)
    ops.gemm(xd, Wf.to(dtype).to(DEV), y, Tout, Cc, k * Cc, lda=s * Cc, ldb=k * Cc, ldc=Cc, batch=(Bb, 1),
             sA=(Tin * Cc, 0), sC=(Tout * Cc, 0), epi=3, aux=u, ld_aux=Cc, sAux=(Tout * Cc, 0), bias=bias.to(dtype).to(DEV))
    out.append((f"{name} conv forward form (overlap+batch+bias+epi 3) C", err(y, act), tol))
    out.append((f"{name} conv forward form C boundary rows", err(y[:, edge], act[:, edge]), tol))
    out.append((f"{name} conv forward form aux (GELU')", err(u, gp), tol))
    out.append((f"{name} conv forward form aux boundary rows", err(u[:, edge], gp[:, edge]), tol))
    # ---- phase form: both stride phases into one NaN-filled output between guard rows
    P = torch.zeros(Bb, Tp, Cc)
    P[:, fp:fp + Tout] = du
    Pd = P.to(dtype).to(DEV)
    xr = torch.zeros(Bb, Tin, Cc, dtype=torch.float64, requires_grad=True)
    dxr, = torch.autograd.grad(TF.conv1d(xr.transpose(1, 2), w.double(), stride=s), xr, du.double().transpose(1, 2))
    refp = dxr * gpv.double()
    G = 4
    buf = gen(G + Bb * Tin + G, Cc, seed=46).to(dtype).to(DEV)
    buf[G:G + Bb * Tin] = nan
    before = buf.clone()
    inner = buf[G:G + Bb * Tin]
    gpd = gpv.to(dtype).to(DEV)
    for r in range(s):
        Jr = J[r]
        Wb = torch.cat([w[:, :, r + s * (Jr - 1 - jj)].t() for jj in range(Jr)], dim=1).contiguous()   # [Cin, Jr * Cout], newest tap first
        Mr = (Tin - r + s - 1) // s
        ops.gemm(Pd, Wb.to(dtype).to(DEV), inner, Mr, Cc, Jr * Cc, lda=Cc, ldb=Jr * Cc, ldc=s * Cc, batch=(Bb, 1),
                 a_off=(fp - Jr + 1) * Cc, sA=(Tp * Cc, 0), c_off=r * Cc, sC=(Tin * Cc, 0), epi=4, aux=gpd, aux_off=r * Cc,
                 ld_aux=s * Cc, sAux=(Tin * Cc, 0))
    got = inner.view(Bb, Tin, Cc)
    out.append((f"{name} conv phase form (a_off+c_off+strided C+epi 4) all rows", err(got, refp), tol))
    for r in range(s):
        out.append((f"{name} conv phase form rows of phase {r}", err(got[:, r::s], refp[:, r::s]), tol))
    edge_in = _edge_rows(Tin)
    out.append((f"{name} conv phase form boundary rows", err(got[:, edge_in], refp[:, edge_in]), tol))
    for nm, sl in (("before", slice(0, G)), ("after", slice(G + Bb * Tin, None))):
        same = torch.equal(buf[sl].view(torch.int16), before[sl].view(torch.int16))
        out.append((f"{name} conv phase form guard rows {nm} the output untouched", 0.0 if same else 1.0, 0.0))
    # ---- weight-gradient form: both operands K-strided, overlapping rows in B, one K batch per utterance with a K tail
    # in each (274 = 4 * 64 + 18), a_off past the front pad; the pad rows lie outside [0, K) and are poisoned
    Pn = torch.full((Bb, Tp, Cc), nan)
    Pn[:, fp:fp + Tout] = du
    Pnd = Pn.to(dtype).to(DEV)
    refw = torch.einsum("bto,btck->okc", du.double(), x.double().unfold(1, k, s)).reshape(Cc, k * Cc)
    for split in (1, 3):
        dWf = torch.full((Cc, k * Cc), nan, dtype=dtype, device=DEV)
        ops.gemm(Pnd, xd, dWf, Cc, k * Cc, Tout, lda=Cc, ldb=s * Cc, ldc=k * Cc, transA=True, transB=True, a_off=fp * Cc,
                 KB=Bb, sA_kb=Tp * Cc, sB_kb=Tin * Cc, split_k=split)
        out.append((f"{name} conv weight-gradient form (tA+tB+overlap+KB+a_off) split={split}", err(dWf, refw), tol))
    return out


def check_gemm_pp3():
    return check_gemm_pp(4, "gemm_pp3")


def check_gemm_w4():
    """the four-wave 256 x 256 kernel (csrc/gemm_w4.hip, variant 5: 128 x 128 accumulators per wave, fragment reads
    software-pipelined between the MFMAs) on the same cases as the eight-wave kernel it shares its LDS image with, plus the
    fused column sums / GELU' epilogue and the grouped launch"""
    out = check_gemm_pp(5, "gemm_w4")
    ops.gemm_set_variant(5)
    try:
        out += [("[w4] " + n, e, t) for n, e, t in check_gemm_colsum()]
    finally:
        ops.gemm_set_variant(0)
    return out


def check_gemm_race():
    """the same ping-pong launch repeated gives bit-identical output (an LDS hazard between the asynchronous operand DMA
    and the fragment reads would show as run-to-run differences); step-sized shapes, both tile shapes, split-K"""
    out = []
    n = 32 * 749
    for name, M, N, K, tA, tB, split in [("192x384 NN", n, 2304, 768, 0, 0, 1), ("256x256 NN", n, 2048, 768, 0, 0, 1),
                                          ("256x256 TT split 7", 3072, 768, n, 1, 1, 7), ("192x384 NT", n, 768, 3072, 0, 1, 1)]:
        A = q(gen(*((K, M) if tA else (M, K)), seed=91), torch.bfloat16).to(torch.bfloat16).to(DEV)
        B = q(gen(*((K, N) if tB else (N, K)), seed=92), torch.bfloat16).to(torch.bfloat16).to(DEV)
        C0, diff = None, 0
        for _ in range(8):
            C = torch.full((M, N), float("nan"), device=DEV, dtype=torch.bfloat16)
            ops.gemm(A, B, C, M, N, K, lda=M if tA else K, ldb=N if tB else K, ldc=N, transA=tA, transB=tB, split_k=split)
            if C0 is None:
                C0 = C
            else:
                diff += int((C.view(torch.int16) != C0.view(torch.int16)).sum().item())
        out.append((f"gemm_race {name} {M}x{N}x{K}: differing elements over 8 launches", float(diff), 0.0))
    return out


def check_gemm_grouped():
    """wavlm_gemm_grouped: weight gradients of several linears over the same rows in one grouped split-K launch,
    accumulated into existing (non-zero) outputs; ragged rows (K tail), ragged M/N tiles, 2-4 members; plus a group the
    256-wide kernel does not take (sequential fall-back inside the library)."""
    out = []
    dtype, tol = torch.bfloat16, TOLBF
    # (n = 5003 with the Base shapes, n = 9000 with ragged tiles: balanced launches -- main workgroups + tail workgroups, see
    #  gemm_common.hpp: gemm_sk_plan; the others: the one-round split)
    for n, shapes in [(1000, [(520, 264), (256, 768)]), (2500, [(2304, 768), (768, 768), (3072, 768), (768, 3072)]),
                      (5003, [(2304, 768), (768, 768), (3072, 768), (768, 3072)]), (9000, [(2000, 1032), (1288, 1032)]),
                      (777, [(264, 392), (512, 256), (304, 520)]), (300, [(64, 48), (96, 64)])]:
        items, refs = [], []
        for k, (N, K) in enumerate(shapes):
            dy, x = q(gen(n, N, seed=50 + k), dtype), q(gen(n, K, seed=60 + k), dtype)
            o0 = q(gen(N, K, seed=70 + k), dtype)
            refs.append(o0.double() + dy.double().t() @ x.double())
            items.append((dy.to(dtype).to(DEV), x.to(dtype).to(DEV), o0.to(dtype).to(DEV).clone()))
        ops.gemm_wgrad_grouped(items, dtype)
        for k, ((N, K), it, ref) in enumerate(zip(shapes, items, refs)):
            out.append((f"gemm_grouped n={n} member {k} [{N}x{K}]", err(it[2], ref), tol))
    return out


# --------------------------------------------------------------------------------------------------- row ops
def check_layernorm():
    out = []
    for dtype in (torch.float32, torch.bfloat16):
        tol = tol_for(dtype)
        for D in (64, 512, 768, 1024):
            rows = 37
            x, r = q(gen(rows, D, seed=1), dtype), q(gen(rows, D, seed=2), dtype)
            g, b = q(1 + 0.1 * gen(D, seed=3), dtype), q(0.1 * gen(D, seed=4), dtype)
            dy = q(gen(rows, D, seed=5), dtype)
            for act in (0, 1):
                xr, rr, gr, br = [t.clone().requires_grad_(True) for t in (x, r, g, b)]
                s = xr + rr
                if dtype == torch.bfloat16:
                    s = s + (s.detach().to(dtype).float() - s.detach())  # straight-through bf16 rounding of the sum
                z = TF.layer_norm(s, (D,), gr, br, 1e-5)
                yr = TF.gelu(z) if act else z
                (yr * dy).sum().backward()
                xd, rd, gd, bd = [t.to(dtype).to(DEV).requires_grad_(True) for t in (x, r, g, b)]
                y, s_out = F.LayerNormFn.apply(xd, rd, gd, bd, 1e-5, act, 0.0, 0, 0.0, 0, 1.0)
                y.backward(dy.to(dtype).to(DEV))
                tag = f"layernorm[{dtype}] D={D} act={act}"
                out.append((tag + " y", err(y, yr), tol))
                out.append((tag + " s", err(s_out, s), tol))
                out.append((tag + " dx", err(xd.grad, xr.grad), tol))
                out.append((tag + " dr", err(rd.grad, rr.grad), tol))
                out.append((tag + " dgamma", err(gd.grad, gr.grad), tol * 2))
                out.append((tag + " dbeta", err(bd.grad, br.grad), tol * 2))
        # dropout consistency: y(p) on kept elements == y(0)/(1-p); grads use the same mask
        D, rows, p = 768, 64, 0.25
        x = gen(rows, D, seed=1).to(dtype).to(DEV).requires_grad_(True)
        r = gen(rows, D, seed=2).to(dtype).to(DEV).requires_grad_(True)
        g = torch.ones(D, dtype=dtype, device=DEV, requires_grad=True)
        b = torch.zeros(D, dtype=dtype, device=DEV, requires_grad=True)
        y0, _ = F.LayerNormFn.apply(x, None, g, b, 1e-5, 0, 0.0, 0, 0.0, 0, 1.0)
        yp, _ = F.LayerNormFn.apply(x, None, g, b, 1e-5, 0, 0.0, 0, p, 777, 1.0)
        keep = (yp != 0)
        frac = keep.float().mean().item()
        out.append((f"layernorm[{dtype}] out-dropout keep fraction", abs(frac - (1 - p)), 0.02))
        out.append((f"layernorm[{dtype}] out-dropout values", err(yp[keep], (y0 / (1 - p))[keep]), tol))
        yp.backward(torch.ones_like(yp))
        # in-dropout: s - x must be r/(1-p) on kept elements, and dr must carry the same mask
        y2, s2 = F.LayerNormFn.apply(x.detach(), r, g, b, 1e-5, 0, p, 999, 0.0, 0, 1.0)
        dlt = (s2.float() - x.detach().float())
        keep2 = dlt.abs() > 1e-6
        out.append((f"layernorm[{dtype}] in-dropout keep fraction", abs(keep2.float().mean().item() - (1 - p)), 0.02))
        y2.backward(gen(rows, D, seed=9).to(dtype).to(DEV))
        out.append((f"layernorm[{dtype}] in-dropout grad mask", float(((r.grad != 0) != keep2).float().mean().item()), 0.01))
        # by-product of the backward pass: column sums of dr (the bias gradient of the linear that produced r), fresh
        # and accumulated into existing tensors, against an explicit column sum of the dr the same call returned
        dyb = gen(rows, D, seed=19).to(dtype).to(DEV)
        _y, sv, mean, rstd = ops.layernorm_fwd(x.detach(), r.detach(), g.detach(), b.detach(), 1e-5, act=0, p_in=p, seed_in=999,
                                               p_out=0.0, seed_out=0, save=True)
        for p_in in (p, 0.0):
            dx_, dr_, _, _, cs = ops.layernorm_bwd(dyb, sv, mean, rstd, g.detach(), b.detach(), p_in=p_in, seed_in=999,
                                                   need_dr=p_in > 0, dr_colsum=True)
            want = (dr_ if dr_ is not None else dx_).double().sum(0)
            out.append((f"layernorm[{dtype}] dr colsum by-product (p_in={p_in})", err(cs, want), tol * 4))
        dg0 = gen(D, seed=21).to(dtype).to(DEV)
        dg, db_, dc = dg0.clone(), dg0.clone(), dg0.clone()
        dx_, dr_, _, _, _ = ops.layernorm_bwd(dyb, sv, mean, rstd, g.detach(), b.detach(), p_in=p, seed_in=999, need_dr=True,
                                              dgamma=dg, dbeta=db_, dr_colsum=dc)
        out.append((f"layernorm[{dtype}] dr colsum accumulated", err(dc, dg0.double() + dr_.double().sum(0)), tol * 4))
        # residual-stream gradient added inside the backward kernel (pre-LN blocks): dx gains dx_add, dr / colsum do not
        extra = gen(rows, D, seed=23).to(dtype).to(DEV)
        dx0, dr0, _, _, cs0 = ops.layernorm_bwd(dyb, sv, mean, rstd, g.detach(), b.detach(), p_in=p, seed_in=999,
                                                need_dr=True, dr_colsum=True)
        dx1, dr1, _, _, cs1 = ops.layernorm_bwd(dyb, sv, mean, rstd, g.detach(), b.detach(), p_in=p, seed_in=999,
                                                need_dr=True, dr_colsum=True, dx_add=extra)
        out.append((f"layernorm[{dtype}] dx_add", err(dx1, dx0.double() + extra.double()), tol))
        # (same values; the two template instantiations may contract the fp32 expression differently: last-bit slack)
        out.append((f"layernorm[{dtype}] dx_add leaves dr", err(dr1, dr0), 1e-6 if dtype == torch.float32 else 0.0))
        out.append((f"layernorm[{dtype}] dx_add leaves colsum", err(cs1, cs0), tol))
        # the same through autograd: y = LN(x) + x with x handed through as an alias
        xa = gen(rows, D, seed=31).to(dtype).to(DEV).requires_grad_(True)
        ya, _s, xal = F.LayerNormFn.apply(xa, None, g.detach(), b.detach(), 1e-5, 0, 0.0, 0, 0.0, 0, 1.0, None, True)
        (ya.float() * dyb.float() + xal.float() * extra.float()).sum().backward()
        xb = xa.detach().clone().requires_grad_(True)
        yb, _s = F.LayerNormFn.apply(xb, None, g.detach(), b.detach(), 1e-5, 0, 0.0, 0, 0.0, 0, 1.0)
        (yb.float() * dyb.float() + xb.float() * extra.float()).sum().backward()
        out.append((f"layernorm[{dtype}] pass_x autograd", err(xa.grad, xb.grad), tol))
    return out


def check_rowops():
    out = []
    for dtype in (torch.float32, torch.bfloat16):
        tol = tol_for(dtype)
        rows, D = 301, 768
        x = q(gen(rows, D, seed=1), dtype)
        xd = x.to(dtype).to(DEV)
        inc = (torch.arange(rows) % 3 == 0)
        exc = (torch.arange(rows) % 5 == 0)
        cs = ops.colsum(xd, torch.float32)
        out.append((f"colsum[{dtype}]", err(cs, x.double().sum(0)), tol))
        cs2 = ops.colsum(xd, torch.float32, include=inc.to(torch.uint8).to(DEV), exclude=exc.to(torch.uint8).to(DEV))
        out.append((f"colsum[{dtype}] masked", err(cs2, x.double()[inc & ~exc].sum(0)), tol))
        emb = q(gen(D, seed=2), dtype)
        y = ops.select_rows(xd, inc.to(torch.uint8).to(DEV), emb.to(dtype).to(DEV), exc.to(torch.uint8).to(DEV))
        ref = x.clone(); ref[inc] = emb; ref[exc] = 0
        out.append((f"select_rows[{dtype}]", err(y, ref), 1e-6))
        idx = torch.tensor([5, -1, 0, 300, 17], dtype=torch.int32)
        gth = ops.gather_rows(xd, idx.to(DEV), 5)
        ref = torch.stack([x[5], torch.zeros(D), x[0], x[300], x[17]])
        out.append((f"gather_rows[{dtype}]", err(gth, ref), 1e-6))
        yv = q(gen(rows, D, seed=3), dtype)
        yd = yv.to(dtype).to(DEV)
        ops.axpby_(yd, xd, 0.5, 2.0)
        out.append((f"axpby[{dtype}]", err(yd, 0.5 * x + 2.0 * yv), tol))
        d1 = ops.dropout(xd, 0.1, 42)
        d2 = ops.dropout(xd, 0.1, 42)
        keep = d1 != 0
        out.append((f"dropout[{dtype}] deterministic", float((d1 != d2).float().mean().item()), 0.0))
        out.append((f"dropout[{dtype}] keep fraction", abs(keep.float().mean().item() - 0.9), 0.01))
        out.append((f"dropout[{dtype}] scale", err(d1[keep], (xd.float() / 0.9)[keep]), tol))
        ss = ops.sumsq(xd, 0.25)
        out.append((f"sumsq[{dtype}]", err(ss, (x.double() ** 2).sum().reshape(1) * 0.25), tol))
        sc = torch.tensor([3.0], device=DEV)
        z = xd.clone(); ops.scale_dev_(z, sc, 0.5)
        out.append((f"scale_dev[{dtype}]", err(z, x * 1.5), tol))
    lr = gen(1000, seed=4).to(DEV)
    out.append(("sum_f32", err(ops.sum_f32(lr), lr.double().sum().reshape(1)), 1e-5))
    return out


# ----------------------------------------------------------------------------------------------------- conv0
def check_conv0():
    out = []
    for dtype in (torch.float32, torch.bfloat16):
        tol = tol_for(dtype)
        for (B, T, C) in [(2, 16000, 512), (3, 4005, 32)]:
            wav = q(gen(B, T, seed=1), dtype)
            W = q(gen(C, 1, 10, seed=2, scale=0.4), dtype)
            g, b = q(1 + 0.1 * gen(C, seed=3), dtype), q(0.1 * gen(C, seed=4), dtype)
            wr, Wr, gr, br = wav.clone(), W.clone().requires_grad_(True), g.clone().requires_grad_(True), b.clone().requires_grad_(True)
            y = TF.gelu(TF.group_norm(TF.conv1d(wr.unsqueeze(1), Wr, stride=5), C, gr, br, 1e-5)).transpose(1, 2)
            dy = q(gen(*y.shape, seed=5), dtype)
            (y * dy).sum().backward()
            Wd, gd, bd = [t.to(dtype).to(DEV).requires_grad_(True) for t in (W, g, b)]
            yd = F.Conv0Fn.apply(wav.to(dtype).to(DEV), Wd, gd, bd, 5, 1e-5, dtype)
            yd.backward(dy.to(dtype).to(DEV))
            tag = f"conv0[{dtype}] B={B} T={T} C={C}"
            out.append((tag + " y", err(yd, y), tol))
            out.append((tag + " dW", err(Wd.grad, Wr.grad), tol * 3))
            out.append((tag + " dgamma", err(gd.grad, gr.grad), tol * 3))
            out.append((tag + " dbeta", err(bd.grad, br.grad), tol * 3))
            # extractor_mode "layer_norm": conv0 -> LayerNorm over channels -> GELU
            Wr2, gr2, br2 = W.clone().requires_grad_(True), g.clone().requires_grad_(True), b.clone().requires_grad_(True)
            y2 = TF.gelu(TF.layer_norm(TF.conv1d(wav.unsqueeze(1), Wr2, stride=5).transpose(1, 2), (C,), gr2, br2, 1e-5))
            (y2 * dy).sum().backward()
            Wd, gd, bd = [t.to(dtype).to(DEV).requires_grad_(True) for t in (W, g, b)]
            yd = F.Conv0LNFn.apply(wav.to(dtype).to(DEV), Wd, gd, bd, 5, 1e-5, dtype)
            yd.backward(dy.to(dtype).to(DEV))
            tag = f"conv0+LN[{dtype}] B={B} T={T} C={C}"
            out.append((tag + " y", err(yd, y2), tol))
            out.append((tag + " dW", err(Wd.grad, Wr2.grad), tol * 3))
            out.append((tag + " dgamma", err(gd.grad, gr2.grad), tol * 3))
            out.append((tag + " dbeta", err(bd.grad, br2.grad), tol * 3))
    # other strides through the GroupNorm-mode kernels (the waveform segment a workgroup stages grows with the stride)
    for st, T in ((8, 33000), (3, 9000)):
        dtype, C, B = torch.bfloat16, 512, 2
        wav = q(gen(B, T, seed=21), dtype)
        W = q(gen(C, 1, 10, seed=22, scale=0.4), dtype)
        g, b = q(1 + 0.1 * gen(C, seed=23), dtype), q(0.1 * gen(C, seed=24), dtype)
        ts = [t.double().clone().requires_grad_(True) for t in (W, g, b)]
        y = TF.gelu(TF.group_norm(TF.conv1d(wav.double().unsqueeze(1), ts[0], stride=st), C, ts[1], ts[2], 1e-5)).transpose(1, 2)
        dy = q(gen(*y.shape, seed=25), dtype)
        gr = torch.autograd.grad(y, ts, dy.double())
        Wd, gd, bd = [t.to(dtype).to(DEV).requires_grad_(True) for t in (W, g, b)]
        yd = F.Conv0Fn.apply(wav.to(dtype).to(DEV), Wd, gd, bd, st, 1e-5, dtype)
        yd.backward(dy.to(dtype).to(DEV))
        tag = f"conv0[{dtype}] stride={st} T={T}"
        out.append((tag + " y", err(yd, y), TOLBF))
        for nm, a, r in zip(("dW", "dgamma", "dbeta"), (Wd.grad, gd.grad, bd.grad), gr):
            out.append((tag + " " + nm, err(a, r), TOLBF * 3))
    return out


def check_conv0_ln():
    """extractor_mode 'layer_norm' block 0 at the width of the real models (C = 512: with bf16 operands the backward runs on the
    matrix cores, conv0_bwd_mfma.hip) with conv bias, ragged chunk ends (512 frames per workgroup, 32 per tile), fewer frames
    than one tile, a bias that moves the frame mean away from zero, and feature_grad_mult-style scaling."""
    out = []
    C = 512
    for dtype in (torch.bfloat16, torch.float32):
        tol = tol_for(dtype)
        for (B, T, boff, gs, st) in [(2, 16000, 0.0, 1.0, 5), (1, 400, 0.0, 1.0, 5), (3, 2565, 0.5, 0.1, 5), (1, 5175, -1.0, 1.0, 5),
                                     (2, 95, 0.0, 1.0, 5), (2, 4106, 0.0, 1.0, 8), (1, 3001, 0.2, 1.0, 3), (2, 10, 0.0, 1.0, 5)]:
            if dtype == torch.float32 and T > 3000:
                continue
            wav = q(gen(B, T, seed=1), dtype)
            W = q(gen(C, 1, 10, seed=2, scale=0.4), dtype)
            g, b = q(1 + 0.1 * gen(C, seed=3), dtype), q(0.1 * gen(C, seed=4), dtype)
            cb = q(boff + 0.2 * gen(C, seed=6), dtype)
            ts = [t.double().clone().requires_grad_(True) for t in (W, g, b, cb)]
            y = TF.gelu(TF.layer_norm(TF.conv1d(wav.double().unsqueeze(1), ts[0], ts[3], stride=st).transpose(1, 2), (C,), ts[1], ts[2], 1e-5))
            dy = q(gen(*y.shape, seed=5), dtype)
            gr = torch.autograd.grad(y, ts, dy.double() * gs)
            Wd, gd, bd, cd = [t.to(dtype).to(DEV) for t in (W, g, b, cb)]
            wd = wav.to(dtype).to(DEV)
            yd = ops.conv0_ln_gelu_fwd(wd, Wd, gd, bd, st, 1e-5, dtype, bias=cd)
            dW, dg, db, dcb = ops.conv0_ln_gelu_bwd(wd, Wd, gd, bd, dy.to(dtype).to(DEV), st, 1e-5, gscale=gs, bias=cd)
            tag = f"conv0+LN+bias[{dtype}] B={B} T={T} off={boff} stride={st}"
            out.append((tag + " y", err(yd, y), tol))
            out.append((tag + " dW", err(dW, gr[0]), tol))
            out.append((tag + " dgamma", err(dg, gr[1]), tol))
            out.append((tag + " dbeta", err(db, gr[2]), tol))
            out.append((tag + " dbias", err(dcb, gr[3]), tol))
    # batch linearity at a size where a workgroup of the matrix-core form walks two chunks (64 rows x 8 chunks = 512 chunks on
    # 256 CUs) and one where it walks one (32 x 8): the gradients of the whole batch are the sums over its two halves
    B, T = 64, 4000 * 5 + 5
    wd = gen(B, T, seed=11).to(torch.bfloat16).to(DEV)
    Wd = gen(C, 1, 10, seed=12, scale=0.4).to(torch.bfloat16).to(DEV)
    gd, bd, cd = [(o + 0.1 * gen(C, seed=13 + i)).to(torch.bfloat16).to(DEV) for i, o in enumerate((1.0, 0.0, 0.3))]
    dy = torch.randn(B, 4000, C, generator=torch.Generator(device=DEV).manual_seed(7), device=DEV).to(torch.bfloat16)
    full = ops.conv0_ln_gelu_bwd(wd, Wd, gd, bd, dy, 5, 1e-5, bias=cd)
    ha = ops.conv0_ln_gelu_bwd(wd[:32].contiguous(), Wd, gd, bd, dy[:32].contiguous(), 5, 1e-5, bias=cd)
    hb = ops.conv0_ln_gelu_bwd(wd[32:].contiguous(), Wd, gd, bd, dy[32:].contiguous(), 5, 1e-5, bias=cd)
    for nm, f, a, b2 in zip(("dW", "dgamma", "dbeta", "dbias"), full, ha, hb):
        out.append((f"conv0+LN batch linearity {nm}", err(f, a.float() + b2.float()), 1e-2))
    return out


def check_conv_ln_block():
    """A conv block of the layer_norm extractor mode (conv -> LayerNorm over channels -> GELU, WavLM/WavLM.py:403-418) at the real
    width: the LayerNorm's backward writes its input gradient straight into the zero-padded layout the conv's backward reads
    (LayerNormFn grad_pad / wavlm_layernorm_bwd_seg).  Against the fp64 reference, and bit-identical to the path with the padded
    copy (ops.LN_SEG_OK = False)."""
    out = []
    C = 512
    dtype = torch.bfloat16
    for (B, T_in, k, s_) in [(3, 101, 3, 2), (2, 64, 2, 2), (2, 37, 3, 2), (1, 200, 2, 2)]:
        x = q(gen(B, T_in, C, seed=1), dtype)
        W = q(gen(C, C, k, seed=2, scale=1.0 / math.sqrt(C * k)), dtype)
        cb = q(0.1 * gen(C, seed=3), dtype)
        g, b = q(1 + 0.1 * gen(C, seed=4), dtype), q(0.1 * gen(C, seed=5), dtype)
        ts = [t.double().clone().requires_grad_(True) for t in (x, W, cb, g, b)]
        yr = TF.gelu(TF.layer_norm(TF.conv1d(ts[0].transpose(1, 2), ts[1], ts[2], stride=s_).transpose(1, 2), (C,), ts[3], ts[4], 1e-5))
        dy = q(gen(*yr.shape, seed=6), dtype)
        gr = torch.autograd.grad(yr, ts, dy.double())
        res = {}
        for seg in (True, False):
            saved = ops.LN_SEG_OK
            ops.LN_SEG_OK = seg
            try:
                td = [t.to(dtype).to(DEV).requires_grad_(True) for t in (x, W, cb, g, b)]
                v = F.ConvStackFn.apply(td[0], ((k, s_),), False, td[1], td[2])
                y, _ = F.layer_norm(v, td[3], td[4], 1e-5, act=1, grad_pad=F.conv_grad_pad(T_in, k, s_))
                res[seg] = (y,) + torch.autograd.grad(y, td, dy.to(dtype).to(DEV))
            finally:
                ops.LN_SEG_OK = saved
        tag = f"conv+LN block B={B} T={T_in} k={k} s={s_}"
        out.append((tag + " y", err(res[True][0], yr), TOLBF))
        for nm, a, r in zip(("dx", "dW", "dbias", "dgamma", "dbeta"), res[True][1:], gr):
            out.append((tag + " " + nm, err(a, r), TOLBF))
        for nm, a, c in zip(("y", "dx", "dW", "dbias", "dgamma", "dbeta"), res[True], res[False]):
            out.append((tag + " " + nm + " == the padded-copy path", 0.0 if torch.equal(a, c) else 1.0, 0.0))
    return out


def check_convstack():
    out = []
    for dtype in (torch.float32, torch.bfloat16):
        tol = tol_for(dtype)
        B, T0, C = 2, 403, 32
        specs = ((3, 2), (3, 2), (2, 2), (2, 2))
        x = q(gen(B, T0, C, seed=1), dtype)
        Ws = [q(gen(C, C, k, seed=10 + i, scale=1.0 / math.sqrt(C * k)), dtype) for i, (k, s) in enumerate(specs)]
        xr = x.clone().requires_grad_(True)
        Wr = [w.clone().requires_grad_(True) for w in Ws]
        h = xr.transpose(1, 2)
        for (k, s), w in zip(specs, Wr):
            h = TF.gelu(TF.conv1d(h, w, stride=s))
        yr = h.transpose(1, 2)
        dy = q(gen(*yr.shape, seed=5), dtype)
        (yr * dy).sum().backward()
        xd = x.to(dtype).to(DEV).requires_grad_(True)
        Wd = [w.to(dtype).to(DEV).requires_grad_(True) for w in Ws]
        yd = F.ConvStackFn.apply(xd, specs, True, *Wd)
        yd.backward(dy.to(dtype).to(DEV))
        tag = f"convstack[{dtype}]"
        out.append((tag + " y", err(yd, yr), tol))
        out.append((tag + " dx", err(xd.grad, xr.grad), tol * 2))
        for i in range(len(specs)):
            out.append((tag + f" dW{i}", err(Wd[i].grad, Wr[i].grad), tol * 2))
    return out


# ---- the conv stack at production width: every launch of every layer on the 256 x 256 / 192 x 384 / four-wave tile kernels
CONV_WIDE_C = 512
CONV_WIDE_VARIANTS = (0, 3, 4, 5)   # ops.gemm_set_variant: automatic, 256 x 256 ping-pong, 192 x 384, four-wave 256 x 256
CONVSTACK_WIDE_CASES = [  # B, T0, specs, also in fp32, conv bias, x.requires_grad
    (3, 1101, ((3, 2), (3, 2)), True, False, True),           # odd T_in twice (1101 -> 550 -> 274); dW0 split 3, dW1 split 1
    (2, 1100, ((3, 2), (2, 2)), False, False, True),          # even T_in into (3,2); odd T_in (549) into (2,2): bp = 1, fp = 0
    (2, 1047, ((2, 2), (2, 2)), True, False, True),           # odd, odd (1047 -> 523 -> 261): the trailing frame is unused
    (2, 1048, ((2, 2), (2, 2)), False, False, True),          # fpp = bpp = 0: the hand-off buffer without a fill
    (2, 2203, ((3, 2), (3, 2), (2, 2)), False, False, True),  # the padded hand-off twice, with different (fp, bp)
    (2, 513, ((3, 2),), False, False, True),                  # T_out = 256 exactly; phase rows 257 / 256
    (2, 512, ((2, 2),), False, False, True),                  # T_out = 256; both phases exactly one tile
    (3, 1101, ((3, 2), (3, 2)), False, True, True),           # bias in the forward epilogue; dbias = column sums over the padded buffer
    (2, 1100, ((3, 2), (2, 2)), False, False, False),         # no dx: the early exit at layer 0, dW still right
]


def _edge_rows(T):
    """the first two and the last two frames of an utterance"""
    return sorted({0, 1, T - 2, T - 1})


def conv_launch_shapes(T0, specs, C):
    """(name, M, N, K, both operands K-strided) of every GEMM ConvStackFn launches for a stack of C -> C layers over T0
    frames: forward, weight gradient and one data-gradient launch per stride phase of every layer"""
    shapes = []
    T_in = T0
    for i, (k, s) in enumerate(specs):
        T_out, J, _, _ = F._conv_geometry(T_in, k, s)
        shapes.append((f"forward {i}", T_out, C, k * C, False))
        shapes.append((f"dW{i}", C, k * C, T_out, True))
        for r in range(s):
            shapes.append((f"dx{i} phase {r}", (T_in - r + s - 1) // s, C, J[r] * C, False))
        T_in = T_out
    return shapes


def conv_shape_guard(T0, specs, C):
    """number of launches a forced tile kernel would hand back to the generic kernel without a word (gemm_pp_ok /
    gemm_pp3_ok: M >= 256 resp. 192, N >= 128 resp. 192, K >= 64, 8-element rows)"""
    return float(sum(1 for (_, M, N, K, tr) in conv_launch_shapes(T0, specs, C)
                     if M < 256 or N < 192 or K < 64 or ((M % 8 or N % 8) if tr else K % 8)))


def unused_trailing_frames(T_in, k, s):
    """frames at the end of an utterance that no window of a (k, s) convolution covers: their gradient is exactly 0"""
    return T_in - (s * ((T_in - k) // s) + k)


def convstack_wide_inputs(case, dtype):
    B, T0, specs, _, bias, _ = case
    C = CONV_WIDE_C
    x = q(gen(B, T0, C, seed=1), dtype)
    Ws = [q(gen(C, C, k, seed=10 + i, scale=1.0 / math.sqrt(C * k)), dtype) for i, (k, s) in enumerate(specs)]
    bs = [q(0.1 * gen(C, seed=20 + i), dtype) for i in range(len(specs))] if bias else []
    T = T0
    for (k, s) in specs:
        T = (T - k) // s + 1
    dy = q(gen(B, T, C, seed=5), dtype)
    return x, Ws, bs, dy


def convstack_wide_ref(inputs, specs, need_dx=True, round_dtype=None):
    """conv1d -> gelu per layer in float64 with nothing rounded in between; autograd for dx, every dW and dbias.  Returns
    {"y", "dx" (if need_dx), "dW0".., "dbias0"..}.
    round_dtype: the pre-activation u and the activation of every layer are rounded through that dtype (straight-through)
    -- the two approximations a bf16 device path has and the exact reference lacks (tests/test_convstack_ref.py)."""
    x, Ws, bs, dy = inputs

    def rnd(t):
        return t if round_dtype is None else t + (t.detach().to(round_dtype).double() - t.detach())

    xr = x.double().requires_grad_(need_dx)
    Wr = [w.double().requires_grad_(True) for w in Ws]
    br = [b.double().requires_grad_(True) for b in bs]
    h = xr.transpose(1, 2)
    for i, (k, s) in enumerate(specs):
        h = rnd(TF.gelu(rnd(TF.conv1d(h, Wr[i], br[i] if br else None, stride=s))))
    yr = h.transpose(1, 2)
    names = (["dx"] if need_dx else []) + [f"dW{i}" for i in range(len(Wr))] + [f"dbias{i}" for i in range(len(br))]
    grads = torch.autograd.grad(yr, ([xr] if need_dx else []) + Wr + br, dy.double())
    res = {"y": yr.detach()}
    res.update(zip(names, grads))
    return res


def conv_compare(tag, got, ref, T_tail, tol, out):
    """results of one device run against the reference: every tensor on its own scale (y at tol, gradients at twice that);
    y and dx also on the scale of the first / last two frames of every utterance alone, so that a wrong edge frame cannot
    hide behind the tensor-wide maximum; dx of the frames no window covers (T_tail of them) exactly 0"""
    for nm, r in ref.items():
        t = tol if nm == "y" else 2 * tol
        out.append((f"{tag} {nm}", err(got[nm], r), t))
        if nm in ("y", "dx"):
            rows = _edge_rows(r.shape[1])
            out.append((f"{tag} {nm} boundary rows", err(got[nm][:, rows], r[:, rows]), t))
    if T_tail > 0 and "dx" in ref:
        out.append((f"{tag} dx unused trailing frame == 0", float((got["dx"][:, -T_tail:] != 0).sum().item()), 0.0))


def _poison(nbytes):
    """NaN into the memory the next torch.empty calls will be handed: the caching allocator has nothing free but the blocks
    filled here (one for the large pool, one for the small), so a row a kernel fails to write reads as NaN, never as a lucky 0"""
    torch.cuda.empty_cache()
    for n in (int(nbytes), 1 << 20):
        t = torch.full((n // 2,), float("nan"), dtype=torch.bfloat16, device=DEV)
        del t


def _poison_reaches_empty(nbytes):
    _poison(nbytes)
    t = torch.empty((int(nbytes) // 8,), dtype=torch.bfloat16, device=DEV)
    s = torch.empty((1024,), dtype=torch.bfloat16, device=DEV)
    ok = bool(t.isnan().all().item()) and bool(s.isnan().all().item())
    return ("poisoned allocations: torch.empty hands out the NaN-filled memory", 0.0 if ok else 1.0, 0.0)


def _convstack_wide_device(case, dtype, inputs):
    B, T0, specs, _, _, need_dx = case
    x, Ws, bs, dy = inputs
    xd = x.to(dtype).to(DEV).requires_grad_(need_dx)
    Wd = [w.to(dtype).to(DEV).requires_grad_(True) for w in Ws]
    bd = [b.to(dtype).to(DEV).requires_grad_(True) for b in bs]
    dyd = dy.to(dtype).to(DEV)
    nbytes = 8 * x.numel() * xd.element_size() + (16 << 20)   # several times all temporaries of the forward or the backward
    _poison(nbytes)
    yd = F.ConvStackFn.apply(xd, specs, True, *Wd, *bd)
    _poison(nbytes)
    grads = torch.autograd.grad(yd, ([xd] if need_dx else []) + Wd + bd, dyd)
    names = (["dx"] if need_dx else []) + [f"dW{i}" for i in range(len(Wd))] + [f"dbias{i}" for i in range(len(bd))]
    res = {"y": yd.detach()}
    res.update(zip(names, grads))
    return res


def check_convstack_wide():
    """ConvStackFn at C = 512 and more than 256 frames out of the last layer, so that every forward, stride-phase and
    weight-gradient launch is taken by the tile kernels production runs (DESIGN.md kernel table), against float64 conv1d ->
    gelu: bf16 under the automatic dispatch and each forced tile kernel, two cases also in fp32 (gemm_f32.hip addresses the
    same way).  Tolerances are check_convstack's; tests/test_convstack_ref.py shows what the reference's side of them is."""
    out = [_poison_reaches_empty(64 << 20)]
    try:
        for case in CONVSTACK_WIDE_CASES:
            B, T0, specs, also_f32, bias, need_dx = case
            name = f"B={B} T0={T0} {'+'.join(f'({k},{s})' for k, s in specs)}" + (" bias" if bias else "") + ("" if need_dx else " no-dx")
            out.append((f"convstack_wide {name}: launches below the tile kernels' shapes", conv_shape_guard(T0, specs, CONV_WIDE_C), 0.0))
            tail = unused_trailing_frames(T0, *specs[0])
            for dtype in (torch.bfloat16,) + ((torch.float32,) if also_f32 else ()):
                inputs = convstack_wide_inputs(case, dtype)
                ref = convstack_wide_ref(inputs, specs, need_dx)
                for v in (CONV_WIDE_VARIANTS if dtype == torch.bfloat16 else (0,)):
                    ops.gemm_set_variant(v)
                    got = _convstack_wide_device(case, dtype, inputs)
                    conv_compare(f"convstack_wide[{dtype}] {name} variant {v}", got, ref, tail, tol_for(dtype), out)
    finally:
        ops.gemm_set_variant(0)
    return out


CONV_LN_WIDE_CASES = [(3, 1101, 3, 2), (2, 1046, 2, 2), (2, 1047, 2, 2), (2, 513, 3, 2)]   # B, T_in, k, s


def check_conv_ln_block_wide():
    """check_conv_ln_block (conv with bias -> LayerNorm over channels -> GELU, the LayerNorm's backward writing straight into
    the conv's zero-padded gradient layout) at sizes the tile kernels take, under every kernel variant, into poisoned
    allocations: more rows than one block of the LayerNorm grid handles, and the hand-off of the padded gradient with
    ragged 256-row tiles behind it."""
    out = [_poison_reaches_empty(64 << 20)]
    C, dtype = CONV_WIDE_C, torch.bfloat16
    saved = ops.LN_SEG_OK
    try:
        for (B, T_in, k, s_) in CONV_LN_WIDE_CASES:
            tag0 = f"conv+LN block wide B={B} T={T_in} k={k} s={s_}"
            out.append((f"{tag0}: launches below the tile kernels' shapes", conv_shape_guard(T_in, ((k, s_),), C), 0.0))
            x = q(gen(B, T_in, C, seed=1), dtype)
            W = q(gen(C, C, k, seed=2, scale=1.0 / math.sqrt(C * k)), dtype)
            cb = q(0.1 * gen(C, seed=3), dtype)
            g, b = q(1 + 0.1 * gen(C, seed=4), dtype), q(0.1 * gen(C, seed=5), dtype)
            ts = [t.double().clone().requires_grad_(True) for t in (x, W, cb, g, b)]
            yr = TF.gelu(TF.layer_norm(TF.conv1d(ts[0].transpose(1, 2), ts[1], ts[2], stride=s_).transpose(1, 2), (C,), ts[3], ts[4], 1e-5))
            dy = q(gen(*yr.shape, seed=6), dtype)
            gr = torch.autograd.grad(yr, ts, dy.double())
            rows = _edge_rows(T_in)
            tail = unused_trailing_frames(T_in, k, s_)
            nbytes = 8 * x.numel() * 2 + (16 << 20)
            for v in CONV_WIDE_VARIANTS:
                ops.gemm_set_variant(v)
                res = {}
                for seg in (True, False):
                    ops.LN_SEG_OK = seg
                    td = [t.to(dtype).to(DEV).requires_grad_(True) for t in (x, W, cb, g, b)]
                    dyd = dy.to(dtype).to(DEV)
                    _poison(nbytes)
                    u = F.ConvStackFn.apply(td[0], ((k, s_),), False, td[1], td[2])
                    y, _ = F.layer_norm(u, td[3], td[4], 1e-5, act=1, grad_pad=F.conv_grad_pad(T_in, k, s_))
                    _poison(nbytes)
                    res[seg] = (y,) + torch.autograd.grad(y, td, dyd)
                tag = f"{tag0} variant {v}"
                out.append((tag + " y", err(res[True][0], yr), TOLBF))
                for nm, a, r in zip(("dx", "dW", "dbias", "dgamma", "dbeta"), res[True][1:], gr):
                    out.append((tag + " " + nm, err(a, r), TOLBF))
                out.append((tag + " dx boundary rows", err(res[True][1][:, rows], gr[0][:, rows]), TOLBF))
                if tail > 0:
                    out.append((tag + " dx unused trailing frame == 0", float((res[True][1][:, -tail:] != 0).sum().item()), 0.0))
                for nm, a, c in zip(("y", "dx", "dW", "dbias", "dgamma", "dbeta"), res[True], res[False]):
                    out.append((tag + " " + nm + " == the padded-copy path", 0.0 if torch.equal(a, c) else 1.0, 0.0))
    finally:
        ops.LN_SEG_OK = saved
        ops.gemm_set_variant(0)
    return out


# -------------------------------------------------------------------------------------------------- attention
def _ref_attention(qkv, gate, tab, kpm, H, scale):
    B, T, D3 = qkv.shape
    D = D3 // 3
    hd = D // H
    qh = qkv[..., :D].view(B, T, H, hd).permute(0, 2, 1, 3)
    kh = qkv[..., D:2 * D].view(B, T, H, hd).permute(0, 2, 1, 3)
    vh = qkv[..., 2 * D:].view(B, T, H, hd).permute(0, 2, 1, 3)
    s = (qh @ kh.transpose(-1, -2)) * scale
    if tab is not None:
        i = torch.arange(T, device=qkv.device)[:, None]   # (the reference runs where its inputs live: CPU or device)
        j = torch.arange(T, device=qkv.device)[None, :]
        rel = tab[:, (j - i) + T - 1]  # [H, T, T]
        s = s + gate.unsqueeze(-1) * rel.unsqueeze(0)
    if kpm is not None:
        s = s.masked_fill(kpm.bool()[:, None, None, :], float("-inf"))
    p = torch.softmax(s, dim=-1)
    return (p @ vh).permute(0, 2, 1, 3).reshape(B, T, D)


def check_attention():
    out = []
    for dtype in (torch.float32, torch.bfloat16):
        tol = tol_for(dtype)
        for (B, T, H, hd, use_pad) in [(2, 49, 2, 32, False), (2, 131, 4, 64, True)]:
            D = H * hd
            qkv = q(gen(B, T, 3 * D, seed=1), dtype)
            gate = 1 + 0.5 * gen(B, H, T, seed=2)
            tab = 0.5 * gen(H, 2 * T - 1, seed=3)
            kpm = None
            if use_pad:
                kpm = torch.zeros(B, T, dtype=torch.uint8)
                kpm[1, T - 20:] = 1
            dO = q(gen(B, T, D, seed=4), dtype)
            qr, gr, tr = qkv.clone().double().requires_grad_(True), gate.clone().double().requires_grad_(True), tab.clone().double().requires_grad_(True)
            Or = _ref_attention(qr, gr, tr, kpm, H, hd ** -0.5)
            (Or * dO.double()).sum().backward()
            qd = qkv.to(dtype).to(DEV).requires_grad_(True)
            gd = gate.to(DEV).requires_grad_(True)
            td = tab.to(DEV).requires_grad_(True)
            kd = kpm.to(DEV) if kpm is not None else None
            Od = F.AttnCoreFn.apply(qd, gd, td, kd, H, hd ** -0.5, 0.0, 0)
            Od.backward(dO.to(dtype).to(DEV))
            tag = f"attn[{dtype}] B={B} T={T} H={H} hd={hd} pad={use_pad}"
            out.append((tag + " O", err(Od, Or), tol))
            out.append((tag + " dqkv", err(qd.grad, qr.grad), tol * 2))
            out.append((tag + " dgate", err(gd.grad, gr.grad), tol * 2))
            out.append((tag + " dtab", err(td.grad, tr.grad), tol * 2))
        # no-bias path
        B, T, H, hd = 1, 40, 2, 32
        qkv = q(gen(B, T, 3 * H * hd, seed=7), dtype)
        Or = _ref_attention(qkv.double(), None, None, None, H, hd ** -0.5)
        Od = F.AttnCoreFn.apply(qkv.to(dtype).to(DEV), None, None, None, H, hd ** -0.5, 0.0, 0)
        out.append((f"attn[{dtype}] no bias O", err(Od, Or), tol))
    # fused kernels (bf16, head_dim 64) at the real frame count, with padding, vs the fp64 reference
    # (1, 999, 16): WavLM-Large's frame count and head count (20 s utterances); (2, 1000, 2, 'ragged'): a full-length row next
    # to one with 63 valid frames (937 padded keys: whole key tiles masked, dead query rows in the same block)
    for (B, T, H, use_pad) in [(2, 749, 3, True), (1, 300, 2, False), (1, 999, 16, False), (2, 1000, 2, 'ragged')]:
        hd, D, dtype, tol = 64, 64 * H, torch.bfloat16, TOLBF
        qkv = q(gen(B, T, 3 * D, seed=11), dtype)
        gate = 1 + 0.5 * gen(B, H, T, seed=12)
        tab = 0.5 * gen(H, 2 * T - 1, seed=13)
        kpm = None
        if use_pad:
            kpm = torch.zeros(B, T, dtype=torch.uint8)
            kpm[1, (63 if use_pad == 'ragged' else T - 100):] = 1
        dO = q(gen(B, T, D, seed=14), dtype)
        qr, gr, tr = qkv.double().requires_grad_(True), gate.double().requires_grad_(True), tab.double().requires_grad_(True)
        Or = _ref_attention(qr, gr, tr, kpm, H, hd ** -0.5)
        (Or * dO.double()).sum().backward()
        qd = qkv.to(dtype).to(DEV).requires_grad_(True)
        gd, td = gate.to(DEV).requires_grad_(True), tab.to(DEV).requires_grad_(True)
        kd = kpm.to(DEV) if kpm is not None else None
        # fused with stored probabilities (WAVLM_ATTN_STORE_P=1), with recomputation (=0, the default), with stored dropout bits
        # (=bits; no dropout here: nothing is stored), unfused composition
        for fused, store in ((True, True), (True, False), (True, "bits"), (False, False)):
            F.USE_FUSED_ATTENTION = fused
            F.ATTN_STORE_P = store
            for t in (qd, gd, td):
                t.grad = None
            Od = F.AttnCoreFn.apply(qd, gd, td, kd, H, hd ** -0.5, 0.0, 0)
            Od.backward(dO.to(dtype).to(DEV))
            tag = f"attn[{('fused, stored bits' if store == 'bits' else 'fused, stored P' if store else 'fused, recompute') if fused else 'unfused'} bf16] B={B} T={T} H={H} pad={use_pad}"
            out.append((tag + " O", err(Od, Or), tol))
            out.append((tag + " dqkv", err(qd.grad, qr.grad), tol * 2))
            out.append((tag + " dgate", err(gd.grad, gr.grad), tol * 2))
            out.append((tag + " dtab", err(td.grad, tr.grad), tol * 2))
        F.USE_FUSED_ATTENTION = True
        F.ATTN_STORE_P = ATTN_STORE_P_DEFAULT
    # fused dropout: deterministic per seed, keep fraction, and forward/backward agree on the mask
    B, T, H, hd = 1, 256, 2, 64
    D = H * hd
    qkv = (0.5 * gen(B, T, 3 * D, seed=21)).to(torch.bfloat16).to(DEV)
    ones_v = qkv.clone()
    ones_v[..., 2 * D:] = 1.0  # V = 1 -> O = sum_j P_drop = (kept mass) / (1 - p)
    O1 = F.AttnCoreFn.apply(ones_v, None, None, None, H, hd ** -0.5, 0.25, 77)
    O2 = F.AttnCoreFn.apply(ones_v, None, None, None, H, hd ** -0.5, 0.25, 77)
    O3 = F.AttnCoreFn.apply(ones_v, None, None, None, H, hd ** -0.5, 0.25, 78)
    out.append(("attn[fused] dropout deterministic", float((O1 != O2).float().mean().item()), 0.0))
    out.append(("attn[fused] dropout seed changes mask", 0.0 if (O1 != O3).any().item() else 1.0, 0.0))
    out.append(("attn[fused] dropout E[kept mass] ~ 1", abs(O1.float().mean().item() - 1.0), 0.02))
    # (forward / backward mask agreement and the numerics under dropout: check_dropout_exact -- exact, not statistical)
    # gate
    # (3, 64): 16-byte fast path with idle lanes, even row count; (12, 64) x 67 rows: Base geometry, odd row count (half
    # step at the end); (2, 32): generic kernel
    for dtype, (B, T, H, hd) in [(dt_, g_) for dt_ in (torch.float32, torch.bfloat16)
                                 for g_ in ((2, 33, 3, 64), (1, 67, 12, 64), (2, 19, 2, 32), (3, 41, 16, 64), (2, 3001, 12, 64))]:
        tol = tol_for(dtype)
        x = q(gen(B, T, H * hd, seed=1), dtype)
        W, b = q(0.2 * gen(8, hd, seed=2), dtype), q(0.1 * gen(8, seed=3), dtype)
        a = q(1 + 0.1 * gen(1, H, 1, 1, seed=4), dtype)
        xr, Wr, br, ar = [t.clone().requires_grad_(True) for t in (x, W, b, a)]
        ql = xr.view(B, T, H, hd).permute(0, 2, 1, 3)
        ga, gb = torch.sigmoid(TF.linear(ql, Wr, br).view(B, H, T, 2, 4).sum(-1)).chunk(2, dim=-1)
        gr = (ga * (gb * ar - 1.0) + 2.0).squeeze(-1)
        dg = gen(B, H, T, seed=5)
        (gr * dg).sum().backward()
        xd, Wd, bd, ad = [t.to(dtype).to(DEV).requires_grad_(True) for t in (x, W, b, a)]
        gdv = F.GateFn.apply(xd, Wd, bd, ad, H)
        gdv.backward(dg.to(DEV))
        tag = f"gate[{dtype}] H={H} hd={hd} rows={B * T}"
        out.append((tag + " gate", err(gdv, gr), tol))
        out.append((tag + " dx", err(xd.grad, xr.grad), tol * 2))
        out.append((tag + " dW", err(Wd.grad, Wr.grad), tol * 2))
        out.append((tag + " dbias", err(bd.grad, br.grad), tol * 2))
        out.append((tag + " dgrep_a", err(ad.grad, ar.grad), tol * 2))
        if hd == 64:  # accumulate form: the gate's gradient of x is added into a buffer that already holds another consumer's
            base = q(gen(B, T, H * hd, seed=6), dtype)
            acc = base.to(dtype).to(DEV).clone()
            _, ga_d, gb_d = ops.gate_fwd(xd.detach(), Wd.detach(), bd.detach(), ad.detach().view(-1), H)
            dx2, _, _, _ = ops.gate_bwd(dg.to(DEV), xd.detach(), Wd.detach(), bd.detach(), ad.detach().view(-1), ga_d, gb_d, H,
                                        dx_accumulate=acc)
            out.append((tag + " dx (accumulate)", err(dx2, xr.grad + base), tol * 2))
    # relpos table
    emb = gen(32, 4, seed=1).requires_grad_(True)
    bucket = torch.randint(0, 32, (97,), generator=torch.Generator().manual_seed(0)).to(torch.int32)
    tr = emb[bucket.long()].t()
    dt_ = gen(4, 97, seed=2)
    (tr * dt_).sum().backward()
    ed = emb.detach().to(DEV).requires_grad_(True)
    td = F.RelPosTableFn.apply(ed, bucket.to(DEV))
    td.backward(dt_.to(DEV))
    out.append(("relpos table", err(td, tr), 1e-6))
    out.append(("relpos table grad", err(ed.grad, emb.grad), 1e-5))
    return out


# ------------------------------------------------------------------------------------------- exact dropout parity
def _attn_kernel_masks(B, H, T, p_drop, seed, gate, tab, kpm, qseed=41, store_p=False):
    """The keep mask each of the three fused attention kernels ACTUALLY applies, read out of the kernels' own results
    (no debug entry point, no re-implementation of the hash): bool [B, H, T, T] (query, key) each.
      forward   V = one-hot over a 64-key chunk  ->  O[i, u] = P_drop[i, j0 + u]: kept iff non-zero;
      dK/dV     dO = one-hot over a 64-query chunk  ->  dV[j, u] = P_drop[i0 + u, j]: kept iff non-zero;
      dQ        K = one-hot over a 64-key chunk, V = dO = e_0 (so dP = 1 everywhere)  ->  dQ[i, u] = scale * dS[i, j0 + u]
                with dS = P sc (keep - kappa_i), kappa_i = kept probability mass of row i in (0, 1): kept iff positive.
    Padded keys (P = 0) carry no information and are reported as False by all three."""
    hd = 64
    D = H * hd
    scale = hd ** -0.5
    qv = (0.5 * gen(B, T, D, seed=qseed)).to(torch.bfloat16).to(DEV)
    kv = (0.5 * gen(B, T, D, seed=qseed + 1)).to(torch.bfloat16).to(DEV)
    keep_f = torch.zeros(B, H, T, T, dtype=torch.bool)
    keep_q = torch.zeros(B, H, T, T, dtype=torch.bool)
    keep_kv = torch.zeros(B, H, T, T, dtype=torch.bool)
    hsel = torch.arange(H, device=DEV) * hd
    for c0 in range(0, T, 64):
        n = min(64, T - c0)
        u = torch.arange(n, device=DEV)
        onehot = torch.zeros(B, T, D, dtype=torch.bfloat16, device=DEV)
        for h in range(H):
            onehot[:, c0 + u, h * hd + u] = 1.0
        # forward: V one-hot on the key chunk
        qkv = torch.cat([qv, kv, onehot], dim=-1).contiguous()
        O, lse, _ = ops.attn_fused_fwd(qkv, gate, tab, kpm, H, scale, p_drop, seed, store_p=store_p)
        keep_f[:, :, :, c0:c0 + n] = (O.view(B, T, H, hd)[..., :n] != 0).permute(0, 2, 1, 3).cpu()
        # dK/dV: dO one-hot on the query chunk (any V)
        qkv2 = torch.cat([qv, kv, kv], dim=-1).contiguous()
        O2, lse2, ps2 = ops.attn_fused_fwd(qkv2, gate, tab, kpm, H, scale, p_drop, seed, store_p=store_p)
        dqkv, _, _ = ops.attn_fused_bwd(qkv2, O2, onehot, lse2, gate, tab, kpm, H, scale, p_drop, seed, pstore=ps2)
        dV = dqkv[..., 2 * D:].view(B, T, H, hd)[..., :n]                       # [b, j, h, u] = P_drop[i0 + u, j]
        keep_kv[:, :, c0:c0 + n, :] = (dV != 0).permute(0, 2, 3, 1).cpu()
        # dQ: K one-hot on the key chunk, V = dO = e_0
        e0 = torch.zeros(B, T, D, dtype=torch.bfloat16, device=DEV)
        e0[..., hsel] = 1.0
        qkv3 = torch.cat([qv, onehot, e0], dim=-1).contiguous()
        O3, lse3, ps3 = ops.attn_fused_fwd(qkv3, gate, tab, kpm, H, scale, p_drop, seed, store_p=store_p)
        dqkv3, _, _ = ops.attn_fused_bwd(qkv3, O3, e0, lse3, gate, tab, kpm, H, scale, p_drop, seed, pstore=ps3)
        dQ = dqkv3[..., :D].view(B, T, H, hd)[..., :n]
        keep_q[:, :, :, c0:c0 + n] = (dQ > 0).permute(0, 2, 1, 3).cpu()
    if kpm is not None:
        valid = ~kpm.bool().cpu()[:, None, None, :]
        keep_f, keep_q, keep_kv = keep_f & valid, keep_q & valid, keep_kv & valid
    return keep_f, keep_q, keep_kv


def _ref_attention_masked(qkv, gate, tab, kpm, H, scale, keep, sc):
    """_ref_attention with an explicit dropout keep mask [B, H, T, T] and scale sc = 1 / (1 - p) on the probabilities"""
    B, T, D3 = qkv.shape
    D = D3 // 3
    hd = D // H
    qh = qkv[..., :D].view(B, T, H, hd).permute(0, 2, 1, 3)
    kh = qkv[..., D:2 * D].view(B, T, H, hd).permute(0, 2, 1, 3)
    vh = qkv[..., 2 * D:].view(B, T, H, hd).permute(0, 2, 1, 3)
    s = (qh @ kh.transpose(-1, -2)) * scale
    if tab is not None:
        i = torch.arange(T, device=qkv.device)[:, None]   # (the reference runs where its inputs live: CPU or device)
        j = torch.arange(T, device=qkv.device)[None, :]
        s = s + gate.unsqueeze(-1) * tab[:, (j - i) + T - 1].unsqueeze(0)
    if kpm is not None:
        s = s.masked_fill(kpm.bool()[:, None, None, :], float("-inf"))
    pr = torch.softmax(s, dim=-1) * keep.to(s.dtype) * sc
    return (pr @ vh).permute(0, 2, 1, 3).reshape(B, T, D)


def check_dropout_exact():
    """Dropout-on is the benchmarked mode: its parity must not be statistical.  (1) The keep masks the forward, dQ and dK/dV
    attention kernels apply are read out of the kernels themselves and must be IDENTICAL -- in the recompute mode three kernels
    regenerate the mask independently (the dK/dV one with a different word-sharing scheme), in the stored-probability mode
    (the default) the backward kernels take the decision from the sign bit the forward stored, through two different
    read paths (register fragments / LDS gather + transposing read); and the storing forward must drop exactly what the
    plain forward drops.  (2) With that mask the fused forward and backward
    are compared with the fp64 reference at the usual bf16 tolerance (multihead_attention.py:278-300 with
    dropout_p = attention_dropout).  (3) The same for the dropouts fused into the LayerNorm kernels (residual-branch
    dropout of post- and pre-LN blocks incl. the fused pre-LN residual stream, output dropout) and the dropout-add."""
    out = []
    p_drop = 0.25   # 16384 / 65536: the kernels' 16-bit threshold represents it exactly, sc = 4/3
    sc = 1.0 / (1.0 - p_drop)
    cases = [(1, 2, 256, False, False, 1234567), (2, 2, 200, True, True, 0x9E3779B97F4A7C15), (1, 16, 331, True, False, 77)]
    for (B, H, T, use_tab, use_pad, seed) in cases:
        gate = tab = kpm = None
        if use_tab:
            gate = (1 + 0.5 * gen(B, H, T, seed=2)).to(DEV)
            tab = (0.5 * gen(H, 2 * T - 1, seed=3)).to(DEV)
        if use_pad:
            kpm = torch.zeros(B, T, dtype=torch.uint8)
            kpm[1, T - 37:] = 1
            kpm = kpm.to(DEV)
        kf, kq, kkv = _attn_kernel_masks(B, H, T, p_drop, seed, gate, tab, kpm)
        tag = f"dropout-exact attn B={B} H={H} T={T} tab={use_tab} pad={use_pad}"
        nvalid = float((~kpm.bool().cpu()).float().mean().item()) if kpm is not None else 1.0
        out.append((tag + " keep fraction", abs(kf.float().mean().item() / nvalid - (1 - p_drop)), 0.01))
        out.append((tag + " mask fwd == dQ (mismatching elements)", float((kf != kq).sum().item()), 0.0))
        out.append((tag + " mask fwd == dK/dV (mismatching elements)", float((kf != kkv).sum().item()), 0.0))
        sf, sq, skv = _attn_kernel_masks(B, H, T, p_drop, seed, gate, tab, kpm, store_p=True)
        out.append((tag + " stored P: storing fwd == plain fwd (mismatching elements)", float((sf != kf).sum().item()), 0.0))
        out.append((tag + " stored P: mask fwd == dQ (mismatching elements)", float((sf != sq).sum().item()), 0.0))
        out.append((tag + " stored P: mask fwd == dK/dV (mismatching elements)", float((sf != skv).sum().item()), 0.0))
        # stored dropout BITS (round 6, WAVLM_ATTN_STORE_P=bits): the forward writes its decisions as bit words, the dQ kernel reads them per
        # row (v_bfe_i32 at the forward's bit order), the dK/dV kernel through its per-row LDS arrays (bit of the lane's key)
        bf, bq, bkv = _attn_kernel_masks(B, H, T, p_drop, seed, gate, tab, kpm, store_p="bits")
        out.append((tag + " stored bits: storing fwd == plain fwd (mismatching elements)", float((bf != kf).sum().item()), 0.0))
        out.append((tag + " stored bits: mask fwd == dQ (mismatching elements)", float((bf != bq).sum().item()), 0.0))
        out.append((tag + " stored bits: mask fwd == dK/dV (mismatching elements)", float((bf != bkv).sum().item()), 0.0))
        # (2) numerics with the forward's own mask
        D = 64 * H
        qkv = q(gen(B, T, 3 * D, seed=11), torch.bfloat16)
        dO = q(gen(B, T, D, seed=14), torch.bfloat16)
        gc, tc = (gate.cpu(), tab.cpu()) if use_tab else (None, None)
        qr = qkv.double().requires_grad_(True)
        gr = gc.double().requires_grad_(True) if use_tab else None
        tr = tc.double().requires_grad_(True) if use_tab else None
        Or = _ref_attention_masked(qr, gr, tr, kpm.cpu() if kpm is not None else None, H, 64 ** -0.5, kf, sc)
        (Or * dO.double()).sum().backward()
        for store in (True, False, "bits"):
            F.ATTN_STORE_P = store
            tg2 = tag + (" [stored bits]" if store == "bits" else " [stored P]" if store else " [recompute]")
            qd = qkv.to(torch.bfloat16).to(DEV).requires_grad_(True)
            gd = gate.clone().requires_grad_(True) if use_tab else None
            td = tab.clone().requires_grad_(True) if use_tab else None
            Od = F.AttnCoreFn.apply(qd, gd, td, kpm, H, 64 ** -0.5, p_drop, seed)
            Od.backward(dO.to(torch.bfloat16).to(DEV))
            out.append((tg2 + " O vs fp64 with the kernel's mask", err(Od, Or), TOLBF))
            out.append((tg2 + " dqkv vs fp64 with the kernel's mask", err(qd.grad, qr.grad), TOLBF * 2))
            if use_tab:
                out.append((tg2 + " dgate", err(gd.grad, gr.grad), TOLBF * 2))
                out.append((tg2 + " dtab", err(td.grad, tr.grad), TOLBF * 2))
        F.ATTN_STORE_P = ATTN_STORE_P_DEFAULT
    # (3) LayerNorm-fused dropouts
    for dtype in (torch.float32, torch.bfloat16):
        tol = tol_for(dtype)
        for D in (768, 1024):
            rows, p = 75, 0.25
            x, r = q(gen(rows, D, seed=1), dtype), q(gen(rows, D, seed=2), dtype)
            g, b = q(1 + 0.1 * gen(D, seed=3), dtype), q(0.1 * gen(D, seed=4), dtype)
            dy, ds = q(gen(rows, D, seed=5), dtype), q(gen(rows, D, seed=6), dtype)
            dev = lambda t: t.to(dtype).to(DEV)
            # the forward's residual-dropout mask: x = 0, r = 1  ->  s = keep / (1 - p)
            _, s_probe = F.LayerNormFn.apply(dev(torch.zeros(rows, D)), dev(torch.ones(rows, D)), dev(g), dev(b), 1e-5, 0, p, 4711,
                                             0.0, 0, 1.0)
            keep = (s_probe != 0).cpu()
            tag = f"dropout-exact layernorm[{dtype}] D={D}"
            out.append((tag + " residual-dropout keep fraction", abs(keep.float().mean().item() - (1 - p)), 0.02))
            for s_grad in (False, True):
                xr, rr, gr, br = [t.clone().double().requires_grad_(True) for t in (x, r, g, b)]
                s_ref = xr + rr * keep.double() / (1 - p)
                s_q = s_ref + (s_ref.detach().to(dtype).double() - s_ref.detach())  # the kernel rounds s to `dtype`
                yr = TF.layer_norm(s_q, (D,), gr, br, 1e-5)
                ((yr * dy.double()).sum() + ((s_q * ds.double()).sum() if s_grad else 0.0)).backward()
                xd, rd, gd, bd = [dev(t).requires_grad_(True) for t in (x, r, g, b)]
                res = F.LayerNormFn.apply(xd, rd, gd, bd, 1e-5, 0, p, 4711, 0.0, 0, 1.0, None, False, s_grad)
                y, s_out = res[0], res[1]
                if s_grad:
                    (y.float() * dev(dy).float()).sum().add((s_out.float() * dev(ds).float()).sum()).backward()
                else:
                    y.backward(dev(dy))
                t2 = tag + (" fused residual stream" if s_grad else "")
                out.append((t2 + " backward mask == forward mask (mismatching elements)",
                            float((((rd.grad != 0).cpu() != keep) & (xd.grad != 0).cpu()).sum().item()), 0.0))
                out.append((t2 + " y", err(y, yr), tol))
                out.append((t2 + " dx", err(xd.grad, xr.grad), tol))
                out.append((t2 + " dr", err(rd.grad, rr.grad), tol))
                out.append((t2 + " dgamma", err(gd.grad, gr.grad), tol * 2))
            # output dropout (the encoder's first LayerNorm): mask from the forward, gradient through the same mask
            xd = dev(x).requires_grad_(True)
            yp, _ = F.LayerNormFn.apply(xd, None, dev(g), dev(b), 1e-5, 0, 0.0, 0, p, 999, 1.0)
            keep_o = (yp != 0).cpu()
            yp.backward(dev(dy))
            xr = x.clone().double().requires_grad_(True)
            yr = TF.layer_norm(xr, (D,), g.double(), b.double(), 1e-5) * keep_o.double() / (1 - p)
            (yr * dy.double()).sum().backward()
            out.append((tag + " output-dropout y", err(yp, yr), tol))
            out.append((tag + " output-dropout dx with the forward's mask", err(xd.grad, xr.grad), tol))
        # dropout-add of the unfused pre-LN block: y = x + dropout(r); backward dr = dropout(dy) with the same mask
        from unispeech_amd.wavlm import ResidualAddFn
        rows, D, p = 64, 1024, 0.1
        xz = torch.zeros(rows, D, dtype=dtype, device=DEV)
        r1 = torch.ones(rows, D, dtype=dtype, device=DEV, requires_grad=True)
        ya = ResidualAddFn.apply(xz, r1, p, 31337)
        ya.backward(torch.ones_like(ya))
        out.append((f"dropout-exact dropout_add[{dtype}] backward mask == forward mask",
                    float(((ya != 0) != (r1.grad != 0)).sum().item()), 0.0))
        out.append((f"dropout-exact dropout_add[{dtype}] keep fraction", abs((ya != 0).float().mean().item() - (1 - p)), 0.02))
    return out


# ---------------------------------------------------------------------------------------- pos_conv / FFN / linear
def check_posconv():
    out = []
    for dtype in (torch.float32, torch.bfloat16):
        tol = tol_for(dtype)
        # (.., 768, 128, 16) / (.., 1024, 128, 16) in bf16 run the direct-convolution kernel (Cg = 48 / 64), at one, two
        # frame segments and every tile height; the rest the overlapping-row GEMM form
        cases = [(2, 49, 64, 16, 4), (2, 75, 768, 128, 16)]
        if dtype == torch.bfloat16:
            cases += [(1, 749, 768, 128, 16), (2, 400, 768, 128, 16), (1, 999, 1024, 128, 16), (2, 330, 1024, 128, 16)]
        for (B, T, D, K, G) in cases:
            Cg = D // G
            x = q(gen(B, T, D, seed=1), dtype)
            v = q(gen(D, Cg, K, seed=2, scale=math.sqrt(4.0 / (K * D))), dtype)
            g = q(v.norm(dim=(0, 1), keepdim=True) * (1 + 0.1 * gen(1, 1, K, seed=3)), dtype)
            bias = q(0.1 * gen(D, seed=4), dtype)
            xr, vr, gr, br = [t.clone().requires_grad_(True) for t in (x, v, g, bias)]
            w = gr * vr / vr.norm(dim=(0, 1), keepdim=True)
            yc = TF.conv1d(xr.transpose(1, 2), w, br, padding=K // 2, groups=G)[:, :, :T]
            yr = xr + TF.gelu(yc).transpose(1, 2)
            dy = q(gen(B, T, D, seed=5), dtype)
            (yr * dy).sum().backward()
            xd, vd, gd, bd = [t.to(dtype).to(DEV).requires_grad_(True) for t in (x, v, g, bias)]
            yd = F.PosConvFn.apply(xd, vd, gd, bd, G)
            yd.backward(dy.to(dtype).to(DEV))
            tag = f"posconv[{dtype}] D={D} K={K} G={G}"
            out.append((tag + " y", err(yd, yr), tol))
            out.append((tag + " dx", err(xd.grad, xr.grad), tol * 2))
            out.append((tag + " dv", err(vd.grad, vr.grad), tol * 3))
            out.append((tag + " dg", err(gd.grad, gr.grad), tol * 3))
            out.append((tag + " dbias", err(bd.grad, br.grad), tol * 2))
            if dtype == torch.bfloat16 and ops.posconv_direct_supported(dtype, Cg, K, T):
                # the two activation-side implementations against each other (same bf16 inputs, fp32 accumulation)
                F.POSCONV_DIRECT = False
                try:
                    x2 = xd.detach().clone().requires_grad_(True)
                    v2 = vd.detach().clone().requires_grad_(True)
                    y2 = F.PosConvFn.apply(x2, v2, gd.detach(), bd.detach(), G)
                    y2.backward(dy.to(dtype).to(DEV))
                finally:
                    F.POSCONV_DIRECT = True
                out.append((tag + " direct vs gemm y", err(yd, y2), 1.0e-2))
                out.append((tag + " direct vs gemm dx", err(xd.grad, x2.grad), 1.0e-2))
                out.append((tag + " direct vs gemm dv", err(vd.grad, v2.grad), 1.0e-2))
    return out


def check_gemm_colsum():
    """column sums of C out of the GEMM epilogue (192 x 384 and 256 x 256 ping-pong kernels) and by the fall-back pass
    (128-wide kernel, fp32), against an explicit sum over the rows of the C the same call stored"""
    out = []
    bf = torch.bfloat16
    for (n, N, K, epi, dtype) in [(1000, 3072, 768, 4, bf), (1000, 768, 3072, 0, bf), (777, 2048, 512, 4, bf),
                                  (300, 2048, 512, 0, bf), (500, 48, 256, 0, bf), (300, 256, 128, 0, torch.float32)]:
        # dx[n, K'] = dy[n, N'] @ W[N', K'] in the dX form the model uses (B K-strided); here N plays K'
        dy = q(gen(n, K, seed=1), dtype).to(dtype).to(DEV)
        W = q(gen(K, N, seed=2, scale=1.0 / math.sqrt(K)), dtype).to(dtype).to(DEV)
        aux = q(gen(n, N, seed=3), dtype).to(dtype).to(DEV) if epi == 4 else None
        Cc = torch.empty((n, N), dtype=dtype, device=DEV)
        base = q(gen(N, seed=4), torch.float32).to(DEV)
        cs = base.clone()
        ops.gemm(dy, W, Cc, n, N, K, lda=K, ldb=N, ldc=N, transB=True, epi=epi, aux=aux, ld_aux=N, colsum=cs,
                 colsum_accumulate=True)
        ref = dy.double() @ W.double()
        if epi == 4:
            ref = ref * aux.double()
        tag = f"gemm colsum[{dtype}] n={n} N={N} K={K} epi={epi}"
        out.append((tag + " C", err(Cc, ref), tol_for(dtype)))
        out.append((tag + " colsum vs stored C", err(cs - base, Cc.double().sum(0)), 2e-3 if dtype == bf else 1e-5))
        out.append((tag + " colsum vs exact", err(cs - base, ref.sum(0)), 5e-3 if dtype == bf else 1e-5))
    return out


def check_linear_ffn():
    out = []
    for dtype in (torch.float32, torch.bfloat16):
        tol = tol_for(dtype)
        n, D, Fd = 300, 768, 3072
        x = q(gen(2, n // 2, D, seed=1), dtype)
        W1, b1 = q(0.03 * gen(Fd, D, seed=2), dtype), q(0.1 * gen(Fd, seed=3), dtype)
        W2, b2 = q(0.03 * gen(D, Fd, seed=4), dtype), q(0.1 * gen(D, seed=5), dtype)
        dy = q(gen(2, n // 2, D, seed=6), dtype)
        xr, W1r, b1r, W2r, b2r = [t.clone().requires_grad_(True) for t in (x, W1, b1, W2, b2)]
        yr = TF.linear(TF.gelu(TF.linear(xr, W1r, b1r)), W2r, b2r)
        (yr * dy).sum().backward()
        xd, W1d, b1d, W2d, b2d = [t.to(dtype).to(DEV).requires_grad_(True) for t in (x, W1, b1, W2, b2)]
        yd = F.FFNFn.apply(xd, W1d, b1d, W2d, b2d, 0.0, 0)
        yd.backward(dy.to(dtype).to(DEV))
        tag = f"ffn[{dtype}]"
        for nm, a, b in [("y", yd, yr), ("dx", xd.grad, xr.grad), ("dW1", W1d.grad, W1r.grad), ("db1", b1d.grad, b1r.grad),
                         ("dW2", W2d.grad, W2r.grad), ("db2", b2d.grad, b2r.grad)]:
            out.append((f"{tag} {nm}", err(a, b), tol * (1 if nm == "y" else 2)))
        xr2, Wr2, br2 = x.clone().requires_grad_(True), W1.clone().requires_grad_(True), b1.clone().requires_grad_(True)
        y2 = TF.linear(xr2, Wr2, br2)
        dy2 = q(gen(*y2.shape, seed=7), dtype)
        (y2 * dy2).sum().backward()
        xd2, Wd2, bd2 = [t.to(dtype).to(DEV).requires_grad_(True) for t in (x, W1, b1)]
        yd2 = F.LinearFn.apply(xd2, Wd2, bd2)
        yd2.backward(dy2.to(dtype).to(DEV))
        for nm, a, b in [("y", yd2, y2), ("dx", xd2.grad, xr2.grad), ("dW", Wd2.grad, Wr2.grad), ("db", bd2.grad, br2.grad)]:
            out.append((f"linear[{dtype}] {nm}", err(a, b), tol * (1 if nm == "y" else 2)))
    return out


# ------------------------------------------------------------------------------------------------------- loss
def check_loss():
    from oracle import wavlm_oracle as O
    out = []
    for dtype in (torch.float32, torch.bfloat16):
        tol = tol_for(dtype)
        for (S, V, Fd) in [(57, 23, 32), (700, 504, 256)]:
            proj = q(gen(S, Fd, seed=1), dtype)
            emb = q(torch.rand(V, Fd, generator=torch.Generator().manual_seed(2)), dtype)
            tgt = torch.randint(0, V, (S,), generator=torch.Generator().manual_seed(3))
            pr, er = proj.clone().requires_grad_(True), emb.clone().requires_grad_(True)
            pos = er[tgt]
            negs = er.unsqueeze(1).expand(-1, S, -1)
            logits = O.compute_nce(pr, pos, negs, 0.1)
            lossr = TF.cross_entropy(logits.float(), torch.zeros(S, dtype=torch.long), reduction="sum")
            corr = ((logits.argmax(-1) == 0) & ~(logits.argmin(-1) == 0)).sum()
            (lossr * 1.7).backward()
            pd, ed = proj.to(dtype).to(DEV).requires_grad_(True), emb.to(dtype).to(DEV).requires_grad_(True)
            loss, nc = F.MaskedPredLossFn.apply(pd, ed, tgt.to(torch.int32).to(DEV), 0.1, True)
            (loss * 1.7).sum().backward()
            tag = f"loss[{dtype}] S={S} V={V}"
            out.append((tag + " loss", err(loss, lossr.reshape(1)), tol))
            out.append((tag + " correct", abs(nc.item() - corr.item()), 0.0 if dtype == torch.float32 else max(2.0, 0.02 * S)))
            out.append((tag + " dproj", err(pd.grad, pr.grad), tol * 3))
            out.append((tag + " demb", err(ed.grad, er.grad), tol * 3))
    f = gen(2, 49, 32, seed=1)
    fr = f.clone().requires_grad_(True)
    (fr.pow(2).mean() * 3.0).backward()
    fd = f.to(DEV).requires_grad_(True)
    pen = F.FeaturesPenFn.apply(fd)
    (pen * 3.0).sum().backward()
    out.append(("features_pen", err(pen, f.pow(2).mean().reshape(1)), 1e-5))
    out.append(("features_pen grad", err(fd.grad, fr.grad), 1e-5))
    # sampled-instance cosine logits + BCE (UniSpeech-SAT utterance-contrastive head): gathered rows, duplicates, the
    # row itself as column 0
    for dtype in (torch.float32, torch.bfloat16):
        tol = tol_for(dtype)
        S, N, C = 301, 9, 256
        y = q(gen(S, C, seed=41), dtype)
        gi = torch.Generator().manual_seed(5)
        idx = torch.cat([torch.arange(S).view(S, 1), torch.randint(0, S, (S, N), generator=gi)], dim=1)
        tg = torch.cat([torch.ones(S, 1, dtype=torch.bool), torch.rand(S, N, generator=gi) < 0.3], dim=1)
        yr = y.clone().double().requires_grad_(True)
        cand = yr[idx.view(-1)].view(S, N + 1, C)
        lg = torch.cosine_similarity(yr.unsqueeze(1), cand, dim=-1) / 0.1
        lr_ = TF.binary_cross_entropy_with_logits(lg, tg.double(), reduction="none").mean()
        lr_.backward()
        yd = y.to(dtype).to(DEV).requires_grad_(True)
        ld, acc = F.UttContrastiveLossFn.apply(yd, idx.to(torch.int32).to(DEV), tg.to(torch.uint8).to(DEV), 0.1)
        ld.sum().backward()
        tag = f"utt_contrastive[{dtype}]"
        out.append((tag + " loss", abs(ld.item() - lr_.item()) / abs(lr_.item()), tol))
        out.append((tag + " accuracy", abs(acc.item() - ((lg >= 0) == tg).double().mean().item()), 1e-6 if dtype == torch.float32 else 0.02))
        out.append((tag + " dproj", err(yd.grad, yr.grad), tol * 3))
    return out



# ------------------------------------------------------------- wav2vec 2.0 / UniSpeech quantised-target head
def argmax_lowest(t):
    """arg-max over the last dimension with the tie rule spelled out: the LOWEST index among the maxima"""
    V = t.shape[-1]
    mx = t.max(-1, keepdim=True).values
    ar = torch.arange(V).expand(t.shape)
    return torch.where(t == mx, ar, torch.full_like(ar, V)).min(-1).values


def prob_perplexity_of(avg_probs):
    """sum over groups of exp(entropy) of avg_probs [G, V] (gumbel_vector_quantizer.py:184-190)"""
    return torch.exp(-torch.sum(avg_probs * torch.log(avg_probs + 1e-7), dim=-1)).sum()


def ref_gumbel_vq(logits, vars_, G, V, tau, training, noise):
    """GumbelVectorQuantizer.forward (src/fairseq/modules/gumbel_vector_quantizer.py:157-213; oracle.gumbel_vq) after the
    weight projection, line by line, in the dtype of its inputs (fp64 in the checks), with the Gumbel draws passed in:
    logits [n, G*V], vars_ [1, G*V, vd], noise [n*G, V] or None (eval).  F.gumbel_softmax(hard=True) is written out as
    y_hard - y_soft.detach() + y_soft, so autograd gives the reference's straight-through gradients.
    Returns (x [n, G*vd], prob_perplexity, code_perplexity, idx [n, G] (code within its group), y_soft [n*G, V] or None)."""
    n = logits.shape[0]
    lg = logits.reshape(n * G, V)
    k = argmax_lowest(lg)
    hard_x = torch.zeros_like(lg).scatter_(-1, k.view(-1, 1), 1.0).view(n, G, V)
    hard_probs = torch.mean(hard_x, dim=0)
    code_ppl = torch.exp(-torch.sum(hard_probs * torch.log(hard_probs + 1e-7), dim=-1)).sum()
    avg_probs = torch.softmax(lg.view(n, G, V), dim=-1).mean(dim=0)
    prob_ppl = prob_perplexity_of(avg_probs)
    y_soft = None
    if training:
        y_soft = torch.softmax((lg + noise) / tau, dim=-1)
        k = argmax_lowest(y_soft)
        y_hard = torch.zeros_like(lg).scatter_(-1, k.view(-1, 1), 1.0)
        y = y_hard - y_soft.detach() + y_soft
    else:
        y = hard_x
    y = y.reshape(n, -1)
    x = (y.unsqueeze(-1) * vars_).view(n, G, V, -1).sum(-2).view(n, -1)
    return x, prob_ppl, code_ppl, k.view(n, G), y_soft


def ref_sampled_negatives(x, y, idx, temp):
    """Wav2Vec2Model.compute_preds (models/wav2vec/wav2vec2.py:533-553) + Wav2vecCriterion with infonce
    (criterions/wav2vec_criterion.py:44-64, 105-113): x [S, C], y [R, C], idx int64 [S, 1 + N] rows of y (column 0 = the
    positive).  neg_is_pos compares the RAW rows of y.  Returns (loss summed, n_correct, logits [S, N + 1])."""
    pos = y[idx[:, 0]]                                   # [S, C]
    negs = y[idx[:, 1:]].permute(1, 0, 2)                # [N, S, C]
    neg_is_pos = (pos == negs).all(-1)                   # [N, S]
    targets = torch.cat([pos.unsqueeze(0), negs], dim=0)
    logits = torch.cosine_similarity(x, targets, dim=-1) / temp
    if neg_is_pos.any():
        logits = torch.cat([logits[:1], logits[1:].masked_fill(neg_is_pos, float("-inf"))], dim=0)
    l2 = logits.transpose(0, 1)                          # [S, N + 1]
    loss = TF.cross_entropy(l2, torch.zeros(l2.size(0), dtype=torch.long), reduction="sum")
    mx, mn = l2.argmax(-1) == 0, l2.argmin(-1) == 0
    n_correct = int(mx.long().sum().item() - (mx & mn).long().sum().item())
    return loss, n_correct, l2


def chi2_quantile(df, tail=1e-6):
    """the chi-square(df) quantile at 1 - tail: scipy when importable, else the Wilson-Hilferty cube"""
    try:
        from scipy.stats import chi2
        return float(chi2.isf(tail, df))
    except ImportError:
        from statistics import NormalDist
        z = NormalDist().inv_cdf(1.0 - tail)
        return df * (1.0 - 2.0 / (9.0 * df) + z * math.sqrt(2.0 / (9.0 * df))) ** 3


def chi2_independence(a, b, K):
    """Pearson statistic of the K x K contingency table of two index vectors against the product of its margins"""
    tab = torch.bincount(a.long() * K + b.long(), minlength=K * K).double().view(K, K)
    exp = tab.sum(1, keepdim=True) * tab.sum(0, keepdim=True) / tab.sum()
    return float(((tab - exp) ** 2 / exp).sum().item())


def seeded_gumbel(rows, V, seed):
    """F.gumbel_softmax's draws (-log of Exp(1) samples), from a generator of their own"""
    g = torch.Generator().manual_seed(seed)
    return -torch.empty((rows, V), dtype=torch.float32).exponential_(generator=g).log()


def vq_near_ties(lg64, noise64, tau):
    """rows [n*G] whose top-two gap of z = (l + g) / tau in fp64 is below 8 * 2^-23 * max|z| of the row: the fp32 rounding
    of the kernel's (l + g) * inv_tau can order those two either way"""
    z = (lg64 + noise64) / tau
    if z.shape[-1] < 2:
        return torch.zeros(z.shape[0], dtype=torch.bool)
    top = z.topk(2, dim=-1).values
    return (top[:, 0] - top[:, 1]) < 8.0 * 2.0 ** -23 * z.abs().max(-1).values


# (G, V, n, seed).  The seeds are ones for which the fp64 reference alone has NO near-tie row (vq_near_ties) in either dtype,
# so that x and dvars, which follow the chosen index, can be compared on every row.
VQ_CASES = [(1, 1, 37, 100), (2, 20, 45, 110), (1, 64, 101, 120), (2, 65, 77, 130), (3, 100, 53, 140), (4, 129, 66, 150),
            (2, 319, 83, 160), (2, 320, 301, 170), (2, 320, 8192 + 37, 180), (4, 320, 4099, 198)]
VQ_TAU = 0.7          # between the schedule's ends (2.0 -> 0.5)
VQ_DIV_WEIGHT = 0.1   # loss_weights[0] of the released wav2vec 2.0 recipes


def vq_case_inputs(G, V, n, dtype, seed):
    """(logits [n, G*V] at scale 3, codebook [1, G*V, vd], Gumbel noise [n*G, V], dx weights [n, G*vd]), rounded through
    dtype where the device holds them in dtype; vd is a multiple of 8 (the GEMM's tested K granule)"""
    vd = 8 if n > 1000 else 16
    return (q(gen(n, G * V, seed=seed, scale=3.0), dtype), q(gen(1, G * V, vd, seed=seed + 1), dtype),
            seeded_gumbel(n * G, V, seed + 2), q(gen(n, G * vd, seed=seed + 3), dtype))


def vq_tie_inputs(dtype, training):
    """rows of a G = 2, V = 320 problem whose maximum appears twice, bit-equal: per row (code a, code b, lowest).  Eval: both
    logits are 9 (exact in bf16).  Training: logits 20 and 21 with noise 1.5 and 0.5, so the SUMS are both 21.5 (exact in
    fp32) while the raw arg-max is the higher code; every other sum stays far below (|l| < 6, Gumbel < 16 never reached)."""
    G, V = 2, 320
    pairs = [(3, 40), (5, 70), (63, 64), (0, V - 1), (130, 131), (191, 192), (64, 256), (17, 273), (255, 256), (127, 128)]
    n = len(pairs)
    logits = q(gen(n, G * V, seed=77, scale=1.0), dtype).view(n, G, V)
    noise = seeded_gumbel(n * G, V, 78).view(n, G, V)
    want = torch.zeros(n, G, dtype=torch.long)
    for r, (lo, hi) in enumerate(pairs):
        for g in range(G):
            if training:   # group 0: the higher raw logit at the higher code; group 1: at the lower code
                big, small = (hi, lo) if g == 0 else (lo, hi)
                logits[r, g, big], noise[r, g, big] = 21.0, 0.5
                logits[r, g, small], noise[r, g, small] = 20.0, 1.5
            else:
                logits[r, g, lo] = logits[r, g, hi] = 9.0
            want[r, g] = lo
    return G, V, logits.reshape(n, G * V).contiguous(), noise.reshape(n * G, V).contiguous(), want


def check_gumbel_vq():
    """csrc/vq.hip + functional.GumbelVQFn against ref_gumbel_vq in fp64 at the released codebook size (V = 320: all five
    lane chunks), every group count, ragged V, row counts beyond one grid pass, both dtypes; the device Gumbel generator's
    law, independence and moments; the API limits.  Tested envelope: V <= 320, G <= 4."""
    from unispeech_amd import _lib
    out = []
    for dtype in (torch.float32, torch.bfloat16):
        tol = tol_for(dtype)
        dn = "fp32" if dtype == torch.float32 else "bf16"
        for (G, V, n, seed) in VQ_CASES:
            tag = f"gumbel_vq[{dn}] G={G} V={V} n={n}"
            logits, vars_, noise, dxw = vq_case_inputs(G, V, n, dtype, seed)
            vd = vars_.shape[-1]
            ld, vdev = logits.to(dtype).to(DEV), vars_.to(dtype).to(DEV)
            goff = torch.arange(G) * V
            div_w = -VQ_DIV_WEIGHT * n / (G * V)     # d criterion / d prob_perplexity: 0.1 * sample_size * (GV - ppl) / GV
            # ---- eval mode: the arg-max does no arithmetic -> exact
            l64 = logits.double().requires_grad_(True)
            v64 = vars_.double().requires_grad_(True)
            xr, pr, cr, kr, _ = ref_gumbel_vq(l64, v64, G, V, VQ_TAU, False, None)
            idx, _, ppl, dA = ops.gumbel_vq_fwd(ld, G, V, VQ_TAU, False)
            kd = idx.cpu().long().view(n, G) - goff
            out.append((tag + " eval idx (mismatches)", float((kd != kr).sum().item()), 0.0))
            le = ld.clone().requires_grad_(True)
            xd, pd, cd = F.GumbelVQFn.apply(le, vdev, G, V, VQ_TAU, False, None, 0)
            pick = vdev.view(G * V, vd)[(kr + goff).view(-1)].view(n, G * vd)
            out.append((tag + " eval x == vars[idx] (differing elements)", float((xd != pick).sum().item()), 0.0))
            out.append((tag + " eval prob_perplexity", err(pd, pr.reshape(1)), tol))
            out.append((tag + " eval code_perplexity", err(cd, cr.reshape(1)), tol))
            out.append((tag + " perplexity pair of the forward call", err(ppl, torch.stack([pr, cr])), tol))
            avg = torch.softmax(logits.double().view(n, G, V), -1).mean(0).requires_grad_(True)
            (dAr,) = torch.autograd.grad(prob_perplexity_of(avg), avg)
            out.append((tag + " dA = d prob_perplexity / d avg_probs", err(dA, dAr.reshape(-1)), tol))
            # backward 2: eval mode, the diversity term alone, at its own scale
            (dl_ref,) = torch.autograd.grad(pr * div_w, l64)
            (dl_dev,) = torch.autograd.grad(pd.sum() * div_w, le)
            out.append((tag + " bwd diversity term alone: dlogits", err(dl_dev, dl_ref), tol * 3))
            # ---- training with host noise
            l64 = logits.double().requires_grad_(True)
            xr, pr, cr, kr, yr = ref_gumbel_vq(l64, v64, G, V, VQ_TAU, True, noise.double())
            nd = noise.to(DEV)
            idx, ys, ppl, dA = ops.gumbel_vq_fwd(ld, G, V, VQ_TAU, True, nd)
            kd = idx.cpu().long().view(n, G) - goff
            near = vq_near_ties(logits.double().view(n * G, V), noise.double(), VQ_TAU)
            nex = int(near.sum().item())
            out.append((tag + " train y_soft", err(ys, yr), TOL32))
            out.append((tag + f" train idx (mismatches outside the {nex} near-tie rows of {n * G})",
                        float(((kd != kr).view(-1) & ~near).sum().item()), 0.0))
            out.append((tag + f" train near-tie rows excluded: {nex} of {n * G} (cap 0.1 %)", nex / (n * G), 1e-3))
            out.append((tag + " train perplexity pair", err(ppl, torch.stack([pr, cr]).detach()), tol))
            # backward 1: the straight-through term alone; backward 3: both, weighted as the criterion does
            lt = ld.clone().requires_grad_(True)
            vt = vdev.clone().requires_grad_(True)
            xd, pd, _ = F.GumbelVQFn.apply(lt, vt, G, V, VQ_TAU, True, nd, 0)
            out.append((tag + " train x", err(xd, xr), tol))
            dxd = dxw.to(dtype).to(DEV)
            g1 = torch.autograd.grad(xd, (lt, vt), dxd, retain_graph=True)
            r1 = torch.autograd.grad((xr * dxw.double()).sum(), (l64, v64), retain_graph=True)
            out.append((tag + " bwd straight-through term alone: dlogits", err(g1[0], r1[0]), tol * 3))
            out.append((tag + " bwd straight-through term alone: dvars", err(g1[1], r1[1]), tol * 3))
            g3 = torch.autograd.grad((xd.float() * dxd.float()).sum() + pd.sum() * div_w, (lt, vt))
            r3 = torch.autograd.grad((xr * dxw.double()).sum() + pr * div_w, (l64, v64))
            out.append((tag + " bwd both terms: dlogits", err(g3[0], r3[0]), tol * 3))
            out.append((tag + " bwd both terms: dvars", err(g3[1], r3[1]), tol * 3))
        # ---- tie rule: the maximum twice, bit-equal -> the lowest index, exactly
        for training in (False, True):
            G, V, logits, noise, want = vq_tie_inputs(dtype, training)
            n = logits.shape[0]
            idx, _, _, _ = ops.gumbel_vq_fwd(logits.to(dtype).to(DEV), G, V, VQ_TAU, training, noise.to(DEV) if training else None)
            kd = idx.cpu().long().view(n, G) - torch.arange(G) * V
            _, _, _, kr, _ = ref_gumbel_vq(logits.double(), torch.zeros(1, G * V, 1).double(), G, V, VQ_TAU, training,
                                           noise.double() if training else None)
            md = "equal logit + noise sums (training)" if training else "equal logits (eval)"
            out.append((f"gumbel_vq[{dn}] ties, {md}: rows not at the lowest index", float((kd != want).sum().item()), 0.0))
            out.append((f"gumbel_vq[{dn}] ties, {md}: reference not at the lowest index", float((kr != want).sum().item()), 0.0))
        # ---- perplexities / dA at the edges: codes with softmax mass ~ 0 that are never chosen (the a -> 0 branch of
        # log(a + 1e-7)), one code taking every row (perplexity ~ 1 per group), one code taken by most rows in training
        G, V, n = 2, 320, 50
        for kind in ("unused block", "one code", "dominant code"):
            logits = gen(n, G, V, seed=301, scale=3.0)
            if kind == "unused block":
                logits[:, :, 100:200] = -30.0
            elif kind == "one code":
                logits[:, 0, 7] = 40.0
                logits[:, 1, 300] = 40.0
            else:
                logits[:, 0, 7] += 12.0
                logits[:, 1, 300] += 12.0
            logits = q(logits.reshape(n, G * V), dtype)
            vars_ = q(gen(1, G * V, 16, seed=302), dtype)
            noise = seeded_gumbel(n * G, V, 303)
            training = kind == "dominant code"
            l64 = logits.double().requires_grad_(True)
            v64 = vars_.double().requires_grad_(True)
            xr, pr, cr, kr, _ = ref_gumbel_vq(l64, v64, G, V, VQ_TAU, training, noise.double() if training else None)
            lt = logits.to(dtype).to(DEV).requires_grad_(True)
            vt = vars_.to(dtype).to(DEV).requires_grad_(True)
            nd = noise.to(DEV) if training else None
            idx, _, ppl, dA = ops.gumbel_vq_fwd(lt.detach(), G, V, VQ_TAU, training, nd)
            xd, pd, cd = F.GumbelVQFn.apply(lt, vt, G, V, VQ_TAU, training, nd, 0)
            avg = torch.softmax(logits.double().view(n, G, V), -1).mean(0).requires_grad_(True)
            (dAr,) = torch.autograd.grad(prob_perplexity_of(avg), avg)
            tag = f"gumbel_vq[{dn}] {kind}"
            cnt = torch.bincount((kr + torch.arange(G) * V).view(-1), minlength=G * V)
            tag += f" (codes never chosen: {int((cnt == 0).sum())}, most chosen: {int(cnt.max())} of {n} rows)"
            out.append((tag + " idx (mismatches)", float((idx.cpu().long().view(n, G) - torch.arange(G) * V != kr).sum().item()), 0.0))
            out.append((tag + " prob_perplexity", err(pd, pr.reshape(1)), tol))
            out.append((tag + " code_perplexity", err(cd, cr.reshape(1)), tol))
            out.append((tag + " dA", err(dA, dAr.reshape(-1)), tol))
            dxw = q(gen(n, G * 16, seed=304), dtype)
            div_w = -VQ_DIV_WEIGHT * n / (G * V)
            gd = torch.autograd.grad((xd.float() * dxw.to(DEV)).sum() + pd.sum() * div_w, (lt, vt))
            gr = torch.autograd.grad((xr * dxw.double()).sum() + pr * div_w, (l64, v64))
            if kind == "one code":
                # eval mode: dlogits is the diversity term alone, gp p_v (dA_v - <p, dA>) with gp = div_w / n.  With p a one-hot
                # to ~1e-17 the bracket cancels to ~1e-13 of |dA|, so any fp32 evaluation (the reference's own fp32 autograd
                # has the same form) carries an absolute error of a few 2^-24 |gp| max|dA| and the tensor's own scale means
                # nothing: the error is taken relative to the terms that cancel, |gp| max|dA|
                scale = abs(div_w) / n * dAr.abs().max().item()
                out.append((tag + " dlogits (relative to |gp| max|dA|, the terms that cancel)",
                            (gd[0].double().cpu() - gr[0]).abs().max().item() / scale, tol * 3))
            else:
                out.append((tag + " dlogits", err(gd[0], gr[0]), tol * 3))
            out.append((tag + " dvars", err(gd[1], gr[1]), tol * 3))
    out += check_gumbel_vq_device_noise()
    # ---- API limits: refused by the entry point (WL_EINVAL through check()), nothing launched
    for nm, (G, V, tau) in (("V = 321", (1, 321, 1.0)), ("G = 5", (5, 8, 1.0)), ("tau = 0", (2, 20, 0.0))):
        lg = torch.zeros(4, G * V, device=DEV)
        for which in ("fwd", "bwd"):
            try:
                if which == "fwd":
                    ops.gumbel_vq_fwd(lg, G, V, tau, True, None, 1)
                else:
                    ops.gumbel_vq_bwd(lg, None, None, torch.zeros(G * V, device=DEV), torch.ones(1, device=DEV), G, V, tau)
                refused = False
            except _lib.WavlmHipError:
                refused = True
            out.append((f"gumbel_vq {which} refuses {nm}", 0.0 if refused else 1.0, 0.0))
    return out


def check_gumbel_vq_device_noise():
    """vq_gumbel (counter hash -> -log(-log u)), the generator training uses by default: reproducible per seed; by the
    Gumbel-max identity P(idx = k) = softmax(l)_k (chi-square against n softmax(l)); independent across consecutive rows and
    across groups (chi-square on 8 x 8 contingency tables); variance and skewness of a Gumbel.  Every threshold is the
    chi-square quantile at 1 - 1e-6 or six standard errors: a correct generator fails one of them about once in 10^5
    seeds, an aliased counter by orders of magnitude."""
    out = []
    G, V, n = 2, 320, 1000
    lg = gen(n, G * V, seed=401, scale=3.0).to(DEV)
    i1, y1, _, _ = ops.gumbel_vq_fwd(lg, G, V, 1.0, True, None, 12345)
    i2, y2, _, _ = ops.gumbel_vq_fwd(lg, G, V, 1.0, True, None, 12345)
    i3, _, _, _ = ops.gumbel_vq_fwd(lg, G, V, 1.0, True, None, 12346)
    out.append(("gumbel_vq device noise: same seed, differing idx", float((i1 != i2).sum().item()), 0.0))
    out.append(("gumbel_vq device noise: same seed, differing y_soft elements", float((y1 != y2).sum().item()), 0.0))
    out.append(("gumbel_vq device noise: other seed, fraction of idx unchanged (< 1/2)", (i1 == i3).float().mean().item(), 0.5))
    # law
    G, V, n = 2, 40, 200000
    perm = torch.randperm(G * V, generator=torch.Generator().manual_seed(402)).view(G, V)
    ell = (2.5 * perm.double() / (G * V - 1)).float()           # fixed, non-uniform, range 2.5: min expected count > 1000
    idx, _, _, _ = ops.gumbel_vq_fwd(ell.view(1, G * V).expand(n, G * V).contiguous().to(DEV), G, V, 1.0, True, None, 20240611)
    k = idx.cpu().long().view(n, G) - torch.arange(G) * V
    thr = chi2_quantile(V - 1)
    for g in range(G):
        expc = n * torch.softmax(ell[g].double(), -1)
        cnt = torch.bincount(k[:, g].clamp(0, V - 1), minlength=V).double()
        out.append((f"gumbel_vq device noise: law, group {g}: chi2({V - 1}) of counts vs n softmax(l) (min expected {expc.min():.0f})",
                    float(((cnt - expc) ** 2 / expc).sum().item()), thr))
    # independence
    G, V = 2, 8
    ell = (1.0 * torch.arange(G * V).double() / (G * V - 1)).float()
    idx, _, _, _ = ops.gumbel_vq_fwd(ell.view(1, G * V).expand(n, G * V).contiguous().to(DEV), G, V, 1.0, True, None, 977)
    k = (idx.cpu().long().view(n, G) - torch.arange(G) * V).clamp(0, V - 1)
    thr = chi2_quantile((V - 1) * (V - 1))
    for g in range(G):
        for par in (0, 1):   # disjoint pairs (row, row + 1) starting at even / odd rows: independent samples of the pair
            a, b = k[par:n - 1:2, g], k[par + 1:n:2, g]
            m = min(a.numel(), b.numel())
            out.append((f"gumbel_vq device noise: independence of rows r, r+1 (group {g}, r = {par} mod 2): chi2(49)",
                        chi2_independence(a[:m], b[:m], V), thr))
    out.append(("gumbel_vq device noise: independence of groups 0, 1 of a row: chi2(49)", chi2_independence(k[:, 0], k[:, 1], V), thr))
    # moments: zero logits, tau = 1 -> log y_soft - row mean = the noise centred within its row
    G, V, n = 2, 320, 2000
    _, ys, _, _ = ops.gumbel_vq_fwd(torch.zeros(n, G * V, device=DEV), G, V, 1.0, True, None, 31337)
    c = ys.double().cpu().log()
    c = c - c.mean(-1, keepdim=True)
    N = c.numel()
    var = float((c ** 2).sum(-1).div(V - 1).mean().item())                       # unbiased under row centring
    m3 = float((c ** 3).mean().item()) / ((1 - 1 / V) * (1 - 2 / V))              # E c^3 = kappa3 (1 - 1/V)(1 - 2/V)
    skew = m3 / var ** 1.5
    # Gumbel cumulants kappa_r = (r - 1)! zeta(r) -> central moments; standard errors of the sample variance and of the
    # sample skewness m3 / m2^1.5 (delta method, influence function a (x^3 - mu3 - 3 mu2 x) - b (x^2 - mu2)) at N samples
    z2, z3, z4, z5, z6 = math.pi ** 2 / 6, 1.2020569031595942, math.pi ** 4 / 90, 1.0369277551433699, math.pi ** 6 / 945
    k2, k3, k4, k5, k6 = z2, 2 * z3, 6 * z4, 24 * z5, 120 * z6
    mu2, mu3, mu4, mu5 = k2, k3, k4 + 3 * k2 ** 2, k5 + 10 * k3 * k2
    mu6 = k6 + 15 * k4 * k2 + 10 * k3 ** 2 + 15 * k2 ** 3
    se_var = math.sqrt((mu4 - mu2 ** 2) / N)
    a, b = mu2 ** -1.5, 1.5 * mu3 * mu2 ** -2.5
    se_skew = math.sqrt((a * a * (mu6 - mu3 ** 2 + 9 * mu2 ** 3 - 6 * mu2 * mu4) - 2 * a * b * (mu5 - 4 * mu2 * mu3)
                         + b * b * (mu4 - mu2 ** 2)) / N)
    out.append((f"gumbel_vq device noise: variance vs pi^2/6 = {mu2:.4f} (margin 6 x {se_var:.2e}, N = {N})", abs(var - mu2), 6 * se_var))
    out.append((f"gumbel_vq device noise: skewness vs {mu3 / mu2 ** 1.5:.4f} (margin 6 x {se_skew:.2e}, N = {N})",
                abs(skew - mu3 / mu2 ** 1.5), 6 * se_skew))
    return out


def sn_near_ties(l2):
    """rows whose fp64 gap between logit 0 and the best other logit is below 8 * 2^-23 * max|logit| (finite entries)"""
    fin = torch.where(torch.isfinite(l2), l2, torch.zeros_like(l2))
    if l2.shape[1] < 2:
        return torch.zeros(l2.shape[0], dtype=torch.bool)
    return (l2[:, 0] - l2[:, 1:].max(-1).values).abs() < 8.0 * 2.0 ** -23 * fin.abs().max(-1).values


def sn_compare(tag, x, y, idx, dtype, out, temp=0.1, skip_rows_x=None, skip_rows_y=None):
    """one SampledNegativesLossFn case against ref_sampled_negatives in fp64: loss, logits (+ exact -inf placement) through a
    direct gather_dot call, dx, dy, n_correct.  skip_rows_*: rows compared on their own (their 1 / eps gradients would
    otherwise set the scale of the whole tensor).  Returns (device logits, reference logits, dx, dy)."""
    tol = tol_for(dtype)
    S = x.shape[0]
    x64, y64 = x.double().requires_grad_(True), y.double().requires_grad_(True)
    lr, ncr, l2 = ref_sampled_negatives(x64, y64, idx, temp)
    gx, gy = torch.autograd.grad(lr, (x64, y64))
    xd, yd = x.to(dtype).to(DEV).requires_grad_(True), y.to(dtype).to(DEV).requires_grad_(True)
    idd = idx.to(torch.int32).to(DEV)
    loss, nc = F.SampledNegativesLossFn.apply(xd, yd, idd, temp)
    dx, dy = torch.autograd.grad(loss.sum(), (xd, yd))
    xn, _ = ops.l2norm_fwd(xd.detach(), dtype)
    yn, _ = ops.l2norm_fwd(yd.detach(), dtype)
    lg = ops.gather_dot(xn, yn, idd, 1.0 / temp, mask_raw=yd.detach()).cpu()
    mref, mdev = torch.isinf(l2) & (l2 < 0), torch.isinf(lg) & (lg < 0)
    zero = torch.zeros(())
    out.append((tag + " loss", err(loss, lr.reshape(1)), tol))
    out.append((tag + f" -inf placement ({int(mref.sum())} masked in the reference; differing positions)", float((mref != mdev).sum().item()), 0.0))
    out.append((tag + " logits", err(torch.where(mdev, zero, lg), torch.where(mref, zero.double(), l2.detach())), tol))
    kx = torch.ones(S, dtype=torch.bool) if skip_rows_x is None else ~skip_rows_x
    ky = torch.ones(y.shape[0], dtype=torch.bool) if skip_rows_y is None else ~skip_rows_y
    out.append((tag + " dx", err(dx.cpu()[kx], gx[kx]), tol * 3))
    out.append((tag + f" dy ({dy.shape[0]} rows)", err(dy.cpu()[ky], gy[ky]), tol * 3))
    if skip_rows_x is not None:
        out.append((tag + " dx, the skipped rows", err(dx.cpu()[~kx], gx[~kx]), tol * 3))
    if skip_rows_y is not None:
        out.append((tag + " dy, the skipped rows", err(dy.cpu()[~ky], gy[~ky]), tol * 3))
    diff = abs(int(round(nc.item())) - ncr)
    if dtype == torch.float32:
        k = int(sn_near_ties(l2.detach()).sum().item())
        out.append((tag + f" n_correct (beyond the {k} near-tie rows)", float(max(0, diff - k)), 0.0))
        out.append((tag + f" near-tie rows: {k} of {S} (cap 0.1 %)", k / S, 1e-3))
    else:
        out.append((tag + " n_correct", float(diff), max(2.0, 0.02 * S)))
    return lg, l2.detach(), dx.cpu(), dy.cpu()


def check_sampled_negatives():
    """functional.SampledNegativesLossFn (l2norm, gather_dot with the neg_is_pos mask, ce_rows, sum_f32, rows_wsum twice,
    l2norm backward) against ref_sampled_negatives in fp64 at the released sizes (final_dim 256 / 768, 100 negatives), every
    float4 lane chunk of gather_dot / rows_wsum (D = 260: first group of chunk 1; D = 1024: the limit), and the index
    patterns of training.  Tested envelope: D <= 1024, D a multiple of 4."""
    out = []
    for dtype in (torch.float32, torch.bfloat16):
        dn = "fp32" if dtype == torch.float32 else "bf16"
        for ci, (S, N, D) in enumerate([(57, 10, 32), (1201, 100, 256), (700, 100, 768), (333, 13, 260), (130, 100, 1024), (5, 1, 4)]):
            x, y = q(gen(S, D, seed=500 + ci), dtype), q(gen(S, D, seed=520 + ci), dtype)
            neg = torch.randint(0, S, (S, N), generator=torch.Generator().manual_seed(540 + ci))
            idx = torch.cat([torch.arange(S).view(S, 1), neg], dim=1)
            sn_compare(f"sampled_negatives[{dn}] S={S} N={N} D={D}", x, y, idx, dtype, out)
        # the index draws of training: sample_negatives_indices, without and with cross-utterance negatives
        for (bsz, tsz, nn_, cross) in [(4, 150, 100, 0), (3, 200, 100, 10)]:
            S, D = bsz * tsz, 256
            with torch.random.fork_rng(devices=[]):
                torch.manual_seed(560 + cross)
                neg = F.sample_negatives_indices(bsz, tsz, tsz, nn_, cross).view(bsz, tsz, nn_ + cross).reshape(S, nn_ + cross)
            idx = torch.cat([torch.arange(S).view(S, 1), neg], dim=1)
            x, y = q(gen(S, D, seed=561), dtype), q(gen(S, D, seed=562), dtype)
            sn_compare(f"sampled_negatives[{dn}] production draws bsz={bsz} tsz={tsz} N={nn_}+{cross}", x, y, idx, dtype, out)
        # quantised targets repeat: y rows from a 12-entry codebook -> the negative IS the positive in ~ 1/12 of the entries
        S, N, D = 400, 100, 256
        cb = q(gen(12, D, seed=570), dtype)
        y = cb[torch.randint(0, 12, (S,), generator=torch.Generator().manual_seed(571))]
        x = q(gen(S, D, seed=572), dtype)
        idx = torch.cat([torch.arange(S).view(S, 1), torch.randint(0, S, (S, N), generator=torch.Generator().manual_seed(573))], dim=1)
        tag = f"sampled_negatives[{dn}] quantised-target repeats"
        lg, l2, _, _ = sn_compare(tag, x, y, idx, dtype, out)
        frac = torch.isinf(l2[:, 1:]).double().mean().item()
        out.append((tag + f" masked fraction {frac:.3f} within [0.02, 0.20]", 0.0 if 0.02 <= frac <= 0.20 else 1.0, 0.0))
        tgt0 = torch.zeros(S, dtype=torch.int32, device=DEV)
        dlog = torch.full((S, N + 1), float("nan"), device=DEV)
        ops.ce_rows(lg.to(DEV), tgt0, N + 1, N + 1, dlog, N + 1, 1.0, flat_wrong=True)
        out.append((tag + " d loss / d logit at the masked entries (non-zero count)", float((dlog.cpu()[torch.isinf(l2)] != 0).sum().item()), 0.0))
        # skewed gathers: one row of y gathered > 500 times, > 30 % of its rows never (positives in the first S rows only)
        S, R, N, D = 300, 600, 20, 256
        x, y = q(gen(S, D, seed=580), dtype), q(gen(R, D, seed=581), dtype)
        gi = torch.Generator().manual_seed(582)
        neg = torch.randint(0, 350, (S, N), generator=gi)
        neg[torch.rand(S, N, generator=gi) < 0.3] = 7
        idx = torch.cat([torch.arange(S).view(S, 1), neg], dim=1)
        cnt = torch.bincount(idx.view(-1), minlength=R)
        tag = f"sampled_negatives[{dn}] skewed gathers (row 7: {int(cnt[7])} times; never gathered: {int((cnt == 0).sum())} of {R} rows)"
        _, _, _, dy = sn_compare(tag, x, y, idx, dtype, out)
        out.append((tag + " premise: > 500 gathers of one row and >= 30 % of the rows never", 0.0 if cnt[7] > 500 and (cnt == 0).sum() >= 0.3 * R else 1.0, 0.0))
        out.append((tag + " dy on the rows never gathered (non-zero elements)", float((dy[cnt == 0] != 0).sum().item()), 0.0))
        # y with more rows than x (negatives_from_everywhere / codebook negatives): the positive points into y
        S, N, D = 150, 30, 64
        R = S + 200
        x, y = q(gen(S, D, seed=590), dtype), q(gen(R, D, seed=591), dtype)
        gi = torch.Generator().manual_seed(592)
        idx = torch.cat([torch.randperm(R, generator=gi)[:S].view(S, 1), torch.randint(0, R, (S, N), generator=gi)], dim=1)
        tag = f"sampled_negatives[{dn}] y has R = S + 200 = {R} rows"
        _, _, _, dy = sn_compare(tag, x, y, idx, dtype, out)
        out.append((tag + " dy row count", float(abs(dy.shape[0] - R)), 0.0))
        # zero rows: the max(||.||, eps) clamp; the zero row of x has all logits equal (0): arg-max = arg-min = 0, which
        # the criterion counts as NOT correct
        S, N, D = 64, 10, 32
        x, y = q(gen(S, D, seed=600), dtype), q(gen(S, D, seed=601), dtype)
        x[3] = 0.0
        y[5] = 0.0
        idx = torch.cat([torch.arange(S).view(S, 1), torch.randint(0, S, (S, N), generator=torch.Generator().manual_seed(602))], dim=1)
        idx[9, 2] = 5
        tag = f"sampled_negatives[{dn}] zero rows"
        rx, ry = torch.arange(S) == 3, torch.arange(S) == 5
        lg, l2, dx, dy = sn_compare(tag, x, y, idx, dtype, out, skip_rows_x=rx, skip_rows_y=ry)
        out.append((tag + " finite loss gradients", 0.0 if torch.isfinite(dx).all() and torch.isfinite(dy).all() else 1.0, 0.0))
        _, corr = ops.ce_rows(lg.to(DEV), torch.zeros(S, dtype=torch.int32, device=DEV), N + 1, N + 1, None, 0, 1.0, flat_wrong=True)
        ref_row = float((l2[3].argmax() == 0) and not (l2[3].argmin() == 0))
        out.append((tag + f" all-equal logit row: kernel counts it as correct = {corr[3].item():.0f}, the criterion {ref_row:.0f}",
                    abs(corr[3].item() - ref_row), 0.0))
        # a negative that is a positive multiple of the positive: the raw rows differ, the reference does not mask it (its
        # logit equals the positive's); the normalised rows the kernel multiplies are identical
        S, N, D = 64, 10, 256
        x, y = q(gen(S, D, seed=610), dtype), q(gen(S, D, seed=611), dtype)
        y[40] = 2.0 * y[11]
        idx = torch.cat([torch.arange(S).view(S, 1), torch.randint(0, S, (S, N), generator=torch.Generator().manual_seed(612))], dim=1)
        idx[11, 4] = 40
        idx[11, 6] = 11      # and the positive's own row among the negatives: masked
        tag = f"sampled_negatives[{dn}] scaled duplicate y[j] = 2 y[pos]"
        lg, l2, _, _ = sn_compare(tag, x, y, idx, dtype, out)
        kv = lg[11, 4].item()
        out.append((tag + f": reference logit {l2[11, 4].item():.4f} (not masked), kernel {kv:.4f}, positive {lg[11, 0].item():.4f}",
                    0.0 if math.isfinite(kv) and kv == lg[11, 0].item() and math.isinf(lg[11, 6].item()) else 1.0, 0.0))
    # ce_rows directly: 101 columns (two 64-lane passes), padded leading dimensions, -inf in non-target columns, an all-equal row
    S, V, ld = 77, 101, 104
    gi = torch.Generator().manual_seed(620)
    lgt = torch.full((S, ld), float("nan"))
    lgt[:, :V] = 4.0 * torch.randn(S, V, generator=gi)
    tgt = torch.randint(0, V, (S,), generator=gi)
    minf = torch.rand(S, V, generator=gi) < 0.1
    minf[torch.arange(S), tgt] = False
    lgt[:, :V][minf] = float("-inf")
    lgt[13, :V] = 1.25
    l64 = lgt[:, :V].double().requires_grad_(True)
    rows_ref = TF.cross_entropy(l64, tgt, reduction="none")
    (dref,) = torch.autograd.grad(rows_ref.sum() * 1.7, l64)
    for ddt in (torch.float32, torch.bfloat16):
        dn = "fp32" if ddt == torch.float32 else "bf16"
        dlog = torch.full((S, ld), float("nan"), dtype=ddt, device=DEV)
        for flat in (False, True):
            rows, corr = ops.ce_rows(lgt.to(DEV), tgt.to(torch.int32).to(DEV), V, ld, dlog, ld, 1.7, flat_wrong=flat)
            mx = l64.detach().max(-1).values
            cref = (l64.detach()[torch.arange(S), tgt] >= mx) & ~(flat & (l64.detach().min(-1).values == mx))
            out.append((f"ce_rows V=101 ld=104 dlogits[{dn}] flat_wrong={flat}: correct rows (mismatches)", float((corr.cpu().bool() != cref).sum().item()), 0.0))
        out.append((f"ce_rows V=101 ld=104 dlogits[{dn}] loss rows", err(rows, rows_ref), TOL32))
        out.append((f"ce_rows V=101 ld=104 dlogits[{dn}] dlogits", err(dlog[:, :V], dref), tol_for(ddt)))
        out.append((f"ce_rows V=101 ld=104 dlogits[{dn}] pad columns (non-zero elements)", float((dlog[:, V:] != 0).sum().item()), 0.0))
    return out


def check_adam():
    from oracle import wavlm_oracle as O
    out = []
    n = 10007
    p, g = gen(n, seed=1), gen(n, seed=2, scale=0.1)
    m, v = torch.zeros(n), torch.zeros(n)
    pd, md, vd = p.clone().to(DEV), m.clone().to(DEV), v.clone().to(DEV)
    plow = torch.empty(n, dtype=torch.bfloat16, device=DEV)
    gd = g.to(torch.bfloat16).to(DEV)
    gq = g.to(torch.bfloat16).float()
    pr, mr, vr = p.clone(), m.clone(), v.clone()
    gn = ops.sumsq(gd)
    mult, max_norm = 0.5, 1.0
    total = gq.norm().item() * mult
    clip = min(1.0, max_norm / (total + 1e-6))
    for step in (1, 2, 3):
        ops.adam_step(pd, md, vd, gd, plow, lr=5e-4, beta1=0.9, beta2=0.98, eps=1e-6, weight_decay=0.01, step=step,
                      grad_mult=mult, gnorm_sq=gn, max_norm=max_norm)
        pr, mr, vr = O.adam_reference_step(pr, gq * mult * clip, mr, vr, step, 5e-4, 0.9, 0.98, 1e-6, 0.01)
    out.append(("adam p", err(pd, pr), 1e-5))
    out.append(("adam m", err(md, mr), 1e-5))
    out.append(("adam v", err(vd, vr), 1e-5))
    out.append(("adam low-precision copy", err(plow, pr), 1e-2))
    return out


def check_activations():
    """elementwise feed-forward activations and gated linear units (wavlm_act_* / wavlm_glu_*) against torch in fp64, forward
    and backward, both dtypes; and FFNFn with every activation_fn against the same composition in torch"""
    import torch.nn.functional as tF
    from unispeech_amd import functional as Fn
    out = []
    refs = {"relu": torch.relu, "tanh": torch.tanh, "gelu": lambda x: tF.gelu(x),
            "gelu_accurate": lambda x: 0.5 * x * (1 + torch.tanh(math.sqrt(2 / math.pi) * (x + 0.044715 * x ** 3)))}
    gates = {"sigmoid": torch.sigmoid, "swish": lambda b: b * torch.sigmoid(b), "relu": torch.relu, "gelu": lambda b: tF.gelu(b),
             "bilinear": lambda b: b}
    for dtype in (torch.float32, torch.bfloat16):
        tol = tol_for(dtype)
        x = q(2.0 * gen(301, 96, seed=5), dtype)
        dy = q(gen(301, 96, seed=6), dtype)
        for kind, f in refs.items():
            xr = x.double().requires_grad_(True)
            yr = f(xr)
            (dxr,) = torch.autograd.grad(yr, xr, dy.double())
            y = ops.act_fwd(x.to('cuda', dtype), kind)
            dx = ops.act_bwd(x.to('cuda', dtype), dy.to('cuda', dtype), kind)
            out.append((f"act[{dtype}] {kind} fwd", err(y.float().cpu(), yr.detach().float()), tol))
            out.append((f"act[{dtype}] {kind} bwd", err(dx.float().cpu(), dxr.float()), tol))
        dyh = q(gen(301, 48, seed=7), dtype)
        for gate, g in gates.items():
            xr = x.double().requires_grad_(True)
            yr = xr[:, :48] * g(xr[:, 48:])
            (dxr,) = torch.autograd.grad(yr, xr, dyh.double())
            y = ops.glu_fwd(x.to('cuda', dtype), gate)
            dx = ops.glu_bwd(x.to('cuda', dtype), dyh.to('cuda', dtype), gate)
            out.append((f"glu[{dtype}] {gate} fwd", err(y.float().cpu(), yr.detach().float()), tol))
            out.append((f"glu[{dtype}] {gate} bwd", err(dx.float().cpu(), dxr.float()), tol))
        # the feed-forward block end to end, every activation_fn (no dropout)
        n, D, Fd = 200, 64, 128
        for act in ("gelu", "relu", "gelu_accurate", "tanh", "linear", "glu"):
            xin = q(gen(n, D, seed=11), dtype)
            W1 = q(0.2 * gen(Fd * (2 if act == "glu" else 1), D, seed=12), dtype)
            b1 = q(0.1 * gen(W1.shape[0], seed=13), dtype)
            W2, b2 = q(0.2 * gen(D, Fd, seed=14), dtype), q(0.1 * gen(D, seed=15), dtype)
            dyo = q(gen(n, D, seed=16), dtype)
            ts = [t.double().requires_grad_(True) for t in (xin, W1, b1, W2, b2)]
            u = tF.linear(ts[0], ts[1], ts[2])
            if act == "glu":
                h = u[:, :Fd] * (u[:, Fd:] * torch.sigmoid(u[:, Fd:]))
            elif act == "linear":
                h = u
            else:
                h = refs[act](u)
            yr = tF.linear(h, ts[3], ts[4])
            gr = torch.autograd.grad(yr, ts, dyo.double())
            td = [t.to('cuda', dtype).requires_grad_(True) for t in (xin, W1, b1, W2, b2)]
            y = Fn.FFNFn.apply(td[0], td[1], td[2], td[3], td[4], 0.0, 0, None, None, False, act)
            gd = torch.autograd.grad(y, td, dyo.to('cuda', dtype))
            out.append((f"ffn[{dtype}] {act} y", err(y.detach().float().cpu(), yr.detach().float()), tol))
            for nm, a, b in zip(("dx", "dW1", "db1", "dW2", "db2"), gd, gr):
                out.append((f"ffn[{dtype}] {act} {nm}", err(a.float().cpu(), b.float()), tol))
    return out


# ------------------------------------------------------------------ row kernels where a wave walks several rows
# Row counts below rest on the launch geometry of rowops.hip / optim.hip: 4 rows per block (one per wave); LayerNorm grid caps
# 1024 (forward, full-width kernels and every forward with dropout), 512 (backward, LN_BWD_BLOCKS), 8192 (general forward without
# dropout), above 131 072 rows: rows / 128 (forward) and rows / 256 (backward); CS_BLOCKS = 512 partial rows of colsum.
LN_ROWS = 8195            # = 2 * 4096 + 3 = 4 * 2048 + 3: forward waves take 2 or 3 rows, backward waves 4 or 5, both last sweeps ragged
LN_ROWS_GENERAL = 32773   # = 32 768 + 5: the general forward without dropout (cap 8192) gives some waves a second row
LN_ROWS_BIG = 262149      # = 2 * 131 072 + 5: caps 2048 (forward) and 1024 (backward)
LN_WIDTHS = (512, 768, 1024)
TOL32_SUM = 2e-4          # long fp32 reductions (module docstring)


def ln_full_enabled():
    """rowops.hip's reading of WAVLM_LN_FULL (first character '0': the general kernels at every width)"""
    import os
    return os.environ.get("WAVLM_LN_FULL", "1")[:1] != "0"


def leaves_no_footprint(fn):
    """run a group and put ops' grow-only workspaces back as they were, then release the cache: a workspace grown while large
    freed blocks are cached pins such a block with stale data around it, and the poisoned allocations of the conv checks that
    run later in the same process (_poison_reaches_empty) would be handed that memory instead of the NaN-filled block"""
    import functools

    @functools.wraps(fn)
    def run():
        saved = dict(ops._WS)
        try:
            return fn()
        finally:
            torch.cuda.synchronize()
            ops._WS.clear()
            ops._WS.update(saved)
            _LN_RAW.clear()
            torch.cuda.empty_cache()
    return run


def errd(a, b):
    """err()'s metric for device tensors, evaluated where they live (one scalar crosses to the host instead of both tensors;
    a NaN or an infinity anywhere in `a` gives inf, as there)"""
    if a.shape != b.shape:
        return float("inf")
    if b.numel() == 0:
        return 0.0
    a, b = a.detach().double(), b.detach().double()
    v = ((a - b).abs().max() / b.abs().max().clamp_min(1e-12)).item()
    return v if math.isfinite(v) else float("inf")


def dgen(*shape, seed, scale=1.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(*shape, generator=g, device=DEV) * scale


def refused(fn):
    """0.0 iff fn() ends in check()'s invalid-argument error"""
    from unispeech_amd._lib import WavlmHipError
    try:
        fn()
    except WavlmHipError as e:
        return 0.0 if "invalid argument" in str(e) else 1.0
    return 1.0


def same_bits(a, b):
    a, b = a.contiguous(), b.contiguous()
    return 0.0 if a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.uint8), b.view(torch.uint8)) else 1.0


_LN_RAW = {}


def ln_inputs(rows, D, dtype, pdtype):
    """fp32 device tensors rounded through the tested dtypes (x, r, dy, extra through dtype; g, b through pdtype): the raw
    draws are made once per (rows, D) and shared by every case of a group"""
    raw = _LN_RAW.get((rows, D))
    if raw is None:
        raw = dict(x=dgen(rows, D, seed=1), r=dgen(rows, D, seed=2), dy=dgen(rows, D, seed=5), extra=dgen(rows, D, seed=23),
                   g=1 + 0.1 * dgen(D, seed=3), b=0.1 * dgen(D, seed=4))
        _LN_RAW[(rows, D)] = raw
    return {k: q(v, pdtype if k in ("g", "b") else dtype) for k, v in raw.items()}


def ln_ref(I, dtype, act, res, m_in=None, m_out=None, eps=1e-5):
    """y = m_out * act(LN(x + m_in * r)) in fp64 on the device and its gradients for the cotangent dy through autograd; the
    pre-norm sum takes the bf16 rounding of the stored tensor (straight through), as in check_layernorm"""
    D = I["x"].shape[-1]
    xs = I["x"].double().requires_grad_(True)
    rs = I["r"].double().requires_grad_(True) if res else None
    gs, bs = I["g"].double().requires_grad_(True), I["b"].double().requires_grad_(True)
    s = xs
    if res:
        s = xs + (rs * m_in if m_in is not None else rs)
        if dtype == torch.bfloat16:
            s = s + (s.detach().to(dtype).double() - s.detach())
    z = TF.layer_norm(s, (D,), gs, bs, eps)
    y = TF.gelu(z) if act else z
    if m_out is not None:
        y = y * m_out
    grads = torch.autograd.grad(y, [xs, gs, bs] + ([rs] if res else []), I["dy"].double())
    return dict(y=y.detach(), s=s.detach(), gx=grads[0], dgamma=grads[1], dbeta=grads[2], gr=grads[3] if res else None)


def ln_rows_case(out, name, rows, D, dtype, pdtype, res, act, saves=(True, False), drop=None, masks=(None, None)):
    """one forward per `save`, and after the saving one a backward (dr and its column sum where there is a residual), against
    ln_ref; mean / rstd against the fp64 statistics of the stored s"""
    I = ln_inputs(rows, D, dtype, pdtype)
    ref = ln_ref(I, dtype, act, res, *masks)
    tol, tols = tol_for(dtype), (TOL32_SUM if dtype == torch.float32 else TOLBF)
    xd, rd, dyd = [I[k].to(dtype) for k in ("x", "r", "dy")]
    gd, bd = I["g"].to(pdtype), I["b"].to(pdtype)
    drop = drop or {}
    tag0 = f"{name}[{dtype},{pdtype}] rows={rows} D={D} res={int(res)} act={act}" + (f" p=({drop['p_in']},{drop['p_out']})" if drop else "")
    for save in saves:
        tag = tag0 + ("" if save else " no-save")
        y, s, mean, rstd = ops.layernorm_fwd(xd, rd if res else None, gd, bd, 1e-5, act=act, save=save, **drop)
        out.append((tag + " y", errd(y, ref["y"]), tol))
        if not save:
            continue
        sd = s.double()
        out.append((tag + " s", errd(s, ref["s"]), tol))
        out.append((tag + " mean of the stored s", errd(mean, sd.mean(1)), TOL32))
        out.append((tag + " rstd of the stored s", errd(rstd, (sd.var(1, unbiased=False) + 1e-5).rsqrt()), TOL32))
        dx, dr, dg, db, cs = ops.layernorm_bwd(dyd, s, mean, rstd, gd, bd, act=act, need_dr=res, dr_colsum=True if res else None, **drop)
        out.append((tag + " dx", errd(dx, ref["gx"]), tol))
        out.append((tag + " dgamma", errd(dg, ref["dgamma"]), tols))
        out.append((tag + " dbeta", errd(db, ref["dbeta"]), tols))
        if res:
            out.append((tag + " dr", errd(dr, ref["gr"]), tol))
            out.append((tag + " dr colsum", errd(cs, ref["gr"].sum(0)), tols))
        if ln_full_enabled() and act == 1 and not res and not drop and D == 512 and dtype == pdtype == torch.bfloat16:
            # these launches took the GELU-table instances (chord table of the normal CDF in LDS): gelu' is within 5.7e-4
            # absolute of the erf form the reference differentiates, a seventh of bf16's half ulp at 1, so TOLBF holds
            out.append((tag + " dgamma, table gelu' against the erf reference", errd(dg, ref["dgamma"]), TOLBF))
            out.append((tag + " dbeta, table gelu' against the erf reference", errd(db, ref["dbeta"]), TOLBF))


def ln_bwd_forms(out, rows, D, dtype, act=1, grad_scale=0.37):
    """every combination of dx_add x need_dr x dr_colsum x dr_incl_add with grad_scale != 1 on one saved forward (the template
    instances CS x HA x HD of the full-width backward), then the three parameter sums accumulated into pre-filled sinks"""
    I = ln_inputs(rows, D, dtype, dtype)
    ref = ln_ref(I, dtype, act, True)
    tol, tols = tol_for(dtype), (TOL32_SUM if dtype == torch.float32 else TOLBF)
    xd, rd, dyd, ed, gd, bd = [I[k].to(dtype) for k in ("x", "r", "dy", "extra", "g", "b")]
    _y, s, mean, rstd = ops.layernorm_fwd(xd, rd, gd, bd, 1e-5, act=act, save=True)
    gx = grad_scale * ref["gx"]
    for add in (False, True):
        for need_dr in (False, True):
            for cs_on in (False, True):
                for incl in (False, True):
                    tag = (f"layernorm_rows[{dtype}] rows={rows} D={D} bwd dx_add={int(add)} dr={int(need_dr)} colsum={int(cs_on)} "
                           f"incl_add={int(incl)} grad_scale={grad_scale}")
                    dx, dr, dg, db, cs = ops.layernorm_bwd(dyd, s, mean, rstd, gd, bd, act=act, grad_scale=grad_scale, need_dr=need_dr,
                                                           dr_colsum=True if cs_on else None, dx_add=ed if add else None, dr_incl_add=incl)
                    rdx = gx + I["extra"].double() if add else gx
                    rdr = rdx if (add and incl) else gx
                    out.append((tag + " dx", errd(dx, rdx), tol))
                    out.append((tag + " dgamma", errd(dg, ref["dgamma"]), tols))
                    out.append((tag + " dbeta", errd(db, ref["dbeta"]), tols))
                    if need_dr:
                        out.append((tag + " dr", errd(dr, rdr), tol))
                    if cs_on:
                        out.append((tag + " dr colsum", errd(cs, rdr.sum(0)), tols))
    sink0 = q(30.0 * dgen(3, D, seed=21), dtype)
    sinks = [t.to(dtype).clone() for t in sink0]
    ops.layernorm_bwd(dyd, s, mean, rstd, gd, bd, act=act, grad_scale=grad_scale, need_dr=True, dgamma=sinks[0], dbeta=sinks[1],
                      dr_colsum=sinks[2])
    tag = f"layernorm_rows[{dtype}] rows={rows} D={D} bwd accumulated into pre-filled sinks"
    for nm, got, base, add_ in zip(("dgamma", "dbeta", "dr colsum"), sinks, sink0, (ref["dgamma"], ref["dbeta"], gx.sum(0))):
        out.append((f"{tag} {nm}", errd(got, base.double() + add_), tols))


LN_SEG_CASES = [((5, 1639), (1, 2)), ((745, 11), (0, 1))]   # (B, T) with B * T = LN_ROWS, dx_pad: the segment is shorter / far shorter than a wave's row step (2048)


def ln_segmented(out):
    """wavlm_layernorm_bwd_seg's padded dx layout with the segment bookkeeping carried over four or five rows per wave, into a
    poisoned allocation (the caller has checked _poison_reaches_empty); without the full-width kernels the call has to be refused"""
    for dtype, D in ((torch.bfloat16, 512), (torch.float32, 768)):
        I = ln_inputs(LN_ROWS, D, dtype, dtype)
        ref = ln_ref(I, dtype, 1, False)
        xd, dyd, gd, bd = [I[k].to(dtype) for k in ("x", "dy", "g", "b")]
        _y, s, mean, rstd = ops.layernorm_fwd(xd, None, gd, bd, 1e-5, act=1, save=True)
        plain = ops.layernorm_bwd(dyd, s, mean, rstd, gd, bd, act=1)
        for (Bn, Tn), (fp, bp) in LN_SEG_CASES:
            assert Bn * Tn == LN_ROWS
            tag = f"layernorm_rows[{dtype}] D={D} segmented dx [{Bn}, {Tn}] pad=({fp},{bp})"
            call = lambda: ops.layernorm_bwd(dyd.view(Bn, Tn, D), s.view(Bn, Tn, D), mean, rstd, gd, bd, act=1, dx_pad=(fp, bp))  # noqa: E731
            if not ln_full_enabled():
                out.append((tag + " refused without the full-width kernels", refused(call), 0.0))
                continue
            # exactly the padded allocation's size: the tensors held here leave free blocks of other sizes behind, and the
            # caching allocator hands out the smallest block that fits
            _poison((Bn * (fp + Tn + bp) + fp + bp) * D * dyd.element_size())
            seg = call()
            padded = seg[0]._padded
            out.append((tag + " interior", errd(seg[0].reshape(LN_ROWS, D), ref["gx"]), tol_for(dtype)))
            pads = padded.clone()
            pads[:, fp:fp + Tn] = 0
            out.append((tag + " pad rows exactly zero", float((pads != 0).sum().item()), 0.0))
            out.append((tag + " dx == the unsegmented call, bit for bit", same_bits(seg[0].reshape(LN_ROWS, D), plain[0]), 0.0))
            out.append((tag + " dgamma == the unsegmented call", same_bits(seg[2], plain[2]), 0.0))
            out.append((tag + " dbeta == the unsegmented call", same_bits(seg[3], plain[3]), 0.0))


def ln_refusals(out):
    """D = 2056 (above LN_MAXC * 512) and D = 12 (no multiple of 8): check()'s error, the given sinks untouched"""
    for D in (2056, 12):
        x = dgen(16, D, seed=1)
        g, b = torch.ones(D, device=DEV), torch.zeros(D, device=DEV)
        out.append((f"layernorm_rows D={D} forward refused", refused(lambda: ops.layernorm_fwd(x, None, g, b, 1e-5)), 0.0))
        st = torch.ones(16, device=DEV)
        sinks = [torch.full((D,), 7.0, device=DEV) for _ in range(3)]
        out.append((f"layernorm_rows D={D} backward refused",
                    refused(lambda: ops.layernorm_bwd(x, x, st, st, g, b, need_dr=True, dgamma=sinks[0], dbeta=sinks[1], dr_colsum=sinks[2])), 0.0))
        torch.cuda.synchronize()
        out.append((f"layernorm_rows D={D} refused backward left its sinks alone", float(sum((t != 7.0).sum().item() for t in sinks)), 0.0))


def ln_above_cap_change(out):
    """262 149 rows x 512, bf16, LayerNorm + GELU without residual: forward grid 2048, backward grid 1024 (and the workspace of
    1024 partial rows); inputs from a seeded device generator, reference by torch's fp64 layer_norm / gelu and autograd on the
    device (about 1 GB per fp64 tensor), everything freed before returning"""
    rows, D, dtype = LN_ROWS_BIG, 512, torch.bfloat16
    g = torch.Generator(device=DEV).manual_seed(77)
    xd = torch.randn(rows, D, generator=g, device=DEV).to(dtype)
    dyd = torch.randn(rows, D, generator=g, device=DEV).to(dtype)
    gd = (1 + 0.1 * torch.randn(D, generator=g, device=DEV)).to(dtype)
    bd = (0.1 * torch.randn(D, generator=g, device=DEV)).to(dtype)
    y, s, mean, rstd = ops.layernorm_fwd(xd, None, gd, bd, 1e-5, act=1, save=True)
    dx, _dr, dg, db, _cs = ops.layernorm_bwd(dyd, s, mean, rstd, gd, bd, act=1)
    xs, gs, bs = [t.double().requires_grad_(True) for t in (xd, gd, bd)]
    yr = TF.gelu(TF.layer_norm(xs, (D,), gs, bs, 1e-5))
    gr = torch.autograd.grad(yr, [xs, gs, bs], dyd.double())
    tag = f"layernorm_rows[{dtype}] rows={rows} D={D} LayerNorm + GELU above the cap change"
    out.append((tag + " y", errd(y, yr), TOLBF))
    out.append((tag + " mean", errd(mean, xs.detach().mean(1)), TOL32))
    out.append((tag + " rstd", errd(rstd, (xs.detach().var(1, unbiased=False) + 1e-5).rsqrt()), TOL32))
    for nm, a, r_ in zip(("dx", "dgamma", "dbeta"), (dx, dg, db), gr):
        out.append((f"{tag} {nm}", errd(a, r_), TOLBF))


@leaves_no_footprint
def check_layernorm_rows():
    """LayerNorm forward / backward with several rows per wave (LN_ROWS = 8195 and the constants beside it; the launch geometry
    they rest on is named there): the software pipeline of the full-width kernels with its clamped last prefetch, the per-lane
    dgamma / dbeta / colsum accumulators over four or five rows, every CS x HA x HD instance at the three widths, bf16
    activations with fp32 parameters, the no-residual and no-save forms, the GELU-table instances, the segmented dx layout,
    the general kernels at widths with a partly filled chunk slot, the grid caps above 131 072 rows.  Under WAVLM_LN_FULL=0
    (tests/test_kernels_gpu.py runs the group that way in a fresh process) the same cases land in the general kernels and the
    segmented ones must be refused.  References: fp64 torch on the device (at these sizes a CPU reference is most of the
    run time).  Left out: the 64-bit offset regime (rows * D >= 2^31) -- it needs more than 4 GB per tensor."""
    out = [_poison_reaches_empty(64 << 20)]   # (before this group holds any memory of its own)
    f32, bf = torch.float32, torch.bfloat16
    try:
        ln_segmented(out)
        for D in LN_WIDTHS:
            for dtype, pdtype in ((f32, f32), (bf, bf), (bf, f32)):
                for res in (True, False):
                    for act in (0, 1):
                        ln_rows_case(out, "layernorm_rows", LN_ROWS, D, dtype, pdtype, res, act)
            for dtype in (f32, bf):
                ln_bwd_forms(out, LN_ROWS, D, dtype)
                # idle waves of a block (early return in the forward, zero partials in the backward); no ragged sweep
                for rows in (1, 5, 8192):
                    ln_rows_case(out, "layernorm_rows", rows, D, dtype, dtype, True, 0, saves=(True,))
        for D in (8, 256, 520, 1032, 2048):   # general kernels: one chunk slot barely used, full, and partly filled at NC = 2 and 4
            for dtype in (f32, bf):
                ln_rows_case(out, "layernorm_rows general", LN_ROWS, D, dtype, dtype, True, int(D == 520), saves=(True,))
        ln_rows_case(out, "layernorm_rows general", LN_ROWS_GENERAL, 256, f32, f32, True, 0)
        ln_refusals(out)
        _LN_RAW.clear()
        ln_above_cap_change(out)
    finally:
        _LN_RAW.clear()
        torch.cuda.empty_cache()
    return out


def binom_bounds(n, p_keep, tail):
    """(lo, hi) for X ~ Binomial(n, p_keep): the largest lo with P(X < lo) <= tail and the smallest hi with P(X > hi) <= tail,
    from the exact probabilities (log-gamma form, summed in fp64 from each end); derived here like chi2_quantile, not typed in"""
    dev = DEV if torch.cuda.is_available() else "cpu"
    k = torch.arange(n + 1, dtype=torch.float64, device=dev)
    logp = (math.lgamma(n + 1) - torch.lgamma(k + 1) - torch.lgamma(n - k + 1) + k * math.log(p_keep) + (n - k) * math.log1p(-p_keep))
    pmf = logp.exp()
    below = pmf.cumsum(0)                     # P(X <= k)
    above = pmf.flip(0).cumsum(0).flip(0)     # P(X >= k)
    lo = int((below <= tail).sum().item())
    hi = int((above > tail).sum().item()) - 1
    return lo, hi


def keep_fraction_lines(out, tag, counts, n, p, tail, quant):
    """two lines: how far the largest / smallest of `counts` (kept cells out of n each) lies above / below n (1 - p), against the
    binomial quantile at `tail` per side plus `quant`, the shift of the expectation by the quantisation of p"""
    lo, hi = binom_bounds(n, 1.0 - p, tail)
    exp_ = n * (1.0 - p)
    out.append((f"{tag} keep fraction above 1 - p (n = {n}, {counts.numel()} of them)", (counts.max().item() - exp_) / n, (hi - exp_) / n + quant))
    out.append((f"{tag} keep fraction below 1 - p (n = {n}, {counts.numel()} of them)", (exp_ - counts.min().item()) / n, (exp_ - lo) / n + quant))


LN_DROP_PAIRS = [(0.25, 0.0), (0.0, 0.25), (0.1, 0.1)]


def ln_probe_masks(rows, D, dtype, drop):
    """the keep masks of a launch, read out of a probe launch with the same (p_in, seed_in, p_out, seed_out): x = 0, r = 1,
    gamma = 0, beta = 1, no activation give s = keep_in * scale_in and y = keep_out * scale_out in every cell"""
    z, o = torch.zeros(rows, D, dtype=dtype, device=DEV), torch.ones(rows, D, dtype=dtype, device=DEV)
    yp, sp, _, _ = ops.layernorm_fwd(z, o, torch.zeros(D, dtype=dtype, device=DEV), torch.ones(D, dtype=dtype, device=DEV), 1e-5,
                                     act=0, save=True, **drop)
    return sp != 0, yp != 0, sp, yp


@leaves_no_footprint
def check_layernorm_dropout_ref():
    """LayerNorm with input- and output-side dropout against the fp64 reference that applies the SAME masks (recovered in full
    by a probe launch: the mask is a function of seeds, row and column only) with scale 1 / (1 - p): y, s, dx, dr, dgamma, dbeta
    and the dr column sum at LN_ROWS rows, where forward (1024 blocks) and backward (512) hand rows to waves differently while
    regenerating one mask; p = 0.1 is quantised to 6554 / 65 536, a scale 7e-6 off 1 / 0.9 and well inside TOL32.  Then the law
    of the recovered masks at D = 1024: overall, per-row and per-column keep fractions inside the binomial quantiles at a
    family-wise tail of 1e-6 (+ 1 / 65 536 for the quantisation of p)."""
    out = []
    f32, bf = torch.float32, torch.bfloat16
    rows = LN_ROWS
    cases = [(D, dtype, pp, 0) for D in LN_WIDTHS for dtype in (f32, bf) for pp in LN_DROP_PAIRS]
    cases += [(768, dtype, (0.1, 0.1), 1) for dtype in (f32, bf)]
    cases += [(520, dtype, (0.1, 0.1), 0) for dtype in (f32, bf)]   # general kernels: the forward with dropout is capped at 1024 blocks too
    stat_masks = []
    try:
        for D, dtype, (p_in, p_out), act in cases:
            drop = dict(p_in=p_in, seed_in=0x9E3779B97F4A7C15 ^ D, p_out=p_out, seed_out=0x5851F42D4C957F2D + 3 * D)
            keep_in, keep_out, sp, yp = ln_probe_masks(rows, D, dtype, drop)
            m_in, m_out = keep_in.double() / (1.0 - p_in), keep_out.double() / (1.0 - p_out)
            tag = f"layernorm_dropout_ref[{dtype}] D={D} p=({p_in},{p_out}) probe"
            out.append((tag + " s is 0 or 1 / (1 - p_in)", errd(sp, m_in), tol_for(dtype)))
            out.append((tag + " y is 0 or 1 / (1 - p_out)", errd(yp, m_out), tol_for(dtype)))
            ln_rows_case(out, "layernorm_dropout_ref", rows, D, dtype, dtype, True, act, saves=(True,), drop=drop,
                         masks=(m_in if p_in else None, m_out if p_out else None))
            if D == 1024 and dtype == f32:
                stat_masks += [(f"in p={p_in} (with p_out={p_out})", keep_in, p_in)] if p_in else []
                stat_masks += [(f"out p={p_out} (with p_in={p_in})", keep_out, p_out)] if p_out else []
        # family: per mask one overall, `rows` per-row and D per-column fractions, two sides each
        D = 1024
        tail = 1e-6 / (len(stat_masks) * 2 * (1 + rows + D))
        for nm, keep, p in stat_masks:
            tag = f"layernorm_dropout_ref mask {nm} rows={rows} D={D}"
            keep_fraction_lines(out, tag + " overall", keep.sum().reshape(1), rows * D, p, tail, 1.0 / 65536)
            keep_fraction_lines(out, tag + " per row", keep.sum(1), D, p, tail, 1.0 / 65536)
            keep_fraction_lines(out, tag + " per column", keep.sum(0), rows, p, tail, 1.0 / 65536)
    finally:
        _LN_RAW.clear()
        torch.cuda.empty_cache()
    return out


@leaves_no_footprint
def check_colsum_rows():
    """ops.colsum against x.double().sum(0) where colsum_finish_kernel's four-loads-in-flight loop runs (more than 192 partial
    rows): rows 799 / 1027 / 1795 / 2048 / 8195 give 200 / 257 / 449 / 512 / 512 partial rows, so that per 64-row slice the
    unrolled loop runs zero times, once or twice, with and without a remainder, and colsum_partial_kernel is strided at 8195
    (CS_BLOCKS = 512 blocks of 4 rows); N = 8, 768 and CS_MAXC * 512 = 4096; ld > N; row masks; accumulation; refusals"""
    out = []
    f32, bf = torch.float32, torch.bfloat16
    raw = dgen(8195, 4096, seed=1)
    for dtype in (f32, bf):
        tols = TOL32_SUM if dtype == f32 else TOLBF
        for N in (8, 768, 4096):
            xq = q(raw[:, :N], dtype)
            for rows in (799, 1027, 1795, 2048, 8195):
                xd = xq[:rows].to(dtype).contiguous()
                out.append((f"colsum_rows[{dtype}] rows={rows} N={N}", errd(ops.colsum(xd, f32), xq[:rows].double().sum(0)), tols))
        rows, N = 8195, 768
        xq = q(raw[:, :N], dtype)
        xd = xq.to(dtype).contiguous()
        want = xq.double().sum(0)
        wide = torch.full((rows, N + 8), float("nan"), dtype=dtype, device=DEV)
        wide[:, :N] = xd
        out.append((f"colsum_rows[{dtype}] rows={rows} N={N} ld=N+8", errd(ops.colsum(wide, f32, rows=rows, N=N, ld=N + 8), want), tols))
        # masks: rows 40..43 are one block's four rows of the first sweep; rows = 44..47 (mod 2048) are ALL rows of block 11
        ar = torch.arange(rows, device=DEV)
        exc = ((ar >= 40) & (ar < 44)) | ((ar % 2048 >= 44) & (ar % 2048 < 48)) | (ar % 5 == 0)
        inc = ar % 3 != 1
        e8, i8 = exc.to(torch.uint8), inc.to(torch.uint8)
        out.append((f"colsum_rows[{dtype}] rows={rows} exclude mask", errd(ops.colsum(xd, f32, exclude=e8), xq.double()[~exc].sum(0)), tols))
        out.append((f"colsum_rows[{dtype}] rows={rows} include mask", errd(ops.colsum(xd, f32, include=i8), xq.double()[inc].sum(0)), tols))
        out.append((f"colsum_rows[{dtype}] rows={rows} include + exclude masks",
                    errd(ops.colsum(xd, f32, include=i8, exclude=e8), xq.double()[inc & ~exc].sum(0)), tols))
        for sdt in (bf, f32):
            sink0 = q(100.0 * dgen(N, seed=7), sdt)
            sink = sink0.to(sdt).clone()
            ops.colsum(xd, sdt, out=sink, accumulate=True)
            out.append((f"colsum_rows[{dtype}] rows={rows} accumulated into a {sdt} sink", errd(sink, sink0.double() + want),
                        TOLBF if bf in (sdt, dtype) else TOL32_SUM))
        for Nbad in (4104, 12):
            xb = torch.ones(64, Nbad, dtype=dtype, device=DEV)
            sink = torch.full((Nbad,), 7.0, device=DEV)
            out.append((f"colsum_rows[{dtype}] N={Nbad} refused", refused(lambda: ops.colsum(xb, f32, out=sink, accumulate=True)), 0.0))
            out.append((f"colsum_rows[{dtype}] N={Nbad} refused call left its sink alone", float((sink != 7.0).sum().item()), 0.0))
    return out


ADAM_HP = dict(lr=5e-4, beta1=0.9, beta2=0.98, eps=1e-6)


def adam_case(out, name, n, *, grad_dtype=torch.bfloat16, lowp=True, weight_decay=0.01, max_norm=1.0, norm=True, mult=0.5,
              mult_dev=None, steps=(1, 2, 3)):
    """`steps` of ops.adam_step on n elements against oracle.adam_reference_step in fp64 on the device (check_adam's tolerances)"""
    from oracle import wavlm_oracle as O
    p = dgen(n, seed=1)
    gq = q(dgen(n, seed=2, scale=0.1), grad_dtype)
    pd, md, vd = p.clone(), torch.zeros_like(p), torch.zeros_like(p)
    gd = gq.to(grad_dtype)
    plow = torch.empty(n, dtype=torch.bfloat16, device=DEV) if lowp else None
    gn = ops.sumsq(gd) if norm else None
    md_ = torch.tensor([mult_dev], device=DEV) if mult_dev is not None else None
    fac = mult * (mult_dev if mult_dev is not None else 1.0)
    clip = 1.0
    if norm and max_norm > 0:
        clip = min(1.0, max_norm / (gq.double().norm().item() * abs(fac) + 1e-6))
    pr, mr, vr = p.double(), torch.zeros(n, dtype=torch.float64, device=DEV), torch.zeros(n, dtype=torch.float64, device=DEV)
    for step in steps:
        ops.adam_step(pd, md, vd, gd, plow, weight_decay=weight_decay, step=step, grad_mult=mult, grad_mult_dev=md_, gnorm_sq=gn,
                      max_norm=max_norm, **ADAM_HP)
        pr, mr, vr = O.adam_reference_step(pr, gq.double() * fac * clip, mr, vr, step, ADAM_HP["lr"], ADAM_HP["beta1"], ADAM_HP["beta2"],
                                           ADAM_HP["eps"], weight_decay)
    tag = f"flat_strided adam {name} n={n} (clip {clip:.3g})"
    out.append((tag + " p", errd(pd, pr), 1e-5))
    out.append((tag + " m", errd(md, mr), 1e-5))
    out.append((tag + " v", errd(vd, vr), 1e-5))
    if lowp:
        out.append((tag + " low-precision copy", errd(plow, pr), 1e-2))


@leaves_no_footprint
def check_flat_strided():
    """the flat grid-stride kernels past their grid caps, at the smallest n beyond the cap plus a ragged tail, against fp64
    torch on the device: adam_step (cap 16384 blocks x 256), axpby / scale_dev (8192 x 256 elements), dropout / dropout_add
    (8192 x 256 vectors of 8), sumsq (1024 blocks x 4096 elements), select_rows / gather_rows (4096 x 256 vectors of 8); and
    adam_step's argument combinations at check_adam's n"""
    out = []
    f32, bf = torch.float32, torch.bfloat16
    adam_case(out, "past the cap", 16384 * 256 + 777, steps=(1,))
    n = 10007
    adam_case(out, "fp32 gradient", n, grad_dtype=f32)
    adam_case(out, "p_lowp=None", n, lowp=False)
    adam_case(out, "weight_decay=0", n, weight_decay=0.0)
    adam_case(out, "max_norm=0 with a norm given", n, max_norm=0.0)
    adam_case(out, "gnorm_sq=None", n, norm=False)
    adam_case(out, "grad_mult_dev given", n, mult_dev=0.75)
    adam_case(out, "clip that does not bind", n, max_norm=1e4)
    for dtype in (f32, bf):
        tol = tol_for(dtype)
        n = 8192 * 256 + 8
        x, y = q(dgen(n, seed=3), dtype), q(dgen(n, seed=4), dtype)
        yd = y.to(dtype).clone()
        ops.axpby_(yd, x.to(dtype), 0.5, 2.0)
        out.append((f"flat_strided axpby[{dtype}] n={n}", errd(yd, 0.5 * x.double() + 2.0 * y.double()), tol))
        yd = torch.full((n,), float("nan"), dtype=dtype, device=DEV)
        ops.axpby_(yd, x.to(dtype), 0.5, 0.0)
        out.append((f"flat_strided axpby[{dtype}] n={n} b=0 (y not read)", errd(yd, 0.5 * x.double()), tol))
        if dtype == f32:
            xb = q(x, bf)
            yd = y.clone()
            ops.axpby_(yd, xb.to(bf), 0.5, 2.0)
            out.append((f"flat_strided axpby bf16 -> fp32 n={n}", errd(yd, 0.5 * xb.double() + 2.0 * y.double()), tol))
        z = x.to(dtype).clone()
        ops.scale_dev_(z, torch.tensor([3.0], device=DEV), 0.5)
        out.append((f"flat_strided scale_dev[{dtype}] n={n}", errd(z, 1.5 * x.double()), tol))
        n = 1024 * 4096 + 5
        x = q(dgen(n, seed=5), dtype)
        out.append((f"flat_strided sumsq[{dtype}] n={n}", errd(ops.sumsq(x.to(dtype), 0.25), 0.25 * (x.double() ** 2).sum().reshape(1)), tol))
        rows, D = 10923, 768   # rows * D / 8 = 1 048 608 vectors, 32 above 4096 x 256
        x = q(dgen(rows, D, seed=6), dtype)
        xd = x.to(dtype)
        ar = torch.arange(rows, device=DEV)
        sel, zero = ar % 3 == 0, ar % 5 == 0
        for edt in ((f32,) if dtype == f32 else (bf, f32)):
            emb = q(dgen(D, seed=7), edt)
            got = ops.select_rows(xd, sel.to(torch.uint8), emb.to(edt), zero.to(torch.uint8))
            ref = x.clone(); ref[sel] = q(emb, dtype); ref[zero] = 0
            out.append((f"flat_strided select_rows[{dtype}, emb {edt}] {rows}x{D}", errd(got, ref), 1e-6))
        got = ops.select_rows(xd, sel.to(torch.uint8), None, None)
        ref = x.clone(); ref[sel] = 0
        out.append((f"flat_strided select_rows[{dtype}] {rows}x{D} no emb, no zero mask", errd(got, ref), 1e-6))
        idx = torch.randperm(rows, generator=torch.Generator().manual_seed(8)).to(DEV)
        idx[ar % 7 == 0] = -1
        got = ops.gather_rows(xd, idx.to(torch.int32), rows)
        ref = torch.where((idx >= 0)[:, None], x[idx.clamp_min(0)], torch.zeros_like(x))
        out.append((f"flat_strided gather_rows[{dtype}] {rows}x{D}", errd(got, ref), 1e-6))
        # dropout / dropout_add: two keep fractions per dtype, two sides each, in one family with a tail of 1e-6
        n = 8 * (8192 * 256 + 3)
        x, r = q(dgen(n, seed=9), dtype), q(dgen(n, seed=10), dtype)
        xd, rd = x.to(dtype), r.to(dtype)
        for p, seed in ((0.1, 42), (0.25, (1 << 40) + 17)):
            tag = f"flat_strided dropout[{dtype}] n={n} p={p}"
            d1, d2 = ops.dropout(rd, p, seed), ops.dropout(rd, p, seed)
            out.append((tag + " deterministic", same_bits(d1, d2), 0.0))
            keep = d1 != 0
            keep_fraction_lines(out, tag, keep.sum().reshape(1), n, p, 1e-6 / 8, 2.0 ** -32)
            one = torch.tensor(1.0, dtype=f32)
            sc = (one / (one - torch.tensor(p, dtype=f32))).item()   # the library's fp32 1 / (1 - p)
            want = torch.where(keep, (r * sc).to(dtype), torch.zeros_like(rd))
            out.append((tag + " exact values on kept cells", same_bits(d1, want), 0.0))
            da = ops.dropout_add(xd, rd, p, seed)
            out.append((tag + " dropout_add deterministic", same_bits(da, ops.dropout_add(xd, rd, p, seed)), 0.0))
            # same mask, same values: on x = 0 the sum IS dropout(r) (0 + v is exact in both dtypes)
            out.append((tag + " dropout_add(0, r) == dropout(r), bit for bit", same_bits(ops.dropout_add(torch.zeros_like(xd), rd, p, seed), d1), 0.0))
            if dtype == f32:
                out.append((tag + " dropout_add(x, r) == x + dropout(r), bit for bit", same_bits(da, xd + d1), 0.0))
            else:
                out.append((tag + " dropout_add(x, r) against x + keep * r / (1 - p)", errd(da, x.double() + keep * r.double() / (1.0 - p)), tol))
        out.append((f"flat_strided dropout_add[{dtype}] n={n} p=0 is the plain sum", errd(ops.dropout_add(xd, rd, 0.0, 5), x.double() + r.double()), tol))
    return out


# ------------------------------------------------ the masked-prediction head at training shapes; loss.hip past its grid caps
# Launch geometry of loss.hip the shapes below rest on (the wavlm_* entry points at the end of that file):
LOSS_ROW_BLOCKS = 8192                       # l2norm_fwd / l2norm_bwd / ce_rows / gather_dot / rows_wsum: 4 rows per block (one per wave)
LOSS_ROWS = 4 * LOSS_ROW_BLOCKS + 5          # = 32 773: five waves take a second row, the last sweep is ragged
GLU_BLOCKS = 8192                            # glu_fwd / glu_bwd: one row per block
GLU_ROWS = GLU_BLOCKS + 3                    # = 8195
ACT_BLOCKS = 8192                            # act_fwd / act_bwd: 256 elements per block
ACT_N = ACT_BLOCKS * 256 + 7
RED_BLOCKS, RED_PER_BLOCK = 1024, 256 * 8    # sum_f32 / bce_logits: grid = n / 2048, capped at 1024 blocks
RED_N = RED_BLOCKS * RED_PER_BLOCK + 5
MP_TEMP, MP_GRAD = 0.1, 1.7                  # logit_temp of the released recipes; the cotangent of the loss
ACT_REFS = {"relu": torch.relu, "tanh": torch.tanh, "gelu": lambda x: TF.gelu(x),
            "gelu_accurate": lambda x: 0.5 * x * (1 + torch.tanh(math.sqrt(2 / math.pi) * (x + 0.044715 * x ** 3)))}
GLU_GATE_REFS = {"sigmoid": torch.sigmoid, "swish": lambda b: b * torch.sigmoid(b), "relu": torch.relu, "gelu": lambda b: TF.gelu(b),
                 "bilinear": lambda b: b}


def mp_reference(p64, e64, tgt, temp, keep=None):
    """the head in fp64 where the inputs live: cos(p, e) / temp with each norm clamped at 1e-8, sum-reduced cross entropy over
    the rows of `keep` (all rows if None), gradients of MP_GRAD * loss.  Returns (loss, logits of every row, dproj, demb)."""
    pr, er = p64.clone().requires_grad_(True), e64.clone().requires_grad_(True)
    logits = TF.normalize(pr, dim=-1, eps=1e-8) @ TF.normalize(er, dim=-1, eps=1e-8).t() / temp
    loss = TF.cross_entropy(logits if keep is None else logits[keep], tgt if keep is None else tgt[keep], reduction="sum")
    gp, ge = torch.autograd.grad(MP_GRAD * loss, (pr, er))
    return loss.detach(), logits.detach(), gp, ge


def mp_gap(l64, tgt, valid):
    """per row, the target logit minus the best other logit (>= 0: the row counts as correct); -inf where the label lies
    outside [0, V) -- such a row is never correct"""
    S, V = l64.shape
    ar = torch.arange(S, device=l64.device)
    ts = tgt.clamp(0, V - 1)
    other = l64.clone()
    other[ar, ts] = float("-inf")
    return torch.where(valid, l64[ar, ts] - other.max(-1).values, torch.full_like(l64[:, 0], float("-inf")))


def mp_inputs(S, V, Fd, dtype, sigma, labels=None, emb_of=None):
    """CPU draws rounded through dtype: emb = gen(V, F) (or emb_of(raw table)), labels uniform unless given, proj = emb[label]
    + sigma * gen(S, F) -- a head that has learnt something: the target cosine stands out of the V - 1 others by about as much
    as their maximum, so that a good share of the rows, not one in V, is correct"""
    emb_raw = gen(V, Fd, seed=1)
    if emb_of is not None:
        emb_raw = emb_of(emb_raw)
    tgt = labels if labels is not None else torch.randint(0, V, (S,), generator=torch.Generator().manual_seed(3))
    proj = q(emb_raw[tgt] + sigma * gen(S, Fd, seed=2), dtype)
    return proj, q(emb_raw, dtype), tgt.clone()


def mp_compare(out, name, S, V, Fd, dtype, sigma=5.0, want_split=None, labels=None, bad=None, zero_p=None, zero_e=None):
    """one MaskedPredLossFn.apply(proj, emb, target, 0.1, True) against mp_reference, and the head's kernels one by one through
    direct calls on the same inputs: l2norm rows and inverse norms; the logits GEMM on the device's own stored rows; ce_rows'
    verdict per row against the fp64 verdict on those stored rows, outside the band of twice the fp32 dot-product bound
    gamma_F |a| |b| / temp for unit rows; its gradient and the pad columns [V, roundup(V, 8)) in a NaN-filled buffer.
    want_split: the split of the label-embedding gradient this shape is here for (asserted on the full grid of 256 blocks).
    bad {row: label}: labels outside [0, V); zero_p / zero_e: a proj / an emb row set to zero, compared on its own (its
    1 / eps gradient would set the scale of the whole tensor).  Returns what the follow-up lines of a case need."""
    f32 = torch.float32
    tol, temp = tol_for(dtype), MP_TEMP
    proj, emb, tgt = mp_inputs(S, V, Fd, dtype, sigma, labels)
    for r, lab in (bad or {}).items():
        tgt[r] = lab
    if zero_p is not None:
        proj[zero_p] = 0.0
    if zero_e is not None:
        emb[zero_e] = 0.0
    pd, ed, td = proj.to(dtype).to(DEV), emb.to(dtype).to(DEV), tgt.to(DEV)
    t32 = td.to(torch.int32)
    valid = (td >= 0) & (td < V)
    kp = torch.ones(S, dtype=torch.bool, device=DEV)
    ke = torch.ones(V, dtype=torch.bool, device=DEV)
    if zero_p is not None:
        kp[zero_p] = False
    if zero_e is not None:
        ke[zero_e] = False
    split = ops.pick_split(V, Fd, (S + 63) // 64)
    tag = f"masked_pred_head[{'fp32' if dtype == f32 else 'bf16'}] {name}S={S} V={V} F={Fd} split={split}"
    if want_split is not None and ops.grid_blocks() == 256:
        out.append((tag + f" premise: the label-embedding gradient runs with split {want_split}", 0.0 if split == want_split else 1.0, 0.0))
    else:
        out.append((tag + f" the label-embedding gradient ran with split {split} on a grid of {ops.grid_blocks()} blocks", 0.0, 0.0))
    # ---- the fp64 reference from the un-normalised inputs, and the premise that the counter has something to count
    lossr, l64, gp, ge = mp_reference(pd.double(), ed.double(), td, temp, keep=valid if bad else None)
    gap = mp_gap(l64, td, valid)
    nref = int((gap >= 0).sum().item())
    frac = nref / max(int(valid.sum().item()), 1)
    out.append((tag + f" premise: the fp64 reference counts {100 * frac:.1f} % of the rows correct, within [40, 90]", 0.0 if 0.4 <= frac <= 0.9 else 1.0, 0.0))
    # ---- the autograd function
    pg, eg = pd.clone().requires_grad_(True), ed.clone().requires_grad_(True)
    loss, nc = F.MaskedPredLossFn.apply(pg, eg, t32, temp, True)
    dproj, demb = torch.autograd.grad((loss * MP_GRAD).sum(), (pg, eg))
    if bad:
        out.append((tag + " loss is NaN", 0.0 if bool(torch.isnan(loss).all()) else 1.0, 0.0))
        out.append((tag + " dproj on the rows with a label outside [0, V) (non-zero elements)", float((dproj[~valid] != 0).sum().item()), 0.0))
    else:
        out.append((tag + " loss", errd(loss, lossr.reshape(1)), tol))
    out.append((tag + " dproj", errd(dproj[kp & valid], gp[kp & valid]), 3 * tol))
    out.append((tag + " demb", errd(demb[ke], ge[ke]), 3 * tol))
    if zero_p is not None:
        out.append((tag + " dproj, the zero row on its own", errd(dproj[~kp], gp[~kp]), 3 * tol))
    if zero_e is not None:
        out.append((tag + " demb, the zero row on its own", errd(demb[~ke], ge[~ke]), 3 * tol))
    diff = abs(int(round(nc.item())) - nref)
    if dtype == f32:
        k = int(((gap.abs() < 8.0 * 2.0 ** -23 * l64.abs().max(-1).values) & valid).sum().item())
        out.append((tag + f" n_correct (beyond the {k} near-tie rows)", float(max(0, diff - k)), 0.0))
        out.append((tag + f" near-tie rows: {k} of {S} (cap 0.1 %)", k / S, 1e-3))
    else:
        out.append((tag + " n_correct", float(diff), max(2.0, 0.02 * S)))
    # ---- the kernels one by one
    pn, inv_p = ops.l2norm_fwd(pd, dtype)
    en, inv_e = ops.l2norm_fwd(ed, dtype)
    for nm, y, inv, x64, kk in (("proj", pn, inv_p, pd.double(), kp), ("emb", en, inv_e, ed.double(), ke)):
        nr = x64.norm(dim=-1).clamp_min(1e-8)
        out.append((tag + f" l2norm {nm} rows", errd(y, x64 / nr[:, None]), tol))
        out.append((tag + f" l2norm {nm} inv_norm", errd(inv[kk], 1.0 / nr[kk]), tol))
        if not bool(kk.all()):
            out.append((tag + f" l2norm {nm} inv_norm of the zero row", errd(inv[~kk], 1.0 / nr[~kk]), tol))
    lg = torch.full((S, V), float("nan"), dtype=f32, device=DEV)
    ops.gemm(pn, en, lg, S, V, Fd, lda=Fd, ldb=Fd, ldc=V, alpha=1.0 / temp)
    ls64 = pn.double() @ en.double().t() / temp
    out.append((tag + " logits from the stored rows", errd(lg, ls64), TOL32))
    ldd = (V + 7) // 8 * 8
    dlog = torch.full((S, ldd), float("nan"), dtype=dtype, device=DEV)
    _, corr = ops.ce_rows(lg, t32, V, V, dlog, ldd, 1.0)
    gs = mp_gap(ls64, td, valid)
    band = gs.abs() < 2.0 * Fd * 2.0 ** -24 / temp * 1.01
    nb = int(band.sum().item())
    out.append((tag + f" correct, row by row (mismatches outside the {nb} rows within 2 F 2^-24 / temp of a tie)",
                float(((corr.bool() != (gs >= 0)) & ~band).sum().item()), 0.0))
    out.append((tag + f" rows within that band: {nb} of {S} (cap 0.5 %)", nb / S, 5e-3))
    dref = torch.softmax(lg.double(), -1)
    dref[torch.arange(S, device=DEV), td.clamp(0, V - 1)] -= 1.0
    dref[~valid] = 0.0
    out.append((tag + " d loss / d logit from the device logits", errd(dlog[:, :V], dref), tol))
    out.append((tag + f" pad columns [{V}, {ldd}) of d loss / d logit (non-zero elements)", float((dlog[:, V:] != 0).sum().item()), 0.0))
    return dict(tag=tag, pd=pd, ed=ed, t32=t32, td=td, loss=loss, nc=nc, dproj=dproj, demb=demb, gp=gp, ge=ge)


def mp_glu_case(out, dtype, S=1029, V=504, Fd=256, sigma=2.5):
    """target_glu as pretrain.py composes it: emb = GLUFn(LinearFn(table[V, F], W[2F, F], b)), then the loss; against the same
    composition in fp64.  proj is drawn around the rows of the fp64 GLU output (about half the scale of the table: sigma
    follows it)."""
    tol = tol_for(dtype)
    table = q(gen(V, Fd, seed=11), dtype)
    W = q(gen(2 * Fd, Fd, seed=12, scale=1.0 / math.sqrt(Fd)), dtype)
    b = q(0.1 * gen(2 * Fd, seed=13), dtype)
    tgt = torch.randint(0, V, (S,), generator=torch.Generator().manual_seed(3))
    proj = q(TF.glu(TF.linear(table.double(), W.double(), b.double()), -1).float()[tgt] + sigma * gen(S, Fd, seed=2), dtype)
    td = tgt.to(DEV)
    ref = [t.to(DEV).double().requires_grad_(True) for t in (proj, table, W, b)]
    e64 = TF.glu(TF.linear(ref[1], ref[2], ref[3]), -1)
    l64 = TF.normalize(ref[0], dim=-1, eps=1e-8) @ TF.normalize(e64, dim=-1, eps=1e-8).t() / MP_TEMP
    lossr = TF.cross_entropy(l64, td, reduction="sum")
    gr = torch.autograd.grad(MP_GRAD * lossr, ref)
    frac = (mp_gap(l64.detach(), td, torch.ones_like(td, dtype=torch.bool)) >= 0).double().mean().item()
    dev = [t.to(dtype).to(DEV).requires_grad_(True) for t in (proj, table, W, b)]
    embd = F.GLUFn.apply(F.LinearFn.apply(dev[1].contiguous(), dev[2], dev[3]))
    loss, _ = F.MaskedPredLossFn.apply(dev[0], embd, td.to(torch.int32), MP_TEMP, True)
    gd = torch.autograd.grad((loss * MP_GRAD).sum(), dev)
    tag = f"masked_pred_head[{'fp32' if dtype == torch.float32 else 'bf16'}] target_glu S={S} V={V} F={Fd}"
    out.append((tag + f" premise: the fp64 reference counts {100 * frac:.1f} % of the rows correct, within [40, 90]", 0.0 if 0.4 <= frac <= 0.9 else 1.0, 0.0))
    out.append((tag + " loss", errd(loss, lossr.detach().reshape(1)), tol))
    for nm, a, r in zip(("dproj", "dtable", "dW", "db"), gd, gr):
        out.append((tag + " " + nm, errd(a, r), 3 * tol))


@leaves_no_footprint
def check_masked_pred_head():
    """functional.MaskedPredLossFn (l2norm twice, the logits GEMM, ce_rows, sum_f32 twice, the two backward GEMMs -- the label-
    embedding one transA, transB with split-K over the S rows -- l2norm backward twice) against fp64 torch on the device at
    the row counts of training: the smallest S for each split of the label-embedding gradient (2: S = 1029 with a ragged first
    K tile; 25: a Base step's 12 805 masked rows; 64, the slab cap: 32 773 rows, which also takes every row kernel of the head
    past its grid cap of 4 x 8192 rows), F = 768, V = 100 (the 128-wide kernel's split policy, ldd = 104), V = 500 (ldd = 504),
    V = 1000, and the floor (5, 2, 8); then skewed labels, labels outside [0, V), zero rows, the paths without a gradient, and
    target_glu.  Inputs are a table and projections scattered around their label's row, so that the fp64 reference counts 40
    to 90 % of the rows correct (asserted per case) and `correct` is compared row by row.
    Tolerances: TOL32 / TOLBF on the tensor scale, three times that for gradients, as check_loss.  An emulation of the bf16 path
    on the CPU (stored bf16 pn, en, dlogits; fp32 accumulation) lies within 1.1e-2 (dproj) and 8.7e-3 (demb) of fp64 at all of
    these shapes, about a sixth of the 6e-2 allowed.
    (gemm_split_range gives every slab ceil(tiles / split) K tiles, so at split 25 and 64 the last slabs hold no tile and are
    all zero: a reduction that drops the LAST slab shows in demb at split 2, 4 and 24 only, one that drops the first at all.)"""
    out = []
    f32, bf = torch.float32, torch.bfloat16
    cases = [  # S, V, F, sigma, split asserted on the full grid
        (1029, 504, 256, 5.0, 2), (12805, 504, 256, 5.0, 25), (LOSS_ROWS, 504, 256, 5.0, 64), (2053, 504, 768, 8.0, 4),
        (1500, 100, 256, 5.0, None), (1029, 500, 256, 5.0, None), (1029, 1000, 256, 4.0, None), (5, 2, 8, 8.0, None)]   # the floor: 3 of its 5 rows correct
    S, V, Fd = 1029, 504, 256
    for dtype in (f32, bf):
        tol = tol_for(dtype)
        plain = None
        for (s_, v_, f_, sigma, want) in cases:
            r = mp_compare(out, "", s_, v_, f_, dtype, sigma=sigma, want_split=want)
            plain = plain or r   # (1029, 504, 256): the shape of everything below
        # skewed labels: label 7 on 60 % of the rows, the labels 304 .. 503 on none; the gradient of a label that never occurs
        # is the pure softmax term, a hundredth of row 7's, so those rows are also compared on their own scale
        n7 = (3 * S + 4) // 5
        rest = torch.randperm(304, generator=torch.Generator().manual_seed(4)).repeat(2)[:S - n7]
        labels = torch.cat([torch.full((n7,), 7), rest])[torch.randperm(S, generator=torch.Generator().manual_seed(5))]
        cnt = torch.bincount(labels, minlength=V)
        r = mp_compare(out, "skewed labels ", S, V, Fd, dtype, labels=labels)
        out.append((r["tag"] + f" premise: label 7 on {int(cnt[7])} rows (>= 60 %), {int((cnt == 0).sum())} of {V} labels never occur (200)",
                    0.0 if cnt[7] >= 0.6 * S and int((cnt == 0).sum()) == 200 else 1.0, 0.0))
        never = (cnt == 0).to(DEV)
        out.append((r["tag"] + " demb on the labels that never occur, on their own scale", errd(r["demb"][never], r["ge"][never]), 3 * tol))
        # labels outside [0, V): NaN loss, a zero gradient row, and the other rows' gradients as if those rows were not there
        mp_compare(out, "labels -1, V, V + 1000 ", S, V, Fd, dtype, bad={3: -1, 500: V, S - 1: V + 1000})
        # the max(||x||, eps) clamp: a zero proj row (all its logits 0: a tie, counted as correct by both) and a zero emb row
        r = mp_compare(out, "zero rows ", S, V, Fd, dtype, zero_p=11, zero_e=5)
        fin = all(bool(torch.isfinite(r[k]).all()) for k in ("loss", "dproj", "demb"))
        out.append((r["tag"] + " loss and gradients finite", 0.0 if fin else 1.0, 0.0))
        # without a gradient: the same two numbers, bit for bit; no rows: zeros
        r = plain
        with torch.no_grad():
            loss0, nc0 = F.MaskedPredLossFn.apply(r["pd"], r["ed"], r["t32"], MP_TEMP, False)
        out.append((r["tag"] + " need_grad=False: loss, bit for bit", same_bits(loss0, r["loss"].detach()), 0.0))
        out.append((r["tag"] + " need_grad=False: n_correct, bit for bit", same_bits(nc0, r["nc"]), 0.0))
        pe = torch.empty((0, Fd), dtype=dtype, device=DEV, requires_grad=True)
        eg = r["ed"].clone().requires_grad_(True)
        lz, nz = F.MaskedPredLossFn.apply(pe, eg, torch.empty(0, dtype=torch.int32, device=DEV), MP_TEMP, True)
        gz = torch.autograd.grad((lz * MP_GRAD).sum(), (pe, eg))
        tag = f"masked_pred_head[{'fp32' if dtype == f32 else 'bf16'}] S=0 V={V} F={Fd}"
        out.append((tag + " loss and n_correct are zero", float(lz.abs().sum().item() + nz.abs().sum().item()), 0.0))
        ok = gz[0].shape == pe.shape and gz[1].shape == eg.shape and gz[0].dtype == dtype and gz[1].dtype == dtype
        out.append((tag + " gradients have the inputs' shapes and dtype", 0.0 if ok else 1.0, 0.0))
        out.append((tag + " demb (non-zero elements)", float((gz[1] != 0).sum().item()), 0.0))
        mp_glu_case(out, dtype)
    return out


@leaves_no_footprint
def check_loss_rows_capped():
    """every other entry point of loss.hip at the smallest size past its grid cap plus a ragged tail (the constants above
    name the caps), element by element against fp64 torch on the device: the second sweep of each grid-stride loop and the
    row * ld index arithmetic on it.  l2norm rows carry scales 1 .. 7 with a period that does not divide 32 768, so that a row
    of the second sweep which reads another row's inverse norm is off by a factor; the all-equal logit row, the repeated
    positive, the empty CSR rows and the tails of the two reductions lie past the cap on purpose.
    Tolerances: tol_for(dtype) for stored tensors, TOL32 for fp32 rows and sums."""
    out = []
    f32, bf = torch.float32, torch.bfloat16
    nan, inf = float("nan"), float("inf")
    rows, first2 = LOSS_ROWS, 4 * LOSS_ROW_BLOCKS
    ar = torch.arange(rows, device=DEV)
    past = ar >= first2
    dn = {f32: "fp32", bf: "bf16"}
    # ---- l2norm_fwd / l2norm_bwd: D = 256 (four full 64-column passes), D = 100 (lanes 36 .. 63 idle in the second pass)
    for D in (256, 100):
        raw, draw = dgen(rows, D, seed=1) * (1 + ar % 7)[:, None], dgen(rows, D, seed=2)
        for ti, to in ((f32, f32), (bf, bf), (f32, bf)):
            tag = f"loss_rows_capped l2norm[{dn[ti]} -> {dn[to]}] {rows}x{D}"
            x = q(raw, ti)
            x64 = x.double().requires_grad_(True)
            yr = TF.normalize(x64, dim=-1, eps=1e-8)
            y, inv = ops.l2norm_fwd(x.to(ti), to)
            out.append((tag + " y", errd(y, yr), tol_for(to)))
            out.append((tag + " inv_norm", errd(inv, 1.0 / x64.detach().norm(dim=-1).clamp_min(1e-8)), TOL32))
            dy = q(draw, to)
            (dxr,) = torch.autograd.grad(yr, x64, dy.double())
            dx = ops.l2norm_bwd(dy.to(to), y, inv, ti)
            tb = TOLBF if bf in (ti, to) else TOL32
            out.append((tag + " dx", errd(dx, dxr), tb))
            out.append((tag + f" dx, the rows from {first2} on their own", errd(dx[past], dxr[past]), tb))
    # ---- ce_rows: 101 columns (two 64-lane passes) in rows of 104, NaN in the pads, -inf in a tenth of the non-target columns,
    # the target raised on every other row (so that half the rows are correct), an all-equal row in the second sweep
    S, V, ld = rows, 101, 104
    gi = torch.Generator(device=DEV).manual_seed(620)
    lgt = torch.full((S, ld), nan, device=DEV)
    lgt[:, :V] = 4.0 * torch.randn(S, V, generator=gi, device=DEV)
    tgt = torch.randint(0, V, (S,), generator=gi, device=DEV)
    minf = torch.rand(S, V, generator=gi, device=DEV) < 0.1
    minf[ar, tgt] = False
    lgt[:, :V].masked_fill_(minf, -inf)
    lgt[ar, tgt] = torch.where(ar % 2 == 1, lgt[:, :V].max(-1).values + 1.0, lgt[ar, tgt])
    flat_row = first2 + 2
    lgt[flat_row, :V] = 1.25
    l64 = lgt[:, :V].double().requires_grad_(True)
    rows_ref = TF.cross_entropy(l64, tgt, reduction="none")
    (dref,) = torch.autograd.grad(rows_ref.sum() * 1.7, l64)
    mx = l64.detach().max(-1).values
    hit = l64.detach()[ar, tgt] >= mx
    all_equal = l64.detach().min(-1).values == mx
    out.append((f"loss_rows_capped ce_rows premise: {int(hit.sum())} of {S} rows correct (40 to 60 %), one all-equal row, at {flat_row}",
                0.0 if 0.4 * S <= int(hit.sum()) <= 0.6 * S and int(all_equal.sum()) == 1 and bool(all_equal[flat_row]) else 1.0, 0.0))
    for ddt in (f32, bf):
        tag = f"loss_rows_capped ce_rows {S}x{V} ld={ld} dlogits[{dn[ddt]}]"
        dlog = torch.full((S, ld), nan, dtype=ddt, device=DEV)
        for flat in (False, True):
            lrows, corr = ops.ce_rows(lgt, tgt.to(torch.int32), V, ld, dlog, ld, 1.7, flat_wrong=flat)
            cref = hit & ~all_equal if flat else hit
            out.append((tag + f" flat_wrong={flat}: correct rows (mismatches)", float((corr.bool() != cref).sum().item()), 0.0))
            out.append((tag + f" flat_wrong={flat}: loss rows", errd(lrows, rows_ref), TOL32))
        out.append((tag + " dlogits", errd(dlog[:, :V], dref), tol_for(ddt)))
        out.append((tag + " pad columns (non-zero elements)", float((dlog[:, V:] != 0).sum().item()), 0.0))
    # ---- gather_dot: 3 columns (the row itself, two draws); in the second sweep, the positive's own row among the negatives
    # and another row of y with the positive's content
    S, N, D = rows, 3, 64
    idx = torch.randint(0, S, (S, N), generator=gi, device=DEV)
    idx[:, 0] = ar
    own, twin = first2 + 2, first2 + 3
    idx[own, 2] = own
    idx[twin, 1] = 100
    i32 = idx.to(torch.int32)
    for dtype in (f32, bf):
        tag = f"loss_rows_capped gather_dot[{dn[dtype]}] S={S} N={N} D={D}"
        X, Y = q(dgen(S, D, seed=11), dtype), q(dgen(S, D, seed=12), dtype)
        Y[100] = Y[twin]
        ref = 10.0 * (X.double()[:, None, :] * Y.double()[idx]).sum(-1)
        mref = torch.zeros((S, N), dtype=torch.bool, device=DEV)
        mref[:, 1:] = (Y[idx[:, 1:]] == Y[idx[:, :1]]).all(-1)
        Xd, Yd = X.to(dtype), Y.to(dtype)
        lg0 = ops.gather_dot(Xd, Yd, i32, 10.0)
        lg1 = ops.gather_dot(Xd, Yd, i32, 10.0, mask_raw=Yd)
        mdev = torch.isinf(lg1) & (lg1 < 0)
        out.append((tag + " without mask_raw", errd(lg0, ref), TOL32))
        out.append((tag + f" premise: the reference masks ({own}, 2) and ({twin}, 1)", 0.0 if bool(mref[own, 2]) and bool(mref[twin, 1]) else 1.0, 0.0))
        out.append((tag + f" with mask_raw: -inf placement ({int(mref.sum())} masked in the reference; differing positions)", float((mref != mdev).sum().item()), 0.0))
        out.append((tag + " with mask_raw: the other logits", errd(torch.where(mdev, torch.zeros_like(lg1), lg1), torch.where(mref, torch.zeros_like(ref), ref)), TOL32))
    # ---- rows_wsum: a CSR with row % 4 entries per row (rows 32 768 and 32 772 are empty), every operand / result dtype pair
    D, R = 64, 1000
    cnt = ar % 4
    off = torch.zeros(rows + 1, dtype=torch.int32, device=DEV)
    off[1:] = torch.cumsum(cnt, 0).to(torch.int32)
    E = int(off[-1].item())
    src = torch.randint(0, R, (E,), generator=gi, device=DEV).to(torch.int32)
    w = dgen(E, seed=22)
    rowid = torch.repeat_interleave(ar, cnt)
    empty_past = past & (cnt == 0)
    for ydt, odt in ((f32, f32), (bf, bf), (bf, f32), (f32, bf)):
        tag = f"loss_rows_capped rows_wsum[{dn[ydt]} -> {dn[odt]}] {rows}x{D}"
        Y = q(dgen(R, D, seed=21), ydt)
        ref = torch.zeros((rows, D), dtype=torch.float64, device=DEV).index_add_(0, rowid, w.double()[:, None] * Y.double()[src.long()])
        o = torch.full((rows, D), nan, dtype=odt, device=DEV)
        ops.rows_wsum(Y.to(ydt), src, w, off, rows, out=o, accumulate=False)
        out.append((tag + " fresh", errd(o, ref), tol_for(odt)))
        out.append((tag + f" fresh: the {int(empty_past.sum())} empty rows from {first2} (non-zero elements)", float((o[empty_past] != 0).sum().item()), 0.0))
        o0 = q(dgen(rows, D, seed=23), odt)
        o = o0.to(odt).clone()
        ops.rows_wsum(Y.to(ydt), src, w, off, rows, out=o, accumulate=True)
        out.append((tag + " accumulated", errd(o, o0.double() + ref), tol_for(odt)))
    # ---- glu_fwd / glu_bwd: one row per block; F = 48 (one partly filled 256-column pass), F = 300 (the second pass ragged)
    for dtype in (f32, bf):
        tol = tol_for(dtype)
        for Fh in (48, 300):
            x, dy = q(2.0 * dgen(GLU_ROWS, 2 * Fh, seed=31), dtype), q(dgen(GLU_ROWS, Fh, seed=32), dtype)
            for gate, g in GLU_GATE_REFS.items():
                xr = x.double().requires_grad_(True)
                yr = xr[:, :Fh] * g(xr[:, Fh:])
                (dxr,) = torch.autograd.grad(yr, xr, dy.double())
                tag = f"loss_rows_capped glu[{dn[dtype]}] {gate} {GLU_ROWS}x{Fh}"
                out.append((tag + " fwd", errd(ops.glu_fwd(x.to(dtype), gate), yr), tol))
                out.append((tag + " bwd", errd(ops.glu_bwd(x.to(dtype), dy.to(dtype), gate), dxr), tol))
        # ---- act_fwd / act_bwd: 256 elements per block
        x, dy = q(2.0 * dgen(ACT_N, seed=41), dtype), q(dgen(ACT_N, seed=42), dtype)
        for kind, f in ACT_REFS.items():
            xr = x.double().requires_grad_(True)
            yr = f(xr)
            (dxr,) = torch.autograd.grad(yr, xr, dy.double())
            tag = f"loss_rows_capped act[{dn[dtype]}] {kind} n={ACT_N}"
            out.append((tag + " fwd", errd(ops.act_fwd(x.to(dtype), kind), yr), tol))
            out.append((tag + " bwd", errd(ops.act_bwd(x.to(dtype), dy.to(dtype), kind), dxr), tol))
    # ---- sum_f32: mean 1, so that a dropped sweep shows; the five elements of the ragged ninth sweep weigh 5 / n = 2.4e-6 of
    # the sum at that mean, below TOL32, so a second sum carries 1000 on each of them (2.4e-3 of the sum)
    n = RED_N
    x = 1.0 + dgen(n, seed=51)
    out.append((f"loss_rows_capped sum_f32 n={n}", errd(ops.sum_f32(x), x.double().sum().reshape(1)), TOL32))
    x[-5:] += 1000.0
    out.append((f"loss_rows_capped sum_f32 n={n}, 1000 on each of the last five", errd(ops.sum_f32(x), x.double().sum().reshape(1)), TOL32))
    # ---- bce_logits: the last five elements are classified correctly by construction, so that the exact count sees the tail
    lg = 2.0 * dgen(n, seed=52)
    t = torch.rand(n, generator=gi, device=DEV) < 0.3
    t[-5:] = lg[-5:] >= 0
    l64 = lg.double()
    gscale = 0.37
    res, dl = ops.bce_logits(lg, t.to(torch.uint8), gscale, want_grad=True)
    res0, dl0 = ops.bce_logits(lg, t.to(torch.uint8), gscale, want_grad=False)
    count = int(((l64 >= 0) == t).sum().item())
    tag = f"loss_rows_capped bce_logits n={n}"
    out.append((tag + " mean loss", errd(res[0:1], TF.binary_cross_entropy_with_logits(l64, t.double()).reshape(1)), TOL32))
    out.append((tag + f" accuracy x n against the fp64 count {count}", float(abs(round(res[1].item() * n) - count)), 0.0))
    out.append((tag + " dlogits", errd(dl, gscale * (torch.sigmoid(l64) - t.double())), TOL32))
    out.append((tag + " want_grad=False: no dlogits, the same loss and accuracy bit for bit", 0.0 if dl0 is None else 1.0, 0.0))
    out.append((tag + " want_grad=False: loss and accuracy", same_bits(res0, res), 0.0))
    return out


# ------------------------------------------------------------------------ pos_conv at batch geometry (module docstring)
PCD_TILES = {48: (768, 512, 384), 64: (512, 384)}   # candidate frame tiles of posconv_direct_kernel (64 MT), larger first
PDW_TCH = {48: 256, 64: 128}                        # frames per chunk of posconv_dw_kernel
PDW_BS = {48: 4, 64: 2}                             # batch splits (fp32 slabs) of posconv_dw_kernel
GM_CAP = 8192 * 256                                 # 8-element chunks one sweep of pc_group_major_kernel's grid covers


def posconv_direct_tile(Cg, T):
    """(frames per workgroup, segments) wavlm_posconv_direct launches at T frames: the candidate tile that pads T the least,
    the larger one on a tie (min() keeps the first of equals)"""
    bm = min(PCD_TILES[Cg], key=lambda m: -(-T // m) * m)
    return bm, -(-T // bm)


def posconv_dw_geometry(Cg, B, T):
    """(bchunk, batches per split, chunks per batch, frames in the last chunk) of posconv_dw_kernel"""
    BS, TCH = PDW_BS[Cg], PDW_TCH[Cg]
    bchunk = -(-B // BS)
    per = tuple(max(0, min(B, (s + 1) * bchunk) - s * bchunk) for s in range(BS))
    nch = -(-T // TCH)
    return bchunk, per, nch, T - (nch - 1) * TCH


def posconv_ref64(x, v, g, bias, G):
    """x + gelu(conv1d(x, g v / ||v||, padding K // 2, groups G) + bias)[:, :T] as a loop over the K taps of a grouped
    matrix product on the zero-padded x -- the reference's SamePad for odd and even K.  Shares nothing with the code under
    test and asks no convolution of the vendor library; autograd differentiates it."""
    B, T, D = x.shape
    Cg, K = v.shape[1], v.shape[2]
    P = K // 2
    w = (g.view(1, 1, K) * v / v.norm(dim=(0, 1), keepdim=True)).view(G, Cg, Cg, K)   # [group, column, channel, tap]
    xp = TF.pad(x, (0, 0, P, P)).view(B, T + 2 * P, G, Cg)
    L = T + 2 * P - K + 1          # frames the padded convolution gives: T + 1 for even K, T for odd
    u = x.new_zeros(B, L, G, Cg)
    for k in range(K):
        u = u + torch.einsum("btgc,gnc->btgn", xp[:, k:k + L], w[..., k])
    return x + TF.gelu(u.reshape(B, L, D)[:, :T] + bias)


def pc_inputs(B, T, D, K, G, dtype):
    """check_posconv's distributions, drawn on the device and rounded through dtype: x, v, g, bias, dy"""
    Cg = D // G
    x = q(dgen(B, T, D, seed=1), dtype)
    v = q(dgen(D, Cg, K, seed=2, scale=math.sqrt(4.0 / (K * D))), dtype)
    g = q(v.norm(dim=(0, 1), keepdim=True) * (1 + 0.1 * dgen(1, 1, K, seed=3)), dtype)
    bias = q(0.1 * dgen(D, seed=4), dtype)
    dy = q(dgen(B, T, D, seed=5), dtype)
    return x, v, g, bias, dy


def pc_ref(inp, G, more_dy=()):
    """(y, [(dx, dv, dg, dbias) for inp's dy and every further dy]) in fp64 on the device"""
    x, v, g, bias, dy = inp
    leaves = [t.double().requires_grad_(True) for t in (x, v, g, bias)]
    y = posconv_ref64(*leaves, G)
    return y.detach(), [torch.autograd.grad(y, leaves, d.double(), retain_graph=True) for d in (dy,) + tuple(more_dy)]


def pc_device(inp, G, dtype, dy=None, x_grad=True, direct=True):
    """PosConvFn forward and backward on copies of the inputs in dtype -> (y, (dx, dv, dg, dbias))"""
    x, v, g, bias, dy0 = inp
    xd = x.to(dtype, copy=True).requires_grad_(x_grad)
    vd, gd, bd = [t.to(dtype, copy=True).requires_grad_(True) for t in (v, g, bias)]
    old = F.POSCONV_DIRECT
    F.POSCONV_DIRECT = old and direct
    try:
        yd = F.PosConvFn.apply(xd, vd, gd, bd, G)
        yd.backward(dy0.to(dtype) if dy is None else dy)
    finally:
        F.POSCONV_DIRECT = old
    return yd.detach(), (xd.grad, vd.grad, gd.grad, bd.grad)


def pc_lines(out, tag, got, ref, tol, names=("dx", "dv", "dg", "dbias")):
    """check_posconv's bounds: y at tol, dx and dbias at twice, dv and dg at three times that"""
    (y, grads), (yr, gr) = got, ref
    if y is not None:
        out.append((tag + " y", errd(y, yr), tol))
    for nm, a, b in zip(("dx", "dv", "dg", "dbias"), grads, gr):
        if nm in names:
            out.append((f"{tag} {nm}", errd(a, b) if a is not None else float("inf"), tol * (3 if nm in ("dv", "dg") else 2)))


def pc_direct_case(out, tag, B, T, D, G, dtype=torch.bfloat16, K=128, more_dy=None):
    """one shape on the direct kernels: the five outputs against fp64, and against the GEMM form on the same inputs.
    more_dy(inputs) names further output gradients for the one reference graph.  Returns (inputs, (y, gradient sets), device run)"""
    inp = pc_inputs(B, T, D, K, G, dtype)
    ref = pc_ref(inp, G, more_dy(inp) if more_dy else ())
    got = pc_device(inp, G, dtype)
    pc_lines(out, tag, got, (ref[0], ref[1][0]), tol_for(dtype))
    alt = pc_device(inp, G, dtype, direct=False)
    for nm, a, b in (("y", got[0], alt[0]), ("dx", got[1][0], alt[1][0]), ("dv", got[1][1], alt[1][1])):
        out.append((f"{tag} direct vs gemm {nm}", errd(a, b), 1.0e-2))
    return inp, ref, got


def pc_tail_dy(dy, first):
    """dy with the frames before `first` zeroed"""
    d = dy.clone()
    d[:, :first] = 0
    return d


def pc_direct_premise(Cg, G, T, K=128):
    ok = F.POSCONV_DIRECT and ops.posconv_direct_supported(torch.bfloat16, Cg, K, T) and ops._lib.lib().wavlm_posconv_dw_direct_splits(Cg, G) > 0
    return 0.0 if ok else 1.0


# Cg, D, B, T and what posconv_dw_kernel makes of them: bchunk, batches per split, chunks per batch, frames in the last chunk
PC_BATCH_CASES = [
    (48, 768, 5, 300, 2, (2, 2, 1, 0), 2, 44),     # a partial and an empty split; a 44-frame tail chunk
    (48, 768, 8, 257, 2, (2, 2, 2, 2), 2, 1),      # all four splits full; a tail chunk of one frame
    (48, 768, 9, 64, 3, (3, 3, 3, 0), 1, 64),      # three batches per workgroup, one chunk each
    (64, 1024, 3, 200, 2, (2, 1), 2, 72),          # TCH = 128: two chunks per batch
    (64, 1024, 5, 129, 3, (3, 2), 2, 1),           # a tail chunk of one frame
]


@leaves_no_footprint
def check_posconv_batch():
    """PosConvFn on the direct kernels (bf16, K = 128, G = 16) where a workgroup of posconv_dw_kernel walks several batches:
    `bb` advances, a split is partial or empty, and the register stage crosses from one batch's last chunk to the next
    batch's first.  Reference: posconv_ref64.  A one-frame tail chunk is 1 / 257 of a weight gradient's terms, about the
    size of the dv bound, so the shapes with a tail also run a backward whose dy is zero outside the last chunk: there a lost
    chunk is the whole gradient.  At (5, 300): the inference forward, a backward without dx, a non-contiguous dy."""
    out = []
    dtype, G = torch.bfloat16, 16
    tol = tol_for(dtype)
    for i, (Cg, D, B, T, bchunk, per, nch, tail) in enumerate(PC_BATCH_CASES):
        tag = f"posconv_batch Cg={Cg} B={B} T={T}"
        out.append((tag + " premise: the direct kernels take it", pc_direct_premise(Cg, G, T), 0.0))
        out.append((tag + f" premise: bchunk {bchunk}, splits of {per} batches, {nch} chunk(s), {tail} frame(s) in the last",
                    0.0 if posconv_dw_geometry(Cg, B, T) == (bchunk, per, nch, tail) else 1.0, 0.0))
        first = (nch - 1) * PDW_TCH[Cg]   # first frame of the last chunk
        inp, (yr, sets), got = pc_direct_case(out, tag, B, T, D, G, more_dy=(lambda I: [pc_tail_dy(I[4], first)]) if nch > 1 else None)
        if nch > 1:
            gt = pc_device(inp, G, dtype, dy=pc_tail_dy(inp[4], first).to(dtype))
            pc_lines(out, tag + f", dy zero outside the last {tail} frame(s):", (None, gt[1]), (yr, sets[1]), tol)
        if i == 0:
            with torch.no_grad():
                yi = F.infer_apply(F.PosConvFn, *[t.to(dtype) for t in inp[:4]], G)
            out.append((tag + " inference forward (no pre-activation kept) == training forward, bit for bit", same_bits(yi, got[0]), 0.0))
            gn = pc_device(inp, G, dtype, x_grad=False)
            out.append((tag + " x.requires_grad == False: dx is None", 0.0 if gn[1][0] is None else 1.0, 0.0))
            pc_lines(out, tag + " x.requires_grad == False:", (None, gn[1]), (yr, sets[0]), tol, names=("dv", "dg", "dbias"))
            dync = inp[4].to(dtype).transpose(0, 1).contiguous().transpose(0, 1)
            out.append((tag + " premise: that dy is not contiguous", 0.0 if not dync.is_contiguous() else 1.0, 0.0))
            gc = pc_device(inp, G, dtype, dy=dync)
            pc_lines(out, tag + " non-contiguous dy:", (None, gc[1]), (yr, sets[0]), tol)
    return out


# T -> (frame tile, segments) that posconv_direct_tile is meant to give, per group width; (D, G) are the smallest with the
# direct weight-gradient kernel
PC_FRAME_DG = {48: (96, 2), 64: (256, 4)}
PC_FRAME_CASES = {
    48: [(1, 384, 1), (16, 384, 1), (63, 384, 1), (127, 384, 1),       # T < K: the window is mostly padding
         (383, 384, 1), (384, 384, 1),                                 # the smallest tile, one short and exact
         (385, 512, 1), (512, 512, 1),                                 # the middle tile
         (513, 768, 1),                                                # 768 = 2 x 384 padded frames: the tie goes to the larger tile
         (768, 768, 1), (769, 512, 2),                                 # exact, and one past: two segments of 512
         (1153, 768, 2),                                               # 1536 padded frames with every tile: the larger one
         (1537, 384, 5)],                                              # five segments, one frame in the last
    64: [(1, 384, 1), (65, 384, 1), (384, 384, 1), (385, 512, 1), (512, 512, 1),
         (513, 384, 2),                                                # 768 against 1024 padded frames
         (1024, 512, 2),                                               # two exact segments of the larger tile
         (1025, 384, 3), (1537, 384, 5)],
}
PC_FRAME_B2 = {48: 769, 64: 513}   # the multi-segment T that also runs with two batches


@leaves_no_footprint
def check_posconv_frames():
    """the frame-tile edges of posconv_direct_kernel (and the chunk edges of posconv_dw_kernel under them) at small channel
    counts, bf16, K = 128: every tile height, the tie-break, exact multiples and one past, T below K, two to five segments"""
    out = []
    for Cg, cases in PC_FRAME_CASES.items():
        D, G = PC_FRAME_DG[Cg]
        for (T, bm, nseg) in cases:
            for B in (1, 2) if T == PC_FRAME_B2[Cg] else (1,):
                tag = f"posconv_frames Cg={Cg} B={B} T={T}"
                out.append((tag + " premise: the direct kernels take it", pc_direct_premise(Cg, G, T), 0.0))
                out.append((tag + f" premise: {nseg} segment(s) of {bm} frames", 0.0 if posconv_direct_tile(Cg, T) == (bm, nseg) else 1.0, 0.0))
                pc_direct_case(out, tag, B, T, D, G)
    return out


def gelu_grad64(a):
    return 0.5 * (1 + torch.erf(a / math.sqrt(2.0))) + a * torch.exp(-0.5 * a * a) / math.sqrt(2 * math.pi)


def pc_group_major_case(out, tag, B, T, D, G, left_pad, Tp, dtype, poison):
    Cg = D // G
    x = q(dgen(B, T, D, seed=61), dtype).to(dtype)
    a = q(2.0 * dgen(B, T, D, seed=62), dtype).to(dtype)

    def placed(t):
        """the group-major, time-padded image by torch indexing"""
        o = torch.zeros((B, G, Tp, Cg), dtype=t.dtype, device=DEV)
        o[:, :, left_pad:left_pad + T] = t.view(B, T, G, Cg).permute(0, 2, 1, 3)
        return o

    def interior(o):
        return o[:, :, left_pad:left_pad + T].permute(0, 2, 1, 3).reshape(B, T, D)

    def pads(o):
        return float((o[:, :, :left_pad] != 0).sum().item() + (o[:, :, left_pad + T:] != 0).sum().item())

    nbytes = B * G * Tp * Cg * x.element_size()
    if poison:
        _poison(nbytes)
    o, nat = ops.group_major(x, None, G, left_pad, Tp)
    out.append((tag + " plain copy == torch indexing, bit for bit", same_bits(o, placed(x)), 0.0))
    out.append((tag + " plain copy: pad rows (non-zero elements)", pads(o), 0.0))
    out.append((tag + " plain copy: no nat unless asked", 0.0 if nat is None else 1.0, 0.0))
    del o
    for is_grad, ref in ((False, x.double() * gelu_grad64(a.double())), (True, x.double() * a.double())):
        sub = tag + (" x * aux" if is_grad else " x * gelu'(aux)")
        if poison:
            _poison(nbytes)
        o, nat = ops.group_major(x, a, G, left_pad, Tp, want_nat=True, aux_is_grad=is_grad)
        out.append((sub, errd(o, placed(ref)), tol_for(dtype)))
        out.append((sub + ": pad rows (non-zero elements)", pads(o), 0.0))
        out.append((sub + ": nat == the interior rows, bit for bit", same_bits(nat, interior(o)), 0.0))
        del o, nat


def pc_image_offsets(Cg, K, layout):
    """offset inside a group's image of element (column n, tap, channel c), as posconv.hip's pc_weight_kernel states it:
    layout 0 = [n][tap][c]; layout 1 = [c / 8][(tap % 16) / 4][tap / 16][tap % 4][n][c % 8]"""
    n = torch.arange(Cg, device=DEV).view(Cg, 1, 1)
    tap = torch.arange(K, device=DEV).view(1, K, 1)
    c = torch.arange(Cg, device=DEV).view(1, 1, Cg)
    if layout == 0:
        return ((n * K + tap) * Cg + c).reshape(-1)
    J = K // 16
    return (((((c // 8 * 4 + tap % 16 // 4) * J + tap // 16) * 4 + tap % 4) * Cg + n) * 8 + c % 8).reshape(-1)


def pc_weight_ref(v, g):
    """fp64: norm [K], w [D, Cg, K]"""
    norm = v.double().norm(dim=(0, 1))
    return norm, g.double().view(1, 1, -1) * v.double() / norm


def pc_weight_fwd_case(out, D, Cg, K, layout, pdt, odt):
    dn = {torch.float32: "fp32", torch.bfloat16: "bf16"}
    tag = f"posconv_layouts weight_fwd[{dn[pdt]} -> {dn[odt]}] D={D} Cg={Cg} K={K} layout {layout}"
    G = D // Cg
    v = q(dgen(D, Cg, K, seed=71, scale=math.sqrt(4.0 / (K * D))), pdt)
    g = q(v.norm(dim=(0, 1)) * (1 + 0.1 * dgen(K, seed=72)), pdt)
    norm, w = pc_weight_ref(v, g)
    w = w.view(G, Cg, Cg, K)                                   # [group, column, channel, tap]
    Ef = w.permute(0, 1, 3, 2)                                 # Wf element (n, tap, c) = w[grp * Cg + n, c, tap]
    Eb = w.flip(-1).permute(0, 2, 3, 1)                        # Wb element (n, tap, c) = w[grp * Cg + c, n, K - 1 - tap]
    off = pc_image_offsets(Cg, K, layout)
    out.append((tag + " premise: the index map is a permutation", 0.0 if torch.equal(off.sort().values, torch.arange(Cg * K * Cg, device=DEV)) else 1.0, 0.0))
    Wf, Wb, nd = ops.posconv_weight_fwd(v.to(pdt), g.to(pdt), odt, layout=layout)
    out.append((tag + " norm", errd(nd, norm), TOL32))
    for nm, W, E in (("Wf", Wf, Ef), ("Wb", Wb, Eb)):
        ref = torch.empty((G, Cg * K * Cg), dtype=torch.float64, device=DEV)
        ref[:, off] = E.reshape(G, -1)
        out.append((f"{tag} {nm}", errd(W.view(G, -1), ref), tol_for(odt)))


def pc_weight_bwd_case(out, D, Cg, K, nsplit, pdt):
    dn = {torch.float32: "fp32", torch.bfloat16: "bf16"}
    tag = f"posconv_layouts weight_bwd[{dn[pdt]}] D={D} Cg={Cg} K={K} nsplit={nsplit}"
    G = D // Cg
    v = q(dgen(D, Cg, K, seed=71, scale=math.sqrt(4.0 / (K * D))), pdt)
    g = q(v.norm(dim=(0, 1)) * (1 + 0.1 * dgen(K, seed=72)), pdt)
    slabs = dgen(nsplit, G, Cg, K * Cg, seed=73)               # [split][group][column][(tap, channel)]
    dw = slabs.double().sum(0).view(G, Cg, K, Cg).permute(0, 1, 3, 2).reshape(D, Cg, K)
    v64, g64 = v.double().requires_grad_(True), g.double().requires_grad_(True)
    _, w = pc_weight_ref(v64, g64)
    dvr, dgr = torch.autograd.grad(w, [v64, g64], dw)
    norm = v.double().norm(dim=(0, 1)).float()
    dv, dg = ops.posconv_weight_bwd(slabs, v.to(pdt), g.to(pdt), norm, nsplit=nsplit)
    out.append((tag + " dv", errd(dv, dvr), 3 * tol_for(pdt)))
    out.append((tag + " dg", errd(dg, dgr), 3 * tol_for(pdt)))


@leaves_no_footprint
def check_posconv_layouts():
    """the pc_* kernels of posconv.hip one by one -- group_major past one sweep of its capped grid (into poisoned memory, so
    that a chunk nobody writes reads as NaN), the two weight images element by element through their index maps, the slab
    sum of the weight-norm backward on known slabs -- and PosConvFn's GEMM form at odd kernel widths, where the left pad of
    the gradient copy is K - 1 - K // 2 and not K // 2 - 1."""
    out = []
    f32, bf = torch.float32, torch.bfloat16
    dn = {f32: "fp32", bf: "bf16"}
    # ---- group_major: 5 x 16 x 3327 x 8 = 2 129 280 chunks, 32 128 past GM_CAP; and the smallest call there is
    B, T, D, G, lp, Tp = 5, 3200, 1024, 16, 64, 3327
    chunks = B * G * Tp * (D // G // 8)
    out.append((f"posconv_layouts group_major premise: {chunks} chunks, between one and two sweeps of {GM_CAP}", 0.0 if GM_CAP < chunks < 2 * GM_CAP else 1.0, 0.0))
    for dtype in (bf, f32):
        pc_group_major_case(out, f"posconv_layouts group_major[{dn[dtype]}] above the cap", B, T, D, G, lp, Tp, dtype, True)
        pc_group_major_case(out, f"posconv_layouts group_major[{dn[dtype]}] B=T=1", 1, 1, 64, 4, 0, 1, dtype, False)
    x = torch.zeros((1, 4, 48), dtype=bf, device=DEV)
    out.append(("posconv_layouts group_major refuses Cg = 12 (no multiple of 8)", refused(lambda: ops.group_major(x, None, 4, 0, 4)), 0.0))
    out.append(("posconv_layouts group_major refuses Tp < left_pad + T", refused(lambda: ops.group_major(x, None, 1, 2, 5)), 0.0))
    # ---- the weight images and norm
    for (D, Cg, K, layouts) in ((96, 48, 128, (0, 1)), (256, 64, 128, (0, 1)), (64, 16, 15, (0,))):
        for layout in layouts:
            for pdt, odt in ((f32, bf), (bf, bf), (f32, f32)):
                pc_weight_fwd_case(out, D, Cg, K, layout, pdt, odt)
    v15 = dgen(64, 16, 15, seed=71)
    out.append(("posconv_layouts weight_fwd refuses layout 1 at K = 15", refused(lambda: ops.posconv_weight_fwd(v15, v15.norm(dim=(0, 1)), f32, layout=1)), 0.0))
    # ---- the slab sum and the weight-norm backward
    for (D, Cg, K) in ((96, 48, 128), (1024, 64, 128)):
        for nsplit in (1, 4):
            for pdt in (f32, bf):
                pc_weight_bwd_case(out, D, Cg, K, nsplit, pdt)
    # ---- PosConvFn, GEMM form, odd and even K
    for K in (15, 3, 16):
        for dtype in (f32, bf):
            B, T, D, G = 2, 49, 64, 4
            tag = f"posconv_layouts PosConvFn[{dn[dtype]}] B={B} T={T} D={D} K={K} G={G}"
            inp = pc_inputs(B, T, D, K, G, dtype)
            yr, sets = pc_ref(inp, G)
            pc_lines(out, tag, pc_device(inp, G, dtype), (yr, sets[0]), tol_for(dtype))
    return out


# ------------------------------------------------------------------------- fused attention at launch geometry
FA_BQ = 128                # query rows per block of the forward and the dQ kernel = key rows per block of the dK/dV kernel (FA_BK1)
FA_PART = 4                # partial rows per block (d(rel) and q|k|v bias gradient): one per wave of 32 rows
FA_RED_STRIDE = 64 * 4     # fa_dtab_reduce_kernel: 64 row slices x 4 rows in flight (u = 0..3), then r0 += 256
FA_PSTORE_MAX_T = 1024     # attn_fused.hpp: no probability store beyond; FA_DKVP_ROWS of the stored-P dK/dV kernel is the same number
ATTN_SCALE = 64 ** -0.5
ATTN_DROP = 0.25           # 16384 / 65536: exact in the kernels' 16-bit threshold, sc = 4 / 3
ATTN_REDUCE_SHAPES = [(17, 1, 100), (33, 2, 130), (11, 1, 700), (32, 1, 749)]   # B, H, T: ntot = 68, 264, 264, 768 partial rows
ATTN_REDUCE_PROBES = (0, 63, 64, 65, 127, 128, 191, 192, 255, 256)              # and ntot - 1: the u and sweep boundaries
ATTN_RAGGED_LENGTHS = (300, 257, 256, 129, 65, 2)                               # items 0..5 of the ragged batch (T = 300)
ATTN_LONG_CASES = [(1, 1, 1024, None), (1, 1, 1025, None), (2, 2, 1153, 1030), (1, 1, 1537, None)]   # B, H, T, length of item 1


def fa_partial_rows(B, T):
    nrow = FA_PART * ((T + FA_BQ - 1) // FA_BQ)
    return nrow, B * nrow


def fa_inputs(B, H, T, tabbed=True, seed=11, host=False):
    """bf16 qkv and dO, fp32 gate and table on the device; host=True: check_attention's CPU draws of the same seeds"""
    D = 64 * H
    g = (lambda *s, seed: gen(*s, seed=seed).to(DEV)) if host else dgen
    qkv = g(B, T, 3 * D, seed=seed).to(torch.bfloat16)
    gate = 1 + 0.5 * g(B, H, T, seed=seed + 1) if tabbed else None
    tab = 0.5 * g(H, 2 * T - 1, seed=seed + 2) if tabbed else None
    dO = g(B, T, D, seed=seed + 3).to(torch.bfloat16)
    return qkv, gate, tab, dO


def fa_ref64(qkv, gate, tab, kpm, H, dO, keep=None, sc=1.0):
    """_ref_attention (_ref_attention_masked with a keep mask) and its gradients in float64 where the inputs live; dbias = column
    sums of dqkv over (b, t)"""
    qr = qkv.double().requires_grad_(True)
    gr = tr = None
    if tab is not None:
        gr, tr = gate.double().requires_grad_(True), tab.double().requires_grad_(True)
    if keep is None:
        Or = _ref_attention(qr, gr, tr, kpm, H, ATTN_SCALE)
    else:
        Or = _ref_attention_masked(qr, gr, tr, kpm, H, ATTN_SCALE, keep, sc)
    g = torch.autograd.grad(Or, [qr] + ([gr, tr] if tab is not None else []), dO.double())
    return {"O": Or.detach(), "dqkv": g[0], "dgate": g[1] if tab is not None else None, "dtab": g[2] if tab is not None else None,
            "dbias": g[0].sum((0, 1))}


def fa_hostile_workspace(dev, B, H, T):
    """0xFF into every byte of the backward's workspace: each float the kernels do not write themselves reads as NaN"""
    from unispeech_amd import _lib
    need = int(_lib.lib().wavlm_attn_fused_bwd_workspace_bytes(B, H, T))
    ops.workspace(dev, need, "attn").fill_(0xFF)


def fa_device(qkv, gate, tab, kpm, H, dO, store, fwd=None, dbias=None, accumulate=False):
    """ops.attn_fused_fwd / attn_fused_bwd without dropout, the backward over a hostile workspace.  `fwd`: a forward of the same
    inputs and mode to reuse (it does not depend on dO)"""
    B, T, _ = qkv.shape
    if fwd is None:
        fwd = ops.attn_fused_fwd(qkv, gate, tab, kpm, H, ATTN_SCALE, 0.0, 0, store_p=store)
    O, lse, ps = fwd
    fa_hostile_workspace(qkv.device, B, H, T)
    dqkv, dgate, dtab = ops.attn_fused_bwd(qkv, O, dO, lse, gate, tab, kpm, H, ATTN_SCALE, 0.0, 0, dbias=dbias,
                                           dbias_accumulate=accumulate, pstore=ps)
    return {"O": O, "dqkv": dqkv, "dgate": dgate, "dtab": dtab, "dbias": dbias}, fwd


def fa_autograd(qkv, gate, tab, kpm, H, dO, fused, store, p_drop=0.0, seed=0):
    """F.AttnCoreFn forward and backward under the given switches (the caller restores them), over a hostile workspace"""
    F.USE_FUSED_ATTENTION, F.ATTN_STORE_P = fused, store
    qd = qkv.clone().requires_grad_(True)
    gd = gate.clone().requires_grad_(True) if tab is not None else None
    td = tab.clone().requires_grad_(True) if tab is not None else None
    Od = F.AttnCoreFn.apply(qd, gd, td, kpm, H, ATTN_SCALE, p_drop, seed)
    fa_hostile_workspace(qkv.device, qkv.shape[0], H, qkv.shape[1])
    Od.backward(dO)
    return {"O": Od.detach(), "dqkv": qd.grad, "dgate": gd.grad if tab is not None else None, "dtab": td.grad if tab is not None else None}


def errd_to(a, b, scale):
    """max |a - b| against a scale taken elsewhere (a slice whose own reference is zero)"""
    v = ((a.detach().double() - b.detach().double()).abs().max() / scale).item()
    return v if math.isfinite(v) else float("inf")


def fa_mode_name(fused, store):
    return ("fused, stored bits" if store == "bits" else "fused, stored P" if store else "fused, recompute") if fused else "unfused"


@leaves_no_footprint
def check_attention_reduce():
    """Every path of fa_dtab_reduce_kernel and of the q|k|v bias gradient (fa_wave_colsum partial rows of the dQ and both dK/dV
    kernels, wl_colsum_finish) at batch geometry, bf16, head_dim 64, against the float64 reference on the device.  The reduction
    adds ntot = B * 4 * ceil(T / 128) partial rows: row slice s of 64 takes rows s + 64 u + 256 k, so the shapes are chosen for
    ntot -- 68 (first use of u = 1), 264 twice (second sweep with a ragged end; once with 8 rows per item, once with 24, so that
    item and row-in-item change in the middle of a sweep) and 768 (the training step's count).  One partial row in 768 moves dtab
    by far less than the bound, so next to whole-batch parity each boundary row is probed ALONE: dO is zero outside the 32 query
    rows of partial row r, dtab and the dq part of dbias then come from that row only and are compared with a B = 1 reference of
    its item -- a reduction that drops or repeats the row is wrong by order 1.  Every backward runs over a workspace of 0xFF bytes
    (the reduction reads ranges the dQ kernel never wrote and must select, never multiply)."""
    out = []
    saved = (F.USE_FUSED_ATTENTION, F.ATTN_STORE_P)
    nan = float("nan")
    forms = {False: ((torch.float32, False), (torch.bfloat16, True)), True: ((torch.bfloat16, False), (torch.float32, True))}
    try:
        for (B, H, T) in ATTN_REDUCE_SHAPES:
            D = 64 * H
            nrow, ntot = fa_partial_rows(B, T)
            qkv, gate, tab, dO = fa_inputs(B, H, T)
            ref = fa_ref64(qkv, gate, tab, None, H, dO)
            fwds = {}
            for store in (False, True):
                for (bdt, acc) in forms[store]:
                    tag = f"attention_reduce B={B} H={H} T={T} ntot={ntot} [{fa_mode_name(True, store)}]"
                    if acc:   # (+)= onto a base of the gradient's own size
                        dbias = (dgen(3 * D, seed=31) * (0.5 * ref["dbias"].abs().max().item())).to(bdt)
                        want = dbias.double() + ref["dbias"]
                    else:     # = into NaN-filled memory
                        dbias = torch.full((3 * D,), nan, dtype=bdt, device=DEV)
                        want = ref["dbias"]
                    got, fwds[store] = fa_device(qkv, gate, tab, None, H, dO, store, fwd=fwds.get(store), dbias=dbias, accumulate=acc)
                    if store:
                        out.append((tag + " the forward returns a store", 0.0 if fwds[store][2] is not None else 1.0, 0.0))
                    out.append((tag + " O", errd(got["O"], ref["O"]), TOLBF))
                    for nm in ("dqkv", "dgate", "dtab"):
                        out.append((tag + " " + nm, errd(got[nm], ref[nm]), 2 * TOLBF))
                    out.append((tag + f" dbias[{str(bdt)[6:]}, accumulate={acc}]", errd(got["dbias"], want), 2 * TOLBF))
            for r in sorted({r for r in ATTN_REDUCE_PROBES + (ntot - 1,) if r < ntot}):
                bs, c = divmod(r, nrow)
                lo, hi = 32 * c, min(32 * c + 32, T)   # (empty past T: everything must come out exactly zero then)
                dOp = torch.zeros_like(dO)
                dOp[bs, lo:hi] = dO[bs, lo:hi]
                ref1 = fa_ref64(qkv[bs:bs + 1], gate[bs:bs + 1], tab, None, H, dOp[bs:bs + 1])
                others = torch.ones(B, dtype=torch.bool, device=DEV)
                others[bs] = False
                for store in (False, True):
                    rows = f"rows {lo}..{hi - 1}" if lo < hi else "no row below T"
                    tag = f"attention_reduce B={B} H={H} T={T} partial row {r} of {ntot} alone (item {bs}, {rows}) [{fa_mode_name(True, store)}]"
                    dbias = torch.full((3 * D,), nan, dtype=torch.float32, device=DEV)
                    got, _ = fa_device(qkv, gate, tab, None, H, dOp, store, fwd=fwds[store], dbias=dbias)
                    out.append((tag + " dtab", errd(got["dtab"], ref1["dtab"]), 2 * TOLBF))
                    out.append((tag + " dbias", errd(got["dbias"], ref1["dbias"]), 2 * TOLBF))
                    out.append((tag + " dqkv of the item", errd(got["dqkv"][bs], ref1["dqkv"][0]), 2 * TOLBF))
                    out.append((tag + " dgate of the item", errd(got["dgate"][bs], ref1["dgate"][0]), 2 * TOLBF))
                    out.append((tag + " dqkv, dgate of the other items == 0 (non-zero elements)",
                                float(((got["dqkv"][others] != 0).sum() + (got["dgate"][others] != 0).sum()).item()), 0.0))
        # TAB = false instantiation of the three backward kernels at batch geometry
        B, H, T = 33, 2, 130
        qkv, _, _, dO = fa_inputs(B, H, T, tabbed=False)
        ref = fa_ref64(qkv, None, None, None, H, dO)
        for store in (False, True):
            tag = f"attention_reduce no bias B={B} H={H} T={T} [{fa_mode_name(True, store)}]"
            dbias = torch.full((3 * 64 * H,), nan, dtype=torch.float32, device=DEV)
            got, _ = fa_device(qkv, None, None, None, H, dO, store, dbias=dbias)
            out.append((tag + " O", errd(got["O"], ref["O"]), TOLBF))
            out.append((tag + " dqkv", errd(got["dqkv"], ref["dqkv"]), 2 * TOLBF))
            out.append((tag + " dbias", errd(got["dbias"], ref["dbias"]), 2 * TOLBF))
    finally:
        F.USE_FUSED_ATTENTION, F.ATTN_STORE_P = saved
    return out


def attn_ragged_mask(T=300):
    """key padding of the ragged batch: items 0..5 right-padded to ATTN_RAGGED_LENGTHS; item 6 with keys [0, 70) and [128, 192)
    masked (its first 64-key tile is dead -- the online softmax meets a tile with no live key before any live one -- and a whole
    dead tile lies between live ones); item 7 with one live key"""
    kpm = torch.zeros(len(ATTN_RAGGED_LENGTHS) + 2, T, dtype=torch.uint8)
    for b, n in enumerate(ATTN_RAGGED_LENGTHS):
        kpm[b, n:] = 1
    kpm[6, :70] = 1
    kpm[6, 128:192] = 1
    kpm[7, 1:] = 1
    return kpm


def fa_item_lines(out, tag, got, ref, D, single=(7,)):
    """O, dqkv, dgate of every item against that item's own reference maximum (err()'s whole-tensor scale is set by the shortest
    item: its dqkv maximum is some 20 times the full-length item's).  Items with ONE live key (`single`): every probability is
    exactly 1, so the reference's dS -- and with it dq, dk and dgate -- is exactly zero and a ratio to the slice means nothing:
    O and dv against the slice, dq | dk and dgate against the whole tensor's scale"""
    B = ref["O"].shape[0]
    qmax, gmax = ref["dqkv"].abs().max(), ref["dgate"].abs().max()
    for b in range(B):
        out.append((tag + f" item {b} O", errd(got["O"][b], ref["O"][b]), TOLBF))
        if b in single:
            out.append((tag + f" item {b} dv", errd(got["dqkv"][b, :, 2 * D:], ref["dqkv"][b, :, 2 * D:]), 2 * TOLBF))
            out.append((tag + f" item {b} dq | dk (tensor scale)", errd_to(got["dqkv"][b, :, :2 * D], ref["dqkv"][b, :, :2 * D], qmax), 2 * TOLBF))
            out.append((tag + f" item {b} dgate (tensor scale)", errd_to(got["dgate"][b], ref["dgate"][b], gmax), 2 * TOLBF))
        else:
            out.append((tag + f" item {b} dqkv", errd(got["dqkv"][b], ref["dqkv"][b]), 2 * TOLBF))
            out.append((tag + f" item {b} dgate", errd(got["dgate"][b], ref["dgate"][b]), 2 * TOLBF))
    out.append((tag + " dtab", errd(got["dtab"], ref["dtab"]), 2 * TOLBF))
    masked = ref["kpm"].bool()
    out.append((tag + " dk, dv of masked keys == 0 (non-zero elements)", float((got["dqkv"][..., D:][masked] != 0).sum().item()), 0.0))


def fa_mask_lines(out, tag, masks, plain, live):
    """forward, dQ and dK/dV keep masks of one mode (_attn_kernel_masks) against each other and against the plain forward's.  The
    dQ read-out takes the sign of dS = P sc (keep - kappa) with kappa the row's kept mass: a row that keeps EVERY live key has
    kappa = 1 and dS = 0 up to rounding, and says nothing (one row in 10^8 at 65 live keys, 9 in 16 at two, all at one); such rows
    are left out of the dQ comparison -- a dQ kernel that drops other elements there misses the numerics that follow"""
    kf, kq, kkv = masks
    readable = (kf.sum(-1) < live.sum(-1)[:, None, None])[..., None]
    if plain is not None:
        out.append((tag + " storing fwd == plain fwd (mismatching elements)", float((kf != plain).sum().item()), 0.0))
    out.append((tag + " mask fwd == dQ (mismatching elements)", float(((kf != kq) & readable).sum().item()), 0.0))
    out.append((tag + " mask fwd == dK/dV (mismatching elements)", float((kf != kkv).sum().item()), 0.0))


@leaves_no_footprint
def check_attention_ragged():
    """Key-padding masks the kernels accept and no other check sends (attn_ragged_mask), B = 8, H = 2, T = 300, bf16, head_dim 64,
    against the float64 reference on the device, PER ITEM (fa_item_lines): without dropout in the recompute, stored-probability
    and unfused forms, with dropout 0.25 in the three fused modes under the kernels' own mask, which must be the same in the
    forward, dQ and dK/dV kernels.  dk and dv of masked keys are exactly zero, and every item computed alone (B = 1) gives the bits
    it gives inside the batch.  The float64 reference of this batch (check_attention's draws, seeds 11..14) has slice maxima of
    0.6 .. 2.7 (O) and 1.0 .. 23.9 (dqkv); rounding P to bf16 alone costs 1e-3 .. 2.3e-3 of a slice, a tenth of TOLBF, so the
    project's bounds hold per item as they are."""
    out = []
    saved = (F.USE_FUSED_ATTENTION, F.ATTN_STORE_P)
    try:
        H, T = 2, 300
        D = 64 * H
        kpm = attn_ragged_mask(T).to(DEV)
        B = kpm.shape[0]
        qkv, gate, tab, dO = fa_inputs(B, H, T, host=True)
        ref = fa_ref64(qkv, gate, tab, kpm, H, dO)
        ref["kpm"] = kpm
        batch = {}
        for fused, store in ((True, False), (True, True), (False, False)):
            got = batch[store if fused else "unfused"] = fa_autograd(qkv, gate, tab, kpm, H, dO, fused, store)
            fa_item_lines(out, f"attention_ragged [{fa_mode_name(fused, store)}]", got, ref, D)
        for store in (False, True):
            for b in range(B):
                one = fa_autograd(qkv[b:b + 1].contiguous(), gate[b:b + 1].contiguous(), tab, kpm[b:b + 1].contiguous(), H,
                                  dO[b:b + 1].contiguous(), True, store)
                diff = sum(same_bits(one[nm][0], batch[store][nm][b]) for nm in ("O", "dqkv", "dgate"))
                out.append((f"attention_ragged [{fa_mode_name(True, store)}] item {b} alone == in the batch (O, dqkv, dgate that differ)", diff, 0.0))
        seed, sc = 0x9E3779B97F4A7C15, 1.0 / (1.0 - ATTN_DROP)
        live = ~kpm.bool().cpu()
        plain = None
        for store in (False, True, "bits"):
            tag = f"attention_ragged dropout [{fa_mode_name(True, store)}]"
            masks = _attn_kernel_masks(B, H, T, ATTN_DROP, seed, gate, tab, kpm, store_p=store)
            fa_mask_lines(out, tag, masks, plain, live)
            if plain is None:
                plain = masks[0]
                out.append((tag + " keep fraction of the live keys", abs(plain.float().sum().item() / (H * T * live.sum().item()) - (1 - ATTN_DROP)), 0.01))
                refd = fa_ref64(qkv, gate, tab, kpm, H, dO, keep=plain.to(DEV), sc=sc)
                refd["kpm"] = kpm
            fa_item_lines(out, tag, fa_autograd(qkv, gate, tab, kpm, H, dO, True, store, ATTN_DROP, seed), refd, D)
    finally:
        F.USE_FUSED_ATTENTION, F.ATTN_STORE_P = saved
    return out


@leaves_no_footprint
def check_attention_long():
    """The fused kernels at and past FA_PSTORE_MAX_T = 1024 (bf16, head_dim 64, gate and table, float64 reference on the device):
    T = 1024 -- the last length with a probability store, where the stored-P dK/dV kernel's per-row LDS arrays (FA_DKVP_ROWS) are
    full --, 1025 (no store: ops.attn_fused_fwd returns None and AttnCoreFn under ATTN_STORE_P=True recomputes), 1153 with a
    padded item, 1537 (30 s of audio is 1499 frames).  At T = 1025 the dropout modes that have no cap -- recompute and stored
    bits -- must apply one mask in all three kernels, agree bit for bit, and match the reference under that mask."""
    out = []
    saved = (F.USE_FUSED_ATTENTION, F.ATTN_STORE_P)
    try:
        for (B, H, T, n1) in ATTN_LONG_CASES:
            kpm = None
            if n1 is not None:
                kpm = torch.zeros(B, T, dtype=torch.uint8, device=DEV)
                kpm[1, n1:] = 1
            qkv, gate, tab, dO = fa_inputs(B, H, T)
            ref = fa_ref64(qkv, gate, tab, kpm, H, dO)
            stored = ops.attn_fused_fwd(qkv, gate, tab, kpm, H, ATTN_SCALE, 0.0, 0, store_p=True)[2] is not None
            out.append((f"attention_long B={B} H={H} T={T} probability store " + ("returned" if T <= FA_PSTORE_MAX_T else "refused (None)"),
                        0.0 if stored == (T <= FA_PSTORE_MAX_T) else 1.0, 0.0))
            for store in (False, True):
                tag = f"attention_long B={B} H={H} T={T} [{fa_mode_name(True, store)}{'' if stored or not store else ' -> recompute'}]"
                got = fa_autograd(qkv, gate, tab, kpm, H, dO, True, store)
                out.append((tag + " O", errd(got["O"], ref["O"]), TOLBF))
                for nm in ("dqkv", "dgate", "dtab"):
                    out.append((tag + " " + nm, errd(got[nm], ref[nm]), 2 * TOLBF))
        B, H, T = 1, 1, 1025
        seed, sc = 77, 1.0 / (1.0 - ATTN_DROP)
        qkv, gate, tab, dO = fa_inputs(B, H, T)
        live = torch.ones(B, T, dtype=torch.bool)
        plain, res = None, {}
        for store in (False, "bits"):
            tag = f"attention_long dropout B={B} H={H} T={T} [{fa_mode_name(True, store)}]"
            masks = _attn_kernel_masks(B, H, T, ATTN_DROP, seed, gate, tab, None, store_p=store)
            fa_mask_lines(out, tag, masks, plain, live)
            if plain is None:
                plain = masks[0]
                out.append((tag + " keep fraction", abs(plain.float().mean().item() - (1 - ATTN_DROP)), 0.01))
                refd = fa_ref64(qkv, gate, tab, None, H, dO, keep=plain.to(DEV), sc=sc)
            got = res[store] = fa_autograd(qkv, gate, tab, None, H, dO, True, store, ATTN_DROP, seed)
            out.append((tag + " O vs fp64 with the kernel's mask", errd(got["O"], refd["O"]), TOLBF))
            for nm in ("dqkv", "dgate", "dtab"):
                out.append((tag + " " + nm + " vs fp64 with the kernel's mask", errd(got[nm], refd[nm]), 2 * TOLBF))
        for nm in ("O", "dqkv", "dgate"):
            out.append((f"attention_long dropout B={B} H={H} T={T} stored bits == recompute: {nm} (bits differ)",
                        same_bits(res[False][nm], res["bits"][nm]), 0.0))
    finally:
        F.USE_FUSED_ATTENTION, F.ATTN_STORE_P = saved
    return out


GROUPS = {
    "gemm": check_gemm, "gemm_pp": check_gemm_pp, "gemm_pp3": check_gemm_pp3, "gemm_w4": check_gemm_w4, "gemm_grouped": check_gemm_grouped, "gemm_race": check_gemm_race, "layernorm": check_layernorm, "rowops": check_rowops, "conv0": check_conv0, "conv0_ln": check_conv0_ln, "conv_ln_block": check_conv_ln_block,
    "conv_ln_block_wide": check_conv_ln_block_wide, "convstack": check_convstack, "convstack_wide": check_convstack_wide, "attention": check_attention, "posconv": check_posconv, "gemm_colsum": check_gemm_colsum,
    "linear_ffn": check_linear_ffn, "activations": check_activations, "loss": check_loss, "adam": check_adam, "dropout_exact": check_dropout_exact,
    "gumbel_vq": check_gumbel_vq, "sampled_negatives": check_sampled_negatives,
    "layernorm_rows": check_layernorm_rows, "layernorm_dropout_ref": check_layernorm_dropout_ref, "colsum_rows": check_colsum_rows,
    "flat_strided": check_flat_strided, "masked_pred_head": check_masked_pred_head, "loss_rows_capped": check_loss_rows_capped,
    "posconv_batch": check_posconv_batch, "posconv_frames": check_posconv_frames, "posconv_layouts": check_posconv_layouts,
    "attention_reduce": check_attention_reduce, "attention_ragged": check_attention_ragged, "attention_long": check_attention_long,
}
# gemm_race's split-K case grows ops' "main" workspace to 63 MiB (7 fp32 slabs of 3072 x 768) while the tensors of the cases before
# lie freed in the cache: when the groups run in a process of their own (pytest tests/test_kernels_gpu.py), the workspace is cut
# out of the middle of a cached 192 MiB block and pins 54 + 75 MiB of stale memory, and layernorm_rows' poisoned 16 MiB request
# is handed the 54 MiB fragment instead of the NaN-filled block (measured on the MI355X, with and without the attention groups)
GROUPS["gemm_race"] = leaves_no_footprint(check_gemm_race)

if __name__ == "__main__":
    import json
    import time
    total = 0
    for name in sys.argv[1:]:   # one group, or several in one process
        t0 = time.time()
        res = GROUPS[name]()
        torch.cuda.synchronize()
        bad = 0
        for (nm, e, t) in res:
            ok = e <= t
            bad += (not ok)
            print(("ok   " if ok else "FAIL ") + f"{nm}: err={e:.3e} tol={t:.1e}")
        print(json.dumps({"group": name, "n": len(res), "failed": bad, "seconds": round(time.time() - t0, 1)}))
        total += bad
    sys.exit(1 if total else 0)
