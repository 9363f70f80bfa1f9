"""The reference side of the `attention_reduce`, `attention_ragged` and `attention_long` groups of tests/gpu_checks.py, on the CPU.

Pinned here, without a GPU: the attention reference the groups run on the device is scaled-dot-product attention with an
additive bias gate[b, h, i] * tab[h, j - i + T - 1], written out element by element; the restated launch geometry gives the partial
row counts the shapes were chosen for, and the probed rows sit on the boundaries of fa_dtab_reduce_kernel's loops; the ragged mask
has the dead tiles its group is about; and the premises of the per-item metric hold in the float64 reference of that batch: the
shortest items set the whole-tensor scale, and an item with one live key has a gradient of exactly zero for q, k and the gate."""
import torch
import torch.nn.functional as TF

import gpu_checks as K


def test_reference_is_biased_scaled_dot_product_attention():
    B, H, T, hd = 2, 2, 7, 4
    g0 = torch.Generator().manual_seed(3)
    qkv = torch.randn(B, T, 3 * H * hd, generator=g0, dtype=torch.float64)
    gate = torch.randn(B, H, T, generator=g0, dtype=torch.float64)
    tab = torch.randn(H, 2 * T - 1, generator=g0, dtype=torch.float64)
    kpm = torch.zeros(B, T, dtype=torch.uint8)
    kpm[1, 5:] = 1
    keep = torch.rand(B, H, T, T, generator=g0) > 0.25
    bias = torch.zeros(B, H, T, T, dtype=torch.float64)
    for i in range(T):
        for j in range(T):
            bias[:, :, i, j] = gate[:, :, i] * tab[:, j - i + T - 1]
    bias = bias.masked_fill(kpm.bool()[:, None, None, :], float("-inf"))
    qh, kh, vh = [t.view(B, T, H, hd).transpose(1, 2) for t in qkv.chunk(3, dim=-1)]
    want = TF.scaled_dot_product_attention(qh, kh, vh, attn_mask=bias, scale=0.3).transpose(1, 2).reshape(B, T, H * hd)
    assert torch.allclose(K._ref_attention(qkv, gate, tab, kpm, H, 0.3), want, rtol=0, atol=1e-12)
    p = torch.softmax(qh @ kh.transpose(-1, -2) * 0.3 + bias, -1) * keep * 1.5
    want = (p @ vh).transpose(1, 2).reshape(B, T, H * hd)
    assert torch.allclose(K._ref_attention_masked(qkv, gate, tab, kpm, H, 0.3, keep, 1.5), want, rtol=0, atol=1e-12)


def test_reduce_shapes_reach_every_loop_of_the_partial_row_reduction():
    assert [K.fa_partial_rows(B, T) for (B, H, T) in K.ATTN_REDUCE_SHAPES] == [(4, 68), (8, 264), (24, 264), (24, 768)]
    counts = [K.fa_partial_rows(B, T)[1] for (B, H, T) in K.ATTN_REDUCE_SHAPES]
    assert 64 < counts[0] <= 128                                    # u = 1 runs, u = 2 does not
    assert all(K.FA_RED_STRIDE < n for n in counts[1:])             # a second sweep
    assert counts[1] % K.FA_RED_STRIDE and counts[3] == 3 * K.FA_RED_STRIDE   # a ragged last sweep; three full ones
    assert K.FA_RED_STRIDE % K.fa_partial_rows(11, 700)[0]          # 24 rows per item: an item straddles rows 63 | 64 and 255 | 256
    probes = set(K.ATTN_REDUCE_PROBES)
    for edge in (64, 128, 192, 256):                                # both sides of each u and sweep boundary
        assert {edge - 1, edge} <= probes
    assert K.fa_partial_rows(32, 749)[1] == 32 * 4 * 6              # the benchmark's B = 32, T = 749


def test_ragged_mask_has_dead_tiles_and_short_items():
    live = ~K.attn_ragged_mask(300).bool()
    assert live.sum(-1).tolist() == [300, 257, 256, 129, 65, 2, 166, 1]
    tiles = [[bool(live[b, t:t + 64].any()) for t in range(0, 300, 64)] for b in range(8)]
    assert tiles[6] == [False, True, False, True, True]             # dead before any live key, dead between live ones
    assert live[6, 70] and not live[6, 69]                          # the first live tile starts masked
    assert tiles[5] == [True, False, False, False, False] and bool(live[7, 0])
    assert all(n <= K.FA_PSTORE_MAX_T for (_, _, n, _) in K.ATTN_LONG_CASES[:1]) and K.ATTN_LONG_CASES[1][2] == K.FA_PSTORE_MAX_T + 1


def test_per_item_metric_premises_in_the_float64_reference():
    saved = K.DEV
    K.DEV = "cpu"
    try:
        qkv, gate, tab, dO = K.fa_inputs(8, 2, 300, host=True)
    finally:
        K.DEV = saved
    ref = K.fa_ref64(qkv, gate, tab, K.attn_ragged_mask(300), 2, dO)
    dmax = [ref["dqkv"][b].abs().max().item() for b in range(8)]
    assert dmax[0] < 1.1 and dmax[5] > 20 * dmax[0]                 # the two-key item hides a 20-fold error of the full-length one
    assert ref["dqkv"][7, :, :256].abs().max().item() == 0.0 and ref["dgate"][7].abs().max().item() == 0.0
    assert ref["dqkv"][7, :, 256:].abs().max().item() > 1.0         # dv of the one-key item is not zero
    masked = K.attn_ragged_mask(300).bool()
    assert ref["dqkv"][..., 128:][masked].abs().max().item() == 0.0   # dk, dv of masked keys
