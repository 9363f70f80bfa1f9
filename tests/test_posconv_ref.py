"""The reference side of the `posconv_batch`, `posconv_frames` and `posconv_layouts` groups of tests/gpu_checks.py, on the CPU.

Pinned here, without a GPU: the tap-loop reference of the groups (posconv_ref64) is the grouped conv1d with the reference's
SamePad for odd and even kernel widths, gradients included; the restated launch geometry gives what the case tables say it
reaches; the restated index maps of the weight images are permutations; and the index arithmetic of PosConvFn.backward's data
gradient -- the gradient copy padded on the left, correlated with the tap-flipped image -- is the true gradient with a pad
of K - 1 - K // 2 rows, and for odd K is not with K // 2 - 1."""
import pytest
import torch
import torch.nn.functional as TF

import gpu_checks as K


@pytest.mark.parametrize("shape", [(2, 9, 8, 3, 2), (2, 20, 16, 15, 4), (1, 7, 8, 4, 1), (2, 30, 16, 16, 2), (1, 1, 8, 8, 2), (1, 3, 8, 15, 1)])
def test_tap_loop_reference_is_the_same_padded_grouped_convolution(shape):
    B, T, D, Kw, G = shape
    g0 = torch.Generator().manual_seed(7)
    x, v, g, b = [torch.randn(*s, generator=g0, dtype=torch.float64).requires_grad_(True)
                  for s in ((B, T, D), (D, D // G, Kw), (1, 1, Kw), (D,))]
    y = K.posconv_ref64(x, v, g, b, G)
    w = g * v / v.norm(dim=(0, 1), keepdim=True)
    y2 = x + TF.gelu(TF.conv1d(x.transpose(1, 2), w, b, padding=Kw // 2, groups=G)[:, :, :T]).transpose(1, 2)
    dy = torch.randn(B, T, D, generator=g0, dtype=torch.float64)
    assert torch.allclose(y, y2, rtol=0, atol=1e-12)
    for a, c in zip(torch.autograd.grad(y, [x, v, g, b], dy), torch.autograd.grad(y2, [x, v, g, b], dy)):
        assert torch.allclose(a, c, rtol=0, atol=1e-11)


def _dx_by_padded_correlation(w, du, P):
    """PosConvFn.backward's data gradient for one group: du in a buffer of T + K - 1 rows behind P zero rows, correlated with
    the image Wb[tap] = w[:, :, K - 1 - tap]"""
    Kw, T = w.shape[2], du.shape[0]
    dug = torch.zeros(T + Kw - 1, w.shape[0], dtype=du.dtype)
    dug[P:P + T] = du
    dx = torch.zeros(T, w.shape[1], dtype=du.dtype)
    for tap in range(Kw):
        dx += dug[tap:tap + T] @ w[:, :, Kw - 1 - tap]
    return dx


@pytest.mark.parametrize("Kw", [3, 4, 15, 16])
def test_left_pad_of_the_gradient_copy(Kw):
    T, C = 23, 5
    g0 = torch.Generator().manual_seed(Kw)
    x = torch.randn(T, C, generator=g0, dtype=torch.float64, requires_grad=True)
    w = torch.randn(C, C, Kw, generator=g0, dtype=torch.float64)
    du = torch.randn(T, C, generator=g0, dtype=torch.float64)
    u = TF.conv1d(x.t()[None], w, padding=Kw // 2)[0, :, :T].t()
    (true,) = torch.autograd.grad(u, x, du)
    assert torch.allclose(_dx_by_padded_correlation(w, du, Kw - 1 - Kw // 2), true, rtol=0, atol=1e-12)
    if Kw % 2:
        assert (_dx_by_padded_correlation(w, du, Kw // 2 - 1) - true).abs().max() > 0.1 * true.abs().max()
    else:
        assert Kw - 1 - Kw // 2 == Kw // 2 - 1


def test_frame_cases_reach_the_tiles_their_table_names():
    for Cg, cases in K.PC_FRAME_CASES.items():
        assert {bm for _, bm, _ in cases} == set(K.PCD_TILES[Cg])               # every tile height
        assert {1, 2, 3, 5} <= {n for c in K.PC_FRAME_CASES.values() for _, _, n in c}
        for (T, bm, nseg) in cases:
            assert K.posconv_direct_tile(Cg, T) == (bm, nseg), (Cg, T)
            assert (nseg - 1) * bm < T <= nseg * bm
        assert K.posconv_direct_tile(Cg, K.PC_FRAME_B2[Cg])[1] > 1
        D, G = K.PC_FRAME_DG[Cg]
        assert D // G == Cg and (G * K.PDW_BS[Cg]) % 8 == 0 and ((G // 2) * K.PDW_BS[Cg]) % 8 != 0   # the smallest G with the direct dw kernel
    assert K.posconv_direct_tile(48, 513) == (768, 1) and -(-513 // 384) * 384 == 768   # the tie


def test_batch_cases_walk_several_batches_per_workgroup():
    for (Cg, D, B, T, bchunk, per, nch, tail) in K.PC_BATCH_CASES:
        assert D // 16 == Cg and K.posconv_dw_geometry(Cg, B, T) == (bchunk, per, nch, tail)
        assert sum(per) == B and bchunk >= 2 and 0 < tail <= K.PDW_TCH[Cg]
    pers = [c[5] for c in K.PC_BATCH_CASES]
    assert any(0 in p for p in pers) and any(0 < min(p) < max(p) for p in pers) and any(min(p) == max(p) for p in pers)
    assert {c[7] for c in K.PC_BATCH_CASES if c[6] > 1} >= {1, 44}


@pytest.mark.parametrize("Cg,Kw,layout", [(48, 128, 0), (48, 128, 1), (64, 128, 1), (16, 15, 0)])
def test_weight_image_index_maps_are_permutations(Cg, Kw, layout, monkeypatch):
    monkeypatch.setattr(K, "DEV", "cpu")
    off = K.pc_image_offsets(Cg, Kw, layout)
    assert torch.equal(off.sort().values, torch.arange(Cg * Kw * Cg))
    # element (column n, tap, channel c) sits where posconv.hip's comment puts it
    n, tap, c = 5, Kw - 2, Cg - 3
    at = off.view(Cg, Kw, Cg)[n, tap, c].item()
    if layout == 0:
        assert at == (n * Kw + tap) * Cg + c
    else:
        strides = torch.tensor([Cg // 8, 4, Kw // 16, 4, Cg, 8])
        idx = [c // 8, tap % 16 // 4, tap // 16, tap % 4, n, c % 8]
        flat = 0
        for i, s in zip(idx, strides.tolist()):
            flat = flat * s + i
        assert at == flat
