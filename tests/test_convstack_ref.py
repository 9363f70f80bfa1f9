"""The reference side of the `convstack_wide` group of tests/gpu_checks.py, on the CPU.

The group compares ConvStackFn in bf16 with an exact float64 conv1d -> gelu stack at check_convstack's tolerances (2e-2 of
the tensor scale for y, 4e-2 for gradients).  The only approximations a correct bf16 device path has and that reference lacks
are the bf16 rounding of every layer's pre-activation u and of the activations handed from layer to layer.  This test inserts
exactly those two roundings into the float64 reference and measures, in the group's own metrics (whole tensor, and the first /
last two frames of every utterance on their own scale), how far that moves it: the figure must stay below HALF the tolerance
for every case of the group's table, so the other half is what the kernels' own arithmetic (fp32 accumulation order, the GELU
chord table, bf16 stores of the gradients) may use.  The figures are printed (pytest -s).

Also pinned here, without a GPU: the shape guard of the wide groups counts no launch below the tile kernels' minimum shapes
for any case, and does count them for the narrow stack of the `convstack` group."""
import pytest
import torch

import gpu_checks as K


def _name(case):
    B, T0, specs, _, bias, need_dx = case
    return f"B{B}-T{T0}-" + "".join(f"k{k}s{s}" for k, s in specs) + ("-bias" if bias else "") + ("" if need_dx else "-nodx")


@pytest.mark.parametrize("case", K.CONVSTACK_WIDE_CASES, ids=_name)
def test_rounding_moves_the_reference_less_than_half_the_tolerance(case):
    _, _, specs, _, _, need_dx = case
    inputs = K.convstack_wide_inputs(case, torch.bfloat16)
    exact = K.convstack_wide_ref(inputs, specs, need_dx)
    rounded = K.convstack_wide_ref(inputs, specs, need_dx, round_dtype=torch.bfloat16)
    figures = []
    K.conv_compare(_name(case), rounded, exact, 0, K.TOLBF, figures)
    assert len(figures) == len(exact) + (2 if need_dx else 1)   # every tensor, plus the boundary rows of y and dx
    for n, e, t in figures:
        print(f"{n}: reference-side figure {e:.2e}, tolerance {t:.0e}")
    bad = [(n, e, t) for n, e, t in figures if not e < 0.5 * t]
    assert not bad, bad


@pytest.mark.parametrize("case", K.CONVSTACK_WIDE_CASES, ids=_name)
def test_every_launch_of_a_wide_case_has_a_tile_kernel_shape(case):
    _, T0, specs, _, _, _ = case
    assert K.conv_shape_guard(T0, specs, K.CONV_WIDE_C) == 0
    shapes = K.conv_launch_shapes(T0, specs, K.CONV_WIDE_C)
    assert len(shapes) == sum(2 + s for _, s in specs)
    T = T0
    for (k, s) in specs:
        T = (T - k) // s + 1
    assert 256 <= T <= 275   # one full 256-row tile, and (but for the exact-tile cases) a ragged one


def test_conv_ln_wide_cases_have_tile_kernel_shapes():
    for (_, T_in, k, s) in K.CONV_LN_WIDE_CASES:
        assert K.conv_shape_guard(T_in, ((k, s),), K.CONV_WIDE_C) == 0


def test_shape_guard_counts_what_the_generic_kernel_would_take():
    # the `convstack` group: N = 32, every launch is the generic kernel's
    specs = ((3, 2), (3, 2), (2, 2), (2, 2))
    assert K.conv_shape_guard(403, specs, 32) == len(K.conv_launch_shapes(403, specs, 32))
    # C = 512 but a short utterance: M and the weight gradient's K fall below the tiles (the `conv_ln_block` group)
    assert K.conv_shape_guard(101, ((3, 2),), 512) == 4
    # one frame less than a full tile out of the last layer
    assert K.conv_shape_guard(511, ((3, 2),), 512) > 0


def test_unused_trailing_frames():
    assert K.unused_trailing_frames(1047, 2, 2) == 1
    assert K.unused_trailing_frames(1100, 3, 2) == 1
    assert [K.unused_trailing_frames(T, k, s) for T, k, s in ((1101, 3, 2), (1048, 2, 2), (513, 3, 2), (512, 2, 2), (2203, 3, 2))] == [0] * 5
