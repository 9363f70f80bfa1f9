"""The weight-gradient launch policy has ONE implementation (csrc/split_policy.hpp), reached through wavlm_split_single /
wavlm_split_grouped / wavlm_slabs_grouped by the fused block, the Python autograd path and these tests alike.  Here the
exported functions are compared with a plain restatement of the rules over a sweep of shapes, grouped tile counts and CU
reservations.  The restatement was fixed when written: over this same sweep it equals what ops.pick_split, ops.grouped_split
and ops.grouped_slabs computed in Python before the policy moved into the library (0 mismatches).  No GPU."""
import itertools

import pytest

from unispeech_amd import ops

RESERVED = (0, 2, 6, 8, 16, 64)              # wavlm_set_reserved_cus: grid = 256 - reserved
FORCED = (0, 1, 2, 7, 14)                    # WAVLM_WGRAD_SPLIT (0 = unset)
DIMS = (64, 128, 200, 255, 256, 257, 512, 768, 1024, 1536, 3072, 4096)
KTILES = (1, 7, 8, 15, 16, 63, 64, 375, 500, 512, 12000)
TILES = (1, 3, 9, 12, 27, 36, 64, 108, 127, 128, 129, 192, 250, 255, 256, 300)


def single_points():
    return itertools.product(DIMS, DIMS, KTILES)


def grouped_points():
    return itertools.product(TILES, KTILES)


def want_single(M, N, ktiles, grid):
    if M >= 256 and N >= 256:       # the 256 x 256 kernels: one round of the grid, at least 8 K-steps per slab
        tiles = -(-M // 256) * -(-N // 256)
        return max(1, min(grid // tiles, ktiles // 8, 64))
    tiles = -(-M // 128) * -(-N // 128)   # the 128-wide kernel: about 768 blocks
    return min(max(1, min(ktiles, -(-768 // tiles))), 64)


def want_grouped(tiles, ktiles, grid, forced):
    if forced > 0:
        return max(2, forced)
    s = min(grid // tiles, ktiles // 8, 64)
    return s if s >= 2 else 0


def want_slabs(tiles, ktiles, grid, forced, balanced):
    split = max(2, want_grouped(tiles, ktiles, grid, forced))
    if balanced and forced <= 0 and tiles < grid and tiles * ktiles >= 8 * grid:
        return max(split, grid // tiles + 1)
    return split


def test_exported_policy_equals_its_restatement():
    n = 0
    for r in RESERVED:
        G = 256 - r
        for M, N, kt in single_points():
            assert ops.pick_split(M, N, kt, G) == want_single(M, N, kt, G), (M, N, kt, G)
            n += 1
        for forced, bal in itertools.product(FORCED, (False, True)):
            for t, kt in grouped_points():
                assert ops.grouped_split(t, kt, G, forced) == want_grouped(t, kt, G, forced), (t, kt, G, forced)
                assert ops.grouped_slabs(t, kt, G, forced, bal) == want_slabs(t, kt, G, forced, bal), (t, kt, G, forced, bal)
                n += 2
    assert n == len(RESERVED) * (len(DIMS) ** 2 * len(KTILES) + 2 * len(FORCED) * 2 * len(TILES) * len(KTILES)) == 30624


@pytest.fixture
def reserved():
    before = ops.get_reserved_cus()
    yield
    ops.set_reserved_cus(before)


def test_defaults_are_the_live_settings(reserved, monkeypatch):
    """grid = 0 is the live reservation; the environment is the library's to read, once: changing it later changes nothing"""
    for r in RESERVED:
        ops.set_reserved_cus(r)
        assert ops.grid_blocks() == 256 - r
        for M, N, kt in ((512, 1536, 12000), (768, 3072, 375), (1024, 1024, 500)):
            assert ops.pick_split(M, N, kt) == ops.pick_split(M, N, kt, 256 - r)
        for t, kt in ((108, 375), (64, 500), (192, 500)):
            assert ops.grouped_split(t, kt) == ops.grouped_split(t, kt, 256 - r)
            assert ops.grouped_slabs(t, kt) == ops.grouped_slabs(t, kt, 256 - r)
    ops.set_reserved_cus(0)
    before = ops.grouped_split(108, 375), ops.grouped_slabs(108, 375), ops.wgrad_grouping()
    monkeypatch.setenv("WAVLM_WGRAD_SPLIT", "14")
    monkeypatch.setenv("WAVLM_WGRAD_STREAMK", "1")
    monkeypatch.setenv("WAVLM_WGRAD_GROUPING", "0")
    assert (ops.grouped_split(108, 375), ops.grouped_slabs(108, 375), ops.wgrad_grouping()) == before
