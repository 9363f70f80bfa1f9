"""unispeech_amd.wavein.pack_filters, the one packer behind mfcc.tables and fbank.tables (CPU, no library call): the packed
form expands back to the dense bank exactly, its triples stay inside the P / 2 bins and the weights the kernels stage, and the
two modules' public tables() still return, array for array, what tests/golden/front_end_tables.npz recorded from their own
packers before these were merged."""
import os

import numpy as np
import pytest

from unispeech_amd import fbank, mfcc, wavein

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "front_end_tables.npz")


def _kaldi(sr):
    return mfcc.mel_filters(sr), mfcc.geometry(sr)[2], mfcc.tables(sr), "kaldi_%d" % sr


def _htk(sr, P, M):
    return fbank.mel_bank(sr, P, M).T, P, fbank.tables(sr, P, int(sr * 0.025), M), "htk_%d_%d_%d" % (sr, P, M)


BANKS = [(_kaldi, (16000,)), (_kaldi, (8000,)), (_htk, (16000, 512, 40)), (_htk, (16000, 512, 128)), (_htk, (8000, 256, 40))]


@pytest.mark.parametrize("make,args", BANKS, ids=lambda v: v.__name__.strip("_") if callable(v) else "-".join(map(str, v)))
def test_pack_filters(make, args):
    bank, P, tables, name = make(*args)                    # bank: dense float64 [filters, P / 2 + 1]
    idx, w = wavein.pack_filters(bank)
    assert idx.dtype == np.int32 and idx.shape == (len(bank), 3) and w.dtype == np.float64 and w.ndim == 1
    dense = np.zeros_like(bank)
    for f, (first, count, off) in enumerate(idx):
        assert first >= 0 and count >= 0 and off >= 0
        assert first + count <= P // 2 and off + count <= len(w), (f, first, count, off)
        dense[f, first:first + count] = w[off:off + count]
    assert np.array_equal(dense, bank)
    assert int(idx[:, 1].sum()) == len(w) <= P             # no gaps between the filters; the kernels stage at most P weights
    with np.load(GOLDEN) as g:
        want = {k.split("/", 1)[1]: g[k] for k in g.files if k.startswith(name + "/")}
    assert sorted(want) == sorted(tables)
    for k, v in want.items():
        got = np.asarray(tables[k])
        assert got.dtype == v.dtype and got.shape == v.shape and np.array_equal(got, v), k
    assert np.array_equal(idx, want["mel_idx"]) and np.array_equal(w, want["mel_w"])


def test_pack_filters_empty():
    """a filter without a weight has count 0 and takes nothing; a bank without any weight packs to an empty mel_w"""
    bank = np.zeros((3, 9))
    bank[1, 2:5] = (0.5, 0.0, 0.25)                        # a zero between two weights stays inside the filter
    idx, w = wavein.pack_filters(bank)
    assert idx.tolist() == [[0, 0, 0], [2, 3, 0], [0, 0, 3]] and w.tolist() == [0.5, 0.0, 0.25]
    idx, w = wavein.pack_filters(np.zeros((2, 9)))
    assert idx.tolist() == [[0, 0, 0], [0, 0, 0]] and w.shape == (0,) and w.dtype == np.float64
