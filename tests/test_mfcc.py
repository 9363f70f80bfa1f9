"""unispeech_amd/mfcc.py on the CPU: the float64 restatement of kaldi.mfcc + deltas against pieces computed another way, the
refused options, the host-side geometry queries and the command line.  torchaudio is not installed and is never run: what is
checked is the restatement, piece by piece."""
import math

import numpy as np
import pytest
import scipy.fft

import mfcc_cases as MC


@pytest.mark.parametrize("sr", [16000, 8000])
def test_frame_counts(sr):
    from unispeech_amd import _lib
    from unispeech_amd.mfcc import geometry, mfcc_reference, num_frames
    W, S, P = geometry(sr)
    assert (W, S, P) == ((400, 160, 512) if sr == 16000 else (200, 80, 256))
    for L, want in ((W - 1, 0), (W, 1), (W + S - 1, 1), (W + S, 2), (sr, 98)):
        assert mfcc_reference(np.zeros(L), sr).shape == (want, 39)
        assert num_frames(L, sr) == want
        assert _lib.lib().wavlm_mfcc_frames(L, W, S) == want


def test_frame_counts_16k_as_stated():
    from unispeech_amd.mfcc import mfcc_reference
    got = [len(mfcc_reference(np.zeros(L), 16000)) for L in (399, 400, 559, 560, 16000)]
    assert got == [0, 1, 1, 2, 98]


def test_dct_rows_are_scipys_orthonormal_dct():
    from unispeech_amd.mfcc import dct_lifter
    lifter = 1.0 + 11.0 * np.sin(math.pi * np.arange(13) / 22.0)
    want = scipy.fft.dct(np.eye(23), type=2, norm="ortho", axis=0)[:13]
    assert np.abs(dct_lifter() / lifter[:, None] - want).max() < 1e-14
    x = np.random.default_rng(0).standard_normal(23)
    assert np.abs(dct_lifter() @ x - scipy.fft.dct(x, type=2, norm="ortho")[:13] * lifter).max() < 1e-12


def test_power_spectrum_is_a_direct_dft():
    """one frame through the oracle's steps up to the power spectrum against an O(N^2) DFT of the padded frame, and the
    cepstra rebuilt from that spectrum against the oracle's"""
    from unispeech_amd.mfcc import EPS32, dct_lifter, mel_filters, mfcc_reference, tables
    sr = 16000
    t = tables(sr)
    x = MC.signal(400, sr, 1).astype(np.float64) / 32768.0
    f = x - x.mean()
    f = f - 0.97 * np.concatenate([f[:1], f[:-1]])
    f = np.concatenate([f * (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(400) / 399)) ** 0.85, np.zeros(112)])
    k = np.arange(257)[:, None] * np.arange(512)[None, :]
    power = np.abs((np.exp(-2j * np.pi * k / 512) * f[None, :]).sum(1)) ** 2
    assert np.abs(power - np.abs(np.fft.rfft(f)) ** 2).max() < 1e-9 * power.max()
    c = dct_lifter() @ np.log(np.maximum(mel_filters(sr) @ power, EPS32))
    assert np.abs(c - mfcc_reference(x, sr, deltas=False)[0]).max() < 1e-9
    # the kernel's tables: the twiddles are the DFT's and the sparse form is the dense filter bank
    assert np.abs(t["twiddle"][:, 0] + 1j * t["twiddle"][:, 1] - np.exp(-2j * np.pi * np.arange(512) / 512)).max() < 1e-15
    dense = np.zeros((23, 257))
    for b, (first, count, off) in enumerate(t["mel_idx"]):
        dense[b, first:first + count] = t["mel_w"][off:off + count]
    assert np.array_equal(dense, mel_filters(sr))


def test_mel_filter_sparsity():
    from unispeech_amd.mfcc import mel_filters, tables
    f = mel_filters(16000)
    nz = (f > 0).sum(1).tolist()
    assert nz[:4] == [5, 6, 7, 7] and nz[-2:] == [47, 52] and sum(nz) == 480
    assert nz == sorted(nz)
    for sr in (16000, 8000):
        f = mel_filters(sr)
        assert (f > 0).sum(0).max() == 2 and np.all(f[:, -1] == 0) and np.all(f[:, 0] == 0)
        t = tables(sr)
        assert t["mel_idx"][:, 1].sum() == len(t["mel_w"]) <= t["P"] and np.all(t["mel_w"] > 0)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_digital_silence_sits_on_the_floor(dtype):
    from unispeech_amd.mfcc import EPS32, mfcc_reference
    r = mfcc_reference(np.zeros(2000), 16000, dtype)
    assert r.dtype == dtype and r.shape == (11, 39)
    c0 = math.sqrt(23.0) * math.log(EPS32)
    assert abs(c0 + 76.457) < 1e-3
    tol = 1e-9 if dtype == np.float64 else 1e-4
    assert np.abs(r[:, 0] - c0).max() < tol and np.abs(r[:, 1:13]).max() < tol
    assert np.all(r[:, 13:] == 0)


def test_delta_edges_replicate_the_rows_own_ends():
    from unispeech_amd.mfcc import compute_deltas_reference
    c = np.array([[1.0], [4.0], [9.0], [16.0], [25.0]])
    assert np.array_equal(compute_deltas_reference(c[:1]), [[0.0]])
    # two frames: t = 0 sees (c0, c0, c0, c1, c1), t = 1 sees (c0, c0, c1, c1, c1)
    assert np.allclose(compute_deltas_reference(c[:2]), [[(3 + 2 * 3) / 10], [(3 + 2 * 3) / 10]])
    want = []
    for t in range(5):
        at = lambda k: c[min(max(t + k, 0), 4), 0]
        want.append([(-2 * at(-2) - at(-1) + at(1) + 2 * at(2)) / 10])
    assert np.allclose(compute_deltas_reference(c), want)
    assert np.allclose(compute_deltas_reference(c)[0], (3 + 2 * 8) / 10) and np.allclose(compute_deltas_reference(c)[2], 6.0)


def test_refused_options_name_the_argument():
    from unispeech_amd.mfcc import check_options, mfcc
    refused = dict(dither=1.0, use_energy=True, snip_edges=False, vtln_warp=1.1, htk_compat=True, subtract_mean=True,
                   window_type="hamming", num_mel_bins=40, num_ceps=20, low_freq=0.0, high_freq=-400.0, cepstral_lifter=0.0)
    for name, value in refused.items():
        with pytest.raises(NotImplementedError, match=name):
            mfcc(None, 16000, **{name: value})       # refused before the waveform is looked at
    check_options(dither=0.0, use_energy=False, snip_edges=True, vtln_warp=1.0, window_type="povey", num_mel_bins=23,
                  num_ceps=13, low_freq=20.0, high_freq=0.0, cepstral_lifter=22.0, htk_compat=False, subtract_mean=False)
    with pytest.raises(TypeError):
        check_options(no_such_option=1)


def test_supported_query_is_a_host_function():
    from unispeech_amd import _lib
    from unispeech_amd.mfcc import geometry, mfcc
    L = _lib.lib()
    assert L.wavlm_mfcc_supported(*geometry(16000)) == 1 and L.wavlm_mfcc_supported(*geometry(8000)) == 1
    assert L.wavlm_mfcc_supported(513, 160, 512) == 0        # a window longer than its padded size
    assert L.wavlm_mfcc_supported(400, 160, 500) == 0        # not a power of two
    assert L.wavlm_mfcc_supported(400, 160, 1024) == 0       # not the next power of two
    assert L.wavlm_mfcc_supported(*geometry(22050)) == 0     # a 1024-point transform is not built
    assert L.wavlm_mfcc_supported(400, 0, 512) == 0 and L.wavlm_mfcc_supported(400, 401, 512) == 0
    with pytest.raises(NotImplementedError, match="22050"):
        mfcc(None, 22050)
    assert L.wavlm_mfcc_frames(1000, 0, 160) == -1


def test_cli_takes_the_reference_positionals():
    from unispeech_amd import kmeans
    a = kmeans._parser().parse_args(["dump_mfcc", "TSV", "train", "4", "1", "FEAT"])
    assert (a.tsv_dir, a.split, a.nshard, a.rank, a.feat_dir, a.sample_rate) == ("TSV", "train", 4, 1, "FEAT", 16000)
    a = kmeans._parser().parse_args(["dump_mfcc", "TSV", "train", "4", "1", "FEAT", "--sample_rate", "8000"])
    assert a.sample_rate == 8000
    a = kmeans._parser().parse_args(["label_audio", "TSV", "train", "-", "-", "km.npz", "4", "1", "LAB", "--features", "mfcc"])
    assert a.features == "mfcc" and a.layer is None and a.ckpt_path == "-" and a.sample_rate == 16000
    a = kmeans._parser().parse_args(["label_audio", "TSV", "train", "ckpt.pt", "9", "km.npz", "4", "1", "LAB"])
    assert a.features is None and a.layer == 9 and a.max_chunk == 1600000
    with pytest.raises(SystemExit):
        kmeans.main(["dump_mfcc", "TSV", "train", "4"])
    with pytest.raises(SystemExit):
        kmeans.main(["label_audio", "TSV", "train", "ckpt.pt", "nine", "km.npz", "4", "1", "LAB"])


def test_feature_source_arguments():
    from unispeech_amd import kmeans
    with pytest.raises(NotImplementedError, match="fbank"):
        kmeans.label_audio(None, np.zeros(1000), None, np.zeros((2, 39), np.float32), features="fbank")
    with pytest.raises(ValueError):
        kmeans._check_features(object(), "mfcc")
    with pytest.raises(ValueError):
        kmeans._check_features(None, None)


def test_near_tie_share_of_the_label_case_is_capped():
    """stands behind tests/test_mfcc_gpu.py::test_labels: from the float64 oracle alone, at most 2 % of the frames are near
    ties (d2 - d1 <= 2 (sqrt d1 + sqrt d2) Delta, Delta = sqrt(39) * 4 * max_j E32[j]) for its inputs and centres"""
    pcm, centres, labels, tie, e = MC.label_case()
    assert centres.shape == (100, 39) and len(np.unique(centres, axis=0)) == 100
    assert len(labels) == 298
    print("near-tie share %.4f, max E32 %.3e" % (tie.mean(), e.max()))
    assert tie.mean() <= 0.02
