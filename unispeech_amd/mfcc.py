"""Kaldi MFCC + deltas on the device (csrc/mfcc.hip, ABI 28): the features of HuBERT's first k-means iteration, what the
reference's src/examples/hubert/simple_kmeans/dump_mfcc_feature.py:46-55 computes per utterance on the CPU,
`torchaudio.compliance.kaldi.mfcc(waveform, sample_frequency=sr, use_energy=False)` with every other argument at its default,
`torchaudio.functional.compute_deltas` twice, and the concatenation [c | d | dd]: 39 columns at 100 frames / s.

    W = int(sr * 0.025);  S = int(sr * 0.010);  P = next power of two >= W
    frames   m = 1 + (len - W) // S   (0 when len < W);  frame i = x[i * S : i * S + W]
    per frame: subtract the mean;  y[j] = x[j] - 0.97 * x[max(j - 1, 0)];  times (0.5 - 0.5 cos(2 pi n / (W - 1))) ** 0.85;
               zero-pad to P;  |rfft_P| ** 2;  23 triangular filters on mel = 1127 ln(1 + f / 700) from 20 Hz to Nyquist
               (weights on bins k < P / 2, the Nyquist bin weighs 0);  log(max(E, 2 ** -23));
               first 13 rows of the orthonormal DCT-II;  times 1 + 11 sin(pi i / 22)
    deltas   d[t] = sum_{k = -2 .. 2} k * c[clamp(t + k, 0, m - 1)] / 10, twice

  * `tables` -- window, twiddles, the mel filters by filter (first bin, count, weights) and DCT x lifter in float64;
    `mfcc` -- the device op, one launch per call; `MfccFeatureReader` -- dump_mfcc_feature.py's class over it.
  * `mfcc_reference` -- the same statement on the CPU in float64 or float32 with numpy's rfft: the tests' and tools' oracle,
    nothing else calls it.
torchaudio is not a dependency and was never run against this: agreement is with the restatement above of its published
source.  The waveform is taken in [-1, 1] as the recipe feeds it (soundfile's values), not in Kaldi's 16-bit integer range.
No CPU path: a CPU tensor is refused like in every other op.
"""
import math

import numpy as np
import torch

from . import _lib
from . import ops
from . import wavein

__all__ = ["geometry", "num_frames", "tables", "mel_filters", "dct_lifter", "mfcc", "MfccFeatureReader", "mfcc_reference",
           "compute_deltas_reference", "check_options"]

NUM_MEL, NUM_CEPS, WIDTH = 23, 13, 39
EPS32 = 1.1920928955078125e-07   # torch.finfo(torch.float32).eps: the floor of the mel energies

# torchaudio.compliance.kaldi.mfcc's keyword arguments and defaults; anything else than the default is refused by name
KALDI_DEFAULTS = dict(blackman_coeff=0.42, cepstral_lifter=22.0, channel=-1, dither=0.0, energy_floor=1.0, frame_length=25.0,
                      frame_shift=10.0, high_freq=0.0, htk_compat=False, low_freq=20.0, num_ceps=13, min_duration=0.0,
                      num_mel_bins=23, preemphasis_coefficient=0.97, raw_energy=True, remove_dc_offset=True,
                      round_to_power_of_two=True, snip_edges=True, subtract_mean=False, use_energy=False, vtln_high=-500.0,
                      vtln_low=100.0, vtln_warp=1.0, window_type="povey")


def check_options(**options):
    """NotImplementedError naming the first kaldi.mfcc argument that is not at the value this op is built for"""
    for name, value in options.items():
        if name not in KALDI_DEFAULTS:
            raise TypeError("mfcc() got an unexpected keyword argument %r" % name)
        want = KALDI_DEFAULTS[name]
        if isinstance(want, (str, bool)):
            same = value == want
        else:
            same = isinstance(value, (int, float)) and float(value) == float(want)
        if not same:
            raise NotImplementedError("mfcc: %s=%r is not implemented (the device op is built for kaldi.mfcc's %s=%r, the "
                                      "first-iteration HuBERT recipe)" % (name, value, name, want))


def geometry(sample_rate):
    """-> (W, S, P): window, shift, padded window in samples"""
    sr = float(sample_rate)
    if not sr > 0:
        raise ValueError("sample_rate=%r" % (sample_rate,))
    W, S = int(sr * 0.025), int(sr * 0.010)
    if W < 2 or S < 1:
        raise ValueError("sample_rate=%r: a window of %d samples" % (sample_rate, W))
    return W, S, 1 << (W - 1).bit_length()


def num_frames(length, sample_rate=16000):
    """frames of a `length`-sample row (snip_edges=True): the count csrc/mfcc.hip's wavlm_mfcc_frames gives"""
    W, S, _ = geometry(sample_rate)
    length = int(length)
    return 0 if length < W else 1 + (length - W) // S


def _mel(f):
    return 1127.0 * np.log(1.0 + np.asarray(f, dtype=np.float64) / 700.0)


def mel_filters(sample_rate):
    """float64 [23, P / 2 + 1]: kaldi get_mel_banks (no VTLN) with the zero Nyquist column fbank pads on"""
    _, _, P = geometry(sample_rate)
    sr = float(sample_rate)
    lo, hi = _mel(20.0), _mel(0.5 * sr)
    delta = (hi - lo) / (NUM_MEL + 1)
    left = lo + np.arange(NUM_MEL, dtype=np.float64)[:, None] * delta
    centre, right = left + delta, left + 2.0 * delta
    mel = _mel(np.arange(P // 2, dtype=np.float64) * (sr / P))[None, :]
    w = np.maximum(0.0, np.minimum((mel - left) / delta, (right - mel) / delta))
    return np.concatenate([w, np.zeros((NUM_MEL, 1))], axis=1)


def dct_lifter():
    """float64 [13, 23]: rows 0 .. 12 of the orthonormal DCT-II over 23 points, row i times 1 + 11 sin(pi i / 22)"""
    n = np.arange(NUM_MEL, dtype=np.float64)[None, :]
    k = np.arange(NUM_CEPS, dtype=np.float64)[:, None]
    dct = np.cos(math.pi / NUM_MEL * (n + 0.5) * k) * math.sqrt(2.0 / NUM_MEL)
    dct[0] = math.sqrt(1.0 / NUM_MEL)
    return dct * (1.0 + 11.0 * np.sin(math.pi * k / 22.0))


def tables(sample_rate):
    """everything the kernel is handed, float64 (rounded to fp32 once on the way to the device):
    window [W]; twiddle [P, 2] = (cos, -sin)(2 pi t / P); mel_idx int32 [23, 3] = (first bin, count, offset into mel_w) and
    mel_w [sum of counts]: filter b is sum_i mel_w[offset + i] * power[first + i]; dct [13, 23] with the lifter folded in"""
    W, S, P = geometry(sample_rate)
    n = np.arange(W, dtype=np.float64)
    window = (0.5 - 0.5 * np.cos(2.0 * math.pi * n / (W - 1))) ** 0.85
    mel_idx, mel_w = wavein.pack_filters(mel_filters(sample_rate))
    return dict(W=W, S=S, P=P, window=window, twiddle=wavein.twiddle(P), mel_idx=mel_idx, mel_w=mel_w, dct=dct_lifter())


def _check_supported(sample_rate, W, S, P):
    if not _lib.lib().wavlm_mfcc_supported(min(W, 1 << 30), min(S, 1 << 30), min(P, 1 << 30)):
        raise NotImplementedError("mfcc at %r Hz (window %d, shift %d, transform %d): the kernel takes transforms of 64 to 512 "
                                  "points (16000 and 8000 Hz are the built rates)" % (sample_rate, W, S, P))


_TABLES = {}   # (sample_rate, device) -> the fp32 / int32 tables on that device


def _device_tables(sample_rate, device):
    key = (float(sample_rate), str(device))
    hit = _TABLES.get(key)
    if hit is None:
        t = tables(sample_rate)
        hit = {k: wavein.upload(t[k], device) for k in ("window", "twiddle", "mel_idx", "mel_w", "dct")}
        _TABLES[key] = hit
    return hit


def mfcc(wavs, sample_rate=16000, lengths=None, deltas=True, **kaldi_options):
    """wavs: [B, L] (or [L]) float32 in [-1, 1] or int16 PCM on the device, unit sample stride, any row stride -- or a list of
    1-D device tensors of unequal length (one dtype), which are padded into one batch.  lengths (optional, B sample counts):
    a row ends there.  -> (features float32 [B, Mmax, 39] ([Mmax, 39] for 1-D input; 13 columns with deltas=False), frames
    per row as a list of ints): rows at or beyond a row's own frame count are zero, Mmax is the frame count of L.  One launch.
    kaldi_options: torchaudio's kaldi.mfcc arguments, accepted at their defaults only (NotImplementedError by name)."""
    check_options(**kaldi_options)
    W, S, P = geometry(sample_rate)
    _check_supported(sample_rate, W, S, P)
    wave, B, L, xs, len_l, len_t, squeeze, dev = wavein.as_batch(wavs, lengths, "mfcc")
    frames = [num_frames(v, sample_rate) for v in len_l]
    Mmax = num_frames(L, sample_rate)
    ncol = WIDTH if deltas else NUM_CEPS
    out = torch.empty((B, Mmax, ncol), dtype=torch.float32, device=dev)
    if Mmax:
        t = _device_tables(sample_rate, dev)
        _lib.check(_lib.lib().wavlm_mfcc_rows(
            ops.ptr(wave), wavein.dtype_code(wave), xs, B, L, ops.ptr(len_t), W, S, P, ops.ptr(t["window"]),
            ops.ptr(t["twiddle"]), ops.ptr(t["mel_idx"]), ops.ptr(t["mel_w"]), t["mel_w"].numel(), ops.ptr(t["dct"]),
            ops.ptr(out), Mmax * ncol, Mmax, ncol, ops.stream()), "wavlm_mfcc_rows")
    return (out[0] if squeeze else out), frames


class MfccFeatureReader:
    """dump_mfcc_feature.MfccFeatureReader: get_feats(path) -> float32 [frames, 39] on the device.  A waveform (1-D array or
    tensor, float in [-1, 1] or int16 PCM) is taken in place of a path."""

    def __init__(self, sample_rate):
        self.sample_rate = sample_rate

    def read_audio(self, path, ref_len=None):
        from .kmeans import read_wav
        wav, sr = read_wav(path)
        assert sr == self.sample_rate, sr
        return wav

    def get_feats(self, path, ref_len=None):
        x = self.read_audio(path, ref_len) if isinstance(path, (str, bytes)) or hasattr(path, "__fspath__") else path
        x = torch.as_tensor(x)
        if x.dim() != 1:
            raise ValueError("get_feats takes one waveform [L], got %s" % (tuple(x.shape),))
        if x.dtype != torch.int16:
            x = x.to(torch.float32)
        if x.numel() == 0:
            return torch.zeros((0, WIDTH), dtype=torch.float32, device="cuda")
        return mfcc(x.cuda(), self.sample_rate)[0]


# --------------------------------------------------------------------------------------------------------- CPU oracle
def compute_deltas_reference(c):
    """torchaudio.functional.compute_deltas (win_length 5, replicate) along axis 0 of c [m, D], in c's dtype"""
    m = c.shape[0]
    if m == 0:
        return c.copy()
    at = lambda k: c[np.clip(np.arange(m) + k, 0, m - 1)]
    # the mirrored pairs first: the same sum, and a constant stretch gives exactly 0 in any precision
    return ((at(1) - at(-1)) + c.dtype.type(2.0) * (at(2) - at(-2))) / c.dtype.type(10.0)


def mfcc_reference(x, sample_rate=16000, dtype=np.float64, deltas=True):
    """the module docstring's statement on the CPU for one waveform x [L] (values as given: scale int16 PCM by 1 / 32768 first),
    in `dtype` (float64, or float32: the tables rounded to fp32, every product and sum and numpy's rfft in fp32, the precision
    the reference computes at) -> numpy [frames, 39] (13 with deltas=False)"""
    dtype = np.dtype(dtype)
    if dtype not in (np.dtype(np.float64), np.dtype(np.float32)):
        raise TypeError("mfcc_reference computes in float64 or float32")
    x = np.asarray(torch.as_tensor(x).detach().cpu().numpy() if isinstance(x, torch.Tensor) else x).astype(dtype)
    if x.ndim != 1:
        raise ValueError("mfcc_reference takes one waveform [L]")
    t = tables(sample_rate)
    W, S, P = t["W"], t["S"], t["P"]
    m = num_frames(len(x), sample_rate)
    ncol = WIDTH if deltas else NUM_CEPS
    if m == 0:
        return np.zeros((0, ncol), dtype=dtype)
    fr = x[np.arange(m)[:, None] * S + np.arange(W)[None, :]]
    fr = fr - fr.mean(axis=1, keepdims=True, dtype=dtype)
    fr = fr - dtype.type(0.97) * np.concatenate([fr[:, :1], fr[:, :-1]], axis=1)
    fr = fr * t["window"].astype(dtype)[None, :]
    fr = np.concatenate([fr, np.zeros((m, P - W), dtype=dtype)], axis=1)
    spec = np.fft.rfft(fr, axis=1)
    power = (np.abs(spec) ** 2).astype(dtype)
    mel = power @ mel_filters(sample_rate).astype(dtype).T
    logmel = np.log(np.maximum(mel, dtype.type(EPS32)))
    c = (logmel @ t["dct"].astype(dtype).T).astype(dtype)
    if not deltas:
        return c
    d = compute_deltas_reference(c)
    return np.concatenate([c, d, compute_deltas_reference(d)], axis=1)
