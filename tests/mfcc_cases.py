"""Inputs and float64 / float32 oracles shared by tests/test_mfcc.py (CPU) and tests/test_mfcc_gpu.py: computed once, never
modified.  Signals are broadband -- white noise plus a tone that sweeps from 300 Hz to a quarter of the rate, under a slow
amplitude envelope -- and quantised to int16 steps, so low-energy mel bands are not pure rounding noise."""
import numpy as np

from oracle_cache import OracleCache

TILE = 56   # csrc/mfcc.hip MF_FT: output frames per workgroup

_SIGNALS, _LABEL = {}, {}


def signal(L, sr, seed, zero=None):
    """int16 PCM [L]; zero = (a, b): samples a .. b - 1 are exact zeros"""
    key = (L, sr, seed, zero)
    if key not in _SIGNALS:
        rng = np.random.default_rng(seed)
        t = np.arange(L, dtype=np.float64) / sr
        dur = max(L / sr, 1e-3)
        phase = 2 * np.pi * (300.0 * t + 0.5 * (sr / 4 - 300.0) / dur * t * t)
        env = 0.55 + 0.45 * np.sin(2 * np.pi * 3.0 * t + seed)
        x = env * (0.05 * rng.standard_normal(L) + 0.3 * np.sin(phase))
        pcm = np.clip(np.round(x * 32767.0), -32768, 32767).astype(np.int16)
        if zero is not None:
            pcm[zero[0]:zero[1]] = 0
        pcm.setflags(write=False)
        _SIGNALS[key] = pcm
    return _SIGNALS[key]


def _reference(x, dtype, sr):
    from unispeech_amd.mfcc import mfcc_reference
    return mfcc_reference(x, sr, dtype)


_ORACLE = OracleCache(_reference, 39)
refs = _ORACLE.refs   # refs(pcm, sr) -> (float64 oracle, float32 oracle) [frames, 39] of pcm / 32768
e32 = _ORACLE.e32     # e32(rows, sr) -> E32[j]: per column the largest |float32 oracle - float64 oracle| over the rows' frames


def lengths(sr):
    """one frame, one sample short of two, two, just short of six, and two workgroup tiles plus 17 frames and 37 samples"""
    from unispeech_amd.mfcc import geometry
    W, S, _ = geometry(sr)
    return [W, W + S - 1, W + S, 3 * W - 1, W + (2 * TILE + 16) * S + 37]


def parity_rows(sr):
    return [signal(L, sr, 11 + i) for i, L in enumerate(lengths(sr))]


def batch_rows(sr):
    """B = 3: a multi-tile row with a stretch of exact zeros, a row shorter than the window, a short row"""
    from unispeech_amd.mfcc import geometry
    W, S, _ = geometry(sr)
    L0 = W + (TILE + 30) * S + 5
    z = (20 * S + 3, 20 * S + 3 + W + 14 * S)          # frames 21 .. 34 lie wholly inside it
    return [signal(L0, sr, 5, zero=z), signal(W - 50, sr, 6), signal(3 * W - 1, sr, 7)], z


def label_case():
    """3 s at 16 kHz with half a second of digital silence, 100 centres drawn from its UNIQUE float64 feature rows (the silent
    frames are one row, so at most one centre), rounded to fp32 as the device holds them.
    -> (pcm, centres fp32 [100, 39], labels of the float64 oracle, near-tie mask, E32)"""
    if not _LABEL:
        sr = 16000
        pcm = signal(48000, sr, 3, zero=(20000, 28000))
        r64, _ = refs(pcm, sr)
        e = e32([pcm], sr)
        uniq = np.unique(r64, axis=0)
        pick = np.random.default_rng(0).choice(len(uniq), 100, replace=False)
        centres = uniq[pick].astype(np.float32)
        d = ((r64[:, None, :] - centres.astype(np.float64)[None]) ** 2).sum(-1)
        order = np.sort(d, axis=1)
        d1, d2 = order[:, 0], order[:, 1]
        delta = np.sqrt(39.0) * 4.0 * e.max()
        tie = (d2 - d1) <= 2.0 * (np.sqrt(d1) + np.sqrt(d2)) * delta
        _LABEL.update(v=(pcm, centres, d.argmin(1), tie, e))
    return _LABEL["v"]
