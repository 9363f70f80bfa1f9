"""Inputs and float64 / float32 oracles shared by tests/test_fbank.py (CPU), tests/test_fbank_gpu.py and
tools/gen_speaker_fbank_golden.py: computed once, never modified.  Parity signals are a few sinusoids plus white noise at 1e-2,
quantised to int16 steps, so no mel column sits on the 1e-6 term; a case is several rows of one length.  `speaker_wave` refills the golden's waveforms from a seed."""
import numpy as np

from oracle_cache import OracleCache

TILE = 56   # csrc/fbank.hip FB_NF: frames per workgroup
LENGTHS = (257, 1600, 16037)   # 2 frames, both under both reflections; last frame centred on the end; one tile + 45 frames
GOLDEN_LENGTHS = (24000, 16037, 24000, 11000)

_SIGNALS = {}


def signal(L, seed):
    """int16 PCM [L] at 16 kHz"""
    key = (L, seed)
    if key not in _SIGNALS:
        rng = np.random.default_rng(seed)
        t = np.arange(L, dtype=np.float64) / 16000.0
        x = 1e-2 * rng.standard_normal(L)
        for f, a in ((220.0, 0.2), (1330.0, 0.1), (3470.0, 0.05), (6100.0, 0.02)):
            x += a * np.sin(2 * np.pi * (f + 10.0 * seed) * t + rng.uniform(0, 2 * np.pi))
        pcm = np.clip(np.round(x * 32767.0), -32768, 32767).astype(np.int16)
        pcm.setflags(write=False)
        _SIGNALS[key] = pcm
    return _SIGNALS[key]


def case_rows(L):
    """the rows of the case of length L: 8 x 2, 4 x 11 and 2 x 101 frames, so that E32 is a maximum over at least 16 numbers per
    column (over the 2 frames of one 257-sample row it would say nothing about a precision)"""
    return [signal(L, 31 + 7 * LENGTHS.index(L) + i) for i in range({257: 8, 1600: 4, 16037: 2}[L])]


def _reference(x, dtype):
    from unispeech_amd.fbank import fbank_reference
    return fbank_reference(x, dtype=dtype)


_ORACLE = OracleCache(_reference, 40)
refs = _ORACLE.refs   # refs(pcm) -> (float64 oracle, float32 oracle) [T, 40] of pcm / 32768
e32 = _ORACLE.e32     # e32(rows) -> E32[m]: per mel column the largest |float32 oracle - float64 oracle| over the rows' frames


def speaker_wave(seed, L, speaker):
    """float32 [L] in [-1, 1], int16-quantised: six frequency-modulated tones, each switched on and off at its own rate, plus
    noise.  The tones' frequencies and rates belong to the speaker, the phases to the utterance: what survives the per-column
    instance norm is the pattern across time and columns, so that is where the speakers differ"""
    rng = np.random.default_rng(seed)
    srng = np.random.default_rng(1000 + speaker)
    t = np.arange(L, dtype=np.float64) / 16000.0
    x = np.zeros(L)
    for f, r in zip(srng.uniform(200.0, 7000.0, 6), srng.uniform(1.0, 15.0, 6)):
        env = np.clip(np.sin(2 * np.pi * r * t + rng.uniform(0, 6.28)), 0.0, None) ** 2
        x += env * np.sin(2 * np.pi * f * t + 30.0 * np.sin(2 * np.pi * rng.uniform(2.0, 6.0) * t))
    x = 0.2 * x / np.abs(x).max() + 3e-3 * rng.standard_normal(L)
    return (np.clip(np.round(x * 32767.0), -32768, 32767) / 32768.0).astype(np.float32)


def golden_waves(seed):
    """four utterances, two per speaker: (0, 1) and (2, 3)"""
    return [speaker_wave(seed + i, L, i // 2) for i, L in enumerate(GOLDEN_LENGTHS)]
