"""Log-mel filter bank on the device (csrc/fbank.hip, ABI 29): the front end of the reference's ECAPA-TDNN baseline without an
upstream model, downstreams/speaker_verification/models/ecapa_tdnn.py:179-182, 253, 257 (`feat_type='fbank'`):
`torchaudio.transforms.MelSpectrogram(sample_rate=sr, n_fft=P, win_length=W, hop_length=S, f_min=0, f_max=sr // 2, pad=0,
n_mels=M)` with everything else at torchaudio 0.9's defaults (periodic Hann window, power 2, center, reflect, one-sided, not
normalised, HTK mel scale, no filter norm), then `+ 1e-6` and `log`.  The speaker model: P = 512, W = int(0.025 sr) = 400,
S = int(0.010 sr) = 160, M = 40.

    T = 1 + L // S frames.  Frame t holds samples i = t S - P / 2 ... t S + P / 2 - 1 of the row, reflected without repeating
        the edge: i < 0 -> -i;  i >= L -> 2 (L - 1) - i.  Needs L > P / 2 (torch refuses the padding otherwise).
    window w[n] = 0.5 - 0.5 cos(2 pi n / W), n < W, placed at offset (P - W) // 2 of the P-point frame, zero elsewhere
    power[k] = re^2 + im^2 of rfft_P, k = 0 .. P / 2
    mel(f) = 2595 log10(1 + f / 700);  M + 2 points equally spaced in mel from mel(0) to mel(sr // 2), back to Hz: f_pts
    bin frequencies f_k = linspace(0, sr // 2, P / 2 + 1);
    fb[k, m] = max(0, min((f_k - f_pts[m]) / (f_pts[m + 1] - f_pts[m]), (f_pts[m + 2] - f_k) / (f_pts[m + 2] - f_pts[m + 1])))
    logmel[t, m] = log(sum_k fb[k, m] power[t, k] + 1e-6)

  * `tables` -- window, twiddles and the mel bank by filter (first bin, count, weights) in float64; `frames` -- the frame count;
    `fbank` -- the device op, one launch per call, [B, T, M] channel-last (the layout the speaker head reads).
  * `fbank_reference` -- the same statement on the CPU in float64 or float32 with numpy's rfft: the tests' and tools' oracle,
    nothing else calls it.
torchaudio is not a dependency and was never run against this: agreement is with the restatement above of its published source,
and tests/test_fbank.py checks the restatement against `torch.stft`, which is what torchaudio's Spectrogram calls.
No CPU path: a CPU tensor is refused like in every other op.
"""
import math

import numpy as np
import torch

from . import _lib
from . import ops
from . import wavein

__all__ = ["geometry", "frames", "tables", "mel_bank", "fbank", "fbank_reference", "check_options", "LOG_ADD"]

LOG_ADD = 1e-6     # ecapa_tdnn.py:253: the constant added before the log
MAX_MELS = 128     # csrc/fbank.hip FB_MAX_MEL

# MelSpectrogram's remaining arguments in the order they are checked, with the value the op is built for (f_max: sr // 2, which
# is also what None means to torchaudio); anything else is refused by name
MEL_OPTIONS = ("power", "center", "pad_mode", "norm", "mel_scale", "normalized", "window_fn", "f_min", "f_max", "pad")


def check_options(sr=16000, **options):
    """NotImplementedError naming the first MelSpectrogram argument that is not at the value this op is built for"""
    for name in options:
        if name not in MEL_OPTIONS:
            raise TypeError("fbank() got an unexpected keyword argument %r" % name)
    built = dict(power=2.0, center=True, pad_mode="reflect", norm=None, mel_scale="htk", normalized=False,
                 window_fn=torch.hann_window, f_min=0.0, f_max=float(int(sr) // 2), pad=0)
    for name in MEL_OPTIONS:
        if name not in options:
            continue
        value, want = options[name], built[name]
        if name == "f_max" and value is None:
            continue
        if name == "window_fn" or want is None:
            same = value is want
        elif isinstance(want, (str, bool)):
            same = type(value) is type(want) and value == want
        else:
            same = isinstance(value, (int, float)) and not isinstance(value, bool) and float(value) == float(want)
        if not same:
            raise NotImplementedError("fbank: %s=%r is not implemented (the device op is built for MelSpectrogram's %s=%r, the "
                                      "ECAPA-TDNN baseline's front end)" % (name, value, name, want))


def geometry(sr=16000, n_fft=512, win_length=None, hop_length=None):
    """-> (W, S, P): window, hop, transform size in samples; the reference's int(sr * 0.025) / int(sr * 0.010) by default"""
    if not float(sr) > 0 or int(sr) != sr:
        raise ValueError("sr=%r" % (sr,))
    W = int(sr * 0.025) if win_length is None else int(win_length)
    S = int(sr * 0.010) if hop_length is None else int(hop_length)
    return W, S, int(n_fft)


def frames(n, S=160, P=512):
    """frames of an n-sample row (center=True): the count csrc/fbank.hip's wavlm_fbank_frames gives, 0 where torch refuses to
    reflect (n <= P / 2)"""
    n = int(n)
    return 0 if n <= P // 2 else 1 + n // S


def _mel(f):
    return 2595.0 * np.log10(1.0 + np.asarray(f, dtype=np.float64) / 700.0)


def mel_bank(sr, P, M):
    """float64 [P / 2 + 1, M]: torchaudio's create_fb_matrix(P / 2 + 1, 0, sr // 2, M, sr), norm None, HTK scale"""
    f_max = float(int(sr) // 2)
    f_k = np.linspace(0.0, f_max, P // 2 + 1)
    m_pts = np.linspace(_mel(0.0), _mel(f_max), M + 2)
    f_pts = 700.0 * (10.0 ** (m_pts / 2595.0) - 1.0)
    f_pts[0], f_pts[-1] = 0.0, f_max     # their exact values: the round trip through mel leaves bin 0 and the Nyquist bin at weight 0
    f_diff = f_pts[1:] - f_pts[:-1]
    slopes = f_pts[None, :] - f_k[:, None]                        # [bins, M + 2]
    down = -slopes[:, :-2] / f_diff[:-1]
    up = slopes[:, 2:] / f_diff[1:]
    return np.maximum(0.0, np.minimum(down, up))


def tables(sr=16000, P=512, W=400, M=40):
    """everything the kernel is handed, float64 (rounded to fp32 once on the way to the device):
    window [W] (periodic Hann); twiddle [P, 2] = (cos, -sin)(2 pi t / P); mel_idx int32 [M, 3] = (first bin, count, offset into
    mel_w) and mel_w [sum of counts]: filter m is sum_i mel_w[offset + i] * power[first + i] (an empty filter: count 0)"""
    n = np.arange(W, dtype=np.float64)
    window = 0.5 - 0.5 * np.cos(2.0 * math.pi * n / W)
    mel_idx, mel_w = wavein.pack_filters(mel_bank(sr, P, M).T)
    return dict(W=W, P=P, M=M, window=window, twiddle=wavein.twiddle(P), mel_idx=mel_idx, mel_w=mel_w)


def _check_supported(sr, W, S, P, M):
    lim = 1 << 30
    if not _lib.lib().wavlm_fbank_supported(max(min(W, lim), -1), max(min(S, lim), -1), max(min(P, lim), -1), max(min(M, lim), -1)):
        raise NotImplementedError("fbank with n_fft=%d, win_length=%d, hop_length=%d, n_mels=%d at %r Hz: the kernel takes "
                                  "transforms of 64 to 512 points (a power of two), n_fft / 2 < win_length <= n_fft, 1 <= "
                                  "hop_length <= win_length and at most %d mel filters" % (P, W, S, M, sr, MAX_MELS))


_TABLES = {}   # (sr, P, W, M, device) -> the fp32 / int32 tables on that device


def _device_tables(sr, P, W, M, device):
    key = (int(sr), P, W, M, str(device))
    hit = _TABLES.get(key)
    if hit is None:
        t = tables(sr, P, W, M)
        hit = {k: wavein.upload(t[k], device) for k in ("window", "twiddle", "mel_idx")}
        # the kernel wants a pointer even where no filter has a weight: one placeholder element, n_mel_w = 0
        hit.update(mel_w=wavein.upload(t["mel_w"] if len(t["mel_w"]) else np.zeros(1), device), n_mel_w=len(t["mel_w"]))
        _TABLES[key] = hit
    return hit


def fbank(wavs, lengths=None, sr=16000, n_mels=40, n_fft=512, win_length=None, hop_length=None, **mel_options):
    """wavs: [B, L] (or [L]) float32 in [-1, 1] or int16 PCM on the device, unit sample stride, any row stride -- or a list of
    1-D device tensors of unequal length (one dtype), which are padded into one batch.  lengths (optional, B sample counts):
    a row ends there and is reflected at its own end.  -> float32 [B, T, n_mels] ([T, n_mels] for 1-D input), T =
    frames(L, hop, n_fft): log(mel energy + 1e-6), channel-last; frames at or beyond a row's own count (frames(length, ...))
    are zero.  One launch.  mel_options: MelSpectrogram's other arguments, accepted at the values the op is built for only
    (NotImplementedError by name)."""
    check_options(sr, **mel_options)
    W, S, P = geometry(sr, n_fft, win_length, hop_length)
    M = int(n_mels)
    _check_supported(sr, W, S, P, M)
    wave, B, L, xs, _, len_t, squeeze, dev = wavein.as_batch(wavs, lengths, "fbank")
    T = frames(L, S, P)
    out = torch.empty((B, T, M), dtype=torch.float32, device=dev)
    if T:
        t = _device_tables(sr, P, W, M, dev)
        _lib.check(_lib.lib().wavlm_fbank_rows(
            ops.ptr(wave), wavein.dtype_code(wave), xs, B, L, ops.ptr(len_t), W, S, P, M, ops.ptr(t["window"]),
            ops.ptr(t["twiddle"]), ops.ptr(t["mel_idx"]), ops.ptr(t["mel_w"]), t["n_mel_w"], ops.ptr(out), T * M, T,
            ops.stream()), "wavlm_fbank_rows")
    return out[0] if squeeze else out


# --------------------------------------------------------------------------------------------------------- CPU oracle
def reflect_frames(x, S, P):
    """x [L] -> [T, P]: the centred frames of the module docstring, in x's dtype"""
    L = len(x)
    T = frames(L, S, P)
    i = np.arange(T)[:, None] * S - P // 2 + np.arange(P)[None, :]
    i = np.where(i < 0, -i, i)
    i = np.where(i >= L, 2 * (L - 1) - i, i)
    return x[i]


def fbank_reference(x, sr=16000, n_mels=40, n_fft=512, win_length=None, hop_length=None, dtype=np.float64, power=False):
    """the module docstring's statement on the CPU for one waveform x [L] (values as given: scale int16 PCM by 1 / 32768 first),
    in `dtype` (float64, or float32: the tables rounded to fp32, every product and sum and numpy's rfft in fp32, the precision
    the reference computes at) -> numpy [T, n_mels]; power=True: the power spectrum [T, n_fft / 2 + 1] instead"""
    dtype = np.dtype(dtype)
    if dtype not in (np.dtype(np.float64), np.dtype(np.float32)):
        raise TypeError("fbank_reference computes in float64 or float32")
    x = np.asarray(torch.as_tensor(x).detach().cpu().numpy() if isinstance(x, torch.Tensor) else x).astype(dtype)
    if x.ndim != 1:
        raise ValueError("fbank_reference takes one waveform [L]")
    W, S, P = geometry(sr, n_fft, win_length, hop_length)
    M = int(n_mels)
    if frames(len(x), S, P) == 0:
        return np.zeros((0, P // 2 + 1 if power else M), dtype=dtype)
    n = np.arange(W, dtype=np.float64)
    win = np.zeros(P, dtype=dtype)
    win[(P - W) // 2:(P - W) // 2 + W] = (0.5 - 0.5 * np.cos(2.0 * math.pi * n / W)).astype(dtype)
    fr = reflect_frames(x, S, P) * win[None, :]
    spec = np.fft.rfft(fr, axis=1)
    pw = (spec.real.astype(dtype) ** 2 + spec.imag.astype(dtype) ** 2).astype(dtype)
    if power:
        return pw
    mel = (pw @ mel_bank(sr, P, M).astype(dtype)).astype(dtype)
    return np.log(mel + dtype.type(LOG_ADD))
