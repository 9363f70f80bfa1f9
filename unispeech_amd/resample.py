"""Sinc resampling on the device (csrc/resample.hip, ABI 27): torchaudio.functional.resample with the defaults the reference
uses (`sinc_interpolation`, lowpass_filter_width 6, rolloff 0.99), the step its speaker and diarization recipes put in front
of the upstream (downstreams/speaker_diarization/models/models.py:138,207, downstreams/speaker_verification/verification.py:46-49).

    g = gcd(orig, new);  o = orig / g;  n = new / g
    base = min(o, n) * rolloff;   width = ceil(lowpass_filter_width * o / base)
    idx = arange(-width, width + o)                                          # 2 * width + o taps
    phase i in [0, n):  t = clamp((-i / n + idx / o) * base, -lpw, lpw)
                        h_i = cos(t * pi / (2 * lpw)) ** 2 * sinc(pi * t) * (base / o)
    x padded with `width` zeros left, `width + o` zeros right
    y[f * n + i] = sum_k h_i[k] * xpad[f * o + k];   output cut to ceil(n * L / o) samples

  * `sinc_table` -- that table in float64; `compact_table` -- what the kernel reads: per phase the 2 * width + 1 taps around the
    window's support and the index of the first (outside |t| < lpw the window is zero, about 1e-33 numerically).
  * `resample` -- the device op; `Resample` -- torchaudio.transforms.Resample's surface over it.
  * `resample_reference` -- the float64 CPU restatement (dense conv1d, all taps): the tests' oracle, nothing else calls it.
torchaudio is not a dependency and was never run against this: agreement is with the restatement of its published formula.
No CPU path: a CPU tensor is refused like in every other op.
"""
import math

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from . import ops
from . import wavein

__all__ = ["sinc_table", "compact_table", "resample", "Resample", "resample_reference", "output_length"]


def _geometry(orig, new, lowpass_filter_width=6, rolloff=0.99):
    orig, new = int(orig), int(new)
    if orig <= 0 or new <= 0:
        raise ValueError("sample rates must be positive, got %r -> %r" % (orig, new))
    if lowpass_filter_width <= 0:
        raise ValueError("lowpass_filter_width=%r" % (lowpass_filter_width,))
    g = math.gcd(orig, new)
    o, n = orig // g, new // g
    base = min(o, n) * rolloff
    return o, n, int(math.ceil(lowpass_filter_width * o / base)), base


def output_length(L, o, n):
    return (int(L) * n + o - 1) // o


def _phase_times(o, n, width, base):
    """t before the clamp, float64 [n, 2 * width + o]"""
    idx = np.arange(-width, width + o, dtype=np.float64)[None, :] / o
    return (np.arange(0, -n, -1, dtype=np.float64)[:, None] / n + idx) * base


def sinc_table(orig, new, lowpass_filter_width=6, rolloff=0.99):
    """-> (table float64 [n, 2 * width + o], width, o, n)"""
    o, n, width, base = _geometry(orig, new, lowpass_filter_width, rolloff)
    lpw = float(lowpass_filter_width)
    t = np.clip(_phase_times(o, n, width, base), -lpw, lpw)
    window = np.cos(t * math.pi / lpw / 2) ** 2
    t = t * math.pi
    safe = np.where(t == 0, 1.0, t)
    table = np.where(t == 0, 1.0, np.sin(safe) / safe) * window * (base / o)
    return table, width, o, n


def compact_table(orig, new, lowpass_filter_width=6, rolloff=0.99):
    """-> (taps float64 [n, 2 * width + 1], first int32 [n], width, o, n): taps[i, j] = table[i, first[i] + j] where the window
    is not zero (|t| < lowpass_filter_width), else 0.  An interval of length 2 * lpw * o / base <= 2 * width holds at most
    2 * width + 1 integers, so nothing inside the window is lost; first[i] <= o - 1 keeps every row inside the dense table."""
    table, width, o, n = sinc_table(orig, new, lowpass_filter_width, rolloff)
    base = min(o, n) * rolloff
    inside = np.abs(_phase_times(o, n, width, base)) < float(lowpass_filter_width)
    tc = 2 * width + 1
    if int(inside.sum(1).max()) > tc:
        raise AssertionError("a phase with more than 2 * width + 1 taps inside the window")
    first = np.minimum(inside.argmax(1), o - 1).astype(np.int32)
    cols = first[:, None].astype(np.int64) + np.arange(tc)[None, :]
    rows = np.arange(n)[:, None]
    taps = np.where(inside[rows, cols], table[rows, cols], 0.0)
    if int(inside.sum()) != int(inside[rows, cols].sum()):
        raise AssertionError("a tap inside the window fell outside its compact row")
    return taps, first, width, o, n


def _check_supported(orig, new, o, n, width):
    if not _lib.lib().wavlm_resample_supported(min(o, 1 << 30), min(n, 1 << 30), min(width, 1 << 30)):
        raise NotImplementedError(
            "resampling %d Hz -> %d Hz (ratio %d : %d, %d taps per phase): the compact filter table or its input tile exceeds "
            "the kernel's LDS budget (48 KiB of table, 32 KiB of samples)" % (orig, new, o, n, 2 * width + 1))


_TABLES = {}   # (orig, new, device) -> (taps fp32, first int32, o, n, width) on that device


def _device_table(orig, new, device):
    key = (int(orig), int(new), str(device))
    hit = _TABLES.get(key)
    if hit is None:
        taps, first, width, o, n = compact_table(orig, new)
        hit = (wavein.upload(taps, device), wavein.upload(first, device), o, n, width)
        _TABLES[key] = hit
    return hit


def resample(wave, orig, new, lengths=None, out_dtype=None, out=None):
    """wave [B, L] (or [L]) float32 or int16 PCM on the device, unit sample stride, any row stride -> [B, ceil(n * L / o)] in
    out_dtype (float32 by default, or bfloat16).  lengths (optional, B ints): samples at or beyond a row's length read as zero
    and outputs at or beyond ceil(n * len / o) are written as zero.  out (optional): a [B, L_out] tensor or view to write into.
    Equal rates return `wave` itself, as torchaudio does."""
    orig, new = int(orig), int(new)
    if orig == new:
        return wave
    o, n, width, _ = _geometry(orig, new)
    _check_supported(orig, new, o, n, width)
    wave, B, L, xs, _, _, squeeze, dev = wavein.as_batch(wave, None, "resample", allow_list=False)
    L_out = output_length(L, o, n)
    out_dtype = out_dtype or (out.dtype if out is not None else torch.float32)
    if out_dtype not in (torch.float32, torch.bfloat16):
        raise TypeError("resample writes float32 or bfloat16, got %s" % out_dtype)
    if out is None:
        out = torch.empty((B, L_out), dtype=out_dtype, device=dev)
    elif (tuple(out.shape) != (B, L_out) or out.dtype != out_dtype or out.device != dev or out.stride(1) != 1
          or (B > 1 and out.stride(0) < L_out)):
        raise ValueError("out must be a [%d, %d] %s tensor on %s with unit sample stride" % (B, L_out, out_dtype, dev))
    len_t = None
    if lengths is not None:            # a tensor or a sequence, as given: the kernel clamps
        len_t = torch.as_tensor(lengths)
        if len_t.numel() != B:
            raise ValueError("lengths must hold %d sample counts" % B)
        len_t = len_t.to(device=dev, dtype=torch.int32).contiguous()
    taps, first, o, n, width = _device_table(orig, new, dev)
    ys = out.stride(0) if B > 1 else L_out
    _lib.check(_lib.lib().wavlm_resample_rows(ops.ptr(wave), wavein.dtype_code(wave), xs, B, L,
                                              ops.ptr(len_t), ops.ptr(taps), ops.ptr(first), o, n, width, ops.ptr(out),
                                              ops.dt(out), ys, ops.stream()), "wavlm_resample_rows")
    return out[0] if squeeze else out


class Resample(nn.Module):
    """torchaudio.transforms.Resample(orig_freq, new_freq): forward(waveform [..., L]) -> [..., ceil(n * L / o)]"""

    def __init__(self, orig_freq=16000, new_freq=16000, resampling_method="sinc_interpolation", lowpass_filter_width=6,
                 rolloff=0.99, beta=None, dtype=None):
        super().__init__()
        if resampling_method not in ("sinc_interpolation", "sinc_interp_hann"):
            raise NotImplementedError("resampling_method=%r: only 'sinc_interpolation' (torchaudio's default; later named "
                                      "'sinc_interp_hann') is built" % (resampling_method,))
        if lowpass_filter_width != 6 or rolloff != 0.99:
            raise NotImplementedError("lowpass_filter_width=%r, rolloff=%r: the device op is built for torchaudio's defaults "
                                      "(6, 0.99)" % (lowpass_filter_width, rolloff))
        self.orig_freq, self.new_freq = int(orig_freq), int(new_freq)
        self.resampling_method, self.lowpass_filter_width, self.rolloff = resampling_method, lowpass_filter_width, rolloff

    def forward(self, waveform):
        if self.orig_freq == self.new_freq:
            return waveform
        lead = waveform.shape[:-1]
        y = resample(waveform.reshape(-1, waveform.shape[-1]), self.orig_freq, self.new_freq)
        return y.view(*lead, y.shape[-1])


def resample_reference(wave, orig, new, table=None):
    """float64 on the CPU: the formula of the module docstring as a dense strided conv1d over all 2 * width + o taps.  wave
    [..., L] of any real dtype (taken as is: scale int16 PCM by 1 / 32768 first).  table (optional): the [n, 2 * width + o]
    filter to use instead of sinc_table's (the tests pass the fp32-rounded one)."""
    wave = torch.as_tensor(wave).detach().cpu().to(torch.float64)
    if int(orig) == int(new):
        return wave
    o, n, width, _ = _geometry(orig, new)
    if table is None:
        table = sinc_table(orig, new)[0]
    kernel = torch.as_tensor(np.asarray(table, dtype=np.float64)).view(n, 1, 2 * width + o)
    lead, L = wave.shape[:-1], wave.shape[-1]
    x = torch.nn.functional.pad(wave.reshape(-1, 1, L), (width, width + o))
    y = torch.nn.functional.conv1d(x, kernel, stride=o)                    # [rows, n, frames]
    y = y.transpose(1, 2).reshape(y.shape[0], -1)[:, :output_length(L, o, n)]
    return y.reshape(*lead, y.shape[-1])
