"""The host side of the waveform input layer (csrc/wave_input.hpp) that `resample`, `mfcc` and `fbank` share: the batch
normalisation of their first argument, and the tables the two spectral front ends build the same way."""
import math

import numpy as np
import torch

from . import _lib
from . import ops

I16 = _lib.I16   # csrc/common.hpp WL_I16: input dtype code of 16-bit PCM


def dtype_code(wave):
    return I16 if wave.dtype == torch.int16 else _lib.F32


def as_batch(wavs, lengths, op, allow_list=True):
    """wavs: [B, L] or [L] float32 / int16 PCM on the device -- or, with allow_list, a list of 1-D device tensors of unequal
    length (one dtype), padded into one batch that carries its own lengths.  lengths: None, or B sample counts (tensor or
    sequence), clamped to [0, L].  `op` names the caller in the messages.
    -> (wave [B, L] with unit sample stride and rows that do not overlap, B, L, the row stride to hand the kernel, the clamped
    lengths as a list ([L] * B without), the same as an int32 device tensor (None without), whether the input was 1-D, device)"""
    squeeze = False
    if allow_list and isinstance(wavs, (list, tuple)):
        if lengths is not None:
            raise ValueError("%s: a list of waveforms carries its own lengths" % op)
        if not wavs:
            raise ValueError("%s: an empty list of waveforms" % op)
        dev = ops._dev(wavs[0])
        if any(w.dim() != 1 or w.dtype != wavs[0].dtype or w.device != dev for w in wavs):
            raise ValueError("%s: a list takes 1-D tensors of one dtype on one device" % op)
        lengths = [int(w.numel()) for w in wavs]
        wave = torch.zeros((len(wavs), max(max(lengths), 1)), dtype=wavs[0].dtype, device=dev)
        for r, w in enumerate(wavs):
            wave[r, :lengths[r]] = w
    else:
        wave = wavs
        dev = ops._dev(wave)
        squeeze = wave.dim() == 1
        if squeeze:
            wave = wave.unsqueeze(0)
    if wave.dtype not in (torch.float32, torch.int16):
        raise TypeError("%s takes float32 or int16 PCM, got %s" % (op, wave.dtype))
    if wave.dim() != 2 or wave.shape[0] < 1 or wave.shape[1] < 1:
        raise ValueError("%s takes [B, L] with B, L >= 1, got %s" % (op, tuple(wave.shape)))
    B, L = wave.shape
    if wave.stride(1) != 1 or (B > 1 and wave.stride(0) < L):
        wave = wave.contiguous()
    len_l, len_t = [L] * B, None
    if lengths is not None:
        len_l = [int(v) for v in (lengths.tolist() if isinstance(lengths, torch.Tensor) else lengths)]
        if len(len_l) != B:
            raise ValueError("lengths must hold %d sample counts" % B)
        len_l = [min(max(v, 0), L) for v in len_l]
        len_t = torch.tensor(len_l, dtype=torch.int32).to(dev)
    return wave, B, L, (wave.stride(0) if B > 1 else L), len_l, len_t, squeeze, dev


def twiddle(P):
    """float64 [P, 2] = (cos, -sin)(2 pi t / P)"""
    t = np.arange(P, dtype=np.float64) * (2.0 * math.pi / P)
    return np.stack([np.cos(t), -np.sin(t)], axis=1)


def pack_filters(bank):
    """dense float64 [filters, bins] -> (mel_idx int32 [filters, 3] = (first bin, count, offset into mel_w), mel_w float64
    [sum of counts]): filter f is sum_i mel_w[offset + i] * power[first + i], from its first to its last non-zero bin (an empty
    filter: count 0; no non-zero weight at all: an empty mel_w)"""
    idx, ws, off = [], [np.zeros(0)], 0
    for row in bank:
        nz = np.nonzero(row)[0]
        first, count = (int(nz[0]), int(nz[-1] - nz[0] + 1)) if len(nz) else (0, 0)
        idx.append((first, count, off))
        ws.append(row[first:first + count])
        off += count
    return np.asarray(idx, dtype=np.int32).reshape(len(bank), 3), np.concatenate(ws)


def upload(a, device):
    """a float array rounded to fp32 (once), an integer one as int32, on the device"""
    a = np.asarray(a)
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32 if a.dtype.kind in "iu" else np.float32)).to(device)
