"""The log-mel front end on one GPU, one process: kernel time, frames / s and the achieved fraction of the derived HBM bound
(160 fp32 samples read and 40 floats written per frame, 800 B, at the 6.3 TB/s a streaming kernel reaches) for a
batch of 64 utterances of 15 s at 16 kHz, fp32 input, and beside it the same transform composed of torch ops on the device
(torch.stft, |.|^2, matmul with the [257, 40] mel matrix, + 1e-6, log), fp32.  Each timed call works on the next of several
buffer sets that together exceed the 256 MiB Infinity Cache; HIP events around the timed loop, after warm-up calls.  Nothing
asserts on these numbers.

    python tools/fbank_bench.py [--reps 50] [--torch-reps 10] [--warmup 3]
Prints one JSON object."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from unispeech_amd.fbank import LOG_ADD, fbank, frames, mel_bank  # noqa: E402

CACHE_BYTES = 256 << 20
STREAM_BPS = 6.3e12
BYTES_PER_FRAME = 160 * 4 + 40 * 4


def timed(fn, reps, warmup):
    for r in range(warmup):
        fn(r)
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for r in range(reps):
        fn(r)
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def torch_fbank(x, window, mel):
    spec = torch.stft(x, 512, 160, 400, window, center=True, pad_mode="reflect", normalized=False, onesided=True,
                      return_complex=True)
    power = spec.real ** 2 + spec.imag ** 2
    return torch.log(power.transpose(1, 2) @ mel + LOG_ADD)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--torch-reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    sr, B, L = 16000, 64, 240000
    T = frames(L)
    window = torch.hann_window(400, device="cuda")
    mel = torch.from_numpy(mel_bank(sr, 512, 40).astype(np.float32)).cuda()
    nbytes = B * (L * 4 + T * 40 * 4)
    sets = CACHE_BYTES // nbytes + 2
    g = torch.Generator(device="cuda").manual_seed(0)
    xs = [(0.1 * torch.randn(B, L, device="cuda", generator=g)).clamp_(-1, 1) for _ in range(sets)]
    keep = [None]

    def run(r):
        keep[0] = fbank(xs[r % sets])

    ms = timed(run, a.reps, a.warmup)
    bound_ms = B * T * BYTES_PER_FRAME / STREAM_BPS * 1e3
    ref = torch_fbank(xs[0], window, mel)
    diff = float((ref - fbank(xs[0])).abs().max())
    del ref
    tms = timed(lambda r: keep.__setitem__(0, torch_fbank(xs[r % sets], window, mel)), a.torch_reps, a.warmup)
    print(json.dumps({"device": torch.cuda.get_device_name(0), "sample_rate": sr, "B": B, "L": L, "frames": B * T,
                      "algorithmic_MB": round(nbytes / 1e6, 2), "buffer_sets": sets, "reps": a.reps, "kernel_ms": round(ms, 4),
                      "frames_per_s": round(B * T / ms * 1e3), "hbm_bound_ms": round(bound_ms, 4),
                      "fraction_of_bound": round(bound_ms / ms, 4), "max_abs_diff_vs_torch": diff, "torch_ms": round(tms, 4),
                      "torch_frames_per_s": round(B * T / tms * 1e3), "speedup": round(tms / ms, 2)}))


if __name__ == "__main__":
    main()
