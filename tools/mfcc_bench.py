"""The MFCC front end on one GPU, one process: kernel time, frames / s and the achieved fraction of the derived HBM bound
(every sample read once, 39 fp32 written per frame, at the 6.3 TB/s a streaming kernel reaches) for a corpus-like
batch (64 utterances of 15 s at 16 kHz), fp32 and int16 input, and beside it the same transform composed of torch ops on the
device (unfold, rfft, two matmuls, replicate-padded deltas), fp32.  Each timed call works on the next of several buffer sets
that together exceed the 256 MiB Infinity Cache.  Nothing asserts on these numbers.

    python tools/mfcc_bench.py [--reps 50] [--torch-reps 5]
Prints one JSON object."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from unispeech_amd.mfcc import EPS32, mel_filters, mfcc, num_frames, tables  # noqa: E402

CACHE_BYTES = 256 << 20
STREAM_BPS = 6.3e12


def timed(fn, reps):
    fn(0)
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for r in range(reps):
        fn(r)
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def torch_deltas(c):
    p = torch.nn.functional.pad(c.transpose(1, 2), (2, 2), mode="replicate")
    m = c.shape[1]
    d = (-2 * p[..., 0:m] - p[..., 1:m + 1] + p[..., 3:m + 3] + 2 * p[..., 4:m + 4]) / 10
    return d.transpose(1, 2)


def torch_mfcc(x, t):
    fr = x.unfold(1, t["W"], t["S"])
    fr = fr - fr.mean(-1, keepdim=True)
    fr = (fr - 0.97 * torch.cat([fr[..., :1], fr[..., :-1]], -1)) * t["window"]
    power = torch.fft.rfft(fr, n=t["P"]).abs().pow(2)
    c = torch.log(torch.clamp(power @ t["mel"], min=EPS32)) @ t["dct"]
    d = torch_deltas(c)
    return torch.cat([c, d, torch_deltas(d)], -1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--torch-reps", type=int, default=5)
    a = ap.parse_args()
    sr, B, L = 16000, 64, 240000
    tb = tables(sr)
    f32 = lambda v: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).cuda()
    tt = dict(W=tb["W"], S=tb["S"], P=tb["P"], window=f32(tb["window"]), mel=f32(mel_filters(sr).T), dct=f32(tb["dct"].T))
    M = num_frames(L, sr)
    out = {"device": torch.cuda.get_device_name(0), "sample_rate": sr, "B": B, "L": L, "frames": B * M, "cases": []}
    g = torch.Generator(device="cuda").manual_seed(0)
    for in_dtype in (torch.float32, torch.int16):
        nbytes = B * (L * torch.empty(0, dtype=in_dtype).element_size() + M * 39 * 4)
        sets = CACHE_BYTES // nbytes + 2
        xs = []
        for _ in range(sets):
            x = (0.1 * torch.randn(B, L, device="cuda", generator=g)).clamp_(-1, 1)
            xs.append((x * 32767).round().to(torch.int16) if in_dtype == torch.int16 else x)
        keep = [None]

        def run(r):
            keep[0] = mfcc(xs[r % sets], sr)[0]

        ms = timed(run, a.reps)
        bound_ms = nbytes / STREAM_BPS * 1e3
        rec = {"in": str(in_dtype)[6:], "algorithmic_MB": round(nbytes / 1e6, 2), "buffer_sets": sets, "kernel_ms": round(ms, 4),
               "frames_per_s": round(B * M / ms * 1e3), "hbm_bound_ms": round(bound_ms, 4),
               "fraction_of_bound": round(bound_ms / ms, 4)}
        if in_dtype == torch.float32:
            ref = torch_mfcc(xs[0], tt)
            rec["max_abs_diff_vs_torch"] = float((ref - mfcc(xs[0], sr)[0]).abs().max())
            del ref
            tms = timed(lambda r: torch_mfcc(xs[r % sets], tt), a.torch_reps)
            rec.update(torch_ms=round(tms, 4), torch_frames_per_s=round(B * M / tms * 1e3), speedup=round(tms / ms, 2))
        out["cases"].append(rec)
        del xs
    print(json.dumps(out))


if __name__ == "__main__":
    main()
