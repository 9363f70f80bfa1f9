"""The sinc resampler on one GPU, one process: kernel time and achieved GB/s against the algorithmic bytes (every input sample
read once, every output sample written once) for one 30 s chunk batch of a diarization recording (20 x 240000 samples, 8 kHz
-> 16 kHz) and for 20 x 30 s of 44.1 kHz audio -> 16 kHz, and the same op written with torch on the device (zero padding,
F.conv1d with the dense [n, 1, 2 * width + o] filter and stride o, transpose, cut), fp32.

Each timed call works on the next of several buffer sets whose total exceeds the 256 MiB Infinity Cache, so neither side reads
its input from a cache the previous call filled.

    python tools/resample_bench.py [--reps 50] [--torch-reps 5]
Prints one JSON object."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from unispeech_amd.resample import output_length, resample, sinc_table  # noqa: E402

CACHE_BYTES = 256 << 20


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


def torch_resample(x, kernel, width, o, n, L_out):
    y = torch.nn.functional.conv1d(torch.nn.functional.pad(x[:, None], (width, width + o)), kernel, stride=o)
    return y.transpose(1, 2).reshape(x.shape[0], -1)[:, :L_out]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--torch-reps", type=int, default=5)
    a = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0), "cases": []}
    g = torch.Generator(device="cuda").manual_seed(0)
    for orig, new, B, L in ((8000, 16000, 20, 240000), (44100, 16000, 20, 1323000)):
        table, width, o, n = sinc_table(orig, new)
        L_out = output_length(L, o, n)
        kernel = torch.from_numpy(table.astype(np.float32)).cuda().view(n, 1, -1)
        for in_dtype, out_dtype in ((torch.float32, torch.float32), (torch.int16, torch.bfloat16)):
            nbytes = B * (L * torch.empty(0, dtype=in_dtype).element_size() + L_out * torch.empty(0, dtype=out_dtype).element_size())
            sets = CACHE_BYTES // nbytes + 2
            xs = []
            for _ in range(sets):
                x = torch.randn(B, L, device="cuda", generator=g).clamp_(-1, 1)
                xs.append((x * 32767).round().to(torch.int16) if in_dtype == torch.int16 else x)
            ys = [torch.empty(B, L_out, dtype=out_dtype, device="cuda") for _ in range(sets)]
            ms = timed(lambda r: resample(xs[r % sets], orig, new, out=ys[r % sets]), a.reps)
            rec = {"orig": orig, "new": new, "B": B, "L": L, "L_out": L_out, "in": str(in_dtype)[6:], "out": str(out_dtype)[6:],
                   "taps_per_output": 2 * width + 1, "algorithmic_MB": round(nbytes / 1e6, 2), "buffer_sets": sets,
                   "kernel_ms": round(ms, 4), "GBps": round(nbytes / ms / 1e6, 1)}
            if in_dtype == torch.float32:
                ref = torch_resample(xs[0], kernel, width, o, n, L_out)
                rec["max_abs_diff_vs_torch"] = float((ref - ys[0]).abs().max())   # ys[0]: the warm-up call
                del ref
                tms = timed(lambda r: torch_resample(xs[r % sets], kernel, width, o, n, L_out), a.torch_reps)
                rec.update(torch_conv1d_ms=round(tms, 4), torch_conv1d_GBps=round(nbytes / tms / 1e6, 1),
                           speedup=round(tms / ms, 2))
            out["cases"].append(rec)
            del xs, ys
    print(json.dumps(out))


if __name__ == "__main__":
    main()
