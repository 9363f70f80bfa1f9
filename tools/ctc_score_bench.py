"""CTC validation scoring at the fine-tuning shape on one GPU, one process: B = 32 utterances of 15 s (T = 749 frames), C = 32
letters, targets of 230 .. 270 letters in words of 1 .. 7, fp32 logits whose greedy decode is the target with about one token in
ten substituted, dropped or doubled.  Timed, on the host clock around calls that end in a copy to the host (so the device work is
inside): one eval-mode CtcCriterion.get_loss -- the loss launches, then the error counts -- and error_counts alone, each on the
device path (wavlm_ctc_score) and under WAVLM_CTC_SCORE_HOST=1 (greedy_decode + the pure-Python edit distance per sample),
alternating, after warm-up calls.  Both paths must give the same logging output; nothing else asserts on these numbers.

The device path is timed over --device-reps calls a round and the host path over --reps: a call of the one takes milliseconds, of
the other a fifth of a second, and both windows should be long against the clock.

    python tools/ctc_score_bench.py [--reps 5] [--device-reps 100] [--warmup 2] [--rounds 3]
Prints one JSON object."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from unispeech_amd import ctc  # noqa: E402

B, T, C = 32, 749, 32


def make_batch(seed=0):
    rng = np.random.default_rng(seed)
    d = ctc.LetterDictionary(["|"] + [chr(ord("A") + i) for i in range(26)] + ["'"])
    rows, x = [], rng.uniform(-1.0, 1.0, (T, B, C)).astype(np.float32)
    for b in range(B):
        n, row = int(rng.integers(230, 271)), []
        while len(row) < n:
            row += [int(v) for v in rng.integers(5, C, rng.integers(1, 8))] + [4]
        row = row[:n]
        rows.append(row)
        path = []
        for v in row:                                       # two or three frames a token, a blank between equal neighbours
            r = rng.random()
            if r < 0.04:
                continue
            v = int(rng.integers(4, C)) if r < 0.08 else v
            if path and path[-1] == v:
                path.append(0)
            path += [v] * int(rng.integers(2, 4))
        path = (path + [0] * T)[:T]
        x[np.arange(T), b, path] += 8.0
    Lt = max(len(r) for r in rows) + 1
    target = torch.full((B, Lt), d.pad(), dtype=torch.long)
    for b, r in enumerate(rows):
        target[b, :len(r)] = torch.tensor(r)
        target[b, len(r)] = d.eos()
    return d, torch.from_numpy(x), target


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--device-reps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/ctc_score_bench.py needs a GPU")
    d, x, target = make_batch()
    logits = x.transpose(0, 1).contiguous().cuda().transpose(0, 1)          # T x B x C view of batch-first storage
    crit = ctc.CtcCriterion(d, zero_infinity=True)
    model = torch.nn.Module().eval()
    sample = {"id": torch.arange(B), "target": target.cuda(), "net_input": {}}
    net = {"encoder_out": logits, "padding_mask": None}
    il = torch.full((B,), T, dtype=torch.long)
    classes = crit._classes(C, logits.device)
    assert classes is not None
    out = {}

    def get_loss():
        with torch.no_grad():
            out["log"] = crit.get_loss(model, sample, net)[2]

    def counts():
        out["counts"] = ctc.error_counts(logits, il, sample["target"], d, "letter", 0, classes=classes)

    def with_switch(fn, host):
        def run():
            if host:
                os.environ["WAVLM_CTC_SCORE_HOST"] = "1"
            else:
                os.environ.pop("WAVLM_CTC_SCORE_HOST", None)
            fn()
        return run

    with_switch(get_loss, False)()
    dev_log = dict(out["log"])
    with_switch(get_loss, True)()
    assert out["log"] == dev_log, (out["log"], dev_log)
    res = {k: [] for k in ("get_loss_device_ms", "get_loss_host_ms", "error_counts_device_ms", "error_counts_host_ms")}
    for _ in range(a.rounds):                                               # alternate: the machine is shared
        res["get_loss_device_ms"].append(timed(with_switch(get_loss, False), a.device_reps, a.warmup))
        res["get_loss_host_ms"].append(timed(with_switch(get_loss, True), a.reps, a.warmup))
        res["error_counts_device_ms"].append(timed(with_switch(counts, False), a.device_reps, a.warmup))
        res["error_counts_host_ms"].append(timed(with_switch(counts, True), a.reps, a.warmup))
    os.environ.pop("WAVLM_CTC_SCORE_HOST", None)
    med = {k: round(float(np.median(v)), 4) for k, v in res.items()}
    print(json.dumps(dict({"device": torch.cuda.get_device_name(0), "B": B, "T": T, "C": C, "Lt": int(target.shape[1]),
                           "reps": a.reps, "device_reps": a.device_reps, "rounds": a.rounds,
                           "log": {k: dev_log[k] for k in ("c_errors", "c_total", "w_errors", "w_total")}},
                          **med, all_rounds={k: [round(t, 4) for t in v] for k, v in res.items()},
                          get_loss_host_over_device=round(med["get_loss_host_ms"] / med["get_loss_device_ms"], 2),
                          error_counts_host_over_device=round(med["error_counts_host_ms"] / med["error_counts_device_ms"], 2))))


if __name__ == "__main__":
    main()
