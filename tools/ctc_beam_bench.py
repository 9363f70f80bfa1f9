"""CTC beam search with an n-gram unit LM at the fine-tuning shape on one GPU, one process: B = 32 utterances of 15 s (T = 749
frames), C = 32 letters, fp32 logits built as tools/ctc_score_bench.py builds them (noise in [-1, 1], +8 on a path of two or
three frames a letter), beam 500, beam_size_token 32, beam_threshold 25, and a synthetic 4-gram over the 28 letter symbols
(every unigram, then each order extends the one below with probability 0.5 / 0.2 / 0.2; log10 scores uniform in (-4, 0)).

Timed on the host clock around calls that end in a copy to the host: ctc.beam_decode of the whole batch on the device
(wavlm_ctc_beam, one launch), and the float64 host reference (ctc.beam_search_reference) on ONE sample of the batch, whose
1-best must be the device's.  Nothing else asserts on these numbers.

    python tools/ctc_beam_bench.py [--reps 5] [--warmup 1] [--rounds 3] [--beam 500] [--beam-threshold 25] [--no-lm]
                                   [--host-only | --device-only]
Prints one JSON object.  --host-only times the reference alone and needs no GPU; --device-only skips it (and its check)."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from unispeech_amd import ctc, ctc_lm  # noqa: E402

B, T, C = 32, 749, 32


def make_lm(d, seed=1):
    rng = np.random.default_rng(seed)
    words = d.symbols[4:] + ["<unk>", "</s>"]
    dens = {2: 0.5, 3: 0.2, 4: 0.2}

    def q():
        return -float(rng.uniform(0.0, 4.0))
    e = {(w,): (q(), q()) for w in words}
    e[("<s>",)] = (-99.0, q())
    prev = [("<s>",)] + [(w,) for w in words if w != "</s>"]
    for k in (2, 3, 4):
        cur = []
        for h in prev:
            for w in words:
                if rng.random() < dens[k]:
                    e[h + (w,)] = (q(), q() if k < 4 else 0.0)
                    if w != "</s>":
                        cur.append(h + (w,))
        prev = cur
    with tempfile.TemporaryDirectory() as tmp:                 # through the file, as a user's LM comes
        path = os.path.join(tmp, "lm.arpa")
        ctc_lm.write_arpa(path, 4, e)
        return ctc_lm.NgramLM.load(path, d), len(e)


def make_batch(seed=0):
    rng = np.random.default_rng(seed)
    d = ctc.LetterDictionary(["|"] + [chr(ord("A") + i) for i in range(26)] + ["'"])
    x = rng.uniform(-1.0, 1.0, (T, B, C)).astype(np.float32)
    for b in range(B):
        n, row = int(rng.integers(230, 271)), []
        while len(row) < n:
            row += [int(v) for v in rng.integers(5, C, rng.integers(1, 8))] + [4]
        path = []
        for v in row[:n]:
            if path and path[-1] == v:
                path.append(0)
            path += [v] * int(rng.integers(2, 4))
        path = (path + [0] * T)[:T]
        x[np.arange(T), b, path] += 8.0
    return d, torch.from_numpy(x)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--beam", type=int, default=500)
    ap.add_argument("--beam-threshold", type=float, default=25.0)
    ap.add_argument("--no-lm", action="store_true")
    ap.add_argument("--host-only", action="store_true")
    ap.add_argument("--device-only", action="store_true")
    a = ap.parse_args()
    d, x = make_batch()
    lm, n_entries = (None, 0) if a.no_lm else make_lm(d)
    kw = {"beam": a.beam, "beam_size_token": 32, "beam_threshold": a.beam_threshold, "lm_weight": 1.0, "sil_weight": 0.0, "nbest": 1}
    out = {"B": B, "T": T, "C": C, "lm_order": 0 if lm is None else 4, "lm_entries": n_entries,
           "lm_nodes": 0 if lm is None else len(lm), **kw}
    host = None
    if not a.device_only:
        t0 = time.perf_counter()
        host = ctc.beam_decode(x[:, :1], None, d, lm, **kw)[0][0]
        out["host_reference_one_sample_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    if not a.host_only:
        if not torch.cuda.is_available():
            raise SystemExit("tools/ctc_beam_bench.py needs a GPU (or --host-only)")
        logits = x.transpose(0, 1).contiguous().cuda().transpose(0, 1)      # T x B x C view of batch-first storage
        res = {}

        def run():
            res["hyps"] = ctc.beam_decode(logits, None, d, lm, **kw)
        times = []
        for _ in range(a.rounds):
            for _ in range(a.warmup):
                run()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.reps):
                run()
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3 / a.reps)
        dev = res["hyps"][0][0]
        ms = float(np.median(times))
        out.update(device=torch.cuda.get_device_name(0), device_batch_ms=round(ms, 3), all_rounds=[round(t, 3) for t in times],
                   device_score=dev[1], reps=a.reps, rounds=a.rounds)
        if host is not None:
            assert dev[0] == host[0], (dev, host)
            out.update(host_score=host[1], host_one_sample_over_device_batch=round(out["host_reference_one_sample_ms"] / ms, 1),
                       host_batch_over_device_batch=round(out["host_reference_one_sample_ms"] * B / ms, 1))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
