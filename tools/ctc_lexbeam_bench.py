"""Lexicon-constrained CTC beam search with a word n-gram LM at the fine-tuning shape on one GPU, one process: B = 32 utterances
of 15 s (T = 749 frames), C = 32 letters, fp32 logits built as tools/ctc_beam_bench.py builds them (noise in [-1, 1], +8 on a
path of two or three frames a letter) but over sentences of the lexicon's words; a synthetic lexicon of about 20 000 words of two
to eight of the 27 letters, every spelling terminated by `|`; a synthetic 3-gram over those words (every unigram, 40 000 bigrams,
20 000 trigrams that extend them; log10 scores uniform in (-4, 0)); beam_size_token 32, beam_threshold 25, lm_weight 1,
word_score 1, no <unk> words.

Timed on the host clock around calls that end in a copy to the host, the medians as tools/ctc_beam_bench.py takes them, at beam
100 and at the largest beam wavlm_ctc_lexbeam_supported admits for this lexicon: ctc_lexicon.lexicon_beam_decode of the whole batch
on the device (wavlm_ctc_lexbeam, one launch); next to it ctc.beam_decode (wavlm_ctc_beam, the lexicon-free kernel with that
tool's 4-gram unit LM) at the same beams; and the float64 host reference on ONE sample at beam 100, whose 1-best words must be the
device's.  Nothing else asserts on these numbers.

    python tools/ctc_lexbeam_bench.py [--reps 5] [--warmup 1] [--rounds 3] [--words 20000] [--beam N ...]
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from unispeech_amd import ctc, ctc_lexicon, ctc_lm, ops  # noqa: E402
import ctc_beam_bench as U  # noqa: E402

B, T, C = U.B, U.T, U.C


def make_lexicon(d, n_words, seed=2):
    """(Lexicon with its word 3-gram, the word spellings as token ids, the number of LM entries), through files as a user's come"""
    rng = np.random.default_rng(seed)
    letters = d.symbols[5:]
    vocab = sorted(set("".join(letters[int(v)] for v in rng.integers(0, len(letters), int(rng.integers(2, 9))))
                       for _ in range(n_words)))

    def q():
        return -float(rng.uniform(0.0, 4.0))
    e = {(w,): (q(), q()) for w in vocab + ["<unk>", "</s>"]}
    e[("<s>",)] = (-99.0, q())
    heads = vocab + ["<s>"]
    bigrams = []
    for _ in range(2 * n_words):
        g = (heads[int(rng.integers(len(heads)))], vocab[int(rng.integers(len(vocab)))])
        if g not in e:
            e[g] = (q(), q())
            bigrams.append(g)
    for _ in range(n_words):
        g = bigrams[int(rng.integers(len(bigrams)))] + (vocab[int(rng.integers(len(vocab)))],)
        e.setdefault(g, (q(), 0.0))
    with tempfile.TemporaryDirectory() as tmp:
        lex, arpa = os.path.join(tmp, "lexicon.txt"), os.path.join(tmp, "lm.arpa")
        with open(lex, "w", encoding="utf-8") as f:
            f.write("".join("%s %s |\n" % (w, " ".join(w)) for w in vocab))
        ctc_lm.write_arpa(arpa, 3, e)
        lexicon = ctc_lexicon.Lexicon.load(lex, d, arpa)
    return lexicon, [[d.index(ch) for ch in w] + [4] for w in vocab], len(e)


def make_batch(d, spellings, seed=0):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1.0, 1.0, (T, B, C)).astype(np.float32)
    for b in range(B):
        n, row = int(rng.integers(230, 271)), []
        while True:
            w = spellings[int(rng.integers(len(spellings)))]
            if len(row) + len(w) > n:
                break
            row += w
        path = []
        for v in row:
            if path and path[-1] == v:
                path.append(0)
            path += [v] * int(rng.integers(2, 4))
        path = (path + [0] * T)[:T]
        x[np.arange(T), b, path] += 8.0
    return torch.from_numpy(x)


def timed(run, a):
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
    return round(float(np.median(times)), 3), [round(t, 3) for t in times]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--words", type=int, default=20000)
    ap.add_argument("--beam", type=int, action="append", help="a beam to measure (repeatable; default: 100 and the largest)")
    ap.add_argument("--host-only", action="store_true")
    ap.add_argument("--device-only", action="store_true")
    a = ap.parse_args()
    d = ctc.LetterDictionary(["|"] + [chr(ord("A") + i) for i in range(26)] + ["'"])
    lexicon, spellings, n_entries = make_lexicon(d, a.words)
    x = make_batch(d, spellings)
    width = lexicon.width(32, False)
    beams = a.beam or [100, ops.ctc_lexbeam_max_beam(C, width, 3, len(lexicon))]
    kw = {"beam_size_token": 32, "beam_threshold": 25.0, "lm_weight": 1.0, "word_score": 1.0, "sil_weight": 0.0, "nbest": 1}
    out = {"B": B, "T": T, "C": C, "words": len(lexicon.words), "trie_nodes": len(lexicon), "width": width, "lm_order": 3,
           "lm_entries": n_entries, "lm_nodes": len(lexicon.lm), "beams": beams, **kw}
    host = None
    if not a.device_only:
        t0 = time.perf_counter()
        host = ctc_lexicon.lexicon_beam_decode(x[:, :1], None, d, lexicon, lexicon.lm, beam=100, **kw)[0][0]
        out["host_reference_one_sample_beam100_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    if not a.host_only:
        if not torch.cuda.is_available():
            raise SystemExit("tools/ctc_lexbeam_bench.py needs a GPU (or --host-only)")
        logits = x.transpose(0, 1).contiguous().cuda().transpose(0, 1)      # T x B x C view of batch-first storage
        unit_lm, _ = U.make_lm(d)
        ukw = {k: v for k, v in kw.items() if k != "word_score"}
        out["device"] = torch.cuda.get_device_name(0)
        for beam in beams:
            res = {}

            def run():
                res["hyps"] = ctc_lexicon.lexicon_beam_decode(logits, None, d, lexicon, lexicon.lm, beam=beam, **kw)
            ms, rounds = timed(run, a)
            free_ms, free_rounds = timed(lambda: ctc.beam_decode(logits, None, d, unit_lm, beam=beam, **ukw), a)
            dev = res["hyps"][0][0]
            out["beam_%d" % beam] = {"lexicon_batch_ms": ms, "lexicon_rounds": rounds, "lexicon_free_batch_ms": free_ms,
                                     "lexicon_free_rounds": free_rounds, "lexicon_over_lexicon_free": round(ms / free_ms, 2),
                                     "candidate_capacity": beam * width, "lexicon_free_candidates": beam * 32,
                                     "device_score": dev[2], "device_words": len(dev[0])}
            if host is not None and beam == 100:
                assert dev[0] == host[0], (dev, host)
                out["beam_100"]["host_score"] = host[2]
                out["host_one_sample_over_device_batch"] = round(out["host_reference_one_sample_beam100_ms"] / ms, 1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
