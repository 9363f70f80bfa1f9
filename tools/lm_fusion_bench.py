"""What does restricting the Transformer LM to the n-best list of an n-gram first pass lose, and what does fusing it cost?
Synthetic emissions, a seeded lexicon, a seeded bigram and a seeded Transformer LM (random weights: the figures say how the two
decoders behave mechanically, nothing about word error rates).  Needs a GPU.

Per utterance a random word sequence is spelt, stretched over frames with repeats and blanks, and turned into emissions by adding
`--boost` to the path's class over N(0, 1) noise.  Two decoders run on the same emissions under one objective (acoustic score +
tlm_weight x Transformer-LM log-prob + word_score x words):
  fused     ctc_lexicon.fused_lexicon_decode: the host search with a NeuralWordLM over TransformerLM.incremental()
  rescored  ctc_lexicon.lexicon_beam_decode on the device with the bigram, --nbest hypotheses, then ctc_lexicon.rescore_nbest
Reported: LM states evaluated and extend() calls per utterance, the seconds per utterance inside the LM (extend + logprob_rows,
synchronised) and in the rest of the fused search, the seconds of the rescored path, how often the two 1-bests are the same word
sequence, and how often the fused 1-best scores higher under the common objective (the rescored one can never score higher than
the true optimum, the fused one is cut by the same beam).

    python tools/lm_fusion_bench.py [--utterances 8 --words 400 --frames 80 --beam 20 --nbest 20 --layers 6 --dim 512 --bf16]
prints one JSON line.
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def build_lexicon(rng, n_words, letters):
    spelt, lines = set(), []
    while len(lines) < n_words:
        w = "".join(rng.choice(letters, size=int(rng.integers(2, 6))))
        if w not in spelt and all(a != b for a, b in zip(w, w[1:])):          # no double letters: the path needs no blank inside
            spelt.add(w)
            lines.append(w)
    return lines


def bigram(rng, words):
    """a seeded bigram in log10: Zipf-like unigrams, eight random successors per word"""
    z = np.log10(1.0 / (np.arange(len(words)) + 10.0))
    z -= np.log10((10.0 ** z).sum() + 0.02)
    e = {("<unk>",): (-4.0, 0.0), ("<s>",): (-99.0, -0.3), ("</s>",): (-2.0, 0.0)}
    for w, l in zip(words, z):
        e[(w,)] = (float(l), -0.3)
    for w in ["<s>"] + words:
        for v in rng.choice(len(words), size=8, replace=False):
            e[(w, words[int(v)])] = (float(-0.5 - 1.5 * rng.random()), 0.0)
    return 2, e


def emissions(rng, d, spelling, T, boost):
    """[T, 1, C] log-probs: the path of `spelling` (token ids, words ending in `|`) stretched to T frames"""
    path = []
    for t in spelling:
        path += [t] * int(rng.integers(1, 3))
        if rng.random() < 0.3:
            path.append(d.bos())
    path = (path + [d.bos()] * T)[:T]
    x = rng.standard_normal((T, 1, len(d)))
    x[np.arange(T), 0, path] += boost
    return torch.log_softmax(torch.from_numpy(x), -1).float()


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--utterances", type=int, default=8)
    p.add_argument("--words", type=int, default=400, help="lexicon and LM vocabulary size")
    p.add_argument("--spoken", type=int, default=6, help="words per utterance")
    p.add_argument("--frames", type=int, default=80)
    p.add_argument("--boost", type=float, default=4.0)
    p.add_argument("--beam", type=int, default=20)
    p.add_argument("--nbest", type=int, default=20)
    p.add_argument("--layers", type=int, default=6)
    p.add_argument("--dim", type=int, default=512)
    p.add_argument("--bf16", action="store_true")
    p.add_argument("--ngram-weight", type=float, default=1.0)
    p.add_argument("--tlm-weight", type=float, default=0.5)
    p.add_argument("--word-score", type=float, default=0.5)
    p.add_argument("--seed", type=int, default=0)
    a = p.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("lm_fusion_bench needs a GPU: nothing is measured without one")
    from unispeech_amd import ctc, ctc_lexicon as X
    from unispeech_amd.ctc_lm import NgramLM
    from unispeech_amd.transformer_lm import TransformerLM

    rng = np.random.default_rng(a.seed)
    letters = [chr(ord("A") + i) for i in range(26)]
    d = ctc.LetterDictionary(["|"] + letters)
    vocab = build_lexicon(rng, a.words, letters)
    words = vocab + [X.UNK]
    spellings = [(i, tuple(d.index(c) for c in w) + (d.index("|"),)) for i, w in enumerate(vocab)]
    order, entries = bigram(rng, vocab)
    lex_ngram = X.Lexicon(words, spellings, d, NgramLM(order, entries, words))
    lm_dict = ctc.LetterDictionary(vocab)
    torch.manual_seed(a.seed)
    tlm = TransformerLM(dict(decoder_embed_dim=a.dim, decoder_ffn_embed_dim=4 * a.dim, decoder_layers=a.layers,
                             decoder_attention_heads=a.dim // 64, max_target_positions=128), len(lm_dict), pad=lm_dict.pad(),
                        eos=lm_dict.eos(), unk=lm_dict.unk())
    with torch.no_grad():
        for prm in tlm.parameters():                                            # seeded weights with some contrast
            if prm.dim() > 1:
                prm.copy_(torch.randn_like(prm) * 2.0 / math.sqrt(prm.shape[-1]))
    tlm = tlm.cuda().to(torch.bfloat16 if a.bf16 else torch.float32)
    scorer = X.NeuralWordLM(tlm, lm_dict, words)
    lex_fused = X.Lexicon(words, spellings, d, scorer)

    lm_time = [0.0]
    store = scorer.store
    for name in ("extend", "logprob_rows"):
        def timed(*args, _f=getattr(store, name), **kw):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = _f(*args, **kw)
            torch.cuda.synchronize()
            lm_time[0] += time.perf_counter() - t0
            return out
        setattr(store, name, timed)

    kw = dict(beam=a.beam, beam_size_token=len(d), beam_threshold=25.0, word_score=a.word_score, sil_weight=0.0, normalized=True)
    res = {k: [] for k in ("states", "calls", "lm_s", "search_s", "rescored_s", "same", "fused_minus_rescored")}
    for u in range(a.utterances + 1):                                           # utterance 0 warms up and is not counted
        spoken = [int(v) for v in rng.integers(0, len(vocab), a.spoken)]
        x = emissions(rng, d, [t for w in spoken for t in spellings[w][1]], a.frames, a.boost)
        stats, lm_time[0] = {}, 0.0
        t0 = time.perf_counter()
        fused = X.fused_lexicon_decode(x, None, d, lex_fused, scorer, lm_weight=a.tlm_weight, nbest=1, stats=stats, **kw)[0]
        t_fused = time.perf_counter() - t0
        t_lm = lm_time[0]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        first = X.lexicon_beam_decode(x.cuda(), None, d, lex_ngram, lex_ngram.lm, lm_weight=a.ngram_weight, nbest=a.nbest, **kw)
        second = X.rescore_nbest(first, tlm, lm_dict, lex_ngram.lm, a.ngram_weight, a.word_score, a.tlm_weight, a.word_score)[0]
        torch.cuda.synchronize()
        t_resc = time.perf_counter() - t0
        if u == 0 or not fused or not second:
            continue
        res["states"].append(stats["states"][0])
        res["calls"].append(stats["calls"][0])
        res["lm_s"].append(t_lm)
        res["search_s"].append(t_fused - t_lm)
        res["rescored_s"].append(t_resc)
        res["same"].append(fused[0][0] == second[0]["words"])
        res["fused_minus_rescored"].append(fused[0][2] - second[0]["score"])
    n = len(res["same"])
    diff = res["fused_minus_rescored"]
    med = lambda v: statistics.median(v) if v else None  # noqa: E731
    print(json.dumps({
        "utterances": n, "frames": a.frames, "lexicon_words": len(vocab), "beam": a.beam, "nbest": a.nbest,
        "lm": {"layers": a.layers, "dim": a.dim, "dtype": "bf16" if a.bf16 else "fp32"},
        "states_per_utterance": {"median": med(res["states"]), "min": min(res["states"], default=None),
                                 "max": max(res["states"], default=None)},
        "extend_calls_per_utterance": med(res["calls"]),
        "fused_lm_seconds_per_utterance": med(res["lm_s"]), "fused_search_seconds_per_utterance": med(res["search_s"]),
        "ngram_plus_rescoring_seconds_per_utterance": med(res["rescored_s"]),
        "same_1best": sum(res["same"]), "fused_better": sum(v > 1e-6 for v in diff), "rescored_better": sum(v < -1e-6 for v in diff),
        "median_objective_gain_of_fused": med(diff)}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
