"""Shared inputs of tests/test_ctc_beam.py and tests/test_ctc_beam_gpu.py: small random n-gram LMs, written as ARPA text to a
temporary directory and read back through the parser, and emissions for which device and reference must agree bit for bit.

The exact cases.  Emissions, LM scores and backoffs are multiples of 2^-6 (emissions in [-10, 0], LM values in (-4, 0]), the
weights are in {0.25, 0.5, 1, 2}, T <= 300 and normalized=True: every partial score is a multiple of 2^-8 below 2^15, exact in
fp32 in any order of summation -- so the device's tokens, counts, n_hyp AND scores must equal the float64 reference's, ==.  Ties
occur in such data; the decoder's total order decides them.  The bf16 case draws multiples of 2^-3 in [-8, 0].

The dictionary of a case with C classes: <s> = 0 (the blank), <pad> = 1, </s> = 2, <unk> = 3, `|` = 4 (the silence token), then
w5 .. w(C-1).  The LM lists `|` and every second w symbol: the others, <pad> and <unk> take <unk>'s row.

The normalized=False case is built like tests/ctc_score_cases.py's batches (noise in [-1, 1], +8 on a path) with a bigram LM;
`inexact()` asserts, on the CPU, that the reference's margin is at least 64 x tol, tol = (T + 8) * 2^-23 * abs_sum."""
import functools
import math
import os
import tempfile

import numpy as np
import torch

BLANK, PAD, EOS, UNK, BAR = 0, 1, 2, 3, 4
INF = math.inf
_TMP = tempfile.TemporaryDirectory(prefix="ctc_beam_lm_")


def dictionary(C):
    from unispeech_amd.ctc import LetterDictionary
    return LetterDictionary(["|"] + ["w%d" % i for i in range(5, C)])


def _q(rng):
    return -int(rng.integers(1, 200)) / 64.0


def random_entries(seed, words, order, dens=0.5):
    """{tuple of words: (log10 p, backoff)}: every unigram, then each higher order extends the one below it with probability
    `dens` per word -- prefix-closed as ARPA files are, NOT suffix-closed: (a, b, c) may be there without (b, c)"""
    rng = np.random.default_rng(seed)
    toks = list(words) + ["<unk>", "</s>"]
    e = {(w,): (_q(rng), _q(rng) if order > 1 else 0.0) for w in toks}
    e[("<s>",)] = (0.0, _q(rng) if order > 1 else 0.0)
    prev = [("<s>",)] + [(w,) for w in toks if w != "</s>"]
    for k in range(2, order + 1):
        cur = []
        for h in prev:
            for w in toks:
                if rng.random() < dens:
                    e[h + (w,)] = (_q(rng), _q(rng) if k < order else 0.0)
                    if w != "</s>":
                        cur.append(h + (w,))
        prev = cur
    return e


def katz(entries, order, hist, w):
    """log10 p(w | hist) from the definition, on the full history"""
    h = tuple(hist)[-(order - 1):] if order > 1 else ()
    acc = 0.0
    while h + (w,) not in entries:
        acc += entries[h][1] if h in entries else 0.0
        h = h[1:]
    return acc + entries[h + (w,)][0]


@functools.lru_cache(maxsize=None)
def lm_of(C, order, seed, dens=0.5, every=2):
    """(NgramLM read from a file written here, its entries, the path); the LM lists `|` and every `every`-th w symbol"""
    from unispeech_amd import ctc_lm
    words = ["|"] + ["w%d" % i for i in range(5, C, every)]
    entries = random_entries(seed, words, order, dens)
    path = os.path.join(_TMP.name, "lm_%d_%d_%d_%d.arpa" % (C, order, seed, every))
    ctc_lm.write_arpa(path, order, entries)
    return ctc_lm.NgramLM.load(path, dictionary(C)), entries, path


def emissions(seed, T, B, C, step=64, lo=-10):
    rng = np.random.default_rng(seed)
    return torch.from_numpy(rng.integers(lo * step, 1, (T, B, C)) / float(step)).float()


# name: T, B, C, LM order (0: none), beam, beam_size_token, threshold, lm_weight, sil_weight, nbest, input lengths (None: all T)
CASES = {
    "beam1_T257": (257, 3, 8, 2, 1, 8, INF, 1.0, 0.0, 1, None),
    "beam2_ktok1": (2, 4, 8, 3, 2, 1, INF, 0.5, 0.0, 2, None),
    "beam2_T257": (257, 2, 6, 3, 2, 6, 2.5, 0.25, -0.5, 2, [257, 256]),
    "T1": (1, 3, 8, 2, 5, 8, INF, 2.0, 0.0, 3, None),
    "lengths": (9, 5, 8, 3, 6, 7, INF, 1.0, 0.25, 3, [0, 8, 9, 1, 0]),
    "beam63": (12, 2, 12, 3, 63, 11, INF, 1.0, 0.0, 3, None),
    "beam64": (12, 2, 12, 3, 64, 12, INF, 0.5, -0.5, 1, None),
    "cut": (12, 3, 12, 3, 16, 12, 2.5, 0.5, -0.5, 3, None),
    "beam65_order5": (10, 2, 9, 5, 65, 14, INF, 0.25, 0.5, 65, None),
    "thr0": (20, 3, 8, 2, 8, 8, 0.0, 1.0, 0.0, 8, None),
    "order1": (15, 2, 10, 1, 16, 9, 2.5, 2.0, 0.0, 3, None),
    "nolm": (30, 3, 10, 0, 7, 10, 2.5, 0.0, -0.25, 3, [30, 29, 0]),
    "beam512": (5, 2, 32, 4, 512, 32, INF, 0.5, 0.0, 3, None),
    "C1024": (5, 2, 1024, 2, 8, 16, INF, 1.0, 0.0, 3, None),
}
FLAT = "capacity"                      # flat emissions, beam 512 x 32 classes, threshold infinity, T = 3: every candidate ties
ALL = list(CASES) + [FLAT]


@functools.lru_cache(maxsize=None)
def case(name):
    """(emissions fp32 [T, B, C], input lengths, dictionary, lm or None, keyword options) -- treat as read-only"""
    if name == FLAT:
        T, B, C, order, beam, ktok, thr, lmw, silw, nbest, il = 3, 1, 32, 3, 512, 32, INF, 1.0, 0.0, 3, None
        x = torch.full((T, B, C), -1.0)
    else:
        T, B, C, order, beam, ktok, thr, lmw, silw, nbest, il = CASES[name]
        x = emissions(sorted(ALL).index(name), T, B, C)
    il = [T] * B if il is None else il
    if name == FLAT:                   # every symbol has a word and most bigrams are entries: 512 distinct (state, token) by frame 2
        lm = lm_of(C, order, 7 + order, 0.9, 1)[0]
    else:
        lm = lm_of(C, order, 7 + order, 0.5 if C <= 32 else 0.05)[0] if order else None
    opts = {"beam": beam, "beam_size_token": ktok, "beam_threshold": thr, "lm_weight": lmw, "sil_weight": silw, "nbest": nbest}
    return x, il, dictionary(C), lm, opts


@functools.lru_cache(maxsize=None)
def reference(name, bf16=False):
    """beam_decode of the case on the host (the float64 reference), once per process"""
    from unispeech_amd.ctc import beam_decode
    x, il, d, lm, opts = case(name)
    if bf16:
        x = bf16_emissions(name)
    return beam_decode(x, il, d, lm, normalized=True, **opts)


@functools.lru_cache(maxsize=None)
def bf16_emissions(name):
    x, _, _, _, _ = case(name)
    T, B, C = x.shape
    return emissions(99, T, B, C, step=8, lo=-8)


# ------------------------------------------------------------------------------------------------------ normalized=False
INEXACT_OPTS = {"beam": 4, "beam_size_token": 6, "beam_threshold": INF, "lm_weight": 0.5, "sil_weight": 0.0, "nbest": 2}
INEXACT_SEED = 0


@functools.lru_cache(maxsize=None)
def inexact():
    """(logits [T, B, 32], input lengths, dictionary, bigram lm, reference hyps, tol per sample): raw logits, noise in [-1, 1]
    with +8 on a path.  Asserts that every decision of the reference was taken by at least 64 x tol."""
    import ctc_score_cases as S
    from unispeech_amd import ctc
    T, C = 12, S.C
    hyps = [S.ids("AB|CD"), S.ids("A"), [], S.ids("HELLO|YOU"), S.ids("AAB")]
    il = [T, T, T - 1, T, T]
    logits = S.logits_for(hyps, T, il, 1000 + INEXACT_SEED)
    d = dictionary(C)
    lm = lm_of(C, 2, 21, 0.3)[0]
    ref, margin, abs_sum = ctc.beam_search_reference(logits, il, BLANK, ctc.silence_token(d), lm, normalized=False, **INEXACT_OPTS)
    tol = [(T + 8) * 2.0 ** -23 * a for a in abs_sum]
    for b in range(len(il)):
        assert margin[b] >= 64 * tol[b], (b, margin[b], tol[b])
    return logits, il, d, lm, ref, tol
