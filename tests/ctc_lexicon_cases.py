"""Shared inputs of tests/test_ctc_lexicon.py and tests/test_ctc_lexicon_gpu.py: small lexicons, written to a temporary directory
and read back through ctc_lexicon.read_lexicon, random word n-gram LMs (the generator and the ARPA writer of ctc_beam_cases), and
emissions for which device and reference must agree bit for bit.

The exact cases.  Emissions, LM scores and backoffs are multiples of 2^-6 (emissions in [-10, 0], LM values in (-3.125, 0]), the
weights are in {0.25, 0.5, 1, 2}, word_score / unk_weight are multiples of 0.25, T <= 300 and normalized=True.  Every term of a
score -- an emission, sil_weight, lm_weight * (max(c) - lexmax(node)), lm_weight * (lm(state, w) - lexmax(node)), word_score -- is
then a multiple of 2^-8, and a partial score is bounded by
    T * (10 + |sil_weight| + lm_weight * 3.125 * order + max(|word_score|, |unk_weight|)) + 2 * lm_weight * 3.125 * order
(|lm(state, w)| <= 3.125 * order: one log p and at most order - 1 backoffs; the smearing terms telescope, so at most one word's
worth of them is outstanding).  case() asserts that this is below 2^15: every partial score is then exact in fp32 in any order of
summation, and the device's words, tokens, counts, n_hyp AND scores must equal the float64 reference's, ==.

The dictionary of a case with C classes is ctc_beam_cases.dictionary(C): `|` = 4 is the silence token, w5 .. w(C-1) the letters.
The LM of a case lists every second word of its lexicon; the others take <unk>'s row.

The normalized=False case is built like ctc_beam_cases.inexact() over the letters of ctc_score_cases; `inexact()` asserts, on the
CPU, that the reference's margin is at least 64 x tol, tol = (T + 8) * 2^-23 * abs_sum."""
import functools
import math
import os
import tempfile

import numpy as np
import torch

import ctc_beam_cases as K

BLANK, BAR = K.BLANK, K.BAR
INF = math.inf
CAP = 16384                            # wavlm_ctc_lexbeam_supported: beam x width <= CAP
LDS_CAP = 8192                         # up to here the kernel keeps a candidate's state and node in LDS, above in its workspace
_TMP = tempfile.TemporaryDirectory(prefix="ctc_lexicon_")

# a one-token word (also spelt with a `|`), three words with one spelling, two with another, a word that is a prefix of another, a
# double letter, `|` inside a spelling, terminated and unterminated spellings, an exact duplicate line
SMALL = """a w5
ab w5 w6 |
ab2 w5 w6 |
ab3 w5 w6 |
cc w7 w7
c|a w7 | w5
b w6 |
b2 w6 |
oov w6 w6 |
b w6 |
a w5 |
abc w5 w6 w7
"""
DEEP = "abc w5 w6 w7 |\n"              # nothing ends before the fourth token


def _random_lexicon(seed, C, n_words, max_len):
    rng = np.random.default_rng(seed)
    lines, spelt = [], []
    for i in range(n_words):
        if spelt and rng.random() < 0.2:
            toks = spelt[int(rng.integers(len(spelt)))]                      # another word for a spelling there is
            if sum(1 for s in spelt if s == toks) >= 6:
                continue
        else:
            toks = ["w%d" % int(v) for v in rng.integers(5, C, int(rng.integers(1, max_len + 1)))]
            if rng.random() < 0.5:
                toks = toks + ["|"]
        spelt.append(toks)
        lines.append("x%d %s" % (i, " ".join(toks)))
    return "\n".join(lines) + "\n"


def _flat_lexicon():
    """the fullest node (the root) gives 29 candidates: fourteen children with a label and children, one with a label alone;
    the bound on a hypothesis's candidates is then 29 + 3 = 32, and beam 512 x 32 is CAP"""
    lines = []
    for i in range(14):
        lines.append("r%d w%d" % (i, 5 + i))
        for j in range(6):
            lines.append("r%d_%d w%d w%d" % (i, j, 5 + i, 5 + j))
    lines.append("leaf w19")
    return "\n".join(lines) + "\n"


LEXICONS = {"small": lambda: SMALL, "deep": lambda: DEEP, "mid": lambda: SMALL + _random_lexicon(3, 12, 30, 4),
            "big": lambda: _random_lexicon(4, 1024, 40, 3), "flat": _flat_lexicon}


def lexicon_path(name):
    path = os.path.join(_TMP.name, "%s.lex" % name)
    if not os.path.exists(path):
        with open(path, "w", encoding="utf-8") as f:
            f.write(LEXICONS[name]())
    return path


@functools.lru_cache(maxsize=None)
def lexicon_of(name, C, order, seed=0):
    """the Lexicon of LEXICONS[name] read from its file, with a random word LM of that order (0: none) read from an ARPA file.
    The LM lists every second word"""
    from unispeech_amd import ctc_lexicon, ctc_lm
    d = K.dictionary(C)
    words, spellings = ctc_lexicon.read_lexicon(lexicon_path(name), d)
    lm = None
    if order:
        listed = [w for w in words if w != "<unk>"][::2]
        entries = K.random_entries(100 + seed + order, listed, order, 0.5 if order <= 3 else 0.2)
        path = os.path.join(_TMP.name, "%s_%d_%d.arpa" % (name, order, seed))
        ctc_lm.write_arpa(path, order, entries)
        lm = ctc_lexicon.load_word_lm(path, words)
    return ctc_lexicon.Lexicon(words, spellings, d, lm)


# name: T, B, C, LM order (0: none), beam, beam_size_token, threshold, lm_weight, word_score, unk_weight, sil_weight, nbest,
# input lengths (None: all T), lexicon
CASES = {
    "beam1_T257": (257, 2, 8, 1, 1, 8, INF, 1.0, 1.0, -INF, 0.0, 1, [257, 256], "small"),
    "beam2_ktok1": (6, 3, 8, 3, 2, 1, INF, 0.5, 0.25, -INF, 0.0, 2, None, "small"),
    "ktok2": (9, 3, 8, 3, 6, 2, 2.5, 1.0, -0.5, -0.75, 0.25, 3, None, "small"),      # the root has three children
    "T1": (1, 3, 8, 3, 5, 8, INF, 2.0, 1.0, 0.5, 0.0, 3, None, "small"),
    "lengths": (9, 5, 8, 3, 6, 7, INF, 1.0, 0.5, -INF, 0.25, 3, [0, 8, 9, 1, 0], "small"),
    "beam63": (12, 2, 12, 3, 63, 11, INF, 1.0, 1.0, -1.0, 0.0, 3, None, "mid"),
    "beam64": (12, 2, 12, 3, 64, 12, INF, 0.5, 0.75, -INF, -0.5, 1, None, "mid"),
    "beam65_order5": (10, 2, 12, 5, 65, 14, INF, 0.25, 1.0, -0.25, 0.5, 65, None, "mid"),
    "cut": (12, 3, 12, 3, 16, 12, 2.5, 0.5, 1.0, -INF, -0.5, 3, None, "mid"),
    "thr0": (20, 3, 8, 1, 8, 8, 0.0, 1.0, 0.0, -INF, 0.0, 8, None, "small"),
    "nolm": (30, 3, 12, 0, 7, 12, 2.5, 0.0, 0.5, -2.0, -0.25, 3, [30, 29, 0], "mid"),
    "noroot": (2, 1, 8, 3, 1, 8, INF, 1.0, 1.0, -INF, 0.0, 1, None, "deep"),          # no survivor ends at the root
    "C1024": (5, 2, 1024, 3, 8, 16, INF, 1.0, 1.0, -1.0, 0.0, 3, None, "big"),
    # the two sides of LDS_CAP (the width of `mid` with <unk> words is 17): the kernel's two instantiations, beams that fill
    "cap_lds_edge": (5, 1, 12, 3, 481, 12, INF, 0.5, 1.0, -1.0, 0.0, 3, None, "mid"),
    "cap_big_edge": (5, 2, 12, 3, 482, 12, INF, 0.5, 1.0, -1.0, 0.25, 3, [5, 4], "mid"),
}
FLAT = "capacity"                      # flat emissions, beam 512 x width 32 = CAP, threshold infinity, T = 3: every candidate ties
ALL = list(CASES) + [FLAT]


@functools.lru_cache(maxsize=None)
def case(name):
    """(emissions fp32 [T, B, C], input lengths, dictionary, Lexicon, keyword options) -- treat as read-only"""
    if name == FLAT:
        T, B, C, order, beam, ktok, thr, lmw, wsc, unk, silw, nbest, il, lex = 3, 1, 32, 0, 512, 32, INF, 1.0, 0.0, -INF, 0.0, 3, None, "flat"
        x = torch.full((T, B, C), -1.0)
    else:
        T, B, C, order, beam, ktok, thr, lmw, wsc, unk, silw, nbest, il, lex = CASES[name]
        x = K.emissions(50 + sorted(ALL).index(name), T, B, C)
    if name == "noroot":                # w5, then w6: with beam 1 the survivor stands two tokens into `abc`
        x = torch.full((T, B, C), -10.0)
        x[0, 0, 5] = 0.0
        x[1, 0, 6] = 0.0
    il = [T] * B if il is None else il
    lexicon = lexicon_of(lex, C, order)
    width = lexicon.width(min(ktok, C), unk != -INF)
    if name == FLAT:
        assert beam * width == CAP, width
    if name == "cap_lds_edge":
        assert beam * width <= LDS_CAP < (beam + 1) * width, width
    if name == "cap_big_edge":
        assert (beam - 1) * width <= LDS_CAP < beam * width <= CAP, width
    big = max(abs(wsc), abs(unk) if unk != -INF else 0.0)
    bound = T * (10 + abs(silw) + lmw * 3.125 * order + big) + 2 * lmw * 3.125 * order
    assert T <= 300 and bound < 2 ** 15, (name, bound)
    opts = {"beam": beam, "beam_size_token": ktok, "beam_threshold": thr, "lm_weight": lmw, "word_score": wsc, "unk_weight": unk,
            "sil_weight": silw, "nbest": nbest}
    return x, il, K.dictionary(C), lexicon, opts


@functools.lru_cache(maxsize=None)
def reference(name, bf16=False):
    """lexicon_beam_decode of the case on the host (the float64 reference), once per process"""
    from unispeech_amd.ctc_lexicon import lexicon_beam_decode
    x, il, d, lexicon, opts = case(name)
    if bf16:
        x = bf16_emissions(name)
    return lexicon_beam_decode(x, il, d, lexicon, lexicon.lm, normalized=True, **opts)


@functools.lru_cache(maxsize=None)
def bf16_emissions(name):
    x, _, _, _, _ = case(name)
    T, B, C = x.shape
    return K.emissions(99, T, B, C, step=8, lo=-8)


# ------------------------------------------------------------------------------------------------------ normalized=False
INEXACT_OPTS = {"beam": 4, "beam_size_token": 6, "beam_threshold": INF, "lm_weight": 0.5, "word_score": 1.0, "unk_weight": -INF,
                "sil_weight": 0.0, "nbest": 2}
INEXACT_WORDS = ["AB", "CD", "A", "HELLO", "YOU", "AAB", "ABC", "HELL"]


@functools.lru_cache(maxsize=None)
def inexact():
    """(logits [T, B, 32], input lengths, dictionary, Lexicon with a bigram, reference hyps, tol per sample): raw logits, noise in
    [-1, 1] with +8 on a path of `|`-terminated words.  Asserts that every decision of the reference was taken by at least
    64 x tol."""
    import ctc_score_cases as S
    from unispeech_amd import ctc, ctc_lexicon, ctc_lm
    T = 12
    hyps = [S.ids("AB|CD|"), S.ids("A|"), [], S.ids("HELLO|YOU|"), S.ids("AAB|")]
    il = [T, T, T - 1, T, T]
    logits = S.logits_for(hyps, T, il, 1000)
    d = S.dictionary()
    path = os.path.join(_TMP.name, "inexact.lex")
    with open(path, "w", encoding="utf-8") as f:
        f.write("".join("%s %s |\n" % (w, " ".join(w)) for w in INEXACT_WORDS))
    words, spellings = ctc_lexicon.read_lexicon(path, d)
    arpa = os.path.join(_TMP.name, "inexact.arpa")
    ctc_lm.write_arpa(arpa, 2, K.random_entries(21, INEXACT_WORDS[::2], 2, 0.3))
    lexicon = ctc_lexicon.Lexicon(words, spellings, d, ctc_lexicon.load_word_lm(arpa, words))
    ref, margin, abs_sum = ctc_lexicon.lexicon_beam_search_reference(logits, il, lexicon, BLANK, ctc.silence_token(d),
                                                                     normalized=False, **INEXACT_OPTS)
    tol = [(T + 8) * 2.0 ** -23 * a for a in abs_sum]
    for b in range(len(il)):
        assert margin[b] >= 64 * tol[b], (b, margin[b], tol[b])
    ref = [[([lexicon.words[w] for w in wds], toks, sc) for wds, toks, sc in h] for h in ref]
    return logits, il, d, lexicon, ref, tol
