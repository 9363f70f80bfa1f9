"""The lexicon-constrained CTC beam search without a GPU: the lexicon reader, the trie and its smearing against a direct
recomputation, the float64 reference against brute force over every frame path and every parse and against the lexicon-free
reference on a degenerate lexicon, the refusals, the command line, and the ABI bookkeeping.  The inputs are in
tests/ctc_lexicon_cases.py."""
import itertools
import math
import os
import re

import numpy as np
import pytest
import torch

import ctc_beam_cases as K
import ctc_lexicon_cases as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = math.inf


# ------------------------------------------------------------------------------------------------------------ the reader
def _lex(tmp_path, text):
    p = tmp_path / "x.lex"
    p.write_text(text)
    return str(p)


def test_reader_formats_duplicates_and_word_ids(tmp_path):
    from unispeech_amd import ctc_lexicon
    d = K.dictionary(8)
    words, spellings = ctc_lexicon.read_lexicon(_lex(tmp_path, "b  w6\t|\n\na w5\nb w6 |\nb w6\n a   w5 | \n"), d)
    assert words == ["b", "a", "<unk>"]                                   # first appearance; <unk> appended
    assert spellings == [(0, (6, 4)), (1, (5,)), (0, (6,)), (1, (5, 4))]  # the exact duplicate counts once
    words, spellings = ctc_lexicon.read_lexicon(_lex(tmp_path, "a w5\n<unk> w6\nb w7\n"), d)
    assert words == ["a", "<unk>", "b"] and len(spellings) == 3           # a listed <unk> keeps its place
    words, spellings = ctc_lexicon.read_lexicon(L.lexicon_path("small"), d)
    assert words == ["a", "ab", "ab2", "ab3", "cc", "c|a", "b", "b2", "oov", "abc", "<unk>"] and len(spellings) == 11


def test_reader_refusals_name_the_line(tmp_path):
    from unispeech_amd import ctc_lexicon
    d = K.dictionary(8)
    for text, what in (("a w5\nb w9\n", r"x\.lex:2: the token 'w9'"), ("a w5\n\nb <unk>\n", r"x\.lex:3: the token '<unk>'"),
                       ("a w5\nb\n", r"x\.lex:2: .*empty spelling"), ("a | w5\n", r"x\.lex:1: .*begin with the silence"),
                       ("".join("h%d w5 w6\n" % i for i in range(7)), r"x\.lex:7: more than 6 words")):
        with pytest.raises(ValueError, match=what):
            ctc_lexicon.read_lexicon(_lex(tmp_path, text), d)
    assert len(ctc_lexicon.read_lexicon(_lex(tmp_path, "".join("h%d w5 w6\n" % i for i in range(6))), d)[1]) == 6
    with pytest.raises(ValueError, match="6 words share"):
        ctc_lexicon.Lexicon(["h%d" % i for i in range(7)] + ["<unk>"], [(i, (5, 6)) for i in range(7)], d)
    with pytest.raises(ValueError, match="silence"):
        ctc_lexicon.Lexicon(["a", "<unk>"], [(0, (4, 5))], d)
    with pytest.raises(ValueError, match="<unk>"):
        ctc_lexicon.Lexicon(["a"], [(0, (5,))], d)


# ---------------------------------------------------------------------------------------------------- trie and smearing
@pytest.mark.parametrize("name,C,order", [("small", 8, 0), ("small", 8, 3), ("mid", 12, 5), ("big", 1024, 1)])
def test_trie_and_smearing_against_a_direct_recomputation(name, C, order):
    from unispeech_amd import ctc_lexicon
    lx = L.lexicon_of(name, C, order)
    d = K.dictionary(C)
    words, spellings = ctc_lexicon.read_lexicon(L.lexicon_path(name), d)
    assert lx.words == words and lx.unk_word == words.index("<unk>")
    by_prefix = {}
    for w, toks in spellings:
        for k in range(len(toks) + 1):
            by_prefix.setdefault(toks[:k], set())
        by_prefix[toks].add(w)
    assert len(lx) == len(by_prefix)
    u = [lx.lm.score_word(lx.lm.start, int(lx.lm.tok_word[w]))[0] if lx.lm is not None else 0.0 for w in range(len(words))]
    if lx.lm is not None:                                       # a word the LM does not list takes <unk>'s row
        unk = lx.lm.score_word(lx.lm.start, int(lx.lm.tok_word[lx.unk_word]))[0]
        listed = set(g[0] for g in lx.lm.entries if len(g) == 1)
        assert any(w not in listed for w in words) and all(u[i] == unk for i, w in enumerate(words) if w not in listed)
    for prefix, ends in by_prefix.items():
        v = 0
        for t in prefix:
            v = lx.child(v, t)
            assert v > 0
        assert lx.labels(v) == sorted(ends)
        toks = lx.child_tok[lx.child_off[v]:lx.child_off[v + 1]].tolist()
        assert toks == sorted(set(p[len(prefix)] for p in by_prefix if len(p) > len(prefix) and p[:len(prefix)] == prefix))
        below = [u[w] for w, s in spellings if s[:len(prefix)] == prefix]           # MAX smearing: the best word at or below
        assert lx.node_max[v] == max(below), prefix
        assert lx.child(v, 0) == -1
    t = lx.to("cpu")
    assert t["node_max"].dtype == torch.float32 and t["child_off"].numel() == len(lx) + 1 and lx.to("cpu") is t
    assert torch.equal(t["node_max"].double(), torch.from_numpy(lx.node_max))       # dyadic: exact in fp32
    # the bound on a hypothesis's candidates
    for unk in (False, True):
        per_node = []
        for v in range(len(lx)):
            n = 0
            for c in lx.child_node[lx.child_off[v]:lx.child_off[v + 1]]:
                n += int(lx.child_off[c + 1] > lx.child_off[c]) + max(len(lx.labels(c)), 1 if unk else 0)
            per_node.append(n)
        assert lx.width(C, unk) == max(per_node) + 3 and lx.width(1, unk) == min(1 + lx.max_labels, max(per_node)) + 3


# -------------------------------------------------------------------------------------------------------- the reference
BRUTE = """a w5
a2 w5
ab w5 w6 |
bb w6 w6
b|a w6 | w5
b w6 |
oov w6
"""


def _collapse(path, blank=0):
    out, last = [], -1
    for a in path:
        if a != last and a != blank:
            out.append(a)
        last = a
    return out


def _parses(seq, spell_words, sil):
    """every way to read the collapsed tokens as words and silences between words, ending between words: lists of words"""
    if not seq:
        yield []
        return
    if seq[0] == sil:
        yield from _parses(seq[1:], spell_words, sil)
        return
    for k in range(1, len(seq) + 1):
        for w in spell_words.get(tuple(seq[:k]), ()):
            for rest in _parses(seq[k:], spell_words, sil):
                yield [w] + rest


@pytest.mark.parametrize("order", [0, 1, 2, 3])
def test_reference_with_an_unbounded_beam_equals_brute_force(tmp_path, order):
    """every one of the paths over the live classes (the blank, `|`, w5, w6: no other class has a child in the trie) and every
    parse of its collapse that ends between words, scored from the definition: emissions, sil_weight per silence frame, per word
    word_score and Katz on the full history, </s> at the end.  The best score is equal exactly."""
    from unispeech_amd import ctc_lexicon, ctc_lm
    Cn, used = 7, [0, 4, 5, 6]
    d = K.dictionary(Cn)
    words, spellings = ctc_lexicon.read_lexicon(_lex(tmp_path, BRUTE), d)
    spell_words = {}
    for w, toks in spellings:
        spell_words.setdefault(toks, []).append(words[w])
    rng = np.random.default_rng(11 + order)
    n = 0
    for trial in range(5):
        lm, entries = None, None
        if order:
            entries = K.random_entries(70 + 10 * order + trial, ["a", "ab", "bb", "b"], order)
            arpa = str(tmp_path / ("lm%d.arpa" % trial))
            ctc_lm.write_arpa(arpa, order, entries)
            lm = ctc_lexicon.load_word_lm(arpa, words)
        lexicon = ctc_lexicon.Lexicon(words, spellings, d, lm)
        T = int(rng.integers(1, 6))
        em = np.full((T, 1, Cn), -1000.0)
        em[:, 0, used] = rng.integers(-640, 1, (T, len(used))) / 64.0
        w, silw = float(rng.choice([0.25, 0.5, 1.0, 2.0])), float(rng.choice([0.0, -0.5, 0.25]))
        wsc = float(rng.choice([0.0, 1.0, -0.75]))
        best = None
        for path in itertools.product(used, repeat=T):
            base = sum(em[t, 0, a] for t, a in enumerate(path)) + silw * sum(1 for a in path if a == K.BAR)
            for parse in _parses(_collapse(path), spell_words, K.BAR):
                sc, h = base, ["<s>"]
                for word in parse:
                    sc += wsc
                    if order:
                        word = word if (word,) in entries else "<unk>"
                        sc += w * K.katz(entries, order, h, word)
                        h.append(word)
                if order:
                    sc += w * K.katz(entries, order, h, "</s>")
                if best is None or sc > best:
                    best = sc
        ref, _, _ = ctc_lexicon.lexicon_beam_search_reference(em, None, lexicon, K.BLANK, K.BAR, beam=10 ** 6, beam_size_token=Cn,
                                                              beam_threshold=INF, lm_weight=w, word_score=wsc, unk_weight=-INF,
                                                              sil_weight=silw, nbest=1, normalized=True)
        assert ref[0][0][2] == best, (order, trial, ref[0][0], best)
        n += 1
    assert n == 5


class _PlainDictionary:
    """classes s0 (the blank) .. s(C-1), no silence token and no unk: every non-blank class may be a one-token word"""

    def __init__(self, C):
        self.symbols = ["s%d" % i for i in range(C)]

    def __len__(self):
        return len(self.symbols)

    def index(self, sym):
        return self.symbols.index(sym)

    def bos(self):
        return 0

    def eos(self):
        return -1

    def unk(self):
        return -1


def test_a_one_token_word_per_class_gives_the_lexicon_free_search():
    """word_score 0, no silence token, every class considered: the n-best, tokens and scores of ctc.beam_search_reference"""
    from unispeech_amd import ctc, ctc_lexicon, ctc_lm
    rng = np.random.default_rng(2)
    for trial in range(15):
        Cn, T, order = int(rng.integers(4, 9)), int(rng.integers(2, 9)), int(rng.integers(0, 4))
        d = _PlainDictionary(Cn)
        words = d.symbols[1:] + ["<unk>"]
        spellings = [(c - 1, (c,)) for c in range(1, Cn)]
        unit_lm = word_lm = None
        if order:
            entries = K.random_entries(300 + trial, d.symbols[1::2], order)
            unit_lm = ctc_lm.NgramLM(order, entries, d.symbols)
            word_lm = ctc_lm.NgramLM(order, entries, words)
        lexicon = ctc_lexicon.Lexicon(words, spellings, d, word_lm)
        x = rng.integers(-4 * 8, 1, (T, 2, Cn)) / 8.0                      # coarse: ties occur
        opts = {"beam": int(rng.choice([1, 2, 5, 50])), "beam_size_token": Cn, "beam_threshold": float(rng.choice([INF, 2.5])),
                "lm_weight": float(rng.choice([0.5, 1.0])), "sil_weight": 0.0, "nbest": 3}
        want = ctc.beam_search_reference(x, None, 0, -1, unit_lm, normalized=True, **opts)[0]
        got = ctc_lexicon.lexicon_beam_search_reference(x, None, lexicon, 0, -1, word_score=0.0, unk_weight=-INF, normalized=True,
                                                        **opts)[0]
        for g, w in zip(got, want):
            assert [(h[1], h[2]) for h in g] == w, trial
            assert all(h[0] == [t - 1 for t in h[1]] for h in g)           # the words are the tokens


def test_a_word_is_completed_once_by_frames_that_repeat_its_token():
    from unispeech_amd import ctc_lexicon
    lexicon = L.lexicon_of("small", 8, 0)
    x = torch.full((3, 1, 8), -10.0)
    x[:, 0, 5] = 0.0                                                        # w5 w5 w5: `a` once
    opts = {"beam": 50, "beam_threshold": INF, "lm_weight": 0.0, "word_score": 1.0, "normalized": True}
    got = ctc_lexicon.lexicon_beam_decode(x, None, K.dictionary(8), lexicon, None, **opts)
    assert got == [[(["a"], [5], 1.0)]]
    x[1, 0, 5], x[1, 0, 0] = -10.0, 0.0                                     # w5 blank w5: twice
    got = ctc_lexicon.lexicon_beam_decode(x, None, K.dictionary(8), lexicon, None, **opts)
    assert got == [[(["a", "a"], [5, 5], 2.0)]]


def test_no_survivor_at_the_root_all_finish():
    """beam 1 on w5, w6 under a lexicon whose only word is w5 w6 w7 |: the survivor stands two tokens into the word"""
    got = L.reference("noroot")
    lexicon = L.case("noroot")[3]
    node = lexicon.child(lexicon.child(0, 5), 6)
    assert node > 0 and lexicon.labels(node) == [] and got == [[([], [5, 6], got[0][0][2])]]


def test_the_cases_and_the_inexact_margin():
    for name in L.ALL:
        x, il, d, lexicon, opts = L.case(name)                             # asserts the magnitude bound
        assert torch.equal(x * 64, (x * 64).round())
    L.inexact()                                                            # asserts margin >= 64 tol
    assert [len(h) for h in L.reference(L.FLAT)] == [3]
    assert L.reference("lengths")[0] == L.reference("lengths")[4] and L.reference("lengths")[0][0][:2] == ([], [])


# ------------------------------------------------------------------------------------------------------------ refusals
def test_refusals_by_name():
    from unispeech_amd import ctc, ctc_lexicon
    d = K.dictionary(8)
    lexicon = L.lexicon_of("small", 8, 0)
    x = torch.zeros(2, 1, 8)
    for kw, name in (({"beam": 0}, "beam"), ({"beam_size_token": 0}, "beam_size_token"), ({"nbest": 0}, "nbest"),
                     ({"beam_threshold": -1.0}, "beam_threshold"), ({"lm_weight": INF}, "lm_weight"),
                     ({"word_score": INF}, "word_score"), ({"unk_weight": INF}, "unk_weight"),
                     ({"unk_weight": float("nan")}, "unk_weight")):
        with pytest.raises(ValueError, match=name):
            ctc_lexicon.lexicon_beam_decode(x, None, d, lexicon, None, **kw)
    with pytest.raises(ValueError, match="finite"):
        ctc_lexicon.lexicon_beam_decode(torch.full((2, 1, 8), -INF), None, d, lexicon, None, normalized=True)
    with pytest.raises(ValueError, match="lexicon was built with"):
        ctc_lexicon.lexicon_beam_decode(x, None, d, lexicon, L.lexicon_of("small", 8, 3).lm)
    with pytest.raises(ValueError, match="token 7"):
        ctc_lexicon.lexicon_beam_decode(torch.zeros(2, 1, 7), None, K.dictionary(7), lexicon, None)
    # the criterion keeps refusing the decoder options
    for name in ("wer_kenlm_model", "wer_lexicon", "wer_args"):
        with pytest.raises(NotImplementedError, match=name):
            ctc.CtcCriterion(d, **{name: "x"})


def test_command_line():
    from unispeech_amd import ctc, ctc_lexicon
    a = ctc_lexicon.parse_args(["score", "ck.pt", "dict.txt", "m.tsv", "l.ltr", "--lexicon", "lex.txt", "--lm", "x.arpa", "--beam",
                                "500", "--beam-size-token", "32", "--beam-threshold", "20", "--lm-weight", "1.5", "--word-score",
                                "-0.5", "--unk-weight", "-3", "--sil-weight", "-0.25", "--nbest", "2", "--results", "out"])
    assert (a.cmd, a.ckpt, a.dict, a.manifest, a.labels, a.lexicon, a.lm, a.results) == \
        ("score", "ck.pt", "dict.txt", "m.tsv", "l.ltr", "lex.txt", "x.arpa", "out")
    assert (a.beam, a.beam_size_token, a.beam_threshold, a.lm_weight, a.word_score, a.unk_weight, a.sil_weight, a.nbest) == \
        (500, 32, 20.0, 1.5, -0.5, -3.0, -0.25, 2)
    a = ctc_lexicon.parse_args(["decode", "ck.pt", "dict.txt", "a.wav", "b.wav", "--lexicon", "lex.txt"])
    assert a.wavs == ["a.wav", "b.wav"] and a.lm is None and a.word_score == 1.0 and a.unk_weight == -INF
    assert (a.beam, a.beam_size_token, a.beam_threshold, a.lm_weight, a.sil_weight, a.nbest) == (50, 100, 25.0, 0.2, 0.0, 1)
    with pytest.raises(SystemExit):                                         # --lexicon is required here
        ctc_lexicon.parse_args(["decode", "ck.pt", "dict.txt", "a.wav"])
    with pytest.raises(NotImplementedError, match="binary format"):
        ctc_lexicon.parse_args(["decode", "ck.pt", "dict.txt", "a.wav", "--lexicon", "lex.txt", "--lm", "lm.bin"])
    with pytest.raises(SystemExit):                                         # and still unknown to unispeech_amd.ctc
        ctc.parse_args(["decode", "ck.pt", "dict.txt", "a.wav", "--lexicon", "lex.txt"])
    with pytest.raises(SystemExit):
        ctc.parse_args(["score", "ck.pt", "dict.txt", "m.tsv", "l.ltr", "--lexicon", "lex.txt"])


# --------------------------------------------------------------------------------------------------- the library, no GPU
NEW = ("wavlm_ctc_lexbeam_supported", "wavlm_ctc_lexbeam_workspace_bytes", "wavlm_ctc_lexbeam")


def test_abi_stays_30_and_the_new_symbols_are_declared_exported_and_bound():
    import ctypes
    from unispeech_amd import _lib, build
    src = open(os.path.join(ROOT, "include", "wavlm_hip.h")).read()
    assert int(re.search(r"#define WAVLM_HIP_ABI_VERSION (\d+)", src).group(1)) == 30 == _lib.ABI_VERSION
    assert "ctc_lexbeam.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "ctc_lexbeam.hip"))
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    if not os.path.exists(_lib.LIB_PATH):
        build.build_library(verbose=False)
    h = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        decl = re.search(r"\b%s\(([^;]*)\);" % name, code).group(1)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[name][1]), name
        assert hasattr(h, name), name
    assert _lib.lib().wavlm_abi_version() == 30


def test_the_envelope_and_the_refusals_of_the_binding():
    import ctypes
    from unispeech_amd import _lib, ops
    lib = _lib.lib()
    ok = lib.wavlm_ctc_lexbeam_supported                                    # (C, beam, width, lm order, trie nodes)
    assert ok(32, 500, 31, 4, 10 ** 6) and ok(1024, 512, 32, 6, 1) and ok(32, 1, 16384, 0, 2 ** 21) and ok(1, 1, 1, 0, 1)
    assert not ok(1025, 1, 1, 0, 1) and not ok(32, 513, 1, 0, 1) and not ok(32, 0, 1, 0, 1) and not ok(32, 1, 0, 0, 1)
    assert not ok(32, 1, 1, 7, 1) and not ok(32, 1, 1, 0, 0) and not ok(32, 1, 1, 0, 2 ** 21 + 1)
    assert not ok(32, 265, 62, 4, 10) and not ok(32, 512, 33, 0, 10) and ok(32, 264, 62, 0, 10)
    assert ops.ctc_lexbeam_max_beam(32, 62, 0, 10) == L.CAP // 62 == 264 and ops.ctc_lexbeam_max_beam(32, 16, 0, 10) == 512
    assert ops.ctc_lexbeam_max_beam(32, L.CAP + 1, 0, 10) == 0 and ops.ctc_lexbeam_max_beam(1025, 1, 0, 10) == 0
    need = lib.wavlm_ctc_lexbeam_workspace_bytes(32, 749, 264, 31)
    assert need >= 32 * 749 * 264 * 8 + 32 * 264 * 31 * 4 and need % 256 == 0
    assert lib.wavlm_ctc_lexbeam_workspace_bytes(32, 749, 500, 31) >= 32 * 749 * 500 * 8 + 32 * 500 * 31 * 12
    assert lib.wavlm_ctc_lexbeam_workspace_bytes(2 ** 31 - 1, 2 ** 31 - 1, 512, 32) == 0          # no wrap-around: refused
    assert lib.wavlm_ctc_lexbeam_workspace_bytes(-1, 1, 1, 1) == 0
    for args, name in (((1025, 1, 1, 0, 1), "C = 1025"), ((32, 513, 1, 0, 1), "beam = 513"), ((32, 4, 4, 7, 1), "order = 7"),
                       ((32, 4, 4, 0, 2 ** 21 + 1), "trie nodes"), ((32, 265, 62, 4, 10), "beam = 265 .* beam <= 264")):
        with pytest.raises(NotImplementedError, match=name):
            ops.ctc_lexbeam_check_supported(*args)
    # -1 before anything is launched: a NULL pointer, a short workspace, sizes beyond the envelope.  The pointers are host
    # buffers that are never read
    buf = (ctypes.c_int32 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    lex = [p, p, p, p, p, p, 3, 2, 2, 3, 4, 2]                              # six tables; nodes, children, labels, words, width, unk

    def call(logits=p, lex=lex, beam=2, ws=p, ws_bytes=1 << 20, nbest=1, words=p, unk_score=-INF):
        return lib.wavlm_ctc_lexbeam(logits, 0, 16, 8, 1, 2, 8, p, 0, 4, 1, None, None, None, None, None, None, None, 0, 0, 0, 0, 0,
                                     *lex, beam, 8, INF, 1.0, 1.0, unk_score, 0.0, nbest, p, p, p, p, words, p, ws, ws_bytes, None)
    assert call(logits=None) == -1 and call(words=None) == -1 and call(ws=None) == -1
    assert call(ws_bytes=lib.wavlm_ctc_lexbeam_workspace_bytes(1, 2, 2, 4) - 1) == -1
    assert call(lex=[None] + lex[1:]) == -1 and call(lex=lex[:3] + [None] + lex[4:]) == -1
    assert call(beam=513) == -1 and call(beam=2049) == -1 and call(nbest=3) == -1 and call(unk_score=INF) == -1
    assert call(lex=lex[:6] + [0] + lex[7:]) == -1 and call(lex=lex[:11] + [3]) == -1      # no trie node; unk not a word
