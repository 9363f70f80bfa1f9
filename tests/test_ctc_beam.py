"""The CTC beam search without a GPU: the ARPA reader and the table walk against Katz backoff from its definition, the float64
reference against brute force over every path and against the greedy decode, the refusals, and the ABI bookkeeping.  The inputs
are in tests/ctc_beam_cases.py."""
import itertools
import os
import re

import numpy as np
import pytest
import torch

import ctc_beam_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# --------------------------------------------------------------------------------------------------------------- the LM
@pytest.mark.parametrize("order", [1, 2, 3, 4])
def test_arpa_round_trip_and_table_walk_equals_katz(order):
    """over a 3-symbol vocabulary (classes 4, 5 and 7 of an 8-class dictionary have words): every history of length 0 to 5, every
    next word and </s> -- exact, the values are dyadic"""
    from unispeech_amd import ctc_lm
    lm, entries, path = K.lm_of(8, order, 40 + order)
    assert ctc_lm.read_arpa(path) == (order, entries) and lm.order == order
    if order >= 3:                                         # the file is not suffix-closed
        assert any(len(g) > 1 and g[1:] not in entries for g in entries)
    d = K.dictionary(8)
    toks = [4, 5, 7]
    for L in range(6):
        for hist in itertools.product(toks, repeat=L):
            words = ["<s>"] + [d.symbols[t] for t in hist]
            state = lm.start
            for t in hist:
                state = lm.score(state, t)[1]
            assert state == lm.state_of(words)
            for t in toks:
                assert lm.score(state, t)[0] == K.katz(entries, order, words, d.symbols[t]), (order, hist, t)
            assert lm.score_eos(state) == K.katz(entries, order, words, "</s>"), (order, hist)


def test_symbols_the_file_does_not_list_take_the_unk_row():
    lm, entries, _ = K.lm_of(8, 2, 42)
    d = K.dictionary(8)
    assert d.symbols[6] == "w6" and ("w6",) not in entries
    for state in (lm.start, lm.score(lm.start, 5)[1]):
        assert lm.score(state, 6) == lm.score(state, K.UNK) == lm.score(state, K.PAD)
    assert lm.score(lm.start, 6)[0] == K.katz(entries, 2, ["<s>"], "<unk>")
    t = lm.to("cpu")
    assert t["child_logp"].dtype == torch.float32 and t["child_off"].numel() == len(lm) + 1 and t["tok_word"].numel() == 8
    assert lm.to("cpu") is t


def _arpa(tmp_path, text):
    p = tmp_path / "x.arpa"
    p.write_text(text)
    return str(p)


GOOD = "\\data\\\nngram 1=4\nngram 2=1\n\n\\1-grams:\n-1.0\t<unk>\t-0.5\n-1.0\t<s>\t-0.5\n-1.0\t</s>\n-1.0\ta\t-0.25\n\n" \
       "\\2-grams:\n-0.5\ta </s>\n\n\\end\\\n"


def test_malformed_files_are_refused_by_line(tmp_path):
    from unispeech_amd import ctc_lm
    order, entries = ctc_lm.read_arpa(_arpa(tmp_path, GOOD))
    assert order == 2 and entries[("a",)] == (-1.0, -0.25) and entries[("</s>",)] == (-1.0, 0.0) and entries[("a", "</s>")][0] == -0.5
    for w in ("<unk>", "<s>", "</s>"):
        with pytest.raises(ValueError, match=re.escape(w)):
            ctc_lm.read_arpa(_arpa(tmp_path, GOOD.replace("-1.0\t%s" % w, "-1.0\tb")))
    with pytest.raises(ValueError, match=r"x\.arpa:7: not a number"):
        ctc_lm.read_arpa(_arpa(tmp_path, GOOD.replace("-1.0\t<s>", "abc\t<s>")))
    with pytest.raises(ValueError, match=r"x\.arpa:12: a 2-gram line"):
        ctc_lm.read_arpa(_arpa(tmp_path, GOOD.replace("-0.5\ta </s>", "-0.5\ta")))
    with pytest.raises(ValueError, match=r"x\.arpa:\d+: .*header says 4"):
        ctc_lm.read_arpa(_arpa(tmp_path, GOOD.replace("-1.0\ta\t-0.25\n", "")))
    with pytest.raises(ValueError, match=r"x\.arpa:\d+: expected \\end"):
        ctc_lm.read_arpa(_arpa(tmp_path, GOOD.replace("\\end\\\n", "")))
    with pytest.raises(ValueError, match=r"x\.arpa:1: expected \\data"):
        ctc_lm.read_arpa(_arpa(tmp_path, "junk\n" + GOOD))
    with pytest.raises(ValueError, match="orders 1 to 6"):
        ctc_lm.read_arpa(_arpa(tmp_path, "\\data\\\n" + "".join("ngram %d=0\n" % k for k in range(1, 8)) + "\\end\\\n"))


# -------------------------------------------------------------------------------------------------------- the reference
def _collapse(path, blank=0):
    out, last = [], -1
    for a in path:
        if a != last and a != blank:
            out.append(a)
        last = a
    return out


def test_reference_with_an_unbounded_beam_equals_brute_force():
    """every one of the C^T paths scored from the definition: emissions, sil_weight per silence frame, Katz on the collapsed
    sequence's full history, </s> at the end.  The best score is equal exactly."""
    from unispeech_amd import ctc
    rng = np.random.default_rng(5)
    n = 0
    for trial in range(24):
        Cn, T, order = int(rng.integers(5, 8)), int(rng.integers(1, 6)), int(rng.integers(1, 4))
        used = [0, 4] + list(range(5, Cn))                   # the blank, `|` and the w symbols: C <= 4 live classes
        used = used[:4]
        lm, entries, _ = K.lm_of(Cn, order, 60 + trial)
        d = K.dictionary(Cn)
        em = np.full((T, 1, Cn), -1000.0)
        em[:, 0, used] = rng.integers(-640, 1, (T, len(used))) / 64.0
        w, silw = float(rng.choice([0.25, 0.5, 1.0, 2.0])), float(rng.choice([0.0, -0.5]))
        best = None
        for path in itertools.product(used, repeat=T):
            sc = sum(em[t, 0, a] for t, a in enumerate(path)) + silw * sum(1 for a in path if a == K.BAR)
            h = ["<s>"]
            for a in _collapse(path):
                word = d.symbols[a] if (d.symbols[a],) in entries else "<unk>"
                sc += w * K.katz(entries, order, h, word)
                h.append(word)
            sc += w * K.katz(entries, order, h, "</s>")
            if best is None or sc > best:
                best = sc
        ref, _, _ = ctc.beam_search_reference(em, None, K.BLANK, K.BAR, lm, beam=10 ** 6, beam_size_token=len(used),
                                              beam_threshold=K.INF, lm_weight=w, sil_weight=silw, nbest=1, normalized=True)
        assert ref[0][0][1] == best, (trial, ref[0][0], best)
        n += 1
    assert n == 24


@pytest.mark.parametrize("beam", [1, 2, 5])
def test_without_an_lm_the_one_best_is_the_greedy_decode(beam):
    from unispeech_amd import ctc
    rng = np.random.default_rng(beam)
    for trial in range(40):
        Cn, T, B = int(rng.integers(5, 12)), int(rng.integers(1, 14)), 3
        x = np.stack([rng.permutation(Cn * T).reshape(T, Cn) for _ in range(B)], 1) / 8.0      # a unique maximum per frame
        x = torch.from_numpy(x)
        il = [T, max(T - 1, 0), 0]
        for normalized in (False, True):
            got = ctc.beam_decode(x, il, K.dictionary(Cn), None, beam=beam, beam_size_token=int(rng.integers(1, Cn + 3)),
                                  beam_threshold=25.0, sil_weight=0.0, normalized=normalized)
            assert [h[0][0] for h in got] == ctc.greedy_decode(x, il, K.BLANK)
    assert ctc.beam_decode(x[:, :1], [0], K.dictionary(Cn), None) == [[([], 0.0)]]


def test_margin_and_abs_sum_of_the_reference():
    from unispeech_amd import ctc
    lm = K.lm_of(8, 2, 42)[0]
    x = np.full((2, 1, 8), -9.0)
    x[0, 0, 5] = -0.5
    x[1, 0, 0] = -0.25
    x[1, 0, 5] = -8.0
    ref, margin, abs_sum = ctc.beam_search_reference(x, None, K.BLANK, K.BAR, lm, beam=1, beam_size_token=2, beam_threshold=K.INF,
                                                     lm_weight=0.5, sil_weight=0.0, nbest=1, normalized=True)
    l5, st = lm.score(lm.start, 5)
    end = lm.score_eos(st)
    assert ref == [[([5], -0.5 + 0.5 * l5 - 0.25 + 0.5 * end)]]
    assert abs_sum == [0.5 + abs(0.5 * l5) + 0.25 + abs(0.5 * end)]
    # frame 0: class 5 against the blank at -9 (the two considered classes), beam 1; frame 1: the blank against class 5 repeated
    assert margin == [min((-0.5 + 0.5 * l5) - -9.0, 7.75)]
    K.inexact()                                           # asserts margin >= 64 tol for the normalized=False case


def test_silence_token():
    from unispeech_amd import ctc
    assert ctc.silence_token(ctc.LetterDictionary(["A", "|", "<sep>"])) == 6
    assert ctc.silence_token(ctc.LetterDictionary(["A", "|"])) == 5
    assert ctc.silence_token(ctc.LetterDictionary(["A"])) == 2


# ------------------------------------------------------------------------------------------------------------ refusals
def test_refusals_by_name(tmp_path):
    from unispeech_amd import ctc
    d = K.dictionary(8)
    x = torch.zeros(2, 1, 8)
    for kw, name in (({"beam": 0}, "beam"), ({"beam_size_token": 0}, "beam_size_token"), ({"nbest": 0}, "nbest"),
                     ({"beam_threshold": -1.0}, "beam_threshold"), ({"lm_weight": K.INF}, "lm_weight")):
        with pytest.raises(ValueError, match=name):
            ctc.beam_decode(x, None, d, None, **kw)
    with pytest.raises(ValueError, match="finite"):
        ctc.beam_decode(torch.full((2, 1, 8), -K.INF), None, d, None, normalized=True)
    with pytest.raises(ValueError, match="maps 8 symbols"):
        ctc.beam_decode(torch.zeros(2, 1, 9), None, K.dictionary(9), K.lm_of(8, 2, 42)[0])
    # the lexicon / word-LM decoder and KenLM's binary format stay unbuilt
    for name in ("wer_kenlm_model", "wer_lexicon", "wer_args"):
        with pytest.raises(NotImplementedError, match=name):
            ctc.CtcCriterion(d, **{name: "x"})
    with pytest.raises(NotImplementedError, match="binary format"):
        ctc.parse_args(["decode", "ck.pt", "dict.txt", "a.wav", "--lm", "lm.bin"])
    with pytest.raises(SystemExit):
        ctc.parse_args(["decode", "ck.pt", "dict.txt", "a.wav", "--lexicon", "lex.txt"])
    a = ctc.parse_args(["score", "ck.pt", "dict.txt", "m.tsv", "l.ltr", "--lm", "x.arpa", "--beam", "500", "--beam-size-token", "32",
                        "--beam-threshold", "20", "--lm-weight", "1.5", "--sil-weight", "-0.5", "--nbest", "2"])
    assert (a.lm, a.beam, a.beam_size_token, a.beam_threshold, a.lm_weight, a.sil_weight, a.nbest) == \
        ("x.arpa", 500, 32, 20.0, 1.5, -0.5, 2)
    a = ctc.parse_args(["decode", "ck.pt", "dict.txt", "a.wav"])
    assert a.lm is None and a.beam == 50 and a.beam_size_token == 100 and a.beam_threshold == 25.0 and a.lm_weight == 0.2


# --------------------------------------------------------------------------------------------------- the library, no GPU
NEW = ("wavlm_ctc_beam_supported", "wavlm_ctc_beam_workspace_bytes", "wavlm_ctc_beam")


def test_abi_stays_30_and_the_new_symbols_are_declared_exported_and_bound():
    import ctypes
    from unispeech_amd import _lib, build
    src = open(os.path.join(ROOT, "include", "wavlm_hip.h")).read()
    assert int(re.search(r"#define WAVLM_HIP_ABI_VERSION (\d+)", src).group(1)) == 30 == _lib.ABI_VERSION
    assert "ctc_beam.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "ctc_beam.hip"))
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
    from unispeech_amd import _lib, ops
    L = _lib.lib()
    ok = L.wavlm_ctc_beam_supported
    assert ok(32, 500, 32, 4) and ok(1024, 512, 16, 6) and ok(1024, 16, 1024, 0) and ok(200, 100, 100, 3) and ok(32, 512, 10 ** 6, 0)
    assert not ok(1025, 1, 1, 0) and not ok(32, 513, 1, 0) and not ok(32, 0, 1, 0) and not ok(32, 1, 0, 0) and not ok(32, 1, 1, 7)
    assert not ok(64, 512, 33, 0) and ok(64, 512, 32, 0) and not ok(1024, 17, 1024, 0)
    assert L.wavlm_ctc_beam_workspace_bytes(32, 749, 500) >= 32 * 749 * 500 * 4
    assert L.wavlm_ctc_beam_workspace_bytes(32, 749, 500) % 256 == 0 and L.wavlm_ctc_beam_workspace_bytes(-1, 1, 1) == 0
    for args, name in (((1025, 1, 1, 0), "C = 1025"), ((32, 513, 1, 0), "beam = 513"), ((32, 4, 4, 7), "order = 7"),
                       ((64, 512, 33, 0), "beam_size_token = 33")):
        with pytest.raises(NotImplementedError, match=name):
            ops.ctc_beam_check_supported(*args)
