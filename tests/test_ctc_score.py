"""CTC validation scoring without a GPU: the host path of error_counts against a full-matrix Levenshtein written here (it is what
tests/test_ctc_score_gpu.py holds the kernel to), the class table of word_classes, the two host functions of the library, the ABI
bookkeeping, and the files and arguments of `python -m unispeech_amd.ctc score`."""
import os
import re

import numpy as np
import pytest
import torch

import ctc_score_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------ the yardstick
def _words(tokens, post_process):
    """words as lists of symbols, restated from the issue's rules and not from dictionary.string(): tokens the dictionary omits
    (<s>, <pad>, </s>) vanish, then `|` separates under "letter"; under None every remaining token is a word"""
    d = K.dictionary()
    syms = [d.symbols[t] for t in tokens if t not in (K.BLANK, K.PAD, K.EOS)]
    if post_process is None:
        return syms
    out, cur = [], []
    for s in syms + ["|"]:
        if s == "|":
            if cur:
                out.append("".join(cur))
            cur = []
        else:
            cur.append(s)
    return out


@pytest.mark.parametrize("post_process", ["letter", None])
@pytest.mark.parametrize("name", ["small", "words", "per4_64"])
def test_host_path_equals_a_full_matrix_levenshtein(name, post_process):
    from unispeech_amd.ctc import error_counts
    logits, il, targets, hyps = K.batch(name)
    counts, decoded = K.host_counts(name, post_process)
    assert decoded == [h if n else [] for h, n in zip(hyps, il)]
    for b, pred in enumerate(decoded):
        targ = [int(v) for v in targets[b] if int(v) not in (K.PAD, K.EOS)]
        pw, tw = _words(pred, post_process), _words(targ, post_process)
        want = [K.levenshtein(pred, targ), len(targ), K.levenshtein(pw, tw), len(tw)]
        assert counts[b].tolist() == want, (name, b, counts[b].tolist(), want)
    total = error_counts(logits, il, targets, K.dictionary(), post_process)
    c_err, c_len, w_err, w_len = (int(v) for v in counts.sum(0))
    assert total == {"c_errors": c_err, "c_total": c_len, "w_errors": w_err, "wv_errors": w_err, "w_total": w_len}


def test_word_rules_hand_counted():
    counts, _ = K.host_counts("words", "letter")
    #                  c_err c_len w_err w_len
    assert counts.tolist() == [[0, 12, 0, 3],      # identical
                               [1, 9, 1, 1],       # one word each, one letter apart
                               [1, 2, 0, 0],       # separators only: no words on either side
                               [3, 4, 0, 2],       # |A||BC| against A|BC: the same two words
                               [1, 9, 1, 2],       # ABCE against ABCD
                               [3, 8, 1, 3],       # A<pad>B</s>C is the word ABC; D<unk>E is not DE
                               [0, 5, 0, 2],       # pad and eos inside the target row are dropped
                               [1, 5, 1, 2]]       # C`e` against CD, `e` beyond the head's classes


def test_cpu_logits_take_the_host_path_without_the_library(monkeypatch):
    from unispeech_amd import _lib, ctc

    def no_library():
        raise AssertionError("host logits must not load the library")
    monkeypatch.setattr(_lib, "lib", no_library)
    logits, il, targets, _ = K.batch("small")
    out = ctc.error_counts(logits, il, targets, K.dictionary())
    assert out["c_total"] == int(K.host_counts("small", "letter")[0][:, 1].sum())
    with pytest.raises(NotImplementedError, match="post_process"):
        ctc.error_counts(logits, il, targets, K.dictionary(), "wordpiece")
    with pytest.raises(ValueError, match="targets"):
        ctc.error_counts(logits, il, targets[:3], K.dictionary())


def test_criterion_eval_goes_through_error_counts(monkeypatch):
    """the logging output keeps its keys and values; the table is built once per (C, device) and only for device logits"""
    from unispeech_amd import ctc
    logits, _, targets, _ = K.batch("small")

    class Stub(torch.nn.Module):
        def forward(self, **kw):
            return {"encoder_out": logits, "padding_mask": None}

    crit = ctc.CtcCriterion(K.dictionary(), zero_infinity=True)
    sample = {"id": torch.arange(8), "target": targets, "net_input": {"source": None}}
    seen = []
    real = ctc.error_counts
    monkeypatch.setattr(ctc, "error_counts", lambda *a, **k: seen.append(k) or real(*a, **k))
    _, _, log = crit(Stub().eval(), sample)
    counts, _ = ctc.sample_error_counts(logits, None, targets, K.dictionary())      # every frame: the model gave no lengths
    assert (log["c_errors"], log["c_total"], log["w_errors"], log["w_total"]) == tuple(int(v) for v in counts.sum(0))
    assert log["wv_errors"] == log["w_errors"] and len(seen) == 1 and seen[0]["classes"] is None
    assert "c_errors" not in crit(Stub().train(), sample)[2] and len(seen) == 1
    tab = crit._classes(K.C, torch.device("cpu"))
    assert tab is crit._classes(K.C, torch.device("cpu")) and tab.dtype == torch.uint8 and tab.numel() == K.C


# --------------------------------------------------------------------------------------------------------------- the table
def test_word_classes():
    from unispeech_amd.ctc import DROP, LETTER, SEP, LetterDictionary, _IndexDictionary, word_classes
    assert (DROP, SEP, LETTER) == (0, 1, 2)
    d = K.dictionary()
    tab = word_classes(d, K.C, "letter")
    assert tab.dtype == np.uint8 and tab.shape == (K.C,)
    assert tab.tolist() == [DROP, DROP, DROP, LETTER, SEP] + [LETTER] * 27          # <unk> is a letter, `|` the separator
    none = word_classes(d, K.C, None)
    assert none.tolist() == [DROP, DROP, DROP] + [LETTER] * 29                      # `|` an ordinary token
    assert word_classes(d, K.C, "none").tolist() == none.tolist()
    assert word_classes(d, len(d), "letter").tolist() == tab.tolist() + [LETTER] * 8
    idx = _IndexDictionary(0, 1, 2)
    assert word_classes(idx, 12, "letter") is None                                  # "1" is a prefix of "10": not prefix-free
    assert word_classes(idx, 12, None).tolist() == [LETTER] * 12                    # string() omits nothing there
    assert word_classes(LetterDictionary(["|", "A", "B C"]), 7, "letter") is None   # a space in a symbol
    assert word_classes(LetterDictionary(["|", "A", "B C"]), 7, None) is None
    assert word_classes(LetterDictionary(["|", "A", "B|"]), 7, "letter") is None    # a `|` in a symbol
    assert word_classes(LetterDictionary(["|", "A", "<"]), 7, "letter") is None     # "<" is a prefix of "<unk>"
    assert word_classes(LetterDictionary(["|", "A", "<"]), 7, None) is not None     # no concatenation: distinct is enough
    assert word_classes(LetterDictionary(["|", "A", "A"]), 7, None) is None         # two ids, one string
    assert word_classes(LetterDictionary(["|", "A", "AB"]), 7, "letter") is None
    assert word_classes(LetterDictionary(["|", "A"]), 9, "letter") is None          # probing class 6 raises
    assert word_classes(LetterDictionary(["A", "|"]), 5, "letter") is None          # `|` beyond the head: an id >= C is a LETTER
    assert word_classes(d, K.C, "wordpiece") is None

    class Other:                                                                    # not a dictionary this package knows
        def string(self, tokens):
            return " ".join("x%d" % t for t in tokens)
    assert word_classes(Other(), 4, None) is None

    class Sub(LetterDictionary):
        pass
    assert word_classes(Sub(["|", "A"]), 6, "letter") is None


# --------------------------------------------------------------------------------------------------- the library, no GPU
NEW = ("wavlm_ctc_score_supported", "wavlm_ctc_score_workspace_bytes", "wavlm_ctc_score")


def test_abi_stays_30_and_the_new_symbols_are_declared_exported_and_bound():
    import ctypes
    from unispeech_amd import _lib, build
    src = open(os.path.join(ROOT, "include", "wavlm_hip.h")).read()
    assert int(re.search(r"#define WAVLM_HIP_ABI_VERSION (\d+)", src).group(1)) == 30 == _lib.ABI_VERSION
    assert "ctc_score.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "ctc_score.hip"))
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    if not os.path.exists(_lib.LIB_PATH):
        build.build_library(verbose=False)
    h = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        decl = re.search(r"\b%s\(([^;]*)\);" % name, code).group(1)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[name][1]), name
        assert hasattr(h, name), name
    assert _lib.lib().wavlm_abi_version() == 30


def test_supported_and_workspace_are_host_functions():
    from unispeech_amd import _lib, ops
    L = _lib.lib()
    for T in (1, 2, 255, 256, 749, 100000):
        for Lt in (0, 1, 64, 256, 257, 1023):
            assert L.wavlm_ctc_score_supported(T, Lt) == 1, (T, Lt)
    assert L.wavlm_ctc_score_supported(0, 10) == 0 and L.wavlm_ctc_score_supported(-1, 10) == 0
    assert L.wavlm_ctc_score_supported(10, -1) == 0 and L.wavlm_ctc_score_supported(10, 1 << 20) == 0
    assert ops.ctc_score_supported(749, 250) is True and ops.ctc_score_supported(0, 250) is False
    ws = L.wavlm_ctc_score_workspace_bytes
    B, T, Lt = 32, 749, 250
    assert ws(B, T, Lt) >= B * (5 * Lt + 4 * T) * 4                   # the word streams and span tables of both sides
    assert ws(B, T, Lt) < B * (5 * Lt + 4 * T) * 4 + 256
    assert ws(0, T, Lt) == 0 and ws(-1, T, Lt) == 0 and ws(B, -1, Lt) == 0 and ws(B, T, -1) == 0
    assert ws(2 * B, T, Lt) > ws(B, T, Lt) and ws(B, 2 * T, Lt) > ws(B, T, Lt) and ws(B, T, 2 * Lt) > ws(B, T, Lt)
    assert all(ws(B, T, n + 1) >= ws(B, T, n) for n in range(0, 1023, 37))      # monotonic in each argument
    assert all(ws(B, n + 1, Lt) >= ws(B, n, Lt) for n in range(1, 2000, 97))
    assert all(ws(n + 1, T, Lt) >= ws(n, T, Lt) for n in range(0, 40, 3))


# ------------------------------------------------------------------------------------------------------ the score command
def test_score_arguments():
    from unispeech_amd import ctc
    a = ctc.parse_args(["score", "ck.pt", "dict.ltr.txt", "test.tsv", "test.ltr"])
    assert (a.cmd, a.ckpt, a.dict, a.manifest, a.labels) == ("score", "ck.pt", "dict.ltr.txt", "test.tsv", "test.ltr")
    assert (a.batch_seconds, a.post_process, a.bf16, a.results) == (160.0, "letter", False, None)
    a = ctc.parse_args(["score", "c", "d", "m", "l", "--batch-seconds", "30", "--post-process", "none", "--bf16", "--results", "out"])
    assert (a.batch_seconds, a.post_process, a.bf16, a.results) == (30.0, "none", True, "out")
    with pytest.raises(SystemExit):
        ctc.parse_args(["score", "ck.pt", "dict.ltr.txt", "test.tsv"])
    with pytest.raises(SystemExit):
        ctc.parse_args(["score", "c", "d", "m", "l", "--post-process", "wordpiece"])
    assert ctc.parse_args(["decode", "ck.pt", "dict.ltr.txt", "a.wav"]).cmd == "decode"           # unchanged


def test_manifest_labels_and_batches(tmp_path):
    from unispeech_amd import ctc
    (tmp_path / "t.tsv").write_text("/data/root\na/1.wav\t16000\nb/2.flac\t8000\n\nc.wav\t24000\n")
    entries = ctc.read_manifest(str(tmp_path / "t.tsv"))
    assert entries == [(os.path.join("/data/root", "a/1.wav"), 16000), (os.path.join("/data/root", "b/2.flac"), 8000),
                       (os.path.join("/data/root", "c.wav"), 24000)]
    (tmp_path / "bad.tsv").write_text("/data/root\na/1.wav 16000\n")
    with pytest.raises(ValueError, match=r"bad\.tsv:2"):
        ctc.read_manifest(str(tmp_path / "bad.tsv"))
    (tmp_path / "empty.tsv").write_text("")
    with pytest.raises(ValueError, match="empty manifest"):
        ctc.read_manifest(str(tmp_path / "empty.tsv"))
    d = K.dictionary()
    (tmp_path / "t.ltr").write_text("T H E | C A T |\n\nA ~ B |\n")
    labels = ctc.read_labels(str(tmp_path / "t.ltr"), d, 3)
    assert labels == [K.ids("THE|CAT|"), [], [d.index("A"), K.UNK, d.index("B"), K.BAR]]       # a symbol it lacks: <unk>
    with pytest.raises(ValueError, match=r"t\.ltr: 3 label lines, but the manifest lists 2 utterances"):
        ctc.read_labels(str(tmp_path / "t.ltr"), d, 2)
    # by length, ascending; a batch's padded size is its longest utterance times its count
    sizes = [16000, 8000, 24000, 8000, 100000]
    assert ctc.length_batches(sizes, 48000) == [[1, 3, 0], [2], [4]]
    assert ctc.length_batches(sizes, 10 ** 9) == [[1, 3, 0, 2, 4]]
    assert ctc.length_batches([], 48000) == []
    assert sorted(i for b in ctc.length_batches(sizes, 1) for i in b) == [0, 1, 2, 3, 4]       # each its own batch
