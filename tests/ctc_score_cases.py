"""Shared inputs of tests/test_ctc_score.py and tests/test_ctc_score_gpu.py: batches whose greedy decode is known by construction.

C = 32 classes: <s> = 0 (the blank), <pad> = 1, </s> = 2, <unk> = 3, `|` = 4, A .. Z = 5 .. 30, ' = 31.  The dictionary goes on with
a .. h = 32 .. 39, symbols the head has no class for: a target may still name them (an id >= C: a LETTER compared by value).

A batch is (logits fp32 [T, B, C], input lengths [B], targets int64 [B, Lt] padded with </s> and <pad>, the decodes the logits
were built for).  Frame t of sample b is noise in [-1, 1] with +8 on the class of the path: a token per frame, a blank between two
equal tokens, blanks to the input length; frames behind the input length carry other tokens, which no decode may see.  The margin
survives the rounding to bf16, so both dtypes decode alike.

batch       B  T    Lt    what it pins
small       8  12   10    (0, 0) (0, 5) (5, 0), (1, 1) equal and different, input length 0 and one below T
words       8  40   20    the word rules: see WORDS below
per4_H      8  *    256   targets of 63 64 65 127 128 129 255 256 tokens against a decode of H tokens: 4 columns per lane, the last
                          lane's last column and every lane-run boundary below it
per16_H     8  *    1023  targets of 63 64 65 127 128 129 257 1023: 16 columns per lane, one past the 4-column kernel's limit
cap         2  70   1024  the cap itself: 1024 and 1009 (63 lanes + 1 column) tokens
H in 1, 64, 65, 300 with T = 255, 256, 257, 640: the decode's 256-frame chunk, one below, one above, and three chunks."""
import functools

import numpy as np
import torch

C = 32
BLANK, PAD, EOS, UNK, BAR = 0, 1, 2, 3, 4
EXTRA = 36                                            # `e`: in the dictionary, beyond the head's classes
HYP_T = {1: 255, 64: 256, 65: 257, 300: 640}


def dictionary():
    from unispeech_amd.ctc import LetterDictionary
    return LetterDictionary(["|"] + [chr(ord("A") + i) for i in range(26)] + ["'"] + [chr(ord("a") + i) for i in range(8)])


def ids(text):
    """'AB|C' -> token ids; `_` = <pad>, `.` = </s>, `?` = <unk>"""
    d = dictionary()
    special = {"_": PAD, ".": EOS, "?": UNK}
    return [special[ch] if ch in special else d.index(ch) for ch in text]


# (decode, target row before padding)
WORDS = [
    ("THE|CAT|SAT|", "THE|CAT|SAT|"),                 # identical: 0 / 0
    ("HELLOWORLD", "HELLOWORD"),                      # no separator at all: one word each
    ("|||", "||"),                                    # only separators: no words
    ("|A||BC|", "A|BC"),                              # leading, trailing, doubled `|`: no empty words
    ("ABCD|ABCE", "ABCD|ABCD"),                       # two words of equal length that differ in the last token
    ("A_B.C|D?E|F", "ABC|DE|F"),                      # pad, eos inside a word: dropped, the word is ABC; unk is a letter
    ("AB|CD", "A_B|.C_D"),                            # pad and eos in the middle of the target row
    ("AB|CD", "AB|Ce"),                               # a target id >= C
]


def _sentence(rng, n):
    out = []
    while len(out) < n:
        out += [int(v) for v in rng.integers(5, C, rng.integers(1, 8))] + [BAR]
    return out[:n]


def _mutate(rng, seq, n):
    """`seq` with every tenth token or so substituted, dropped or doubled, cut or padded to n tokens"""
    out = []
    for v in seq:
        r = rng.random()
        if r < 0.04:
            continue
        out.append(int(rng.integers(4, C)) if r < 0.08 else v)
        if r > 0.96:
            out.append(int(rng.integers(4, C)))
    out += _sentence(rng, n)
    return out[:n]


def _pad_rows(rows, Lt):
    t = torch.full((len(rows), Lt), PAD, dtype=torch.long)
    for b, r in enumerate(rows):
        assert len(r) <= Lt
        t[b, :len(r)] = torch.tensor(r, dtype=torch.long)
        if len(r) < Lt:
            t[b, len(r)] = EOS
    return t


def logits_for(hyps, T, il, seed):
    B = len(hyps)
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1.0, 1.0, (T, B, C)).astype(np.float32)
    for b, h in enumerate(hyps):
        path = []
        for i, v in enumerate(h):
            path.append(v)
            if i + 1 < len(h) and h[i + 1] == v:
                path.append(BLANK)
        assert len(path) <= il[b] <= T, (len(path), il[b], T)
        path += [BLANK] * (il[b] - len(path))
        path += [int(v) for v in rng.integers(1, C, T - il[b])]
        x[np.arange(T), b, path] += 8.0
    return torch.from_numpy(x)


@functools.lru_cache(maxsize=None)
def batch(name):
    """(logits, input lengths, targets, decodes) -- treat as read-only"""
    if name == "small":
        T = 12
        hyps = [[], [], ids("AB|CD"), ids("A"), ids("A"), [], ids("AB|C"), ids("HELLO|YOU")]
        rows = [[], ids("AB|CD"), [], ids("A"), ids("B"), ids("AB"), ids("AB|D"), ids("HELLO|YOU")]
        il = [T, T, T, T, T, 0, T - 1, T]
        return logits_for(hyps, T, il, 1), il, _pad_rows(rows, 10), hyps
    if name == "words":
        hyps = [ids(h) for h, _ in WORDS]
        rows = [ids(t) for _, t in WORDS]
        return logits_for(hyps, 40, [40] * 8, 2), [40] * 8, _pad_rows(rows, 20), hyps
    if name == "cap":
        rng = np.random.default_rng(3)
        rows = [_sentence(rng, 1024), _sentence(rng, 1009)]
        hyps = [_mutate(rng, rows[0][500:], 33), _mutate(rng, rows[1], 30)]
        return logits_for(hyps, 70, [70, 70], 4), [70, 70], _pad_rows(rows, 1024), hyps
    kind, H = name.split("_")
    H = int(H)
    T = HYP_T[H]
    lens, Lt = {"per4": ((63, 64, 65, 127, 128, 129, 255, 256), 256), "per16": ((63, 64, 65, 127, 128, 129, 257, 1023), 1023)}[kind]
    rng = np.random.default_rng(100 * H + Lt)
    rows, hyps = [], []
    for n in lens:
        base = _sentence(rng, max(n, H))
        rows.append(base[:n])
        hyps.append(_mutate(rng, base, H))
    il = [T] * 8
    il[3] = T - 7
    return logits_for(hyps, T, il, H + Lt), il, _pad_rows(rows, Lt), hyps


LONG = ["%s_%d" % (k, h) for k in ("per4", "per16") for h in (1, 64, 65, 300)]
ALL = ["small", "words", "cap"] + LONG


def levenshtein(a, b):
    """the full (len(a) + 1) x (len(b) + 1) matrix, no rolling rows: the yardstick's yardstick"""
    D = np.zeros((len(a) + 1, len(b) + 1), dtype=np.int64)
    D[:, 0] = np.arange(len(a) + 1)
    D[0, :] = np.arange(len(b) + 1)
    for i in range(1, len(a) + 1):
        for j in range(1, len(b) + 1):
            D[i, j] = min(D[i - 1, j] + 1, D[i, j - 1] + 1, D[i - 1, j - 1] + (a[i - 1] != b[j - 1]))
    return int(D[len(a), len(b)])


@functools.lru_cache(maxsize=None)
def host_counts(name, post_process):
    """[B, 4] of the host path of sample_error_counts on the batch's fp32 logits, computed once per process"""
    from unispeech_amd.ctc import sample_error_counts
    logits, il, targets, _ = batch(name)
    counts, decoded = sample_error_counts(logits, il, targets, dictionary(), post_process)
    counts.setflags(write=False)
    return counts, decoded
