"""CTC forced alignment without a GPU: forced_align_reference against brute force over every frame path (paths ==, the tie rule
included), its invariants on random cases, the time stamps, the word segments and the CTM text on constructed examples, the
command line, and the ABI bookkeeping.  The inputs are in tests/ctc_align_cases.py."""
import math
import os
import re

import numpy as np
import pytest
import torch

import ctc_align_cases as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ref(x, labels, il=None):
    from unispeech_amd.ctc_align import forced_align_reference
    x = np.asarray(x)
    if x.ndim == 2:
        x, labels = x[:, None], [labels]
    flat = np.array([v for lab in labels for v in lab], dtype=np.int64)
    return forced_align_reference(x, flat, il, [len(lab) for lab in labels], 0)


# ------------------------------------------------------------------------------------------------------- brute force
@pytest.mark.parametrize("integer", [True, False], ids=["integer_ties", "float"])
def test_reference_equals_exhaustive_enumeration(integer):
    feasible = infeasible = tied = 0
    for T, labels in A.grid():
        for seed in range(6 if integer else 2):
            x = A.grid_logits(T, 100 * T + seed, integer)
            got = _ref(x, labels)
            want = A.brute_force(x, labels)
            L = len(labels)
            if want is None:
                infeasible += 1
                assert T < A.tight(labels)
                assert got.score[0] == -math.inf and np.all(got.frames == -2) and np.all(got.spans == -1)
                assert np.all(got.token_scores == 0)
                continue
            feasible += 1
            states, classes = want
            frames, spans, tok, total = A.path_outputs(x, states, classes, L)
            assert got.frames[0].tolist() == frames, (T, labels, seed)
            assert got.spans[0].tolist() == spans, (T, labels, seed)
            assert abs(got.score[0] - total) <= 1e-12 and np.allclose(got.token_scores[0], tok, rtol=0, atol=1e-12)
            if integer and T >= 2:
                tied += 1
    assert feasible >= 100 and infeasible >= 40 and (tied > 300 or not integer)


def test_the_tie_rule_on_all_equal_logits():
    """every path ties: the greatest state sequence read from the end -- the trailing blank for as long as it can be held"""
    got = _ref(np.zeros((6, 3)), [1, 2])
    assert got.frames[0].tolist() == [0, 1, -1, -1, -1, -1]          # states 1 3 4 4 4 4: S - 1 at the end, and it stays there
    got = _ref(np.zeros((3, 3)), [1, 1])
    assert got.frames[0].tolist() == [0, -1, 1]
    got = _ref(np.zeros((2, 3)), [1])
    assert got.frames[0].tolist() == [0, -1] and got.spans[0].tolist() == [[0, 1]]


# ---------------------------------------------------------------------------------------------------------- invariants
def test_invariants_on_random_cases():
    rng = np.random.RandomState(3)
    for trial in range(40):
        T, B, C = int(rng.randint(1, 40)), int(rng.randint(1, 4)), int(rng.randint(2, 9))
        labels = [[int(v) for v in rng.randint(1, C, size=rng.randint(0, 12))] for _ in range(B)]
        il = [int(rng.randint(0, T + 1)) for _ in range(B)]
        x = rng.randn(T, B, C).astype(np.float32)
        for b, n in enumerate(il):
            x[n:, b] = np.nan                                          # never read
        got = _ref(x, labels, il)
        shifted = _ref(x.astype(np.float64) + rng.randint(-8, 9, size=(T, 1, 1)), labels, il)     # a constant per frame
        assert np.array_equal(shifted.frames, got.frames)
        for b in range(B):
            L, Tb = len(labels[b]), il[b]
            if Tb < A.tight(labels[b]) or (Tb == 0 and L > 0):
                assert got.score[b] == -math.inf and np.all(got.frames[b] == -2) and np.all(got.spans[b] == -1)
                continue
            if Tb == 0:
                assert got.score[b] == 0.0
                continue
            f = got.frames[b]
            assert np.all(f[Tb:] == -2) and np.all(f[:Tb] >= -1)
            nb = f[:Tb][f[:Tb] >= 0]
            assert np.all(np.diff(nb) >= 0) and sorted(set(nb.tolist())) == list(range(L))       # every label, in order
            cover = np.full(Tb, -1)
            for j in range(L):
                s0, s1 = got.spans[b, j]
                assert 0 <= s0 < s1 <= Tb and np.all(cover[s0:s1] == -1)
                cover[s0:s1] = j
            assert np.array_equal(cover, f[:Tb])                                                  # spans tile the label frames
            assert np.all(got.spans[b, L:] == -1) and np.all(got.token_scores[b, L:] == 0)
            xb = x[:Tb, b].astype(np.float64)
            lp = xb - (xb.max(-1, keepdims=True) + np.log(np.exp(xb - xb.max(-1, keepdims=True)).sum(-1, keepdims=True)))
            cls = [labels[b][j] if j >= 0 else 0 for j in f[:Tb]]
            per_frame = lp[np.arange(Tb), cls]
            assert abs(got.score[b] - per_frame.sum()) <= 1e-10
            for j in range(L):
                assert abs(got.token_scores[b, j] - per_frame[f[:Tb] == j].sum()) <= 1e-10


def test_out_of_range_labels_and_host_tensors():
    x = torch.randn(5, 2, 4)
    got = _ref(x.numpy(), [[1, 4], [2]])
    assert math.isnan(got.score[0]) and np.all(got.frames[0] == -2) and np.all(got.spans[0] == -1)
    assert math.isfinite(got.score[1])
    from unispeech_amd.ctc_align import forced_align_reference
    padded = forced_align_reference(x.to(torch.bfloat16), torch.tensor([[1, 3], [2, 0]]), torch.tensor([5, 4]), [2, 1], 0)
    flat = forced_align_reference(x.to(torch.bfloat16).float().numpy(), [1, 3, 2], [5, 4], [2, 1], 0)
    assert all(np.array_equal(p, f) for p, f in zip(padded, flat))


def test_forced_align_has_no_cpu_fallback():
    from unispeech_amd import _lib
    from unispeech_amd.ctc_align import forced_align
    with pytest.raises(_lib.WavlmHipError, match="no CPU fallback"):
        forced_align(torch.zeros(3, 1, 4), [1], None, [1])


# --------------------------------------------------------------------------------------------------------- time stamps
def test_timesteps_of_a_hand_written_path():
    from unispeech_amd.ctc_align import frame_tokens, get_timesteps, timesteps
    blank = 0
    path = [0, 3, 3, 0, 3, 5, 5, 0, 0, 2]                              # per-frame classes: 3 _ 3 5 2
    assert get_timesteps(path, blank) == [1, 4, 5, 9]                  # w2l_decoder.py:256-262 by hand
    x = np.full((len(path), 1, 6), -5.0, dtype=np.float32)
    x[np.arange(len(path)), 0, path] = 5.0                             # the path is the only good one
    hyp = [3, 3, 5, 2]
    assert timesteps(x, None, [hyp], blank) == [get_timesteps(path, blank)]
    got = _ref(x, [hyp])
    assert frame_tokens(got.frames[0], hyp, blank) == path
    # two samples, one of them without an alignment, and an empty hypothesis
    x2 = np.concatenate([x, x], 1)
    assert timesteps(torch.from_numpy(x2), [10, 3], [hyp, hyp], blank) == [[1, 4, 5, 9], None]
    assert timesteps(x2, None, [[], [3]], blank) == [[], [1]]


# -------------------------------------------------------------------------------------------------- words and the CTM
def _dictionary():
    from unispeech_amd.ctc import LetterDictionary
    return LetterDictionary(["|", "A", "B", "C"])                      # ids 4 .. 7


def test_word_segments_and_ctm_text():
    from unispeech_amd.ctc_align import ctm_lines, frame_stride, word_segments
    d = _dictionary()
    stride = frame_stride("[(512,10,5)] + [(512,3,2)] * 4 + [(512,2,2)] * 2")
    assert stride == 320 and frame_stride([(8, 3, 2), (8, 2, 3)]) == 6
    tokens = [5, 6, 4, 2, 7, 4]                                        # A B | </s> C |   (</s> is dropped by string())
    spans = [[2, 4], [5, 6], [6, 7], [7, 8], [10, 13], [13, 14]]
    scores = [-0.5, -0.25, -0.125, -9.0, -1.5, -0.0625]
    segs = word_segments(tokens, spans, scores, d, stride)
    assert [(s.word, s.start_frame, s.end_frame, s.score) for s in segs] == [("AB", 2, 6, -0.75), ("C", 10, 13, -1.5)]
    assert segs[0].start == 2 * 320 / 16000 and segs[0].end == 6 * 320 / 16000
    assert segs[0].confidence == math.exp(-0.75 / 3) and segs[1].confidence == math.exp(-1.5 / 3)
    assert ctm_lines("utt1", segs) == ["utt1 1 0.040 0.080 AB %.4f" % math.exp(-0.25), "utt1 1 0.200 0.060 C %.4f" % math.exp(-0.5)]
    toks = word_segments(tokens, spans, scores, d, stride, each_token=True)
    assert [(s.word, s.start_frame, s.end_frame) for s in toks] == [("A", 2, 4), ("B", 5, 6), ("|", 6, 7), ("C", 10, 13), ("|", 13, 14)]
    with pytest.raises(ValueError, match="no span"):
        word_segments([5], [[-1, -1]], [0.0], d, stride)
    # through the reference: the words of an aligned transcript tile its label frames
    path = [0, 5, 5, 6, 0, 4, 7, 7, 0]
    x = np.full((len(path), 1, len(d)), -4.0, dtype=np.float32)
    x[np.arange(len(path)), 0, path] = 4.0
    got = _ref(x, [[5, 6, 4, 7]])
    segs = word_segments([5, 6, 4, 7], got.spans[0], got.token_scores[0], d, stride)
    assert [(s.word, s.start_frame, s.end_frame) for s in segs] == [("AB", 1, 4), ("C", 6, 8)]
    assert all(0.0 < s.confidence <= 1.0 for s in segs)


def test_command_line():
    from unispeech_amd import ctc_align
    a = ctc_align.parse_args(["ck.pt", "dict.txt", "m.tsv", "l.ltr"])
    assert (a.ckpt, a.dict, a.manifest, a.labels, a.out, a.tokens, a.max_samples) == \
        ("ck.pt", "dict.txt", "m.tsv", "l.ltr", None, False, 160 * 16000)
    a = ctc_align.parse_args(["ck.pt", "dict.txt", "m.tsv", "l.ltr", "--out", "x.ctm", "--tokens", "--max-samples", "32000"])
    assert (a.out, a.tokens, a.max_samples) == ("x.ctm", True, 32000)
    with pytest.raises(SystemExit):
        ctc_align.parse_args(["ck.pt", "dict.txt", "m.tsv"])
    with pytest.raises(SystemExit):
        ctc_align.parse_args(["ck.pt", "dict.txt", "m.tsv", "l.ltr", "--lm", "x.arpa"])


# --------------------------------------------------------------------------------------------------- the library, no GPU
NEW = ("wavlm_ctc_align_supported", "wavlm_ctc_align_workspace_bytes", "wavlm_ctc_align")


def test_abi_stays_30_and_the_new_symbols_are_declared_exported_and_bound():
    import ctypes
    from unispeech_amd import _lib, build, ctc_align
    src = open(os.path.join(ROOT, "include", "wavlm_hip.h")).read()
    assert int(re.search(r"#define WAVLM_HIP_ABI_VERSION (\d+)", src).group(1)) == 30 == _lib.ABI_VERSION
    assert int(re.search(r"#define WAVLM_CTC_ALIGN_BLOCK (\d+)", src).group(1)) == ctc_align.ALIGN_BLOCK
    assert "ctc_align.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "ctc_align.hip"))
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
    lib = _lib.lib()
    ok = lib.wavlm_ctc_align_supported
    assert ok(0) and ok(1) and ok(1023) and not ok(1024) and not ok(-1)
    need = lib.wavlm_ctc_align_workspace_bytes
    assert need(-1, 1, 1) == 0 and need(1, 1, 0) > 0
    # the back-pointers are 2 bits per (b, t, s), in 16-byte groups of 64 positions
    assert need(4, 100, 1023) - need(4, 100, 0) == 4 * 100 * (32 - 1) * 16
    assert need(32, 749, 100) < 32 * 749 * (201 * 4)                   # far below an int32 per (b, t, s)
    ops.ctc_align_check_supported(1023)
    with pytest.raises(NotImplementedError, match=r"L = 1024\b"):
        ops.ctc_align_check_supported(1024)
    # every NULL pointer, a bad view and a short workspace are refused before anything is launched
    import ctypes
    buf = ctypes.create_string_buffer(1 << 16)
    p = ctypes.cast(buf, ctypes.c_void_p)
    base = [p, 0, 40, 4, 2, 10, 4, p, p, 3, 2, p, 0, p, p, p, p, p, 1 << 16, None]
    assert need(2, 10, 2) <= 1 << 16

    def call(**kw):
        names = ["logits", "dtype", "sb", "st", "B", "T", "C", "targets", "offsets", "n", "Lmax", "il", "blank", "frames",
                 "spans", "tok", "score", "ws", "ws_bytes", "stream"]
        args = list(base)
        for k, v in kw.items():
            args[names.index(k)] = v
        return lib.wavlm_ctc_align(*args)

    for name in ("logits", "targets", "offsets", "il", "frames", "spans", "tok", "score", "ws"):
        assert call(**{name: None}) == -1, name
    assert call(Lmax=1024) == -1 and call(dtype=2) == -1 and call(blank=4) == -1 and call(blank=-1) == -1 and call(C=0) == -1
    assert call(sb=39) == -1 and call(st=3) == -1                      # the view overlaps itself
    assert call(ws_bytes=need(2, 10, 2) - 1) == -1
    assert call(B=0) == 0                                              # nothing to do: nothing is launched
