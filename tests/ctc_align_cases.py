"""Inputs shared by tests/test_ctc_align.py (host) and tests/test_ctc_align_gpu.py (device): the brute force over every frame path
that forced_align_reference is held against, the random and the constructed cases, and the comparison of a device result with
the float64 reference (paths ==, scores within one fp32 rounding)."""
import functools
import itertools
import math

import numpy as np
import torch

C = 32                # classes of the device cases; class 0 is the blank
BOUND = 2.0 ** -22    # |device - float64 reference| <= BOUND * max(1, |reference|): one fp32 rounding (2^-24 relative) plus the
#                       float64 log-sum-exp's error (1e-14 relative), with a 4x margin


# ------------------------------------------------------------------------------------------------------------ brute force
def brute_force(x, labels, blank=0):
    """x [T, C] float64, T >= 1: every CTC path of `labels` through all T frames, its value the raw logits added left to right.
    Returns (the best path's states, its classes), ties to the path whose states read from the last frame to the first are
    lexicographically greatest, or None without a path."""
    T = x.shape[0]
    ext = [blank]
    for v in labels:
        ext += [v, blank]
    S = len(ext)
    best = None
    for p in itertools.product(range(S), repeat=T):
        if p[0] > 1 or p[-1] < S - 2:
            continue
        ok = True
        for a, b in zip(p, p[1:]):
            d = b - a
            if d not in (0, 1) and not (d == 2 and b % 2 == 1 and ext[b] != ext[b - 2]):
                ok = False
                break
        if not ok:
            continue
        val = float(x[0, ext[p[0]]])
        for t in range(1, T):
            val = val + float(x[t, ext[p[t]]])
        key = (val, p[::-1])
        if best is None or key > best:
            best = key
    if best is None:
        return None
    states = best[1][::-1]
    return list(states), [ext[s] for s in states]


def path_outputs(x, states, classes, L):
    """(frames, spans, token scores, score) of a state path through x [T, C]: log-probabilities added in ascending t"""
    lp = x - np.log(np.exp(x - x.max(-1, keepdims=True)).sum(-1, keepdims=True)) - x.max(-1, keepdims=True)
    frames = [(s >> 1) if s & 1 else -1 for s in states]
    spans = [[-1, -1] for _ in range(L)]
    tok = [0.0] * L
    total = 0.0
    for t, (s, c) in enumerate(zip(states, classes)):
        total += float(lp[t, c])
        if s & 1:
            j = s >> 1
            if spans[j][0] < 0:
                spans[j][0] = t
            spans[j][1] = t + 1
            tok[j] += float(lp[t, c])
    return frames, spans, tok, total


def grid():
    """(T, labels) for every T <= 6 and every label sequence over {1, 2} with L <= 3 (C = 3): repeats and infeasible cases included"""
    for T in range(1, 7):
        for L in range(0, 4):
            for labels in itertools.product((1, 2), repeat=L):
                yield T, list(labels)


def grid_logits(T, seed, integer):
    rng = np.random.RandomState(seed)
    if integer:
        return rng.randint(-1, 2, size=(T, 3)).astype(np.float64)
    return rng.randn(T, 3).astype(np.float32).astype(np.float64)


# ------------------------------------------------------------------------------------------------------------ device cases
def labels_of(L, rng, repeats=True):
    """L labels in [1, C); with repeats roughly one adjacent pair in sixteen is equal"""
    lab = rng.randint(1, C, size=L)
    if repeats and L > 1:
        same = rng.rand(L) < 1.0 / 16
        for j in range(1, L):
            if same[j]:
                lab[j] = lab[j - 1]
    return [int(v) for v in lab]


def tight(labels):
    """the fewest frames that align `labels`: L + the number of adjacent equal pairs"""
    return len(labels) + sum(1 for a, b in zip(labels, labels[1:]) if a == b)


SIZES = (0, 1, 127, 128, 255, 256, 511, 512, 1023)     # S = 2 L + 1 on both sides of every PER boundary, and the cap


@functools.lru_cache(maxsize=None)
def size_case(L, kind):
    """(x [T, B, C] fp32, labels, input lengths).  kind "tight": every sample has exactly the frames its labels need, so one
    path; "loose": T is about 2 L.  B = 2 (other labels in the second sample) except at L = 1023, which is one sample."""
    rng = np.random.RandomState(1000 + L + (7 if kind == "tight" else 0))
    B = 1 if L == 1023 else 2
    labels = [labels_of(L, rng) for _ in range(B)]
    if kind == "tight":
        il = [max(tight(lab), 1) for lab in labels]
    else:
        il = [tight(labels[0]) + 40] if L == 1023 else [2 * L + 3, 2 * L + 1]
    T = max(il)
    x = torch.from_numpy(rng.randn(T, B, C).astype(np.float32))
    return x, labels, il


@functools.lru_cache(maxsize=None)
def block_case(block):
    """input lengths one below the back-trace's staging block, at it, one above and two blocks + 1; NaN behind every length"""
    rng = np.random.RandomState(77)
    il = [block - 1, block, block + 1, 2 * block + 1]
    labels = [labels_of(n, rng) for n in (5, 9, 12, 20)]
    x = torch.from_numpy(rng.randn(max(il), 4, C).astype(np.float32))
    for b, n in enumerate(il):
        x[n:, b] = float("nan")
    return x, labels, il


@functools.lru_cache(maxsize=None)
def special_case():
    """all-equal labels with exactly enough frames (2 L - 1) and with one too few; input length 0 with and without labels; a
    length shorter than T; labels out of range on either side; NaN behind every length"""
    rng = np.random.RandomState(5)
    labels = [[5] * 6, [5] * 6, [], [3, 4], [1, 2, 3], [1, C, 2], [4, -1]]
    il = [11, 10, 0, 0, 7, 12, 12]
    x = torch.from_numpy(rng.randn(12, len(il), C).astype(np.float32))
    for b, n in enumerate(il):
        x[n:, b] = float("nan")
    return x, labels, il


@functools.lru_cache(maxsize=None)
def tie_case(name):
    """integer-valued logits, so that many paths tie exactly: all zeros, and {-1, 0, 1} at random; S below and above 256"""
    rng = np.random.RandomState(11)
    L, T = {"zeros": (5, 20), "small": (7, 40), "wide": (140, 300)}[name]
    labels = [labels_of(L, rng), labels_of(L, rng), [9] * min(L, 10)]
    if name == "zeros":
        labels[0] = [1, 2, 3, 4, 5]
        x = torch.zeros(T, 3, C)
    else:
        x = torch.from_numpy(rng.randint(-1, 2, size=(T, 3, C)).astype(np.float32))
    return x, labels, [T, T - 3, T]


@functools.lru_cache(maxsize=None)
def bf16_case():
    """values bf16 holds exactly (it is the rounded tensor that both sides read)"""
    x, labels, il = size_case(127, "loose")
    return x.to(torch.bfloat16).float(), labels, il


@functools.lru_cache(maxsize=None)
def reference(key, *args):
    """forced_align_reference of a case above, computed once"""
    from unispeech_amd.ctc_align import forced_align_reference
    x, labels, il = globals()[key](*args)
    flat = np.array([v for lab in labels for v in lab], dtype=np.int64)
    return forced_align_reference(x, flat, il, [len(lab) for lab in labels], 0)


def put(x, dtype=torch.float32, batch_first=True):
    x = x.to(dtype)
    if batch_first:
        return x.transpose(0, 1).contiguous().cuda().transpose(0, 1)     # the T x B x C view of batch-first storage: the model's
    return x.contiguous().cuda()                                         # T x B x C storage


def device(x, labels, il, dtype=torch.float32, batch_first=True):
    from unispeech_amd.ctc_align import forced_align
    flat = np.array([v for lab in labels for v in lab], dtype=np.int64)
    a = forced_align(put(x, dtype, batch_first), flat, il, [len(lab) for lab in labels], 0)
    return tuple(v.cpu().numpy() for v in a)


def assert_equal_to_reference(got, want, what=""):
    """paths ==; scores within BOUND of the float64 value; -inf and NaN where the reference has them"""
    frames, spans, tok, score = got
    assert frames.dtype == np.int32 and spans.dtype == np.int32 and tok.dtype == np.float32 and score.dtype == np.float32
    assert frames.shape == want.frames.shape and spans.shape == want.spans.shape, what
    assert np.array_equal(frames, want.frames), what
    assert np.array_equal(spans, want.spans), what
    for g, w in ((score, want.score), (tok, want.token_scores)):
        g, w = g.astype(np.float64).reshape(-1), w.reshape(-1)
        fin = np.isfinite(w)
        assert np.array_equal(np.isnan(g), np.isnan(w)) and np.array_equal(g[~fin & ~np.isnan(w)], w[~fin & ~np.isnan(w)]), what
        err = np.abs(g[fin] - w[fin])
        lim = BOUND * np.maximum(1.0, np.abs(w[fin]))
        assert np.all(err <= lim), (what, float((err / lim).max()))
