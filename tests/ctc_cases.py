"""Shared inputs of tests/test_ctc.py and tests/test_ctc_gpu.py: seeded cases and their float64 results from torch's own
F.ctc_loss on the CPU, computed once per process.  Blank 0 in CASES; BLANK_CASES carry a blank of their own.

Cases A to E: logits = randn * 3.
case  T, B, C        target lengths                 input lengths     what it pins
A     5, 3, 4        2, 0, 4 (two repeated pairs)   5, 3, 5           empty target; sample 2 needs 6 frames: no alignment, loss inf
B     70, 2, 32      40, 33, with repeats           70, 66            S = 81 > 64: positions cross a wave; ragged input lengths
C     300, 2, 48     140, 1                         300, 2            S = 281 > 256: lanes loop over positions; 2 frames beside 300
D     12, 2, 5       7, 12                          12, 12            T == L with repeats: sample 1 has no alignment
E     400, 4, 1000   150, 130, 1, 0                 400, 390, 3, 10   wide vocabulary; the class sum over a long row
Repeats are placed as t[1] = t[0]; t[3] = t[2] when L > 3.

The kernels of csrc/ctc.hip are compiled per number of extended positions a lane owns, PER = 1, 2, 4, 8 for S = 2 Lmax + 1 up to
256, 512, 1024, 2047 (variant() restates the rule), and the longest target of the batch picks the variant for every sample of it.
The cases below sit on each side of every boundary; their names carry the variant.  All have C = 32 unless the name says otherwise.

"peaked" cases (key peak): logits = randn, plus PEAK on the class of one valid CTC path per sample (monotone, a blank forced
between repeated labels, the spare frames spread at random over all 2 L + 1 positions) -- the regime of a trained model.  With
randn * 3 the loss of a 500-label sample is in the thousands and E32, the tolerance's unit (e32() below), grows until 4 x E32 of
the gradient is a few per cent of the gradient itself; peaked, it stays below 1 % (tests/test_ctc.py asserts that, and that E32
is not below the rounding of an fp32 output either).  A sample without an alignment gets no path.
case              T     target lengths        input lengths            S     what it pins
L127_per1         300   127, 60               300, 250                 255   PER 1, lane 255 idle
L128_per2         300   128, 90               290, 300                 257   PER 2, the second sweep holds one position
L255_per2         560   255, 200              560, 500                 511   PER 2, one position short of full
L256_per4         560   256, 120, 256         560, 540, 257            513   PER 4; sample 2 needs 258 frames: loss inf
L511_per4         1100  511, 300              1100, 1000               1023  PER 4, one position short of full
L512_per8         1100  512, 300, 300         1090, 1100, 301          1025  PER 8; sample 2 needs 302 frames: loss inf
L600_per8         1100  600, 150              1100, 900                1201  PER 8 with labels in the fifth sweep (at S = 1025 that
                                                                             sweep holds position 1024 alone, a blank: no skip there)
L1023_per8        2100  1023, 0, 5, 300       2100, 2100, 1500, 2000   2047  the cap; short riders under PER 8 and the widest alpha
                                                                             stride; alone they run PER 1 and PER 4 (same bits)
L1023tight_per8   1100  1023, 700             1100, 1050               2047  1100 frames for 1023 labels: 75 spare frames
runs256_per4      580   256 equal, 256 a b    580, 560                 513   one class 256 times (one lane sums them; no skip
                        a b ...                                              transition; 511 frames needed) | two classes
                                                                             alternating, every skip open, 128 occurrences each
Not peaked (randn * 3, many competing paths):
bench_per4        749   230, 270, 251         749, 700, 730            541   the distribution of tools/ctc_bench.py
C1024_per1        60    40, 30                60, 55    C = 1024: the cap; classes 768, 1023 present (slot q = 3, lane 255)
C257_per1         60    40, 20                60, 55    C = 257: slot 1 holds one class, 256, present in both samples
C1_per1           20    0, 0                  20, 7     C = 1: only the blank; loss and gradient are exactly 0
BLANK_CASES (T, C = 70, 32; 40, 33 labels; 70, 66 frames; randn * 3):
blank31           blank = C - 1, labels from [0, 31)
blank7            blank = 7; labels 2, 3 (a repeated pair) and 10 of sample 0 are 7 themselves: a label that names the blank"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

BLANK = 0
PEAK = 6.0
CASES = {
    "A": dict(T=5, B=3, C=4, tl=[2, 0, 4], il=[5, 3, 5], seed=11),
    "B": dict(T=70, B=2, C=32, tl=[40, 33], il=[70, 66], seed=12),
    "C": dict(T=300, B=2, C=48, tl=[140, 1], il=[300, 2], seed=13),
    "D": dict(T=12, B=2, C=5, tl=[7, 12], il=[12, 12], seed=14),
    "E": dict(T=400, B=4, C=1000, tl=[150, 130, 1, 0], il=[400, 390, 3, 10], seed=15),
    "L127_per1": dict(T=300, B=2, C=32, tl=[127, 60], il=[300, 250], seed=31, peak=PEAK),
    "L128_per2": dict(T=300, B=2, C=32, tl=[128, 90], il=[290, 300], seed=32, peak=PEAK),
    "L255_per2": dict(T=560, B=2, C=32, tl=[255, 200], il=[560, 500], seed=33, peak=PEAK),
    "L256_per4": dict(T=560, B=3, C=32, tl=[256, 120, 256], il=[560, 540, 257], seed=34, peak=PEAK),
    "L511_per4": dict(T=1100, B=2, C=32, tl=[511, 300], il=[1100, 1000], seed=135, peak=PEAK),
    "L512_per8": dict(T=1100, B=3, C=32, tl=[512, 300, 300], il=[1090, 1100, 301], seed=36, peak=PEAK),
    "L600_per8": dict(T=1100, B=2, C=32, tl=[600, 150], il=[1100, 900], seed=44, peak=PEAK),
    "L1023_per8": dict(T=2100, B=4, C=32, tl=[1023, 0, 5, 300], il=[2100, 2100, 1500, 2000], seed=137, peak=PEAK),
    "L1023tight_per8": dict(T=1100, B=2, C=32, tl=[1023, 700], il=[1100, 1050], seed=38, peak=PEAK),
    "runs256_per4": dict(T=580, B=2, C=32, tl=[256, 256], il=[580, 560], seed=239, peak=PEAK, labels=["same", "alt"]),
    "bench_per4": dict(T=749, B=3, C=32, tl=[230, 270, 251], il=[749, 700, 730], seed=40),
    "C1024_per1": dict(T=60, B=2, C=1024, tl=[40, 30], il=[60, 55], seed=641, put=[(0, 5, 1023), (0, 6, 768), (1, 7, 1023)]),
    "C257_per1": dict(T=60, B=2, C=257, tl=[40, 20], il=[60, 55], seed=242, put=[(0, 5, 256), (1, 7, 256)]),
    "C1_per1": dict(T=20, B=2, C=1, tl=[0, 0], il=[20, 7], seed=43),
}
BLANK_CASES = {
    "blank31": dict(T=70, B=2, C=32, tl=[40, 33], il=[70, 66], seed=551, blank=31),
    "blank7": dict(T=70, B=2, C=32, tl=[40, 33], il=[70, 66], seed=652, blank=7, put=[(0, 2, 7), (0, 3, 7), (0, 10, 7)]),
}
INF_SAMPLES = {"A": [2], "B": [], "C": [], "D": [1], "E": [], "L127_per1": [], "L128_per2": [], "L255_per2": [],
               "L256_per4": [2], "L511_per4": [], "L512_per8": [2], "L600_per8": [], "L1023_per8": [], "L1023tight_per8": [], "runs256_per4": [],
               "bench_per4": [], "C1024_per1": [], "C257_per1": [], "C1_per1": [], "blank31": [], "blank7": []}
NEW_CASES = [n for n in list(CASES) + list(BLANK_CASES) if n not in ("A", "B", "C", "D", "E")]


def variant(Lmax):
    """positions per lane of the kernels that a batch whose longest target has Lmax labels runs (wavlm_ctc_loss's dispatch)"""
    S = 2 * Lmax + 1
    return 1 if S <= 256 else 2 if S <= 512 else 4 if S <= 1024 else 8


def _path(t, blank, frames, g):
    """the classes of a valid CTC path of `frames` frames for the labels t, or None if there is none"""
    S = 2 * len(t) + 1
    ext = torch.full((S,), blank, dtype=torch.long)
    ext[1::2] = t
    dur = torch.zeros(S, dtype=torch.long)
    dur[1::2] = 1
    if len(t) > 1:
        dur[2:-1:2] = (t[1:] == t[:-1]).long()           # the blank between a repeated label cannot be left out
    spare = frames - int(dur.sum())
    if spare < 0:
        return None
    dur += torch.bincount(torch.randint(0, S, (spare,), generator=g), minlength=S)
    return torch.repeat_interleave(ext, dur)


@functools.lru_cache(maxsize=None)
def case(name):
    """(logits fp32 [T, B, C], flat targets int64, input lengths, target lengths) -- treat as read-only.
    Optional keys: peak (randn logits + peak along one valid path per sample), labels (per sample "same": one class throughout,
    "alt": two classes alternating, neither with the repeated pairs), put ((sample, index, label) written after the pairs),
    blank (labels are drawn from the classes other than it)."""
    c = CASES[name] if name in CASES else BLANK_CASES[name]
    g = torch.Generator().manual_seed(c["seed"])
    logits = torch.randn(c["T"], c["B"], c["C"], generator=g) * (1 if "peak" in c else 3)
    rows = []
    for b, L in enumerate(c["tl"]):
        kind = c["labels"][b] if "labels" in c else None
        if c["C"] == 1:
            t = torch.zeros(L, dtype=torch.long)          # no class but the blank: only L = 0 has labels in range
        elif kind is not None:
            two = torch.randperm(c["C"] - 1, generator=g)[:2] + 1
            t = two[0].repeat(L) if kind == "same" else two[torch.arange(L) % 2]
        elif "blank" in c:
            t = torch.randint(0, c["C"] - 1, (L,), generator=g)
            t = t + (t >= c["blank"]).long()
        else:
            t = torch.randint(1, c["C"], (L,), generator=g)
        if L > 3 and kind is None:
            t[1] = t[0]
            t[3] = t[2]
        for pb, i, label in c.get("put", ()):
            if pb == b:
                t[i] = label
        rows.append(t)
    if "peak" in c:
        for b, t in enumerate(rows):
            path = _path(t, c.get("blank", BLANK), c["il"][b], g)
            if path is not None:
                logits[torch.arange(len(path)), b, path] += c["peak"]
    return logits, torch.cat(rows), list(c["il"]), list(c["tl"])


def torch_ctc(logits, targets, il, tl, dtype, zero_infinity=False, weights=None, blank=BLANK):
    """torch's F.ctc_loss on the CPU in `dtype` on log_softmax(logits): (loss [B], d sum_b w_b loss_b / d logits [T, B, C]),
    both returned as float64 numpy"""
    x = logits.detach().to(dtype).clone().requires_grad_(True)
    loss = F.ctc_loss(F.log_softmax(x, -1), targets, torch.tensor(il), torch.tensor(tl), blank, reduction="none",
                      zero_infinity=zero_infinity)
    w = torch.ones(len(il), dtype=dtype) if weights is None else torch.as_tensor(weights, dtype=dtype)
    fin = torch.isfinite(loss)                   # an inf sample's rows are NaN in torch; keep it out of the others' sum
    grad, = torch.autograd.grad((loss[fin] * w[fin]).sum(), x) if fin.any() else (torch.zeros_like(x),)
    return loss.detach().double().numpy(), grad.double().numpy()


@functools.lru_cache(maxsize=None)
def ref64(name, zero_infinity=False, bf16=False, blank=BLANK):
    """float64 loss and gradient (of the sum over the samples that have an alignment); bf16: on the logits rounded to bf16"""
    logits, targets, il, tl = case(name)
    if bf16:
        logits = logits.to(torch.bfloat16).float()
    return torch_ctc(logits, targets, il, tl, torch.float64, zero_infinity, blank=blank)


@functools.lru_cache(maxsize=None)
def e32(name, bf16=False, blank=BLANK):
    """E32: the error of torch's own fp32 CPU F.ctc_loss against float64 on the same inputs -- per sample for the loss, and
    per sample the largest absolute error over (t, c) for the gradient.  (E32loss [B], E32grad [B])"""
    logits, targets, il, tl = case(name)
    if bf16:
        logits = logits.to(torch.bfloat16).float()
    l32, g32 = torch_ctc(logits, targets, il, tl, torch.float32, blank=blank)
    l64, g64 = ref64(name, False, bf16, blank)
    with np.errstate(invalid="ignore"):
        el = np.where(np.isfinite(l64), np.abs(l32 - l64), 0.0)
    eg = np.abs(g32 - g64).max(axis=(0, 2))
    return el, eg
