"""Shared inputs of tests/test_ctc.py and tests/test_ctc_gpu.py: five seeded cases (logits = randn * 3, blank 0) and their float64
results from torch's own F.ctc_loss on the CPU, computed once per process.

case  T, B, C        target lengths                 input lengths     what it pins
A     5, 3, 4        2, 0, 4 (two repeated pairs)   5, 3, 5           empty target; sample 2 needs 6 frames: no alignment, loss inf
B     70, 2, 32      40, 33, with repeats           70, 66            S = 81 > 64: positions cross a wave; ragged input lengths
C     300, 2, 48     140, 1                         300, 2            S = 281 > 256: lanes loop over positions; 2 frames beside 300
D     12, 2, 5       7, 12                          12, 12            T == L with repeats: sample 1 has no alignment
E     400, 4, 1000   150, 130, 1, 0                 400, 390, 3, 10   wide vocabulary; the class sum over a long row
Repeats are placed as t[1] = t[0]; t[3] = t[2] when L > 3."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

BLANK = 0
CASES = {
    "A": dict(T=5, B=3, C=4, tl=[2, 0, 4], il=[5, 3, 5], seed=11),
    "B": dict(T=70, B=2, C=32, tl=[40, 33], il=[70, 66], seed=12),
    "C": dict(T=300, B=2, C=48, tl=[140, 1], il=[300, 2], seed=13),
    "D": dict(T=12, B=2, C=5, tl=[7, 12], il=[12, 12], seed=14),
    "E": dict(T=400, B=4, C=1000, tl=[150, 130, 1, 0], il=[400, 390, 3, 10], seed=15),
}
INF_SAMPLES = {"A": [2], "B": [], "C": [], "D": [1], "E": []}


@functools.lru_cache(maxsize=None)
def case(name):
    """(logits fp32 [T, B, C], flat targets int64, input lengths, target lengths) -- treat as read-only"""
    c = CASES[name]
    g = torch.Generator().manual_seed(c["seed"])
    logits = torch.randn(c["T"], c["B"], c["C"], generator=g) * 3
    rows = []
    for L in c["tl"]:
        t = torch.randint(1, c["C"], (L,), generator=g)
        if L > 3:
            t[1] = t[0]
            t[3] = t[2]
        rows.append(t)
    return logits, torch.cat(rows), list(c["il"]), list(c["tl"])


def torch_ctc(logits, targets, il, tl, dtype, zero_infinity=False, weights=None):
    """torch's F.ctc_loss on the CPU in `dtype` on log_softmax(logits): (loss [B], d sum_b w_b loss_b / d logits [T, B, C]),
    both returned as float64 numpy"""
    x = logits.detach().to(dtype).clone().requires_grad_(True)
    loss = F.ctc_loss(F.log_softmax(x, -1), targets, torch.tensor(il), torch.tensor(tl), BLANK, reduction="none",
                      zero_infinity=zero_infinity)
    w = torch.ones(len(il), dtype=dtype) if weights is None else torch.as_tensor(weights, dtype=dtype)
    fin = torch.isfinite(loss)                   # an inf sample's rows are NaN in torch; keep it out of the others' sum
    grad, = torch.autograd.grad((loss[fin] * w[fin]).sum(), x) if fin.any() else (torch.zeros_like(x),)
    return loss.detach().double().numpy(), grad.double().numpy()


@functools.lru_cache(maxsize=None)
def ref64(name, zero_infinity=False, bf16=False):
    """float64 loss and gradient (of the sum over the samples that have an alignment); bf16: on the logits rounded to bf16"""
    logits, targets, il, tl = case(name)
    if bf16:
        logits = logits.to(torch.bfloat16).float()
    return torch_ctc(logits, targets, il, tl, torch.float64, zero_infinity)


@functools.lru_cache(maxsize=None)
def e32(name, bf16=False):
    """E32: the error of torch's own fp32 CPU F.ctc_loss against float64 on the same inputs -- per sample for the loss, and
    per sample the largest absolute error over (t, c) for the gradient.  (E32loss [B], E32grad [B])"""
    logits, targets, il, tl = case(name)
    if bf16:
        logits = logits.to(torch.bfloat16).float()
    l32, g32 = torch_ctc(logits, targets, il, tl, torch.float32)
    l64, g64 = ref64(name, False, bf16)
    with np.errstate(invalid="ignore"):
        el = np.where(np.isfinite(l64), np.abs(l32 - l64), 0.0)
    eg = np.abs(g32 - g64).max(axis=(0, 2))
    return el, eg
