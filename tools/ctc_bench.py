"""The CTC loss at the fine-tuning shape on one GPU, one process: B = 32 utterances of 15 s (T = 749 frames), C = 32 letters,
targets of 230 .. 270 labels, fp32 logits.  Timed: wavlm_ctc_loss (loss and gradient with respect to the logits, one call, three
launches) against torch's own device path for the same result -- F.log_softmax + F.ctc_loss(reduction="sum") forward, and the
backward of both -- alternating, HIP events around each timed loop after warm-up calls.  Also printed: the largest difference of
the two losses and gradients.  Nothing asserts on these numbers.

    python tools/ctc_bench.py [--reps 20] [--warmup 3] [--rounds 3]
Prints one JSON object."""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from unispeech_amd import ops  # noqa: E402


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    B, T, C = 32, 749, 32
    g = torch.Generator().manual_seed(0)
    tl = torch.randint(230, 271, (B,), generator=g).tolist()
    il = torch.randint(700, T + 1, (B,), generator=g).tolist()
    il[0] = T
    targets = torch.randint(1, C, (sum(tl),), generator=g)
    x = (torch.randn(B, T, C, generator=g) * 3).cuda()                    # batch-first, as the encoder leaves it
    t32 = targets.to(torch.int32).cuda()
    off = torch.tensor(np.concatenate([[0], np.cumsum(tl)]).astype(np.int32)).cuda()
    il32 = torch.tensor(il, dtype=torch.int32).cuda()
    ones = torch.ones(B, device="cuda")
    keep = [None]

    def ours():
        keep[0] = ops.ctc_loss_fwd_bwd(x, t32, off, sum(tl), max(tl), il32, 0, ones, False)

    xt = x.transpose(0, 1).detach().requires_grad_(True)                  # T x B x C view of the same storage
    tdev, ild, tld = targets.cuda(), torch.tensor(il).cuda(), torch.tensor(tl).cuda()

    def torch_fwd():
        return F.ctc_loss(F.log_softmax(xt, -1), tdev, ild, tld, 0, reduction="sum")

    def torch_fwd_bwd():
        xt.grad = None
        torch_fwd().backward()

    ours()
    nll, dx = keep[0]
    torch_fwd_bwd()
    dloss = abs(float(nll.double().sum()) - float(torch_fwd().detach().double()))
    dgrad = float((dx.transpose(0, 1) - xt.grad).abs().max())
    ms, tms, tfw = [], [], []
    for _ in range(a.rounds):                                             # alternate: the machine is shared
        ms.append(timed(ours, a.reps, a.warmup))
        tms.append(timed(torch_fwd_bwd, a.reps, a.warmup))
        with torch.no_grad():
            tfw.append(timed(torch_fwd, a.reps, a.warmup))
    m, t = float(np.median(ms)), float(np.median(tms))
    print(json.dumps({"device": torch.cuda.get_device_name(0), "B": B, "T": T, "C": C, "target_lengths": [min(tl), max(tl)],
                      "reps": a.reps, "rounds": a.rounds, "ctc_hip_fwd_bwd_ms": round(m, 4), "all_rounds_ms": [round(v, 4) for v in ms],
                      "torch_fwd_bwd_ms": round(t, 4), "torch_all_rounds_ms": [round(v, 4) for v in tms],
                      "torch_fwd_only_ms": round(float(np.median(tfw)), 4), "torch_over_hip": round(t / m, 3),
                      "loss_abs_diff": dloss, "grad_max_abs_diff": dgrad}))


if __name__ == "__main__":
    main()
