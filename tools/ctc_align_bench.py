"""CTC forced alignment at the fine-tuning shape of tools/ctc_bench.py on one GPU, one process: B = 32 utterances of 15 s (T = 749
frames), C = 32 letters, transcripts of 230 .. 270 labels, fp32 logits.  Timed: wavlm_ctc_align (two launches) next to
wavlm_ctc_loss forward + backward on the same inputs, alternating, HIP events around each timed loop after warm-up calls.  The
phases of the alignment kernel -- forward pass, back-trace, sums -- come from the clock stamps each sample's workgroup leaves in
front of the workspace (100 MHz ticks; include/wavlm_hip.h), averaged over the samples of the last call.  Nothing asserts on
these numbers.

    python tools/ctc_align_bench.py [--reps 20] [--warmup 3] [--rounds 3]
Prints one JSON object."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from unispeech_amd import _lib, ops  # noqa: E402
from ctc_bench import timed  # noqa: E402


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
    ws = torch.empty(_lib.lib().wavlm_ctc_align_workspace_bytes(B, T, max(tl)), dtype=torch.uint8, device="cuda")
    keep = [None, None]

    def align():
        keep[0] = ops.ctc_align(x, t32, off, sum(tl), max(tl), il32, 0, ws=ws)

    def loss():
        keep[1] = ops.ctc_loss_fwd_bwd(x, t32, off, sum(tl), max(tl), il32, 0, ones, False)

    ams, lms = [], []
    for _ in range(a.rounds):                                             # alternate: the machine is shared
        ams.append(timed(align, a.reps, a.warmup))
        lms.append(timed(loss, a.reps, a.warmup))
    ticks = ws[:B * 32].view(torch.int64).view(B, 4).cpu().numpy().astype(np.float64)
    phase = np.diff(ticks, axis=1) / 100.0                                # microseconds per sample: forward, back-trace, sums
    fwd, back, sums = (float(v) for v in phase.mean(0))
    am, lm = float(np.median(ams)), float(np.median(lms))
    print(json.dumps({"device": torch.cuda.get_device_name(0), "B": B, "T": T, "C": C, "target_lengths": [min(tl), max(tl)],
                      "reps": a.reps, "rounds": a.rounds, "ctc_align_ms": round(am, 4), "all_rounds_ms": [round(v, 4) for v in ams],
                      "ctc_loss_fwd_bwd_ms": round(lm, 4), "loss_all_rounds_ms": [round(v, 4) for v in lms],
                      "align_over_loss": round(am / lm, 3), "kernel_forward_us": round(fwd, 1), "kernel_backtrace_us": round(back, 1),
                      "kernel_sums_us": round(sums, 1), "backtrace_share_of_kernel": round(back / (fwd + back + sums), 3),
                      "slowest_sample_us": round(float((ticks[:, 3] - ticks[:, 0]).max() / 100.0), 1),
                      "finite_scores": int(torch.isfinite(keep[0][3]).sum())}))


if __name__ == "__main__":
    main()
