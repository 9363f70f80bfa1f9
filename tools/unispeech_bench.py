"""The UniSpeech multitask step at the Large recipe's per-GPU batch on one GPU, one process (src/examples/unispeech/scripts/
one2one_large_pretrain_en1350.sh: 24 layers, d = 1024, FFN 4096, 16 heads, layer_norm extractor, final_dim 768, 320 x 2 codebook,
transpose, negatives_from_everywhere, 100 negatives, mtlalpha 0.5, replace_prob 0.5; --max-tokens 1200000 = 5 utterances of 15 s,
T = 749 frames), bf16, forward + backward:

  unispeech_step_ms   Unispeech + UnispeechCriterion (contrastive head, replace-mix, CTC head over a 32-symbol dictionary, CTC loss)
  wav2vec2_step_ms    Wav2Vec2Model + Wav2vecCriterion with the same configuration and input, the step without the CTC branch
  replace_mix_ms / dropout_ms          wavlm_replace_mix next to wavlm_dropout on the [B * T, 1024] bf16 tensor of the step (they move
  replace_mix_bwd_ms                   the same bytes; the backward writes two tensors)

alternating, HIP events around each timed loop after warm-up calls.  Nothing asserts on these numbers.

    python tools/unispeech_bench.py [--batch 5] [--seconds 15] [--reps 10] [--warmup 3] [--rounds 3]
Prints one JSON object."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from unispeech_amd import ops  # noqa: E402
from unispeech_amd.unispeech import UniSpeechConfig, Unispeech, UnispeechCriterion  # noqa: E402
from unispeech_amd.wav2vec2 import Wav2Vec2Config, Wav2Vec2Model, Wav2vecCriterion  # noqa: E402

LARGE = dict(extractor_mode="layer_norm", encoder_layers=24, encoder_embed_dim=1024, encoder_ffn_embed_dim=4096,
             encoder_attention_heads=16, final_dim=768, layer_norm_first=True, conv_bias=True, logit_temp=0.1, quantize_targets=True,
             latent_vars=320, latent_groups=2, latent_temp=(2, 0.1, 0.999995), mask_length=10, mask_prob=0.5, encoder_layerdrop=0.0,
             dropout_input=0.1, dropout_features=0.1, feature_grad_mult=1.0, conv_pos=128, conv_pos_groups=16, num_negatives=100,
             cross_sample_negatives=0, dropout=0.1, attention_dropout=0.1, negatives_from_everywhere=True, transpose=True)
NCLS = 32


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
    ap.add_argument("--batch", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=15.0)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    B, n = a.batch, int(16000 * a.seconds)
    g = torch.Generator().manual_seed(0)
    wav = torch.randn(B, n, generator=g).cuda().to(torch.bfloat16)
    pm = torch.zeros(B, n, dtype=torch.bool)
    tl = torch.randint(180, 221, (B,), generator=g)
    target = torch.randint(4, NCLS, (B, int(tl.max())), generator=g)
    target[torch.arange(target.shape[1]).view(1, -1) >= tl.view(-1, 1)] = 1
    sample = {"id": torch.arange(B), "target": target, "target_lengths": tl, "ntokens": int(tl.sum()),
              "net_input": {"source": wav, "padding_mask": pm.cuda(), "padding_mask_cpu": pm}}
    torch.manual_seed(0)
    uni = Unispeech(UniSpeechConfig(replace_prob=0.5, final_dropout=0.1, **LARGE), NCLS).cuda().to(torch.bfloat16).train()
    ucrit = UnispeechCriterion(blank_idx=0, pad_idx=1, eos_idx=2, mtlalpha=0.5, infonce=True, loss_weights=[0.1, 0.0],
                               post_process=None)
    torch.manual_seed(0)
    w2v = Wav2Vec2Model(Wav2Vec2Config(**LARGE)).cuda().to(torch.bfloat16).train()
    wcrit = Wav2vecCriterion(None, infonce=True, loss_weights=[0.1, 0.0])
    last = {}

    def step(model, crit, tag):
        def fn():
            for p in model.parameters():
                p.grad = None
            loss, _, _ = crit(model, sample)
            loss.backward()
            last[tag] = loss
        return fn

    uni_step, w2v_step = step(uni, ucrit, "unispeech"), step(w2v, wcrit, "wav2vec2")
    np.random.seed(1)
    uni_step()
    T = n
    for k, s in [(10, 5)] + [(3, 2)] * 4 + [(2, 2)] * 2:                        # frames of the default conv_feature_layers
        T = (T - k) // s + 1
    rows, D = B * T, LARGE["encoder_embed_dim"]
    x = torch.randn(rows, D, generator=g).cuda().to(torch.bfloat16)
    q = torch.randn(rows, D, generator=g).cuda().to(torch.bfloat16)
    sel = (torch.rand(rows, generator=g) < 0.5).to(torch.uint8).cuda()
    kern = {"replace_mix_ms": lambda: ops.replace_mix(x, q, sel, 0.1, 7), "dropout_ms": lambda: ops.dropout(x, 0.1, 7),
            "replace_mix_bwd_ms": lambda: ops.replace_mix_bwd(x, sel, 0.1, 7)}
    res = {"unispeech_step_ms": [], "wav2vec2_step_ms": [], **{k: [] for k in kern}}
    for _ in range(a.rounds):                                                   # alternate: the machine is shared
        res["unispeech_step_ms"].append(timed(uni_step, a.reps, a.warmup))
        res["wav2vec2_step_ms"].append(timed(w2v_step, a.reps, a.warmup))
        for k, fn in kern.items():
            res[k].append(timed(fn, 20 * a.reps, a.warmup))
    out = {"device": torch.cuda.get_device_name(0), "batch": B, "seconds": a.seconds, "frames": T, "classes": NCLS, "reps": a.reps,
           "rounds": a.rounds, "replace_mix_rows": rows, "replace_mix_D": D,
           "unispeech_loss": float(last["unispeech"]), "wav2vec2_loss": float(last["wav2vec2"])}
    for k, v in res.items():
        out[k] = round(float(np.median(v)), 4)
        out[k.replace("_ms", "_all_rounds_ms")] = [round(float(t), 4) for t in v]
    out["unispeech_over_wav2vec2"] = round(out["unispeech_step_ms"] / out["wav2vec2_step_ms"], 4)
    out["replace_mix_over_dropout"] = round(out["replace_mix_ms"] / out["dropout_ms"], 4)
    out["replace_mix_GBps"] = round(2 * rows * D * 2 / (out["replace_mix_ms"] * 1e-3) / 1e9, 1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
