"""What does a step of the seq2seq beam search cost on the device, and how close to the memory system does the cross-attention
kernel run?  A seeded decoder (random weights: the figures say what the launches cost, nothing about word error rates) over a
synthetic encoder output -- the encoder itself is not part of this (bench.py measures it).  Needs a GPU.

Shape: decoder 768 wide, 6 layers, 12 heads of 64, B = 16 sentences of Ts = 750 frames, beam 5, V = 32 and V = 10 000.
Per vocabulary, one JSON line:
  step_ms              the search loop (Wav2Vec2Seq2Seq.search: every launch of a step, the reads of the finished counter) over the
                       steps it ran, a host clock around work that ends in a device synchronise; median of --repeats runs
  tokens_per_s         tokens of the returned 1-bests over that time
  host_reads           device-to-host reads inside the loop (Wav2Vec2Seq2Seq.loop_reads)
  cross_attn_us        wavlm_attn_cross_fwd alone at the loop's shape (R = B * beam rows, live = all), device events around
                       --kernel-iters launches
  cross_attn_bytes     K | V of every sentence once, + Q + O: what the shared pass has to move
  cross_attn_gbs, share_of_hbm_peak     bytes over time, against 8000 GB/s
  per_row_bytes        what a wave per row would move: K | V once per row (beam x the K | V above)

    python tools/seq2seq_bench.py [--bf16] [--vocab 32 10000] [--max-len 64] [--repeats 5]
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0


def build(V, a, dtype):
    from unispeech_amd.seq2seq import Wav2Vec2Seq2Seq
    from unispeech_amd.wav2vec2 import Wav2Vec2Config, Wav2Vec2Model
    # the wrapped encoder only gives the model its width here; it is never run
    inner = Wav2Vec2Model(Wav2Vec2Config(encoder_layers=1, encoder_embed_dim=a.dim, encoder_ffn_embed_dim=a.dim,
                                         encoder_attention_heads=a.dim // 64))
    inner.remove_pretraining_modules()
    torch.manual_seed(a.seed)
    m = Wav2Vec2Seq2Seq(inner, V, dict(decoder_embed_dim=a.dim, decoder_ffn_embed_dim=4 * a.dim, decoder_layers=a.layers,
                                       decoder_attention_heads=a.dim // 64, max_target_positions=a.max_len + 2))
    with torch.no_grad():
        for prm in m.decoder.parameters():
            if prm.dim() > 1:
                prm.copy_(torch.randn_like(prm) / math.sqrt(prm.shape[-1]))
    return m.cuda().to(dtype)


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--vocab", type=int, nargs="+", default=[32, 10000])
    p.add_argument("--batch", type=int, default=16)
    p.add_argument("--beam", type=int, default=5)
    p.add_argument("--frames", type=int, default=750)
    p.add_argument("--dim", type=int, default=768)
    p.add_argument("--layers", type=int, default=6)
    p.add_argument("--max-len", type=int, default=64)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--kernel-iters", type=int, default=200)
    p.add_argument("--bf16", action="store_true")
    p.add_argument("--seed", type=int, default=0)
    a = p.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("seq2seq_bench needs a GPU: nothing is measured without one")
    from unispeech_amd import ops
    dtype = torch.bfloat16 if a.bf16 else torch.float32
    es = 2 if a.bf16 else 4
    B, beam, Ts, D, H = a.batch, a.beam, a.frames, a.dim, a.dim // 64
    g = torch.Generator().manual_seed(a.seed + 1)
    x = torch.randn(B, Ts, D, generator=g).cuda().to(dtype)
    for V in a.vocab:
        m = build(V, a, dtype)
        with torch.no_grad():
            enc = m.attend_to(x, None)
        times, steps, tokens = [], 0, 0
        for r in range(a.repeats + 1):                                          # run 0 warms up and is not counted
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = m.search(enc, 0, beam=beam, max_len_b=a.max_len)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if r:
                times.append(dt)
            tokens = sum(h[0]["tokens"].numel() for h in res if h)
            steps = max((h[0]["tokens"].numel() for h in res if h), default=0)
        steps_run = m.loop_steps
        t = statistics.median(times)
        # the kernel alone at the loop's shape
        R = B * beam
        q = torch.randn(R, D, generator=g).cuda().to(dtype)
        off = (torch.arange(B + 1, dtype=torch.int32) * beam).cuda()
        out = torch.empty_like(q)
        for _ in range(10):
            ops.attn_cross_fwd(q, enc[2][0], H, off, None, None, max_group=beam, out=out)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(a.kernel_iters):
            ops.attn_cross_fwd(q, enc[2][i % a.layers], H, off, None, None, max_group=beam, out=out)
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) * 1e3 / a.kernel_iters
        kv_bytes = B * Ts * 2 * D * es
        moved = kv_bytes + 2 * R * D * es
        print(json.dumps({
            "V": V, "dtype": "bf16" if a.bf16 else "fp32", "B": B, "beam": beam, "Ts": Ts, "decoder": {"dim": D, "layers": a.layers,
                                                                                                  "heads": H},
            "steps": steps_run, "longest_hypothesis": steps, "loop_ms": round(t * 1e3, 3), "step_ms": round(t * 1e3 / steps_run, 4),
            "loop_ms_min_max": [round(min(times) * 1e3, 3), round(max(times) * 1e3, 3)],
            "tokens_per_s": round(tokens / t, 1), "host_reads": m.loop_reads,
            "cross_attn_us": round(us, 2), "cross_attn_bytes": moved, "cross_attn_gbs": round(moved / us * 1e-3, 1),
            "share_of_hbm_peak": round(moved / us * 1e-3 / HBM_PEAK_GBS, 4), "per_row_bytes": beam * kv_bytes + 2 * R * D * es}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
