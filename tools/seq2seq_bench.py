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
  fused_step_ms        the same loop with shallow fusion of a Transformer LM (--lm-dim wide, --lm-layers layers; default 512 and
                       6) at lm_weight 0.7 and no_repeat_ngram_size 3: its stack over the same tree, one GEMM onto V, and
                       wavlm_beam_step_fused in place of wavlm_beam_step
  fused_host_reads     device-to-host reads inside that loop
  beam_step_us, beam_step_fused_us     the step kernels alone at R = B * beam rows and step 32, device events around --kernel-iters
                       launches: wavlm_beam_step, and wavlm_beam_step_fused with fp32 LM logits and n = 3 over random histories

    python tools/seq2seq_bench.py [--bf16] [--vocab 32 10000] [--max-len 64] [--repeats 5] [--lm-dim 512 --lm-layers 6]
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


def build_lm(V, a, dtype):
    from unispeech_amd.transformer_lm import TransformerLM
    torch.manual_seed(a.seed + 2)
    lm = TransformerLM(dict(decoder_embed_dim=a.lm_dim, decoder_ffn_embed_dim=4 * a.lm_dim, decoder_layers=a.lm_layers,
                            decoder_attention_heads=a.lm_dim // 64, max_target_positions=a.max_len + 2,
                            decoder_normalize_before=True), V)
    with torch.no_grad():
        for prm in lm.parameters():
            if prm.dim() > 1:
                prm.copy_(torch.randn_like(prm) / math.sqrt(prm.shape[-1]))
    return lm.cuda().to(dtype)


def timed_loop(run, repeats):
    """median, min and max wall time of run() over `repeats` runs after one that warms up; -> (times, the last result)"""
    times, res = [], None
    for r in range(repeats + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = run()
        torch.cuda.synchronize()
        if r:
            times.append(time.perf_counter() - t0)
    return times, res


def step_kernels_us(V, B, beam, iters, seed):
    """(wavlm_beam_step, wavlm_beam_step_fused) alone in microseconds: full beams at step 32 of 64, random fp32 logits, LM logits
    and histories over 8 symbols; the state is rebuilt outside the timed region, each launch reads the same rows"""
    from unispeech_amd import ops
    R, step, max_len = B * beam, 32, 64
    g = torch.Generator().manual_seed(seed + 3)
    logits = (3.0 * torch.randn(R, V, generator=g)).cuda()
    lm = (2.0 * torch.randn(R, V, generator=g)).cuda()
    hist = torch.randint(4, min(V, 12), (step + 1, R), generator=g).to(torch.int32)
    out = []
    for fused in (False, True):
        st = ops.BeamState(B, beam, max_len, 2, "cuda")
        st.tree_token[:(step + 1) * R] = hist.reshape(-1).cuda()
        st.anc[0][:, :step] = (torch.arange(step).view(1, -1) * R + torch.arange(R).view(-1, 1)).to(torch.int32).cuda()
        snap = None
        kw = dict(max_len=max_len, min_len=1, pad=1, unk=3, eos=2, step=step)

        def reset():
            st.n_live.fill_(beam)
            st.n_fin.zero_()
            st.cum.copy_(snap)
            st.tokens.copy_(hist[step].cuda())
        snap = -5.0 * torch.rand(R, generator=g).cuda()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        total = 0.0
        for i in range(iters + 5):
            reset()
            work = logits.clone() if fused else logits               # the fused step consumes its logits
            e0.record()
            if fused:
                ops.beam_step_fused(work, st, V, lm_logits=lm, lm_weight=0.7, no_repeat_ngram_size=3, **kw)
            else:
                ops.beam_step(work, st, V, **kw)
            e1.record()
            torch.cuda.synchronize()
            if i >= 5:
                total += e0.elapsed_time(e1)
        out.append(total * 1e3 / iters)
    return out


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
    p.add_argument("--lm-dim", type=int, default=512)
    p.add_argument("--lm-layers", type=int, default=6)
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
        reads = m.loop_reads
        lm = build_lm(V, a, dtype)
        ftimes, _ = timed_loop(lambda: m.search(enc, 0, beam=beam, max_len_b=a.max_len, lm_model=lm, lm_weight=0.7,
                                                no_repeat_ngram_size=3), a.repeats)
        ft, fsteps, freads = statistics.median(ftimes), m.loop_steps, m.loop_reads
        bs_us, bsf_us = step_kernels_us(V, B, beam, min(a.kernel_iters, 50), a.seed)
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
            "tokens_per_s": round(tokens / t, 1), "host_reads": reads,
            "lm": {"dim": a.lm_dim, "layers": a.lm_layers}, "fused_steps": fsteps, "fused_loop_ms": round(ft * 1e3, 3),
            "fused_step_ms": round(ft * 1e3 / fsteps, 4), "fused_host_reads": freads,
            "beam_step_us": round(bs_us, 2), "beam_step_fused_us": round(bsf_us, 2),
            "cross_attn_us": round(us, 2), "cross_attn_bytes": moved, "cross_attn_gbs": round(moved / us * 1e-3, 1),
            "share_of_hbm_peak": round(moved / us * 1e-3 / HBM_PEAK_GBS, 4), "per_row_bytes": beam * kv_bytes + 2 * R * D * es}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
