"""Times the output layer of the Transformer LM (csrc/lm.hip wavlm_lm_logprob) against the composition one would run without
it -- wavlm_gemm into fp32 logits + wavlm_ce_rows in row chunks of a fixed budget, WAVLM_LM_LOGPROB_COMPOSED=1 -- on the same
inputs, and TransformerLM.score of a 16-layer D 1024 model on a batch of the same size.  Needs a GPU.

Method: HIP events around each call, warm-up first, the two sides alternating inside one process, medians.  Derived figures: the
kernel's share of the bf16 MFMA peak (2 R V D FLOPs over its time), and the composition's algorithmic HBM traffic (X and W once
per row chunk, the fp32 logits written by the GEMM and read by the row kernel) over its time.

    python tools/transformer_lm_bench.py [--rows 32768 --vocab 200000 --dim 1024 --iters 7 --warmup 2 --layers 16]
prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BF16_MFMA_PEAK_TFLOPS = 2500.0
HBM_PEAK_GBS = 8000.0


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--rows", type=int, default=32768)
    p.add_argument("--vocab", type=int, default=200000)
    p.add_argument("--dim", type=int, default=1024)
    p.add_argument("--iters", type=int, default=7)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--layers", type=int, default=16, help="0: skip the model")
    a = p.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("transformer_lm_bench needs a GPU: nothing is measured without one")
    from unispeech_amd import _lib, transformer_lm as T
    R, V, D = a.rows, a.vocab, a.dim
    g = torch.Generator(device="cuda").manual_seed(0)
    X = (torch.randn(R, D, generator=g, device="cuda") * 0.5).to(torch.bfloat16)
    W = (torch.randn(V, D, generator=g, device="cuda") * D ** -0.5).to(torch.bfloat16)
    tgt = torch.randint(0, V, (R,), generator=g, device="cuda", dtype=torch.int32)

    def kernel():
        os.environ["WAVLM_LM_LOGPROB_COMPOSED"] = "0"
        return T.lm_logprob(X, W, tgt)[0]

    def composed():
        os.environ["WAVLM_LM_LOGPROB_COMPOSED"] = "1"
        return T.lm_logprob(X, W, tgt)[0]
    for _ in range(a.warmup):
        lk, lc = kernel(), composed()
    torch.cuda.synchronize()
    diff = (lk - lc).abs().max().item()
    tk, tc = [], []
    for _ in range(a.iters):                                  # alternating: both sides see the same neighbours
        tk.append(timed(kernel)[0])
        tc.append(timed(composed)[0])
    mk, mc = statistics.median(tk), statistics.median(tc)
    flops = 2.0 * R * V * D
    ld = (V + 3) // 4 * 4
    chunk = max(1, min(R, T.COMPOSED_BUDGET_BYTES // (4 * ld)))
    nchunks = (R + chunk - 1) // chunk
    comp_bytes = R * D * 2 + nchunks * V * D * 2 + 2 * R * ld * 4
    out = {"rows": R, "vocab": V, "dim": D, "dtype": "bf16", "iters": a.iters,
           "kernel_ms": round(mk, 3), "kernel_ms_min_max": [round(min(tk), 3), round(max(tk), 3)],
           "composed_ms": round(mc, 3), "composed_ms_min_max": [round(min(tc), 3), round(max(tc), 3)],
           "kernel_over_composed": round(mk / mc, 3),
           "kernel_tflops": round(flops / (mk * 1e-3) / 1e12, 1),
           "kernel_frac_of_bf16_mfma_peak": round(flops / (mk * 1e-3) / 1e12 / BF16_MFMA_PEAK_TFLOPS, 4),
           "composed_row_chunks": nchunks, "composed_hbm_gbytes": round(comp_bytes / 1e9, 2),
           "composed_hbm_gbs": round(comp_bytes / (mc * 1e-3) / 1e9, 1),
           "composed_frac_of_hbm_peak": round(comp_bytes / (mc * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
           "kernel_workspace_mbytes": round(_lib.lib().wavlm_lm_logprob_workspace_bytes(R, V) / 2 ** 20, 1),
           "max_abs_difference": diff}
    if a.layers > 0:
        del X
        cfg = dict(decoder_embed_dim=D, decoder_ffn_embed_dim=4 * D, decoder_layers=a.layers, decoder_attention_heads=D // 64,
                   share_decoder_input_output_embed=True)
        model = T.TransformerLM(cfg, V, max_tokens=R).to(torch.bfloat16).cuda()
        words = 40
        n = max(1, R // (words + 1))
        rng = torch.Generator().manual_seed(1)
        sents = torch.randint(4, V, (n, words), generator=rng).tolist()
        ts = {}
        for mode in ("0", "1"):
            os.environ["WAVLM_LM_LOGPROB_COMPOSED"] = mode
            model.score(sents[:8])
            model.score(sents)
            torch.cuda.synchronize()
            t = []
            for _ in range(3):
                t0 = time.perf_counter()
                model.score(sents)                             # ends in a device-to-host copy
                t.append((time.perf_counter() - t0) * 1e3)
            ts[mode] = statistics.median(t)
        out.update({"model_layers": a.layers, "model_sentences": n, "model_rows": n * (words + 1),
                    "model_score_ms": round(ts["0"], 1), "model_score_composed_ms": round(ts["1"], 1)})
    os.environ.pop("WAVLM_LM_LOGPROB_COMPOSED", None)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
