"""Diarization head on one GPU, one process, bf16: (a) the HIP head (unispeech_amd/diarization.py estimate_states), also under
frozen_parameters(), (b) the reference's formula written in plain torch on the same tensors, batched (the baseline of the
ratio) and one chunk per call (the reference's own loop, diarization.py:182-205), (c) each csrc/diar.hip kernel alone with its
achieved GB/s or TF/s against algorithmic bytes / flops, and the FFN's ReLU pass (wavlm_spk_rowact over [B * T, 2048]), at
Base (13 states [20, 1499, 768]) and Large (25 states [20, 1499, 1024]): a 10-minute recording in 30 s chunks.  With --upstream
also one extract_features call at Base width on the same chunks, for the head's share of a whole call.

    python tools/diarization_bench.py [--reps 20] [--upstream]
Prints one JSON object.  Run it as three processes and report the spread."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as TF

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from unispeech_amd import _lib, ops  # noqa: E402
from unispeech_amd import functional as F  # noqa: E402
from unispeech_amd.diarization import TransformerDiarization  # noqa: E402

HEAD = dict(n_speakers=3, all_n_speakers=1, n_units=256, n_heads=8, n_layers=6, spk_emb_dim=256, sr=8000, frame_shift=320)


def timed(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def torch_formula(m, states, frames):
    """models.py get_feat + forward + estimate and transformer.py restated with torch ops on m's parameters (eval mode)"""
    x = (TF.softmax(m.feature_weight, -1).view(-1, 1, 1, 1) * torch.stack(states, 0)).sum(0)
    x = TF.instance_norm(x.transpose(1, 2) + 1e-6, eps=1e-5)
    x = TF.interpolate(x[:, :, ::m.subsampling], frames, mode="linear").transpose(1, 2)
    B, T, _ = x.shape
    enc, H = m.enc, m.n_heads
    e = TF.linear(x.reshape(B * T, -1), enc.linear_in.weight, enc.linear_in.bias)
    for i in range(enc.n_layers):
        ln1, ln2 = getattr(enc, "lnorm1_%d" % i), getattr(enc, "lnorm2_%d" % i)
        a, ff = getattr(enc, "self_att_%d" % i), getattr(enc, "ff_%d" % i)
        e = TF.layer_norm(e, ln1.normalized_shape, ln1.weight, ln1.bias, ln1.eps)
        q, k, v = (TF.linear(e, l.weight, l.bias).reshape(B, T, H, -1) for l in (a.linearQ, a.linearK, a.linearV))
        s = torch.matmul(q.transpose(1, 2), k.permute(0, 2, 3, 1)) / (q.shape[-1] ** 0.5)
        o = torch.matmul(TF.softmax(s, dim=3), v.transpose(1, 2)).transpose(1, 2).reshape(B * T, -1)
        e = e + TF.linear(o, a.linearO.weight, a.linearO.bias)
        e = TF.layer_norm(e, ln2.normalized_shape, ln2.weight, ln2.bias, ln2.eps)
        e = e + TF.linear(TF.relu(TF.linear(e, ff.linear1.weight, ff.linear1.bias)), ff.linear2.weight, ff.linear2.bias)
    e = TF.layer_norm(e, enc.lnorm_out.normalized_shape, enc.lnorm_out.weight, enc.lnorm_out.bias, enc.lnorm_out.eps)
    z = torch.sigmoid(TF.linear(e, m.linear.weight, m.linear.bias).reshape(B, T, -1))
    vecs = []
    for s_ in range(m.n_speakers):
        lin = getattr(m, "linear%d" % s_)
        v = TF.linear(e, lin.weight, lin.bias).reshape(B, T, -1)
        v = (v / torch.norm(v, dim=2, keepdim=True) * z[:, :, s_:s_ + 1]).sum(1)
        vecs.append(v / torch.norm(v, dim=1, keepdim=True))
    return z, torch.stack(vecs, 1)


def kernels(B, Tp, T, D, n, reps):
    bf = torch.bfloat16
    r = {}
    states = [torch.randn(B, Tp, D, device="cuda").to(bf) for _ in range(n)]
    w = torch.softmax(torch.randn(n, device="cuda"), 0)
    out = torch.empty(B, T, D, device="cuda", dtype=bf)
    ms = timed(lambda: ops.diar_front(states, w, T, out=out), reps)
    r["front"] = {"ms": round(ms, 4), "GBps": round((n * Tp + T) * B * D * 2 / ms / 1e6, 1)}
    del states, out
    H, d = 8, 32
    qkv = torch.randn(B, T, 3 * H * d, device="cuda").to(bf)
    ms = timed(lambda: ops.attn_plain_fwd(qkv, H), reps)
    r["attn_plain"] = {"ms": round(ms, 4), "tflops": round(4.0 * B * H * T * T * d / ms / 1e9, 2)}
    S, E = 3, 256
    z = torch.randn(B, T, S + S * E, device="cuda").to(bf)
    ms = timed(lambda: ops.diar_estimate(z, S, E), reps)
    r["estimate"] = {"ms": round(ms, 4), "GBps": round(B * T * (S + S * E) * 2 / ms / 1e6, 1)}
    h = torch.randn(B * T, 2048, device="cuda").to(bf)
    L = _lib.lib()
    ms = timed(lambda: L.wavlm_spk_rowact(ops.ptr(h), 1, B * T * 2048, 2048, ops.ptr(h), 1, B * T * 2048, 2048, 1, B * T, 2048, 0,
                                          None, None, None, None, ops.stream()), reps)
    r["ffn_relu_rowact"] = {"ms": round(ms, 4), "GBps": round(2 * B * T * 2048 * 2 / ms / 1e6, 1)}
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--upstream", action="store_true")
    a = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0), "dtype": "bf16", "shapes": []}
    torch.manual_seed(0)
    B, Tp, T = 20, 1499, 750
    for name, D, n in (("base", 768, 13), ("large", 1024, 25)):
        m = TransformerDiarization(feat_dim=D, num_states=n, **HEAD)
        for p in m.parameters():
            if p.dim() > 1:
                torch.nn.init.normal_(p, std=(1.0 / p[0].numel()) ** 0.5)
        m = m.to(torch.bfloat16).cuda().eval()
        states = [torch.randn(B, Tp, D, device="cuda").bfloat16() for _ in range(n)]
        with torch.no_grad():
            head = timed(lambda: m.estimate_states(states, T), a.reps)
            with F.frozen_parameters():
                head_cached = timed(lambda: m.estimate_states(states, T), a.reps)
            ref = timed(lambda: torch_formula(m, states, T), a.reps)
            per_chunk = [[s[b:b + 1] for s in states] for b in range(B)]
            loop = timed(lambda: [torch_formula(m, c, T) for c in per_chunk], max(2, a.reps // 4))
        rec = {"name": name, "B": B, "T_up": Tp, "T": T, "D": D, "states": n, "head_ms": round(head, 3),
               "head_frozen_parameters_ms": round(head_cached, 3), "torch_formula_batched_ms": round(ref, 3),
               "torch_formula_chunk_loop_ms": round(loop, 3), "ratio": round(ref / head, 2),
               "ratio_frozen_parameters": round(ref / head_cached, 2), "ratio_chunk_loop": round(loop / head, 2)}
        del states, per_chunk
        rec["kernels"] = kernels(B, Tp, T, D, n, a.reps)
        out["shapes"].append(rec)
    if a.upstream:
        from unispeech_amd.wavlm import WavLM, WavLMConfig
        up = WavLM(WavLMConfig(dict(relative_position_embedding=True, gru_rel_pos=True, num_buckets=320, max_distance=800)))
        up = up.to(torch.bfloat16).cuda().eval()
        wav = torch.randn(B, 480000, device="cuda").bfloat16()
        with torch.no_grad():
            ms = timed(lambda: up.extract_features(wav), 5)
        out["extract_features_base_20x30s_ms"] = round(ms, 3)
        for key in ("head_ms", "head_frozen_parameters_ms"):
            h = out["shapes"][0][key]
            out["share_of_call_" + key[:-3]] = round(h / (ms + h), 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
