"""Speaker head on one GPU, one process, bf16: (a) the HIP head (unispeech_amd/speaker.py forward_states), (b) the reference's
formula written in plain torch on the same tensors (stack, weighted sum, transpose, InstanceNorm1d, conv1d / batch_norm /
relu chain, softmax pooling), and each spkhead.hip kernel alone with its achieved GB/s against algorithmic bytes (TF/s for
the Res2 chain), at Base (32 x 15 s: 13 states [32, 749, 768]) and Large (25 states [16, 999, 1024]).  With --upstream also
the time of one extract_features call at Base width, for the head's share of a whole call.

    python tools/speaker_bench.py [--reps 20] [--upstream]
Prints one JSON object."""
import argparse
import ctypes as C
import json
import os
import sys

import torch
import torch.nn.functional as TF

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from unispeech_amd import _lib, ops  # noqa: E402
from unispeech_amd import functional as F  # noqa: E402
from unispeech_amd.speaker import ECAPA_TDNN_SMALL  # noqa: E402


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


def torch_formula(m, states):
    """ecapa_tdnn.py get_feat + forward restated with torch ops on m's parameters (eval mode)"""
    def crb(x, c, dil=1, pad=0):
        return TF.batch_norm(TF.relu(TF.conv1d(x, c.conv.weight, c.conv.bias, padding=pad, dilation=dil)), c.bn.running_mean,
                             c.bn.running_var, c.bn.weight, c.bn.bias, False, 0.0, c.bn.eps)

    x = (TF.softmax(m.feature_weight, -1).view(-1, 1, 1, 1) * torch.stack(states, 0)).sum(0)
    x = TF.instance_norm(x.transpose(1, 2) + 1e-6, eps=1e-5)
    out = crb(x, m.layer1, pad=2)
    outs = []
    for blk in (m.layer2, m.layer3, m.layer4):
        res, d = out, blk.dilation
        x = crb(out, blk.Conv1dReluBn1)
        r2, sp, ys = blk.Res2Conv1dReluBn, None, []
        spx = torch.split(x, 64, 1)
        for i in range(7):
            sp = spx[i] if i == 0 else sp + spx[i]
            b = r2.bns[i]
            sp = TF.batch_norm(TF.relu(TF.conv1d(sp, r2.convs[i].weight, r2.convs[i].bias, padding=d, dilation=d)),
                               b.running_mean, b.running_var, b.weight, b.bias, False, 0.0, b.eps)
            ys.append(sp)
        ys.append(spx[7])
        x = crb(torch.cat(ys, 1), blk.Conv1dReluBn2)
        se = blk.SE_Connect
        g = torch.sigmoid(TF.linear(TF.relu(TF.linear(x.mean(2), se.linear1.weight, se.linear1.bias)), se.linear2.weight,
                                    se.linear2.bias))
        out = x * g.unsqueeze(2) + res
        outs.append(out)
    x = TF.relu(TF.conv1d(torch.cat(outs, 1), m.conv.weight, m.conv.bias))
    a = torch.tanh(TF.conv1d(x, m.pooling.linear1.weight, m.pooling.linear1.bias))
    a = torch.softmax(TF.conv1d(a, m.pooling.linear2.weight, m.pooling.linear2.bias), dim=2)
    mean = (a * x).sum(2)
    std = torch.sqrt(((a * x * x).sum(2) - mean * mean).clamp(min=1e-9))
    p = TF.batch_norm(torch.cat([mean, std], 1), m.bn.running_mean, m.bn.running_var, m.bn.weight, m.bn.bias, False, 0.0, m.bn.eps)
    return TF.linear(p, m.linear.weight, m.linear.bias)


def kernels(B, T, D, n, reps):
    L, st, P = _lib.lib(), ops.stream, lambda t: C.c_void_p(t.data_ptr())
    bf = torch.bfloat16
    r = {}
    states = [torch.randn(B, T, D, device="cuda").to(bf) for _ in range(n)]
    w = torch.softmax(torch.randn(n, device="cuda"), 0)
    out = torch.zeros(B, T + 4, D, device="cuda", dtype=bf)
    ptrs = (C.c_void_p * n)(*[s.data_ptr() for s in states])
    sb, stt = (C.c_int64 * n)(*[T * D] * n), (C.c_int64 * n)(*[D] * n)
    ms = timed(lambda: L.wavlm_spk_mix_norm(ptrs, sb, stt, n, 1, P(w), None, B, T, D, ops.ptr(out, 2 * D), 1, (T + 4) * D, D, 2,
                                            1e-6, 1e-5, st()), reps)
    r["mix_norm"] = {"ms": round(ms, 4), "GBps": round((n + 1) * B * T * D * 2 / ms / 1e6, 1)}
    del states, out
    x, y = torch.randn(B, T, 512, device="cuda").to(bf), torch.empty(B, T, 512, device="cuda", dtype=bf)
    img, v = torch.randn(7, 3, 64, 64, device="cuda") / 14, torch.rand(7, 64, device="cuda")
    for d in (2, 4):
        ms = timed(lambda: L.wavlm_spk_res2(P(x), 1, T * 512, 512, P(y), 1, T * 512, 512, B, T, 512, d, P(img), P(v), P(v), P(v),
                                            None, st()), reps)
        r["res2_d%d" % d] = {"ms": round(ms, 4), "tflops": round(7 * 2 * 192 * 64 * B * T / ms / 1e9, 2),
                             "GBps": round(2 * B * T * 512 * 2 / ms / 1e6, 1)}
    mean, sc = torch.empty(B, 512, device="cuda"), torch.rand(512, device="cuda")
    ms = timed(lambda: L.wavlm_spk_rowact(P(x), 1, T * 512, 512, P(y), 1, T * 512, 512, B, T, 512, 0, P(sc), P(sc), None, P(mean),
                                          st()), reps)
    r["rowact_mean_512"] = {"ms": round(ms, 4), "GBps": round(2 * B * T * 512 * 2 / ms / 1e6, 1)}
    ms = timed(lambda: L.wavlm_spk_rowact(P(x), 1, T * 512, 512, P(y), 1, T * 512, 512, B, T, 512, 0, P(sc), P(sc), None, None,
                                          st()), reps)
    r["rowact_512"] = {"ms": round(ms, 4), "GBps": round(2 * B * T * 512 * 2 / ms / 1e6, 1)}
    w1, w2 = torch.randn(128, 512, device="cuda").to(bf) / 22, torch.randn(512, 128, device="cuda").to(bf) / 11
    b1, b2 = torch.zeros(128, device="cuda", dtype=bf), torch.zeros(512, device="cuda", dtype=bf)
    nb = L.wavlm_spk_se_workspace_bytes(B, 512)
    ws, res = torch.empty(nb, dtype=torch.uint8, device="cuda"), torch.randn(B, T, 512, device="cuda").to(bf)
    ms = timed(lambda: L.wavlm_spk_se_residual(P(x), 1, T * 512, 512, P(mean), P(w1), P(b1), P(w2), P(b2), 1, P(res), 1, T * 512,
                                               512, P(y), 1, T * 512, 512, B, T, 512, 128, None, P(ws), nb, st()), reps)
    r["se_residual"] = {"ms": round(ms, 4), "GBps": round(3 * B * T * 512 * 2 / ms / 1e6, 1)}
    x, lg = torch.randn(B, T, 1536, device="cuda").to(bf), torch.randn(B, T, 1536, device="cuda").to(bf)
    po = torch.empty(B, 3072, device="cuda", dtype=bf)
    ms = timed(lambda: L.wavlm_spk_asp(P(x), 1, T * 1536, 1536, P(lg), 1, T * 1536, 1536, B, T, 1536, None, None, None, None, P(po),
                                       1, st()), reps)
    r["asp"] = {"ms": round(ms, 4), "GBps": round(2 * B * T * 1536 * 2 / ms / 1e6, 1)}
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--upstream", action="store_true")
    a = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0), "dtype": "bf16", "shapes": []}
    torch.manual_seed(0)
    for name, B, T, D, n in (("base", 32, 749, 768, 13), ("large", 16, 999, 1024, 25)):
        m = ECAPA_TDNN_SMALL(D, num_states=n)
        for p in m.parameters():
            if p.dim() > 1:
                torch.nn.init.normal_(p, std=(1.0 / p[0].numel()) ** 0.5)
        m = m.to(torch.bfloat16).cuda().eval()
        states = [torch.randn(B, T, D, device="cuda").bfloat16() for _ in range(n)]
        with torch.no_grad():
            head = timed(lambda: m.forward_states(states), a.reps)
            with F.frozen_parameters():
                head_cached = timed(lambda: m.forward_states(states), a.reps)
            ref = timed(lambda: torch_formula(m, states), a.reps)
        rec = {"name": name, "B": B, "T": T, "D": D, "states": n, "head_ms": round(head, 3),
               "head_frozen_parameters_ms": round(head_cached, 3), "torch_formula_ms": round(ref, 3),
               "ratio": round(ref / head, 2), "ratio_frozen_parameters": round(ref / head_cached, 2)}
        del states
        rec["kernels"] = kernels(B, T, D, n, a.reps)
        out["shapes"].append(rec)
    if a.upstream:
        from unispeech_amd.wavlm import WavLM, WavLMConfig
        up = WavLM(WavLMConfig(dict(relative_position_embedding=True, gru_rel_pos=True, num_buckets=320, max_distance=800)))
        up = up.to(torch.bfloat16).cuda().eval()
        wav = torch.randn(32, 240000, device="cuda").bfloat16()
        with torch.no_grad():
            ms = timed(lambda: up.extract_features(wav), 5)
        out["extract_features_base_32x15s_ms"] = round(ms, 3)
        for key in ("head_ms", "head_frozen_parameters_ms"):
            h = out["shapes"][0][key]
            out["share_of_call_" + key[:-3]] = round(h / (ms + h), 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
