"""Generate tests/golden/speaker.npz: the reference's ECAPA-TDNN speaker head (downstreams/speaker_verification/models/
ecapa_tdnn.py) and its standalone WavLM (WavLM/WavLM.py) on the CPU, fp32.

Runs where the reference tree exists:  python tools/gen_speaker_golden.py [REFERENCE_ROOT]
(default REFERENCE_ROOT: $UNISPEECH_REF, else ../reference next to the repository).  The tests read only the .npz.

The reference file imports torchaudio.transforms and models/utils.py (s3prl, fairseq, omegaconf); none of them is reached by
the upstream path.  Inert stand-ins are registered for torchaudio, and models.utils is replaced by a stand-in UpstreamExpert
that returns prepared hidden states or wraps the reference's standalone WavLM with the reference's hook rule
(models/utils.py:49-56: the input of every encoder layer, transposed, then the encoder's output).

No weights are stored: every state dict is refilled from a seed (tests/test_speaker.py fill_state_dict, sorted-key order)
and the hidden states of the head cases come from make_states(seed, ...) there.  Contents:
  keys, key_shapes             the reference head's state-dict names / shapes (-1 padded)
  head768/*, head1024/*        seed_w, seed_x, shape [B, T, n, D]; emb, cos, normed_chk (ramp-weighted time sums of the
                               instance-normed features), out2_mean, out4_mean, pooled
  head768/emb_bf16_ref, e_ref, cos_err_bf16   the reference head in bf16 on the CPU on bf16-rounded states
  lengths/*                    three utterances of 149 / 100 / 61 frames, each ALONE through the reference
  e2e_tiny/*, e2e_tiny_preln/* int16 2 s crops of four vox1_data files, hidden-state checksums, emb, cos; upstream at the TINY
                               width (post-LN default extractor / pre-LN + layer_norm extractor + normalize)
"""
import os
import sys
import types
import wave

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from test_speaker import cos_matrix, fill_state_dict, make_states, offdiag, ramp  # noqa: E402

SEEDS = dict(head768=(101, 201), head1024=(102, 202), lengths=(101, 203), e2e_tiny=(111, 112), e2e_tiny_preln=(121, 122))
WAVS = ["David_Faustino/hn8GyCJIfLM_0000012.wav", "David_Faustino/xTOk1Jz-F_g_0000015.wav",
        "Josh_Gad/HXUqYaOwrxA_0000015.wav", "Josh_Gad/RFyw7V3SOnQ_0000001.wav"]


class _Layer(nn.Module):
    """what ecapa_tdnn.py:199-202 looks at in a 24-layer upstream"""

    def __init__(self):
        super().__init__()
        self.self_attn = nn.Identity()


class UpstreamExpert(nn.Module):
    """stand-in for models/utils.py UpstreamExpert.  spec = dict(states=[...]) or dict(wavlm=model, normalize=bool)"""

    def __init__(self, spec):
        super().__init__()
        self.spec = spec
        self.captured = []
        if "wavlm" in spec:
            self.model = spec["wavlm"]
            for layer in self.model.encoder.layers:
                layer.register_forward_hook(lambda m, i, o: self.captured.append(i[0].transpose(0, 1)))
            self.model.encoder.register_forward_hook(lambda m, i, o: self.captured.append(o[0]))
        else:
            self.model = nn.Module()
            self.model.encoder = nn.Module()
            self.model.encoder.layers = nn.ModuleList([_Layer() for _ in range(len(spec["states"]) - 1)])
            self.anchor = nn.Parameter(torch.zeros(1))

    def forward(self, wavs):
        if "states" in self.spec:
            return {"hidden_states": list(self.spec["states"])}
        if self.spec["normalize"]:
            wavs = [F.layer_norm(w, w.shape) for w in wavs]
        lens = torch.LongTensor([len(w) for w in wavs])
        mask = ~torch.lt(torch.arange(int(lens.max())).unsqueeze(0), lens.unsqueeze(1))
        padded = torch.nn.utils.rnn.pad_sequence(wavs, batch_first=True)
        self.captured = []
        self.model.extract_features(padded, padding_mask=mask, mask=None)
        return {"hidden_states": list(self.captured)}


def install(ref):
    for name in ("torchaudio", "torchaudio.transforms"):
        m = types.ModuleType(name)
        m.__path__ = []
        sys.modules.setdefault(name, m)
    sys.modules["torchaudio"].transforms = sys.modules["torchaudio.transforms"]
    sv = os.path.join(ref, "downstreams", "speaker_verification")
    sys.path.insert(0, sv)
    import models  # noqa: F401  (the reference's package; its utils module is replaced before ecapa_tdnn imports it)
    u = types.ModuleType("models.utils")
    u.UpstreamExpert = UpstreamExpert
    sys.modules["models.utils"] = u
    from models.ecapa_tdnn import ECAPA_TDNN_SMALL
    return ECAPA_TDNN_SMALL, sv


def head_keys(sd):
    return {k: v for k, v in sd.items() if not k.startswith("feature_extract.")}


def run_head(model, states, out, prefix):
    """states [n, B, T, D] fp32 -> reference outputs and intermediates under out[prefix + ...]"""
    model.feature_extract.spec["states"] = list(states.unbind(0))
    got = {}
    hooks = [model.instance_norm.register_forward_hook(lambda m, i, o: got.__setitem__("normed", o)),
             model.layer2.register_forward_hook(lambda m, i, o: got.__setitem__("out2", o)),
             model.layer4.register_forward_hook(lambda m, i, o: got.__setitem__("out4", o)),
             model.pooling.register_forward_hook(lambda m, i, o: got.__setitem__("pooled", o))]
    with torch.no_grad():
        emb = model(torch.zeros(states.shape[1], 16000))
    for h in hooks:
        h.remove()
    T = states.shape[2]
    out[prefix + "emb"] = emb.numpy()
    out[prefix + "cos"] = cos_matrix(emb.numpy()).astype(np.float32)
    out[prefix + "normed_chk"] = (got["normed"].double().numpy() * ramp(T)[None, None, :]).sum(-1).astype(np.float32)
    out[prefix + "out2_mean"] = got["out2"].mean(-1).numpy()
    out[prefix + "out4_mean"] = got["out4"].mean(-1).numpy()
    out[prefix + "pooled"] = got["pooled"].numpy()
    return emb


def read_crop(path, n=32000):
    with wave.open(path, "rb") as w:
        assert w.getsampwidth() == 2 and w.getnchannels() == 1 and w.getframerate() == 16000, path
        data = np.frombuffer(w.readframes(w.getnframes()), dtype="<i2")
    assert len(data) >= 16000 + n, (path, len(data))
    return data[16000:16000 + n].copy()


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("UNISPEECH_REF", os.path.join(os.path.dirname(ROOT), "reference"))
    ECAPA, sv = install(ref)
    sys.path.insert(0, os.path.join(ref, "WavLM"))
    import WavLM as ref_wavlm
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    from gen_golden import TINY
    torch.manual_seed(0)
    out = {}

    def build(D, states):
        m = ECAPA(feat_dim=D, emb_dim=256, feat_type="wavlm", config_path=dict(states=list(states.unbind(0))))
        return m.eval()

    for name, (B, T, n, D) in (("head768", (4, 149, 13, 768)), ("head1024", (2, 99, 25, 1024))):
        sw, sx = SEEDS[name]
        states = make_states(sx, B, T, n, D)
        m = build(D, states)
        hk = head_keys(m.state_dict())
        m.load_state_dict(fill_state_dict(hk, sw), strict=False)
        if name == "head768":
            keys = sorted(hk)
            out["keys"] = np.array(keys)
            out["key_shapes"] = np.array([list(hk[k].shape) + [-1] * (4 - hk[k].dim()) for k in keys], dtype=np.int64)
            print("head: %d entries, %.2f M parameters" % (len(keys), sum(v.numel() for v in hk.values()) / 1e6))
        emb = run_head(m, states, out, name + "/")
        out[name + "/seed_w"], out[name + "/seed_x"] = np.int64(sw), np.int64(sx)
        out[name + "/shape"] = np.array([B, T, n, D], dtype=np.int64)
        od = offdiag(out[name + "/cos"])
        print(name, "off-diagonal cosines %.3f .. %.3f" % (od.min(), od.max()))
        if name == "head768":
            assert od.max() - od.min() >= 0.3, "the cosines must spread: a head that ignores its input would pass"
            mb = build(D, states)
            mb.load_state_dict(fill_state_dict(hk, sw), strict=False)
            mb = mb.bfloat16()
            mb.feature_extract.spec["states"] = list(states.bfloat16().unbind(0))
            with torch.no_grad():
                eb = mb(torch.zeros(B, 16000)).float().numpy()
            out[name + "/emb_bf16_ref"] = eb
            e_ref = np.abs(eb - emb.numpy()).max() / np.abs(emb.numpy()).max()
            out[name + "/e_ref"] = np.float64(e_ref)
            out[name + "/cos_err_bf16"] = np.float64(np.abs(cos_matrix(eb) - cos_matrix(emb.numpy())).max())
            print("bf16 reference head on the CPU: e_ref %.3e, cosine error %.3e" % (e_ref, out[name + "/cos_err_bf16"]))
            # lengths: each utterance alone
            sw, sx = SEEDS["lengths"]
            frames = [149, 100, 61]
            full = make_states(sx, 3, 149, 13, 768)
            embs = []
            for b, L in enumerate(frames):
                m.feature_extract.spec["states"] = list(full[:, b:b + 1, :L].unbind(0))
                with torch.no_grad():
                    embs.append(m(torch.zeros(1, 16000))[0].numpy())
            out["lengths/emb"] = np.stack(embs)
            out["lengths/frames"] = np.array(frames, dtype=np.int64)
            out["lengths/seed_w"], out["lengths/seed_x"] = np.int64(sw), np.int64(sx)

    wavs = np.stack([read_crop(os.path.join(sv, "vox1_data", p)) for p in WAVS])
    for name, extra in (("e2e_tiny", {}),
                        ("e2e_tiny_preln", dict(layer_norm_first=True, extractor_mode="layer_norm", normalize=True))):
        s_up, s_head = SEEDS[name]
        cfgd = dict(TINY)
        cfgd.update(extra)
        up = ref_wavlm.WavLM(ref_wavlm.WavLMConfig(cfgd)).eval()
        up.load_state_dict(fill_state_dict(up.state_dict(), s_up))
        m = ECAPA(feat_dim=64, emb_dim=256, feat_type="wavlm",
                  config_path=dict(wavlm=up, normalize=bool(cfgd.get("normalize", False)))).eval()
        m.load_state_dict(fill_state_dict(head_keys(m.state_dict()), s_head), strict=False)
        x = torch.from_numpy(wavs.astype(np.float32) / 32768.0)
        with torch.no_grad():
            hs = m.feature_extract([w for w in x])["hidden_states"]
            emb = m(x).numpy()
        assert len(hs) == 3 and hs[0].shape == (4, 99, 64), [h.shape for h in hs]
        out[name + "/wav_i16"] = wavs
        out[name + "/hs_chk"] = np.stack([(h.double().numpy() * ramp(99)[None, :, None]).sum(1) for h in hs]).astype(np.float32)
        out[name + "/hs_max"] = np.array([float(h.abs().max()) for h in hs])
        out[name + "/emb"] = emb
        out[name + "/cos"] = cos_matrix(emb).astype(np.float32)
        out[name + "/seed_up"], out[name + "/seed_head"] = np.int64(s_up), np.int64(s_head)
        out[name + "/cfg_keys"] = np.array(sorted(extra))
        out[name + "/cfg_vals"] = np.array([str(extra[k]) for k in sorted(extra)])
        print(name, "cosines", np.round(offdiag(out[name + "/cos"]), 3))
    path = os.path.join(ROOT, "tests", "golden", "speaker.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
