"""Generate tests/golden/speaker_fbank.npz: the reference's ECAPA_TDNN_SMALL(feat_dim=40, feat_type='fbank')
(downstreams/speaker_verification/models/ecapa_tdnn.py, verification.py's `ecapa_tdnn`) on the CPU, fp32.

Runs where the reference tree exists:  python tools/gen_speaker_fbank_golden.py [REFERENCE_ROOT]
(default REFERENCE_ROOT: $UNISPEECH_REF, else ../reference next to the repository).  The tests read only the .npz.

The reference file imports torchaudio.transforms and models/utils.py (s3prl, fairseq, omegaconf); neither is installed.
models.utils gets an inert stand-in (the fbank model never touches it).  torchaudio.transforms.MelSpectrogram is THIS file's
small module, written from torchaudio 0.9's published source: `torch.stft` (what its Spectrogram calls) with a periodic Hann
window, |.|^2, and create_fb_matrix's HTK triangles evaluated in fp32 torch as torchaudio evaluates them; buffers named as
torchaudio names them (spectrogram.window, mel_scale.fb).  torchaudio itself was never run.

No weights and no waveforms are stored: the state dict is refilled from a seed (tests/test_speaker.py fill_state_dict, head
keys only) and the waveforms from tests/fbank_cases.py golden_waves(seed).  Contents:
  keys, key_shapes         the reference model's state-dict names / shapes (-1 padded), feature_extract.* included
  seed_w, seed_x, lengths  four utterances of unequal length, two per speaker, each ALONE through the reference
  emb, cos                 embeddings [4, 256], cosine matrix; normed_chk: ramp-weighted time sums of the instance-normed
                           log-mel features [4, 40]
  emb_bf16_ref, e_ref, cos_err_bf16   the reference head in bf16 on the CPU on the bf16-rounded normed features (front end and
                           instance norm in fp32, as this project's bf16 mode runs them)
"""
import math
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from fbank_cases import GOLDEN_LENGTHS, golden_waves  # noqa: E402
from test_speaker import cos_matrix, fill_state_dict, offdiag, ramp  # noqa: E402

SEED_W, SEED_X = 131, 231


def fb_matrix(n_freqs, f_min, f_max, n_mels, sample_rate):
    """torchaudio.functional.create_fb_matrix (norm None, HTK), in torch's default dtype like the original"""
    all_freqs = torch.linspace(0, sample_rate // 2, n_freqs)
    m_min = 2595.0 * math.log10(1.0 + f_min / 700.0)
    m_max = 2595.0 * math.log10(1.0 + f_max / 700.0)
    m_pts = torch.linspace(m_min, m_max, n_mels + 2)
    f_pts = 700.0 * (10 ** (m_pts / 2595.0) - 1.0)
    f_diff = f_pts[1:] - f_pts[:-1]
    slopes = f_pts.unsqueeze(0) - all_freqs.unsqueeze(1)
    down = (-1.0 * slopes[:, :-2]) / f_diff[:-1]
    up = slopes[:, 2:] / f_diff[1:]
    return torch.max(torch.zeros(1), torch.min(down, up))


class MelSpectrogram(nn.Module):
    """stand-in for torchaudio.transforms.MelSpectrogram at the defaults the reference leaves alone"""

    def __init__(self, sample_rate=16000, n_fft=400, win_length=None, hop_length=None, f_min=0.0, f_max=None, pad=0, n_mels=128):
        super().__init__()
        assert pad == 0
        self.n_fft = n_fft
        self.win_length = n_fft if win_length is None else win_length
        self.hop_length = self.win_length // 2 if hop_length is None else hop_length
        self.spectrogram, self.mel_scale = nn.Module(), nn.Module()
        self.spectrogram.register_buffer("window", torch.hann_window(self.win_length))
        f_max = float(sample_rate // 2) if f_max is None else float(f_max)
        self.mel_scale.register_buffer("fb", fb_matrix(n_fft // 2 + 1, f_min, f_max, n_mels, sample_rate))

    def forward(self, wav):
        spec = torch.stft(wav.float(), self.n_fft, self.hop_length, self.win_length, self.spectrogram.window.float(), center=True,
                          pad_mode="reflect", normalized=False, onesided=True, return_complex=True)
        power = spec.abs().pow(2.0)                                          # [B, n_fft / 2 + 1, T]
        return torch.matmul(power.transpose(1, 2), self.mel_scale.fb.float()).transpose(1, 2)


def install(ref):
    ta, tr = types.ModuleType("torchaudio"), types.ModuleType("torchaudio.transforms")
    ta.__path__ = []
    tr.MelSpectrogram = MelSpectrogram
    ta.transforms = tr
    sys.modules["torchaudio"], sys.modules["torchaudio.transforms"] = ta, tr
    sv = os.path.join(ref, "downstreams", "speaker_verification")
    sys.path.insert(0, sv)
    import models  # noqa: F401  (the reference's package; its utils module is replaced before ecapa_tdnn imports it)
    u = types.ModuleType("models.utils")
    u.UpstreamExpert = None
    sys.modules["models.utils"] = u
    from models.ecapa_tdnn import ECAPA_TDNN_SMALL
    return ECAPA_TDNN_SMALL


def head_keys(sd):
    return {k: v for k, v in sd.items() if not k.startswith("feature_extract.")}


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("UNISPEECH_REF", os.path.join(os.path.dirname(ROOT), "reference"))
    ECAPA = install(ref)
    torch.manual_seed(0)
    out = {}

    def build():
        m = ECAPA(feat_dim=40, emb_dim=256, feat_type="fbank").eval()
        m.load_state_dict(fill_state_dict(head_keys(m.state_dict()), SEED_W), strict=False)
        return m

    m = build()
    sd = m.state_dict()
    keys = sorted(sd)
    out["keys"] = np.array(keys)
    out["key_shapes"] = np.array([list(sd[k].shape) + [-1] * (4 - sd[k].dim()) for k in keys], dtype=np.int64)
    assert "feature_weight" not in keys
    print("model: %d entries, %.2f M head parameters" % (len(keys), sum(v.numel() for v in head_keys(sd).values()) / 1e6))

    # the bf16 reference: head modules in bf16, front end and instance norm in fp32, the normed features rounded to bf16
    mb = build()
    for name, child in mb.named_children():
        if name not in ("feature_extract", "instance_norm"):
            child.bfloat16()
    mb.instance_norm.register_forward_hook(lambda mod, i, o: o.bfloat16())

    waves = golden_waves(SEED_X)
    embs, embs_b, chk = [], [], []
    got = {}
    m.instance_norm.register_forward_hook(lambda mod, i, o: got.__setitem__("normed", o))
    for w in waves:
        x = torch.from_numpy(w)[None]
        with torch.no_grad():
            embs.append(m(x)[0].numpy())
            embs_b.append(mb(x)[0].float().numpy())
        n = got["normed"][0].double().numpy()                                  # [40, T]
        assert n.shape == (40, 1 + len(w) // 160), n.shape
        chk.append((n * ramp(n.shape[1])[None, :]).sum(-1))
    emb, eb = np.stack(embs), np.stack(embs_b)
    out["emb"], out["cos"] = emb, cos_matrix(emb).astype(np.float32)
    out["normed_chk"] = np.stack(chk).astype(np.float32)
    out["seed_w"], out["seed_x"] = np.int64(SEED_W), np.int64(SEED_X)
    out["lengths"] = np.array(GOLDEN_LENGTHS, dtype=np.int64)
    od = offdiag(out["cos"])
    print("off-diagonal cosines %.3f .. %.3f" % (od.min(), od.max()), np.round(out["cos"], 3))
    # a model that ignores its input scores 1 everywhere: with every pair at least 0.1 below that and the pairs 0.1 apart, the
    # tests' 1e-3 on the cosine tells the two apart a hundred times over
    assert od.max() <= 0.9 and od.max() - od.min() >= 0.1, "the cosines must stay clear of 1 and spread"
    out["emb_bf16_ref"] = eb
    out["e_ref"] = np.float64(np.abs(eb - emb).max() / np.abs(emb).max())
    out["cos_err_bf16"] = np.float64(np.abs(cos_matrix(eb) - cos_matrix(emb)).max())
    print("bf16 reference head on the CPU: e_ref %.3e, cosine error %.3e" % (out["e_ref"], out["cos_err_bf16"]))
    path = os.path.join(ROOT, "tests", "golden", "speaker_fbank.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
