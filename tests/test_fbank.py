"""Log-mel front end, host side (unispeech_amd/fbank.py, the fbank mode of unispeech_amd/speaker.py): the restatement against
torch.stft, the mel bank against a dense evaluation written another way, frame counts, refusals, the fbank speaker model's
state dict against tests/golden/speaker_fbank.npz (tools/gen_speaker_fbank_golden.py) and the command line.  No GPU."""
import os

import numpy as np
import pytest
import torch

from conftest import load_golden

import fbank_cases as FC


def g():
    return load_golden("speaker_fbank.npz")


# --------------------------------------------------------------------------------------------------- against torch.stft
@pytest.mark.parametrize("L", [257, 400, 1600, 16037])
def test_power_spectrum_equals_torch_stft(L):
    """reflection, window centring and frame count, pinned by torch.stft (what torchaudio's Spectrogram calls) in float64"""
    from unispeech_amd.fbank import fbank_reference, frames
    x = FC.signal(L, 3).astype(np.float64) / 32768.0
    spec = torch.stft(torch.from_numpy(x), 512, 160, 400, torch.hann_window(400, dtype=torch.float64), center=True,
                      pad_mode="reflect", normalized=False, onesided=True, return_complex=True)
    want = (spec.real ** 2 + spec.imag ** 2).T.numpy()                       # [T, 257]
    got = fbank_reference(x, power=True)
    assert got.shape == want.shape == (frames(L), 257) == (1 + L // 160, 257)
    err = np.abs(got - want).max() / want.max()
    print("L=%d: power spectrum against torch.stft, relative error %.2e" % (L, err))
    assert err <= 1e-9
    # and through the mel bank and the log
    from unispeech_amd.fbank import mel_bank
    lm = np.log(want @ mel_bank(16000, 512, 40) + 1e-6)
    assert np.abs(fbank_reference(x) - lm).max() <= 1e-9 * np.abs(lm).max()


def test_float32_reference_is_float32_throughout():
    from unispeech_amd.fbank import fbank_reference
    x = FC.signal(1600, 3).astype(np.float64) / 32768.0
    r32, r64 = fbank_reference(x, dtype=np.float32), fbank_reference(x, dtype=np.float64)
    assert r32.dtype == np.float32 and r64.dtype == np.float64
    e = np.abs(r32 - r64).max()
    assert 0 < e < 1e-4, e
    with pytest.raises(TypeError):
        fbank_reference(x, dtype=np.float16)
    assert fbank_reference(x[:256]).shape == (0, 40)


# ------------------------------------------------------------------------------------------------------------ mel bank
def dense_bank(sr, P, M):
    """fb[k, m] of the statement, one scalar at a time"""
    mel = lambda f: 2595.0 * np.log10(1.0 + f / 700.0)
    hz = lambda m: 700.0 * (10.0 ** (m / 2595.0) - 1.0)
    top = float(sr // 2)
    pts = [hz(mel(0.0) + i * (mel(top) - mel(0.0)) / (M + 1)) for i in range(M + 2)]
    fb = np.zeros((P // 2 + 1, M))
    for k in range(P // 2 + 1):
        f = top * k / (P // 2)
        for m in range(M):
            fb[k, m] = max(0.0, min((f - pts[m]) / (pts[m + 1] - pts[m]), (pts[m + 2] - f) / (pts[m + 2] - pts[m + 1])))
    return fb


@pytest.mark.parametrize("M", [40, 80, 128])
def test_mel_bank(M):
    """A filter is empty when no bin lies strictly inside its two mel steps.  The lowest filter is 2 * 0.6214 Hz / mel *
    2840.02 mel / (M + 1) wide: 86.1 Hz at M = 40, 43.6 Hz at M = 80 -- both above the 31.25 Hz between bins, so neither bank has
    an empty filter (the M = 80 bank was expected to; it does not, by this arithmetic and by the dense evaluation below) -- and
    27.4 Hz at M = 128, the kernel's limit, where a filter that falls between two bins is empty and gives the constant column
    log(1e-6)."""
    from unispeech_amd.fbank import fbank_reference, mel_bank, tables
    fb = mel_bank(16000, 512, M)
    assert fb.shape == (257, M) and fb.min() >= 0 and fb.max() <= 1
    assert ((fb > 0).sum(1) <= 2).all()                                       # every bin under at most two filters
    assert (fb[0] == 0).all() and (fb[256] == 0).all()                        # bin 0 and the Nyquist bin weigh nothing
    assert np.abs(fb - dense_bank(16000, 512, M)).max() <= 1e-9
    t = tables(16000, 512, 400, M)
    idx, w = t["mel_idx"], t["mel_w"]
    assert idx.shape == (M, 3) and idx.dtype == np.int32 and len(w) == idx[:, 1].sum() <= 510
    back = np.zeros_like(fb)
    for m, (first, count, off) in enumerate(idx):
        assert first + count <= 256                                           # what the kernel's bins k < P / 2 hold
        back[first:first + count, m] = w[off:off + count]
    assert np.array_equal(back, fb)
    empty = [m for m in range(M) if idx[m, 1] == 0]
    assert (fb.sum(0) == 0).nonzero()[0].tolist() == empty
    if M <= 80:
        assert not empty
    else:
        assert empty and max(empty) < 40
        x = FC.signal(1600, 3).astype(np.float64) / 32768.0
        lm = fbank_reference(x, n_mels=M)
        assert (lm[:, empty] == np.log(1e-6)).all() and (np.delete(lm, empty, 1) > np.log(1e-6) + 1).all()


def test_window_and_twiddles():
    from unispeech_amd.fbank import tables
    t = tables(16000, 512, 400, 40)
    assert np.allclose(t["window"], torch.hann_window(400, dtype=torch.float64).numpy(), atol=1e-15)
    k = np.arange(512)
    assert np.allclose(t["twiddle"][:, 0] + 1j * t["twiddle"][:, 1], np.exp(-2j * np.pi * k / 512), atol=1e-15)


# -------------------------------------------------------------------------------------------------- frames and refusals
def test_frame_counts():
    from unispeech_amd import _lib
    from unispeech_amd.fbank import frames
    lib = _lib.lib()
    for n, want in ((256, 0), (257, 2), (319, 2), (320, 3), (16000, 101), (0, 0)):
        assert frames(n, 160, 512) == lib.wavlm_fbank_frames(n, 160, 512) == want, n
    assert lib.wavlm_fbank_frames(-5, 160, 512) == 0 and lib.wavlm_fbank_frames(1000, 0, 512) == -1


def test_supported_geometries():
    from unispeech_amd import _lib
    sup = _lib.lib().wavlm_fbank_supported
    assert sup(400, 160, 512, 40) == 1 and sup(400, 160, 512, 128) == 1 and sup(200, 80, 256, 40) == 1 and sup(64, 1, 64, 1) == 1
    assert sup(400, 160, 1024, 40) == 0 and sup(800, 160, 1024, 40) == 0      # P = 1024
    assert sup(400, 160, 512, 129) == 0 and sup(400, 160, 512, 0) == 0        # M
    assert sup(256, 160, 512, 40) == 0 and sup(513, 160, 512, 40) == 0        # W <= P / 2, W > P
    assert sup(400, 0, 512, 40) == 0 and sup(400, 401, 512, 40) == 0          # S
    assert sup(400, 160, 500, 40) == 0 and sup(30, 10, 32, 8) == 0            # not a power of two, below 64
    assert sup(512, 512, 512, 40) == 0                                        # 55 * 512 + 512 samples do not fit the LDS budget


def test_options_are_refused_by_name():
    from unispeech_amd.fbank import check_options, fbank
    check_options(16000, power=2.0, center=True, pad_mode="reflect", norm=None, mel_scale="htk", normalized=False,
                  window_fn=torch.hann_window, f_min=0.0, f_max=8000, pad=0)
    check_options(16000, f_max=None, power=2)
    for kw, word in ((dict(power=1.0), "power"), (dict(center=False), "center"), (dict(pad_mode="constant"), "pad_mode"),
                     (dict(norm="slaney"), "norm"), (dict(mel_scale="slaney"), "mel_scale"), (dict(normalized=True), "normalized"),
                     (dict(window_fn=torch.hamming_window), "window_fn"), (dict(f_min=20.0), "f_min"), (dict(f_max=7600.0), "f_max"),
                     (dict(pad=1), "pad"), (dict(pad=1, power=1.0), "power"), (dict(f_max=7600.0, norm="slaney"), "norm=")):
        with pytest.raises(NotImplementedError, match=word):
            check_options(16000, **kw)
    with pytest.raises(TypeError, match="top_db"):
        check_options(16000, top_db=80.0)
    with pytest.raises(NotImplementedError, match="power"):     # before any tensor is looked at
        fbank(None, power=1.0)
    with pytest.raises(NotImplementedError, match="n_fft=1024"):
        fbank(None, n_fft=1024, win_length=1024)
    with pytest.raises(NotImplementedError, match="n_mels=129"):
        fbank(None, n_mels=129)


# ------------------------------------------------------------------------------------------------------------ the model
def test_fixture_integrity():
    z = g()
    keys = [str(k) for k in z["keys"]]
    assert "feature_weight" not in keys and "layer3.Res2Conv1dReluBn.convs.4.weight" in keys
    assert [k for k in keys if k.startswith("feature_extract.")] == ["feature_extract.mel_scale.fb", "feature_extract.spectrogram.window"]
    assert z["emb"].shape == (4, 256) and z["cos"].shape == (4, 4) and z["normed_chk"].shape == (4, 40)
    assert [int(v) for v in z["lengths"]] == list(FC.GOLDEN_LENGTHS)
    from test_speaker import cos_matrix, offdiag
    assert np.allclose(cos_matrix(z["emb"]), z["cos"], atol=1e-5)
    od = offdiag(z["cos"])
    assert od.max() <= 0.9 and od.max() - od.min() >= 0.1, (od.min(), od.max())   # a model that ignores its input scores 1
    e = np.abs(z["emb_bf16_ref"] - z["emb"]).max() / np.abs(z["emb"]).max()
    assert np.isclose(e, float(z["e_ref"]), rtol=1e-5) and 0 < e < 0.1
    assert os.path.getsize(os.path.join(os.path.dirname(__file__), "golden", "speaker_fbank.npz")) < 64 << 10


def test_fbank_model_has_the_reference_key_set():
    from unispeech_amd.fbank import mel_bank
    from unispeech_amd.speaker import ECAPA_TDNN, ECAPA_TDNN_SMALL
    z = g()
    m = ECAPA_TDNN_SMALL(feat_dim=40, feat_type="fbank")
    assert not hasattr(m, "feature_weight") and m.feat_dim == 40
    sd = m.state_dict()
    assert sorted(sd) == sorted(str(k) for k in z["keys"])
    for k, s in zip(z["keys"], z["key_shapes"]):
        assert tuple(sd[str(k)].shape) == tuple(int(v) for v in s if v >= 0), k
    assert tuple(m.layer1.conv.weight.shape) == (512, 40, 5)
    assert torch.equal(sd["feature_extract.spectrogram.window"], torch.hann_window(400, dtype=torch.float64).float())
    assert np.array_equal(sd["feature_extract.mel_scale.fb"].numpy(), mel_bank(16000, 512, 40).astype(np.float32))
    # the released file's layout loads as verification.py loads it; an unknown key is reported, not fatal
    from test_speaker import fill_state_dict
    filled = fill_state_dict({k: v for k, v in sd.items() if not k.startswith("feature_extract.")}, 5)
    filled["projection.weight"] = torch.zeros(3)
    r = m.load_state_dict(filled, strict=False)
    assert r.unexpected_keys == ["projection.weight"] and sorted(r.missing_keys) == sorted(k for k in sd if k.startswith("feature_extract."))
    assert torch.equal(m.layer1.conv.weight, filled["layer1.conv.weight"])
    assert ECAPA_TDNN(80, feat_type="fbank").layer1.conv.weight.shape == (512, 80, 5)


def test_fbank_model_refusals():
    from unispeech_amd.speaker import ECAPA_TDNN
    with pytest.raises(NotImplementedError, match=r"fbank.*768.*128 mel filters"):
        ECAPA_TDNN(768, feat_type="fbank")
    with pytest.raises(NotImplementedError, match="fbank"):
        ECAPA_TDNN(129, feat_type="fbank")
    with pytest.raises(NotImplementedError, match="mfcc"):
        ECAPA_TDNN(40, feat_type="mfcc")
    with pytest.raises(NotImplementedError, match="16 kHz"):
        ECAPA_TDNN(40, feat_type="fbank", sr=8000)
    with pytest.raises(ValueError, match="num_states"):
        ECAPA_TDNN(40, feat_type="fbank", num_states=13)
    m = ECAPA_TDNN(40, feat_type="fbank").eval()
    with torch.no_grad():
        with pytest.raises(ValueError, match="hidden states"):
            m.hidden_states([torch.zeros(400)])
        with pytest.raises(ValueError, match="hidden states"):
            m.forward_states([torch.zeros(1, 5, 40)])
    with pytest.raises(NotImplementedError, match="training mode"):
        m.train()([torch.zeros(400)])


def test_cli_takes_no_upstream_with_fbank():
    from unispeech_amd import speaker
    a = speaker.parse_args(["verify", "--fbank", "head.pt", "a.wav", "b.wav"])
    assert (a.cmd, a.fbank, a.upstream, a.head, a.wav1, a.wav2, a.emb_dim, a.bf16) == ("verify", True, None, "head.pt", "a.wav",
                                                                                       "b.wav", 256, False)
    a = speaker.parse_args(["embed", "head.pt", "a.wav", "b.wav", "--fbank", "--bf16"])
    assert a.upstream is None and a.head == "head.pt" and a.wavs == ["a.wav", "b.wav"] and a.bf16 and a.fbank
    a = speaker.parse_args(["verify", "up.pt", "head.pt", "a.wav", "b.wav"])
    assert not a.fbank and a.upstream == "up.pt"
    with pytest.raises(SystemExit):
        speaker.parse_args(["verify", "--fbank", "up.pt", "head.pt", "a.wav", "b.wav"])
