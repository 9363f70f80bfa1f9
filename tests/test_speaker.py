"""Speaker head, host side (unispeech_amd/speaker.py): the fixture tests/golden/speaker.npz (tools/gen_speaker_golden.py),
state-dict compatibility with the reference's ECAPA_TDNN, frame-count arithmetic, refusals, the command line and the wav
reader.  No GPU.

This file also holds what the generator and the GPU tests share: `fill_state_dict` (weights are not stored; both sides
refill a state dict from a seed in sorted-key order) and `make_states` (structured hidden states from a seed)."""
import os
import wave

import numpy as np
import pytest
import torch

from conftest import load_golden

RECIPE = dict(gain=1.4)


def fill_state_dict(sd, seed, gain=RECIPE["gain"]):
    """{name: fp32 tensor of sd[name]'s shape}, drawn in sorted-key order from numpy.random.default_rng(seed).  Every entry
    consumes one standard_normal and one random draw of its size, whatever its kind, so the stream depends on the shapes
    only.  Kinds: num_batches_tracked 0; running_var U(0.5, 1.5); running_mean 0.7 + 0.1 N (about the mean of the rectified
    input a BatchNorm of this network sees; with means near 0 a common offset grows through the ReLUs and every pair of
    embeddings scores near 1); feature_weight N (non-uniform
    softmax); weight_g U(0.5, 1.5); 1-D `.weight` (BatchNorm / LayerNorm / GroupNorm) 1 + 0.1 N; other vectors 0.1 N;
    matrices and kernels gain * N / sqrt(fan_in)."""
    rng = np.random.default_rng(seed)
    out = {}
    for k in sorted(sd):
        shape = tuple(sd[k].shape)
        if k.endswith("num_batches_tracked"):
            out[k] = torch.zeros(shape, dtype=torch.long)
            continue
        n = int(np.prod(shape)) if shape else 1
        z, u = rng.standard_normal(n), rng.random(n)
        if k.endswith("running_var") or k.endswith("weight_g"):
            a = 0.5 + u
        elif k.endswith("running_mean"):
            a = 0.7 + 0.1 * z
        elif k.endswith("feature_weight"):
            a = z
        elif len(shape) == 1 and k.endswith(".weight"):
            a = 1.0 + 0.1 * z
        elif len(shape) <= 1:
            a = 0.1 * z
        else:
            a = gain * z / np.sqrt(float(np.prod(shape[1:])))
        out[k] = torch.from_numpy(a.reshape(shape).astype(np.float32))
    return out


def make_states(seed, B, T, n, D, rank=2, noise=0.2):
    """fp32 [n, B, T, D]: utterance b is a rank-2 autoregressive process z_b(t) mixed into the channels by A_b, scaled per
    layer, plus noise and a per-layer offset.  Utterances 2 j and 2 j + 1 share most of A and the process's memory (0.9 for
    even j, 0.2 for odd j): one "speaker".  That makes the reference's cosines spread; i.i.d. noise puts every pair near 1."""
    rng = np.random.default_rng(seed)
    x = np.empty((n, B, T, D), dtype=np.float32)
    A = None
    for b in range(B):
        if b % 2 == 0:
            A = rng.standard_normal((D, rank))
            Ab = A
        else:
            Ab = A + 0.2 * rng.standard_normal((D, rank))
        e = rng.standard_normal((T, rank))
        z = np.empty_like(e)
        z[0] = e[0]
        ar = 0.9 if (b // 2) % 2 == 0 else 0.2
        for t in range(1, T):
            z[t] = ar * z[t - 1] + np.sqrt(1 - ar * ar) * e[t]
        base = z @ Ab.T
        for l in range(n):
            off = 0.2 * rng.standard_normal(D)
            x[l, b] = (0.5 + l / n) * base + noise * rng.standard_normal((T, D)) + off
    return torch.from_numpy(x)


def ramp(T):
    """time weights of the stored checksums (an instance-normed channel sums to zero; its ramp-weighted sum does not)"""
    return np.linspace(0.5, 1.5, T)


def cos_matrix(e):
    e = np.asarray(e, np.float64)
    n = e / np.maximum(np.linalg.norm(e, axis=1, keepdims=True), 1e-8)
    return n @ n.T


def offdiag(c):
    c = np.asarray(c)
    return c[~np.eye(len(c), dtype=bool)]


def z():
    return load_golden("speaker.npz")


def head(feat_dim, num_states, **kw):
    from unispeech_amd.speaker import ECAPA_TDNN_SMALL
    return ECAPA_TDNN_SMALL(feat_dim, num_states=num_states, **kw)


# ------------------------------------------------------------------------------------------------------------- fixture
def test_fixture_integrity():
    g = z()
    keys, shapes = [str(k) for k in g["keys"]], g["key_shapes"]
    assert len(keys) == len(shapes) and "feature_weight" in keys and "layer3.Res2Conv1dReluBn.convs.4.weight" in keys
    assert not any(k.startswith("feature_extract.") for k in keys)
    for name, B, T, n, D in (("head768", 4, 149, 13, 768), ("head1024", 2, 99, 25, 1024)):
        assert [int(v) for v in g[name + "/shape"]] == [B, T, n, D]
        assert g[name + "/emb"].shape == (B, 256) and g[name + "/cos"].shape == (B, B)
        assert g[name + "/normed_chk"].shape == (B, D) and g[name + "/pooled"].shape == (B, 3072)
        assert g[name + "/out2_mean"].shape == (B, 512) and g[name + "/out4_mean"].shape == (B, 512)
        assert np.allclose(cos_matrix(g[name + "/emb"]), g[name + "/cos"], atol=1e-5)
    od = offdiag(g["head768/cos"])
    assert od.max() - od.min() >= 0.3, (od.min(), od.max())   # a head that ignores its input cannot pass the score test
    assert g["head768/emb_bf16_ref"].shape == (4, 256)
    e = np.abs(g["head768/emb_bf16_ref"] - g["head768/emb"]).max() / np.abs(g["head768/emb"]).max()
    assert np.isclose(e, float(g["head768/e_ref"]), rtol=1e-5) and 0 < e < 0.1
    assert g["lengths/emb"].shape == (3, 256) and [int(v) for v in g["lengths/frames"]] == [149, 100, 61]
    for name in ("e2e_tiny", "e2e_tiny_preln"):
        assert g[name + "/wav_i16"].dtype == np.int16 and g[name + "/wav_i16"].shape == (4, 32000)
        assert g[name + "/hs_chk"].shape == (3, 4, 64) and g[name + "/emb"].shape == (4, 256)
    assert os.path.getsize(os.path.join(os.path.dirname(__file__), "golden", "speaker.npz")) < 1 << 20


# ---------------------------------------------------------------------------------------------------------- state dict
def test_state_dict_names_and_shapes_equal_the_reference():
    g = z()
    sd = head(768, 13).state_dict()
    assert sorted(sd) == sorted(str(k) for k in g["keys"])
    for k, s in zip(g["keys"], g["key_shapes"]):
        assert tuple(sd[str(k)].shape) == tuple(int(v) for v in s if v >= 0), k


def test_strict_load_of_the_head_and_combined_dict():
    from unispeech_amd.speaker import ECAPA_TDNN_SMALL
    from unispeech_amd.wavlm import WavLM, WavLMConfig
    from conftest import TINY
    m = head(768, 13)
    filled = fill_state_dict(m.state_dict(), 5)
    m.load_state_dict(filled, strict=True)
    assert torch.equal(m.layer2.Res2Conv1dReluBn.convs[4].weight, filled["layer2.Res2Conv1dReluBn.convs.4.weight"])
    with pytest.raises(RuntimeError):
        m.load_state_dict({k: v for k, v in filled.items() if k != "bn.running_mean"}, strict=True)
    # the released layout: head keys + the upstream under feature_extract.model.* + keys this model does not have
    up = WavLM(WavLMConfig(dict(TINY)))
    full = ECAPA_TDNN_SMALL(64, upstream=up)
    assert full.feat_num == 3 and all(not p.requires_grad for p in full.feature_extract.parameters())
    names = set(full.state_dict())
    assert {"feature_extract.model." + k for k in up.state_dict()} <= names
    comb = fill_state_dict(full.state_dict(), 6)
    comb["feature_extract.model.final_proj.weight"] = torch.zeros(3, 3)
    comb.pop("linear.bias")
    r = full.load_state_dict(comb, strict=False)
    assert r.missing_keys == ["linear.bias"] and r.unexpected_keys == ["feature_extract.model.final_proj.weight"]
    assert torch.equal(full.feature_extract.model.encoder.layers[1].fc1.weight,
                       comb["feature_extract.model.encoder.layers.1.fc1.weight"])


# ------------------------------------------------------------------------------------------------------ frame arithmetic
def test_frame_counts_and_length_groups():
    from unispeech_amd.speaker import frame_count, group_by_length
    assert frame_count(16000) == 49 and frame_count(32000) == 99 and frame_count(240000) == 749
    assert frame_count(400) == 1 and frame_count(32000, "[(32,10,5)] + [(32,3,2)] * 4 + [(32,2,2)] * 2") == 99
    # against a direct count of the windows of each layer
    for n in (4000, 16001, 19999, 47870):
        m = n
        for k, s in [(10, 5)] + [(3, 2)] * 4 + [(2, 2)] * 2:
            m = len(range(0, m - k + 1, s))
        assert frame_count(n) == m
    assert group_by_length([5, 7, 5, 9, 7]) == {5: [0, 2], 7: [1, 4], 9: [3]}


# -------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_name_the_option():
    from unispeech_amd.speaker import ECAPA_TDNN
    for kw, word in ((dict(global_context_att=True), "global_context_att"), (dict(feat_type="fbank"), "fbank"),
                     (dict(feat_type="mfcc"), "mfcc"), (dict(update_extract=True), "update_extract"),
                     (dict(sr=8000), "16 kHz"), (dict(channels=1024), "channels")):
        with pytest.raises(NotImplementedError, match=word):
            ECAPA_TDNN(768, num_states=13, **kw)
    m = head(64, 3)
    st = [torch.zeros(1, 5, 64)] * 3
    with pytest.raises(NotImplementedError, match="training mode"):
        m.train().forward_states(st)
    with pytest.raises(NotImplementedError, match="gradients"):
        m.eval().forward_states(st)
    with torch.no_grad():
        with pytest.raises(NotImplementedError, match="mono"):
            m.eval()._wav_list([torch.zeros(2, 100)])
        with pytest.raises(ValueError, match="upstream"):
            m.hidden_states([torch.zeros(400)])


# ---------------------------------------------------------------------------------------------------- CLI and wav reader
def write_wav(path, samples_i16, sr=16000, channels=1):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(channels)
        w.setsampwidth(2)
        w.setframerate(sr)
        w.writeframes(np.asarray(samples_i16, dtype="<i2").tobytes())


def test_cli_arguments_and_wav_reader(tmp_path):
    from unispeech_amd import speaker
    a = speaker.parse_args(["verify", "up.pt", "head.pt", "a.wav", "b.wav"])
    assert (a.cmd, a.upstream, a.head, a.wav1, a.wav2, a.emb_dim, a.bf16) == ("verify", "up.pt", "head.pt", "a.wav", "b.wav",
                                                                             256, False)
    a = speaker.parse_args(["embed", "up.pt", "head.pt", "a.wav", "b.wav", "c.wav", "--bf16", "--emb_dim", "192"])
    assert a.wavs == ["a.wav", "b.wav", "c.wav"] and a.bf16 and a.emb_dim == 192
    with pytest.raises(SystemExit):
        speaker.parse_args(["verify", "up.pt", "head.pt", "a.wav"])
    s = (np.arange(-400, 400) * 40).astype(np.int16)
    write_wav(tmp_path / "a.wav", s)
    w = speaker.read_wav_16k(str(tmp_path / "a.wav"))
    assert w.dtype == torch.float32 and torch.equal(w, torch.from_numpy(s.astype(np.float32) / 32768.0))
    write_wav(tmp_path / "b.wav", s, sr=8000)
    with pytest.raises(NotImplementedError, match="16 kHz"):
        speaker.read_wav_16k(str(tmp_path / "b.wav"))
