"""The sinc resampler without a GPU: the filter table against the figures of torchaudio's published formula, the float64
restatement that is the GPU tests' oracle, the compact table the kernel reads, the refusals, and the 8 kHz chunking of
diarization.predict(input_rate=...)."""
import math
import os
import re
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# orig, new -> (o, n, width, taps of the dense filter)
RATIOS = {(8000, 16000): (1, 2, 7, 15), (44100, 16000): (441, 160, 17, 475), (48000, 16000): (3, 1, 19, 41),
          (11025, 16000): (441, 640, 7, 455), (22050, 16000): (441, 320, 9, 459)}


@pytest.mark.parametrize("rates", sorted(RATIOS))
def test_sinc_table_geometry_phase_sums_and_compact_form(rates):
    from unispeech_amd.resample import compact_table, sinc_table
    o, n, width, taps = RATIOS[rates]
    table, w, o_, n_ = sinc_table(*rates)
    assert (o_, n_, w) == (o, n, width) and table.shape == (n, taps) and table.dtype == np.float64
    sums = table.sum(1)
    print(rates, "phase sums", sums.min(), sums.max(), "max abs sum", np.abs(table).sum(1).max())
    assert sums.min() >= 1.00003 and sums.max() <= 1.0009
    assert np.abs(table).sum(1).max() <= 1.87
    ctab, first, w2, o2, n2 = compact_table(*rates)
    tc = 2 * width + 1
    assert (w2, o2, n2) == (width, o, n) and ctab.shape == (n, tc) and first.shape == (n,) and first.dtype == np.int32
    assert first.min() >= 0 and first.max() + tc <= taps
    # every tap of the dense table is either in its phase's compact row, bit for bit, or below 1e-30
    kept = np.zeros_like(table, dtype=bool)
    for i in range(n):
        row = table[i, first[i]:first[i] + tc]
        nz = ctab[i] != 0
        assert np.array_equal(ctab[i][nz], row[nz])
        kept[i, first[i]:first[i] + tc] = nz
    assert np.abs(table[~kept]).max(initial=0.0) < 1e-30
    assert (kept.sum(1) <= tc).all()


def test_16k_to_8k_table():
    from unispeech_amd.resample import sinc_table
    table, width, o, n = sinc_table(16000, 8000)
    assert (o, n, width, table.shape) == (2, 1, 13, (1, 28))
    assert abs(table.sum() - 1.0) < 1e-3


@pytest.mark.parametrize("L", [1, 5, 999, 1000])
def test_reference_output_length(L):
    from unispeech_amd.resample import resample_reference
    x = torch.linspace(-1, 1, 2 * L).view(2, L)
    for (orig, new), (o, n, _, _) in RATIOS.items():
        y = resample_reference(x, orig, new)
        assert y.dtype == torch.float64 and y.shape == (2, math.ceil(n * L / o)), (orig, new, y.shape)
    assert resample_reference(x, 16000, 8000).shape == (2, math.ceil(L / 2))
    assert resample_reference(x[0], 8000, 16000).shape == (2 * L,)


def test_one_khz_sine_keeps_its_shape_from_8k_to_16k():
    """a property of the filter, not of a copy of it: 1.7e-4 on these 4000 samples, bound 1e-3 (up to 2.7e-4 was seen on other
    lengths when the formula was written down: a margin of about four)"""
    from unispeech_amd.resample import resample_reference
    t8 = torch.arange(4000, dtype=torch.float64) / 8000
    y = resample_reference(torch.sin(2 * math.pi * 1000 * t8), 8000, 16000)
    want = torch.sin(2 * math.pi * 1000 * torch.arange(8000, dtype=torch.float64) / 16000)
    err = (y - want).abs()[50:-50].max().item()
    print("1 kHz sine 8k -> 16k: max error away from the edges", err)
    assert y.shape == (8000,) and err < 1e-3


def test_reference_is_the_plain_double_sum():
    """the conv1d form against the formula written as loops (44.1 k -> 16 k, a short signal)"""
    from unispeech_amd.resample import resample_reference, sinc_table
    table, width, o, n = sinc_table(44100, 16000)
    g = torch.Generator().manual_seed(3)
    x = torch.rand(1500, generator=g, dtype=torch.float64) * 2 - 1
    y = resample_reference(x, 44100, 16000).numpy()
    xp = np.concatenate([np.zeros(width), x.numpy(), np.zeros(width + o)])
    for m in (0, 1, 159, 160, 161, 300, len(y) - 1):
        f, i = divmod(m, n)
        assert abs(y[m] - float(table[i] @ xp[f * o:f * o + table.shape[1]])) < 1e-13


def test_equal_rates_return_the_input():
    from unispeech_amd.resample import Resample, resample, resample_reference
    x = torch.randn(2, 100)
    assert resample(x, 16000, 16000) is x                       # no device needed: nothing runs
    assert Resample(8000, 8000)(x) is x
    assert torch.equal(resample_reference(x, 441, 441), x.double())


def test_refusals():
    from unispeech_amd import _lib
    from unispeech_amd.resample import Resample, resample
    with pytest.raises(NotImplementedError, match="kaiser_window"):
        Resample(8000, 16000, resampling_method="kaiser_window")
    with pytest.raises(NotImplementedError, match="44100 Hz -> 48001 Hz"):
        resample(torch.zeros(1, 10), 44100, 48001)              # 48001 phases: refused before any table is built
    with pytest.raises(NotImplementedError, match="16000 Hz -> 1 Hz"):
        resample(torch.zeros(1, 10), 16000, 1)                  # one phase of about 194 thousand taps
    with pytest.raises(_lib.WavlmHipError, match="no CPU fallback"):
        resample(torch.zeros(1, 10), 8000, 16000)
    L = _lib.lib()
    for o, n, w in ((1, 2, 7), (441, 160, 17), (3, 1, 19), (441, 640, 7), (441, 320, 9), (2, 1, 13)):
        assert L.wavlm_resample_supported(o, n, w) == 1
    assert L.wavlm_resample_supported(441, 1280, 7) == 0 and L.wavlm_resample_supported(0, 1, 7) == 0


def test_predict_at_the_config_rate_chunks_at_8_khz_and_resamples_one_batch(monkeypatch):
    from unispeech_amd import diarization
    from unispeech_amd import resample as rs
    from unispeech_amd.diarization import diarize, predict
    calls, seen = [], []

    def fake_resample(wave, orig, new):
        calls.append((tuple(wave.shape), orig, new))
        return rs.resample_reference(wave, orig, new).float()

    def batch_estimate(chunks):
        seen.append(chunks)
        B, T = len(chunks), 750
        acts = torch.arange(B * T * 3, dtype=torch.float32).view(B, T, 3)
        return acts, torch.ones(B, 3, 4) * torch.arange(B).view(B, 1, 1)

    monkeypatch.setattr(rs, "resample", fake_resample)
    assert diarization._resample is rs
    stub = types.SimpleNamespace(sr=8000, frame_shift=320, subsampling=1, batch_estimate=batch_estimate, n_speakers=3)
    n8 = 2 * 240000 + 50000                                     # two whole 30 s chunks and 6.25 s, counted at 8 kHz
    wav8 = torch.sin(torch.arange(n8, dtype=torch.float32) * 0.05)
    acti_list, svec, lens = predict(stub, wav8, 750, input_rate=8000)
    assert calls == [((3, 240000), 8000, 16000)] and lens == [750, 750, 156]
    assert len(seen) == 1 and tuple(seen[0].shape) == (3, 480000)
    # the third chunk is the LAST 240000 samples (it starts inside the second), resampled on its own
    want = rs.resample_reference(wav8[n8 - 240000:], 8000, 16000).float()
    assert torch.equal(seen[0][2], want)
    assert torch.equal(seen[0][1], rs.resample_reference(wav8[240000:480000], 8000, 16000).float())
    assert [a.shape for a in acti_list] == [(750, 3), (750, 3), (156, 3)] and svec.shape == (9, 4)
    assert acti_list[2][0, 0] == (2 * 750 + 750 - 156) * 3      # the new frames are the chunk's last ones
    # 16 kHz input is untouched by all this
    calls.clear(), seen.clear()
    predict(stub, torch.zeros(2 * n8), 750)
    assert calls == [] and [len(c) for c in seen[0]] == [480000] * 3
    for rate in (11025, 44100):
        with pytest.raises(NotImplementedError, match="input_rate=%d" % rate):
            predict(stub, wav8, 750, input_rate=rate)
        with pytest.raises(NotImplementedError, match="input_rate=%d" % rate):
            diarize(stub, wav8, 750, input_rate=rate)


def test_readers_report_the_rate(tmp_path):
    from test_speaker import write_wav
    from unispeech_amd import diarization, speaker
    s = (np.arange(-400, 400) * 40).astype(np.int16)
    write_wav(tmp_path / "a.wav", s, sr=8000)
    w, sr = speaker.read_wav(str(tmp_path / "a.wav"))
    assert sr == 8000 and w.dtype == torch.float32 and torch.equal(w, torch.from_numpy(s.astype(np.float32) / 32768.0))
    w2, sr2 = diarization.read_recording(str(tmp_path / "a.wav"), 8000)
    assert sr2 == 8000 and torch.equal(w, w2)
    write_wav(tmp_path / "b.wav", s, sr=44100)
    assert speaker.read_wav(str(tmp_path / "b.wav"))[1] == 44100
    with pytest.raises(NotImplementedError, match="44100"):
        diarization.read_recording(str(tmp_path / "b.wav"), 8000)
    write_wav(tmp_path / "c.wav", s)
    assert diarization.read_recording(str(tmp_path / "c.wav"), 8000)[1] == 16000


def test_entry_points_declared_and_bound():
    from unispeech_amd import _lib, build
    src = open(os.path.join(ROOT, "include", "wavlm_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert int(re.search(r"#define WAVLM_HIP_ABI_VERSION (\d+)", src).group(1)) >= 27 and _lib.ABI_VERSION >= 27
    for name in ("wavlm_resample_supported", "wavlm_resample_rows"):
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["wavlm_resample_rows"][1]) == code[code.index("wavlm_resample_rows"):].split(")")[0].count(",") + 1
    assert "resample.hip" in build.SOURCES
