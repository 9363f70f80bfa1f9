"""csrc/mfcc.hip on the device against mfcc_reference (tests/mfcc_cases.py holds the inputs and both oracles).

Tolerance: measured on the reference side, never on the device's.  For a case -- one sample rate and the rows the call is
given -- E32[j] is the largest |mfcc_reference(float32) - mfcc_reference(float64)| of output column j over the frames of the
case's rows: what the reference's own precision (fp32 tables, fp32 pocketfft, fp32 sums) costs on that input.  The device must
lie within 4 x E32[j] of the float64 value in every column; the factor covers a butterfly order and table rounding that differ
from pocketfft's while both carry fp32 error growing with log P.  A case pools its rows (lengths of one frame, one sample short
of two, two, just short of six, and two workgroup tiles + 17 frames): the one- and two-frame rows alone would make E32[j] a
maximum over one or two numbers, which says nothing about a precision.  The worst ratio per case is printed (-s)."""
import os
import wave

import numpy as np
import pytest
import torch

import mfcc_cases as MC

pytestmark = pytest.mark.gpu


def _dev(pcm, dtype):
    t = torch.from_numpy(np.array(pcm))
    return (t if dtype == torch.int16 else t.to(torch.float32) / 32768.0).cuda()


def _ratio(got, rows, sr, E):
    """worst |device - float64 oracle| / E32[j] over the rows; got: list of [frames, 39] arrays"""
    worst = 0.0
    for g, pcm in zip(got, rows):
        r64 = MC.refs(pcm, sr)[0]
        assert g.shape == r64.shape
        if not len(r64):
            continue
        err = np.abs(g.astype(np.float64) - r64).max(0)
        assert np.all(err[E == 0] == 0)
        worst = max(worst, float((err[E > 0] / E[E > 0]).max()))
    return worst


@pytest.mark.parametrize("dtype", [torch.float32, torch.int16], ids=["fp32", "int16"])
@pytest.mark.parametrize("sr", [16000, 8000])
def test_parity(sr, dtype):
    from unispeech_amd.mfcc import mfcc, num_frames
    rows = MC.parity_rows(sr)
    E = MC.e32(rows, sr)
    feats, frames = mfcc([_dev(p, dtype) for p in rows], sr)
    assert frames == [num_frames(len(p), sr) for p in rows] == [1, 1, 2, 5, 2 * MC.TILE + 17]
    assert feats.shape == (len(rows), max(frames), 39) and feats.dtype == torch.float32
    f = feats.cpu().numpy()
    for r, n in enumerate(frames):
        assert np.all(f[r, n:] == 0)                                  # padded rows are written, as zero
    worst = _ratio([f[r, :n] for r, n in enumerate(frames)], rows, sr, E)
    print("mfcc parity sr=%d %s: worst |dev - f64| / E32 = %.3f (max E32 %.3e)" % (sr, dtype, worst, E.max()))
    assert worst <= 4.0
    # each length alone: the same bits as inside the batch, and the one-frame row has zero deltas
    for r, p in enumerate(rows):
        alone, n1 = mfcc(_dev(p, dtype), sr)
        assert n1 == [frames[r]] and torch.equal(alone, feats[r, :frames[r]])
    assert np.all(f[0, 0, 13:] == 0)


@pytest.mark.parametrize("sr", [16000, 8000])
def test_batch_of_unequal_rows(sr):
    """B = 3 as one [B, L] tensor with lengths: a multi-tile row with an exact-zero stretch, a row shorter than the window,
    a short row; what lies beyond a row's length is garbage the kernel must not read into the features"""
    from unispeech_amd.mfcc import EPS32, geometry, mfcc, num_frames, tables
    W, S, _ = geometry(sr)
    rows, z = MC.batch_rows(sr)
    lens = [len(p) for p in rows]
    E = MC.e32(rows, sr)
    pcm = np.full((3, max(lens)), 12345, np.int16)
    for r, p in enumerate(rows):
        pcm[r, :lens[r]] = p
    x16 = torch.from_numpy(pcm).cuda()
    x32 = x16.to(torch.float32) / 32768.0
    feats, frames = mfcc(x32, sr, lengths=lens)
    want = [num_frames(n, sr) for n in lens]
    assert frames == want and want[1] == 0 and want[0] > MC.TILE
    assert feats.shape == (3, num_frames(max(lens), sr), 39)
    f = feats.cpu().numpy()
    for r, n in enumerate(frames):
        assert np.all(f[r, n:] == 0)
    worst = _ratio([f[r, :n] for r, n in enumerate(frames)], rows, sr, E)
    print("mfcc batch sr=%d: worst |dev - f64| / E32 = %.3f (max E32 %.3e)" % (sr, worst, E.max()))
    assert worst <= 4.0
    # frames wholly inside the zero stretch sit on the floor exactly: the bits of digital silence, c0 = sqrt(23) ln(eps32)
    inside = [i for i in range(frames[0]) if i * S >= z[0] and i * S + W <= z[1]]
    assert len(inside) == 14
    silence = mfcc(torch.zeros(W + 8 * S, device="cuda"), sr)[0]
    assert torch.equal(silence[:, 13:], torch.zeros_like(silence[:, 13:]))
    for i in inside:
        assert torch.equal(feats[0, i, :13], silence[0, :13])
    assert torch.equal(feats[0, inside[4]:inside[-4], 13:], torch.zeros_like(feats[0, inside[4]:inside[-4], 13:]))
    dct = tables(sr)["dct"]
    c0 = np.sqrt(23.0) * np.log(EPS32)
    bound = 24 * 2.0 ** -24 * np.abs(dct).sum(1).max() * abs(np.log(EPS32))      # 23 fmaf's + the rounding of the log
    s = silence[0].cpu().numpy().astype(np.float64)
    assert abs(s[0] - c0) <= bound and np.abs(s[1:13]).max() <= bound
    # bit-identity: a row alone, int16 against fp32 of pcm / 32768, deltas=False against the first 13 columns
    for r, p in enumerate(rows):
        alone, n1 = mfcc(_dev(p, torch.float32), sr)
        assert n1 == [frames[r]] and torch.equal(alone, feats[r, :frames[r]])
    f16, fr16 = mfcc(x16, sr, lengths=torch.tensor(lens))
    assert fr16 == frames and torch.equal(f16, feats)
    c13, fr13 = mfcc(x32, sr, lengths=lens, deltas=False)
    assert fr13 == frames and c13.shape == feats.shape[:2] + (13,) and torch.equal(c13, feats[..., :13])
    # a strided view of a wider buffer reads the same
    wide = torch.zeros(3, max(lens) + 7, device="cuda")
    wide[:, :max(lens)] = x32
    assert torch.equal(mfcc(wide[:, :max(lens)], sr, lengths=lens)[0], feats)


def test_labels():
    """label_audio(features="mfcc") against the float64 oracle's argmin on every frame that is not a near tie (the share of
    near ties is capped at 2 % by tests/test_mfcc.py from the oracle alone)"""
    from unispeech_amd.kmeans import label_audio
    pcm, centres, want, tie, _ = MC.label_case()
    assert tie.mean() <= 0.02
    x = pcm.astype(np.float32) / 32768.0
    got = label_audio(None, x, None, centres, features="mfcc")
    assert got.dtype == torch.int32 and got.is_cuda
    got = got.cpu().numpy()
    assert got.shape == want.shape
    bad = (got != want) & ~tie
    print("mfcc labels: %d frames, %d near ties, %d differ on a near tie" % (len(want), tie.sum(), ((got != want) & tie).sum()))
    assert not bad.any(), np.nonzero(bad)[0]
    assert torch.equal(label_audio(None, torch.from_numpy(pcm.copy()), None, centres, features="mfcc").cpu(),
                       torch.from_numpy(got))                          # int16 PCM in gives the same labels


def _write_wav(path, pcm, sr):
    with wave.open(path, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(sr)
        w.writeframes(pcm.astype("<i2").tobytes())


@pytest.mark.parametrize("sr", [16000, 8000])
def test_shard_round_trip(tmp_path, sr):
    from unispeech_amd import kmeans
    from unispeech_amd.mfcc import MfccFeatureReader, mfcc, num_frames
    root = tmp_path / "audio"
    root.mkdir()
    pcms = [MC.signal(sr // 2 + 123, sr, 21), MC.signal(sr // 4 + 7, sr, 22)]
    lines = [str(root)]
    for i, p in enumerate(pcms):
        _write_wav(str(root / ("u%d.wav" % i)), p, sr)
        lines.append("u%d.wav\t%d" % (i, len(p)))
    (tmp_path / "train.tsv").write_text("\n".join(lines) + "\n")
    feats = [mfcc(_dev(p, torch.float32), sr)[0] for p in pcms]
    centres = torch.cat(feats)[::3][:20].cpu().numpy()
    lab = kmeans.dump_labels(str(tmp_path), "train", None, None, centres, 1, 0, str(tmp_path / "lab"), features="mfcc",
                             sample_rate=sr)
    got = [list(map(int, ln.split())) for ln in open(lab).read().splitlines()]
    want = [kmeans.label_audio(None, kmeans.read_wav(str(root / ("u%d.wav" % i)))[0], None, centres, features="mfcc",
                               sample_rate=sr).cpu().tolist() for i in range(2)]
    assert got == want and [len(g) for g in got] == [num_frames(len(p), sr) for p in pcms]
    # one utterance per launch writes the same lines
    lab1 = kmeans.dump_labels(str(tmp_path), "train", None, None, centres, 1, 0, str(tmp_path / "lab1"), features="mfcc",
                              sample_rate=sr, max_batch_samples=1)
    assert open(lab1).read() == open(lab).read()
    npy, ln = kmeans.dump_mfcc_features(str(tmp_path), "train", sr, 1, 0, str(tmp_path / "feat"))
    assert os.path.basename(npy) == "train_0_1.npy"
    assert [int(v) for v in open(ln).read().split()] == [num_frames(len(p), sr) for p in pcms]
    arr = np.load(npy)
    assert arr.dtype == np.float32 and np.array_equal(arr, torch.cat(feats).cpu().numpy())
    reader = MfccFeatureReader(sr)
    assert torch.equal(reader.get_feats(str(root / "u1.wav")), feats[1])
    assert torch.equal(reader.get_feats(pcms[1].copy()), feats[1])
