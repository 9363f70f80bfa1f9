"""k-means labels, host side (unispeech_amd/kmeans.py): manifest sharding, the wav reader, the .km / .len / .npy /
dict.km.txt formats, option refusal, and the fp64 restatement of the mini-batch centre update.  Where the reference tree
is present its own readers / writers (src/examples/hubert/simple_kmeans/) are run on our files; where sklearn is
importable the restatement is checked against sklearn's _minibatch_update_dense."""
import importlib
import os
import sys
import types
import wave

import numpy as np
import pytest

from oracle import ref_shim

KM_DIR = os.path.join(ref_shim.REF_ROOT, "src", "examples", "hubert", "simple_kmeans")
needs_ref = pytest.mark.skipif(not os.path.isdir(KM_DIR), reason="reference tree not present")


def _write_wav(path, samples, sr=16000, width=2, channels=1):
    with wave.open(path, "wb") as w:
        w.setnchannels(channels)
        w.setsampwidth(width)
        w.setframerate(sr)
        w.writeframes(np.ascontiguousarray(samples).tobytes())


def _manifest(tmp_path, n):
    rng = np.random.default_rng(0)
    root = tmp_path / "audio"
    root.mkdir()
    lines = [str(root)]
    for i in range(n):
        s = rng.integers(-32768, 32767, 1600 + 160 * i).astype("<i2")
        _write_wav(str(root / ("u%d.wav" % i)), s)
        lines.append("u%d.wav\t%d" % (i, len(s)))
    tsv = tmp_path / "train.tsv"
    tsv.write_text("\n".join(lines) + "\n")
    return str(tsv)


def mb_update_fp64(c, w, x, labels):
    """sklearn _minibatch_update_dense restated in fp64: clusters that received rows move to
    (c w + sum x) / (w + n) and w += n; the others stay"""
    c = c.astype(np.float64).copy()
    w = w.astype(np.float64).copy()
    for j in range(c.shape[0]):
        m = labels == j
        n = int(m.sum())
        if n:
            c[j] = (c[j] * w[j] + x[m].astype(np.float64).sum(0)) / (w[j] + n)
            w[j] += n
    return c, w


def lloyd_update_fp64(c, x, labels):
    c = c.astype(np.float64).copy()
    for j in range(c.shape[0]):
        m = labels == j
        if m.any():
            c[j] = x[m].astype(np.float64).mean(0)
    return c


def test_sharding_matches_the_reference_rule(tmp_path):
    from unispeech_amd.kmeans import get_path_iterator
    tsv = _manifest(tmp_path, 7)
    seen = []
    for rank in range(3):
        it, n = get_path_iterator(tsv, 3, rank)
        items = list(it())
        assert len(items) == n
        seen += items
    # ceil(7 / 3) = 3: shards of 3, 3, 1, in manifest order, every utterance once
    assert [os.path.basename(p) for p, _ in seen] == ["u%d.wav" % i for i in range(7)]
    assert [n for _, n in seen] == [1600 + 160 * i for i in range(7)]


def test_wav_reader_values_and_refusals(tmp_path):
    from unispeech_amd.kmeans import read_wav
    s = np.array([-32768, -1, 0, 1, 16384, 32767], dtype="<i2")
    p = str(tmp_path / "a.wav")
    _write_wav(p, s)
    wav, sr = read_wav(p)
    assert sr == 16000 and wav.dtype == np.float64
    assert np.array_equal(wav, s.astype(np.float64) / 32768.0)  # soundfile.read's float64 values for 16-bit PCM
    st = np.stack([s, s[::-1]], 1).astype("<i2")
    p2 = str(tmp_path / "st.wav")
    _write_wav(p2, st, channels=2)
    assert np.array_equal(read_wav(p2)[0], (st.astype(np.float64) / 32768.0).mean(-1))
    p3 = str(tmp_path / "u8.wav")
    _write_wav(p3, np.arange(10, dtype=np.uint8), width=1)
    with pytest.raises(NotImplementedError, match="16-bit PCM"):
        read_wav(p3)
    p4 = str(tmp_path / "x.wav")
    open(p4, "wb").write(b"not a wav file at all")
    with pytest.raises(NotImplementedError, match="16-bit PCM"):
        read_wav(p4)


def test_option_refusal_by_name():
    from unispeech_amd.kmeans import MiniBatchKMeans
    with pytest.raises(NotImplementedError, match="reassignment_ratio"):
        MiniBatchKMeans(n_clusters=4, reassignment_ratio=0.01)
    with pytest.raises(NotImplementedError, match="random"):
        MiniBatchKMeans(n_clusters=4, init="random")
    with pytest.raises(NotImplementedError, match="elkan"):
        MiniBatchKMeans(n_clusters=4, algorithm="elkan")
    MiniBatchKMeans(n_clusters=4, init=np.zeros((4, 3), np.float32))  # an explicit array is accepted


def test_cli_arguments_parse():
    from unispeech_amd import kmeans
    with pytest.raises(SystemExit):
        kmeans.main(["learn", "feat", "train"])  # missing positionals: argparse refuses, as the reference scripts do


def _fake_feature_dump(tmp_path, lens, D=5):
    """our .npy / .len writer driven with synthetic features (no model): dump_features with a stub feature source"""
    from unispeech_amd import kmeans
    feats = [np.random.default_rng(i).standard_normal((n, D)).astype(np.float32) for i, n in enumerate(lens)]
    tsv_dir = tmp_path / "tsv"
    tsv_dir.mkdir()
    root = tmp_path / "audio"
    root.mkdir()
    lines = [str(root)]
    for i, n in enumerate(lens):
        _write_wav(str(root / ("u%d.wav" % i)), np.zeros(16 * n, "<i2"))
        lines.append("u%d.wav\t%d" % (i, 16 * n))
    (tsv_dir / "train.tsv").write_text("\n".join(lines) + "\n")
    it = iter(feats)

    class _T:
        def __init__(self, a):
            self.a = a

        def float(self):
            return self

        def cpu(self):
            return self

        def numpy(self):
            return self.a

    orig = kmeans._get_feats
    kmeans._get_feats = lambda *a, **k: _T(next(it))
    try:
        npy, ln = kmeans.dump_features(str(tsv_dir), "train", object(), 3, 1, 0, str(tmp_path / "feat"), normalize=False)
    finally:
        kmeans._get_feats = orig
    return feats, npy, ln


def test_feature_dump_format(tmp_path):
    from unispeech_amd.kmeans import get_feat_iterator
    feats, npy, ln = _fake_feature_dump(tmp_path, [3, 1, 4])
    assert os.path.basename(npy) == "train_0_1.npy" and os.path.basename(ln) == "train_0_1.len"
    assert open(ln).read() == "3\n1\n4\n"
    a = np.load(npy)
    assert a.dtype == np.float32 and a.shape == (8, 5)
    assert np.array_equal(a, np.concatenate(feats))
    it, n = get_feat_iterator(str(tmp_path / "feat"), "train", 1, 0)
    assert n == 3 and all(np.array_equal(u, f) for u, f in zip(it(), feats))


def _ref_module(name, stubs=()):
    """import a reference simple_kmeans script with inert stand-ins for the modules it imports but this check never uses"""
    saved = {m: sys.modules.get(m) for m in stubs}
    for m in stubs:
        mod = types.ModuleType(m)
        if m == "fairseq.data.audio.audio_utils":
            mod.parse_path = lambda p: (p, [])
            mod.read_from_stored_zip = mod.is_sf_audio_data = None
        if m == "npy_append_array":
            mod.NpyAppendArray = None
        sys.modules[m] = mod
    sys.path.insert(0, KM_DIR)
    try:
        return importlib.import_module(name)
    finally:
        sys.path.remove(KM_DIR)
        for m, v in saved.items():
            if v is None:
                sys.modules.pop(m, None)
            else:
                sys.modules[m] = v


@needs_ref
def test_reference_readers_accept_our_files(tmp_path):
    feats, _, _ = _fake_feature_dump(tmp_path, [2, 5, 3])
    ref = _ref_module("dump_km_label")
    it, n = ref.get_feat_iterator(str(tmp_path / "feat"), "train", 1, 0)
    assert n == 3 and all(np.array_equal(u, f) for u, f in zip(it(), feats))
    hub = _ref_module("dump_hubert_feature", stubs=("fairseq", "fairseq.data", "fairseq.data.audio",
                                                    "fairseq.data.audio.audio_utils", "soundfile", "npy_append_array"))
    from unispeech_amd.kmeans import get_path_iterator
    (tmp_path / "m").mkdir()
    tsv = _manifest(tmp_path / "m", 5)
    for rank in range(2):
        a, na = hub.get_path_iterator(tsv, 2, rank)
        b, nb = get_path_iterator(tsv, 2, rank)
        assert na == nb and list(a()) == list(b())


@needs_ref
def test_label_lines_match_the_reference_writer(tmp_path):
    """dump_km_label.dump_label on a feature dump and our CLI `dump_label` path write byte-identical .km files; the
    label arithmetic is the reference's own numpy ApplyKmeans on both sides here (ours runs on the GPU: tests/
    test_kmeans_gpu.py), so this pins the line format and the sharding of the label file"""
    joblib = pytest.importorskip("joblib")
    sk = pytest.importorskip("sklearn.cluster")
    feats, _, _ = _fake_feature_dump(tmp_path, [4, 1, 6])
    km = sk.MiniBatchKMeans(n_clusters=3)
    km.cluster_centers_ = np.random.default_rng(1).standard_normal((3, 5)).astype(np.float32)
    kp = str(tmp_path / "km.bin")
    joblib.dump(km, kp)
    ref = _ref_module("dump_km_label")
    ref.dump_label(str(tmp_path / "feat"), "train", kp, 1, 0, str(tmp_path / "lab_ref"))
    app = ref.ApplyKmeans(kp)
    ours = "".join(" ".join(map(str, app(f).tolist())) + "\n" for f in feats)
    assert open(tmp_path / "lab_ref" / "train_0_1.km").read() == ours


def test_minibatch_restatement_against_sklearn():
    pytest.importorskip("sklearn")
    from sklearn.cluster._k_means_minibatch import _minibatch_update_dense
    rng = np.random.default_rng(3)
    K, D, n = 6, 9, 50
    x = rng.standard_normal((n, D)).astype(np.float64)
    c = rng.standard_normal((K, D)).astype(np.float64)
    w = rng.integers(0, 20, K).astype(np.float64)
    labels = rng.integers(0, K - 1, n).astype(np.int32)  # cluster K-1 receives nothing
    cn = np.empty_like(c)
    ws = w.copy()
    _minibatch_update_dense(x, np.ones(n), c, cn, ws, labels, 1)
    want_c, want_w = mb_update_fp64(c, w, x, labels)
    assert np.allclose(cn, want_c, rtol=1e-12, atol=1e-12)
    assert np.array_equal(ws, want_w)
    assert np.array_equal(want_c[K - 1], c[K - 1])
