"""k-means kernels on the MI355X (csrc/kmeans.hip through unispeech_amd/kmeans.py) against fp64 restatements and the
fixture tests/golden/kmeans.npz (sklearn fits and the reference's own ApplyKmeans labels, tools/gen_kmeans_golden.py).

Assignment criterion: a label l is accepted when d(l) - d(best) <= 1e-6 (|x|^2 + |c_best|^2) with d in fp64 from the
exact input values; at least 99.9 % of the labels must be the fp64 argmin itself (all of them on the blob data)."""
import os
import wave

import numpy as np
import pytest
import torch

from conftest import TINY, golden_state_dict, load_golden
from test_kmeans import lloyd_update_fp64, mb_update_fp64

pytestmark = pytest.mark.gpu


def _bits(b):
    return (b.astype(np.uint32) << 16).view(np.float32)


def _d64(x, c):
    x = np.asarray(x, np.float64)
    c = np.asarray(c, np.float64)
    return (x * x).sum(1)[:, None] - 2 * x @ c.T + (c * c).sum(1)[None, :]


def _check_labels(x, c, lab, all_exact=False):
    d = _d64(x, c)
    best = d.argmin(1)
    n = np.arange(len(x))
    gap = d[n, lab] - d[n, best]
    bound = 1e-6 * ((np.asarray(x, np.float64) ** 2).sum(1) + (np.asarray(c, np.float64) ** 2).sum(1)[best])
    assert lab.min() >= 0 and lab.max() < len(c)
    assert (gap <= bound).all(), float((gap - bound).max())
    exact = (lab == best).mean()
    assert exact >= (1.0 if all_exact else 0.999), exact
    return d, best, bound


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("N,D,K", [(1, 39, 1), (37, 39, 7), (23968, 39, 100), (37, 64, 500), (2000, 768, 1000),
                                   (23968, 768, 500), (513, 1024, 7), (37, 1024, 1000)])
def test_assign_matches_fp64_argmin(dtype, N, D, K):
    g = torch.Generator().manual_seed(N * 7 + D + K)
    x = torch.randn(N, D + 5, generator=g)[:, 2:2 + D].to(dtype)   # ldx = D + 5 > D
    c = torch.randn(K, D, generator=g)
    from unispeech_amd.kmeans import assign
    lab, dist = assign(x.cuda(), c, return_dist=True)
    lab = lab.cpu().numpy()
    xf = x.float().numpy()
    d, best, _ = _check_labels(xf, c.numpy(), lab)
    want = d[np.arange(N), lab]
    assert np.allclose(dist.cpu().numpy(), want, rtol=1e-5, atol=0)


def test_fixture_blobs_and_reference_labels():
    z = load_golden("kmeans.npz")
    from unispeech_amd.kmeans import ApplyKmeans
    for name in ("blobs", "hard"):
        x = _bits(z[name + "/x_bf16"])
        c = z[name + "/centres"][0]
        app = ApplyKmeans(c)
        for xin in (torch.from_numpy(x).cuda(), torch.from_numpy(x).cuda().bfloat16(), x):
            lab = app(xin)
            assert lab.dtype == np.int64
            d, best, bound = _check_labels(x, c, lab, all_exact=(name == "blobs"))
        ref = z[name + "/ref_labels"]
        n = np.arange(len(x))
        diff = lab != ref
        assert (d[n, ref] - d[n, best] <= bound)[diff].all() and (d[n, lab] - d[n, best] <= bound)[diff].all()
    g = np.random.default_rng(int(z["ties/seed"]))
    x = g.standard_normal((int(z["ties/n"]), 768), dtype=np.float32)
    c = g.standard_normal((int(z["ties/k"]), 768), dtype=np.float32)
    lab = ApplyKmeans(c)(x)
    d, best, bound = _check_labels(x, c, lab)
    ref = z["ties/ref_labels"]
    n = np.arange(len(x))
    assert (d[n, ref] - d[n, best] <= bound)[lab != ref].all()


def test_ties_go_to_the_lowest_index():
    from unispeech_amd.kmeans import assign
    g = torch.Generator().manual_seed(5)
    D, K = 64, 200
    c = torch.randn(K, D, generator=g)
    # duplicates inside one 64-centre tile (3 -> 9) and across tiles (10 -> 70, 130, 199)
    for dup, src in ((9, 3), (70, 10), (130, 10), (199, 10)):
        c[dup] = c[src]
    x = c[[3, 10, 9, 70, 199]].clone()
    for dt in (torch.float32, torch.bfloat16):
        lab = assign(x.to(dt).cuda(), c).cpu().numpy()
        assert lab[:5].tolist() == [3, 10, 3, 10, 10], lab
    # all centres identical: every row takes centre 0
    cc = c[:1].repeat(300, 1)
    assert (assign(torch.randn(100, D, generator=g).cuda(), cc) == 0).all()


def test_accumulate_update_and_determinism():
    z = load_golden("kmeans.npz")
    x = _bits(z["blobs/x_bf16"])
    c0 = z["blobs/centres"][0] + 0.25 * np.random.default_rng(0).standard_normal((32, 64)).astype(np.float32)
    from unispeech_amd import kmeans as KM
    xt = torch.from_numpy(x).cuda()
    C = KM.Centres(c0)
    lab = KM.assign(xt, C)
    lab_np = lab.cpu().numpy()
    _check_labels(x, c0, lab_np, all_exact=True)
    sums, counts = KM.accumulate(xt, lab, 32)
    s2, n2 = KM.accumulate(xt, lab, 32)
    assert torch.equal(sums, s2) and torch.equal(counts, n2)
    assert np.array_equal(counts.cpu().numpy(), np.bincount(lab_np, minlength=32))
    # Lloyd step
    KM.update(C, sums, counts)
    assert np.allclose(C.C.cpu().numpy(), lloyd_update_fp64(c0, x, lab_np), rtol=1e-5, atol=1e-5)
    # mini-batch step on a batch, from given centres and weights
    C = KM.Centres(c0)
    w0 = np.random.default_rng(1).integers(0, 50, 32).astype(np.float32)
    w = torch.from_numpy(w0).cuda()
    xb = xt[:500]
    lb = KM.assign(xb, C)
    sb, nb = KM.accumulate(xb, lb, 32)
    KM.update(C, sb, nb, w)
    want_c, want_w = mb_update_fp64(c0, w0, x[:500], lb.cpu().numpy())
    assert np.allclose(C.C.cpu().numpy(), want_c, rtol=1e-5, atol=1e-5)
    assert np.array_equal(w.cpu().numpy().astype(np.float64), want_w)
    # skew: every row in one cluster (many chunks of one list), bf16 input, bitwise repeatable
    one = torch.full((x.shape[0],), 5, dtype=torch.int32, device="cuda")
    xb16 = xt.bfloat16()
    a, na = KM.accumulate(xb16, one, 32)
    b, nb_ = KM.accumulate(xb16, one, 32)
    assert torch.equal(a, b) and torch.equal(na, nb_)
    assert int(na[5]) == x.shape[0] and int(na.sum()) == x.shape[0]
    assert np.allclose(a[5].cpu().numpy(), x.astype(np.float64).sum(0), rtol=1e-5, atol=1e-3)
    assert (a[torch.arange(32) != 5] == 0).all()


@pytest.mark.parametrize("name", ["blobs", "hard"])
def test_fit_quality_and_determinism(name):
    z = load_golden("kmeans.npz")
    x = torch.from_numpy(_bits(z[name + "/x_bf16"])).cuda()
    from unispeech_amd.kmeans import MiniBatchKMeans, assign
    kw = dict(n_clusters=int(z[name + "/k"]), batch_size=int(z[name + "/batch_size"]), max_iter=100, tol=0.0,
              max_no_improvement=100, n_init=20, reassignment_ratio=0.0, seed=3)
    km = MiniBatchKMeans(**kw).fit(x)
    assert km.inertia_ <= 1.01 * float(z[name + "/inertia"].max()), (km.inertia_, z[name + "/inertia"])
    _, d = assign(x, km.cluster_centers_, return_dist=True)
    assert abs(km.inertia_ - d.double().sum().item()) <= 1e-9 * km.inertia_
    assert abs(km.score(x) + km.inertia_) <= 1e-9 * km.inertia_
    km2 = MiniBatchKMeans(**kw).fit(x)
    assert np.array_equal(km.cluster_centers_, km2.cluster_centers_)
    if name == "blobs":
        ll = MiniBatchKMeans(algorithm="lloyd", **kw).fit(x)
        assert ll.inertia_ <= 1.01 * float(z[name + "/inertia"].max())


def _tiny_model():
    from unispeech_amd.wavlm import WavLM, WavLMConfig
    z = load_golden("tiny_wavlm.npz")
    sd = golden_state_dict(z)
    m = WavLM(WavLMConfig(dict(TINY)))
    m.load_state_dict(sd)
    return m.cuda().eval(), sd, z


def _feature_bound(lab, best, c, xg, xo):
    """a feature error e moves d(x, a) - d(x, b) by at most 2 |e| |c_a - c_b|"""
    e = np.linalg.norm(xg - xo, axis=1)
    return 2 * e * np.linalg.norm(c[lab] - c[best], axis=1) + 1e-5


def test_label_audio_and_dump_labels_end_to_end(tmp_path):
    from conftest import Cfg
    from oracle import wavlm_oracle as O
    from unispeech_amd.kmeans import dump_labels, label_audio, read_wav
    model, sd, z = _tiny_model()
    rng = np.random.default_rng(0)
    pcm = [rng.integers(-8000, 8000, n).astype("<i2") for n in (20000, 13000)]
    root = tmp_path / "audio"
    root.mkdir()
    for i, s in enumerate(pcm):
        with wave.open(str(root / ("u%d.wav" % i)), "wb") as w:
            w.setnchannels(1)
            w.setsampwidth(2)
            w.setframerate(16000)
            w.writeframes(s.tobytes())
    (tmp_path / "train.tsv").write_text("%s\nu0.wav\t20000\nu1.wav\t13000\n" % root)
    cfg = Cfg(**TINY)
    lines = []
    c = None
    for i in range(2):
        wav, _ = read_wav(str(root / ("u%d.wav" % i)))
        xo = torch.cat([O.extract_features(sd, cfg, torch.from_numpy(wav).float().view(1, -1)[:, s:s + 8000],
                                           output_layer=1)["x"] for s in range(0, len(wav), 8000)], 1)[0].numpy()
        if c is None:
            c = xo[::3][:16].astype(np.float32).copy()
        lab = label_audio(model, wav, 1, c, max_chunk=8000).cpu().numpy()
        from unispeech_amd.kmeans import _get_feats
        xg = _get_feats(model, wav, 1, 8000, False).float().cpu().numpy()
        d = _d64(xo, c)
        best = d.argmin(1)
        n = np.arange(len(xo))
        assert len(lab) == len(xo)
        assert (d[n, lab] - d[n, best] <= _feature_bound(lab, best, c, xg, xo)).all()
        lines.append(" ".join(map(str, lab.tolist())) + "\n")
    np.save(str(tmp_path / "km.npy"), c)
    out = dump_labels(str(tmp_path), "train", model, 1, str(tmp_path / "km.npy"), 1, 0, str(tmp_path / "lab"),
                      max_chunk=8000)
    assert os.path.basename(out) == "train_0_1.km"
    assert open(out).read() == "".join(lines)
    assert open(tmp_path / "lab" / "dict.km.txt").read() == "".join("%d 1\n" % i for i in range(16))


def test_base_width_labels():
    from unispeech_amd.kmeans import ApplyKmeans, label_audio
    from unispeech_amd.wavlm import WavLM, WavLMConfig
    torch.manual_seed(0)
    m = WavLM(WavLMConfig({})).cuda().to(torch.bfloat16).eval()
    g = torch.Generator().manual_seed(1)
    wavs = [torch.randn(240000, generator=g) * 0.1 for _ in range(2)]
    from unispeech_amd.kmeans import _get_feats
    feats = [_get_feats(m, w, 9, 1_600_000, False) for w in wavs]
    allf = torch.cat(feats).float()
    c = allf[torch.randperm(allf.size(0), generator=g)[:500].cuda()].clone()
    app = ApplyKmeans(c)
    for w, f in zip(wavs, feats):
        lab = label_audio(m, w, 9, app).cpu().numpy()
        xf = f.float().cpu().numpy()
        d, best, bound = _check_labels(xf, c.cpu().numpy(), lab)
        # the reference formula run through torch on the device (fp32), agreeing except at near-ties
        ff = f.float()
        tl = (ff.pow(2).sum(1, keepdim=True) - 2 * ff @ c.t() + c.pow(2).sum(1)[None]).argmin(1).cpu().numpy()
        n = np.arange(len(xf))
        near = d[n, tl] - d[n, best] <= 1e-5 * ((xf.astype(np.float64) ** 2).sum(1) + (c.double().cpu().numpy() ** 2).sum(1)[best])
        assert near[tl != lab].all()
