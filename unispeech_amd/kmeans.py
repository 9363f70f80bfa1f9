"""k-means units for HuBERT / WavLM pre-training targets, on the device (csrc/kmeans.hip, ABI 22).

Replaces the reference's src/examples/hubert/simple_kmeans/ steps 2 and 3:
  * `MiniBatchKMeans`  -- learn_kmeans.py (sklearn MiniBatchKMeans with the recipe's flags): k-means++ inits on a
    subsample, the best by inertia on a validation subsample, mini-batch steps with sklearn's update rule and its
    EWA-inertia / max_no_improvement stop; `algorithm="lloyd"` runs full-batch iterations on the same kernels.
  * `ApplyKmeans`      -- dump_km_label.py:25-47, same call interface (numpy int64 labels); `assign` stays on the device.
  * `label_audio` / `dump_labels` -- dump_hubert_feature.py's chunked `get_feats` straight into the assignment, so no
    feature file is written; `dump_features` writes the reference's `.npy` / `.len` pair for interchange.
  * `features="mfcc"` (`label_audio`, `dump_labels`, `dump_mfcc_features`) -- iteration 1 of the recipe, which has no model
    yet: dump_mfcc_feature.py's 39-wide Kaldi MFCCs from the device op of unispeech_amd/mfcc.py (csrc/mfcc.hip).
`python -m unispeech_amd.kmeans {learn,dump_label,label_audio,dump_mfcc}` takes the reference scripts' positional arguments.
"""
import math
import os
import wave

import numpy as np
import torch

from . import _lib

__all__ = ["ApplyKmeans", "MiniBatchKMeans", "assign", "accumulate", "label_audio", "dump_labels", "dump_features",
           "dump_mfcc_features", "read_wav", "get_path_iterator"]


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _features(x):
    """device [N, D] view the kernels read: fp32 or bf16, unit column stride (any row stride)"""
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    if not x.is_cuda:
        x = x.cuda()
    if x.dim() != 2:
        raise ValueError("features must be 2-D [N, D], got shape %s" % (tuple(x.shape),))
    if x.dtype not in (torch.float32, torch.bfloat16):
        x = x.float()
    if x.stride(1) != 1 or x.stride(0) < x.size(1):
        x = x.contiguous()
    return x


def _dt(x):
    return _lib.BF16 if x.dtype == torch.bfloat16 else _lib.F32


class Centres:
    """fp32 centres [K, D] and the image the assignment kernel reads (padded rows + squared norms)."""

    def __init__(self, centres):
        c = torch.as_tensor(centres) if not isinstance(centres, torch.Tensor) else centres
        c = c.detach().to(device="cuda", dtype=torch.float32).contiguous()
        if c.dim() != 2 or c.size(0) < 1 or c.size(1) < 1:
            raise ValueError("centres must be [K, D] with K, D >= 1")
        self.C = c
        self.K, self.D = c.shape
        nbytes = _lib.lib().wavlm_kmeans_centres_bytes(self.K, self.D)
        self.image = torch.empty(nbytes // 4, dtype=torch.float32, device=c.device)
        self.refresh()

    def refresh(self):
        """rebuild the image after self.C changed (the update kernel writes C in place)"""
        _lib.check(_lib.lib().wavlm_kmeans_prepare(self.C.data_ptr(), self.K, self.D, self.image.data_ptr(),
                                                   self.image.numel() * 4, _stream()), "wavlm_kmeans_prepare")


def assign(x, centres, return_dist=False):
    """labels int32 [N] (ties -> lowest index) and optionally min_dist fp32 [N] = |x - c_label|^2; device, no sync"""
    x = _features(x)
    if not isinstance(centres, Centres):
        centres = Centres(centres)
    N, D = x.shape
    if D != centres.D:
        raise ValueError("feature width %d != centre width %d" % (D, centres.D))
    labels = torch.empty(N, dtype=torch.int32, device=x.device)
    dist = torch.empty(N, dtype=torch.float32, device=x.device) if return_dist else None
    if N:
        _lib.check(_lib.lib().wavlm_kmeans_assign(x.data_ptr(), _dt(x), N, D, x.stride(0), centres.image.data_ptr(),
                                                  centres.K, labels.data_ptr(), dist.data_ptr() if return_dist else None,
                                                  _stream()), "wavlm_kmeans_assign")
    return (labels, dist) if return_dist else labels


def accumulate(x, labels, K):
    """per-cluster sums fp32 [K, D] and counts int32 [K]; bitwise reproducible"""
    x = _features(x)
    N, D = x.shape
    labels = labels.to(device=x.device, dtype=torch.int32).contiguous()
    if labels.numel() != N:
        raise ValueError("labels: %d entries for %d rows" % (labels.numel(), N))
    sums = torch.empty(K, D, dtype=torch.float32, device=x.device)
    counts = torch.empty(K, dtype=torch.int32, device=x.device)
    L = _lib.lib()
    ws_bytes = L.wavlm_kmeans_accumulate_workspace_bytes(N, K, D)
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=x.device)
    _lib.check(L.wavlm_kmeans_accumulate(x.data_ptr(), _dt(x), N, D, x.stride(0), labels.data_ptr(), K, sums.data_ptr(),
                                         counts.data_ptr(), ws.data_ptr(), ws_bytes, _stream()), "wavlm_kmeans_accumulate")
    return sums, counts


def update(centres, sums, counts, weights=None):
    """in place: Lloyd (weights None: c = sums / n) or mini-batch (c = (c w + sums) / (w + n), w += n); empty clusters
    keep their centre.  Refreshes the image."""
    mode = 0 if weights is None else 1
    _lib.check(_lib.lib().wavlm_kmeans_update(centres.C.data_ptr(), weights.data_ptr() if weights is not None else None,
                                              sums.data_ptr(), counts.data_ptr(), centres.K, centres.D, mode, _stream()),
               "wavlm_kmeans_update")
    centres.refresh()


def _load_centres(km):
    if isinstance(km, (str, os.PathLike)):
        p = os.fspath(km)
        if p.endswith(".npz"):
            z = np.load(p)
            return np.asarray(z["cluster_centers_"] if "cluster_centers_" in z.files else z[z.files[0]])
        if p.endswith(".npy"):
            return np.load(p)
        import joblib  # a joblib file written by sklearn (the reference's km_path); only cluster_centers_ is read
        return np.asarray(joblib.load(p).cluster_centers_)
    if isinstance(km, MiniBatchKMeans):
        return km.cluster_centers_
    if hasattr(km, "cluster_centers_"):
        return np.asarray(km.cluster_centers_)
    return km


class ApplyKmeans:
    """drop-in for dump_km_label.ApplyKmeans: `km` is a joblib file of a fitted sklearn model, an .npz / .npy of centres,
    a fitted MiniBatchKMeans or an array [K, D]"""

    def __init__(self, km):
        self.centres = Centres(_load_centres(km))

    def assign(self, x, return_dist=False):
        return assign(x, self.centres, return_dist)

    def __call__(self, x):
        return self.assign(x).cpu().numpy().astype(np.int64)


class MiniBatchKMeans:
    """sklearn.cluster.MiniBatchKMeans (as learn_kmeans.py configures it) on the device kernels.

    Random numbers come from a seeded torch CPU generator of this class, not from numpy: same seed and input give
    bit-identical centres, but not sklearn's centres.  Not supported (NotImplementedError): reassignment_ratio > 0 and
    any init other than "k-means++" or an explicit [K, D] array."""

    def __init__(self, n_clusters=8, init="k-means++", max_iter=100, batch_size=1024, tol=0.0, max_no_improvement=10,
                 n_init=3, reassignment_ratio=0.0, seed=0, init_size=None, algorithm="minibatch", verbose=0):
        if reassignment_ratio and reassignment_ratio > 0:
            raise NotImplementedError("MiniBatchKMeans: reassignment_ratio > 0 (random reassignment of small clusters) "
                                      "is not implemented; the recipe uses 0")
        if isinstance(init, str) and init != "k-means++":
            raise NotImplementedError("MiniBatchKMeans: init=%r is not implemented (k-means++ or an array)" % (init,))
        if algorithm not in ("minibatch", "lloyd"):
            raise NotImplementedError("MiniBatchKMeans: algorithm=%r is not implemented (minibatch, lloyd)" % (algorithm,))
        self.n_clusters, self.init, self.max_iter, self.batch_size = int(n_clusters), init, int(max_iter), int(batch_size)
        self.tol, self.max_no_improvement, self.n_init = float(tol), max_no_improvement, int(n_init)
        self.reassignment_ratio, self.seed, self.init_size = reassignment_ratio, int(seed), init_size
        self.algorithm, self.verbose = algorithm, verbose
        self._centres = None
        self.inertia_ = None

    # -- sklearn surface
    @property
    def cluster_centers_(self):
        return None if self._centres is None else self._centres.C.cpu().numpy()

    def _inertia(self, x, centres):
        _, d = assign(x, centres, return_dist=True)
        return d.double().sum()

    def predict(self, X):
        return assign(X, self._centres).cpu().numpy().astype(np.int64)

    def score(self, X):
        return -float(self._inertia(_features(X), self._centres))

    # -- fitting
    def _kmeanspp(self, x, g):
        """sklearn _kmeans_plusplus (greedy, 2 + int(log k) local trials); distances through the assignment kernel"""
        n, K = x.size(0), self.n_clusters
        trials = 2 + int(np.log(K))
        ids = [int(torch.randint(0, n, (1,), generator=g))]
        first = x[ids[0]:ids[0] + 1]
        closest = assign(x, Centres(first.float()), return_dist=True)[1].double()
        pot = closest.sum()
        rows = [first.float()]
        for _ in range(1, K):
            u = torch.rand(trials, generator=g, dtype=torch.float64).to(x.device)
            cand = torch.searchsorted(torch.cumsum(closest, 0), u * pot).clamp_(max=n - 1)
            cx = x.index_select(0, cand).float()
            d = torch.stack([assign(x, Centres(cx[t:t + 1]), return_dist=True)[1] for t in range(trials)]).double()
            d = torch.minimum(d, closest.unsqueeze(0))
            pots = d.sum(1)
            b = torch.argmin(pots)
            pot, closest = pots[b], d[b]
            rows.append(cx.index_select(0, b.view(1)))
        return torch.cat(rows, 0)

    def fit(self, X):
        x = _features(X)
        n = x.size(0)
        K = self.n_clusters
        if n < K:
            raise ValueError("n_samples=%d should be >= n_clusters=%d" % (n, K))
        g = torch.Generator().manual_seed(self.seed)
        init_size = self.init_size if self.init_size is not None else 3 * self.batch_size
        init_size = min(max(init_size, K), n)
        valid = x.index_select(0, torch.randint(0, n, (init_size,), generator=g).to(x.device))
        if not isinstance(self.init, str):
            best = Centres(self.init)
        else:
            best, best_inertia = None, None
            for _ in range(self.n_init):
                sub = x.index_select(0, torch.randint(0, n, (init_size,), generator=g).to(x.device))
                c = Centres(self._kmeanspp(sub, g))
                inertia = float(self._inertia(valid, c))
                if best_inertia is None or inertia < best_inertia:
                    best, best_inertia = c, inertia
        self._centres = best
        if self.algorithm == "lloyd":
            self._fit_lloyd(x)
        else:
            self._fit_minibatch(x, g)
        self.inertia_ = float(self._inertia(x, self._centres))
        return self

    def _fit_minibatch(self, x, g):
        n, K, bs = x.size(0), self.n_clusters, min(self.batch_size, x.size(0))
        c = self._centres
        weights = torch.zeros(K, dtype=torch.float32, device=x.device)
        tol = 0.0
        if self.tol > 0:  # sklearn _tolerance: tol * mean feature variance
            tol = float(x.float().var(0, unbiased=False).mean()) * self.tol
        n_steps = (self.max_iter * n) // bs
        ewa, ewa_min, no_improvement = None, None, 0
        self.n_steps_ = 0
        for i in range(n_steps):
            xb = x.index_select(0, torch.randint(0, n, (bs,), generator=g).to(x.device))
            labels, d = assign(xb, c, return_dist=True)
            batch_inertia = d.double().sum()
            old = c.C.clone() if tol > 0 else None
            sums, counts = accumulate(xb, labels, K)
            update(c, sums, counts, weights)
            self.n_steps_ = i + 1
            # sklearn MiniBatchKMeans._mini_batch_convergence
            if i == 0:
                continue
            bi = float(batch_inertia) / bs
            if ewa is None:
                ewa = bi
            else:
                alpha = min(bs * 2.0 / (n + 1), 1.0)
                ewa = ewa * (1 - alpha) + bi * alpha
            if tol > 0 and float(((c.C - old) ** 2).sum()) <= tol:
                break
            if ewa_min is None or ewa < ewa_min:
                no_improvement, ewa_min = 0, ewa
            else:
                no_improvement += 1
            if self.max_no_improvement is not None and no_improvement >= self.max_no_improvement:
                break
        self.n_iter_ = int(math.ceil(self.n_steps_ * bs / n))

    def _fit_lloyd(self, x):
        """full-batch iterations; an empty cluster keeps its centre (sklearn KMeans relocates it instead)"""
        c, K = self._centres, self.n_clusters
        prev = None
        self.n_iter_ = 0
        for i in range(self.max_iter):
            labels = assign(x, c)
            old = c.C.clone()
            sums, counts = accumulate(x, labels, K)
            update(c, sums, counts)
            self.n_iter_ = i + 1
            if prev is not None and torch.equal(prev, labels):
                break
            if self.tol > 0 and float(((c.C - old) ** 2).sum()) <= self.tol:
                break
            prev = labels

    def save(self, path):
        """`path`.npz (cluster_centers_, inertia_); if sklearn is importable also `path` as a joblib file that the
        reference's dump_km_label.ApplyKmeans loads (an sklearn MiniBatchKMeans with cluster_centers_ set)"""
        centres = self.cluster_centers_
        base = path[:-4] if path.endswith(".npz") else path
        np.savez(base + ".npz", cluster_centers_=centres, inertia_=np.float64(self.inertia_ or 0.0))
        written = [base + ".npz"]
        try:
            import joblib
            from sklearn.cluster import MiniBatchKMeans as SkMBK
        except ImportError:
            return written
        km = SkMBK(n_clusters=self.n_clusters, max_iter=self.max_iter, batch_size=self.batch_size, tol=self.tol,
                   max_no_improvement=self.max_no_improvement, n_init=self.n_init, reassignment_ratio=0.0,
                   compute_labels=False)
        km.cluster_centers_ = centres
        km.n_features_in_ = centres.shape[1]
        km._n_threads = 1
        if self.inertia_ is not None:
            km.inertia_ = self.inertia_
        joblib.dump(km, path if path != base + ".npz" else base + ".joblib")
        written.append(path if path != base + ".npz" else base + ".joblib")
        return written


# ---------------------------------------------------------------------------------------------------- audio -> labels
def read_wav(path):
    """16-bit PCM wav as float64 in [-1, 1) (soundfile.read's values: int16 / 32768), channels averaged like the
    reference's read_audio; returns (wav, sample_rate).  Anything but 16-bit PCM is refused by name."""
    try:
        w = wave.open(path, "rb")
    except wave.Error as e:
        raise NotImplementedError("read_wav: %s is not a PCM wav file (%s); only 16-bit PCM is read" % (path, e))
    with w:
        if w.getcomptype() != "NONE" or w.getsampwidth() != 2:
            raise NotImplementedError("read_wav: %s: sample width %d bytes / compression %s; only 16-bit PCM is read"
                                      % (path, w.getsampwidth(), w.getcomptype()))
        ch, sr = w.getnchannels(), w.getframerate()
        data = np.frombuffer(w.readframes(w.getnframes()), dtype="<i2").astype(np.float64) / 32768.0
    if ch > 1:
        data = data.reshape(-1, ch).mean(-1)
    return data, sr


def get_path_iterator(tsv, nshard, rank):
    """dump_hubert_feature.get_path_iterator: shard `rank` of `nshard` of the manifest (ceil-sized shards)"""
    with open(tsv, "r") as f:
        root = f.readline().rstrip()
        lines = [line.rstrip() for line in f]
    tot = len(lines)
    shard_size = math.ceil(tot / nshard)
    start, end = rank * shard_size, min((rank + 1) * shard_size, tot)
    assert start < end, "start=%d, end=%d" % (start, end)
    lines = lines[start:end]

    def iterate():
        for line in lines:
            subpath, nsample = line.split("\t")[:2]
            yield os.path.join(root, subpath), int(nsample)

    return iterate, len(lines)


def _get_feats(model, wav, layer, max_chunk, normalize):
    x = torch.as_tensor(wav)
    x = x.to(device="cuda", dtype=torch.float32)
    if normalize:
        x = torch.nn.functional.layer_norm(x, x.shape)
    x = x.view(1, -1)
    dt = next(model.parameters()).dtype
    feats = []
    with torch.no_grad():
        for start in range(0, x.size(1), max_chunk):
            chunk = x[:, start:start + max_chunk].to(dt)
            f, _ = model.extract_features(source=chunk, padding_mask=None, mask=False, output_layer=layer)
            feats.append(f)
    return torch.cat(feats, 1).squeeze(0)


def _normalize_flag(model, normalize):
    if normalize is not None:
        return bool(normalize)
    return bool(getattr(getattr(model, "cfg", None), "normalize", False))


def _check_features(model, features):
    if features not in (None, "mfcc"):
        raise NotImplementedError("features=%r is not implemented (None: a model's layer states, 'mfcc')" % (features,))
    if features == "mfcc" and model is not None:
        raise ValueError("features='mfcc' takes model=None: the first iteration has no model")
    if features is None and model is None:
        raise ValueError("model=None needs features='mfcc'")


def _mfcc_wave(wav):
    """what dump_mfcc_feature.get_feats feeds kaldi.mfcc: the waveform as float32 (int16 PCM stays PCM), on the device"""
    x = torch.as_tensor(wav)
    if x.dtype != torch.int16:
        x = x.to(torch.float32)
    return x.reshape(-1).cuda()


def label_audio(model, wav, layer, km, max_chunk=1_600_000, normalize=None, features=None, sample_rate=16000):
    """dump_hubert_feature.get_feats (chunks of max_chunk samples, output_layer=layer, layer_norm of the waveform when
    the model's cfg.normalize is set) followed by the assignment, on the device: int32 labels, no host sync.
    model=None, features="mfcc": dump_mfcc_feature.get_feats at `sample_rate` instead (layer, max_chunk, normalize unused)"""
    _check_features(model, features)
    app = km if isinstance(km, ApplyKmeans) else ApplyKmeans(km)
    if features == "mfcc":
        from .mfcc import mfcc
        return app.assign(mfcc(_mfcc_wave(wav), sample_rate)[0])
    feats = _get_feats(model, wav, layer, max_chunk, _normalize_flag(model, normalize))
    return app.assign(feats)


def _check_rate(path, sr, want=16000):
    if sr != want:
        raise ValueError("%s: sample rate %d, the model expects %d" % (path, sr, want))


def _mfcc_batches(generator, sample_rate, max_batch_samples):
    """the shard's waveforms (float32, on the device) in manifest order, grouped into lists whose padded size B * Lmax stays
    within max_batch_samples (a longer utterance goes alone): one mfcc launch each"""
    batch, longest = [], 0
    for path, _ in generator():
        wav, sr = read_wav(path)
        _check_rate(path, sr, sample_rate)
        if batch and (len(batch) + 1) * max(longest, len(wav)) > max_batch_samples:
            yield batch
            batch, longest = [], 0
        batch.append(_mfcc_wave(wav))
        longest = max(longest, len(wav))
    if batch:
        yield batch


def _mfcc_utterances(generator, sample_rate, max_batch_samples):
    """-> per utterance of the shard its [frames, 39] device features; a row's bits do not depend on the batch it was in"""
    from .mfcc import mfcc
    for batch in _mfcc_batches(generator, sample_rate, max_batch_samples):
        feats, frames = mfcc(batch, sample_rate)
        for r, n in enumerate(frames):
            yield feats[r, :n]


def dump_labels(tsv_dir, split, model, layer, km, nshard, rank, lab_dir, max_chunk=1_600_000, normalize=None, features=None,
                sample_rate=16000, max_batch_samples=1 << 24):
    """waveforms of shard `rank` -> `{lab_dir}/{split}_{rank}_{nshard}.km` (dump_km_label.py's line format) and
    `{lab_dir}/dict.km.txt`; no feature file.  model=None, features="mfcc": waveform -> MFCC -> assignment, the shard's
    utterances batched into launches of at most max_batch_samples padded samples (no label depends on the batching)"""
    _check_features(model, features)
    app = km if isinstance(km, ApplyKmeans) else ApplyKmeans(km)
    norm = _normalize_flag(model, normalize)
    generator, _ = get_path_iterator(os.path.join(tsv_dir, split + ".tsv"), nshard, rank)
    os.makedirs(lab_dir, exist_ok=True)
    lab_path = os.path.join(lab_dir, "%s_%d_%d.km" % (split, rank, nshard))
    with open(lab_path, "w") as f:
        if features == "mfcc":
            for feat in _mfcc_utterances(generator, sample_rate, max_batch_samples):
                f.write(" ".join(map(str, app.assign(feat).cpu().numpy().astype(np.int64).tolist())) + "\n")
        else:
            for path, _ in generator():
                wav, sr = read_wav(path)
                _check_rate(path, sr)
                lab = app.assign(_get_feats(model, wav, layer, max_chunk, norm)).cpu().numpy().astype(np.int64).tolist()
                f.write(" ".join(map(str, lab)) + "\n")
    with open(os.path.join(lab_dir, "dict.km.txt"), "w") as f:
        for i in range(app.centres.K):
            f.write("%d 1\n" % i)
    return lab_path


def dump_features(tsv_dir, split, model, layer, nshard, rank, feat_dir, max_chunk=1_600_000, normalize=None):
    """dump_hubert_feature.dump_feature: `{split}_{rank}_{nshard}.npy` (fp32 [frames, D]) + `.len` (frames per utterance)"""
    norm = _normalize_flag(model, normalize)
    generator, _ = get_path_iterator(os.path.join(tsv_dir, split + ".tsv"), nshard, rank)

    def feats():
        for path, _ in generator():
            wav, sr = read_wav(path)
            _check_rate(path, sr)
            yield _get_feats(model, wav, layer, max_chunk, norm)

    return _write_feature_shard(feats(), feat_dir, split, nshard, rank)


def dump_mfcc_features(tsv_dir, split, sample_rate, nshard, rank, feat_dir, max_batch_samples=1 << 24):
    """dump_mfcc_feature.dump_feature: the same `.npy` (fp32 [frames, 39]) / `.len` pair from the device MFCC op"""
    generator, _ = get_path_iterator(os.path.join(tsv_dir, split + ".tsv"), nshard, rank)
    return _write_feature_shard(_mfcc_utterances(generator, sample_rate, max_batch_samples), feat_dir, split, nshard, rank,
                                width=39)


def _write_feature_shard(feats, feat_dir, split, nshard, rank, width=None):
    """per-utterance [frames, D] tensors -> `{split}_{rank}_{nshard}.npy` + `.len`, streamed through a raw part file"""
    os.makedirs(feat_dir, exist_ok=True)
    stem = os.path.join(feat_dir, "%s_%d_%d" % (split, rank, nshard))
    raw = stem + ".npy.part"
    total = 0
    with open(raw, "wb") as rf, open(stem + ".len", "w") as lf:
        for feat in feats:
            feat = feat.float().cpu().numpy()
            width = feat.shape[1]
            rf.write(np.ascontiguousarray(feat, dtype="<f4").tobytes())
            total += feat.shape[0]
            lf.write("%d\n" % len(feat))
    with open(stem + ".npy", "wb") as out, open(raw, "rb") as rf:
        np.lib.format.write_array_header_1_0(out, {"descr": "<f4", "fortran_order": False, "shape": (total, width or 0)})
        while True:
            b = rf.read(1 << 24)
            if not b:
                break
            out.write(b)
    os.remove(raw)
    return stem + ".npy", stem + ".len"


def get_feat_iterator(feat_dir, split, nshard, rank):
    """dump_km_label.get_feat_iterator: the utterances of one `.npy` / `.len` pair"""
    stem = os.path.join(feat_dir, "%s_%d_%d" % (split, rank, nshard))
    with open(stem + ".len") as f:
        lengs = [int(line.rstrip()) for line in f]
    offsets = [0] + np.cumsum(lengs[:-1]).tolist()

    def iterate():
        feat = np.load(stem + ".npy", mmap_mode="r")
        assert feat.shape[0] == offsets[-1] + lengs[-1]
        for o, n in zip(offsets, lengs):
            yield feat[o:o + n]

    return iterate, len(lengs)


def load_feature(feat_dir, split, nshard, seed, percent):
    """learn_kmeans.load_feature (numpy seeded with `seed`; percent < 0: every frame)"""
    np.random.seed(seed)
    out = []
    for r in range(nshard):
        stem = os.path.join(feat_dir, "%s_%d_%d" % (split, r, nshard))
        if percent < 0:
            out.append(np.load(stem + ".npy", mmap_mode="r"))
            continue
        with open(stem + ".len") as f:
            lengs = [int(line.rstrip()) for line in f]
        offsets = [0] + np.cumsum(lengs[:-1]).tolist()
        k = int(np.ceil(len(lengs) * percent))
        idx = np.random.choice(len(lengs), k, replace=False)
        feat = np.load(stem + ".npy", mmap_mode="r")
        out.append(np.concatenate([feat[offsets[i]:offsets[i] + lengs[i]] for i in idx], axis=0))
    return np.concatenate(out, axis=0)


def load_model(ckpt_path):
    """the checkpoint forms INTEGRATION section 2 documents: a dict with `cfg` + `model` (standalone WavLM)"""
    from .wavlm import WavLM, WavLMConfig
    ckpt = torch.load(ckpt_path, map_location="cpu", weights_only=False)
    if not (isinstance(ckpt, dict) and "cfg" in ckpt and "model" in ckpt):
        raise NotImplementedError("%s: only the standalone checkpoint dict {'cfg', 'model'} is loaded (no fairseq "
                                  "load_model_ensemble_and_task path)" % ckpt_path)
    model = WavLM(WavLMConfig(ckpt["cfg"]))
    model.load_state_dict(ckpt["model"])
    return model.cuda().eval()


def _layer_arg(v):
    """label_audio's LAYER: an integer, or '-' where --features mfcc makes it unused"""
    return None if v == "-" else int(v)


def _parser():
    import argparse
    ap = argparse.ArgumentParser(prog="python -m unispeech_amd.kmeans")
    sub = ap.add_subparsers(dest="cmd", required=True)
    p = sub.add_parser("learn", help="learn_kmeans.py")
    for a, t in (("feat_dir", str), ("split", str), ("nshard", int), ("km_path", str), ("n_clusters", int)):
        p.add_argument(a, type=t)
    p.add_argument("--seed", default=0, type=int)
    p.add_argument("--percent", default=-1, type=float)
    p.add_argument("--init", default="k-means++")
    p.add_argument("--max_iter", default=100, type=int)
    p.add_argument("--batch_size", default=10000, type=int)
    p.add_argument("--tol", default=0.0, type=float)
    p.add_argument("--max_no_improvement", default=100, type=int)
    p.add_argument("--n_init", default=20, type=int)
    p.add_argument("--reassignment_ratio", default=0.0, type=float)
    p = sub.add_parser("dump_label", help="dump_km_label.py")
    for a, t in (("feat_dir", str), ("split", str), ("km_path", str), ("nshard", int), ("rank", int), ("lab_dir", str)):
        p.add_argument(a, type=t)
    p = sub.add_parser("label_audio", help="waveforms -> .km labels, no feature dump")
    for a, t in (("tsv_dir", str), ("split", str), ("ckpt_path", str), ("layer", _layer_arg), ("km_path", str), ("nshard", int),
                 ("rank", int), ("lab_dir", str)):
        p.add_argument(a, type=t)
    p.add_argument("--max_chunk", default=1600000, type=int)
    p.add_argument("--features", default=None, choices=["mfcc"], help="mfcc: iteration 1, ckpt_path and layer are ignored ('-')")
    p.add_argument("--sample_rate", default=16000, type=int, help="with --features mfcc")
    p = sub.add_parser("dump_mfcc", help="dump_mfcc_feature.py")
    for a, t in (("tsv_dir", str), ("split", str), ("nshard", int), ("rank", int), ("feat_dir", str)):
        p.add_argument(a, type=t)
    p.add_argument("--sample_rate", default=16000, type=int)
    return ap


def main(argv=None):
    a = _parser().parse_args(argv)
    if a.cmd == "learn":
        feat = load_feature(a.feat_dir, a.split, a.nshard, a.seed, a.percent)
        km = MiniBatchKMeans(n_clusters=a.n_clusters, init=a.init, max_iter=a.max_iter, batch_size=a.batch_size, tol=a.tol,
                             max_no_improvement=a.max_no_improvement, n_init=a.n_init,
                             reassignment_ratio=a.reassignment_ratio, seed=a.seed).fit(feat)
        km.save(a.km_path)
        print("total inertia: %.5f" % (km.inertia_ / len(feat)))
    elif a.cmd == "dump_label":
        app = ApplyKmeans(a.km_path)
        generator, _ = get_feat_iterator(a.feat_dir, a.split, a.nshard, a.rank)
        os.makedirs(a.lab_dir, exist_ok=True)
        with open(os.path.join(a.lab_dir, "%s_%d_%d.km" % (a.split, a.rank, a.nshard)), "w") as f:
            for feat in generator():
                f.write(" ".join(map(str, app(np.asarray(feat)).tolist())) + "\n")
    elif a.cmd == "dump_mfcc":
        dump_mfcc_features(a.tsv_dir, a.split, a.sample_rate, a.nshard, a.rank, a.feat_dir)
    elif a.features == "mfcc":
        dump_labels(a.tsv_dir, a.split, None, None, a.km_path, a.nshard, a.rank, a.lab_dir, features="mfcc",
                    sample_rate=a.sample_rate)
    else:
        if a.layer is None:
            raise SystemExit("label_audio: LAYER '-' needs --features mfcc")
        dump_labels(a.tsv_dir, a.split, load_model(a.ckpt_path), a.layer, a.km_path, a.nshard, a.rank, a.lab_dir,
                    a.max_chunk)


if __name__ == "__main__":
    main()
