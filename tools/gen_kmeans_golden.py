"""Generate tests/golden/kmeans.npz: sklearn MiniBatchKMeans results and the reference's own ApplyKmeans labels
(src/examples/hubert/simple_kmeans/dump_km_label.py, numpy path) on small fixed datasets.

Runs where sklearn, joblib and the reference tree exist:  python tools/gen_kmeans_golden.py [REFERENCE_ROOT]
(default REFERENCE_ROOT: $UNISPEECH_REF, else ../reference next to the repository).  The GPU tests read only the .npz.

Contents (bf16-exact data is stored as raw bf16 bits, uint16):
  blobs/x_bf16     4096 x 64, 32 well-separated Gaussian blobs
  hard/x_bf16      1024 x 128, Student-t (3 dof) entries: heavy tails, no cluster structure
  <set>/k, <set>/batch_size          the fit's n_clusters / batch_size (other flags: the recipe's, learn_kmeans.py)
  <set>/centres    [5, k, D] fp32    sklearn centres for random_state 0..4
  <set>/inertia    [5] fp64          -score(x) of each
  <set>/ref_labels [N] int64         reference ApplyKmeans labels of x against the seed-0 centres
  ties/seed, ties/n, ties/k          regenerate x = default_rng(seed).standard_normal((n, 768), float32) and
                                     c = the next standard_normal((k, 768), float32)
  ties/ref_labels  [n] int64         reference ApplyKmeans labels of x against c
"""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECIPE = dict(init="k-means++", max_iter=100, tol=0.0, max_no_improvement=100, n_init=20, reassignment_ratio=0.0)


def bf16_bits(x):
    """round-to-nearest-even fp32 -> bf16 bits"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) >> 16
    return u.astype(np.uint16)


def from_bits(b):
    return (b.astype(np.uint32) << 16).view(np.float32)


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("UNISPEECH_REF",
                                                               os.path.join(os.path.dirname(ROOT), "reference"))
    sys.path.insert(0, os.path.join(ref, "src", "examples", "hubert", "simple_kmeans"))
    import joblib
    from dump_km_label import ApplyKmeans
    from sklearn.cluster import MiniBatchKMeans

    rng = np.random.default_rng(20261016)
    means = rng.normal(0.0, 6.0, (32, 64))
    lab = rng.integers(0, 32, 4096)
    blobs = bf16_bits(means[lab] + rng.normal(0.0, 1.0, (4096, 64)))
    hard = bf16_bits(rng.standard_t(3, (1024, 128)))
    out = {}
    tmp = tempfile.mkdtemp()
    for name, bits, k, bs in (("blobs", blobs, 32, 256), ("hard", hard, 16, 128)):
        x = from_bits(bits)
        cs, inert = [], []
        for seed in range(5):
            km = MiniBatchKMeans(n_clusters=k, batch_size=bs, compute_labels=False, init_size=None, random_state=seed,
                                 **RECIPE).fit(x)
            cs.append(km.cluster_centers_.astype(np.float32))
            inert.append(-km.score(x))
            if seed == 0:
                p = os.path.join(tmp, name + ".km")
                joblib.dump(km, p)
                out[name + "/ref_labels"] = np.asarray(ApplyKmeans(p)(x), dtype=np.int64)
        out[name + "/x_bf16"] = bits
        out[name + "/k"] = np.int64(k)
        out[name + "/batch_size"] = np.int64(bs)
        out[name + "/centres"] = np.stack(cs)
        out[name + "/inertia"] = np.asarray(inert, dtype=np.float64)
    seed, n, k = 7, 2000, 500
    g = np.random.default_rng(seed)
    x = g.standard_normal((n, 768), dtype=np.float32)
    c = g.standard_normal((k, 768), dtype=np.float32)
    km = MiniBatchKMeans(n_clusters=k)
    km.cluster_centers_ = c
    p = os.path.join(tmp, "ties.km")
    joblib.dump(km, p)
    out["ties/seed"], out["ties/n"], out["ties/k"] = np.int64(seed), np.int64(n), np.int64(k)
    out["ties/ref_labels"] = np.asarray(ApplyKmeans(p)(x), dtype=np.int64)
    path = os.path.join(ROOT, "tests", "golden", "kmeans.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
