"""Generate tests/golden/diarization.npz: the reference's EEND-vector-clustering head (downstreams/speaker_diarization/models/
models.py, models/transformer.py), its host stage (diarization.py) and its standalone WavLM (WavLM/WavLM.py) on the CPU, fp32.

Runs where the reference tree exists:  python tools/gen_diarization_golden.py [REFERENCE_ROOT]
(default REFERENCE_ROOT: $UNISPEECH_REF, else ../reference next to the repository).  The tests read only the .npz.  Needs
scipy and scikit-learn (the reference's own clustering); the package itself needs neither.

Stand-ins, all inert on this path: `torchaudio.transforms` (a Resample that asserts orig_freq == new_freq and returns its
input -- torchaudio's own behaviour for equal rates -- so the reference is built with sr=16000, frame_shift=640; the released
config's sr=8000, frame_shift=320 gives the same frame counts on the same audio), `models.utils.UpstreamExpert` (returns
prepared states or wraps the reference's standalone WavLM with the reference's hook rule), empty modules for h5py, soundfile,
fire, yamlargparse and utils.*.  sklearn's AgglomerativeClustering lost the keyword `affinity` the reference passes: a wrapper
hands it on as `metric`.  numpy >= 1.24 refuses the ragged list the reference turns into an array when the last chunk is
shorter; the module's `np` is wrapped so that such a list becomes the object array older numpy built.

No weights are stored: every state dict is refilled from a seed (tests/test_speaker.py fill_state_dict, sorted-key order)
and the hidden states of the head cases come from make_states(seed, ...) there.  Contents:
  keys, key_shapes              the reference head's state-dict names / shapes (-1 padded)
  head768/*, head1024/*         seed_w, seed_x, shape [B, T', n, D], frames; feat_chk / enc_chk / spk_chk (ramp-weighted time
                                sums of the front end's output, the encoder's output, the per-frame speaker vectors), ys, acti,
                                vecs and the largest magnitudes *_max.  head768_long: 1499 -> 750 frames, B = 2
  head768/*_bf16_ref, e_ref_*   the reference head in bf16 on the CPU on bf16-rounded states
  e2e/wav_i16, e2e_tiny/*, e2e_tiny_preln/*   a 7 s int16 recording, TINY upstream, chunk_size 50: hidden-state checksums,
                                activities, vectors, clslab, clustered output, RTTM
  cluster/<case>/*              constructed inputs for the host stage and the reference's clslab, stitched output, RTTM
"""
import os
import sys
import tempfile
import types
import wave

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from test_speaker import fill_state_dict, make_states, ramp  # noqa: E402
from unispeech_amd.diarization import chunk_recording  # noqa: E402

SEEDS = dict(head768=(301, 401), head1024=(302, 402), head768_long=(301, 403), e2e_tiny=(311, 312), e2e_tiny_preln=(321, 322))
WAVS = ["David_Faustino/xTOk1Jz-F_g_0000015.wav", "Josh_Gad/HXUqYaOwrxA_0000015.wav"]
HEAD = dict(n_speakers=3, all_n_speakers=5, n_units=256, n_heads=8, n_layers=6, dropout_rate=0.1, spk_emb_dim=256, sr=16000,
            frame_shift=640, frame_size=200, context_size=0, subsampling=1, feature_selection="hidden_states",
            interpolate_mode="linear")
E2E_HEAD = dict(HEAD, n_layers=2, spk_emb_dim=64)
E2E_ARGS = dict(num_speakers=3, sil_spk_th=0.05, ahc_dis_th=1.0, clink_dis=1.0e4, session="rec", threshold=0.5, median=5)
FP32_BOUND = 5e-4     # tests/test_diarization_gpu.py: the fp32 head's bound, relative to the tensor's largest magnitude
CLUSTER_TH = 0.8


class _Layer(nn.Module):
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


class Resample(nn.Module):
    def __init__(self, orig_freq, new_freq):
        super().__init__()
        assert orig_freq == new_freq, "the stand-in resampler only passes equal rates through"

    def forward(self, x):
        return x


class _Numpy:
    """the reference module's `np`: numpy, but a ragged list becomes an object array (numpy < 1.24 behaviour)"""

    def __getattr__(self, name):
        return getattr(np, name)

    @staticmethod
    def array(obj, *a, **k):
        try:
            return np.array(obj, *a, **k)
        except ValueError:
            out = np.empty(len(obj), dtype=object)
            for i, o in enumerate(obj):
                out[i] = o
            return out


def install(ref):
    for name in ("torchaudio", "torchaudio.transforms", "h5py", "soundfile", "fire", "yamlargparse", "utils", "utils.utils",
                 "utils.dataset", "utils.kaldi_data"):
        m = types.ModuleType(name)
        m.__path__ = []
        sys.modules.setdefault(name, m)
    sys.modules["torchaudio"].transforms = sys.modules["torchaudio.transforms"]
    sys.modules["torchaudio.transforms"].Resample = Resample
    sys.modules["utils.utils"].parse_config_or_kwargs = None
    sys.modules["utils.dataset"].DiarizationDataset = None
    sys.modules["utils.kaldi_data"].KaldiData = None
    sd = os.path.join(ref, "downstreams", "speaker_diarization")
    sys.path.insert(0, sd)
    import models  # noqa: F401  (the reference's package; its utils module is replaced before models.models imports it)
    u = types.ModuleType("models.utils")
    u.UpstreamExpert = UpstreamExpert
    sys.modules["models.utils"] = u
    from models.models import TransformerDiarization
    import diarization as ref_diar
    from sklearn.cluster import AgglomerativeClustering
    ref_diar.AgglomerativeClustering = lambda affinity=None, **k: AgglomerativeClustering(metric=affinity, **k)
    ref_diar.np = _Numpy()
    return TransformerDiarization, ref_diar


def head_keys(sd):
    return {k: v for k, v in sd.items() if not k.startswith("feature_extract.")}


def run_head(model, states, frames, out, prefix, store=True):
    """states [n, B, T', D] -> reference outputs under out[prefix + ...]; returns (ys, acti, vecs)"""
    model.feature_extract.spec["states"] = list(states.unbind(0))
    B = states.shape[1]
    got = {}
    hook = model.enc.register_forward_hook(lambda m, i, o: got.update(feat=i[0], enc=o))
    wav = torch.zeros(B, frames * model.frame_shift * model.subsampling, dtype=states.dtype)
    with torch.no_grad():
        ys, spks = model(wav)
        est = model.batch_estimate(wav)
    hook.remove()
    acti = torch.stack(list(est[0]))                                         # [B, T, S]
    vecs = torch.stack([torch.stack(list(v)) for v in est[1:]], dim=1)       # [B, S, E]
    r = ramp(frames)
    res = dict(feat_chk=(got["feat"].double().numpy() * r[None, :, None]).sum(1),
               enc_chk=(got["enc"].double().reshape(B, frames, -1).numpy() * r[None, :, None]).sum(1),
               spk_chk=np.stack([(s.double().numpy() * r[None, :, None]).sum(1) for s in spks]),
               ys=ys.float().numpy(), acti=acti.float().numpy(), vecs=vecs.float().numpy(),
               feat_max=float(got["feat"].abs().max()), enc_max=float(got["enc"].abs().max()),
               spk_max=float(max(s.abs().max() for s in spks)))
    if store:
        for k, v in res.items():
            out[prefix + k] = np.asarray(v, dtype=np.float32 if np.ndim(v) else np.float64)
    return res


def read_crop(path, start, n):
    with wave.open(path, "rb") as w:
        assert w.getsampwidth() == 2 and w.getnchannels() == 1 and w.getframerate() == 16000, path
        data = np.frombuffer(w.readframes(w.getnframes()), dtype="<i2")
    assert len(data) >= start + n, (path, len(data))
    return data[start:start + n].copy()


def ref_host_stage(ref_diar, args, acti_list, svec, frame_shift, subsampling, sampling_rate):
    """the reference's cluster() in its own steps (so that clslab can be stored) + make_rttm -> dict"""
    acti = ref_diar.np.array([np.array(a, dtype=np.float64) for a in acti_list])
    cl_lst, sil_lst = ref_diar.get_cl_sil(args, acti, None)
    res = dict(cl_lst=np.array(cl_lst, dtype=np.int64).reshape(-1, 2), sil_lst=np.array(sil_lst, dtype=np.int64))
    n_samples = len(acti_list) * args.num_speakers - len(sil_lst)
    if n_samples >= 2:
        clslab, cls_num = ref_diar.clustering(args, svec, None, args.ahc_dis_th, cl_lst, sil_lst)
        res.update(clslab=np.array(clslab, dtype=np.int64), cls_num=np.int64(cls_num))
        acti, clslab = ref_diar.merge_acti_clslab(args, acti, clslab, cls_num)
        res["clslab_merged"] = np.array(clslab, dtype=np.int64)
        out_chunks = ref_diar.stitching(args, acti, clslab, cls_num)
    else:
        res.update(clslab=np.zeros((0, args.num_speakers), np.int64), cls_num=np.int64(-1))
        res["clslab_merged"] = res["clslab"]
        out_chunks = acti
    data = np.vstack(list(out_chunks))
    res["outdata"] = data.astype(np.float64)
    with tempfile.TemporaryDirectory() as td:
        args.out_rttm_file = os.path.join(td, "out.rttm")
        conf = dict(model=dict(frame_shift=frame_shift, subsampling=subsampling), dataset=dict(sampling_rate=sampling_rate))
        ref_diar.make_rttm(args, conf, data)
        res["rttm"] = np.array(open(args.out_rttm_file).read())
    return res


def check_margins(args, acti_list, svec, res):
    """the condition under which the partition does not hang on rounding (see the cluster cases below)"""
    mean = np.concatenate([np.mean(a, axis=0) for a in acti_list])
    assert np.all(np.abs(mean - args.sil_spk_th) > 0.01), mean
    if res["cls_num"] < 0:
        return
    keep = [i for i in range(len(svec)) if i not in set(res["sil_lst"].tolist())]
    v = np.asarray(svec, np.float64)[keep]
    dist = np.sqrt(((v[:, None] - v[None]) ** 2).sum(-1))
    tbl = {o: n for n, o in enumerate(keep)}
    for a, b in res["cl_lst"]:
        dist[tbl[a], tbl[b]] = dist[tbl[b], tbl[a]] = args.clink_dis
    lab = res["clslab"].reshape(-1)[keep]
    th = args.ahc_dis_th
    for c in np.unique(lab):
        inn = np.where(lab == c)[0]
        for i in inn:
            rest = [j for j in inn if j != i]
            assert not rest or dist[i, rest].mean() < 0.5 * th, ("within", c, dist[i, rest])
        for c2 in np.unique(lab):
            if c2 > c:
                assert dist[np.ix_(inn, np.where(lab == c2)[0])].mean() > 1.5 * th, ("between", c, c2)


def cluster_cases():
    """constructed inputs: name -> (args overrides, acti_list, svec).  3 slots, vectors of 16, chunk of 40 frames"""
    rng = np.random.default_rng(77)
    E, T, n = 16, 40, 3
    base = np.linalg.qr(rng.standard_normal((E, E)))[0][:4]          # four orthonormal "speakers": sqrt(2) apart

    def vec(spk, noise=0.02):
        v = base[spk] + noise * rng.standard_normal(E)
        return v / np.linalg.norm(v)

    def act(levels, frames=T):
        """levels per slot: mean activity; frames alternate around it so that thresholding / median filtering has work"""
        a = np.zeros((frames, n))
        for s, lv in enumerate(levels):
            if lv > 0.2:
                on = rng.integers(3, frames // 2)
                a[:, s] = 0.1 + 0.05 * rng.random(frames)
                a[on:on + max(4, int(frames * lv)), s] = 0.8 + 0.15 * rng.random(len(a[on:on + max(4, int(frames * lv)), s]))
            else:
                a[:, s] = lv * (0.5 + rng.random(frames))
        return a

    cases = {}
    perms = [(0, 1, 2), (2, 0, 1), (1, 2, 0), (0, 2, 1)]
    cases["permuted"] = ({}, [act([0.5, 0.4, 0.6]) for _ in perms], np.stack([vec(s) for p in perms for s in p]))
    sil = [(0, 1, None), (None, 0, 1), (1, None, 0)]
    cases["silent"] = ({}, [act([0.5 if s is not None else 0.01 for s in p]) for p in sil],
                       np.stack([vec(s) if s is not None else vec(3, 0.3) for p in sil for s in p]))
    # chunk 1 carries speaker 0 on two slots (the second 0.25 off the centre): the cannot-link keeps them apart
    v = [vec(s) for s in (0, 1, 2)]
    b = base[0] + 0.25 * base[3]
    v += [vec(0), b / np.linalg.norm(b), vec(1)] + [vec(s) for s in (2, 0, 1)] + [vec(s) for s in (1, 2, 0)]
    cases["cannot_link"] = ({}, [act([0.5, 0.4, 0.6]) for _ in range(4)], np.stack(v))
    cases["single"] = ({}, [act([0.5, 0.01, 0.02]), act([0.01, 0.02, 0.01])], np.stack([vec(s) for s in (0, 1, 2, 0, 1, 2)]))
    # a weak cannot-link (clink_dis 1.0): chunk 2's two slots of speaker 0 end in one cluster and are merged
    v = [vec(s) for s in (0, 1, 2)] + [vec(s) for s in (1, 0, 2)] + [vec(0), vec(0), vec(2)] + [vec(s) for s in (0, 2, 1)] + \
        [vec(s) for s in (2, 1, 0)] + [vec(s) for s in (0, 1, 2)]
    cases["merge"] = (dict(clink_dis=1.0), [act([0.5, 0.4, 0.6]) for _ in range(6)], np.stack(v))
    return cases


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("UNISPEECH_REF", os.path.join(os.path.dirname(ROOT), "reference"))
    Diar, ref_diar = install(ref)
    sys.path.insert(0, os.path.join(ref, "WavLM"))
    import WavLM as ref_wavlm
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    from gen_golden import TINY
    torch.manual_seed(0)
    out = {}

    def build(D, spec, conf=HEAD):
        return Diar(feat_dim=D, feat_type=spec, **conf).eval()

    for name, (B, T, n, D, frames) in (("head768", (3, 499, 13, 768, 250)), ("head1024", (2, 499, 25, 1024, 250)),
                                       ("head768_long", (2, 1499, 13, 768, 750))):
        sw, sx = SEEDS[name]
        states = make_states(sx, B, T, n, D)
        m = build(D, dict(states=list(states.unbind(0))))
        hk = head_keys(m.state_dict())
        m.load_state_dict(fill_state_dict(hk, sw), strict=False)
        if name == "head768":
            keys = sorted(hk)
            out["keys"] = np.array(keys)
            out["key_shapes"] = np.array([list(hk[k].shape) + [-1] * (4 - hk[k].dim()) for k in keys], dtype=np.int64)
            print("head: %d entries, %.2f M parameters" % (len(keys), sum(v.numel() for v in hk.values()) / 1e6))
        res = run_head(m, states, frames, out, name + "/")
        out[name + "/seed_w"], out[name + "/seed_x"] = np.int64(sw), np.int64(sx)
        out[name + "/shape"] = np.array([B, T, n, D], dtype=np.int64)
        out[name + "/frames"] = np.int64(frames)
        print(name, "activities %.3f .. %.3f, |ys| max %.2f" % (res["acti"].min(), res["acti"].max(), np.abs(res["ys"]).max()))
        if name == "head768":
            mb = build(D, dict(states=list(states.unbind(0))))
            mb.load_state_dict(fill_state_dict(hk, sw), strict=False)
            rb = run_head(mb.bfloat16(), states.bfloat16(), frames, out, "", store=False)
            for k in ("ys", "acti", "vecs"):
                out[name + "/" + k + "_bf16_ref"] = rb[k]
                e = np.abs(rb[k] - res[k]).max() / np.abs(res[k]).max()
                out[name + "/e_ref_" + k] = np.float64(e)
                print("bf16 reference head on the CPU: e_ref_%s %.3e" % (k, e))

    # ---- end to end: one recording, the last chunk shifted back; the chunks go through the reference one at a time, as its prediction() does
    wav = np.concatenate([read_crop(os.path.join(ref, "downstreams", "speaker_verification", "vox1_data", p), 16000, 56000)
                          for p in WAVS])
    out["e2e/wav_i16"] = wav
    chunk_size = 50
    for name, extra in (("e2e_tiny", {}),
                        ("e2e_tiny_preln", dict(layer_norm_first=True, extractor_mode="layer_norm", normalize=True))):
        s_up, s_head = SEEDS[name]
        cfgd = dict(TINY)
        cfgd.update(extra)
        up = ref_wavlm.WavLM(ref_wavlm.WavLMConfig(cfgd)).eval()
        up.load_state_dict(fill_state_dict(up.state_dict(), s_up))
        m = build(64, dict(wavlm=up, normalize=bool(cfgd.get("normalize", False))), E2E_HEAD)
        m.load_state_dict(fill_state_dict(head_keys(m.state_dict()), s_head), strict=False)
        audio = wav.astype(np.float32) / 32768.0
        # the package's own chunking (tests/test_diarization.py checks it against hand-computed spans); the reference's lives
        # inside its main() next to the file reading and cannot be called on its own
        spans, chunk_len_list = chunk_recording(len(audio), chunk_size, E2E_HEAD["frame_shift"], E2E_HEAD["subsampling"])
        wav_list = [torch.from_numpy(audio[s:e]).float() for s, e in spans]
        starts = [s for s, _ in spans]
        assert chunk_len_list == [50, 50, 50, 25] and starts[-1] == 80000, (chunk_len_list, starts)
        acti_full, vecs, hs_chk = [], [], []
        with torch.no_grad():
            for w in wav_list:
                hs = m.feature_extract([w])["hidden_states"]
                hs_chk.append(np.stack([(h.double().numpy()[0] * ramp(h.shape[1])[:, None]).sum(0) for h in hs]))
                o = m.batch_estimate(w.unsqueeze(0))
                acti_full.append(o[0][0].numpy())
                vecs += [o[i + 1][0].numpy() for i in range(3)]
        assert hs[0].shape == (1, 99, 64), hs[0].shape
        acti_full, vecs = np.stack(acti_full), np.stack(vecs)
        acti_list = [a[-n:] for a, n in zip(acti_full, chunk_len_list)]
        args = types.SimpleNamespace(**E2E_ARGS)
        res = ref_host_stage(ref_diar, args, acti_list, vecs, E2E_HEAD["frame_shift"], 1, 16000)
        near = np.abs(res["outdata"] - args.threshold) <= FP32_BOUND
        assert near.mean() <= 0.01, "reference activities within the fp32 bound of the threshold: %.4f" % near.mean()
        out[name + "/hs_chk"] = np.stack(hs_chk).astype(np.float32)          # [chunks, states, D]
        out[name + "/acti_full"], out[name + "/vecs"] = acti_full, vecs
        out[name + "/chunk_len"] = np.array(chunk_len_list, dtype=np.int64)
        for k in ("clslab", "cls_num", "outdata", "rttm"):
            out[name + "/" + k] = res[k]
        out[name + "/seed_up"], out[name + "/seed_head"] = np.int64(s_up), np.int64(s_head)
        out[name + "/cfg_keys"] = np.array(sorted(extra))
        out[name + "/cfg_vals"] = np.array([str(extra[k]) for k in sorted(extra)])
        print(name, "clslab", res["clslab"].tolist(), "rttm lines", len(str(res["rttm"]).splitlines()))
    out["e2e/args_keys"] = np.array(sorted(E2E_ARGS))
    out["e2e/args_vals"] = np.array([str(E2E_ARGS[k]) for k in sorted(E2E_ARGS)])
    out["e2e/head_keys"] = np.array(sorted(E2E_HEAD))
    out["e2e/head_vals"] = np.array([str(E2E_HEAD[k]) for k in sorted(E2E_HEAD)])
    out["e2e/chunk_size"] = np.int64(chunk_size)

    # ---- the host stage on constructed inputs
    names = []
    for cname, (over, acti_list, svec) in cluster_cases().items():
        a = dict(E2E_ARGS, ahc_dis_th=CLUSTER_TH, threshold=0.4, median=5, session="c")
        a.update(over)
        args = types.SimpleNamespace(**a)
        res = ref_host_stage(ref_diar, args, [x.copy() for x in acti_list], svec.copy(), 640, 1, 16000)
        check_margins(args, acti_list, svec, res)
        p = "cluster/%s/" % cname
        out[p + "acti"], out[p + "svec"] = np.stack(acti_list), svec
        out[p + "clink_dis"], out[p + "ahc_dis_th"] = np.float64(args.clink_dis), np.float64(args.ahc_dis_th)
        for k, v in res.items():
            out[p + k] = v
        names.append(cname)
        print(cname, "clslab", res["clslab"].tolist(), "-> merged", res["clslab_merged"].tolist(), "out", res["outdata"].shape,
              "rttm lines", len(str(res["rttm"]).splitlines()))
    out["cluster/names"] = np.array(names)
    assert (out["cluster/merge/clslab"] != out["cluster/merge/clslab_merged"]).any(), "the merge case must merge"
    assert out["cluster/single/cls_num"] < 0 and len(out["cluster/silent/sil_lst"]) == 3
    path = os.path.join(ROOT, "tests", "golden", "diarization.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
