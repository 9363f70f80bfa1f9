"""Diarization head, host side (unispeech_amd/diarization.py): the fixture tests/golden/diarization.npz
(tools/gen_diarization_golden.py), state-dict compatibility with the reference's TransformerDiarization, chunking, the
silence / cannot-link lists, constrained clustering, merge, stitching, median filter and RTTM against the reference's recorded
results, frame arithmetic, the interpolation taps and the refusals.  No GPU.

Cluster labels are arbitrary numbers: they are compared as partitions (`canon`: numbered by first appearance, the silent
label kept last); merge / stitching / RTTM are then checked exactly, once on the reference's own labels and once through the
whole pipeline with the output columns brought into the reference's label order."""
import os
import types

import numpy as np
import pytest
import torch

from conftest import load_golden
from test_speaker import fill_state_dict

HEAD = dict(n_speakers=3, all_n_speakers=5, n_units=256, n_heads=8, n_layers=6, dropout_rate=0.1, spk_emb_dim=256, sr=16000,
            frame_shift=640, frame_size=200, context_size=0, subsampling=1, feature_selection="hidden_states",
            interpolate_mode="linear")


def z():
    return load_golden("diarization.npz")


def head(feat_dim, num_states, **kw):
    from unispeech_amd.diarization import TransformerDiarization
    conf = dict(HEAD)
    conf.update(kw)
    return TransformerDiarization(feat_dim=feat_dim, num_states=num_states, **conf)


def stored_dict(g, prefix):
    def conv(v):
        for t in (int, float):
            try:
                return t(v)
            except ValueError:
                pass
        return {"True": True, "False": False}.get(v, v)
    return {str(k): conv(str(v)) for k, v in zip(g[prefix + "_keys"], g[prefix + "_vals"])}


def case_args(g, p):
    from unispeech_amd.diarization import infer_args
    if p.startswith("cluster/"):
        return infer_args(num_speakers=3, ahc_dis_th=float(g[p + "ahc_dis_th"]), clink_dis=float(g[p + "clink_dis"]),
                          threshold=0.4, median=5, session="c")
    return infer_args(**stored_dict(g, "e2e/args"))


def canon(clslab, sil_lab):
    """labels renumbered by first appearance (row-major), the silent label kept as it is; also the map old -> new"""
    m, out = {}, np.array(clslab).copy()
    for i, v in enumerate(np.array(clslab).reshape(-1)):
        if v != sil_lab and v not in m:
            m[int(v)] = len(m)
        out.reshape(-1)[i] = sil_lab if v == sil_lab else m[int(v)]
    return out, m


def host_cases(g):
    out = [("cluster/%s/" % n, list(g["cluster/%s/acti" % n]), g["cluster/%s/svec" % n]) for n in g["cluster/names"]]
    for n in ("e2e_tiny", "e2e_tiny_preln"):
        acti = [a[-int(k):] for a, k in zip(g[n + "/acti_full"], g[n + "/chunk_len"])]
        out.append((n + "/", acti, g[n + "/vecs"]))
    return out


# ------------------------------------------------------------------------------------------------------------- fixture
def test_fixture_integrity():
    g = z()
    keys = [str(k) for k in g["keys"]]
    assert "feature_weight" in keys and "enc.self_att_5.linearQ.weight" in keys and "linear2.bias" in keys and "embed.weight" in keys
    assert not any(k.startswith("feature_extract.") for k in keys)
    for name, B, T, n, D, fr in (("head768", 3, 499, 13, 768, 250), ("head1024", 2, 499, 25, 1024, 250),
                                 ("head768_long", 2, 1499, 13, 768, 750)):
        assert [int(v) for v in g[name + "/shape"]] == [B, T, n, D] and int(g[name + "/frames"]) == fr
        assert g[name + "/ys"].shape == (B, fr, 3) and g[name + "/acti"].shape == (B, fr, 3)
        assert g[name + "/vecs"].shape == (B, 3, 256) and g[name + "/spk_chk"].shape == (3, B, 256)
        assert g[name + "/feat_chk"].shape == (B, D) and g[name + "/enc_chk"].shape == (B, 256)
        assert np.allclose(np.linalg.norm(g[name + "/vecs"], axis=-1), 1.0, atol=1e-5)
        assert np.allclose(1.0 / (1.0 + np.exp(-g[name + "/ys"].astype(np.float64))), g[name + "/acti"], atol=1e-6)
    for k in ("ys", "acti", "vecs"):
        e = np.abs(g["head768/%s_bf16_ref" % k] - g["head768/" + k]).max() / np.abs(g["head768/" + k]).max()
        assert np.isclose(e, float(g["head768/e_ref_" + k]), rtol=1e-5) and 0 < e < 0.1
    assert g["e2e/wav_i16"].dtype == np.int16 and g["e2e/wav_i16"].shape == (112000,)
    for n in ("e2e_tiny", "e2e_tiny_preln"):
        assert g[n + "/acti_full"].shape == (4, 50, 3) and g[n + "/vecs"].shape == (12, 64)
        assert g[n + "/hs_chk"].shape == (4, 3, 64) and [int(v) for v in g[n + "/chunk_len"]] == [50, 50, 50, 25]
        assert g[n + "/outdata"].shape[0] == 175 and len(str(g[n + "/rttm"]).splitlines()) > 3
        # the cap the GPU test relies on: at most 1 % of the reference's frames lie within the fp32 bound of the threshold
        assert (np.abs(g[n + "/outdata"] - 0.5) <= 5e-4).mean() <= 0.01
    assert sorted(str(n) for n in g["cluster/names"]) == ["cannot_link", "merge", "permuted", "silent", "single"]
    assert os.path.getsize(os.path.join(os.path.dirname(__file__), "golden", "diarization.npz")) < 1 << 20


# ---------------------------------------------------------------------------------------------------------- state dict
def test_state_dict_names_and_shapes_equal_the_reference():
    g = z()
    sd = head(768, 13).state_dict()
    assert sorted(sd) == sorted(str(k) for k in g["keys"])
    for k, s in zip(g["keys"], g["key_shapes"]):
        assert tuple(sd[str(k)].shape) == tuple(int(v) for v in s if v >= 0), k


def test_load_of_a_released_layout():
    from unispeech_amd.diarization import TransformerDiarization, fix_state_dict
    from unispeech_amd.wavlm import WavLM, WavLMConfig
    from conftest import TINY
    m = head(768, 13)
    filled = fill_state_dict(m.state_dict(), 5)
    m.load_state_dict(filled, strict=True)
    assert torch.equal(m.enc.self_att_3.linearK.weight, filled["enc.self_att_3.linearK.weight"])
    up = WavLM(WavLMConfig(dict(TINY)))
    full = TransformerDiarization(feat_dim=64, upstream=up, **dict(HEAD, n_layers=2))
    assert full.feat_num == 3 and all(not p.requires_grad for p in full.feature_extract.parameters())
    assert {"feature_extract.model." + k for k in up.state_dict()} <= set(full.state_dict())
    comb = fill_state_dict(full.state_dict(), 6)
    wrapped = {"module.net." + k: v for k, v in comb.items()}
    wrapped["module.net.feature_extract.model.final_proj.weight"] = torch.zeros(3, 3)
    wrapped.pop("module.net.linear1.bias")
    r = full.load_state_dict(fix_state_dict(wrapped), strict=False)
    assert r.missing_keys == ["linear1.bias"] and r.unexpected_keys == ["feature_extract.model.final_proj.weight"]
    assert torch.equal(full.enc.ff_1.linear2.weight, comb["enc.ff_1.linear2.weight"])
    assert fix_state_dict({"net.a": 1, "module.b": 2, "c": 3}) == {"a": 1, "b": 2, "c": 3}


# ------------------------------------------------------------------------------------------------------ frame arithmetic
def test_frame_counts_and_chunking():
    from unispeech_amd.diarization import chunk_recording, frame_count
    m = head(768, 13)
    assert m.n_frames(160000) == 250 and m.n_frames(480000) == 750 and m.n_frames(32000) == 50
    m8 = head(768, 13, sr=8000, frame_shift=320)                    # the released config counts 8 kHz samples: same frames
    assert m8.n_frames(480000) == 750 and m8.n_frames(160000) == 250
    assert head(768, 13, subsampling=2).n_frames(160000) == 125
    assert frame_count(480000) == 1499 and frame_count(160000) == 499
    spans, lens = chunk_recording(112000, 50, 640, 1)
    assert spans == [(0, 32000), (32000, 64000), (64000, 96000), (80000, 112000)] and lens == [50, 50, 50, 25]
    assert len({e - s for s, e in spans}) == 1                      # one length: one batch
    spans, lens = chunk_recording(64000, 50, 640, 1)
    assert spans == [(0, 32000), (32000, 64000)] and lens == [50, 50]
    spans, lens = chunk_recording(20000, 50, 640, 1)                # shorter than a chunk: start clamps at 0
    assert spans == [(0, 20000)] and lens == [31]
    spans, lens = chunk_recording(100000, 25, 640, 2)
    assert spans[-1] == (68000, 100000) and lens == [25, 25, 25, 3]



def test_released_config_rate_chunks_in_8_khz_samples_and_predict_takes_the_new_frames():
    """the released config: sr 8000, frame_shift 320, chunk_size 750 -- chunking is defined on 8 kHz samples, the waveform is 16 kHz"""
    from unispeech_amd.diarization import predict, recording_chunks
    calls = []

    def batch_estimate(chunks):
        calls.append([len(c) for c in chunks])
        B, T = len(chunks), 750
        acts = torch.arange(B * T * 3, dtype=torch.float32).view(B, T, 3)
        return acts, torch.ones(B, 3, 4) * torch.arange(B).view(B, 1, 1)

    stub = types.SimpleNamespace(sr=8000, frame_shift=320, subsampling=1, batch_estimate=batch_estimate)
    n16 = 2 * 480000 + 100000                                   # two whole 30 s chunks and 6.25 s
    spans, lens = recording_chunks(stub, n16, 750)
    assert spans == [(0, 480000), (480000, 960000), (580000, 1060000)] and lens == [750, 750, 156]   # 50000 // 320
    assert recording_chunks(stub, n16 + 1, 750) == (spans, lens)          # an odd 16 kHz sample has no 8 kHz sample
    assert recording_chunks(stub, 480000, 750) == ([(0, 480000)], [750])
    assert recording_chunks(stub, 100000, 750) == ([(0, 100000)], [156])
    stub16 = types.SimpleNamespace(sr=16000, frame_shift=640, subsampling=1)
    assert recording_chunks(stub16, n16, 750) == (spans, lens)            # the same audio, counted at 16 kHz
    with pytest.raises(NotImplementedError, match="sr="):
        recording_chunks(types.SimpleNamespace(sr=11025, frame_shift=320, subsampling=1), n16, 750)
    acti_list, svec, lens2 = predict(stub, torch.zeros(n16), 750)
    assert calls == [[480000, 480000, 480000]] and lens2 == lens
    assert [a.shape for a in acti_list] == [(750, 3), (750, 3), (156, 3)] and svec.shape == (9, 4)
    assert acti_list[2][0, 0] == (2 * 750 + 750 - 156) * 3 and acti_list[1][0, 0] == 750 * 3    # the LAST 156 frames of chunk 2
    assert svec[:, 0].tolist() == [0, 0, 0, 1, 1, 1, 2, 2, 2]
    with pytest.raises(NotImplementedError, match="mono"):
        predict(stub, torch.zeros(2, 100), 750)


def test_interpolation_taps_equal_torch():
    from unispeech_amd.diarization import interp_taps
    g = torch.Generator().manual_seed(3)
    for T_in, T_out in ((499, 250), (1499, 750), (99, 50), (50, 50), (250, 375), (7, 3), (1, 4), (750, 749)):
        x = torch.randn(2, 5, T_in, generator=g)
        i0, i1, f = interp_taps(T_in, T_out)
        assert i0.min() >= 0 and i1.max() <= T_in - 1 and f.min() >= 0 and f.max() < 1
        # The source position (up to T_in) is evaluated in fp32 by torch and by the kernel alike, each within 2 ulp(T_in) of
        # the exact value (one product, one difference), so the two may differ by 4 ulp(T_in) = 4 T_in 2^-23 in position;
        # a position error moves the result by that times the step between the two taps.
        ulp = T_in * 2.0 ** -23
        exact = np.maximum((np.arange(T_out) + 0.5) * T_in / T_out - 0.5, 0)
        assert np.abs(i0 + f.astype(np.float64) - exact).max() <= 2 * ulp, (T_in, T_out)
        eff = i0 + f.astype(np.float64) * (i1 - i0)                       # beyond the last frame both taps are that frame
        ramp64 = torch.arange(T_in, dtype=torch.float64).view(1, 1, -1)   # interpolating a ramp returns the position itself
        pos = torch.nn.functional.interpolate(ramp64, T_out, mode="linear").numpy()[0, 0]
        assert np.abs(eff - pos).max() <= 2 * ulp, (T_in, T_out)
        got = (1 - f) * x.numpy()[..., i0] + f * x.numpy()[..., i1]
        want = torch.nn.functional.interpolate(x, T_out, mode="linear").numpy()
        step = np.abs(x.numpy()[..., i1] - x.numpy()[..., i0]).max()
        assert np.abs(got - want).max() <= 4 * ulp * step + 1e-6, (T_in, T_out, np.abs(got - want).max())
    i0, i1, f = interp_taps(50, 50)
    assert np.array_equal(i0, np.arange(50)) and not f.any()


def test_median_filter_against_hand_computed_rows():
    from unispeech_amd.diarization import medfilt_rows
    a = np.array([[1, 0], [1, 0], [0, 1], [1, 0], [1, 1], [0, 1], [0, 1]])
    # column 0 windows (zeros beyond the ends): 0 1 1 | 1 1 0 | 1 0 1 | 0 1 1 | 1 1 0 | 1 0 0 | 0 0 0
    assert medfilt_rows(a, 3).T.tolist() == [[1, 1, 1, 1, 1, 0, 0], [0, 0, 0, 1, 1, 1, 1]]
    # kernel 5, column 1: 0 0 0 0 1 | 0 0 0 1 0 | 0 0 1 0 1 | 0 1 0 1 1 | 1 0 1 1 1 | 0 1 1 1 0 | 1 1 1 0 0
    assert medfilt_rows(a, 5)[:, 1].tolist() == [0, 0, 0, 1, 1, 1, 1]
    assert medfilt_rows(a, 1).tolist() == a.tolist()
    with pytest.raises(ValueError, match="odd"):
        medfilt_rows(a, 4)


# ------------------------------------------------------------------------------------------------------------ host stage
def test_silence_and_cannot_link_lists():
    from unispeech_amd.diarization import get_cl_sil
    g = z()
    for p, acti, _ in host_cases(g):
        if p + "cl_lst" not in g.files:
            continue
        cl, sil = get_cl_sil(case_args(g, p), acti, None)
        assert [list(c) for c in cl] == g[p + "cl_lst"].tolist() and list(sil) == g[p + "sil_lst"].tolist(), p
    assert g["cluster/silent/sil_lst"].tolist() == [2, 3, 7] and len(g["cluster/single/sil_lst"]) == 5
    # a known cluster count below the slot count silences the weakest slot of every chunk first (diarization.py:29-34)
    a = [np.tile([0.5, 0.2, 0.4], (10, 1)), np.tile([0.1, 0.6, 0.3], (10, 1))]
    cl, sil = get_cl_sil(case_args(g, "cluster/permuted/"), a, 2)
    assert sil == [1, 3] and cl == [(2, 0), (4, 5)]


def test_clustering_gives_the_reference_partition():
    from unispeech_amd.diarization import clustering, get_cl_sil
    g = z()
    n = 0
    for p, acti, svec in host_cases(g):
        if int(g[p + "cls_num"]) < 0:
            continue
        args = case_args(g, p)
        cl, sil = get_cl_sil(args, acti, None)
        clslab, cls_num = clustering(args, svec, None, args.ahc_dis_th, cl, sil)
        assert cls_num == int(g[p + "cls_num"]), p
        assert np.array_equal(canon(clslab, cls_num)[0], canon(g[p + "clslab"], cls_num)[0]), p
        n += 1
    assert n == 6
    assert int(g["cluster/cannot_link/cls_num"]) == 4 and int(g["cluster/permuted/cls_num"]) == 3
    # a given cluster count stops the merging there
    args = case_args(g, "cluster/cannot_link/")
    acti, svec = list(g["cluster/cannot_link/acti"]), g["cluster/cannot_link/svec"]
    cl, sil = get_cl_sil(args, acti, None)
    clslab, cls_num = clustering(args, svec, 5, args.ahc_dis_th, cl, sil)
    assert cls_num == 5 and len(np.unique(clslab)) == 5


def test_average_linkage_small_cases():
    from unispeech_amd.diarization import average_linkage
    d = np.array([[0, 1, 6, 7], [1, 0, 5, 6], [6, 5, 0, 2], [7, 6, 2, 0]], dtype=float)
    assert average_linkage(d, distance_threshold=3.0).tolist() == [0, 0, 1, 1]
    assert average_linkage(d, distance_threshold=0.5).tolist() == [0, 1, 2, 3]
    assert average_linkage(d, distance_threshold=6.01).tolist() == [0, 0, 0, 0]   # (6 + 7 + 5 + 6) / 4 = 6
    assert average_linkage(d, distance_threshold=6.0).tolist() == [0, 0, 1, 1]    # merged only BELOW the threshold
    assert average_linkage(d, n_clusters=3).tolist() == [0, 0, 1, 2]


def test_merge_stitching_and_rttm_on_the_reference_labels():
    from unispeech_amd.diarization import make_rttm, merge_acti_clslab, stitching
    g = z()
    for p, acti, _ in host_cases(g):
        args = case_args(g, p)
        cls_num = int(g[p + "cls_num"])
        if cls_num >= 0:
            acti = [np.array(a, dtype=np.float64) for a in acti]
            clslab = g[p + "clslab"].copy()
            acti, clslab = merge_acti_clslab(args, acti, clslab, cls_num)
            if p + "clslab_merged" in g.files:
                assert np.array_equal(clslab, g[p + "clslab_merged"]), p
            data = np.vstack(stitching(args, acti, clslab, cls_num))
        else:
            data = np.vstack(acti)
        assert data.shape == g[p + "outdata"].shape and np.array_equal(data, g[p + "outdata"]), p
        lines = make_rttm(args, data, 640, 1, 16000)
        assert "".join(l + "\n" for l in lines) == str(g[p + "rttm"]), p
    assert str(g["cluster/permuted/rttm"]).splitlines()[0].startswith("SPEAKER c 1 ")


def test_whole_host_stage_up_to_label_order():
    from unispeech_amd.diarization import cluster, make_rttm
    g = z()
    for p, acti, svec in host_cases(g):
        args = case_args(g, p)
        info = {}
        data = cluster(args, acti, svec, info=info)
        want = g[p + "outdata"]
        assert data.shape == want.shape, p
        cls_num = int(g[p + "cls_num"])
        if cls_num >= 0:
            _, mine = canon(info["clslab"], cls_num)         # my label -> first-appearance rank
            _, ref = canon(g[p + "clslab"], cls_num)
            back = {v: k for k, v in ref.items()}            # rank -> reference label
            # stitching's output column of label l is l, less one beyond the removed silent column; other columns stay
            col = lambda l: l if l < cls_num else l - 1       # noqa: E731
            perm = list(range(want.shape[1]))
            for l_mine, rank in mine.items():
                perm[col(back[rank])] = col(l_mine)
            data = data[:, perm]
        assert np.array_equal(data, want), p
        assert "".join(l + "\n" for l in make_rttm(args, data, 640, 1, 16000)) == str(g[p + "rttm"]), p


# -------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_name_the_option():
    for kw, word in ((dict(feat_type="fbank"), "fbank"), (dict(feat_type="mfcc"), "mfcc"),
                     (dict(update_extract=True), "update_extract"), (dict(context_size=2), "context_size"),
                     (dict(interpolate_mode="nearest"), "interpolate_mode"), (dict(feature_selection="default"), "feature_selection"),
                     (dict(n_heads=4), "n_heads")):
        with pytest.raises(NotImplementedError, match=word):
            head(768, 13, **kw)
    m = head(64, 3, n_layers=1)
    st = [torch.zeros(1, 9, 64)] * 3
    with pytest.raises(NotImplementedError, match="training mode"):
        m.train().forward_states(st, 5)
    with pytest.raises(NotImplementedError, match="gradients"):
        m.eval().forward_states(st, 5)
    for fn in (m.get_loss, m.batch_estimate_with_perm, m.spk_loss_parallel):
        with pytest.raises(NotImplementedError, match="PIT loss"):
            fn(None)
    with torch.no_grad():
        with pytest.raises(ValueError, match="upstream"):
            m.hidden_states([torch.zeros(400)])
        with pytest.raises(ValueError, match="3 states|states given"):
            m.forward_states(st[:2], 5)


def test_long_chunk_on_an_unfused_upstream_is_refused_clearly():
    from unispeech_amd.diarization import TransformerDiarization
    from unispeech_amd.wavlm import WavLM, WavLMConfig
    from conftest import TINY
    full = TransformerDiarization(feat_dim=64, upstream=WavLM(WavLMConfig(dict(TINY))), **dict(HEAD, n_layers=1)).eval()
    with torch.no_grad():
        with pytest.raises(ValueError, match=r"1499 upstream frames.*float32.*1024"):
            full.hidden_states(torch.zeros(2, 480000))
        with pytest.raises(ValueError, match="one length"):
            full.hidden_states([torch.zeros(32000), torch.zeros(16000)])


def test_cli_arguments_config_and_wav_reader(tmp_path):
    import json
    from unispeech_amd import diarization
    from test_speaker import write_wav
    a = diarization.parse_args(["up.pt", "head.pt", "conf.yaml", "a.wav", "--threshold", "0.5", "--bf16"])
    assert (a.upstream, a.head, a.config, a.wav, a.threshold, a.median, a.ahc_dis_th, a.bf16) == \
        ("up.pt", "head.pt", "conf.yaml", "a.wav", 0.5, 25, 1.0, True)
    conf = dict(model=dict(HEAD, sr=8000, frame_shift=320), dataset=dict(chunk_size=750, num_speakers=3, sampling_rate=8000))
    (tmp_path / "c.json").write_text(json.dumps(conf))
    assert diarization.load_config(str(tmp_path / "c.json")) == conf
    s = (np.arange(-400, 400) * 40).astype(np.int16)
    write_wav(tmp_path / "a.wav", s)
    assert torch.equal(diarization.read_wav(str(tmp_path / "a.wav"), 8000), torch.from_numpy(s.astype(np.float32) / 32768.0))
    write_wav(tmp_path / "b.wav", s, sr=8000)
    with pytest.raises(NotImplementedError, match="Resample"):
        diarization.read_wav(str(tmp_path / "b.wav"), 8000)
