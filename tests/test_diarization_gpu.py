"""Diarization head on the MI355X (csrc/diar.hip through unispeech_amd/diarization.py): every kernel alone against an fp64
numpy restatement written here, the head against the reference's outputs in tests/golden/diarization.npz
(tools/gen_diarization_golden.py) in fp32 and bf16 mode, the path from int16 samples to the RTTM, batch independence and
reproducibility.

Tolerances.  fp32 kernels: 5e-5 of the result's max magnitude (sums of <= 1536 fp32 terms), as tests/test_speaker_gpu.py.  bf16
storage adds one rounding of the output, 2^-8 of the max magnitude; the bf16 attention also rounds the probabilities to bf16 as
the MFMA operand (2^-9 each, a convex combination of V), so its bound is taken on V's magnitude.  Head in fp32 mode: 5e-4 of
each tensor's max magnitude (the bound tests/test_speaker_gpu.py uses for its fp32 head).  Head in bf16 mode: 2 * e_ref, the
error of the reference head run in bf16 on the CPU, stored in the fixture per output.

Measured on an MI355X (fp32 mode, relative to each tensor's max magnitude; bf16 mode against 2 * e_ref): see DESIGN 4.6."""
import numpy as np
import pytest
import torch

from conftest import TINY
from test_diarization import HEAD, case_args, stored_dict, z
from test_speaker import fill_state_dict, make_states, ramp

pytestmark = pytest.mark.gpu

F32_TOL, BF16_TOL, HEAD_TOL = 5e-5, 2.0 ** -8, 5e-4


def f64(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


def rel(got, want):
    want = np.asarray(want, np.float64)
    got = f64(got) if isinstance(got, torch.Tensor) else np.asarray(got, np.float64)
    assert np.isfinite(got).all()
    return np.abs(got - want).max() / np.abs(want).max()


def kernel_tol(dtype):
    return F32_TOL + (BF16_TOL if dtype == torch.bfloat16 else 0.0)


# ------------------------------------------------------------------------------------------------------- kernels alone
def front_ref(states, w, T_out, sub, add=1e-6, eps=1e-5):
    from unispeech_amd.diarization import interp_taps
    mixed = sum(wl * s for wl, s in zip(w, states)) + add                   # [B, T, D] fp64
    normed = (mixed - mixed.mean(1, keepdims=True)) / np.sqrt(mixed.var(1, keepdims=True) + eps)
    x = normed[:, ::sub]
    i0, i1, f = interp_taps(x.shape[1], T_out)
    f = f.astype(np.float64)[None, :, None]
    return (1 - f) * x[:, i0] + f * x[:, i1]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("T,T_out,D,n,sub,strided", [(499, 250, 768, 13, 1, False), (99, 50, 64, 3, 1, True),
                                                     (1499, 750, 48, 25, 1, False), (1600, 700, 40, 4, 1, True),
                                                     (1700, 425, 32, 3, 2, False), (250, 375, 24, 2, 1, False),
                                                     (50, 50, 16, 1, 1, False)])
def test_front_kernel(dtype, T, T_out, D, n, sub, strided):
    from unispeech_amd import ops
    g = torch.Generator().manual_seed(T + D)
    B = 2
    if strided:   # the states as views of larger tensors: batch and row strides larger than the shape
        big = [torch.full((B, T + 2, D + 24), 3.0e4, dtype=dtype) for _ in range(n)]
        states = [b_[:, 1:T + 1, 8:8 + D] for b_ in big]
        for s in states:
            s.copy_((torch.randn(B, T, D, generator=g) + 0.3).to(dtype))
        states = [b_.cuda()[:, 1:T + 1, 8:8 + D] for b_ in big]
    else:
        states = [(torch.randn(B, T, D, generator=g) * (1 + 0.2 * l) + 0.3).to(dtype).cuda() for l in range(n)]
    w = torch.softmax(torch.randn(n, generator=g), 0)
    out = ops.diar_front(states, w.cuda(), T_out, sub)
    want = front_ref([f64(s) for s in states], w.double().numpy(), T_out, sub)
    assert out.shape == (B, T_out, D) and out.dtype == dtype and out.is_contiguous()
    e = rel(out, want)
    print("front", dtype, T, T_out, D, "error", e)
    assert e <= kernel_tol(dtype), e


def attn_ref(qkv, H):
    B, T, D3 = qkv.shape
    d = D3 // (3 * H)
    q, k, v = (qkv[..., i * H * d:(i + 1) * H * d].reshape(B, T, H, d).transpose(0, 2, 1, 3) for i in range(3))
    s = q @ k.transpose(0, 1, 3, 2) / np.sqrt(d)
    p = np.exp(s - s.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    return (p @ v).transpose(0, 2, 1, 3).reshape(B, T, H * d)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("T", [50, 250, 750, 1100, 1, 33, 129])
def test_attention_kernel_against_the_plain_formula_in_fp64(dtype, T):
    from unispeech_amd import ops
    g = torch.Generator().manual_seed(T)
    B, H = (1, 8) if T > 500 else (3, 8)
    # scores with a spread of a few units (sharp and flat rows both occur), V with an offset
    qkv = torch.randn(B, T, 3 * H * 32, generator=g)
    qkv[..., :H * 32] *= 1.5
    qkv[..., 2 * H * 32:] += 0.5
    qkv = qkv.to(dtype).cuda()
    o = ops.attn_plain_fwd(qkv, H)
    want = attn_ref(f64(qkv), H)
    assert o.shape == (B, T, H * 32) and o.dtype == dtype
    vmax = np.abs(f64(qkv[..., 2 * H * 32:])).max()
    err = np.abs(f64(o) - want).max()
    print("attention", dtype, T, "error", err, "of |V| max", vmax, "=", err / vmax)
    assert np.isfinite(f64(o)).all() and err <= kernel_tol(dtype) * vmax, (err, vmax)


def test_attention_refuses_other_head_widths():
    from unispeech_amd import _lib, ops
    with pytest.raises(_lib.WavlmHipError, match="invalid argument"):
        ops.attn_plain_fwd(torch.zeros(1, 8, 3 * 2 * 64, device="cuda"), 2)


def estimate_ref(zz, S, E):
    y, v = zz[..., :S], zz[..., S:].reshape(zz.shape[0], zz.shape[1], S, E)
    a = 1 / (1 + np.exp(-y))
    u = v / np.linalg.norm(v, axis=-1, keepdims=True)
    sm = (a[..., None] * u).sum(1)
    return a, sm / np.linalg.norm(sm, axis=-1, keepdims=True)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("T,S,E,pad", [(250, 3, 256, 0), (750, 3, 256, 5), (50, 3, 64, 0), (7, 2, 40, 3), (1499, 4, 512, 0)])
def test_estimate_kernel(dtype, T, S, E, pad):
    from unispeech_amd import ops
    g = torch.Generator().manual_seed(T + E)
    B = 2
    big = (torch.randn(B, T, S + S * E + pad, generator=g) * 1.3).to(dtype).cuda()
    zz = big[..., :S + S * E]
    act, vec = ops.diar_estimate(zz, S, E)
    wa, wv = estimate_ref(f64(zz), S, E)
    assert act.shape == (B, T, S) and act.dtype == torch.float32 and vec.shape == (B, S, E) and vec.dtype == dtype
    ea, ev = rel(act, wa), rel(vec, wv)
    print("estimate", dtype, T, S, E, "activities", ea, "vectors", ev)
    assert ea <= F32_TOL and ev <= kernel_tol(dtype), (ea, ev)
    assert np.allclose(np.linalg.norm(f64(vec), axis=-1), 1.0, atol=2 * BF16_TOL if dtype == torch.bfloat16 else 1e-5)


# ------------------------------------------------------------------------------------------------------------ the head
def build_head(g, name, D, n, dtype=torch.float32, **kw):
    from unispeech_amd.diarization import TransformerDiarization
    m = TransformerDiarization(feat_dim=D, num_states=n, **dict(HEAD, **kw))
    assert m.load_state_dict(fill_state_dict(m.state_dict(), int(g[name + "/seed_w"])), strict=True)
    return m.to(dtype).cuda().eval()


def head_figures(g, name, m, states, frames):
    inter = {}
    with torch.no_grad():
        ys, spks = m.forward_states(states, frames, intermediates=inter)
        acti, vecs = m.estimate_states(states, frames)
    B = states.shape[1]
    r = ramp(frames)[None, :, None]
    figs = dict(feat_chk=rel((f64(inter["feat"]) * r).sum(1), g[name + "/feat_chk"]),
                enc_chk=rel((f64(inter["enc"]).reshape(B, frames, -1) * r).sum(1), g[name + "/enc_chk"]),
                spk_chk=rel(np.stack([(f64(s) * r).sum(1) for s in spks]), g[name + "/spk_chk"]),
                ys=rel(ys, g[name + "/ys"]), acti=rel(acti, g[name + "/acti"]), vecs=rel(vecs, g[name + "/vecs"]))
    return figs, ys, acti, vecs


@pytest.mark.parametrize("name", ["head768", "head1024", "head768_long"])
def test_head_fp32_vs_reference(name):
    g = z()
    B, T, n, D = (int(v) for v in g[name + "/shape"])
    frames = int(g[name + "/frames"])
    m = build_head(g, name, D, n)
    states = make_states(int(g[name + "/seed_x"]), B, T, n, D).cuda()
    figs, ys, acti, vecs = head_figures(g, name, m, states, frames)
    print(name, "fp32 head:", {k: "%.3e" % v for k, v in figs.items()})
    assert ys.shape == (B, frames, 3) and acti.shape == (B, frames, 3) and vecs.shape == (B, 3, 256)
    assert all(v <= HEAD_TOL for v in figs.values()), figs


def test_head_bf16_within_twice_the_reference_bf16_error():
    g = z()
    B, T, n, D = (int(v) for v in g["head768/shape"])
    m = build_head(g, "head768", D, n, torch.bfloat16)
    states = make_states(int(g["head768/seed_x"]), B, T, n, D).bfloat16().cuda()
    figs, ys, acti, vecs = head_figures(g, "head768", m, states, 250)
    e_ref = {k: float(g["head768/e_ref_" + k]) for k in ("ys", "acti", "vecs")}
    print("bf16 head:", {k: "%.3e (e_ref %.3e)" % (figs[k], e_ref[k]) for k in e_ref})
    assert vecs.dtype == torch.bfloat16 and acti.dtype == torch.float32
    assert all(figs[k] <= 2 * e_ref[k] for k in e_ref), (figs, e_ref)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_one_batch_equals_one_call_per_chunk_and_runs_repeat_bit_for_bit(dtype):
    g = z()
    m = build_head(g, "head768", 768, 13, dtype)
    states = make_states(int(g["head768/seed_x"]), 3, 499, 13, 768).to(dtype).cuda()
    with torch.no_grad():
        a1, v1 = m.estimate_states(states, 250)
        a1, v1 = a1.clone(), v1.clone()
        a2, v2 = m.estimate_states(states, 250)
        assert torch.equal(a1, a2) and torch.equal(v1, v2)
        for b in range(3):
            ab, vb = m.estimate_states(states[:, b:b + 1].contiguous(), 250)
            assert torch.equal(ab[0], a1[b]) and torch.equal(vb[0], v1[b]), b


def test_frozen_parameters_gives_the_same_bits():
    from unispeech_amd import functional as F
    g = z()
    m = build_head(g, "head768", 768, 13, torch.bfloat16)
    states = make_states(int(g["head768/seed_x"]), 3, 499, 13, 768).bfloat16().cuda()
    with torch.no_grad():
        a1, v1 = m.estimate_states(states, 250)
        with F.frozen_parameters():
            a2, v2 = m.estimate_states(states, 250)
            a3, v3 = m.estimate_states(states, 250)       # the second call inside reads the kept images
        assert torch.equal(a1, a2) and torch.equal(v1, v2) and torch.equal(a1, a3) and torch.equal(v1, v3)
        # a parameter write is seen: the images are rebuilt
        with F.frozen_parameters():
            m.linear.bias.add_(1.0)
            a4, _ = m.estimate_states(states, 250)
        assert not torch.equal(a1, a4)
    F.invalidate_derived()


# ------------------------------------------------------------------------------------------------------------- end to end
def build_e2e(g, name):
    from unispeech_amd.diarization import TransformerDiarization
    from unispeech_amd.wavlm import WavLM, WavLMConfig
    cfgd = dict(TINY)
    for k, v in zip(g[name + "/cfg_keys"], g[name + "/cfg_vals"]):
        cfgd[str(k)] = {"True": True, "False": False}.get(str(v), str(v))
    up = WavLM(WavLMConfig(cfgd))
    up.load_state_dict(fill_state_dict(up.state_dict(), int(g[name + "/seed_up"])))
    conf = stored_dict(g, "e2e/head")
    m = TransformerDiarization(feat_dim=64, upstream=up, **conf)
    head = fill_state_dict({k: v for k, v in m.state_dict().items() if not k.startswith("feature_extract.")},
                           int(g[name + "/seed_head"]))
    assert m.load_state_dict(head, strict=False).unexpected_keys == []
    return m.cuda().eval(), cfgd


@pytest.mark.parametrize("name", ["e2e_tiny", "e2e_tiny_preln"])
def test_end_to_end_from_int16_samples_to_rttm(name):
    from unispeech_amd.diarization import chunk_recording, cluster, diarize, make_rttm, predict
    g = z()
    m, _ = build_e2e(g, name)
    args = case_args(g, name + "/")
    chunk_size = int(g["e2e/chunk_size"])
    wav = torch.from_numpy(g["e2e/wav_i16"].astype(np.float32) / 32768.0).cuda()
    spans, lens = chunk_recording(len(wav), chunk_size, m.frame_shift, m.subsampling)
    assert lens == [int(v) for v in g[name + "/chunk_len"]]
    chunks = torch.stack([wav[s:e] for s, e in spans])
    with torch.no_grad():
        hs = m.hidden_states(chunks)
        acti, vecs = m.batch_estimate(chunks)
    assert len(hs) == 3 and hs[0].shape == (4, 99, 64)
    for l, h in enumerate(hs):
        chk = (f64(h) * ramp(99)[None, :, None]).sum(1)
        want = g[name + "/hs_chk"][:, l]
        err = np.abs(chk - want).max()
        print(name, "state", l, "checksum error", err, "checksum max", float(np.abs(want).max()))
        assert err <= HEAD_TOL * np.abs(want).max(), (l, err)
    ea, ev = rel(acti, g[name + "/acti_full"]), rel(vecs.reshape(12, -1), g[name + "/vecs"])
    print(name, "activities error", ea, "vectors error", ev)
    assert ea <= HEAD_TOL and ev <= HEAD_TOL, (ea, ev)

    acti_list, svec, lens2 = predict(m, wav, chunk_size)
    assert lens2 == lens and [len(a) for a in acti_list] == lens
    info = {}
    raw = cluster(args, acti_list, svec, info=info)
    data, want = raw, g[name + "/outdata"]
    # random-weight heads cluster by slot: the partition is the reference's; bring the columns into its label order
    cls_num = int(g[name + "/cls_num"])
    assert info["cls_num"] == cls_num == 3
    ref_lab, my_lab = g[name + "/clslab"][0], info["clslab"][0]
    assert all(np.array_equal(row, info["clslab"][0]) for row in info["clslab"])
    data = data[:, [int(my_lab[int(np.where(ref_lab == l)[0][0])]) for l in range(cls_num)]]
    assert data.shape == want.shape
    assert np.abs(data - want).max() <= HEAD_TOL * np.abs(want).max()
    # binarised frames, leaving out those whose reference activity lies within the fp32 bound of the threshold (<= 1 %)
    near = np.abs(want - args.threshold) <= HEAD_TOL * np.abs(want).max()
    print(name, "frames left out", int(near.sum()), "of", near.size)
    assert near.mean() <= 0.01
    assert np.array_equal((data > args.threshold)[~near], (want > args.threshold)[~near])
    lines = make_rttm(args, np.where(near, want, data), m.frame_shift, m.subsampling, 16000)
    assert "".join(l + "\n" for l in lines) == str(g[name + "/rttm"])
    # the one-call form gives exactly the lines of the steps above (in its own label order) ...
    mine = diarize(m, wav, chunk_size, args, 16000)
    assert mine == make_rttm(args, raw, m.frame_shift, m.subsampling, 16000)
    # ... which are the reference's segments up to the speaker numbering, once the frames left out above are set to the reference
    strip = lambda ls: sorted(" ".join(l.split()[:5]) for l in ls)   # noqa: E731
    assert strip(lines) == strip(str(g[name + "/rttm"]).splitlines())
    if not near.any():
        assert strip(mine) == strip(lines)


def test_cli_writes_the_rttm(tmp_path, capsys):
    import json
    from unispeech_amd import diarization
    from test_speaker import write_wav
    g = z()
    m, cfgd = build_e2e(g, "e2e_tiny")
    torch.save({"cfg": cfgd, "model": {k: v.cpu() for k, v in m.feature_extract.model.state_dict().items()}}, tmp_path / "up.pt")
    torch.save({"model": {"module." + k: v.cpu() for k, v in m.state_dict().items()}}, tmp_path / "head.pt")
    conf = dict(model=stored_dict(g, "e2e/head"), dataset=dict(chunk_size=50, num_speakers=3, sampling_rate=16000))
    conf["model"].pop("all_n_speakers")                      # read from the checkpoint's embed.weight, as diarization.py:272-273
    conf["model"].update(feat_dim=64, feat_type="config/upstream.th")
    (tmp_path / "c.json").write_text(json.dumps(conf))
    write_wav(tmp_path / "a.wav", g["e2e/wav_i16"])
    diarization.main([str(tmp_path / "up.pt"), str(tmp_path / "head.pt"), str(tmp_path / "c.json"), str(tmp_path / "a.wav"),
                      "--threshold", "0.5", "--median", "5", "--session", "rec", "--out_rttm_file", str(tmp_path / "o.rttm")])
    got = (tmp_path / "o.rttm").read_text().splitlines()
    want = str(g["e2e_tiny/rttm"]).splitlines()
    strip = lambda ls: sorted(" ".join(l.split()[:5]) for l in ls)   # noqa: E731
    assert len(got) == len(want) and strip(got) == strip(want)


def test_base_width_bf16_upstream_takes_a_30_s_chunk():
    from unispeech_amd.diarization import TransformerDiarization
    from unispeech_amd.wavlm import WavLM, WavLMConfig
    g = z()
    torch.manual_seed(0)
    up = WavLM(WavLMConfig(dict(relative_position_embedding=True, gru_rel_pos=True, num_buckets=320, max_distance=800,
                                dropout=0.0, attention_dropout=0.0, encoder_layerdrop=0.0)))
    m = TransformerDiarization(feat_dim=768, upstream=up, **HEAD)
    head = fill_state_dict({k: v for k, v in m.state_dict().items() if not k.startswith("feature_extract.")}, 7)
    m.load_state_dict(head, strict=False)
    m = m.to(torch.bfloat16).cuda().eval()
    wav = torch.randn(2, 480000, generator=torch.Generator().manual_seed(1)).cuda()
    with torch.no_grad():
        hs = m.hidden_states(wav)
        acti, vecs = m.estimate_states(hs, m.n_frames(480000))
    assert len(hs) == 13 and hs[0].shape == (2, 1499, 768) and hs[0].dtype == torch.bfloat16
    assert acti.shape == (2, 750, 3) and vecs.shape == (2, 3, 256)
    assert torch.isfinite(acti).all() and torch.isfinite(vecs.float()).all()
    # the fp32-mode head on the same (bf16-valued) states
    m32 = TransformerDiarization(feat_dim=768, num_states=13, **HEAD)
    m32.load_state_dict({k: v.float() for k, v in m.state_dict().items() if not k.startswith("feature_extract.")}, strict=True)
    m32 = m32.cuda().eval()
    with torch.no_grad():
        a32, v32 = m32.estimate_states([h.float() for h in hs], 750)
    ea, ev = rel(acti, f64(a32)), rel(vecs, f64(v32))
    print("30 s chunk, bf16 head against the fp32-mode head: activities %.3e vectors %.3e (2 e_ref %.3e / %.3e)"
          % (ea, ev, 2 * float(g["head768/e_ref_acti"]), 2 * float(g["head768/e_ref_vecs"])))
    assert ea <= 2 * float(g["head768/e_ref_acti"]) and ev <= 2 * float(g["head768/e_ref_vecs"])
