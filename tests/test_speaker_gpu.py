"""Speaker head on the MI355X (csrc/spkhead.hip through unispeech_amd/speaker.py): every kernel alone against an fp64 numpy
restatement written here, the head against the reference's outputs in tests/golden/speaker.npz (tools/gen_speaker_golden.py)
in fp32 and bf16 mode, frame counts, the path from int16 samples to the cosine matrix, and reproducibility.

Tolerances.  fp32 kernels: 5e-5 of the result's max magnitude (sums of <= 1536 fp32 terms).  bf16 storage adds one rounding
of the output, 2^-8 of the max magnitude.  Head in fp32 mode: 5e-4 of each tensor's max magnitude (the figure
test_base_width_vs_oracle uses for fp32 mode), cosines 1e-3.  Head in bf16 mode: 2 * e_ref and twice the cosine error of the
reference head run in bf16 on the CPU, both stored in the fixture (e_ref = 1.35e-2, cosine error 1.2e-3)."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import TINY
from test_speaker import cos_matrix, fill_state_dict, make_states, ramp, write_wav, z

pytestmark = pytest.mark.gpu

F32_TOL, BF16_TOL = 5e-5, 2.0 ** -8
GARBAGE = 3.0e4   # finite and large: an absent frame that leaks is seen at once


def L():
    from unispeech_amd import _lib
    return _lib, _lib.lib()


def stream():
    from unispeech_amd import ops
    return ops.stream()


def P(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def DT(t):
    return 1 if t.dtype == torch.bfloat16 else 0


def f64(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


def close(got, want, dtype, what=""):
    want = np.asarray(want, np.float64)
    tol = (F32_TOL + (BF16_TOL if dtype == torch.bfloat16 else 0.0)) * max(np.abs(want).max(), 1e-3)
    err = np.abs(f64(got) - want).max()
    assert np.isfinite(f64(got)).all() and err <= tol, (what, err, tol)


def strided(x, off):
    """the same values inside a larger tensor: row stride and batch stride larger than the shape, base pointer `off` elements in"""
    B, T, Cc = x.shape
    big = torch.full((B, T + 3, Cc + 2 * off + 2), GARBAGE, dtype=x.dtype, device=x.device)
    v = big[:, 1:T + 1, off:off + Cc]
    v.copy_(x)
    return v


def tail(x, lengths, fill):
    """frames beyond each utterance's length overwritten with `fill`"""
    x = x.clone()
    for b, n in enumerate(lengths):
        x[b, n:] = fill
    return x


def lens_for(B, T, mode):
    if mode == "none":
        return None
    return [max(1, T - (b * 7 + 3) % T) if b else T for b in range(B)]


# ------------------------------------------------------------------------------------------------------ mix + instance norm
def mix_ref(states, w, lengths, eps=1e-5):
    x = sum(wi * s for wi, s in zip(w, states)) + 1e-6       # [B, T, D] fp64
    out = np.zeros_like(x)
    for b in range(x.shape[0]):
        n = x.shape[1] if lengths is None else lengths[b]
        v = x[b, :n]
        out[b, :n] = (v - v.mean(0)) / np.sqrt(v.var(0) + eps)
    return out


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("T,D,n,off,mode", [(1, 64, 3, 0, "none"), (5, 768, 13, 2, "zero"), (61, 1024, 25, 0, "garbage"),
                                            (749, 64, 13, 3, "garbage"), (999, 768, 3, 0, "none"), (1100, 64, 3, 0, "garbage"),
                                            (333, 70, 13, 2, "zero"), (77, 65, 3, 1, "garbage")])
def test_mix_norm_kernel(dtype, T, D, n, off, mode):
    _lib, lib = L()
    B, pad = 3, 2
    g = torch.Generator().manual_seed(T * 31 + D + n)
    lengths = lens_for(B, T, mode)
    states = []
    for l in range(n):
        s = (torch.randn(B, T, D, generator=g) * (1 + l % 3) + 0.3 * l).to(dtype).cuda()
        if lengths is not None:
            s = tail(s, lengths, 0.0 if mode == "zero" else GARBAGE)
        states.append(strided(s, off) if off else s)
    w = torch.softmax(torch.randn(n, generator=g), 0).cuda()
    out = torch.full((B, T + 2 * pad, D), GARBAGE, dtype=dtype, device="cuda")
    lt = torch.tensor(lengths, dtype=torch.int32, device="cuda") if lengths is not None else None
    ptrs = (C.c_void_p * n)(*[s.data_ptr() for s in states])
    sb = (C.c_int64 * n)(*[s.stride(0) for s in states])
    st = (C.c_int64 * n)(*[s.stride(1) for s in states])
    _lib.check(lib.wavlm_spk_mix_norm(ptrs, sb, st, n, DT(out), P(w), P(lt), B, T, D,
                                      C.c_void_p(out.data_ptr() + pad * D * out.element_size()), DT(out), (T + 2 * pad) * D, D, pad,
                                      1e-6, 1e-5, stream()), "mix_norm")
    want = mix_ref([f64(s) for s in states], f64(w), lengths)
    close(out[:, pad:T + pad], want, dtype, "normed")
    assert (out[:, :pad] == 0).all() and (out[:, T + pad:] == 0).all()      # the convolution's padding frames
    if lengths is not None:
        for b, nb in enumerate(lengths):
            assert (out[b, pad + nb:] == 0).all()


# ---------------------------------------------------------------------------------------------------------- row activation
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("T,Cc,act,mode,want_mean", [(1, 64, 0, "none", True), (5, 512, 0, "garbage", True),
                                                     (61, 128, 1, "zero", False), (749, 1536, 0, "none", False),
                                                     (313, 512, 0, "garbage", True), (999, 70, 1, "garbage", False)])
def test_rowact_kernel(dtype, T, Cc, act, mode, want_mean):
    _lib, lib = L()
    B = 3
    g = torch.Generator().manual_seed(T + Cc)
    lengths = lens_for(B, T, mode)
    x = torch.randn(B, T, Cc, generator=g).to(dtype).cuda()
    if lengths is not None:
        x = tail(x, lengths, 0.0 if mode == "zero" else GARBAGE)
    xs = strided(x, 2)
    scale = (1 + 0.1 * torch.randn(Cc, generator=g)).cuda() if act == 0 else None
    shift = (0.1 * torch.randn(Cc, generator=g)).cuda() if act == 0 else None
    y = torch.full((B, T, Cc), GARBAGE, dtype=dtype, device="cuda")
    mean = torch.full((B, Cc), GARBAGE, device="cuda") if want_mean else None
    lt = torch.tensor(lengths, dtype=torch.int32, device="cuda") if lengths is not None else None
    _lib.check(lib.wavlm_spk_rowact(P(xs), DT(x), xs.stride(0), xs.stride(1), P(y), DT(y), T * Cc, Cc, B, T, Cc, act, P(scale),
                                    P(shift), P(lt), P(mean), stream()), "rowact")
    xf = f64(x)
    v = np.maximum(xf, 0) if act == 0 else np.tanh(xf)
    if act == 0:
        v = v * f64(scale) + f64(shift)
    want = np.zeros_like(v)
    wm = np.zeros((B, Cc))
    for b in range(B):
        nb = T if lengths is None else lengths[b]
        want[b, :nb] = v[b, :nb]
        wm[b] = v[b, :nb].mean(0)
    close(y, want, dtype, "y")
    if want_mean:
        close(mean, wm, torch.float32, "mean")   # fp32, taken before the store rounds


# ------------------------------------------------------------------------------------------------------------- Res2 chain
def bf16_round(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).bfloat16().double().numpy()


def res2_ref(x, W, bias, scale, shift, dil, lengths, bf16_operands=False):
    """x [B, T, 512] fp64; W [7, out, in, 3].  bf16_operands: what bf16 mode computes -- each convolution's input rounded to
    bf16 as the MFMA operand (the weights are bf16 values already), everything else exact"""
    B, T, _ = x.shape
    y = np.zeros_like(x)
    for b in range(B):
        n = T if lengths is None else lengths[b]
        xv = np.zeros((T, 512))
        xv[:n] = x[b, :n]
        sp = None
        for i in range(7):
            sp = xv[:, 64 * i:64 * i + 64] if i == 0 else sp + xv[:, 64 * i:64 * i + 64]
            pd = np.zeros((T + 2 * dil, 64))
            pd[dil:dil + T] = bf16_round(sp) if bf16_operands else sp
            o = bias[i][None, :] + sum(pd[k * dil:k * dil + T] @ W[i, :, :, k].T for k in range(3))
            sp = np.maximum(o, 0) * scale[i] + shift[i]
            sp[n:] = 0
            y[b, :, 64 * i:64 * i + 64] = sp
        y[b, :, 448:] = xv[:, 448:]
    return y


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("T,dil,mode", [(1, 2, "none"), (5, 4, "garbage"), (61, 3, "zero"), (300, 4, "garbage"),
                                        (749, 2, "none"), (129, 4, "garbage"), (999, 3, "garbage")])
def test_res2_kernel(dtype, T, dil, mode):
    _lib, lib = L()
    B = 2
    g = torch.Generator().manual_seed(T + dil)
    lengths = lens_for(B, T, mode)
    x = torch.randn(B, T, 512, generator=g).to(dtype).cuda()
    if lengths is not None:
        x = tail(x, lengths, 0.0 if mode == "zero" else GARBAGE)
    xs = strided(x, 2)
    W = (torch.randn(7, 64, 64, 3, generator=g) / 192 ** 0.5).to(dtype).float()
    bias, shift = 0.1 * torch.randn(7, 64, generator=g), 0.1 * torch.randn(7, 64, generator=g)
    scale = 1 + 0.1 * torch.randn(7, 64, generator=g)
    img = W.permute(0, 3, 2, 1).contiguous().cuda()
    y = torch.full((B, T + 1, 520), GARBAGE, dtype=dtype, device="cuda")[:, :T, :512]
    lt = torch.tensor(lengths, dtype=torch.int32, device="cuda") if lengths is not None else None
    bc, sc, sh = bias.cuda(), scale.cuda(), shift.cuda()
    _lib.check(lib.wavlm_spk_res2(P(xs), DT(x), xs.stride(0), xs.stride(1), P(y), DT(x), y.stride(0), y.stride(1), B, T, 512,
                                  dil, P(img), P(bc), P(sc), P(sh), P(lt), stream()), "res2")
    want = res2_ref(f64(x), f64(W), f64(bias), f64(scale), f64(shift), dil, lengths, bf16_operands=dtype == torch.bfloat16)
    # bf16 mode: the running tensor stays fp32 on chip and is rounded to bf16 only as the MFMA operand, which the restatement
    # does too; the stored output is rounded once more.  An fp32-sized difference in the running tensor can move one operand
    # across a rounding boundary: one bf16 ulp of one of 192 inputs times a weight of ~0.07, far inside 2^-8 of the maximum
    close(y, want, dtype, "res2")
    assert lib.wavlm_spk_res2(P(xs), DT(x), xs.stride(0), xs.stride(1), P(xs), DT(x), xs.stride(0), xs.stride(1), B, T, 512, dil,
                              P(img), P(bc), P(sc), P(sh), P(lt), stream()) == -1     # in place is refused


# ------------------------------------------------------------------------------------------------ squeeze-excite + residual
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("T,mode", [(1, "none"), (5, "zero"), (61, "garbage"), (749, "zero"), (999, "none"), (333, "garbage")])
def test_se_residual_kernel(dtype, T, mode):
    _lib, lib = L()
    B, Cc, Cb = 3, 512, 128
    g = torch.Generator().manual_seed(T)
    lengths = lens_for(B, T, mode)
    x, res = (torch.randn(B, T, Cc, generator=g).to(dtype).cuda() for _ in range(2))
    if lengths is not None:
        x, res = (tail(t, lengths, 0.0 if mode == "zero" else GARBAGE) for t in (x, res))
    mean = torch.randn(B, Cc, generator=g).cuda()
    w1, w2 = (torch.randn(Cb, Cc, generator=g) / Cc ** 0.5).to(dtype).cuda(), (torch.randn(Cc, Cb, generator=g) / Cb ** 0.5).to(dtype).cuda()
    b1, b2 = (0.1 * torch.randn(Cb, generator=g)).to(dtype).cuda(), (0.1 * torch.randn(Cc, generator=g)).to(dtype).cuda()
    cat = torch.full((B, T, 3 * Cc), GARBAGE, dtype=dtype, device="cuda")
    out, rs = cat[:, :, Cc:2 * Cc], strided(res, 2)
    lt = torch.tensor(lengths, dtype=torch.int32, device="cuda") if lengths is not None else None
    nb = lib.wavlm_spk_se_workspace_bytes(B, Cc)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    _lib.check(lib.wavlm_spk_se_residual(P(x), DT(x), T * Cc, Cc, P(mean), P(w1), P(b1), P(w2), P(b2), DT(x), P(rs), DT(x),
                                         rs.stride(0), rs.stride(1), P(out), DT(x), out.stride(0), out.stride(1), B, T, Cc, Cb,
                                         P(lt), P(ws), nb, stream()), "se_residual")
    hid = np.maximum(f64(mean) @ f64(w1).T + f64(b1), 0)
    gate = 1 / (1 + np.exp(-(hid @ f64(w2).T + f64(b2))))
    v = f64(x) * gate[:, None, :] + f64(res)
    want = np.zeros_like(v)
    for b in range(B):
        n = T if lengths is None else lengths[b]
        want[b, :n] = v[b, :n]
    close(out, want, dtype, "se")
    assert (cat[:, :, :Cc] == GARBAGE).all() and (cat[:, :, 2 * Cc:] == GARBAGE).all()   # the neighbours' slices are untouched


# ------------------------------------------------------------------------------------------- attentive statistics pooling
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("T,Cc,mode", [(1, 64, "none"), (5, 1536, "garbage"), (61, 70, "zero"), (749, 1536, "none"),
                                       (999, 128, "garbage")])
def test_asp_kernel(dtype, T, Cc, mode):
    _lib, lib = L()
    B = 3
    g = torch.Generator().manual_seed(T + Cc)
    lengths = lens_for(B, T, mode)
    x = torch.randn(B, T, Cc, generator=g).abs().to(dtype).cuda()
    lg = (3 * torch.randn(B, T, Cc, generator=g)).to(dtype).cuda()
    if lengths is not None:
        x, lg = (tail(t, lengths, 0.0 if mode == "zero" else GARBAGE) for t in (x, lg))
    scale, shift = (1 + 0.1 * torch.randn(2 * Cc, generator=g)).cuda(), (0.1 * torch.randn(2 * Cc, generator=g)).cuda()
    raw = torch.full((B, 2 * Cc), GARBAGE, device="cuda")
    out = torch.full((B, 2 * Cc), GARBAGE, dtype=dtype, device="cuda")
    lt = torch.tensor(lengths, dtype=torch.int32, device="cuda") if lengths is not None else None
    xs = strided(x, 2)
    _lib.check(lib.wavlm_spk_asp(P(xs), DT(x), xs.stride(0), xs.stride(1), P(lg), DT(x), T * Cc, Cc, B, T, Cc, P(lt), P(scale),
                                 P(shift), P(raw), P(out), DT(out), stream()), "asp")
    want, vmax = np.zeros((B, 2 * Cc)), 1e-3
    for b in range(B):
        n = T if lengths is None else lengths[b]
        l, v = f64(lg)[b, :n], f64(x)[b, :n]
        vmax = max(vmax, (v * v).max())
        a = np.exp(l - l.max(0))
        a /= a.sum(0)
        m = (a * v).sum(0)
        want[b] = np.concatenate([m, np.sqrt(np.maximum((a * v * v).sum(0) - m * m, 1e-9))])
    # the mean directly; the deviation through its square: sum a x^2 - mean^2 cancels (exactly, for one frame), an fp32 error
    # of F32_TOL * max(x^2) in it is all the arithmetic allows, and the square root of a difference that small is ill-conditioned
    # (the reference's own fp32 sum has the same property)
    r = f64(raw)
    close(raw[:, :Cc], want[:, :Cc], torch.float32, "mean")
    verr = np.abs(r[:, Cc:] ** 2 - want[:, Cc:] ** 2).max()
    assert verr <= F32_TOL * vmax, verr
    close(out, r * f64(scale) + f64(shift), dtype, "BatchNorm of the pooled statistics")


# ---------------------------------------------------------------------------------------------------- head vs the reference
def build_head(g, name, D, n, dtype=torch.float32):
    from unispeech_amd.speaker import ECAPA_TDNN_SMALL
    m = ECAPA_TDNN_SMALL(D, num_states=n)
    m.load_state_dict(fill_state_dict(m.state_dict(), int(g[name + "/seed_w"])), strict=True)
    return m.to(dtype).cuda().eval()


def rel(got, want):
    want = np.asarray(want, np.float64)
    return np.abs(f64(got) - want).max() / np.abs(want).max()


@pytest.mark.parametrize("name", ["head768", "head1024"])
def test_head_fp32_vs_reference(name):
    g = z()
    B, T, n, D = (int(v) for v in g[name + "/shape"])
    m = build_head(g, name, D, n)
    states = make_states(int(g[name + "/seed_x"]), B, T, n, D).cuda()
    inter = {}
    with torch.no_grad():
        emb = m.forward_states(states, intermediates=inter)
    chk = (f64(inter["normed"]) * ramp(T)[None, :, None]).sum(1)
    figs = dict(normed_chk=rel(torch.from_numpy(chk), g[name + "/normed_chk"]), out2_mean=rel(inter["out2_mean"], g[name + "/out2_mean"]),
                out4_mean=rel(inter["out4_mean"], g[name + "/out4_mean"]), pooled=rel(inter["pooled"], g[name + "/pooled"]),
                emb=rel(emb, g[name + "/emb"]))
    cerr = np.abs(cos_matrix(f64(emb)) - g[name + "/cos"]).max()
    print(name, figs, "cos", cerr)
    assert all(v <= 5e-4 for v in figs.values()), figs
    assert cerr <= 1e-3, cerr


def test_head_bf16_within_twice_the_reference_bf16_error():
    g = z()
    B, T, n, D = (int(v) for v in g["head768/shape"])
    m = build_head(g, "head768", D, n, torch.bfloat16)
    states = make_states(int(g["head768/seed_x"]), B, T, n, D).bfloat16().cuda()
    with torch.no_grad():
        emb = m.forward_states(states)
    e_ref, c_ref = float(g["head768/e_ref"]), float(g["head768/cos_err_bf16"])
    e = rel(emb, g["head768/emb"])
    cerr = np.abs(cos_matrix(f64(emb)) - g["head768/cos"]).max()
    print("bf16 head: error %.3e (e_ref %.3e), cosine error %.3e (reference bf16 %.3e)" % (e, e_ref, cerr, c_ref))
    assert emb.dtype == torch.bfloat16 and e <= 2 * e_ref, (e, e_ref)
    assert cerr <= 2 * c_ref, (cerr, c_ref)


@pytest.mark.parametrize("fill", [0.0, GARBAGE])
def test_padded_batch_equals_stand_alone_reference(fill):
    g = z()
    frames = [int(v) for v in g["lengths/frames"]]
    m = build_head(g, "lengths", 768, 13)
    states = make_states(int(g["lengths/seed_x"]), 3, 149, 13, 768)
    states = torch.stack([tail(s, frames, fill) for s in states.unbind(0)]).cuda()
    with torch.no_grad():
        emb = m.forward_states(states, lengths=frames)
        alone = m.forward_states(states[:, 2:3, :61].contiguous())
    e = rel(emb, g["lengths/emb"])
    print("lengths: error", e)
    assert e <= 5e-4, e
    assert rel(alone, g["lengths/emb"][2:3]) <= 5e-4


def test_two_runs_are_bit_identical():
    g = z()
    m = build_head(g, "head768", 768, 13, torch.bfloat16)
    states = make_states(int(g["head768/seed_x"]), 4, 149, 13, 768).bfloat16().cuda()
    with torch.no_grad():
        a = m.forward_states(states, lengths=[149, 100, 61, 149]).clone()
        b = m.forward_states(states, lengths=[149, 100, 61, 149])
    assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------------------- end to end
def build_e2e(g, name):
    from unispeech_amd.speaker import ECAPA_TDNN_SMALL
    from unispeech_amd.wavlm import WavLM, WavLMConfig
    cfgd = dict(TINY)
    for k, v in zip(g[name + "/cfg_keys"], g[name + "/cfg_vals"]):
        cfgd[str(k)] = {"True": True, "False": False}.get(str(v), str(v))
    up = WavLM(WavLMConfig(cfgd))
    up.load_state_dict(fill_state_dict(up.state_dict(), int(g[name + "/seed_up"])))
    m = ECAPA_TDNN_SMALL(64, upstream=up)
    head = fill_state_dict({k: v for k, v in m.state_dict().items() if not k.startswith("feature_extract.")},
                           int(g[name + "/seed_head"]))
    assert m.load_state_dict(head, strict=False).unexpected_keys == []
    return m.cuda().eval(), cfgd


@pytest.mark.parametrize("name", ["e2e_tiny", "e2e_tiny_preln"])
def test_end_to_end_from_int16_samples(name):
    g = z()
    m, cfgd = build_e2e(g, name)
    wav = torch.from_numpy(g[name + "/wav_i16"].astype(np.float32) / 32768.0).cuda()
    with torch.no_grad():
        hs, frames = m.hidden_states(wav)
        emb = m(wav)
    assert frames is None and len(hs) == 3 and hs[0].shape == (4, 99, 64)
    for l, h in enumerate(hs):
        chk = (f64(h) * ramp(99)[None, :, None]).sum(1)
        want = g[name + "/hs_chk"][l]
        err = np.abs(chk - want).max()
        print(name, "state", l, "checksum error", err, "checksum max", float(np.abs(want).max()))
        assert err <= 5e-4 * np.abs(want).max(), (l, err)
    e = rel(emb, g[name + "/emb"])
    cerr = np.abs(cos_matrix(f64(emb)) - g[name + "/cos"]).max()
    print(name, "embedding error", e, "cosine error", cerr)
    assert e <= 5e-4 and cerr <= 1e-3, (e, cerr)

    # a second model with forward hooks placed by the reference's rule (models/utils.py:49-56) sees the same states, bit for bit
    m2, _ = build_e2e(g, name)
    up, cap = m2.feature_extract.model, []
    for layer in up.encoder.layers:
        layer.register_forward_hook(lambda mod, i, o: cap.append(i[0].transpose(0, 1)))
    up.encoder.register_forward_hook(lambda mod, i, o: cap.append(o[0]))
    w = wav
    if cfgd.get("normalize", False):
        w = torch.stack([torch.nn.functional.layer_norm(x, x.shape) for x in wav])
    with torch.no_grad():
        up.extract_features(w, padding_mask=torch.zeros(w.shape, dtype=torch.bool, device=w.device), mask=None)
    assert len(cap) == 3
    for a, b in zip(cap, hs):
        assert torch.equal(a.contiguous(), b.contiguous())


def test_unequal_waveforms_equal_one_call_per_file():
    g = z()
    m, _ = build_e2e(g, "e2e_tiny")
    wav = torch.from_numpy(g["e2e_tiny/wav_i16"].astype(np.float32) / 32768.0).cuda()
    wavs = [wav[0], wav[1, :20000], wav[2], wav[3, :9000]]
    with torch.no_grad():
        hs, frames = m.hidden_states(wavs)
        emb = m(wavs)
        one = torch.cat([m([w]) for w in wavs])
    assert frames == [99, 62, 99, 27] and hs[0].shape == (4, 99, 64) and (hs[1][3, 27:] == 0).all()
    assert rel(emb, f64(one)) <= 5e-4   # the head's fp32 tolerance: the GEMMs tile a different M
    assert rel(emb[0:1], g["e2e_tiny/emb"][0:1]) <= 5e-4


def test_cli_verify_prints_the_reference_sentence(tmp_path, capsys):
    from unispeech_amd import speaker
    g = z()
    m, cfgd = build_e2e(g, "e2e_tiny")
    up = m.feature_extract.model
    torch.save({"cfg": cfgd, "model": {k: v.cpu() for k, v in up.state_dict().items()}}, tmp_path / "up.pt")
    torch.save({"model": {k: v.cpu() for k, v in m.state_dict().items()}}, tmp_path / "head.pt")
    for i in (0, 2):
        write_wav(tmp_path / ("%d.wav" % i), g["e2e_tiny/wav_i16"][i])
    speaker.main(["verify", str(tmp_path / "up.pt"), str(tmp_path / "head.pt"), str(tmp_path / "0.wav"), str(tmp_path / "2.wav")])
    out = capsys.readouterr().out.strip()
    want = "The similarity score between two audios is {:.4f} (-1.0, 1.0).".format(float(g["e2e_tiny/cos"][0, 2]))
    assert out.startswith("The similarity score between two audios is ") and out.endswith(" (-1.0, 1.0).")
    assert abs(float(out.split()[-3]) - float(want.split()[-3])) <= 1e-3, (out, want)


def test_base_width_smoke_bf16():
    from unispeech_amd.speaker import ECAPA_TDNN_SMALL
    from unispeech_amd.wavlm import WavLM, WavLMConfig
    torch.manual_seed(0)
    up = WavLM(WavLMConfig(dict(relative_position_embedding=True, gru_rel_pos=True, num_buckets=320, max_distance=800,
                                dropout=0.0, attention_dropout=0.0, encoder_layerdrop=0.0)))
    m = ECAPA_TDNN_SMALL(768, upstream=up)
    head = fill_state_dict({k: v for k, v in m.state_dict().items() if not k.startswith("feature_extract.")}, 7)
    m.load_state_dict(head, strict=False)
    m = m.to(torch.bfloat16).cuda().eval()
    wav = torch.randn(2, 240000, generator=torch.Generator().manual_seed(1)).cuda()
    with torch.no_grad():
        emb = m(wav)
        hs, frames = m.hidden_states(wav)
        again = m.forward_states(hs, frames)
    assert len(hs) == 13 and hs[0].shape == (2, 749, 768) and hs[0].dtype == torch.bfloat16
    assert emb.shape == (2, 256) and emb.dtype == torch.bfloat16 and torch.isfinite(emb.float()).all()
    assert torch.equal(emb, again)
