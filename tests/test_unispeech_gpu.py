"""UniSpeech multitask pre-training on the GPU: the replace-mix kernel (exact), Wav2Vec2Model(transpose=True) and Unispeech +
UnispeechCriterion against the goldens written by tools/gen_unispeech_golden.py from the reference's own code.

Bounds.  The kernel tests have none: the results are bitwise those of wavlm_dropout and a select.  The model tests use RTOL / GTOL of
tests/test_model_gpu.py (1e-4 on loss and activations, 5e-4 on gradients with its `gmax` floor), the project's fp32 bounds -- for the
CTC term as well, which did not need the bound of tests/test_ctc_gpu.py.  bf16 against the fp32 mode of the same path: loss 2e-3
relative, gradient norm 2e-2, the bounds of tests/test_bf16_e2e_gpu.py."""
import numpy as np
import pytest
import torch

from conftest import golden_state_dict, load_golden
from unispeech_cases import UNISPEECH_GOLDENS, build, sample_of, w2v2_fields

pytestmark = pytest.mark.gpu

RTOL, GTOL = 1e-4, 5e-4


def rel_err(a, b):
    a = torch.as_tensor(a).detach().double().cpu()
    b = torch.as_tensor(b).detach().double().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    assert torch.isfinite(a).all()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-12)).item()


def _seed():
    from unispeech_amd import functional as F
    np.random.seed(77)
    torch.manual_seed(31)
    F._SEED_CTR[0] = 0            # the dropout seeds are torch's seed mixed with a per-process call counter


# ---------------------------------------------------------------------------------------------------------- the kernel
def _sel(kind, rows, g):
    if kind == "mixed":
        s = torch.rand(rows, generator=g) < 0.5
        s[0], s[-1] = True, rows == 1                    # both values wherever there is more than one row
        return s.to(torch.uint8)
    return torch.full((rows,), 1 if kind == "ones" else 0, dtype=torch.uint8)


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("rows,D", [(147, 64), (5, 8), (1, 1024), (16400, 1024)])
def test_replace_mix_is_bitwise_dropout_of_the_selected_row(rows, D, dtype):
    """(16400, 1024): 2 099 200 eight-element chunks, past the 8192 x 256 grid, so the stride loop runs twice"""
    from unispeech_amd import ops
    g = torch.Generator().manual_seed(rows + D)
    x = torch.randn(rows, D, generator=g).cuda().to(dtype)
    q = torch.randn(rows, D, generator=g).cuda().to(dtype)
    dy = torch.randn(rows, D, generator=g).cuda().to(dtype)
    zero = torch.zeros_like(dy)
    for p in (0.0, 0.1):
        seed = 0x1234567 + int(p * 10)
        dx_, dq_, dg_ = ops.dropout(x, p, seed), ops.dropout(q, p, seed), ops.dropout(dy, p, seed)
        if p == 0.0:
            assert torch.equal(_bits(dx_), _bits(x))                               # a plain select
        else:
            assert 0.05 < (dx_ == 0).float().mean().item() < 0.15 or rows * D < 1000
        for kind in ("zeros", "ones", "mixed"):
            sel = _sel(kind, rows, g).cuda()
            s = sel.bool().view(-1, 1)
            y = ops.replace_mix(x, q, sel, p, seed)
            assert torch.equal(_bits(y), _bits(torch.where(s, dq_, dx_))), (p, kind)
            gx, gq = ops.replace_mix_bwd(dy, sel, p, seed)
            assert torch.equal(_bits(gx), _bits(torch.where(s, zero, dg_))), (p, kind)
            assert torch.equal(_bits(gq), _bits(torch.where(s, dg_, zero))), (p, kind)


def test_replace_mix_writes_nothing_outside_its_tensors_and_refuses_bad_arguments():
    from unispeech_amd import _lib, ops
    rows, D, G = 147, 64, 4096
    g = torch.Generator().manual_seed(9)
    sel = _sel("mixed", rows, g).cuda()
    for dtype in (torch.float32, torch.bfloat16):
        bufs = [torch.full((G + rows * D + G,), 7.0, dtype=dtype, device="cuda") for _ in range(5)]
        xb, qb, yb, dxb, dqb = bufs
        x, q, y, dx, dq = [b[G:G + rows * D].view(rows, D) for b in bufs]
        x.copy_(torch.randn(rows, D, generator=g))
        q.copy_(torch.randn(rows, D, generator=g))
        y.fill_(float("nan")); dx.fill_(float("nan")); dq.fill_(float("nan"))
        before = [b.clone() for b in (xb, qb)]
        L = _lib.lib()
        args = (rows, D, 0.1, 77, ops.dt(x), ops.stream())
        _lib.check(L.wavlm_replace_mix(ops.ptr(x), ops.ptr(q), ops.ptr(sel), ops.ptr(y), *args), "wavlm_replace_mix")
        _lib.check(L.wavlm_replace_mix_bwd(ops.ptr(y), ops.ptr(sel), ops.ptr(dx), ops.ptr(dq), *args), "wavlm_replace_mix_bwd")
        torch.cuda.synchronize()
        assert torch.equal(xb, before[0]) and torch.equal(qb, before[1])           # the inputs and their surroundings
        for b in (yb, dxb, dqb):
            assert (b[:G] == 7).all() and (b[G + rows * D:] == 7).all() and torch.isfinite(b[G:G + rows * D].float()).all()
        assert torch.equal(y, ops.replace_mix(x.contiguous(), q.contiguous(), sel, 0.1, 77))
    x = torch.zeros(4, 12, device="cuda")
    with pytest.raises(_lib.WavlmHipError, match="wavlm_replace_mix failed: invalid argument"):
        ops.replace_mix(x, x, torch.zeros(4, dtype=torch.uint8, device="cuda"), 0.0, 1)          # D = 12
    x = torch.zeros(4, 16, device="cuda")
    s4 = torch.zeros(4, dtype=torch.uint8, device="cuda")
    with pytest.raises(_lib.WavlmHipError, match="wavlm_replace_mix failed: invalid argument"):
        ops.replace_mix(x, x, s4, 1.0, 1)                                                         # p = 1
    with pytest.raises(_lib.WavlmHipError, match="wavlm_replace_mix_bwd failed: invalid argument"):
        ops.replace_mix_bwd(x, s4, 1.0, 1)
    L = _lib.lib()                                                                                # rows == 0 is fine
    assert L.wavlm_replace_mix(ops.ptr(x), ops.ptr(x), ops.ptr(s4), ops.ptr(x), 0, 16, 0.1, 1, ops.dt(x), ops.stream()) == 0
    assert L.wavlm_replace_mix_bwd(ops.ptr(x), ops.ptr(s4), ops.ptr(x), ops.ptr(x), 0, 16, 0.1, 1, ops.dt(x), ops.stream()) == 0
    assert L.wavlm_replace_mix(None, ops.ptr(x), ops.ptr(s4), ops.ptr(x), 4, 16, 0.1, 1, ops.dt(x), ops.stream()) == -1
    e = torch.zeros(0, 16, device="cuda")
    assert ops.replace_mix(e, e, torch.zeros(0, dtype=torch.uint8, device="cuda"), 0.1, 1).shape == (0, 16)


def test_replace_mix_function_routes_gradients():
    from unispeech_amd import functional as F
    g = torch.Generator().manual_seed(4)
    x = torch.randn(3, 7, 16, generator=g).cuda().requires_grad_(True)
    q = torch.randn(3, 7, 16, generator=g).cuda().requires_grad_(True)
    sel = _sel("mixed", 21, g).cuda()
    y = F.replace_mix(x, q, sel, 0.25, training=False)                              # eval: a plain select whatever p is
    s = sel.bool().view(3, 7, 1)
    assert torch.equal(y, torch.where(s, q, x))
    w = torch.randn(3, 7, 16, generator=g).cuda()
    (y * w).sum().backward()
    assert torch.equal(x.grad, torch.where(s, torch.zeros_like(w), w)) and torch.equal(q.grad, torch.where(s, w, torch.zeros_like(w)))
    torch.manual_seed(5)
    y1 = F.replace_mix(x, q, sel, 0.25, training=True)
    kept = y1 != 0
    assert 0.6 < kept.float().mean().item() < 0.9
    assert torch.allclose(y1[kept], (torch.where(s, q, x) / 0.75)[kept], rtol=1e-6, atol=0)


# -------------------------------------------------------------------------------------- wav2vec 2.0 with transpose=True
def test_wav2vec2_transpose_vs_reference_golden():
    """the assertions of test_model_gpu.test_wav2vec2_model_vs_reference_golden on tiny_w2v2_transpose.npz"""
    from unispeech_amd.wav2vec2 import Wav2Vec2Config, Wav2Vec2Model, Wav2vecCriterion
    z = load_golden("tiny_w2v2_transpose.npz")
    f = w2v2_fields(transpose=True)
    m = Wav2Vec2Model(Wav2Vec2Config(**{k: v for k, v in f.items() if k in Wav2Vec2Config.__dataclass_fields__}))
    m.load_state_dict(golden_state_dict(z), strict=True)
    m = m.cuda().train()
    m.quantizer.gumbel_noise = "host"
    lw = [float(v) for v in z["in/loss_weights"]]
    crit = Wav2vecCriterion(None, infonce=True, loss_weights=lw)
    pm = torch.zeros(3, 16000, dtype=torch.bool)
    sample = {"id": torch.arange(3), "net_input": {"source": torch.from_numpy(z["in/source"]).cuda(), "padding_mask": pm.cuda(),
                                                   "padding_mask_cpu": pm}}
    _seed()
    loss, ss, log = crit(m, sample)
    assert ss == int(z["out/sample_size"])
    assert abs(loss.item() - float(z["out/loss"])) < RTOL * abs(float(z["out/loss"])), (loss.item(), float(z["out/loss"]))
    assert int(log["correct"]) == int(z["log/correct"])
    for k in ("loss_0", "loss_1", "loss_2"):
        assert abs(log[k] - float(z["log/" + k])) < RTOL * abs(float(z["log/" + k])) + 1e-6, k
    loss.backward()
    gmax = max(float(np.abs(z[k]).max()) for k in z.files if k.startswith("grad/"))
    for n, p in m.named_parameters():
        ref = torch.from_numpy(z["grad/" + n])
        g = p.grad.detach().cpu() if p.grad is not None else torch.zeros_like(ref)
        tol = GTOL * max(ref.abs().max().item(), 1e-6 * gmax) + 1e-8
        assert (g - ref).abs().max().item() <= tol, (n, (g - ref).abs().max().item(), tol)
    _seed()
    with torch.no_grad():
        net = m(**sample["net_input"])
        lg = m.get_logits(net).cpu()
    ref = torch.from_numpy(z["out/logits"])
    fin = torch.isfinite(ref)
    assert torch.equal(torch.isfinite(lg), fin) and rel_err(lg[fin], ref[fin]) < RTOL
    assert abs(float(net["prob_perplexity"]) - float(z["out/prob_perplexity"])) < RTOL * float(z["out/prob_perplexity"])
    assert abs(float(net["code_perplexity"]) - float(z["out/code_perplexity"])) < RTOL * float(z["out/code_perplexity"])
    assert net["q"].shape == (3, net["features"].shape[1], 64)                      # transposed: q at the encoder width


# ---------------------------------------------------------------------------------- the multitask model and criterion
@pytest.mark.parametrize("golden", sorted(UNISPEECH_GOLDENS))
def test_unispeech_step_vs_reference_golden(golden):
    """fp32, host Gumbel noise.  replace_mat bit-equal: the host RNG stream is aligned through the whole forward.  Bounds: RTOL on
    the loss, its CTC and InfoNCE parts and encoder_out, GTOL (gmax floor) on every gradient; the CTC term needed no other bound."""
    m, crit, z = build(golden, "cuda")
    m.train()
    sample = sample_of(z, "cuda")
    _seed()
    loss, ss, log = crit(m, sample)
    assert ss == int(z["out/sample_size"]) == log["infonce"]["sample_size"]
    assert int(log["infonce"]["correct"]) == int(z["log/infonce/correct"])
    for k in ("ntokens", "nsentences", "sample_size"):
        assert log["ctc"][k] == int(z["log/ctc/" + k]), k
    assert log["ntokens"] == 21 and log["nsentences"] == 3
    figs = [("loss", loss.item(), float(z["out/loss"])), ("ctc", log["ctc"]["loss"], float(z["log/ctc/loss"])),
            ("infonce", log["infonce"]["loss"], float(z["log/infonce/loss"]))]
    figs += [("infonce/" + k, log["infonce"][k], float(z["log/infonce/" + k])) for k in ("loss_0", "loss_1", "loss_2")]
    for name, got, want in figs:
        print("%s %s: %.6f reference %.6f" % (golden, name, got, want))
    for name, got, want in figs:
        assert abs(got - want) < RTOL * abs(want) + 1e-6, (name, got, want)
    loss.backward()
    gmax = max(float(np.abs(z[k]).max()) for k in z.files if k.startswith("grad/"))
    worst = (0.0, None)
    for n, p in m.named_parameters():
        ref = torch.from_numpy(z["grad/" + n])
        assert p.grad is not None, n
        err = (p.grad.detach().cpu() - ref).abs().max().item()
        tol = GTOL * max(ref.abs().max().item(), 1e-6 * gmax) + 1e-8
        worst = max(worst, (err / tol, n))
        assert err <= tol, (n, err, tol)
    print("%s: worst gradient error / bound %.3f (%s)" % (golden, worst[0], worst[1]))
    _seed()
    with torch.no_grad():
        net = m(**sample["net_input"])
    assert torch.equal(net["replace_mat"], torch.from_numpy(z["out/replace_mat"]))
    assert net["encoder_out"].shape == z["out/encoder_out"].shape and rel_err(net["encoder_out"], z["out/encoder_out"]) < RTOL
    assert net["encoder_out"].stride(1) > net["encoder_out"].stride(0)              # T x B x C view of batch-first storage


@pytest.mark.parametrize("golden", sorted(UNISPEECH_GOLDENS))
def test_unispeech_validation_vs_reference_golden(golden):
    """model.eval(): no time mask (every frame is a position), hard codes, the replace draw all the same, error counts"""
    m, crit, z = build(golden, "cuda")
    m.eval()
    sample = sample_of(z, "cuda")
    _seed()
    with torch.no_grad():
        net = m(**sample["net_input"])
    assert net["encoder_out"].grad_fn is None and not net["encoder_out"].requires_grad
    assert net["contrastive_res"]["head"]["loss"].grad_fn is None
    assert torch.equal(net["replace_mat"], torch.from_numpy(z["eval/replace_mat"]))
    _seed()
    with torch.no_grad():
        loss, ss, log = crit(m, sample)
    print("%s eval: loss %.6f reference %.6f, ctc %.6f / %.6f, infonce %.6f / %.6f" % (
        golden, loss.item(), float(z["eval/loss"]), log["ctc"]["loss"], float(z["eval/ctc_loss"]), log["infonce"]["loss"],
        float(z["eval/infonce_loss"])))
    assert ss == int(z["eval/sample_size"]) == 3 * net["encoder_out"].shape[0]
    assert abs(loss.item() - float(z["eval/loss"])) < RTOL * abs(float(z["eval/loss"]))
    for k in ("c_errors", "c_total", "w_errors", "w_total"):
        assert log["ctc"][k] == int(z["eval/" + k]), (k, log["ctc"][k], int(z["eval/" + k]))
    assert int(log["infonce"]["correct"]) == int(z["eval/correct"])


def _step(golden, dtype, **more):
    m, crit, z = build(golden, "cuda", **more)
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(p.to(torch.bfloat16).float())
    m = m.to(dtype).train()
    sample = sample_of(z, "cuda", dtype)
    _seed()
    loss, ss, log = crit(m, sample)
    loss.backward()
    return m, loss.item(), ss, log


def test_unispeech_bf16_vs_fp32_mode_of_the_same_path():
    """bf16 against the fp32 mode with bf16-rounded parameters and waveform and identical host draws: loss within 2e-3 relative,
    gradient norm within 2e-2 (tests/test_bf16_e2e_gpu.py)"""
    out = {}
    for dtype in (torch.float32, torch.bfloat16):
        m, l, ss, log = _step("tiny_unispeech.npz", dtype)
        gn = torch.sqrt(sum((p.grad.float() ** 2).sum() for p in m.parameters())).item()
        out[dtype] = (l, ss, gn, log["ctc"]["loss"], log["infonce"]["loss"])
    (l32, s32, g32, c32, n32), (l16, s16, g16, c16, n16) = out[torch.float32], out[torch.bfloat16]
    msg = "unispeech bf16 %.4f vs fp32 %.4f (ctc %.4f / %.4f, infonce %.4f / %.4f), gradient norm %.4f vs %.4f" % (
        l16, l32, c16, c32, n16, n32, g16, g32)
    print(msg)
    assert s16 == s32
    assert abs(l16 - l32) <= 2e-3 * abs(l32), msg
    assert abs(g16 - g32) <= 2e-2 * abs(g32), msg


def test_unispeech_final_dropout_is_reproducible():
    outs = []
    for _ in range(2):
        m, crit, z = build("tiny_unispeech.npz", "cuda", final_dropout=0.1)
        m.train()
        sample = sample_of(z, "cuda")
        _seed()
        loss, _, _ = crit(m, sample)
        assert torch.isfinite(loss)
        _seed()
        with torch.no_grad():
            outs.append(m(**sample["net_input"])["encoder_out"].clone())
    assert torch.equal(outs[0], outs[1])
    m0, _, z = build("tiny_unispeech.npz", "cuda")                                 # and dropout does change the logits
    m0.train()
    _seed()
    with torch.no_grad():
        assert not torch.equal(m0(**sample_of(z, "cuda")["net_input"])["encoder_out"], outs[0])


def test_unispeech_loss_ends_zero_the_expected_parameter_groups():
    """feature_grad_mult = 0 detaches the extractor.  mtlalpha = 1: only the CTC branch has a gradient -- the CTC head, the encoder,
    and through q the quantiser, project_q and final_proj; the extractor has none.  mtlalpha = 0 (no loss weights): the CTC head
    has none."""
    from unispeech_amd.unispeech import UnispeechCriterion
    from unispeech_cases import dictionary
    for alpha in (0.0, 1.0):
        m, _, z = build("tiny_unispeech.npz", "cuda", feature_grad_mult=0.0)
        m.train()
        crit = UnispeechCriterion(dictionary(), mtlalpha=alpha, infonce=True)
        _seed()
        loss, _, log = crit(m, sample_of(z, "cuda"))
        loss.backward()
        grads = {n: (p.grad is not None and bool(p.grad.abs().sum() > 0)) for n, p in m.named_parameters()}
        assert not any(v for n, v in grads.items() if ".feature_extractor." in n), alpha
        assert grads["w2v_encoder.w2v_model.encoder.layers.0.fc1.weight"] and grads["w2v_encoder.w2v_model.project_q.weight"]
        assert grads["w2v_encoder.w2v_model.final_proj.weight"] and grads["w2v_encoder.w2v_model.quantizer.vars"]
        assert grads["w2v_encoder.proj.weight"] == (alpha > 0) and grads["w2v_encoder.proj.bias"] == (alpha > 0)
        if alpha == 0.0:
            assert log["ctc"] == {} and log["ntokens"] == log["infonce"]["ntokens"]


def test_unispeech_twenty_adam_steps_lower_the_loss():
    from unispeech_amd.optim import FusedAdam
    m, crit, z = build("tiny_unispeech.npz", "cuda", final_dropout=0.1)
    m.train()
    m.w2v_encoder.w2v_model.quantizer.gumbel_noise = "device"                       # the production mode
    sample = sample_of(z, "cuda")
    opt = FusedAdam(m.parameters(), lr=1e-3, weight_decay=0.0)
    losses = []
    for step in range(20):
        m.set_num_updates(step)
        _seed()
        opt.zero_grad()
        loss, _, _ = crit(m, sample)
        loss.backward()
        opt.step()
        losses.append(loss.item())
    print("unispeech e2e: loss %.4f -> %.4f" % (losses[0], losses[-1]))
    assert np.isfinite(losses).all() and losses[-1] < losses[0]
