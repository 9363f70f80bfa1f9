"""csrc/ctc.hip on the device against torch's float64 F.ctc_loss on the CPU (tests/ctc_cases.py holds the cases and both
oracles), and EncoderCtc + CtcCriterion end to end on the tiny configuration of tests/test_model_gpu.py.

Tolerance: measured on the reference side, never on the device's.  E32 is the error of torch's own fp32 CPU F.ctc_loss against
float64 on the same inputs -- per sample for the loss, per sample the largest absolute error over (t, c) for the gradient.  The
kernel must lie within 4 x E32 of the float64 value (the factor of the fp32 front ends, tests/test_fbank_gpu.py): a log-add-exp
chain of several hundred steps rounds differently in any other evaluation order.  bf16 logits: float64 on the bf16 values, the
same loss bound; for the gradient, its one rounding to bf16 is added to 4 x E32.  bf16 keeps 8 significant bits, so rounding to
nearest moves a value g by up to 2^-8 |g| (just above a power of two) and no bf16 output can do better: the bound is, element by
element, err[t, c] <= 4 x E32 + 2^-8 |g[t, c]|.  The issue wrote 2^-9 |g|; element by element that is below the format's own
rounding: the test prints the largest (err - 4 x E32) / |g| in units of 2^-9 (measured: up to 1.84, i.e. between 2^-9 and 2^-8).
Per sample it is asserted as well, as 4 x E32 + 2^-9 P with P the power of two at or above the sample's largest |g|: half a bf16
ulp of the largest elements.  (It used to read 2^-9 max |g|, which cases A to E meet only because their largest |g| is 0.92 to
1.00; in the peaked cases it is 0.51 to 0.87, an element between 0.5 and that rounds by up to 2^-9 whatever computed it, and the
kernel's correctly rounded output measured 0.00194 against 0.00189.)  Worst ratios are printed
(-s); for bf16 the printed gradient ratio is the largest (err - 2^-8 |g|) / E32 over the elements, floored at 0.
A sample without an alignment: loss inf and, as in torch, NaN in its gradient rows; under zero_infinity exactly 0 for both.

Variants.  The two heavy kernels are compiled for 1, 2, 4 or 8 extended positions per lane (S = 2 Lmax + 1 up to 256, 512, 1024,
2047) and the longest target of a batch picks the variant for all of it.  The parity tests run every case of ctc_cases.CASES in
both dtypes; the names of the cases added for this carry the variant (L127_per1 ... L1023_per8: S = 255 | 257, 511 | 513,
1023 | 1025 and 2047), and tests/test_ctc.py asserts without a GPU that together they reach all four, that each variant meets a
sample shorter than the batch's longest, and that 4 x E32 of the peaked cases is below 1 % of the gradient.  Across variants
(test_same_bits_in_every_variant): the L = 5 and L = 300 samples of the Lmax = 1023 batch run alone (PER 1 and PER 4), the
two together (L = 5 under PER 4), the L = 0 sample alone, and the L = 90 sample of L128_per2 alone (PER 1 beside PER 2) give
torch.equal loss and gradient rows to what they give in their batch, in fp32 and bf16; so do a permutation of the Lmax = 1023
batch and a second run of it.  Another blank than 0, and labels that name the blank (ctc_cases.BLANK_CASES), go through the same
parity check; strides, the guard band and autograd are repeated on a PER = 4 case."""
import numpy as np
import pytest
import torch

import ctc_cases as CC
from conftest import TINY

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def leave_no_device_memory_behind():
    """the kernel's workspace is cached for the life of the process; drop it when this module is done, so that later modules
    meet the caching allocator as they did before this one existed"""
    yield
    import gc
    from unispeech_amd import ops
    for key in [k for k in ops._WS if k[1] == "ctc"]:
        del ops._WS[key]
    gc.collect()
    torch.cuda.empty_cache()


def _args(targets, tl, il):
    t = targets.to(torch.int32).cuda()
    if t.numel() == 0:
        t = torch.zeros(1, dtype=torch.int32, device="cuda")
    off = torch.tensor(np.concatenate([[0], np.cumsum(tl)]).astype(np.int32)).cuda()
    return t, off, int(sum(tl)), int(max(tl)), torch.tensor(il, dtype=torch.int32).cuda()


def _run(name, dtype=torch.float32, zero_infinity=False, tbc_view=False, samples=None, grad_out=None, blank=CC.BLANK):
    """(nll [B], dlogits [T, B, C]) as float64 numpy + the raw device tensors; samples: a subset / permutation of the batch"""
    from unispeech_amd import ops
    logits, targets, il, tl = CC.case(name)
    if samples is not None:
        offs = np.concatenate([[0], np.cumsum(tl)])
        targets = torch.cat([targets[offs[b]:offs[b + 1]] for b in samples]) if samples else targets[:0]
        logits, il, tl = logits[:, samples], [il[b] for b in samples], [tl[b] for b in samples]
    x = logits.to(dtype)
    if tbc_view:
        x = x.contiguous().cuda().transpose(0, 1)              # T x B x C storage, read through its [B, T, C] view
    else:
        x = x.transpose(0, 1).contiguous().cuda()              # batch-first storage
    nll, dx = ops.ctc_loss_fwd_bwd(x, *_args(targets, tl, il), blank, grad_out, zero_infinity)
    torch.cuda.synchronize()
    return nll, dx.transpose(0, 1)


def f64(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


def _check_parity(name, dtype, blank=CC.BLANK):
    bf16 = dtype == torch.bfloat16
    _, _, il, tl = CC.case(name)
    l64, g64 = CC.ref64(name, False, bf16, blank)
    el, eg = CC.e32(name, bf16, blank)
    nll_t, dx_t = _run(name, dtype, blank=blank)
    nll, dx = f64(nll_t), f64(dx_t)
    assert dx_t.dtype == dtype and nll_t.dtype == torch.float32
    inf = CC.INF_SAMPLES[name]
    assert [b for b in range(len(il)) if not np.isfinite(l64[b])] == inf
    worst_l = worst_g = 0.0
    for b in range(len(il)):
        assert (dx[il[b]:, b] == 0).all(), "rows at or beyond the input length must be exactly zero"
        if b in inf:
            assert nll[b] == np.inf and np.isnan(dx[:il[b], b]).all()
            continue
        err_l = abs(nll[b] - l64[b])
        err_g = np.abs(dx[:, b] - g64[:, b])
        slack = 2.0 ** -8 * np.abs(g64[:, b]) if bf16 else 0.0                 # element by element: the rounding to bf16
        rl = err_l / el[b] if el[b] > 0 else (0.0 if err_l == 0 else np.inf)
        over = float((err_g - slack).max())
        rg = max(over / eg[b], 0.0) if eg[b] > 0 else (0.0 if over <= 0 else np.inf)     # E32 = 0: a single class, all zeros
        big = np.abs(g64[:, b]) > 1e-3
        if bf16 and big.any():
            print("ctc parity %s bf16 sample %d: largest (err - 4 E32) / |g| = %.3f x 2^-9 over the elements with |g| > 1e-3"
                  % (name, b, float(((err_g[big] - 4 * eg[b]) / np.abs(g64[:, b][big])).max() * 2.0 ** 9)))
        print("ctc parity %s %s sample %d: loss %.6g err %.3e (E32 %.3e, ratio %.3f); grad err %.3e (E32 %.3e, ratio %.3f)"
              % (name, "bf16" if bf16 else "fp32", b, l64[b], err_l, el[b], rl, err_g.max(), eg[b], rg))
        worst_l, worst_g = max(worst_l, rl), max(worst_g, rg)
        assert err_l <= 4 * el[b]
        assert (err_g <= 4 * eg[b] + slack).all()
        gmax = np.abs(g64[:, b]).max()
        if bf16 and gmax > 0:                                   # per sample like E32: half a bf16 ulp at the largest magnitude
            assert err_g.max() <= 4 * eg[b] + 2.0 ** -9 * 2.0 ** np.ceil(np.log2(gmax))
    print("ctc parity %s %s: worst loss ratio %.3f, worst gradient ratio %.3f" % (name, "bf16" if bf16 else "fp32", worst_l, worst_g))
    # zero_infinity: the samples without an alignment are exactly zero, the others the same bits
    z_nll, z_dx = _run(name, dtype, zero_infinity=True, blank=blank)
    for b in range(len(il)):
        if b in inf:
            assert z_nll[b].item() == 0.0 and (z_dx[:, b] == 0).all()
        else:
            assert torch.equal(z_nll[b], nll_t[b]) and torch.equal(z_dx[:, b], dx_t[:, b])


@pytest.mark.parametrize("name", list(CC.CASES))
def test_parity_fp32(name):
    _check_parity(name, torch.float32)


@pytest.mark.parametrize("name", list(CC.CASES))
def test_parity_bf16(name):
    _check_parity(name, torch.bfloat16)


@pytest.mark.parametrize("name", list(CC.BLANK_CASES))
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_parity_with_another_blank(name, dtype):
    """blank = C - 1; blank = 7 with three labels that are 7 themselves (two of them a repeated pair): the blank wave owns those
    positions, and the ranks of the other classes skip over them"""
    _check_parity(name, dtype, CC.BLANK_CASES[name]["blank"])


def _check_strides_and_guard_band(name):
    from unispeech_amd import ops
    a_nll, a_dx = _run(name)
    b_nll, b_dx = _run(name, tbc_view=True)
    assert torch.equal(a_nll, b_nll) and torch.equal(a_dx, b_dx)
    # a view of a wider buffer: [B, T + 3, C + 5] storage, frames 2 .. T + 1 and classes 0 .. C - 1 of it
    logits, targets, il, tl = CC.case(name)
    T, B, C = logits.shape
    wide_x = torch.full((B, T + 3, C + 5), 123.0, device="cuda")
    wide_x[:, 2:T + 2, :C] = logits.transpose(0, 1).cuda()
    wide_g = torch.full((B, T + 3, C + 5), 7.0, device="cuda")
    view = wide_g[:, 2:T + 2, :C]
    nll, dx = ops.ctc_loss_fwd_bwd(wide_x[:, 2:T + 2, :C], *_args(targets, tl, il), CC.BLANK, None, False, dlogits=view)
    assert dx.data_ptr() == view.data_ptr()
    assert torch.equal(nll, a_nll) and torch.equal(view.transpose(0, 1), a_dx)
    outside = torch.ones_like(wide_g, dtype=torch.bool)
    outside[:, 2:T + 2, :C] = False
    assert (wide_g[outside] == 7.0).all(), "bytes outside the B x T x C view were written"


def test_strides_and_guard_band():
    _check_strides_and_guard_band("B")


def test_strides_and_guard_band_at_four_positions_per_lane():
    """S = 1023: the alpha workspace's stride and the dx stores of the second to fourth sweep"""
    assert CC.variant(max(CC.case("L511_per4")[3])) == 4
    _check_strides_and_guard_band("L511_per4")


def test_reproducible_and_independent_of_the_batch():
    a = _run("E")
    b = _run("E")
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    c_nll, c_dx = _run("C")
    s_nll, s_dx = _run("C", samples=[0])
    assert torch.equal(s_nll[0], c_nll[0]) and torch.equal(s_dx[:, 0], c_dx[:, 0])
    perm = [2, 0, 3, 1]
    p_nll, p_dx = _run("E", samples=perm)
    for i, b in enumerate(perm):
        assert torch.equal(p_nll[i], a[0][b]) and torch.equal(p_dx[:, i], a[1][:, b])


def _same_bits(name, dtype, samples, batch):
    """the samples run as a batch of their own give the bits of their rows in `batch`, the (nll, dx) of the whole case"""
    nll, dx = _run(name, dtype, samples=samples)
    for i, b in enumerate(samples):
        assert torch.equal(nll[i], batch[0][b]), (name, samples, b)
        assert torch.equal(dx[:, i], batch[1][:, b]), (name, samples, b)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_same_bits_in_every_variant(dtype):
    """a sample's loss and gradient do not depend on the variant its batch picks: the riders of the Lmax = 1023 batch (PER 8,
    alpha stride 2047) alone, where the L = 5 one runs PER 1 with stride 11 and the L = 300 one PER 4 with stride 601"""
    name = "L1023_per8"
    tl = CC.case(name)[3]
    assert tl == [1023, 0, 5, 300] and [CC.variant(L) for L in tl] == [8, 1, 1, 4]
    batch = _run(name, dtype)
    again = _run(name, dtype)
    assert torch.equal(batch[0], again[0]) and torch.equal(batch[1], again[1])
    assert torch.isfinite(batch[0]).all() and (batch[0] > 0).all()
    _same_bits(name, dtype, [2], batch)              # PER 1
    _same_bits(name, dtype, [3], batch)              # PER 4
    _same_bits(name, dtype, [1], batch)              # the empty target: S = 1
    _same_bits(name, dtype, [2, 3], batch)           # L = 5 under PER 4
    _same_bits(name, dtype, [3, 1, 0, 2], batch)     # a permutation of the batch
    name = "L128_per2"
    assert [CC.variant(L) for L in CC.case(name)[3]] == [2, 1]
    _same_bits(name, dtype, [1], _run(name, dtype))  # PER 1 alone, PER 2 in its batch


def test_edge_inputs_against_the_restatement():
    """input_length 0 (empty and non-empty target), an empty target on a full input, and a sample whose label is out of range
    beside valid ones: the Tb == 0 and the rejected-sample branches of both kernels, against ctc_reference"""
    from unispeech_amd import ops
    from unispeech_amd.ctc import ctc_reference
    g = torch.Generator().manual_seed(21)
    T, B, C = 9, 5, 6
    logits = torch.randn(T, B, C, generator=g) * 3
    tl, il = [0, 2, 0, 3, 2], [0, 0, 9, 9, 7]
    targets = torch.tensor([3, 4, 1, 2, 5, 2, 1])
    want_l, want_g = ctc_reference(logits.double().numpy(), targets.numpy(), il, tl, CC.BLANK)
    assert want_l[0] == 0 and want_l[1] == np.inf and np.isfinite(want_l[2:]).all()
    for zi in (False, True):
        x = logits.transpose(0, 1).contiguous().cuda()
        nll, dx = ops.ctc_loss_fwd_bwd(x, *_args(targets, tl, il), CC.BLANK, None, zi)
        nll, dx = f64(nll), f64(dx.transpose(0, 1))
        assert nll[0] == 0 and nll[1] == (0 if zi else np.inf) and (dx[:, :2] == 0).all()
        assert np.abs(nll[2:] - want_l[2:]).max() <= 2.0 ** -22 * want_l[2:].max()      # fp32 output: two ulps
        assert np.abs(dx[:, 2:] - want_g[:, 2:]).max() <= 1e-5 and (dx[7:, 4] == 0).all()
    # sample 1's label 6 is not a class, sample 3's offsets run backwards: NaN loss, zero gradient, the others untouched
    bad_t = torch.tensor([3, 6, 1, 2, 5, 2, 1], dtype=torch.int32).cuda()
    off = torch.tensor([0, 0, 2, 2, 5, 7], dtype=torch.int32).cuda()
    il9 = torch.tensor([9, 9, 9, 9, 7], dtype=torch.int32).cuda()
    x = logits.transpose(0, 1).contiguous().cuda()
    good_nll, good_dx = ops.ctc_loss_fwd_bwd(x, targets.to(torch.int32).cuda(), off, 7, 3, il9, CC.BLANK)
    nll, dx = ops.ctc_loss_fwd_bwd(x, bad_t, off, 7, 3, il9, CC.BLANK)
    assert torch.isnan(nll[1]) and (dx[1] == 0).all()
    keep = [0, 2, 3, 4]
    assert torch.equal(nll[keep], good_nll[keep]) and torch.equal(dx[keep], good_dx[keep])
    off_bad = torch.tensor([0, 0, 2, 5, 2, 7], dtype=torch.int32).cuda()
    nll, dx = ops.ctc_loss_fwd_bwd(x, targets.to(torch.int32).cuda(), off_bad, 7, 3, il9, CC.BLANK)
    assert torch.isnan(nll[3]) and (dx[3] == 0).all() and torch.equal(nll[:2], good_nll[:2])


@pytest.mark.parametrize("name", ["B", "C", "L511_per4"])
def test_autograd(name):
    from unispeech_amd.ctc import ctc_loss
    logits, targets, il, tl = CC.case(name)
    _, g64 = CC.ref64(name)
    l64, _ = CC.ref64(name)
    el, eg = CC.e32(name)
    x = logits.cuda().requires_grad_(True)
    loss = ctc_loss(x, targets, il, tl, blank=CC.BLANK, reduction="sum")
    # three fp32 roundings (two samples, their sum) of half an ulp each: 2^-22 relative is two ulps
    assert loss.dim() == 0 and abs(loss.item() - l64.sum()) <= 2.0 ** -22 * l64.sum()
    loss.backward()
    assert x.grad.shape == x.shape
    assert (np.abs(f64(x.grad) - g64).max(axis=(0, 2)) <= 4 * eg).all()
    # a non-trivial upstream gradient per sample
    w = [0.25, -3.0]
    _, gw64 = CC.torch_ctc(logits, targets, il, tl, torch.float64, weights=w)
    x.grad = None
    (ctc_loss(x, targets, il, tl, blank=CC.BLANK, reduction="none") * torch.tensor(w).cuda()).sum().backward()
    assert (np.abs(f64(x.grad) - gw64).max(axis=(0, 2)) <= 4 * eg * np.abs(w)).all()
    # targets as a padded [B, Lmax] tensor read the same
    offs = np.concatenate([[0], np.cumsum(tl)])
    padded = torch.zeros(len(tl), max(tl), dtype=torch.long)
    for b in range(len(tl)):
        padded[b, :tl[b]] = targets[offs[b]:offs[b + 1]]
    with torch.no_grad():
        assert torch.equal(ctc_loss(x, padded, il, tl, reduction="none"), ctc_loss(x, targets, il, tl, reduction="none"))


def _tie_lattice():
    g = torch.Generator().manual_seed(5)
    return torch.randint(0, 3, (37, 3, 6), generator=g).float(), [37, 20, 0]


def test_greedy_decode_on_the_device_equals_the_host():
    from unispeech_amd.ctc import greedy_decode
    for name in ("B", "C"):
        logits, _, il, _ = CC.case(name)
        host = greedy_decode(logits, il, CC.BLANK)
        assert greedy_decode(logits.cuda(), il, CC.BLANK) == host
        assert greedy_decode(logits.transpose(0, 1).contiguous().cuda().transpose(0, 1), il, CC.BLANK) == host
    lat, il = _tie_lattice()
    host = greedy_decode(lat, il, 1)
    assert host[2] == [] and len(host[0]) > 3
    assert greedy_decode(lat.cuda(), il, 1) == host
    assert greedy_decode(lat.to(torch.bfloat16).cuda(), il, 1) == host


def test_refusals_name_the_argument():
    from unispeech_amd.ctc import ctc_loss
    x = torch.zeros(4, 1, 1025, device="cuda")
    with pytest.raises(NotImplementedError, match=r"C = 1025"):
        ctc_loss(x, torch.ones(2, dtype=torch.long), [4], [2])
    x = torch.zeros(4, 1, 8, device="cuda")
    with pytest.raises(NotImplementedError, match=r"L = 1024"):
        ctc_loss(x, torch.ones(1024, dtype=torch.long), [4], [1024])


# -------------------------------------------------------------------------------------------------------------- end to end
NCLS = 12


def _tiny_ctc(dtype=torch.float32, **options):
    from unispeech_amd.ctc import CtcCriterion, EncoderCtc
    from unispeech_amd.pretrain import WavLMPretrainConfig, WavLMPretrainModel
    torch.manual_seed(0)
    cfg = WavLMPretrainConfig(**{k: v for k, v in TINY.items() if k in WavLMPretrainConfig.__dataclass_fields__})
    w2v = WavLMPretrainModel(cfg, None, [range(23)])
    w2v.remove_pretraining_modules()
    model = EncoderCtc(w2v, NCLS, **options).cuda().to(dtype).train()
    crit = CtcCriterion(blank_idx=0, pad_idx=1, eos_idx=2, zero_infinity=True, post_process=None)
    g = torch.Generator().manual_seed(1)
    wav = torch.randn(2, 8000, generator=g)
    pm = torch.zeros(2, 8000, dtype=torch.bool)
    pm[1, 6400:] = True
    wav[1, 6400:] = 0
    target = torch.tensor([[4, 5, 5, 7, 9, 2], [6, 3, 8, 2, 1, 1]])          # eos = 2, pad = 1
    sample = {"id": torch.arange(2), "target": target.cuda(),
              "net_input": {"source": wav.to(dtype).cuda(), "padding_mask": pm.cuda()}}
    return model, crit, sample


def test_e2e_loss_is_ctc_loss_of_the_models_own_logits():
    from unispeech_amd.ctc import ctc_loss
    model, crit, sample = _tiny_ctc()
    net = model(**sample["net_input"])
    x = net["encoder_out"]
    T, B, C = x.shape
    # batch-first storage behind a T x B x C view (rows of 16: the head pads its 12 classes to a multiple of 8 for the call)
    assert (B, C) == (2, NCLS) and x.stride() == (16, T * 16, 1)
    loss, sample_size, log = crit.get_loss(model, sample, net)
    il = (~net["padding_mask"]).sum(-1).tolist()
    assert il[0] == T and 0 < il[1] < T
    want = ctc_loss(x.detach(), torch.tensor([4, 5, 5, 7, 9, 6, 3, 8]), il, [5, 3], blank=0, reduction="sum", zero_infinity=True)
    assert torch.equal(loss.detach(), want) and torch.isfinite(loss) and loss.item() > 0
    assert (sample_size, log["ntokens"], log["nsentences"]) == (8, 8, 2) and log["loss"] == loss.item()
    model.eval()
    with torch.no_grad():
        _, _, elog = crit(model, sample)
    assert elog["c_total"] == 8 and 0 <= elog["c_errors"] and elog["wv_errors"] == elog["w_errors"]


def test_e2e_freeze_and_feature_grad_mult():
    model, crit, sample = _tiny_ctc(freeze_finetune_updates=2, feature_grad_mult=0.0)
    enc = model.w2v_encoder
    model.set_num_updates(0)
    crit(model, sample)[0].backward()
    assert enc.proj.weight.grad is not None and enc.proj.weight.grad.abs().max() > 0 and enc.proj.bias.grad is not None
    assert all(p.grad is None for p in enc.w2v_model.parameters())
    model.zero_grad(set_to_none=True)
    model.set_num_updates(2)
    crit(model, sample)[0].backward()
    seen = 0
    for n, p in enc.w2v_model.encoder.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), n
        if n.endswith(("fc1.weight", "fc2.weight", "out_proj.weight", "v_proj.weight")):
            assert p.grad.abs().max() > 0, n
            seen += 1
    assert seen >= 8
    assert all(p.grad is None for p in enc.w2v_model.feature_extractor.parameters())
    # with a multiplier the extractor trains too
    model, crit, sample = _tiny_ctc(feature_grad_mult=0.5)
    crit(model, sample)[0].backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in model.w2v_encoder.w2v_model.feature_extractor.parameters())


def test_e2e_twenty_adam_steps_lower_the_loss():
    from unispeech_amd.optim import FusedAdam
    model, crit, sample = _tiny_ctc()
    opt = FusedAdam(model.parameters(), lr=1e-3, weight_decay=0.0)
    losses = []
    for step in range(20):
        model.set_num_updates(step)
        opt.zero_grad()
        loss, _, _ = crit(model, sample)
        loss.backward()
        opt.step()
        losses.append(loss.item())
    print("ctc e2e: loss %.4f -> %.4f" % (losses[0], losses[-1]))
    assert np.isfinite(losses).all() and losses[-1] < losses[0]


def test_e2e_bf16_runs():
    model, crit, sample = _tiny_ctc(torch.bfloat16)
    loss, _, _ = crit(model, sample)
    assert loss.dtype == torch.float32 and torch.isfinite(loss)
    loss.backward()
    assert torch.isfinite(model.w2v_encoder.proj.weight.grad.float()).all()


def test_e2e_validation_keeps_no_graph_and_decode_command(tmp_path, capsys):
    """under the caller's no_grad the fine-tuned encoder records nothing (hubert_asr.py:324 uses a null context there); and
    `python -m unispeech_amd.ctc decode` on a checkpoint file written here: one line per wav file"""
    import wave
    from unispeech_amd import ctc
    model, crit, sample = _tiny_ctc()
    model.eval()
    with torch.no_grad():
        net = model(**sample["net_input"])
    assert not net["encoder_out"].requires_grad and net["encoder_out"].grad_fn is None
    d = ["|"] + [chr(ord("A") + i) for i in range(NCLS - 5)]                    # 4 specials + 8 symbols = NCLS classes
    (tmp_path / "dict.ltr.txt").write_text("".join("%s 1\n" % c for c in d))
    cfg = {k: v for k, v in TINY.items()}
    torch.save({"cfg": cfg, "model": model.state_dict(), "arch": "wavlm", "normalize": False}, str(tmp_path / "ck.pt"))
    wavs = []
    for i, n in enumerate((8000, 5000)):
        pcm = (sample["net_input"]["source"][i, :n].float().cpu().clamp(-1, 1) * 3000).to(torch.int16).numpy()
        path = str(tmp_path / ("u%d.wav" % i))
        with wave.open(path, "wb") as w:
            w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000); w.writeframes(pcm.tobytes())
        wavs.append(path)
    assert ctc.main(["decode", str(tmp_path / "ck.pt"), str(tmp_path / "dict.ltr.txt")] + wavs) == 0
    lines = capsys.readouterr().out.splitlines()
    assert len(lines) == 2                                  # (an untrained head: the text itself means nothing)
    # the same through the functions: what the command printed is the greedy decode of the loaded model
    dic = ctc.LetterDictionary.load(str(tmp_path / "dict.ltr.txt"))
    loaded, normalize = ctc.load_ctc_checkpoint(str(tmp_path / "ck.pt"), len(dic))
    assert not normalize and len(dic) == NCLS
    from unispeech_amd.kmeans import read_wav
    x = torch.as_tensor(read_wav(wavs[0])[0], dtype=torch.float32).cuda().view(1, -1)
    with torch.no_grad():
        toks = ctc.greedy_decode(loaded(source=x, padding_mask=None)["encoder_out"], None, 0)[0]
    assert ctc.post_process(dic.string(toks), "letter") == lines[0]
