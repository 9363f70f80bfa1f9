"""CTC fine-tuning, host side (unispeech_amd/ctc.py): the float64 restatement against torch's F.ctc_loss (another blank than 0
included), the conditions that the cases of tests/ctc_cases.py must meet for the GPU parity tests to mean something (every
kernel variant reached; the tolerance neither blind nor below the output format), the criterion against a
restatement of the reference's criterions/ctc.py:110-160 on a stub model, the edit distance, the greedy decode's host path, the
key set and the refusals of EncoderCtc, and the ABI bookkeeping.  No GPU."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ctc_cases as CC
from conftest import TINY

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("name", list(CC.CASES))
def test_reference_equals_torch_float64(name):
    from unispeech_amd.ctc import ctc_reference
    logits, targets, il, tl = CC.case(name)
    l64, g64 = CC.ref64(name)
    loss, grad = ctc_reference(logits.double().numpy(), targets.numpy(), il, tl, CC.BLANK)
    fin = np.isfinite(l64)
    assert [b for b in range(len(il)) if not fin[b]] == CC.INF_SAMPLES[name]
    assert (np.abs(loss[fin] - l64[fin]) <= 1e-10 * np.abs(l64[fin])).all()
    assert np.abs(grad[:, fin] - g64[:, fin]).max() <= 1e-10 * np.abs(g64[:, fin]).max()
    assert (loss[~fin] == np.inf).all()
    for b in np.flatnonzero(~fin):                      # torch's rows of such a sample are NaN as well
        assert np.isnan(grad[:il[b], b]).all() and (grad[il[b]:, b] == 0).all()
    zl, zg = ctc_reference(logits.double().numpy(), targets.numpy(), il, tl, CC.BLANK, zero_infinity=True)
    tzl, tzg = CC.ref64(name, True)
    assert (zl[~fin] == 0).all() and (zg[:, ~fin] == 0).all() and (tzl[~fin] == 0).all() and (tzg[:, ~fin] == 0).all()
    assert np.array_equal(zl[fin], loss[fin]) and np.array_equal(zg[:, fin], grad[:, fin])
    # padded targets read the same
    offs = np.concatenate([[0], np.cumsum(tl)])
    padded = np.zeros((len(tl), max(tl)), dtype=np.int64)
    for b in range(len(tl)):
        padded[b, :tl[b]] = targets.numpy()[offs[b]:offs[b + 1]]
    pl, _ = ctc_reference(logits.double().numpy(), padded, il, tl, CC.BLANK)
    assert np.array_equal(pl, loss)


@pytest.mark.parametrize("name", list(CC.BLANK_CASES))
def test_reference_equals_torch_float64_with_another_blank(name):
    """blank = C - 1, and blank = 7 with labels that are 7 themselves"""
    from unispeech_amd.ctc import ctc_reference
    logits, targets, il, tl = CC.case(name)
    blank = CC.BLANK_CASES[name]["blank"]
    first = targets[:tl[0]].tolist()
    assert blank != CC.BLANK and (blank in first) == (name == "blank7")
    if name == "blank7":
        assert first[2] == first[3] == first[10] == 7 and first.count(7) == 3
    l64, g64 = CC.ref64(name, blank=blank)
    assert np.isfinite(l64).all() and CC.INF_SAMPLES[name] == []
    loss, grad = ctc_reference(logits.double().numpy(), targets.numpy(), il, tl, blank)
    assert (np.abs(loss - l64) <= 1e-10 * np.abs(l64)).all() and np.abs(grad - g64).max() <= 1e-10 * np.abs(g64).max()
    wrong, _ = CC.ref64(name)                            # the blank matters: with blank 0 the same labels cost something else
    assert (np.abs(wrong - l64) > 1e-3 * l64).all()


def test_the_new_cases_reach_every_variant_and_their_bound_can_tell():
    """Conditions on the inputs of tests/ctc_cases.py, decided by the references alone (torch float64 and torch fp32 on the
    CPU), on the fp32 logits and on their bf16 roundings.
    Coverage: the cases reach PER = 1, 2, 4, 8, each with a sample shorter than the batch's longest, and S on both sides of every
    boundary.  Peaked cases: 4 x E32 is at most 1 % of the sample's largest gradient and 1e-4 of its loss, so an error of a few
    per cent cannot pass.  Every new case: E32 is at least 2^-24 of the loss and of the largest gradient -- half an ulp of an fp32
    output at most, so the float64 result rounded to fp32 is within the bound.  The random cases are exempt from the 1 % cap
    (their ratio is printed)."""
    reached, with_rider, S_seen = set(), set(), set()
    for name, c in list(CC.CASES.items()) + list(CC.BLANK_CASES.items()):
        per = CC.variant(max(c["tl"]))
        reached.add(per)
        S_seen.add(2 * max(c["tl"]) + 1)
        if min(c["tl"]) < max(c["tl"]):
            with_rider.add(per)
        if name in CC.NEW_CASES and name in CC.CASES:
            assert name.endswith("_per%d" % per), "the name of a case states the variant it runs"
    assert reached == with_rider == {1, 2, 4, 8}
    assert {255, 257, 511, 513, 1023, 1025, 2047} <= S_seen
    assert [c["tl"] for c in CC.CASES.values()].count([1023, 0, 5, 300]) == 1       # the riders that are also run alone
    assert CC.variant(5) == 1 and CC.variant(300) == 4 and CC.variant(1023) == 8
    for name in CC.NEW_CASES:
        c = CC.CASES[name] if name in CC.CASES else CC.BLANK_CASES[name]
        blank = c.get("blank", CC.BLANK)
        for bf16 in (False, True):
            l64, g64 = CC.ref64(name, False, bf16, blank)
            el, eg = CC.e32(name, bf16, blank)
            assert [b for b in range(c["B"]) if not np.isfinite(l64[b])] == CC.INF_SAMPLES[name]
            zl, zg = CC.ref64(name, True, bf16, blank)
            for b in range(c["B"]):
                if b in CC.INF_SAMPLES[name]:
                    assert c["il"][b] < c["T"] and zl[b] == 0 and (zg[:, b] == 0).all()
                    continue
                gmax = np.abs(g64[:, b]).max()
                print("ctc conditions %s %s sample %d: loss %.6g, 4 E32loss / loss %.2e, E32loss / (2^-24 loss) %.2f; max |g| %.3f, "
                      "4 E32grad / max |g| %.2e" % (name, "bf16" if bf16 else "fp32", b, l64[b], 4 * el[b] / max(l64[b], 1e-300),
                                                   el[b] / max(2.0 ** -24 * l64[b], 1e-300), gmax, 4 * eg[b] / max(gmax, 1e-300)))
                assert el[b] >= 2.0 ** -24 * l64[b] and eg[b] >= 2.0 ** -24 * gmax
                if "peak" in c:
                    assert 4 * eg[b] <= 0.01 * gmax and 4 * el[b] <= 1e-4 * l64[b]
    for name, c in CC.CASES.items():
        if "peak" in c:
            assert c["C"] == 32 and min(c["il"]) < c["T"]
            _, targets, _, tl = CC.case(name)
            if "labels" not in c:
                assert targets[1] == targets[0] and targets[3] == targets[2]
    # the label structures the table promises
    _, t, _, tl = CC.case("runs256_per4")
    same, alt = t[:256], t[256:]
    assert (same == same[0]).all() and (alt[::2] == alt[0]).all() and (alt[1::2] == alt[1]).all() and alt[0] != alt[1]
    _, t, _, tl = CC.case("C1024_per1")
    assert {768, 1023} <= set(t[:tl[0]].tolist()) and 1023 in t[tl[0]:].tolist()
    _, t, _, tl = CC.case("C257_per1")
    assert 256 in t[:tl[0]].tolist() and 256 in t[tl[0]:].tolist()


def test_reference_input_length_zero_and_host_autograd():
    from unispeech_amd.ctc import ctc_loss, ctc_reference
    logits, targets, il, tl = CC.case("A")
    loss, grad = ctc_reference(logits.numpy(), targets.numpy(), [0, 0, 5], tl)
    assert loss[0] == np.inf and loss[1] == 0 and (grad[:, :2] == 0).all()
    x = logits[:, :2].clone().requires_grad_(True)
    w = torch.tensor([0.5, -2.0])
    (ctc_loss(x, targets[:2], il[:2], tl[:2], reduction="none") * w).sum().backward()
    _, g64 = CC.torch_ctc(logits[:, :2], targets[:2], il[:2], tl[:2], torch.float64, weights=w.tolist())
    assert np.abs(x.grad.double().numpy() - g64).max() <= 1e-6
    with pytest.raises(ValueError, match="reduction"):
        ctc_loss(x, targets[:2], il[:2], tl[:2], reduction="batchmean")


# ------------------------------------------------------------------------------------------------------------- criterion
class _Stub(torch.nn.Module):
    def __init__(self, logits, padding_mask=None):
        super().__init__()
        self.logits, self.pm = logits, padding_mask

    def forward(self, **kw):
        return {"encoder_out": self.logits, "encoder_padding_mask": self.pm, "padding_mask": self.pm}


PAD, EOS = 1, 2


def _restate(logits, sample, net_output, sentence_avg, zero_infinity):
    """criterions/ctc.py:110-160 with F.ctc_loss on the CPU in float64"""
    lprobs = F.log_softmax(logits.double(), -1)
    if "src_lengths" in sample["net_input"]:
        input_lengths = sample["net_input"]["src_lengths"]
    elif net_output["padding_mask"] is not None:
        input_lengths = (~net_output["padding_mask"]).long().sum(-1)
    else:
        input_lengths = lprobs.new_full((lprobs.size(1),), lprobs.size(0), dtype=torch.long)
    pad_mask = (sample["target"] != PAD) & (sample["target"] != EOS)
    targets_flat = sample["target"].masked_select(pad_mask)
    target_lengths = pad_mask.sum(-1)
    loss = F.ctc_loss(lprobs, targets_flat, input_lengths, target_lengths, blank=0, reduction="sum", zero_infinity=zero_infinity)
    ntokens = sample["ntokens"] if "ntokens" in sample else target_lengths.sum().item()
    sample_size = sample["target"].size(0) if sentence_avg else ntokens
    return loss, sample_size, {"loss": loss.item(), "ntokens": ntokens, "nsentences": sample["id"].numel(),
                               "sample_size": sample_size}


@pytest.mark.parametrize("lengths_from", ["src_lengths", "padding_mask", "neither"])
@pytest.mark.parametrize("sentence_avg", [False, True])
def test_criterion_equals_the_reference_restated(lengths_from, sentence_avg):
    from unispeech_amd.ctc import CtcCriterion
    g = torch.Generator().manual_seed(3)
    T, B, C = 30, 3, 9
    logits = (torch.randn(T, B, C, generator=g) * 3).requires_grad_(True)
    target = torch.tensor([[4, 4, 5, 8, EOS, PAD, PAD], [3, 6, 7, 7, 7, 5, EOS], [EOS, PAD, PAD, PAD, PAD, PAD, PAD]])
    sample = {"id": torch.arange(B), "target": target, "net_input": {"source": None}}
    pm = None
    if lengths_from == "src_lengths":
        sample["net_input"]["src_lengths"] = torch.tensor([30, 22, 9])
    elif lengths_from == "padding_mask":
        pm = torch.zeros(B, T, dtype=torch.bool)
        pm[1, 25:] = True
        pm[2, 4:] = True
    model = _Stub(logits, pm).train()
    crit = CtcCriterion(blank_idx=0, pad_idx=PAD, eos_idx=EOS, sentence_avg=sentence_avg)
    loss, sample_size, log = crit(model, sample)
    want, want_size, want_log = _restate(logits.detach(), sample, model(), sentence_avg, False)
    assert sample_size == want_size == (3 if sentence_avg else 10)
    assert set(log) == {"loss", "ntokens", "nsentences", "sample_size"}
    assert abs(loss.item() - want.item()) <= 2.0 ** -22 * want.item()              # the loss is returned in fp32
    assert abs(log["loss"] - want_log["loss"]) <= 2.0 ** -22 * want.item()
    assert {k: log[k] for k in ("ntokens", "nsentences", "sample_size")} == {k: want_log[k] for k in ("ntokens", "nsentences", "sample_size")}
    loss.backward()
    x64 = logits.detach().double().requires_grad_(True)
    _restate(x64, sample, model(), sentence_avg, False)[0].backward()
    assert (logits.grad.double() - x64.grad).abs().max() <= 1e-6
    sample["ntokens"] = 77                                                          # the sample's own count wins
    assert crit(model, sample)[2]["ntokens"] == 77


def test_criterion_eval_counts_and_indices():
    from unispeech_amd.ctc import CtcCriterion, LetterDictionary
    d = LetterDictionary(["|", "A", "B", "C"])                   # | = 4, A = 5, B = 6, C = 7; blank = <s> = 0
    assert (len(d), d.bos(), d.pad(), d.eos()) == (8, 0, 1, 2) and d.string([5, 6, 4, 7]) == "A B | C"
    crit = CtcCriterion(d, zero_infinity=True)
    assert (crit.blank_idx, crit.pad_idx, crit.eos_idx) == (0, 1, 2)

    class Task:
        target_dictionary = d
    assert CtcCriterion(Task()).blank_idx == 0
    # frames decode to "A B | C" and "A | | B" (a repeat, blanks between)
    paths = [[5, 5, 0, 6, 4, 4, 7, 0], [5, 0, 4, 0, 4, 6, 6, 0]]
    logits = torch.full((8, 2, 8), -5.0)
    for b, path in enumerate(paths):
        for t, c in enumerate(path):
            logits[t, b, c] = 5.0
    target = torch.tensor([[5, 6, 4, 7, 2], [5, 4, 6, 2, 1]])   # "AB C" and "A B": sample 1 has one letter too many
    sample = {"id": torch.arange(2), "target": target, "net_input": {"source": None}}
    model = _Stub(logits).eval()
    _, _, log = crit(model, sample)
    assert (log["c_errors"], log["c_total"]) == (1, 7)
    assert (log["w_errors"], log["w_total"], log["wv_errors"]) == (0, 4, 0)
    assert crit.logging_outputs_can_be_summed() is True
    out = CtcCriterion.reduce_metrics([log, log])
    assert out["ntokens"] == 14 and abs(out["uer"] - 100.0 / 7) < 1e-9 and out["wer"] == 0.0 and out["raw_wer"] == 0.0
    model.train()
    assert "c_errors" not in crit(model, sample)[2]


def test_criterion_refusals():
    from unispeech_amd.ctc import CtcCriterion
    for name in ("wer_kenlm_model", "wer_lexicon", "wer_args"):
        with pytest.raises(NotImplementedError, match=name):
            CtcCriterion(blank_idx=0, pad_idx=1, eos_idx=2, **{name: "x"})
    with pytest.raises(NotImplementedError, match="post_process"):
        CtcCriterion(blank_idx=0, pad_idx=1, eos_idx=2, post_process="wordpiece")
    with pytest.raises(ValueError, match="dictionary"):
        CtcCriterion()
    crit = CtcCriterion(blank_idx=0, pad_idx=1, eos_idx=2)
    with pytest.raises(NotImplementedError, match="reduce=False"):
        crit.get_loss(None, None, None, reduce=False)


# ---------------------------------------------------------------------------------------------- edit distance, greedy decode
def test_edit_distance_hand_counted():
    from unispeech_amd.ctc import edit_distance
    assert edit_distance([], []) == 0
    assert edit_distance([1, 2, 3], []) == 3 and edit_distance([], [1, 2]) == 2
    assert edit_distance([1, 2, 3], [1, 2, 3]) == 0
    assert edit_distance([1, 2, 3], [1, 3]) == 1                     # one deletion
    assert edit_distance([1, 2, 3], [1, 4, 3]) == 1                  # one substitution
    assert edit_distance("kitten", "sitting") == 3
    assert edit_distance("the cat sat".split(), "the cat sat down".split()) == 1
    assert edit_distance([1, 2, 3, 4], [4, 3, 2, 1]) == 4
    assert edit_distance("abc", "cab") == 2


def test_greedy_decode_host_path():
    from unispeech_amd.ctc import greedy_decode, post_process
    #            t:  0        1        2        3        4        5        6
    rows = [[0, 9, 1], [0, 9, 9], [9, 0, 0], [0, 9, 0], [3, 3, 3], [0, 0, 9], [0, 0, 9]]
    lat = torch.tensor(rows, dtype=torch.float32).view(7, 1, 3)
    # argmax: 1, 1 (tie of classes 1 and 2 -> the lower), 0, 1, 0 (three-way tie), 2, 2
    assert greedy_decode(lat, [7], 0) == [[1, 1, 2]]                 # the blank between them keeps both 1s
    assert greedy_decode(lat, [2], 0) == [[1]] and greedy_decode(lat, [0], 0) == [[]]
    assert greedy_decode(lat, None, 1) == [[0, 0, 2]]                # another blank: the 0s are separated by the 1 at t = 3
    assert greedy_decode(lat, [99], 2) == [[1, 0, 1, 0]]             # lengths are clamped to T
    assert post_process("H E L L O | W O R L D |", "letter") == "HELLO WORLD"
    assert post_process("A B", None) == "A B"


# ------------------------------------------------------------------------------------------------------------ EncoderCtc
def _tiny_w2v():
    from unispeech_amd.pretrain import WavLMPretrainConfig, WavLMPretrainModel
    cfg = WavLMPretrainConfig(**{k: v for k, v in TINY.items() if k in WavLMPretrainConfig.__dataclass_fields__})
    return cfg, WavLMPretrainModel(cfg, None, [range(23)])


def test_encoder_ctc_key_set_and_head():
    from unispeech_amd.ctc import EncoderCtc
    cfg, w2v = _tiny_w2v()
    with pytest.raises(ValueError, match="remove_pretraining_modules"):
        EncoderCtc(w2v, 12)
    w2v.remove_pretraining_modules()
    inner = set(w2v.state_dict())
    assert inner and not any(k.startswith(("final_proj", "label_embs")) for k in inner)
    m = EncoderCtc(w2v, 12, final_dropout=0.1, freeze_finetune_updates=3)
    want = {"w2v_encoder.w2v_model." + k for k in inner} | {"w2v_encoder.proj.weight", "w2v_encoder.proj.bias"}
    assert set(m.state_dict()) == want
    proj = m.w2v_encoder.proj
    assert proj.weight.shape == (12, cfg.encoder_embed_dim) and (proj.bias == 0).all()
    bound = (6.0 / (12 + cfg.encoder_embed_dim)) ** 0.5                  # xavier_uniform_
    assert proj.weight.abs().max() <= bound and proj.weight.abs().max() > 0.5 * bound
    assert m.w2v_encoder.w2v_model.feature_grad_mult == 0.0            # HubertAsrConfig's default, not the pre-training one
    m.set_num_updates(5)
    assert m.w2v_encoder.num_updates == 5 and w2v.num_updates == 5
    # get_logits leaves padded frames alone, as the reference's assignment into a masked copy does
    x = torch.randn(4, 2, 12)
    pm = torch.zeros(2, 4, dtype=torch.bool)
    pm[1, 2:] = True
    net = {"encoder_out": x.clone(), "encoder_padding_mask": pm, "padding_mask": pm}
    assert torch.equal(m.get_logits(net), x)
    assert torch.allclose(m.get_normalized_probs(net, True).exp().sum(-1), torch.ones(4, 2))
    # the wav2vec 2.0 encoder under the same wrapper, through build() with an override
    from unispeech_amd.wav2vec2 import Wav2Vec2Config
    wcfg = Wav2Vec2Config(**{k: v for k, v in TINY.items() if k in Wav2Vec2Config.__dataclass_fields__})
    m2 = EncoderCtc.build(wcfg, 7, arch="wav2vec2", mask_prob=0.3, layerdrop=0.0, apply_mask=True)
    keys = set(m2.state_dict())
    assert {"w2v_encoder.proj.weight", "w2v_encoder.proj.bias"} <= keys
    assert all(k.startswith(("w2v_encoder.w2v_model.", "w2v_encoder.proj.")) for k in keys)
    assert m2.w2v_encoder.w2v_model.mask_prob == 0.3 and m2.w2v_encoder.apply_mask
    assert not any("final_proj" in k or "quantizer" in k or "project_q" in k for k in keys)


def test_encoder_ctc_refused_options_raise_with_their_names():
    from unispeech_amd.ctc import EncoderCtc
    _, w2v = _tiny_w2v()
    w2v.remove_pretraining_modules()
    for name, value in (("no_pretrained_weights", True), ("normalize", True), ("decoder_layers", 2), ("w2v_args", {"x": 1}),
                        ("share_decoder_input_output_embed", True)):
        with pytest.raises(NotImplementedError, match=name):
            EncoderCtc(w2v, 12, **{name: value})
    EncoderCtc(w2v, 12, normalize=False, decoder_layers=6, w2v_args=None)           # defaults pass
    with pytest.raises(ValueError, match="mask_prob"):
        EncoderCtc(w2v, 12, mask_prob=0.3)                                          # a field of the wrapped config: build()
    with pytest.raises(TypeError, match="no_such_option"):
        EncoderCtc(w2v, 12, no_such_option=1)


# ------------------------------------------------------------------------------------------------------------------- ABI
def test_abi_30_and_the_new_symbols():
    from unispeech_amd import _lib, build
    src = open(os.path.join(ROOT, "include", "wavlm_hip.h")).read()
    assert int(re.search(r"#define WAVLM_HIP_ABI_VERSION (\d+)", src).group(1)) == 30 == _lib.ABI_VERSION
    assert "ctc.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "ctc.hip"))
    for name in ("wavlm_ctc_supported", "wavlm_ctc_workspace_bytes", "wavlm_ctc_loss", "wavlm_ctc_greedy"):
        assert re.search(r"\b%s\(" % name, src), name
        assert name in _lib.SIGNATURES
    # argument counts of the binding against the header's declarations
    for name in ("wavlm_ctc_loss", "wavlm_ctc_greedy", "wavlm_ctc_workspace_bytes", "wavlm_ctc_supported"):
        decl = re.search(r"\b%s\(([^;]*)\);" % name, src).group(1)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[name][1]), name
    L = _lib.lib()                                   # loading needs no GPU; neither do the two host functions
    assert L.wavlm_abi_version() == 30
    assert L.wavlm_ctc_supported(1024, 1023) == 1 and L.wavlm_ctc_supported(32, 0) == 1
    assert L.wavlm_ctc_supported(1025, 10) == 0 and L.wavlm_ctc_supported(32, 1024) == 0 and L.wavlm_ctc_supported(0, 1) == 0
    B, T, Lm = 32, 749, 250
    assert L.wavlm_ctc_workspace_bytes(B, T, Lm) >= B * T * (2 * Lm + 1) * 4 + B * T * 8 + B * 8
    assert L.wavlm_ctc_workspace_bytes(B, T, Lm) < B * T * (2 * Lm + 1) * 4 + B * T * 8 + B * 8 + 3 * 256


def test_cli_arguments():
    from unispeech_amd import ctc
    a = ctc.parse_args(["decode", "ck.pt", "dict.ltr.txt", "a.wav", "b.wav"])
    assert (a.cmd, a.ckpt, a.dict, a.wavs, a.post_process, a.bf16) == ("decode", "ck.pt", "dict.ltr.txt", ["a.wav", "b.wav"],
                                                                         "letter", False)
    with pytest.raises(SystemExit):
        ctc.parse_args(["decode", "ck.pt", "dict.ltr.txt"])
