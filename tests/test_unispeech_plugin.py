"""The UniSpeech model and criterion register through the reference's own fairseq decorators, and a checkpoint of the multitask
model is fine-tuned through the CTC model names.  Needs the reference tree for fairseq's registries and is skipped where that is
absent, like tests/test_ctc_plugin.py."""
import dataclasses
from types import SimpleNamespace

import pytest
import torch

from oracle import ref_shim
from unispeech_cases import dictionary, unispeech_config

pytestmark = pytest.mark.skipif(not ref_shim.available(), reason="reference tree not present")

OLD_MODELS = ("wavlm_mi355x", "hubert_mi355x", "unispeech_sat_mi355x", "ils_hubert_mi355x", "wav2vec2_mi355x", "hubert_ctc_mi355x",
              "wav2vec_ctc_mi355x")
OLD_CRITERIA = ("wavlm_mi355x", "hubert_mi355x", "wav2vec_mi355x", "ctc_mi355x")


def test_unispeech_names_register_and_old_ones_stay():
    ref_shim.fairseq_wavlm()
    from fairseq.criterions import CRITERION_DATACLASS_REGISTRY, CRITERION_REGISTRY, FairseqCriterion
    from fairseq.models import MODEL_DATACLASS_REGISTRY, MODEL_REGISTRY, BaseFairseqModel
    from unispeech_amd import fairseq_plugin, unispeech
    fairseq_plugin.register()
    models = {k: MODEL_REGISTRY[k] for k in OLD_MODELS}
    criteria = {k: CRITERION_REGISTRY[k] for k in OLD_CRITERIA}
    fairseq_plugin.register()                                                       # a second call changes nothing
    assert all(MODEL_REGISTRY[k] is v for k, v in models.items()) and all(CRITERION_REGISTRY[k] is v for k, v in criteria.items())
    M, C = MODEL_REGISTRY["unispeech_mi355x"], CRITERION_REGISTRY["unispeech_criterion_mi355x"]
    assert issubclass(M, unispeech.Unispeech) and issubclass(M, BaseFairseqModel)
    assert issubclass(C, unispeech.UnispeechCriterion) and issubclass(C, FairseqCriterion)
    # the model's dataclass: the wav2vec2_mi355x fields plus the two new ones, the reference's defaults
    mf = {f.name: f for f in dataclasses.fields(MODEL_DATACLASS_REGISTRY["unispeech_mi355x"])}
    wf = {f.name for f in dataclasses.fields(MODEL_DATACLASS_REGISTRY["wav2vec2_mi355x"])}
    assert set(mf) == wf | {"replace_prob", "final_dropout"}
    assert (mf["replace_prob"].default, mf["final_dropout"].default, mf["transpose"].default) == (0.5, 0.1, False)
    cf = {f.name: f for f in dataclasses.fields(CRITERION_DATACLASS_REGISTRY["unispeech_criterion_mi355x"])}
    both = {f.name for k in ("wav2vec_mi355x", "ctc_mi355x") for f in dataclasses.fields(CRITERION_DATACLASS_REGISTRY[k])}
    assert set(cf) == both | {"mtlalpha"} and cf["mtlalpha"].default == 0.5 and cf["post_process"].default == "letter"
    # build through the registered classes
    cfg, _ = unispeech_config("tiny_unispeech.npz")
    task = SimpleNamespace(target_dictionary=dictionary())
    torch.manual_seed(0)
    m = M.build_model(cfg, task)
    assert m.w2v_encoder.proj.weight.shape == (12, 64) and m.w2v_encoder.replace_prob == 0.5
    assert all(k.startswith(("w2v_encoder.w2v_model.", "w2v_encoder.proj.")) for k in m.state_dict())
    ccfg = SimpleNamespace(mtlalpha=0.3, infonce=True, loss_weights=[0.1, 10.0], log_keys=[], zero_infinity=True, sentence_avg=False,
                           post_process="letter", wer_kenlm_model=None, wer_lexicon=None, wer_args=None)
    c = C(ccfg, task)
    assert c.mtlalpha == 0.3 and c.ctc_criterion.zero_infinity and c.ctc_criterion.blank_idx == 0 and c.w2v_criterion.infonce
    assert c.w2v_criterion.loss_weights == [0.1, 10.0] and c.task is task and not C.logging_outputs_can_be_summed()
    ccfg.wer_lexicon = "lexicon.txt"
    with pytest.raises(NotImplementedError, match="wer_lexicon"):
        C(ccfg, task)


def test_unispeech_override_names_are_saved_and_restored():
    ref_shim.fairseq_wavlm()
    from fairseq.criterions import CRITERION_DATACLASS_REGISTRY, CRITERION_REGISTRY
    from fairseq.models import (ARCH_CONFIG_REGISTRY, ARCH_MODEL_NAME_REGISTRY, ARCH_MODEL_REGISTRY, MODEL_DATACLASS_REGISTRY,
                                MODEL_REGISTRY)
    from unispeech_amd import fairseq_plugin, unispeech
    fairseq_plugin.register()
    regs = (MODEL_REGISTRY, ARCH_MODEL_REGISTRY, ARCH_MODEL_NAME_REGISTRY, MODEL_DATACLASS_REGISTRY, ARCH_CONFIG_REGISTRY,
            CRITERION_REGISTRY, CRITERION_DATACLASS_REGISTRY)
    saved = [dict(r) for r in regs]
    assert "unispeech" in saved[0] and "unispeech_criterion" in saved[5]           # the reference's own are there to replace
    try:
        fairseq_plugin.register(override=True)
        assert issubclass(MODEL_REGISTRY["unispeech"], unispeech.Unispeech)
        assert MODEL_REGISTRY["unispeech"] is ARCH_MODEL_REGISTRY["unispeech"] is MODEL_REGISTRY["unispeech_mi355x"]
        assert MODEL_DATACLASS_REGISTRY["unispeech"] is MODEL_DATACLASS_REGISTRY["unispeech_mi355x"]
        assert issubclass(CRITERION_REGISTRY["unispeech_criterion"], unispeech.UnispeechCriterion)
        assert CRITERION_DATACLASS_REGISTRY["unispeech_criterion"] is CRITERION_DATACLASS_REGISTRY["unispeech_criterion_mi355x"]
    finally:
        fairseq_plugin.unregister_override()
        for r, s in zip(regs, saved):
            r.clear()
            r.update(s)
    assert not issubclass(MODEL_REGISTRY["unispeech"], unispeech.Unispeech)
    assert not issubclass(CRITERION_REGISTRY["unispeech_criterion"], unispeech.UnispeechCriterion)


@pytest.mark.parametrize("name", ["hubert_ctc_mi355x", "wav2vec_ctc_mi355x"])
def test_fine_tuning_builds_from_a_unispeech_checkpoint(tmp_path, name):
    ref_shim.fairseq_wavlm()
    from fairseq.models import MODEL_REGISTRY
    from unispeech_amd import fairseq_plugin
    from unispeech_amd.unispeech import Unispeech
    fairseq_plugin.register()
    cfg, _ = unispeech_config("tiny_unispeech.npz")
    torch.manual_seed(0)
    pre = Unispeech(cfg, 12)
    path = str(tmp_path / "unispeech.pt")
    torch.save({"cfg": {"model": dict(dataclasses.asdict(cfg), _name="unispeech"), "task": {"normalize": False}},
                "model": pre.state_dict()}, path)
    d = dictionary()
    mcfg = SimpleNamespace(w2v_path=path, normalize=False, mask_prob=0.4, final_dropout=0.1)
    m = MODEL_REGISTRY[name].build_model(mcfg, SimpleNamespace(target_dictionary=d))
    enc = m.w2v_encoder
    assert enc.proj.weight.shape == (12, 64) and enc.w2v_model.mask_prob == 0.4
    assert not torch.equal(enc.proj.weight, pre.w2v_encoder.proj.weight)           # the pre-training head is dropped
    assert enc.w2v_model.quantizer is None and enc.w2v_model.final_proj is None
    ref = pre.w2v_encoder.w2v_model.state_dict()
    inner = enc.w2v_model.state_dict()
    assert inner and all(torch.equal(v, ref[k]) for k, v in inner.items())          # the inner weights are loaded
    assert all(k.startswith(("w2v_encoder.w2v_model.", "w2v_encoder.proj.")) for k in m.state_dict())
