"""The CTC model and criterion register through the reference's own fairseq decorators and build from a checkpoint file.  Needs the
reference tree for fairseq's registries and is skipped where that is absent, like tests/test_fairseq_plugin.py."""
from types import SimpleNamespace

import pytest
import torch

from conftest import TINY
from oracle import ref_shim

pytestmark = pytest.mark.skipif(not ref_shim.available(), reason="reference tree not present")


def test_ctc_names_register_and_build(tmp_path):
    ref_shim.fairseq_wavlm()
    from fairseq.criterions import CRITERION_REGISTRY
    from fairseq.models import MODEL_REGISTRY, BaseFairseqModel
    from unispeech_amd import ctc, fairseq_plugin
    from unispeech_amd.pretrain import WavLMPretrainConfig, WavLMPretrainModel
    before = {k: MODEL_REGISTRY[k] for k in ("wavlm_mi355x", "hubert_mi355x", "wav2vec2_mi355x") if k in MODEL_REGISTRY}
    fairseq_plugin.register()
    for name in ("hubert_ctc_mi355x", "wav2vec_ctc_mi355x"):
        assert issubclass(MODEL_REGISTRY[name], ctc.EncoderCtc) and issubclass(MODEL_REGISTRY[name], BaseFairseqModel)
    assert issubclass(CRITERION_REGISTRY["ctc_mi355x"], ctc.CtcCriterion)
    assert all(MODEL_REGISTRY[k] is v for k, v in before.items())                 # the existing registrations are unchanged
    # build_model from a pre-training checkpoint file, with an override and the reference's key set
    cfg = WavLMPretrainConfig(**{k: v for k, v in TINY.items() if k in WavLMPretrainConfig.__dataclass_fields__})
    torch.manual_seed(0)
    pre = WavLMPretrainModel(cfg, None, [range(23)])
    path = str(tmp_path / "pre.pt")
    torch.save({"cfg": {"model": dict(TINY, _name="hubert"), "task": {"normalize": False}}, "model": pre.state_dict()}, path)
    d = ctc.LetterDictionary(["|", "A", "B"])
    mcfg = SimpleNamespace(w2v_path=path, normalize=False, mask_prob=0.4, freeze_finetune_updates=7, final_dropout=0.1)
    m = MODEL_REGISTRY["hubert_ctc_mi355x"].build_model(mcfg, SimpleNamespace(target_dictionary=d))
    enc = m.w2v_encoder
    assert enc.proj.weight.shape == (7, 64) and enc.freeze_finetune_updates == 7 and enc.w2v_model.mask_prob == 0.4
    assert torch.equal(enc.w2v_model.post_extract_proj.weight, pre.post_extract_proj.weight)     # pre-trained weights are loaded
    assert all(k.startswith(("w2v_encoder.w2v_model.", "w2v_encoder.proj.")) for k in m.state_dict())
    with pytest.raises(AssertionError, match="normalization"):
        MODEL_REGISTRY["hubert_ctc_mi355x"].build_model(SimpleNamespace(w2v_path=path, normalize=True),
                                                       SimpleNamespace(target_dictionary=d))
    crit = CRITERION_REGISTRY["ctc_mi355x"](SimpleNamespace(zero_infinity=True, sentence_avg=False, post_process="letter",
                                                            wer_kenlm_model=None, wer_lexicon=None, wer_args=None),
                                            SimpleNamespace(target_dictionary=d))
    assert (crit.blank_idx, crit.pad_idx, crit.eos_idx, crit.zero_infinity) == (0, 1, 2, True)
    with pytest.raises(NotImplementedError, match="wer_kenlm_model"):
        CRITERION_REGISTRY["ctc_mi355x"](SimpleNamespace(zero_infinity=True, sentence_avg=False, post_process="letter",
                                                         wer_kenlm_model="lm.bin", wer_lexicon=None, wer_args=None),
                                         SimpleNamespace(target_dictionary=d))


def test_ctc_override_names():
    ref_shim.fairseq_wavlm()
    from fairseq.criterions import CRITERION_DATACLASS_REGISTRY, CRITERION_REGISTRY
    from fairseq.models import (ARCH_CONFIG_REGISTRY, ARCH_MODEL_NAME_REGISTRY, ARCH_MODEL_REGISTRY, MODEL_DATACLASS_REGISTRY,
                                MODEL_REGISTRY)
    from unispeech_amd import ctc, fairseq_plugin
    fairseq_plugin.register()
    regs = (MODEL_REGISTRY, ARCH_MODEL_REGISTRY, ARCH_MODEL_NAME_REGISTRY, MODEL_DATACLASS_REGISTRY, ARCH_CONFIG_REGISTRY,
            CRITERION_REGISTRY, CRITERION_DATACLASS_REGISTRY)
    saved = [dict(r) for r in regs]
    try:
        fairseq_plugin.register(override=True)
        for name in ("hubert_ctc", "wav2vec_ctc"):
            if name in saved[0]:
                assert issubclass(MODEL_REGISTRY[name], ctc.EncoderCtc)
        if "ctc" in saved[5]:
            assert issubclass(CRITERION_REGISTRY["ctc"], ctc.CtcCriterion)
    finally:
        fairseq_plugin.unregister_override()
        for r, s in zip(regs, saved):
            r.clear()
            r.update(s)
