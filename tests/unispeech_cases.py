"""What tests/test_unispeech.py and tests/test_unispeech_gpu.py share: the configurations of the three goldens written by
tools/gen_unispeech_golden.py, the dictionary and the sample."""
import torch

from conftest import golden_state_dict, load_golden

SYMBOLS = ["|", "A", "B", "C", "D", "E", "F", "G"]                     # + <s> <pad> </s> <unk> = 12 classes
# golden -> (config overrides on top of test_oracle_vs_golden.W2V2 + transpose, mtlalpha)
UNISPEECH_GOLDENS = {
    "tiny_unispeech.npz": (dict(negatives_from_everywhere=True, cross_sample_negatives=0, replace_prob=0.5), 0.5),
    "tiny_unispeech_local.npz": (dict(negatives_from_everywhere=False, cross_sample_negatives=3, replace_prob=0.3), 0.2),
}


def w2v2_fields(**overrides):
    from test_oracle_vs_golden import W2V2
    from unispeech_amd.unispeech import UniSpeechConfig
    d = dict(W2V2)
    d.update(overrides)
    return {k: v for k, v in d.items() if k in UniSpeechConfig.__dataclass_fields__}


def unispeech_config(golden, **more):
    from unispeech_amd.unispeech import UniSpeechConfig
    over, alpha = UNISPEECH_GOLDENS[golden]
    fields = dict(over, transpose=True, final_dropout=0.0)
    fields.update(more)
    return UniSpeechConfig(**w2v2_fields(**fields)), alpha


def dictionary():
    from unispeech_amd.ctc import LetterDictionary
    return LetterDictionary(SYMBOLS)


def build(golden, device="cpu", dtype=torch.float32, **more):
    """(model with the golden's weights, criterion, golden)"""
    from unispeech_amd.unispeech import Unispeech, UnispeechCriterion
    z = load_golden(golden)
    cfg, alpha = unispeech_config(golden, **more)
    m = Unispeech(cfg, dictionary())
    m.load_state_dict(golden_state_dict(z), strict=True)
    m = m.to(device).to(dtype)
    m.w2v_encoder.w2v_model.quantizer.gumbel_noise = "host"
    crit = UnispeechCriterion(dictionary(), mtlalpha=alpha, infonce=True, loss_weights=[float(v) for v in z["in/loss_weights"]])
    return m, crit, z


def sample_of(z, device="cpu", dtype=torch.float32):
    pm = torch.zeros(3, 16000, dtype=torch.bool)
    tl = torch.from_numpy(z["in/target_lengths"])
    return {"id": torch.arange(3), "target": torch.from_numpy(z["in/target"]), "target_lengths": tl, "ntokens": int(tl.sum()),
            "net_input": {"source": torch.from_numpy(z["in/source"]).to(device).to(dtype), "padding_mask": pm.to(device),
                          "padding_mask_cpu": pm}}
