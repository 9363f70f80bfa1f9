"""Shared by tests/test_transformer_lm.py, tests/test_transformer_lm_gpu.py and tools/gen_transformer_lm_golden.py: the three
tiny models of tests/golden/transformer_lm.npz, the formula that fills their weights (none are stored: the reference's state
dict and this package's have the same keys and shapes, so both sides fill from the same seed), the sentences, and the rescoring
case.

  A  pre-LN + final norm, sinusoidal positions, ReLU, D 64, 2 heads (32 wide), FFN 128, 2 layers
  B  post-LN, GELU, learned positions, shared input / output embedding, layernorm_embedding, no_scale_embedding, 1 head (64 wide)
  C  adaptive input (cut-offs 20, 40, factor 4), decoder_input_dim 32, decoder_output_dim 32 (project_out_dim)
The dictionary has 100 entries: <s> <pad> </s> <unk> = 0 .. 3, then 96 words."""
import functools

import numpy as np
import torch

VOCAB, PAD, EOS, UNK = 100, 1, 2, 3
_BASE = dict(decoder_embed_dim=64, decoder_ffn_embed_dim=128, decoder_layers=2, decoder_attention_heads=2,
             max_target_positions=64)
MODELS = {
    "A": dict(_BASE, decoder_normalize_before=True, activation_fn="relu"),
    "B": dict(_BASE, decoder_attention_heads=1, decoder_normalize_before=False, activation_fn="gelu", decoder_learned_pos=True,
              share_decoder_input_output_embed=True, layernorm_embedding=True, no_scale_embedding=True),
    "C": dict(_BASE, decoder_normalize_before=True, activation_fn="relu", adaptive_input=True, adaptive_input_cutoff="20,40",
              adaptive_input_factor=4, decoder_input_dim=32, decoder_output_dim=32),
}
SEEDS = {"A": 11, "B": 12, "C": 13}
GAIN = 1.0
NOT_WEIGHTS = ("version", "_float_tensor")


def fill_state_dict(sd, seed, shared=False):
    """{name: fp32 tensor} for the floating-point weights of `sd`, drawn in sorted-key order from
    numpy.random.default_rng(seed): a 1-D `.weight` (LayerNorm) is 1 + 0.1 N, another vector 0.1 N, a matrix GAIN * N / sqrt(its
    row length).  `version` and `_float_tensor` buffers are left out (load with strict=False).  shared: the output projection is
    the input embedding."""
    rng = np.random.default_rng(seed)
    out = {}
    for k in sorted(sd):
        if k.rsplit(".", 1)[-1] in NOT_WEIGHTS:
            continue
        shape = tuple(sd[k].shape)
        z = rng.standard_normal(int(np.prod(shape)))
        if len(shape) == 1:
            a = 1.0 + 0.1 * z if k.endswith(".weight") else 0.1 * z
        else:
            a = GAIN * z / np.sqrt(float(shape[-1]))
        out[k] = torch.from_numpy(a.reshape(shape).astype(np.float32))
    if shared:
        out["decoder.output_projection.weight"] = out["decoder.embed_tokens.weight"]
    return out


@functools.lru_cache(maxsize=None)
def sentences():
    """lengths 0, 1, 7 and 33; the one of 7 holds unk; the words cover the three bands of model C"""
    rng = np.random.default_rng(5)
    out = [[int(v) for v in rng.integers(4, VOCAB, n)] for n in (0, 1, 7, 33)]
    out[2][3] = UNK
    out[3][0], out[3][1], out[3][2] = 5, 25, 77
    return out


def build(name, dtype=torch.float32, device=None):
    """this package's model `name` with the filled weights -- built anew at every call"""
    from unispeech_amd.transformer_lm import TransformerLM
    m = TransformerLM(dict(MODELS[name]), VOCAB, pad=PAD, eos=EOS, unk=UNK)
    m.load_state_dict(fill_state_dict(m.state_dict(), SEEDS[name], MODELS[name].get("share_decoder_input_output_embed", False)),
                      strict=False)
    if device is not None:
        m = m.to(device)
    return m.to(dtype)


# ---------------------------------------------------------------------------------------------------------- rescoring
RESCORE_CASE = "beam63"                # tests/ctc_lexicon_cases.py: T 12, B 2, C 12, trigram word LM, lexicon `mid`
RESCORE_NBEST = 8
RESCORE_OPTS = dict(rescore_weight=0.5, rescore_word_score=0.5)
UNKNOWN_TO_LM = ("oov", "x7")          # words of the lexicon the Transformer LM's dictionary does not list


@functools.lru_cache(maxsize=None)
def rescoring():
    """(emissions, input lengths, dictionary, Lexicon, first-pass options with nbest = RESCORE_NBEST, the LM's dictionary)"""
    import ctc_lexicon_cases as L
    from unispeech_amd.ctc import LetterDictionary
    x, il, d, lexicon, opts = L.case(RESCORE_CASE)
    opts = dict(opts, nbest=RESCORE_NBEST)
    words = [w for w in lexicon.words if w != "<unk>" and w not in UNKNOWN_TO_LM]
    assert len(words) <= VOCAB - 4
    lm_dict = LetterDictionary(words + ["filler%d" % i for i in range(VOCAB - 4 - len(words))])
    assert len(lm_dict) == VOCAB
    return x, il, d, lexicon, opts, lm_dict
