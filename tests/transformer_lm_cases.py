"""Shared by tests/test_transformer_lm.py, tests/test_transformer_lm_gpu.py and tools/gen_transformer_lm_golden.py: the three
tiny models of tests/golden/transformer_lm.npz, the formula that fills their weights (none are stored: the reference's state
dict and this package's have the same keys and shapes, so both sides fill from the same seed), the sentences, and the rescoring
case.

  A  pre-LN + final norm, sinusoidal positions, ReLU, D 64, 2 heads (32 wide), FFN 128, 2 layers
  B  post-LN, GELU, learned positions, shared input / output embedding, layernorm_embedding, no_scale_embedding, 1 head (64 wide)
  C  adaptive input (cut-offs 20, 40, factor 4), decoder_input_dim 32, decoder_output_dim 32 (project_out_dim)
The dictionary has 100 entries: <s> <pad> </s> <unk> = 0 .. 3, then 96 words.

Further down: models W and X at production width (tests/golden/transformer_lm_wide.npz) and the seeded builders of the kernel
cases whose properties tests/test_transformer_lm.py asserts on the CPU and tests/test_transformer_lm_gpu.py runs on the device."""
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


# --------------------------------------------------------------------------------------------- models at production width
# tests/golden/transformer_lm_wide.npz (tools/gen_transformer_lm_golden.py --wide).  Widths at which ops.gemm picks the 256-wide
# ping-pong kernels (N >= 256 with 256 rows or more), sentences whose T crosses the 128-query block of the attention, and a
# vocabulary of three slabs of wavlm_lm_logprob with a ragged last one (5003 = 2 x 2048 + 907).
#   W  pre-LN + final norm, ReLU, sinusoidal positions, D 512, 8 heads (64 wide), FFN 2048, 2 layers
#   X  post-LN, GELU, learned positions, D 256, 8 heads (32 wide), FFN 1024, 2 layers
WIDE_VOCAB = 5003
WIDE_MODELS = {
    "W": dict(decoder_embed_dim=512, decoder_ffn_embed_dim=2048, decoder_layers=2, decoder_attention_heads=8,
              max_target_positions=256, decoder_normalize_before=True, activation_fn="relu"),
    "X": dict(decoder_embed_dim=256, decoder_ffn_embed_dim=1024, decoder_layers=2, decoder_attention_heads=8,
              max_target_positions=256, decoder_normalize_before=False, activation_fn="gelu", decoder_learned_pos=True),
}
WIDE_SEEDS = {"W": 21, "X": 22}
WIDE_LENGTHS = (0, 1, 126, 127, 128, 200)          # words; T = words + 1 = 1, 2, 127, 128, 129, 201
WIDE_UNK_AT = (2, 60)                              # (sentence, word) that holds unk


@functools.lru_cache(maxsize=None)
def wide_sentences():
    rng = np.random.default_rng(6)
    out = [[int(v) for v in rng.integers(4, WIDE_VOCAB, n)] for n in WIDE_LENGTHS]
    out[WIDE_UNK_AT[0]][WIDE_UNK_AT[1]] = UNK
    out[5][0], out[5][1], out[5][2] = 4, 2048, WIDE_VOCAB - 1           # the first word, a slab's first entry, the last entry
    return out


def build_wide(name, dtype=torch.float32, device=None):
    """this package's model W or X with the filled weights -- built anew at every call"""
    from unispeech_amd.transformer_lm import TransformerLM
    m = TransformerLM(dict(WIDE_MODELS[name]), WIDE_VOCAB, pad=PAD, eos=EOS, unk=UNK)
    m.load_state_dict(fill_state_dict(m.state_dict(), WIDE_SEEDS[name]), strict=False)
    if device is not None:
        m = m.to(device)
    return m.to(dtype)


# ------------------------------------------------------------------------------------------ wavlm_lm_logprob: built cases
LM_SLAB, LM_TILE = 2048, 128                      # csrc/lm.hip: LM_SLAB, LM_BN


def bf16_valued(t):
    return t.to(torch.bfloat16).float()


def logprob_reference(X, W, tgt):
    """float64 (z [R, V], lse [R], logprob [R]) of fp32 tensors X [R, D], W [V, D] and int32 targets: 0 for a negative target,
    NaN for one >= V"""
    R, V = X.shape[0], W.shape[0]
    z = X.double().numpy() @ W.double().numpy().T
    m = z.max(1)
    lse = m + np.log(np.exp(z - m[:, None]).sum(1))
    t = tgt.numpy()
    ok = (t >= 0) & (t < V)
    lp = np.where(ok, z[np.arange(R), np.clip(t, 0, V - 1)] - lse, np.where(t < 0, 0.0, np.nan))
    return z, lse, lp


def slot_targets(R=256, V=2051):
    """row r < 128 targets entry 1920 + r (the last tile of slab 0); row r >= 128 targets entry 2048 + (r - 128) while slab 1
    holds it and 1792 + (r - 128) beyond: each block of 128 rows has a target at every one of the 128 positions of a tile, so
    every accumulator register acc[j][i] of either half-wave holds some row's target"""
    r = torch.arange(R, dtype=torch.int32)
    second = torch.where(2048 + (r - 128) <= V - 1, 2048 + (r - 128), 1792 + (r - 128))
    return torch.where(r < 128, 1920 + r, second).to(torch.int32)


@functools.lru_cache(maxsize=None)
def slot_case():
    """(X, W, targets, z, lse, logprob): R 256, V 2051, D 32 with slot_targets"""
    g = torch.Generator().manual_seed(256205132)
    X = bf16_valued(torch.randn(256, 32, generator=g))
    W = bf16_valued(torch.randn(2051, 32, generator=g))
    tgt = slot_targets()
    return (X, W, tgt) + logprob_reference(X, W, tgt)


STAIR_V, STAIR_D, STAIR_C = 6200, 16, (2.0, -2.0, 1.0, -1.0, 0.0)


@functools.lru_cache(maxsize=None)
def staircase_case():
    """(X, W, targets, z, lse, logprob): the logits of row c rise (c > 0) or fall (c < 0) by c / 4 from one 128-entry tile to the
    next, so the running maximum of the online softmax is renewed at almost every tile and the mass gathered so far is never
    negligible: channel 0 of W[v] is (v // 128) / 4 and of X[r] is STAIR_C[r]; the other channels are N(0, 1) in X and
    0.25 N(0, 1) in W.  Every value is exact in bf16."""
    g = torch.Generator().manual_seed(7)
    X = torch.randn(len(STAIR_C), STAIR_D, generator=g)
    W = 0.25 * torch.randn(STAIR_V, STAIR_D, generator=g)
    X[:, 0] = torch.tensor(STAIR_C)
    W[:, 0] = (torch.arange(STAIR_V) // LM_TILE).float() / 4
    X, W = bf16_valued(X), bf16_valued(W)
    assert torch.equal(W[:, 0], (torch.arange(STAIR_V) // LM_TILE).float() / 4)
    tgt = torch.tensor([STAIR_V - 1, 0, 2048, 4095, 6143], dtype=torch.int32)
    return (X, W, tgt) + logprob_reference(X, W, tgt)


def staircase_profile(z_row):
    """of one row of float64 logits: (tiles, tiles whose maximum exceeds every earlier tile's, the largest share of the row's
    mass in one tile, the share of each slab)"""
    V = z_row.shape[0]
    p = np.exp(z_row - z_row.max())
    p /= p.sum()
    edges = list(range(0, V, LM_TILE))
    tmax = np.array([z_row[a:a + LM_TILE].max() for a in edges])
    renew = 1 + int((tmax[1:] > np.maximum.accumulate(tmax)[:-1]).sum())
    share = max(p[a:a + LM_TILE].sum() for a in edges)
    slabs = [p[a:a + LM_SLAB].sum() for a in range(0, V, LM_SLAB)]
    return len(edges), renew, share, slabs


# --------------------------------------------------------------------------------------- wavlm_attn_causal_fwd: built cases
LONG_LENGTHS = (300, 257, 256, 129, 128, 97, 64, 0)


def long_causal_qkv(d, H=3, T=300):
    """bf16-valued packed q|k|v [8, T, 3 H d] of the long case (lengths LONG_LENGTHS)"""
    g = torch.Generator().manual_seed(3000 + d)
    qkv = torch.randn(len(LONG_LENGTHS), T, 3 * H * d, generator=g)
    qkv[..., :H * d] *= 1.5
    qkv[..., 2 * H * d:] += 0.5
    return bf16_valued(qkv)


RISING_B, RISING_H, RISING_T, RISING_STEP = 2, 4, 300, 32


def rising_constant(d):
    """Q's channel 0 in the rising heads: a score then grows by constant / (4 sqrt(d)) = 0.5 per 32-key step (exact in bf16 for
    d = 64, rounded to bf16 for d = 32).  Under the other channels a score's noise has standard deviation 0.125, so the maximum
    of a last step that holds a few keys only is about 0.25 below that of a full step: 0.5 still renews it, and nearly every
    step renews the maximum.  A full step holds about 1 - exp(-0.5) = 0.39 of the mass at and below it: no step holds half."""
    return float(bf16_valued(torch.tensor(2.0 * d ** 0.5)))


def rising_heads():
    return [h for h in range(RISING_H) if h % 2 == 0]


def rising_causal_qkv(d):
    """bf16-valued packed q|k|v [2, 300, 3 * 4 * d]: K's channel 0 is (key // 32) / 4 in every head; Q's channel 0 is
    rising_constant(d) in heads 0 and 2 and its negative in heads 1 and 3; the other channels of Q are 0.125 N(0, 1), of K
    N(0, 1); V is N(0, 1) + 0.5"""
    g = torch.Generator().manual_seed(4000 + d)
    B, H, T = RISING_B, RISING_H, RISING_T
    qkv = torch.randn(B, T, 3, H, d, generator=g)
    qkv[:, :, 0] *= 0.125
    qkv[:, :, 2] += 0.5
    c = rising_constant(d)
    for h in range(H):
        qkv[:, :, 0, h, 0] = c if h % 2 == 0 else -c
    qkv[:, :, 1, :, 0] = ((torch.arange(T) // RISING_STEP).float() / 4).view(1, T, 1)
    return bf16_valued(qkv.reshape(B, T, 3 * H * d))


def rising_profile(qkv, d):
    """float64 causal scores of the rising heads' queries >= 128: (the smallest fraction of a query's 32-key steps whose maximum
    exceeds every earlier step's, the largest share of a query's mass in one step)"""
    B, T, _ = qkv.shape
    H = RISING_H
    x = qkv.double().numpy().reshape(B, T, 3, H, d)
    worst_renew, worst_share = 1.0, 0.0
    for b in range(B):
        for h in rising_heads():
            s = x[b, :, 0, h] @ x[b, :, 1, h].T / np.sqrt(d)
            for q in range(128, T):
                row = s[q, :q + 1]
                p = np.exp(row - row.max())
                p /= p.sum()
                edges = list(range(0, q + 1, RISING_STEP))
                smax = np.array([row[a:a + RISING_STEP].max() for a in edges])
                renew = 1 + int((smax[1:] > np.maximum.accumulate(smax)[:-1]).sum())
                worst_renew = min(worst_renew, renew / len(edges))
                worst_share = max(worst_share, max(p[a:a + RISING_STEP].sum() for a in edges))
    return worst_renew, worst_share


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
