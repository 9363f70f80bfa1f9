"""Shared by tests/test_seq2seq.py, tests/test_seq2seq_gpu.py and tools/gen_seq2seq_golden.py: the two tiny seq2seq models of
tests/golden/seq2seq.npz, the formula that fills their decoders (no weights are stored: the reference's state dict and this
package's have the same keys and shapes, so both sides fill from the same seed; the encoder's weights are those of
tests/golden/tiny_w2v2.npz), the batch, and the seeded builders of the kernel cases.

  A  D 64 = 2 heads of 32, FFN 128, 2 layers, post-LN, sinusoidal positions, separate embed_out
  B  D 128 = 2 heads of 64, FFN 256, 2 layers, pre-LN + final norm, learned positions, shared input / output embedding
Both sit on the tiny wav2vec 2.0 encoder of tests/golden/tiny_w2v2.npz, which is 64 wide: B therefore has encoder.proj (64 -> 128)
and A, whose decoder is as wide as the encoder, has none -- either form of Wav2VecEncoder is covered once.
The dictionary has 12 entries: <s> <pad> </s> <unk> = 0 .. 3, then 8 letters."""
import functools
import math

import numpy as np
import torch

SYMBOLS = ["|", "A", "B", "C", "D", "E", "F", "G"]
VOCAB, PAD, EOS, UNK = 12, 1, 2, 3
MODELS = {
    "A": dict(decoder_embed_dim=64, decoder_ffn_embed_dim=128, decoder_layers=2, decoder_attention_heads=2,
              decoder_normalize_before=False, decoder_learned_pos=False, share_decoder_input_output_embed=False,
              max_target_positions=64),
    "B": dict(decoder_embed_dim=128, decoder_ffn_embed_dim=256, decoder_layers=2, decoder_attention_heads=2,
              decoder_normalize_before=True, decoder_learned_pos=True, share_decoder_input_output_embed=True,
              max_target_positions=64),
}
SEEDS = {"A": 55, "B": 47}          # chosen by tools/gen_seq2seq_golden.py's assertions: margins, early and late eos
GAIN = 1.5
NOT_WEIGHTS = ("version", "_float_tensor")
ENCODER_GOLDEN = "tiny_w2v2.npz"
WAVE_LENGTHS = (16000, 12000, 9040)
MAX_LEN_B = 12
BEAMS = (1, 5)
HEAD_TOL = 5e-4                        # the fp32-mode bound of a head, of the max magnitude (tests/test_diarization_gpu.py)


def fill_decoder(sd, seed):
    """{name: fp32 tensor} for the floating-point entries of `sd` outside encoder.w2v_model.*, drawn in sorted-key order from
    numpy.random.default_rng(seed): a 1-D `.weight` (LayerNorm) is 1 + 0.1 N, another vector 0.1 N, a matrix GAIN * N / sqrt(its
    row length)"""
    rng = np.random.default_rng(seed)
    out = {}
    for k in sorted(sd):
        if k.startswith("encoder.w2v_model.") or k.rsplit(".", 1)[-1] in NOT_WEIGHTS:
            continue
        shape = tuple(sd[k].shape)
        z = rng.standard_normal(int(np.prod(shape)))
        if len(shape) == 1:
            a = 1.0 + 0.1 * z if k.endswith(".weight") else 0.1 * z
        else:
            a = GAIN * z / np.sqrt(float(shape[-1]))
        out[k] = torch.from_numpy(a.reshape(shape).astype(np.float32))
    return out


def w2v_fields():
    """the configuration tests/golden/tiny_w2v2.npz was written with (oracle/gen_golden.py gen_tiny_w2v2)"""
    from conftest import TINY
    f = dict(TINY)
    f.update(final_dim=32, quantize_targets=True, latent_vars=20, latent_groups=2, latent_dim=0,
             latent_temp=(2.0, 0.5, 0.999995), num_negatives=7, cross_sample_negatives=3, logit_temp=0.1,
             relative_position_embedding=False, gru_rel_pos=False)
    return f


def encoder_state(keys):
    """the golden encoder's weights under `encoder.w2v_model.`, for the names in `keys` (the pre-training heads are gone)"""
    from conftest import golden_state_dict, load_golden
    sd = golden_state_dict(load_golden(ENCODER_GOLDEN))
    return {k: sd[k[len("encoder.w2v_model."):]] for k in keys if k.startswith("encoder.w2v_model.")}


def build(name, dtype=torch.float32, device=None):
    """this package's model `name` with the filled weights -- built anew at every call"""
    from unispeech_amd.seq2seq import Wav2Vec2Seq2Seq
    from unispeech_amd.wav2vec2 import Wav2Vec2Config
    f = w2v_fields()
    wcfg = Wav2Vec2Config(**{k: v for k, v in f.items() if k in Wav2Vec2Config.__dataclass_fields__})
    m = Wav2Vec2Seq2Seq.build(wcfg, VOCAB, dict(MODELS[name]), arch="wav2vec2", pad=PAD, eos=EOS, unk=UNK)
    sd = m.state_dict()
    full = fill_decoder(sd, SEEDS[name])
    full.update(encoder_state(sd.keys()))
    full.update({k: v for k, v in sd.items() if k.rsplit(".", 1)[-1] in NOT_WEIGHTS})
    m.load_state_dict(full, strict=True)
    if device is not None:
        m = m.to(device)
    return m.to(dtype)


@functools.lru_cache(maxsize=None)
def batch():
    """(source fp32 [3, 16000] zero beyond a length, padding_mask bool [3, 16000]): three waveforms of different lengths"""
    g = torch.Generator().manual_seed(909)
    src = torch.randn(len(WAVE_LENGTHS), max(WAVE_LENGTHS), generator=g)
    pm = torch.zeros(src.shape, dtype=torch.bool)
    for b, n in enumerate(WAVE_LENGTHS):
        src[b, n:] = 0
        pm[b, n:] = True
    return src, pm


@functools.lru_cache(maxsize=None)
def forced_tokens():
    """prev_output_tokens long [3, 9]: eos, then 8 / 5 / 3 letters, right-padded with pad"""
    g = torch.Generator().manual_seed(910)
    tok = torch.full((3, 9), PAD, dtype=torch.long)
    for b, n in enumerate((8, 5, 3)):
        tok[b, 0] = EOS
        tok[b, 1:1 + n] = torch.randint(4, VOCAB, (n,), generator=g)
    return tok


# ---------------------------------------------------------------------------------------- wavlm_attn_cross_fwd: built cases
CROSS_TS = 300
# every length of the first fifteen has rows; the empty groups sit on two further sentences (lengths that occur above as well),
# one between groups that have rows and one at the end
CROSS_LENGTHS = (1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300, 64, 129, 300)
CROSS_GROUPS = (1, 1, 5, 32, 33, 70, 1, 2, 2, 3, 6, 7, 33, 1, 4, 0, 2, 0)
CROSS_LONG = dict(Ts=1500, lengths=(1500, 1217), groups=(5, 33))
CROSS_TOL_F32, CROSS_TOL_BF16 = 5e-5, 2.0 ** -8          # of max |V| (tests/test_lm_incremental_gpu.py)


def bf16_valued(t):
    return t.to(torch.bfloat16).float()


def cross_case(d, H, Ts=CROSS_TS, lengths=CROSS_LENGTHS, groups=CROSS_GROUPS, seed=0, holes=True):
    """bf16-valued (q [R, H d], kv [B, Ts, 2 H d], src_lengths int32 [B], row_offsets int32 [B + 1], live int32 [R]): one row in
    seven is dead where `holes`"""
    g = torch.Generator().manual_seed(5000 + 100 * seed + d + H)
    B, R, D = len(lengths), sum(groups), H * d
    q = bf16_valued(1.5 * torch.randn(R, D, generator=g))
    kv = torch.randn(B, Ts, 2 * D, generator=g)
    kv[..., D:] += 0.5
    kv = bf16_valued(kv)
    off = torch.tensor(np.concatenate([[0], np.cumsum(groups)]), dtype=torch.int32)
    live = torch.ones(R, dtype=torch.int32)
    if holes:
        live[3::7] = 0
        live[5::11] = -2
        for b in range(B):                                   # the holes leave every sentence that has rows a live one
            assert groups[b] == 0 or int(live[int(off[b]):int(off[b + 1])].max()) > 0, b
    return q, kv, torch.tensor(lengths, dtype=torch.int32), off, live


def cross_reference(q, kv, src_lengths, row_offsets, live, H, scale=None):
    """float64 [R, H d]: zeros for a dead row or an empty sentence"""
    R, D = q.shape
    d = D // H
    scale = d ** -0.5 if scale is None else scale
    out = torch.zeros(R, D, dtype=torch.float64)
    for b in range(kv.shape[0]):
        n = max(0, min(int(src_lengths[b]), kv.shape[1])) if src_lengths is not None else kv.shape[1]
        lo, hi = int(row_offsets[b]), int(row_offsets[b + 1])
        if n == 0 or hi <= lo:
            continue
        k = kv[b, :n, :D].double().view(n, H, d).transpose(0, 1)
        v = kv[b, :n, D:].double().view(n, H, d).transpose(0, 1)
        qq = q[lo:hi].double().view(hi - lo, H, d).transpose(0, 1)
        o = torch.softmax(scale * qq @ k.transpose(1, 2), -1) @ v
        out[lo:hi] = o.transpose(0, 1).reshape(hi - lo, D)
    if live is not None:
        out[live <= 0] = 0
    return out


def poison(q, kv, src_lengths, live):
    """NaN into K and V at and beyond every length and into the dead rows of q (copies)"""
    q, kv = q.clone(), kv.clone()
    for b in range(kv.shape[0]):
        kv[b, int(src_lengths[b]):] = math.nan
    if live is not None:
        q[live <= 0] = math.nan
    return q, kv


# -------------------------------------------------------------------------------------------- wavlm_beam_step: built cases
BEAM_V = (5, 32, 2048, 2049, 10001)
BEAM_WIDTHS = (1, 5, 32)
BEAM_GAP = 1e-4


def beam_case(V, beam, kind, seed=0):
    """one call of wavlm_beam_step over B = 3 sentences.  kind: "first" (step 0, one live row), "later" (step 3, full beams, one
    row at -inf where beam > 1, two logits at -inf, sentence 1 finished), "forced" (step == max_len: only eos survives), "blocked" (step < min_len),
    "ties" (integer logits, rows and tokens duplicated).  -> dict(logits fp32 [3 beam, V], cum fp32 [3 beam], n_live, n_fin,
    step, max_len, min_len, unk_penalty).  Except in "ties" the float64 scores of neighbouring candidates among the best
    2 beam + 1 differ by more than BEAM_GAP: the seed is advanced until they do."""
    from unispeech_amd.seq2seq import beam_step_reference
    B = 3
    step = 0 if kind == "first" else 3
    max_len, min_len = (3, 1) if kind == "forced" else ((12, 5) if kind == "blocked" else (12, 1))
    for attempt in range(200):
        g = torch.Generator().manual_seed(7000 + 1000 * seed + 17 * V + beam + 100003 * attempt)
        if kind == "ties":
            logits = torch.randint(0, 3, (B * beam, V), generator=g).float()
            logits[:, 1::2] = logits[:, 0:V - 1:2][:, :logits[:, 1::2].shape[1]]        # tokens duplicated in pairs
            for b in range(B):
                blk = logits[b * beam:(b + 1) * beam]
                blk[1::2] = blk[0:beam - 1:2][:blk[1::2].shape[0]]                       # rows duplicated in pairs
            cum = -torch.randint(0, 3, (B * beam,), generator=g).float()
            cum.view(B, beam)[:, 1::2] = cum.view(B, beam)[:, 0:beam - 1:2][:, :cum.view(B, beam)[:, 1::2].shape[1]]
        else:
            logits = 3.0 * torch.randn(B * beam, V, generator=g)
            cum = -5.0 * torch.rand(B * beam, generator=g)
        if step == 0:
            cum = torch.zeros(B * beam)
            n_live = [1, 1, 1]
            n_fin = [0, 0, 0]
        else:
            n_live = [beam, 0, beam]
            n_fin = [0, beam, min(2, beam - 1)]
            if beam > 1 and kind != "ties":
                cum[2 * beam + 1] = -math.inf
        if kind == "later":
            logits[0, 0] = logits[0, V - 1] = -math.inf                                 # tokens of probability 0: lane 0's first
            #                                                                             entry of the log-sum-exp, and the last
        if kind == "later" and beam > 2:
            logits[2 * beam, 1] = math.nan                                              # one NaN: the row's log-sum-exp is NaN, and
            #                                                                             every entry of the row becomes -inf
        case = dict(logits=logits, cum=cum, n_live=n_live, n_fin=n_fin, step=step, max_len=max_len, min_len=min_len,
                    unk_penalty=0.5, V=V, beam=beam, kind=kind)
        if kind == "ties":
            return case
        ok = True
        for b in range(B):
            if n_live[b] == 0:
                continue
            r = beam_step_reference(logits[b * beam:b * beam + n_live[b]].double(), cum[b * beam:b * beam + n_live[b]].double(),
                                    step, n_fin[b], full=True, **reference_options(case))
            s = [v for v, _ in r["all"][:2 * beam + 1] if v > -math.inf]
            if any(a - c <= BEAM_GAP for a, c in zip(s[:-1], s[1:])):
                ok = False
        if ok:
            return case
    raise AssertionError("no seed separates the candidates of V=%d beam=%d %s" % (V, beam, kind))


def reference_options(case):
    return dict(beam=case["beam"], max_len=case["max_len"], min_len=case["min_len"], pad=PAD, unk=UNK, eos=EOS,
                unk_penalty=case["unk_penalty"], temperature=1.0, len_penalty=1.0, normalize_scores=True)


def beam_expected(case):
    """per sentence: None where nothing lives, else beam_step_reference's result in float64"""
    from unispeech_amd.seq2seq import beam_step_reference
    beam, out = case["beam"], []
    for b, n in enumerate(case["n_live"]):
        if n == 0:
            out.append(None)
            continue
        out.append(beam_step_reference(case["logits"][b * beam:b * beam + n].double(), case["cum"][b * beam:b * beam + n].double(),
                                       case["step"], case["n_fin"][b], **reference_options(case)))
    return out


BEAM_KINDS = ("first", "later", "forced", "blocked", "ties")


def beam_cases():
    """(V, beam, kind) of every built case: all V x beams for "first" and "later", the rest at V 32 and 2049"""
    out = [(V, beam, kind) for V in BEAM_V for beam in BEAM_WIDTHS for kind in ("first", "later")]
    out += [(V, beam, kind) for V in (32, 2049) for beam in BEAM_WIDTHS for kind in ("forced", "blocked", "ties")]
    return out
