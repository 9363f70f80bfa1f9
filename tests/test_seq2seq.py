"""unispeech_amd.seq2seq on the CPU: loading by the reference's keys, the float64 references against tests/golden/seq2seq.npz
(tools/gen_seq2seq_golden.py: the reference's model and its SequenceGenerator), the rules of a search step on hand-made
logits, the refusals, and the new symbols.  Nothing here needs a GPU."""
import math
import os
import re

import numpy as np
import pytest
import torch

import seq2seq_cases as C
from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    return load_golden("seq2seq.npz")


@pytest.fixture(scope="module")
def models():
    return {name: C.build(name) for name in C.MODELS}


def encoder_of(golden, model):
    from unispeech_amd import seq2seq as S
    return S.encoder_proj_reference(model, torch.from_numpy(golden["enc/x"])), torch.from_numpy(golden["enc/padding_mask"])


# ---------------------------------------------------------------------------------------------------------------- loading
@pytest.mark.parametrize("name", list(C.MODELS))
def test_state_dict_round_trip_by_the_references_keys(golden, models, name):
    m = models[name]
    keys = [str(k) for k in golden[name + "/keys"]]
    assert sorted(m.state_dict()) == keys
    assert ("encoder.proj.weight" in keys) == (name == "B") and ("decoder.embed_out" in keys) == (name == "A")
    assert ("decoder.layer_norm.weight" in keys) == (name == "B")
    assert ("decoder.embed_positions.weight" in keys) == (name == "B")
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    other = C.build(name)
    other.load_state_dict(sd, strict=True)
    for k, v in other.state_dict().items():
        assert torch.equal(v, sd[k]), k
    extra = dict(sd, **{"decoder.layers.0.no_such.weight": torch.zeros(1)})
    with pytest.raises(RuntimeError, match="no_such"):
        other.load_state_dict(extra, strict=True)
    missing = {k: v for k, v in sd.items() if k != "decoder.layers.1.encoder_attn.k_proj.bias"}
    with pytest.raises(RuntimeError, match="encoder_attn.k_proj.bias"):
        other.load_state_dict(missing, strict=True)


def test_from_checkpoint(tmp_path, models):
    from unispeech_amd.ctc import LetterDictionary
    from unispeech_amd.seq2seq import Wav2Vec2Seq2Seq
    d = LetterDictionary(C.SYMBOLS)
    assert len(d) == C.VOCAB and (d.pad(), d.eos(), d.unk()) == (C.PAD, C.EOS, C.UNK)
    pre = tmp_path / "pre.pt"
    torch.save({"cfg": {"model": C.w2v_fields()}, "model": {}}, pre)
    for name, how in (("A", "w2v_args"), ("B", "w2v_path")):
        cfg = dict(C.MODELS[name], _name="wav2vec_seq2seq", final_dropout=0.0, mask_channel_before=False)
        cfg[how] = C.w2v_fields() if how == "w2v_args" else str(pre)
        path = tmp_path / (name + ".pt")
        torch.save({"cfg": {"model": cfg}, "model": models[name].state_dict()}, path)
        m = Wav2Vec2Seq2Seq.from_checkpoint(str(path), d)
        for k, v in models[name].state_dict().items():
            assert torch.equal(m.state_dict()[k], v), k
    torch.save({"model": {}}, tmp_path / "bad.pt")
    with pytest.raises(NotImplementedError, match="checkpoint dict"):
        Wav2Vec2Seq2Seq.from_checkpoint(str(tmp_path / "bad.pt"), d)


# -------------------------------------------------------------------------------------------------- float64 references
@pytest.mark.parametrize("name", list(C.MODELS))
def test_decoder_reference_against_the_golden_logits(golden, models, name):
    from unispeech_amd import seq2seq as S
    enc, pm = encoder_of(golden, models[name])
    got = S.decoder_reference(models[name], enc, pm, C.forced_tokens()).numpy()
    want, mx = golden[name + "/logits"].astype(np.float64), float(golden[name + "/max"])
    err = np.abs(got - want).max()
    print("decoder_reference", name, "error", err, "of max", mx, "=", err / mx)
    assert got.shape == want.shape == (3, 9, C.VOCAB) and float(golden[name + "/inc_err"]) <= 1e-5
    assert err <= 1e-5 * mx


@pytest.mark.parametrize("beam", C.BEAMS)
@pytest.mark.parametrize("name", list(C.MODELS))
def test_search_reference_reproduces_the_golden_hypotheses(golden, models, name, beam):
    from unispeech_amd import seq2seq as S
    enc, pm = encoder_of(golden, models[name])
    src, _ = C.batch()
    margins = []
    res = S.generate_reference(models[name], enc, pm, src.shape[1], beam=beam, max_len_b=C.MAX_LEN_B, margins=margins)
    p = "%s/beam%d/" % (name, beam)
    lens = golden[p + "lens"]
    assert min(margins) == pytest.approx(float(golden[p + "margin"]), rel=1e-6) and min(margins) > 1e-3
    for b in range(3):
        assert len(res[b]) == int((lens[b] > 0).sum()) == beam
        for j, h in enumerate(res[b]):
            n = int(lens[b, j])
            assert h["tokens"].tolist() == golden[p + "tokens"][b, j, :n].tolist()
            assert abs(float(h["score"]) - float(golden[p + "score"][b, j])) <= 1e-5
            assert np.abs(h["positional_scores"].numpy() - golden[p + "pos"][b, j, :n]).max() <= 1e-5
    all_lens = lens[lens > 0]
    if beam == 5:
        assert (all_lens < C.MAX_LEN_B + 1).any() and (all_lens == C.MAX_LEN_B + 1).any()


# ---------------------------------------------------------------------------------------------------- one search step
OPTS = dict(beam=2, max_len=10, min_len=1, pad=C.PAD, unk=C.UNK, eos=C.EOS)


def test_tie_rule_on_integer_logits():
    """rows 0 and 1 are equal and tokens 4 and 5 are equal in both: four candidates tie at the top; the order is by k * V + token"""
    from unispeech_amd.seq2seq import beam_step_reference
    V = 8
    row = torch.tensor([0.0, 0.0, 0.0, 0.0, 3.0, 3.0, 1.0, 1.0])
    r = beam_step_reference(torch.stack([row, row]), [-1.0, -1.0], 2, 0, **OPTS)
    assert [i for _, i in r["candidates"]] == [4, 5, V + 4, V + 5]
    s = [v for v, _ in r["candidates"]]
    assert s[0] == s[1] == s[2] == s[3]
    assert [(k, t) for k, t, _, _ in r["rows"]] == [(0, 4), (0, 5)] and not r["finished"] and not r["done"]
    # an eos tied with a letter: the smaller flat index comes first, here the eos (token 2)
    row = torch.tensor([0.0, 0.0, 3.0, 0.0, 3.0, 0.0, 0.0, 0.0])
    r = beam_step_reference(row.view(1, -1), [0.0], 1, 0, **OPTS)
    assert [i for _, i in r["candidates"]][:2] == [2, 4] and len(r["finished"]) == 1 and r["finished"][0][3:] == (0, 2)
    for case in (C.beam_case(32, 5, "ties"), C.beam_case(2049, 32, "ties")):
        for e in C.beam_expected(case):
            if e is not None:
                c = e["candidates"]
                assert any(a[0] == b[0] for a, b in zip(c[:-1], c[1:]))             # the built tie cases do tie
                assert all(a[0] > b[0] or (a[0] == b[0] and a[1] < b[1]) for a, b in zip(c[:-1], c[1:]))


def test_step_rules_on_hand_made_logits():
    from unispeech_amd.seq2seq import beam_step_reference
    V = 8
    x = torch.tensor([[9.0, 50.0, 1.0, 8.0, 2.0, 3.0, 0.0, 0.0]])                  # pad would win, unk is second
    lse = float(torch.logsumexp(x[0], 0))
    r = beam_step_reference(x, [0.0], 3, 0, **OPTS)
    assert all(i != C.PAD for _, i in r["candidates"]) and len(r["candidates"]) == min(4, V - 1)
    assert r["candidates"][0] == (pytest.approx(9.0 - lse), 0)
    r = beam_step_reference(x, [0.0], 3, 0, unk_penalty=7.5, **OPTS)                 # unk 8 - 7.5 falls behind bos, 5 and 4
    assert [i for _, i in r["candidates"]] == [0, 5, 4, 2] and r["candidates"][3][0] == pytest.approx(1.0 - lse)
    # step >= max_len: only eos survives, it is finalized with the length-normalised score, and the sentence is done
    r = beam_step_reference(x, [-2.0], 10, 0, **OPTS)
    assert r["candidates"][0] == (pytest.approx(1.0 - lse - 2.0), C.EOS) and r["candidates"][1][0] == -math.inf
    assert r["done"] and r["rows"] == [] and len(r["finished"]) == 1
    score, raw, step_score, k, length = r["finished"][0]
    assert raw == pytest.approx(1.0 - lse - 2.0) and score == pytest.approx(raw / 11) and step_score == pytest.approx(1.0 - lse)
    assert (k, length) == (0, 11)
    assert beam_step_reference(x, [-2.0], 10, 0, **dict(OPTS, normalize_scores=False))["finished"][0][0] == pytest.approx(raw)
    assert beam_step_reference(x, [-2.0], 10, 0, **dict(OPTS, len_penalty=0.5))["finished"][0][0] == pytest.approx(raw / 11 ** 0.5)
    # step < min_len: eos is out
    y = torch.tensor([[0.0, 0.0, 9.0, 0.0, 1.0, 2.0, 0.0, 0.0]])
    r = beam_step_reference(y, [0.0], 1, 0, **dict(OPTS, min_len=2))
    assert all(i != C.EOS or s == -math.inf for s, i in r["candidates"]) and not r["finished"]
    r = beam_step_reference(y, [0.0], 2, 0, **dict(OPTS, min_len=2))
    assert r["candidates"][0][1] == C.EOS and len(r["finished"]) == 1
    # a NaN logit: the row's log-softmax is NaN, every entry of the row becomes -inf; the other row goes on
    z = torch.tensor([[0.0, 0.0, math.nan, 0.0, 1.0, 2.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0, 1.0, 2.0, 0.0, 0.0]])
    r = beam_step_reference(z, [0.0, -50.0], 3, 0, **OPTS)
    assert [i // V for _, i in r["candidates"]] == [1, 1, 1, 1] and all(math.isfinite(s) for s, _ in r["candidates"])
    # an eos beyond the first `beam` ranks is neither finalized nor continued; a full finished list takes no more
    w = torch.tensor([[0.0, 0.0, 5.0, 0.0, 9.0, 8.0, 0.0, 0.0]])
    r = beam_step_reference(w, [0.0], 3, 0, **OPTS)
    assert [i for _, i in r["candidates"]][:3] == [4, 5, 2] and not r["finished"] and [t for _, t, _, _ in r["rows"]] == [4, 5]
    r = beam_step_reference(y, [0.0], 3, 2, **OPTS)
    assert not r["finished"] and r["done"]
    # an eos at -inf is no eos: it is carried as a row (sequence_generator.py:407)
    r = beam_step_reference(torch.tensor([[0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0]]), [-math.inf], 3, 0, **dict(OPTS, beam=1))
    assert r["candidates"][0] == (-math.inf, 0) and not r["finished"]


def test_search_reference_walks_back_through_the_beam():
    """a two-step search by hand: V 6, beam 2; the second-best first token wins in the end"""
    from unispeech_amd.seq2seq import beam_search_reference
    lp = lambda *p: torch.log(torch.tensor(p, dtype=torch.float64))  # noqa: E731
    table = {(2,): lp(0.0, 0.0, 0.0, 0.0, 0.6, 0.4), (2, 4): lp(0.0, 0.0, 0.5, 0.0, 0.25, 0.25), (2, 5): lp(0.0, 0.0, 0.9, 0.0, 0.05, 0.05)}

    def fn(b, prefixes):
        return torch.stack([table.get(tuple(p), lp(0.0, 0.0, 1.0, 0.0, 0.0, 0.0)) for p in prefixes])
    res = beam_search_reference(fn, 1, bos=2, beam=2, max_len=4, min_len=1, pad=1, unk=3, eos=2, normalize_scores=False)[0]
    assert [h["tokens"].tolist() for h in res] == [[5, 2], [4, 2]]
    assert float(res[0]["score"]) == pytest.approx(math.log(0.4 * 0.9)) and float(res[1]["score"]) == pytest.approx(math.log(0.3))
    assert res[0]["positional_scores"].tolist() == pytest.approx([math.log(0.4), math.log(0.9)])


# -------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_by_name(models):
    from unispeech_amd.ctc import EncoderCtc
    from unispeech_amd.seq2seq import Seq2SeqConfig, Wav2Vec2Seq2Seq
    from unispeech_amd.wav2vec2 import Wav2Vec2Config, Wav2Vec2Model
    f = C.w2v_fields()
    w2v = Wav2Vec2Model(Wav2Vec2Config(**{k: v for k, v in f.items() if k in Wav2Vec2Config.__dataclass_fields__}))
    with pytest.raises(ValueError, match="remove_pretraining_modules"):
        Wav2Vec2Seq2Seq(w2v, C.VOCAB, dict(C.MODELS["A"]))
    w2v.remove_pretraining_modules()
    assert Seq2SeqConfig().decoder_attention_heads == 4 and Seq2SeqConfig().decoder_embed_dim == 768
    with pytest.raises(NotImplementedError, match=r"decoder_embed_dim=768 / decoder_attention_heads=4"):
        Wav2Vec2Seq2Seq(w2v, C.VOCAB)                                               # the reference's default: heads 192 wide
    with pytest.raises(NotImplementedError, match="decoder_attention_heads=3"):
        Wav2Vec2Seq2Seq(w2v, C.VOCAB, dict(C.MODELS["A"], decoder_attention_heads=3))
    with pytest.raises(TypeError, match="no_such_option"):
        Wav2Vec2Seq2Seq(w2v, C.VOCAB, dict(C.MODELS["A"], no_such_option=1))
    with pytest.raises(NotImplementedError, match="decoder_layers"):               # the CTC wrapper goes on refusing them
        EncoderCtc(w2v, 12, decoder_layers=2)
    m = models["A"]
    with pytest.raises(NotImplementedError, match="train"):
        m.train()
    assert m.eval() is m and not m.training
    drop = Wav2Vec2Seq2Seq(w2v, C.VOCAB, dict(C.MODELS["A"], decoder_layerdrop=0.1))
    with pytest.raises(NotImplementedError, match="decoder_layerdrop"):
        drop.train()
    src, pm = C.batch()
    with pytest.raises(NotImplementedError, match="gradients"):
        m(src.clone().requires_grad_(True), pm, C.forced_tokens())
    with pytest.raises(NotImplementedError, match="gradients"):
        m.generate(src.clone().requires_grad_(True), pm)
    for name, value in (("prefix_tokens", torch.zeros(3, 1)), ("constraints", [1]), ("sampling", True), ("match_source_len", True),
                        ("no_repeat_ngram_size", 2), ("lm_model", object()), ("models", [m, m])):
        with pytest.raises(NotImplementedError, match=name):
            m.generate(src, pm, **{name: value})
    with pytest.raises(TypeError, match="no_such"):
        m.generate(src, pm, no_such=1)
    with pytest.raises(ValueError, match="min_len"):
        m.generate(src, pm, max_len_b=3, min_len=4)
    with pytest.raises(NotImplementedError, match="beam=33"):
        m.generate(src, pm, beam=33)
    assert m._max_len(16000, 0, 200) == 63 and m._max_len(16000, 0.001, 3) == 19   # min(int(a * src_len + b), positions - 1)


# ------------------------------------------------------------------------------------------------------------------- ABI
def test_new_symbols_exported_and_bound():
    from unispeech_amd import _lib, build, ops
    src = open(os.path.join(ROOT, "include", "wavlm_hip.h")).read()
    assert int(re.search(r"#define WAVLM_HIP_ABI_VERSION (\d+)", src).group(1)) == 30 == _lib.ABI_VERSION
    assert "s2s.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "s2s.hip"))
    L = _lib.lib()
    for name in ("wavlm_attn_cross_fwd_supported", "wavlm_attn_cross_fwd", "wavlm_beam_step_supported",
                 "wavlm_beam_step_workspace_bytes", "wavlm_beam_step"):
        decl = re.search(r"\b%s\(([^;]*)\);" % name, src).group(1)
        assert name in _lib.SIGNATURES and len(decl.split(",")) == len(_lib.SIGNATURES[name][1]), name
        assert hasattr(L, name)
    for fn in ("attn_cross_fwd", "attn_cross_fwd_supported", "beam_step", "beam_step_supported", "BeamState"):
        assert hasattr(ops, fn)
    assert ops.attn_cross_fwd_supported(32, torch.float32) and ops.attn_cross_fwd_supported(64, torch.bfloat16)
    assert not ops.attn_cross_fwd_supported(48, torch.float32) and not L.wavlm_attn_cross_fwd_supported(64, 2)
    assert ops.beam_step_supported(32, 65536, 65535, torch.bfloat16) and ops.beam_step_supported(1, 2, 1, torch.float32)
    for beam, V, B in ((0, 32, 1), (33, 32, 1), (5, 1, 1), (5, 65537, 1), (5, 32, 0), (5, 32, 65536)):
        assert not ops.beam_step_supported(beam, V, B, torch.float32)
    assert L.wavlm_beam_step_workspace_bytes(3, 5) == 256 and L.wavlm_beam_step_workspace_bytes(16, 32) == 8448
    assert L.wavlm_beam_step_workspace_bytes(0, 5) == 0
    with pytest.raises(_lib.WavlmHipError):
        ops.attn_cross_fwd(torch.zeros(2, 64), torch.zeros(1, 4, 128), 2, torch.zeros(2, dtype=torch.int32))


def test_cli_arguments():
    from unispeech_amd import seq2seq
    a = seq2seq.parse_args(["decode", "ck.pt", "dict.txt", "a.wav", "--beam", "3", "--max-len-a", "0.01", "--lenpen", "0.5"])
    assert (a.cmd, a.wavs, a.beam, a.max_len_a, a.max_len_b, a.lenpen, a.nbest) == ("decode", ["a.wav"], 3, 0.01, 200, 0.5, 1)
    a = seq2seq.parse_args(["score", "ck.pt", "dict.txt", "m.tsv", "l.ltr", "--results", "out", "--nbest", "2"])
    assert (a.cmd, a.manifest, a.labels, a.results, a.beam, a.nbest) == ("score", "m.tsv", "l.ltr", "out", 5, 2)
