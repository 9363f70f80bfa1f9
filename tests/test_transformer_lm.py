"""Transformer LM, host side (unispeech_amd/transformer_lm.py, the rescoring of unispeech_amd/ctc_lexicon.py): the float64
reference against tests/golden/transformer_lm.npz (tools/gen_transformer_lm_golden.py: the reference's TransformerLanguageModel
on the CPU), state-dict compatibility, refusals, the workspace bound of wavlm_lm_logprob, S_ngram against the first pass, and
rescore_reference.  No GPU."""
import math
import os

import numpy as np
import pytest
import torch

import ctc_lexicon_cases as L
import transformer_lm_cases as C
from conftest import GOLDEN, load_golden


@pytest.fixture(scope="module")
def g():
    return load_golden("transformer_lm.npz")


@pytest.fixture(scope="module")
def reference_scores():
    """score_reference of the three models on the fixture's sentences, once"""
    from unispeech_amd.transformer_lm import score_reference
    return {name: score_reference(C.build(name), C.sentences()) for name in C.MODELS}


@pytest.mark.parametrize("name", list(C.MODELS))
def test_score_reference_equals_the_fixture(g, reference_scores, name):
    """float64 against the reference's fp32: 1e-5 absolute; unk is -inf; the empty sentence is log p(eos | eos)"""
    lp, tot = (v.numpy() for v in reference_scores[name])
    want = g[name + "/logprobs"]
    assert lp.shape == want.shape == (4, 34)
    fin = np.isfinite(want)
    assert np.array_equal(fin, np.isfinite(lp))
    err = np.abs(lp[fin] - want[fin]).max()
    print(name, "max |score_reference - reference| = %.3e" % err)
    assert err <= 1e-5
    s = C.sentences()
    assert lp[2, 3] == -math.inf and s[2][3] == C.UNK and tot[2] == -math.inf
    assert lp[0, 0] < 0 and not lp[0, 1:].any() and tot[0] == lp[0, 0]           # the empty sentence
    for i in (0, 1, 3):
        assert abs(tot[i] - float(g[name + "/totals"][i])) <= 1e-5 * (len(s[i]) + 1) + 1e-5
        assert not lp[i, len(s[i]) + 1:].any()


def test_score_reference_is_independent_of_the_batch(reference_scores):
    from unispeech_amd.transformer_lm import score_reference
    s = C.sentences()
    lp, tot = reference_scores["B"]
    lp2, tot2 = score_reference(C.build("B"), [s[3], s[1]])
    assert torch.equal(lp2[0], lp[3]) and torch.equal(lp2[1, :2], lp[1, :2]) and torch.equal(tot2, tot[[3, 1]])


@pytest.mark.parametrize("name", list(C.MODELS))
def test_state_dict_keys_are_the_references(g, name):
    """every key of the reference's state dict is consumed and none is invented"""
    m = C.build(name)
    keys = [str(k) for k in g[name + "/keys"]]
    assert sorted(m.state_dict()) == sorted(keys)
    m.load_state_dict({k: v.clone() for k, v in m.state_dict().items()}, strict=True)
    if name == "B":
        assert m.decoder.output_projection.weight is m.decoder.embed_tokens.weight
    if name == "C":
        assert [tuple(m.state_dict()["decoder.embed_tokens.embeddings.%d.0.weight" % i].shape) for i in range(3)] == \
            [(20, 32), (20, 8), (60, 2)]
        assert tuple(m.decoder.project_out_dim.weight.shape) == (32, 64)


@pytest.mark.parametrize("option, value", [("character_embeddings", True), ("base_layers", 2), ("cross_self_attention", True),
                                           ("tie_adaptive_weights", True)])
def test_refused_options_raise_by_name(option, value):
    from unispeech_amd.transformer_lm import TransformerLM
    with pytest.raises(NotImplementedError, match=option):
        TransformerLM(dict(C.MODELS["A"], **{option: value}), C.VOCAB)


def test_refused_head_width_and_ignored_quant_noise():
    from unispeech_amd.transformer_lm import TransformerLM
    with pytest.raises(NotImplementedError, match="decoder_attention_heads"):
        TransformerLM(dict(C.MODELS["A"], decoder_attention_heads=4), C.VOCAB)           # 16 wide
    m = TransformerLM(dict(C.MODELS["A"], quant_noise_pq=0.1, quant_noise_pq_block_size=8), C.VOCAB)
    assert sorted(m.state_dict()) == sorted(C.build("A").state_dict())


def test_learned_positions_refuse_a_sentence_that_is_too_long():
    from unispeech_amd.transformer_lm import score_reference
    m = C.build("B")
    score_reference(m, [[5] * 63])
    with pytest.raises(ValueError, match="max_target_positions"):
        score_reference(m, [[5] * 64])
    with pytest.raises(ValueError, match="dictionary"):
        score_reference(m, [[C.VOCAB]])


def test_from_checkpoint_and_command_line(tmp_path, capsys, reference_scores):
    """{"args": Namespace, "model"} and {"cfg": dict, "model"} load; `score --cpu-reference` prints one line per sentence"""
    import argparse
    from unispeech_amd import transformer_lm as T
    sd = C.build("A").state_dict()
    torch.save({"cfg": dict(C.MODELS["A"]), "model": sd}, tmp_path / "a.pt")
    torch.save({"args": argparse.Namespace(**C.MODELS["A"]), "cfg": None, "model": sd}, tmp_path / "b.pt")
    for f in ("a.pt", "b.pt"):
        m = T.TransformerLM.from_checkpoint(str(tmp_path / f))
        assert m.vocab == C.VOCAB
        assert torch.equal(T.score_reference(m, C.sentences()[:2])[1], reference_scores["A"][1][:2])
    with pytest.raises(NotImplementedError):
        torch.save({"model": sd}, tmp_path / "c.pt")
        T.TransformerLM.from_checkpoint(str(tmp_path / "c.pt"))
    (tmp_path / "dict.txt").write_text("".join("w%d 1\n" % i for i in range(C.VOCAB - 4)))
    (tmp_path / "text.txt").write_text("w1 w2 w3\n\nw5 nosuchword\n")
    assert T.main(["score", str(tmp_path / "a.pt"), str(tmp_path / "dict.txt"), str(tmp_path / "text.txt"), "--cpu-reference"]) == 0
    lines = capsys.readouterr().out.splitlines()
    assert len(lines) == 4 and lines[3].startswith("corpus: 3 sentences, 5 scored tokens")
    want = T.score_reference(C.build("A"), [[5, 6, 7]])[1].item()
    assert lines[0].split("\t") == ["%.4f" % want, "3", "%.4f" % math.exp(-want / 4)]
    assert lines[2].split("\t")[0] == "-inf"


def test_logprob_workspace_is_rows_times_slabs():
    """a host function: O(R x slabs), never O(R x V)"""
    from unispeech_amd import _lib
    h = _lib.lib()
    big = h.wavlm_lm_logprob_workspace_bytes(32768, 200000)
    assert 0 < big < 64 << 20
    assert big < 32768 * 200000 * 4 // 500
    assert h.wavlm_lm_logprob_workspace_bytes(130, 2051) >= 130 * 2 * 12          # more than one slab at V = 2051
    assert h.wavlm_lm_logprob_workspace_bytes(2 * 32768, 200000) <= 2 * big
    assert h.wavlm_lm_logprob_workspace_bytes(0, 5) == 0
    for D, V, dt, ok in [(8, 1, 0, 1), (8192, 2 ** 31 - 1, 1, 1), (80, 257, 1, 1), (4, 5, 0, 0), (36, 5, 1, 0), (8200, 5, 1, 0),
                         (64, 0, 1, 0), (64, 5, 2, 0)]:
        assert h.wavlm_lm_logprob_supported(D, V, dt) == ok, (D, V, dt)
    assert [h.wavlm_attn_causal_fwd_supported(d, 1) for d in (16, 32, 64, 128)] == [0, 1, 1, 0]


def test_no_cpu_fallback_for_the_output_layer():
    from unispeech_amd import _lib
    from unispeech_amd.transformer_lm import lm_logprob
    with pytest.raises(_lib.WavlmHipError):
        lm_logprob(torch.zeros(2, 32), torch.zeros(5, 32), torch.zeros(2, dtype=torch.int32))
    with pytest.raises(_lib.WavlmHipError):
        C.build("A").score([[5]])


# ---------------------------------------------------------------------------------------------------------- rescoring
def test_ngram_sum_is_what_the_first_pass_added():
    """the reference search with lm_weight = w and with lm_weight = 0, same emissions, a beam that prunes nothing: for every
    (words, tokens) in both lists, s1(w) - w * S_ngram(words) == s1(0)"""
    from unispeech_amd import ctc, ctc_lexicon as X
    x, il, d, lexicon, opts = L.case("beam63")
    kw = dict(opts, beam=400, beam_size_token=12, beam_threshold=math.inf, nbest=400)
    w = 0.75
    runs = []
    for lmw in (w, 0.0):
        hyps = X.lexicon_beam_search_reference(x, il, lexicon, L.BLANK, ctc.silence_token(d), normalized=True,
                                               **dict(kw, lm_weight=lmw))[0]
        runs.append([{(tuple(wds), tuple(toks)): sc for wds, toks, sc in h} for h in hyps])
    n = 0
    for with_lm, without in zip(*runs):
        for key in set(with_lm) & set(without):
            assert abs(with_lm[key] - w * X.ngram_sum(lexicon.lm, key[0]) - without[key]) <= 1e-9, key
            # word strings give the same sum as the lexicon's ids
            assert X.ngram_sum(lexicon.lm, [lexicon.words[v] for v in key[0]]) == X.ngram_sum(lexicon.lm, key[0])
            n += 1
    assert n >= 5
    assert X.ngram_sum(None, ["a", "b"]) == 0.0


def _lm_dict():
    from unispeech_amd.ctc import LetterDictionary
    return LetterDictionary(["w%d" % i for i in range(C.VOCAB - 4)])


def test_rescore_reference_by_hand():
    """two hypotheses, a bigram first pass whose scores are written out here"""
    from unispeech_amd import ctc_lexicon as X
    from unispeech_amd.ctc_lm import NgramLM
    from unispeech_amd.transformer_lm import score_reference
    entries = {("<unk>",): (-2.0, 0.0), ("<s>",): (-99.0, -0.5), ("</s>",): (-1.0, 0.0), ("w1",): (-1.5, -0.25),
               ("w2",): (-1.25, -0.125), ("<s>", "w1"): (-0.5, 0.0), ("w1", "w2"): (-0.75, 0.0), ("w2", "</s>"): (-0.375, 0.0)}
    lm1 = NgramLM(2, entries, ["w1", "w2", "<unk>"])
    assert X.ngram_sum(lm1, ["w1", "w2"]) == -0.5 - 0.75 - 0.375
    assert X.ngram_sum(lm1, ["w2"]) == (-0.5 - 1.25) - 0.375                     # backs off from <s>
    assert X.ngram_sum(lm1, ["zzz"]) == (-0.5 - 2.0) - 1.0                       # <unk>, then a unigram </s>
    m, d = C.build("A"), _lm_dict()
    tl = score_reference(m, [[d.index("w1"), d.index("w2")], [d.index("w2")]])[1].tolist()
    hyps = [[(["w1", "w2"], [5, 6], -3.0), (["w2"], [6], -2.5)]]
    res = X.rescore_reference(hyps, m, d, lm1, lm_weight=2.0, word_score=1.0, rescore_weight=0.25, rescore_word_score=-0.5)[0]
    want = [-3.0 - 2.0 * -1.625 + 0.25 * tl[0] + (-0.5 - 1.0) * 2, -2.5 - 2.0 * -2.125 + 0.25 * tl[1] + (-0.5 - 1.0) * 1]
    got = {tuple(e["words"]): e for e in res}
    assert abs(got[("w1", "w2")]["score"] - want[0]) <= 1e-12 and abs(got[("w2",)]["score"] - want[1]) <= 1e-12
    assert got[("w1", "w2")]["first_pass_score"] == -3.0 and got[("w1", "w2")]["lm_score"] == tl[0]
    assert [e["score"] for e in res] == sorted(want, reverse=True)
    assert res[0]["tokens"] == ([5, 6] if want[0] > want[1] else [6])
    # without a first-pass LM and with the first pass's own word score nothing but the LM term is added
    res0 = X.rescore_reference(hyps, m, d, None, 0.0, 1.0, 1.0, 1.0)[0]
    assert {tuple(e["words"]): e["score"] for e in res0} == {("w1", "w2"): -3.0 + tl[0], ("w2",): -2.5 + tl[1]}


def test_rescoring_is_stable_on_ties_and_all_inf():
    from unispeech_amd import ctc_lexicon as X
    m, d = C.build("A"), _lm_dict()
    tie = [[(["w1"], [5], -1.0), (["w1"], [5, 4], -1.0), (["w1"], [4, 5], -1.0)]]
    assert [e["tokens"] for e in X.rescore_reference(tie, m, d)[0]] == [[5], [5, 4], [4, 5]]
    unknown = [[(["zzz"], [7], -5.0), (["w1", "<unk>"], [5], -1.0), (["yyy", "w2"], [6], -3.0)], []]
    res = X.rescore_reference(unknown, m, d)
    assert [e["tokens"] for e in res[0]] == [[7], [5], [6]] and all(e["score"] == -math.inf for e in res[0]) and res[1] == []
    assert [e["first_pass_score"] for e in res[0]] == [-5.0, -1.0, -3.0]
    mixed = [[(["zzz"], [7], 9.0), (["w1"], [5], -1.0)]]
    assert [e["tokens"] for e in X.rescore_reference(mixed, m, d)[0]] == [[5], [7]]
    # rescore_weight 0 leaves an unknown word's hypothesis finite: 0 x -inf is not formed
    assert X.rescore_reference(mixed, m, d, rescore_weight=0.0)[0][0]["score"] == 9.0


def test_rescoring_case_of_the_fixture(g):
    """the float64 second pass over the float64 first pass reproduces the stored order and scores; each distinct word sequence is
    scored once"""
    from unispeech_amd import ctc_lexicon as X, transformer_lm as T
    x, il, d, lexicon, opts, lm_dict = C.rescoring()
    hyps = X.lexicon_beam_decode(x, il, d, lexicon, lexicon.lm, normalized=True, **opts)
    m, calls = C.build("A"), []
    real = T.score_reference

    def counting(model, sents):
        calls.append([tuple(s) for s in sents])
        return real(model, sents)
    T.score_reference = counting
    try:
        res = X.rescore_reference(hyps, m, lm_dict, lexicon.lm, opts["lm_weight"], opts["word_score"], **C.RESCORE_OPTS)
    finally:
        T.score_reference = real
    assert len(calls) == 1 and len(set(calls[0])) == len(calls[0])
    changed = 0
    for b, (utt, r) in enumerate(zip(hyps, res)):
        first = [(tuple(h[0]), tuple(h[1])) for h in utt]
        order = [first.index((tuple(e["words"]), tuple(e["tokens"]))) for e in r]
        assert order == list(g["rescore/order_%d" % b])
        s2, want = np.array([e["score"] for e in r]), g["rescore/s2_%d" % b]
        assert np.array_equal(np.isfinite(s2), np.isfinite(want)) and np.allclose(s2[np.isfinite(s2)], want[np.isfinite(want)], atol=1e-9)
        assert s2[0] - s2[1] > 2 * float(g["rescore/tol"])
        changed += order[0] != 0
    assert changed >= 1                                  # the second pass overturns at least one first-pass winner


def test_fixture_is_small():
    assert os.path.getsize(os.path.join(GOLDEN, "transformer_lm.npz")) < 256 * 1024
    assert os.path.getsize(os.path.join(GOLDEN, "transformer_lm_wide.npz")) < 256 * 1024


# ------------------------------------------------------------------------------------------- the models at production width
@pytest.mark.parametrize("name", list(C.WIDE_MODELS))
def test_wide_score_reference_equals_the_fixture(name):
    """models W and X (D 512 / 256, V 5003, sentences of up to 200 words) against tests/golden/transformer_lm_wide.npz: the bound
    of test_score_reference_equals_the_fixture"""
    from unispeech_amd.transformer_lm import score_reference
    g = load_golden("transformer_lm_wide.npz")
    s = C.wide_sentences()
    assert [len(x) for x in s] == [0, 1, 126, 127, 128, 200] and C.WIDE_VOCAB > 2 * C.LM_SLAB and C.WIDE_VOCAB % C.LM_TILE
    lp, tot = (v.numpy() for v in score_reference(C.build_wide(name), s))
    want = g[name + "/logprobs"]
    assert lp.shape == want.shape == (6, 201)
    fin = np.isfinite(want)
    assert np.array_equal(fin, np.isfinite(lp))
    err = np.abs(lp[fin] - want[fin]).max()
    print(name, "max |score_reference - reference| = %.3e" % err)
    assert err <= 1e-5
    i, t = C.WIDE_UNK_AT
    assert s[i][t] == C.UNK and lp[i, t] == -math.inf and tot[i] == -math.inf and (~fin).sum() == 1
    for i in range(6):
        if i != C.WIDE_UNK_AT[0]:
            assert abs(tot[i] - float(g[name + "/totals"][i])) <= 1e-5 * (len(s[i]) + 1) + 1e-5
        assert not lp[i, len(s[i]) + 1:].any()
    assert float(g[name + "/max"]) == np.abs(want[fin]).max() and 0 < float(g[name + "/e_ref"]) < 0.05


# ------------------------------------------------------------- what the built kernel cases of the GPU suite rest on
def test_slot_targets_cover_every_position_of_a_tile():
    """each block of 128 rows has a target at each of the 128 positions of a tile; the first block's tile is the last one of slab
    0, the second block's targets lie in slab 1 as far as it has entries"""
    t = C.slot_targets().numpy()
    assert t.shape == (256,) and t.min() >= 0 and t.max() < 2051
    for b in range(2):
        assert sorted(t[128 * b:128 * b + 128] % C.LM_TILE) == list(range(128))
    assert (t[:128] // C.LM_TILE == 15).all() and (t[:128] // C.LM_SLAB == 0).all()
    assert t[128:131].tolist() == [2048, 2049, 2050] and (t[131:] // C.LM_TILE == 14).all()
    assert np.array_equal(C.slot_case()[2].numpy(), t)


def test_staircase_keeps_the_online_softmax_rescaling():
    """from the float64 logits alone: the c = 2 row renews its running tile maximum in at least 40 of the 49 tiles while no tile
    holds more than 40 % of its mass, and in the c = 0 row each of the three full slabs holds 25 % to 40 %"""
    X, W, tgt, z, lse, lp = C.staircase_case()
    assert torch.equal(X, C.bf16_valued(X)) and torch.equal(W, C.bf16_valued(W))
    assert X[:, 0].tolist() == list(C.STAIR_C) and z.shape == (5, 6200)
    tiles, renew, share, slabs = C.staircase_profile(z[0])
    print("c = 2: %d of %d tiles renew the maximum, largest tile %.2f, slabs %s" % (renew, tiles, share, np.round(slabs, 2)))
    assert tiles == 49 and renew >= 40 and share <= 0.40
    tiles, renew, share, slabs = C.staircase_profile(z[4])
    print("c = 0: slabs", np.round(slabs, 3))
    assert len(slabs) == 4 and all(0.25 <= s <= 0.40 for s in slabs[:3])


@pytest.mark.parametrize("d", [32, 64])
def test_rising_scores_keep_the_attention_rescaling(d):
    """from the float64 scores alone, for queries >= 128 of the rising heads: at least three quarters of the 32-key steps a query
    sees renew its running maximum and no step holds more than half of its mass"""
    qkv = C.rising_causal_qkv(d)
    assert torch.equal(qkv, C.bf16_valued(qkv))
    x = qkv.view(C.RISING_B, C.RISING_T, 3, C.RISING_H, d)
    assert (x[:, :, 0, 0, 0] == C.rising_constant(d)).all() and (x[:, :, 0, 1, 0] == -C.rising_constant(d)).all()
    assert torch.equal(x[0, :, 1, 3, 0], (torch.arange(C.RISING_T) // 32).float() / 4)
    renew, share = C.rising_profile(qkv, d)
    print("d %d: smallest fraction of renewing steps %.2f, largest share of one step %.2f" % (d, renew, share))
    assert renew >= 0.75 and share <= 0.5
