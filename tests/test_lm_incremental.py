"""Transformer LM inside the first pass, host side: incremental_reference (unispeech_amd/transformer_lm.py) against
score_reference and against tests/golden/transformer_lm_incremental.npz (tools/gen_transformer_lm_incremental_golden.py: the
reference's decoder run with incremental_state), NeuralWordLM and fused_lexicon_decode (unispeech_amd/ctc_lexicon.py) against the
lexicon search with the same scorer, the margin the GPU search test rests on, and the command line's refusals.  No GPU."""
import math
import os

import numpy as np
import pytest
import torch

import lm_incremental_cases as I
import transformer_lm_cases as C
from conftest import GOLDEN, load_golden


@pytest.fixture(scope="module")
def gi():
    return load_golden("transformer_lm_incremental.npz")


@pytest.fixture(scope="module")
def chains():
    """per model: the store and, per sentence of the fixture, the float64 rows [n + 1, V] of its chain of states"""
    from unispeech_amd.transformer_lm import incremental_reference
    out = {}
    for name in C.MODELS:
        store = incremental_reference(C.build(name))
        out[name] = store, {i: store.logprob_rows(I.walk_chain(store, C.sentences()[i])).numpy() for i in range(4)}
    return out


@pytest.mark.parametrize("name", list(C.MODELS))
def test_chains_equal_score_reference(chains, name):
    """every sentence of sentences() walked one word per extend(): the target's entry of each row is score_reference's, 1e-9"""
    from unispeech_amd.transformer_lm import score_reference
    want = score_reference(C.build(name), C.sentences())[0].numpy()
    for i, s in enumerate(C.sentences()):
        rows = chains[name][1][i]
        assert rows.shape == (len(s) + 1, C.VOCAB) and rows.dtype == np.float64
        assert np.abs(np.exp(rows).sum(1) - 1).max() <= 1e-12                   # normalised
        got = np.array([rows[t, w] for t, w in enumerate(s + [C.EOS])])
        fin = np.isfinite(want[i, :len(s) + 1])                                  # score_reference writes -inf at an unk target
        assert [w != C.UNK for w in s + [C.EOS]] == list(fin)
        err = np.abs(got[fin] - want[i, :len(s) + 1][fin]).max()
        print(name, "sentence", i, "max |incremental - full| = %.3e" % err)
        assert err <= 1e-9


@pytest.mark.parametrize("name", list(C.MODELS))
def test_branching_tree_gives_the_rows_of_the_full_sentences(name):
    """shared prefix, two continuations, the older branch extended after the newer: full rows against the full forward"""
    from unispeech_amd.transformer_lm import _forward64, incremental_reference
    m = C.build(name)
    store = incremental_reference(m)
    walks = I.walk_tree(store)
    assert walks[0][:4] == walks[1][:4] and len(set(walks[0] + walks[1])) == 1 + 3 + 3 + 2 == len(store)
    for states, s in zip(walks, I.tree_sentences()):
        with torch.no_grad():
            want = _forward64(m, s).numpy()
        assert np.abs(store.logprob_rows(states).numpy() - want).max() <= 1e-9
    cols = [C.EOS, 7, 99]
    assert torch.equal(store.logprob_rows(walks[1], cols), store.logprob_rows(walks[1])[:, cols])
    n = len(store)
    store.reset()
    assert len(store) == 1 and store.extend([0], [5]) == [1] and n == 9


@pytest.mark.parametrize("name", list(C.MODELS))
def test_incremental_reference_equals_the_fixture(gi, chains, name):
    """float64 against the reference's decoder with incremental_state in fp32, full rows: 1e-5 absolute, the bound of
    tests/test_transformer_lm.py test_score_reference_equals_the_fixture"""
    assert float(gi[name + "/full_err"]) <= 1e-5 and 0 < float(gi[name + "/e_ref"]) < 0.05
    worst = 0.0
    for i in I.GOLDEN_SENTENCES:
        want = gi["%s/rows_%d" % (name, i)]
        got = chains[name][1][i]
        assert want.shape == got.shape and want.dtype == np.float32
        worst = max(worst, float(np.abs(got - want).max()))
    print(name, "max |incremental_reference - reference| = %.3e" % worst)
    assert worst <= 1e-5
    assert float(gi[name + "/max"]) == max(np.abs(gi["%s/rows_%d" % (name, i)]).max() for i in I.GOLDEN_SENTENCES)


def test_fixture_is_small():
    assert os.path.getsize(os.path.join(GOLDEN, "transformer_lm_incremental.npz")) < 256 * 1024


def test_depth_beyond_max_target_positions_and_bad_ids_raise():
    from unispeech_amd.transformer_lm import incremental_reference
    store = incremental_reference(C.build("B"))                                  # max_target_positions 64
    st = I.walk_chain(store, [5] * 63)
    with pytest.raises(ValueError, match="max_target_positions"):
        store.extend([st[-1]], [5])
    with pytest.raises(ValueError, match="dictionary"):
        store.extend([0], [C.VOCAB])
    with pytest.raises(ValueError, match="state"):
        store.extend([len(store)], [5])
    with pytest.raises(ValueError):
        store.extend([0, 0], [5])
    assert store.extend([], []) == [] and tuple(store.logprob_rows([]).shape) == (0, C.VOCAB)


def test_no_cpu_fallback_for_the_device_store():
    from unispeech_amd import _lib
    with pytest.raises(_lib.WavlmHipError):
        C.build("A").incremental()


def test_step_kernel_is_declared_and_answers_on_the_host():
    from unispeech_amd import _lib
    h = _lib.lib()
    assert [h.wavlm_attn_step_supported(d, 1) for d in (16, 32, 64, 128)] == [0, 1, 1, 0]
    assert h.wavlm_attn_step_supported(64, 0) == 1 and h.wavlm_attn_step_supported(64, 2) == 0


# --------------------------------------------------------------------------------------------------------- the scorer
def test_neural_word_lm_follows_fairseqlm():
    """natural log, a word the LM's dictionary lacks is its unk, unk scores -inf, a history reached twice is one state; prepare
    evaluates the listed states that have no row in one extend() per depth; rows can be dropped and come back"""
    from unispeech_amd import ctc_lexicon as X
    from unispeech_amd.transformer_lm import incremental_reference, score_reference
    x, il, d, lexicon, opts, lm_dict = I.search_case(incremental_reference(C.build("A")))
    lm = lexicon.lm
    assert isinstance(lm, X.NeuralWordLM) and len(lm.tok_word) == len(lexicon.words) == len(lm.words)
    known = [w for w in range(len(lexicon.words)) if lm.tok_word[w] != lm_dict.unk()]
    for w in C.UNKNOWN_TO_LM + ("<unk>",):
        assert lm.tok_word[lexicon.words.index(w)] == lm_dict.unk()
    a, b = known[0], known[3]
    la, sa = lm.score_word(lm.start, int(lm.tok_word[a]))
    lb, sab = lm.score_word(sa, int(lm.tok_word[b]))
    le = lm.score_eos(sab)
    want = score_reference(C.build("A"), [[int(lm.tok_word[a]), int(lm.tok_word[b])]])[0][0].tolist()
    assert max(abs(la - want[0]), abs(lb - want[1]), abs(le - want[2])) <= 1e-9
    assert lm.score_word(lm.start, int(lm.tok_word[a]))[1] == sa                 # one state per history
    lu, su = lm.score_word(sa, lm_dict.unk())
    assert lu == -math.inf and su not in (sa, sab)
    assert lexicon.word_unigram[a] == la and lexicon.word_unigram[lexicon.unk_word] == -math.inf     # smeared with the start row
    # naming a state costs nothing; asking a score of one evaluates it alone; prepare takes the rest in one extend()
    n0, c0 = lm.evaluated, lm.calls
    s1 = [lm.score_word(sab, int(lm.tok_word[w]))[1] for w in known[:3]]
    assert (lm.evaluated - n0, lm.calls - c0) == (0, 0)
    s2 = lm.score_word(s1[0], int(lm.tok_word[b]))[1]
    assert (lm.evaluated - n0, lm.calls - c0) == (1, 1)
    lm.prepare(s1 + [s2, sab, s1[0]])
    assert (lm.evaluated - n0, lm.calls - c0) == (4, 2)
    lm.prepare(s1 + [s2])
    assert (lm.evaluated - n0, lm.calls - c0) == (4, 2)
    row = lm._row(s2).copy()
    lm.drop_rows()
    assert np.array_equal(lm._row(s2), row) and lm.evaluated - n0 == 4           # rebuilt from the hidden row, not re-evaluated
    lm.empty_cache()
    assert len(lm.store) == 1 and lm.score_word(lm.start, int(lm.tok_word[a])) == (la, 1)


# --------------------------------------------------------------------------------------------------------- the search
def test_fused_decode_is_the_lexicon_search_with_the_scorer_plugged_in():
    """fused_lexicon_decode (prepare per frame, a cache emptied per utterance) returns exactly what lexicon_beam_search_reference
    returns with the same scorer in the Lexicon and no hook: the arithmetic is the same"""
    from unispeech_amd import ctc, ctc_lexicon as X
    from unispeech_amd.transformer_lm import incremental_reference
    x, il, d, lexicon, opts, _ = I.search_case(incremental_reference(C.build("A")))
    stats = {}
    got = X.fused_lexicon_decode(x, il, d, lexicon, lexicon.lm, normalized=True, stats=stats, **opts)
    x2, _, _, plain, _, _ = I.search_case(incremental_reference(C.build("A")))
    want = X.lexicon_beam_search_reference(x2, il, plain, d.bos(), ctc.silence_token(d), normalized=True, **opts)[0]
    assert [len(u) for u in got] == [I.SEARCH_NBEST] * 2
    for gu, wu in zip(got, want):
        assert len(gu) == len(wu)
        for (gw, gt, gs), (ww, wt, ws) in zip(gu, wu):
            assert gw == [plain.words[w] for w in ww] and gt == wt and gs == ws
    ref = I.search_reference()
    assert got == ref[0] and stats["states"] == ref[3]
    assert all(c <= x.shape[0] + 1 for c in stats["calls"])                      # at most one extend() per frame and one at the end
    assert plain.lm.calls == plain.lm.evaluated - 1 > max(stats["calls"])         # without the hook: one state per call
    with pytest.raises(ValueError, match="lexicon.lm"):
        X.fused_lexicon_decode(x, il, d, lexicon, plain.lm, normalized=True, **opts)
    # host emissions in either layout, and input lengths that cut an utterance short
    cut = X.fused_lexicon_decode(x, [5, 0], d, lexicon, lexicon.lm, normalized=True, **opts)
    assert cut[1] == [([], [], 0.2 * lexicon.lm.score_eos(lexicon.lm.start))] and len(cut[0][0][1]) <= 5


def test_the_float64_search_is_decided_by_more_than_twice_the_tolerance():
    """the margin condition of the GPU search test, from float64 alone: the smallest difference among the merges, the beam
    boundary and the n-best order between scores that are not exactly equal exceeds 2 x tol in every utterance, with
    tol = lm_weight x (longest word count + 1) x HEAD_TOL x max |log-prob|"""
    hyps, margins, mx, states, whole = I.search_reference()
    opts = dict(C.rescoring()[4], **I.SEARCH_OPTS)
    assert opts["beam_threshold"] == math.inf                                     # no threshold cut in this case
    tol = I.search_tol(hyps, I.HEAD_TOL * mx, opts["lm_weight"])
    print("margins", margins, "tol", tol, "max |log-prob|", mx, "states", states)
    assert len(margins) == 2 and all(0 < m < math.inf for m in margins)
    assert min(margins) > 2 * tol
    for utt, w in zip(hyps, whole):
        assert len(utt) == I.SEARCH_NBEST and len(w) >= len(utt)
        assert all(math.isfinite(h[2]) and len(h[0]) >= 2 for h in utt)
        assert [w[(tuple(h[0]), tuple(h[1]))] for h in utt] == [h[2] for h in utt]
    # the LM decides: two returned hypotheses of an utterance differ in a word and in nothing else
    assert any(a[1] == b[1] and a[0] != b[0] for utt in hyps for a in utt for b in utt)


def test_unequal_margins_leave_the_reported_margin_alone():
    """the additive hooks change no result of lexicon_beam_search_reference"""
    import ctc_lexicon_cases as L
    from unispeech_amd import ctc, ctc_lexicon as X
    x, il, d, lexicon, opts = L.case("beam63")
    seen, ne = [], []
    a = X.lexicon_beam_search_reference(x, il, lexicon, L.BLANK, ctc.silence_token(d), normalized=True, **opts)
    b = X.lexicon_beam_search_reference(x, il, lexicon, L.BLANK, ctc.silence_token(d), normalized=True, prepare=seen.append,
                                        unequal_margins=ne, **opts)
    assert a == b and len(seen) == sum(il) + len(il) and len(ne) == len(il)
    assert all(n >= m and n > 0 for n, m in zip(ne, a[1]))


# ------------------------------------------------------------------------------------------------------- command line
@pytest.mark.parametrize("extra, message", [
    (["--fuse-lm", "lm.pt"], "--fuse-lm and --fuse-dict go together"),
    (["--fuse-dict", "d.txt"], "--fuse-lm and --fuse-dict go together"),
    (["--fuse-lm", "lm.pt", "--fuse-dict", "d.txt", "--lm", "w.arpa"], "--fuse-lm and --lm are exclusive"),
    (["--fuse-lm", "lm.pt", "--fuse-dict", "d.txt", "--rescore-lm", "r.pt", "--rescore-dict", "r.txt"],
     "--fuse-lm and --rescore-lm are exclusive"),
])
@pytest.mark.parametrize("cmd", ["decode", "score"])
def test_command_line_refusals(cmd, extra, message, capsys):
    from unispeech_amd import ctc_lexicon as X
    args = [cmd, "ckpt.pt", "dict.txt"] + (["a.wav"] if cmd == "decode" else ["m.tsv", "m.ltr"]) + ["--lexicon", "lex.txt"]
    with pytest.raises(SystemExit) as e:
        X.parse_args(args + extra)
    assert e.value.code == 2 and message in capsys.readouterr().err
    ok = X.parse_args(args + ["--fuse-lm", "lm.pt", "--fuse-dict", "d.txt"])
    assert ok.fuse_lm == "lm.pt" and ok.fuse_dict == "d.txt" and ok.lm is None and ok.rescore_lm is None
