"""csrc/ctc_lexbeam.hip on the device against the float64 reference of the same call (ctc_lexicon.lexicon_beam_search_reference),
hypothesis for hypothesis: on the exact cases of tests/ctc_lexicon_cases.py the n-best words, tokens, their number and their
SCORES are compared with == (every partial score is a dyadic number fp32 holds exactly), so there is no tolerance in this file
except for the one normalized=False case, whose bound is derived in ctc_lexicon_cases.  Then bf16 and both storage orders, batch
independence, and the `decode` / `score` commands on the tiny configuration of tests/test_ctc_gpu.py against the float64 search on
the host copy of the same logits."""
import pytest
import torch

import ctc_beam_cases as K
import ctc_lexicon_cases as L

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def leave_no_device_memory_behind():
    """as in tests/test_ctc_beam_gpu.py: ops' grow-only workspaces are put back as they were, the cached cases (whose lexicons and
    LMs keep their tables on the device) are dropped and the cache is released"""
    import gc
    from unispeech_amd import ops
    saved = dict(ops._WS)
    yield
    torch.cuda.synchronize()
    ops._WS.clear()
    ops._WS.update(saved)
    for cached in (L.inexact, L.reference, L.case, L.lexicon_of):
        cached.cache_clear()
    gc.collect()
    torch.cuda.empty_cache()


def _put(x, dtype=torch.float32, batch_first=True):
    x = x.to(dtype)
    if batch_first:
        return x.transpose(0, 1).contiguous().cuda().transpose(0, 1)     # the T x B x C view of batch-first storage: the model's
    return x.contiguous().cuda()                                         # T x B x C storage


def _device(name, dtype=torch.float32, batch_first=True, samples=None, x=None):
    from unispeech_amd.ctc_lexicon import lexicon_beam_decode
    x0, il, d, lexicon, opts = L.case(name)
    x = x0 if x is None else x
    if samples is not None:
        x, il = x[:, samples], [il[b] for b in samples]
    return lexicon_beam_decode(_put(x, dtype, batch_first), il, d, lexicon, lexicon.lm, normalized=True, **opts)


# -------------------------------------------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("name", L.ALL)
def test_device_equals_the_reference(name):
    want = L.reference(name)
    got = _device(name)
    assert [len(h) for h in got] == [len(h) for h in want]                 # n_hyp
    for b, (g, w) in enumerate(zip(got, want)):
        assert [h[0] for h in g] == [h[0] for h in w], (name, b)           # words (and so the word counts)
        assert [h[1] for h in g] == [h[1] for h in w], (name, b)           # tokens (and so the counts)
        assert [h[2] for h in g] == [h[2] for h in w], (name, b)           # scores, ==
    x, il, _, _, opts = L.case(name)
    assert all(len(h) >= 1 for h in got) and all(len(h) <= opts["nbest"] for h in got)
    if name == L.FLAT:
        assert [len(h) for h in got] == [3]
    if name == "lengths":                                                  # input length 0: one empty hypothesis, the end score
        assert got[0] == want[0] and len(got[0]) == 1 and got[0][0][:2] == ([], []) and got[4] == got[0]
    if name == "noroot":                                                   # nobody at the root: everybody finishes
        assert got[0][0][:2] == ([], [5, 6])


def test_frames_behind_the_input_length_are_not_seen():
    """the same batch with other values behind each sample's length decodes alike"""
    x, il, _, _, _ = L.case("lengths")
    y = x.clone()
    for b, n in enumerate(il):
        y[n:, b] = torch.flip(y[n:, b], dims=[-1]) - 3.0
    assert not torch.equal(x, y)
    assert _device("lengths", x=y) == L.reference("lengths")


@pytest.mark.parametrize("name", ["beam63", "beam1_T257", "nolm", "cap_big_edge"])
def test_bf16_logits_and_both_layouts(name):
    want = L.reference(name)
    for batch_first in (True, False):
        assert _device(name, torch.float32, batch_first) == want, batch_first
    xb = L.bf16_emissions(name)                                            # multiples of 2^-3 in [-8, 0]: exact in bf16
    assert torch.equal(xb.to(torch.bfloat16).float(), xb)
    want = L.reference(name, bf16=True)
    for batch_first in (True, False):
        assert _device(name, torch.bfloat16, batch_first, x=xb) == want, batch_first


def test_a_sample_alone_and_in_a_permuted_batch_and_twice():
    for name in ("lengths", "cut", "beam64", "cap_big_edge"):
        a = _device(name)
        assert _device(name) == a
        B = len(a)
        for s in range(B):
            assert _device(name, samples=[s]) == [a[s]]
        perm = list(reversed(range(B)))
        assert _device(name, samples=perm) == [a[i] for i in perm]


def test_raw_logits_against_the_float64_reference():
    """normalized=False: the kernel subtracts each frame's log-sum-exp in fp32.  ctc_lexicon_cases.inexact() has asserted that
    every decision of the reference was taken by at least 64 x tol, tol = (T + 8) * 2^-23 * abs_sum (the forward error bound of
    an fp32 running sum plus the log-sum-exp's rounding per frame): words and tokens are equal, the scores within tol."""
    from unispeech_amd.ctc_lexicon import lexicon_beam_decode
    logits, il, d, lexicon, ref, tol = L.inexact()
    for batch_first in (True, False):
        got = lexicon_beam_decode(_put(logits, torch.float32, batch_first), il, d, lexicon, lexicon.lm, normalized=False,
                                  **L.INEXACT_OPTS)
        for b, (g, w) in enumerate(zip(got, ref)):
            assert [h[:2] for h in g] == [h[:2] for h in w], b
            err = [abs(x[2] - y[2]) for x, y in zip(g, w)]
            print("sample %d: score error %s, tol %.3g" % (b, err, tol[b]))
            assert max(err) <= tol[b], (b, err, tol[b])


def test_ops_returns_device_tensors_and_refuses_by_name():
    from unispeech_amd import ops
    x, il, d, lexicon, opts = L.case("beam63")
    xd = _put(x).transpose(0, 1)
    ild = torch.tensor(il, dtype=torch.int32).cuda()
    tokens, counts, scores, n_hyp, words, word_counts = ops.ctc_lexbeam(xd, ild, L.BLANK, L.BAR, lexicon, 63, 11, L.INF, 1.0, 1.0,
                                                                        -1.0, 0.0, 3, True)
    B, T = x.shape[1], x.shape[0]
    assert tokens.is_cuda and tokens.shape == (B, 3, T) and tokens.dtype == torch.int32 and counts.shape == (B, 3)
    assert words.is_cuda and words.shape == (B, 3, T) and words.dtype == torch.int32 and word_counts.shape == (B, 3)
    assert scores.dtype == torch.float32 and n_hyp.cpu().tolist() == [3] * B
    tok, cnt, wd, wcnt = tokens.cpu(), counts.cpu(), words.cpu(), word_counts.cpu()
    for b, hyps in enumerate(L.reference("beam63")):
        for h, (wds, seq, sc) in enumerate(hyps):
            assert tok[b, h, :cnt[b, h]].tolist() == seq and (tok[b, h, cnt[b, h]:] == -1).all() and float(scores[b, h]) == sc
            assert [lexicon.words[w] for w in wd[b, h, :wcnt[b, h]].tolist()] == wds and (wd[b, h, wcnt[b, h]:] == -1).all()
    with pytest.raises(NotImplementedError, match="beam = 513"):
        ops.ctc_lexbeam(xd, ild, L.BLANK, L.BAR, lexicon, 513, 11, L.INF, 1.0, 1.0, -1.0, 0.0, 3, True)
    from unispeech_amd.ctc_lexicon import Lexicon
    d32 = K.dictionary(32)                                                 # 27 letters, each a word and the head of another
    wide = Lexicon(["x%d" % t for t in range(5, 32)] + ["y%d" % t for t in range(5, 32)] + ["<unk>"],
                   [(t - 5, (t,)) for t in range(5, 32)] + [(27 + t - 5, (t, 5)) for t in range(5, 32)], d32)
    width = wide.width(32, False)
    assert width == 57 and 287 * width <= L.CAP < 288 * width
    with pytest.raises(NotImplementedError, match="beam = 288"):          # one past beam x width = CAP
        ops.ctc_lexbeam(torch.zeros(1, 2, 32, device="cuda"), ild[:1], L.BLANK, L.BAR, wide, 288, 32, L.INF, 1.0, 1.0, -L.INF, 0.0,
                        1, True)
    with pytest.raises(ValueError, match="nbest"):
        ops.ctc_lexbeam(xd, ild, L.BLANK, L.BAR, lexicon, 2, 11, L.INF, 1.0, 1.0, -1.0, 0.0, 3, True)
    with pytest.raises(ValueError, match="input_lengths"):
        ops.ctc_lexbeam(xd, ild.long(), L.BLANK, L.BAR, lexicon, 2, 11, L.INF, 1.0, 1.0, -1.0, 0.0, 1, True)


# -------------------------------------------------------------------------------------------------------------- end to end
HEAD_SCALE = 10.0        # the CTC head's weight is multiplied by this: an untrained head gives nearly flat logits and no words;
#                          with the head scaled and a narrow beam every decision of the float64 search is taken by more than
#                          64 x tol (asserted in _host), so the fp32 search has to take the same ones
E2E = {"beam": 3, "beam_size_token": 3, "beam_threshold": K.INF, "lm_weight": 1.5, "word_score": -0.5, "unk_weight": -4.0,
       "sil_weight": -0.25}


def _e2e_setup(tmp_path, head_scale=HEAD_SCALE):
    """two synthetic wavs, a manifest and labels, a dictionary, a lexicon and a trigram over its words, and a tiny checkpoint
    whose head is scaled: (dictionary, Lexicon, loaded model, wav paths, labels, the files' paths)"""
    import wave
    from test_ctc_gpu import NCLS, _tiny_ctc
    from conftest import TINY
    from unispeech_amd import ctc, ctc_lexicon, ctc_lm
    model, _, sample = _tiny_ctc()
    sd = model.state_dict()
    heads = [k for k, v in sd.items() if k.endswith("proj.weight") and v.shape[0] == NCLS]
    assert len(heads) == 1
    sd[heads[0]] = sd[heads[0]] * head_scale
    syms = ["|"] + [chr(ord("A") + i) for i in range(NCLS - 5)]
    (tmp_path / "dict.ltr.txt").write_text("".join("%s 1\n" % c for c in syms))
    torch.save({"cfg": dict(TINY), "model": sd, "arch": "wavlm", "normalize": False}, str(tmp_path / "ck.pt"))
    letters = syms[1:]
    vocab = list(letters) + [a + b for a in letters[:4] for b in letters[:4]]
    (tmp_path / "lex.txt").write_text("".join("%s %s |\n" % (w, " ".join(w)) for w in vocab) + "AB2 A B |\n")
    arpa = str(tmp_path / "lm.arpa")
    ctc_lm.write_arpa(arpa, 3, K.random_entries(3, vocab[::2], 3, 0.2))
    lines, wavs = ["%s" % tmp_path], []
    for i, n in enumerate((8000, 5000)):
        pcm = (sample["net_input"]["source"][i, :n].float().cpu().clamp(-1, 1) * 3000).to(torch.int16).numpy()
        with wave.open(str(tmp_path / ("u%d.wav" % i)), "wb") as w:
            w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000); w.writeframes(pcm.tobytes())
        lines.append("u%d.wav\t%d" % (i, n))
        wavs.append(str(tmp_path / ("u%d.wav" % i)))
    (tmp_path / "t.tsv").write_text("\n".join(lines) + "\n")
    (tmp_path / "t.ltr").write_text("A B | C A B |\nB | D\n")
    d = ctc.LetterDictionary.load(str(tmp_path / "dict.ltr.txt"))
    lexicon = ctc_lexicon.Lexicon.load(str(tmp_path / "lex.txt"), d, arpa)
    loaded, _ = ctc.load_ctc_checkpoint(str(tmp_path / "ck.pt"), len(d))
    labels = [[d.index(s) for s in "A B | C A B |".split()], [d.index(s) for s in "B | D".split()]]
    return d, lexicon, loaded, wavs, labels, arpa


def _e2e_logits(loaded, wavs):
    """(the logits of each file alone, the logits and input lengths of the padded batch `score` forms: shortest first)"""
    from unispeech_amd.kmeans import read_wav
    audio = [torch.as_tensor(read_wav(p)[0], dtype=torch.float32) for p in wavs]
    src, pm = torch.zeros(2, 8000), torch.ones(2, 8000, dtype=torch.bool)
    for r, i in enumerate((1, 0)):
        src[r, :audio[i].numel()] = audio[i]
        pm[r, :audio[i].numel()] = False
    with torch.no_grad():
        single = [loaded(source=x.cuda().view(1, -1), padding_mask=None)["encoder_out"] for x in audio]
        o = loaded(source=src.cuda(), padding_mask=pm.cuda())
    return single, o["encoder_out"], (~o["padding_mask"]).sum(-1)


def _host(logits, il, d, lexicon, nbest, kw=None):
    """the float64 search on the host copy of the logits: per sample (hypotheses with word strings, tol), after asserting that
    every decision was taken by at least 64 x tol, tol = (T + 8) * 2^-23 * abs_sum as in ctc_lexicon_cases.inexact() -- so the
    fp32 search must have taken the same decisions"""
    from unispeech_amd import ctc, ctc_lexicon
    x = logits.float().cpu()
    lens = None if il is None else [int(v) for v in il.cpu()]
    ref, margin, abs_sum = ctc_lexicon.lexicon_beam_search_reference(x, lens, lexicon, d.bos(), ctc.silence_token(d), nbest=nbest,
                                                                     **(E2E if kw is None else kw))
    out = []
    for b, hyps in enumerate(ref):
        tol = (x.shape[0] + 8) * 2.0 ** -23 * abs_sum[b]
        print("sample %d: margin %.3g, 64 x tol %.3g" % (b, margin[b], 64 * tol))
        assert margin[b] >= 64 * tol, (b, margin[b], tol)
        out.append(([([lexicon.words[w] for w in wds], toks, sc) for wds, toks, sc in hyps], tol))
    return out


def test_decode_and_score_commands(tmp_path, capsys):
    """`decode` and `score` on a tiny checkpoint print the words, scores and error counts of the float64 host search on the same
    logits; the device search underneath them agrees with it hypothesis for hypothesis"""
    from unispeech_amd import ctc, ctc_lexicon
    d, lexicon, loaded, wavs, labels, arpa = _e2e_setup(tmp_path)
    single, batch, il = _e2e_logits(loaded, wavs)
    flags = ["--lexicon", str(tmp_path / "lex.txt"), "--lm", arpa, "--beam", "3", "--beam-size-token", "3", "--beam-threshold",
             "inf", "--lm-weight", "1.5", "--word-score", "-0.5", "--unk-weight", "-4", "--sil-weight", "-0.25"]
    host = [_host(x, None, d, lexicon, 2)[0] for x in single]
    capsys.readouterr()
    # decode
    head = ["decode", str(tmp_path / "ck.pt"), str(tmp_path / "dict.ltr.txt")] + wavs
    assert ctc_lexicon.main(head + flags + ["--nbest", "2"]) == 0
    out = capsys.readouterr().out.splitlines()
    assert len(out) == sum(len(h) for h, _ in host) and all(1 <= len(h) <= 2 for h, _ in host)   # (only those at the root finish)
    k = 0
    for (hyps, tol), x in zip(host, single):
        dev = ctc_lexicon.lexicon_beam_decode(x, None, d, lexicon, lexicon.lm, nbest=2, **E2E)[0]
        assert [h[:2] for h in dev] == [h[:2] for h in hyps]
        for (words, _, sc), (_, _, dsc) in zip(hyps, dev):
            score, text = out[k].split("\t")
            assert text == " ".join(words) and abs(dsc - sc) <= tol and score == "%.4f" % dsc
            k += 1
    assert ctc_lexicon.main(head + flags) == 0
    assert capsys.readouterr().out.splitlines() == [" ".join(h[0][0]) for h, _ in host]
    # score: the host search on the padded batch (shortest first), its counts by the host edit distance
    hb = [h[0] for h, _ in _host(batch, il, d, lexicon, 1)]
    capsys.readouterr()
    order = (1, 0)                                                          # row r of the batch is utterance order[r]
    c_err = sum(ctc.edit_distance(h[1], labels[i]) for h, i in zip(hb, order))
    w_err = sum(ctc.edit_distance(h[0], ctc.post_process(d.string(labels[i]), "letter").split()) for h, i in zip(hb, order))
    argv = ["score", str(tmp_path / "ck.pt"), str(tmp_path / "dict.ltr.txt"), str(tmp_path / "t.tsv"), str(tmp_path / "t.ltr")]
    res = tmp_path / "res"
    assert ctc_lexicon.main(argv + flags + ["--results", str(res)]) == 0
    line = capsys.readouterr().out.strip().splitlines()[-1].split()
    assert line[4:] == ["c_errors", str(c_err), "c_total", "10", "w_errors", str(w_err), "w_total", "4"]
    by_utt = {i: h for h, i in zip(hb, order)}
    assert (res / "hypo.units").read_text().splitlines() == ["%s (None-%d)" % (d.string(by_utt[i][1]), i) for i in (0, 1)]
    assert (res / "hypo.word").read_text().splitlines() == ["%s (None-%d)" % (" ".join(by_utt[i][0]), i) for i in (0, 1)]
    assert (res / "ref.word").read_text().splitlines() == ["AB CAB (None-0)", "B D (None-1)"]
    assert sorted(p.name for p in res.iterdir()) == ["hypo.units", "hypo.word", "ref.units", "ref.word"]
