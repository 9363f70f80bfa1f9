"""csrc/ctc_beam.hip on the device against the float64 reference of the same call (ctc.beam_search_reference), hypothesis for
hypothesis: on the exact cases of tests/ctc_beam_cases.py the n-best token lists, their number and their SCORES are compared with
== (every partial score is a dyadic number fp32 holds exactly), so there is no tolerance in this file except for the one
normalized=False case, whose bound is derived in ctc_beam_cases.  Then the greedy decode, bf16 and both storage orders, batch
independence, and the `decode` / `score` commands with --lm on the tiny configuration of tests/test_ctc_gpu.py."""
import pytest
import torch

import ctc_beam_cases as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def leave_no_device_memory_behind():
    """as in tests/test_ctc_score_gpu.py: ops' grow-only workspaces are put back as they were and the cache is released, so that
    later modules meet the caching allocator as they did before this one existed.  The LMs of ctc_beam_cases keep their tables
    on the device (NgramLM.to caches them): the cached cases are dropped with them, or those small live tensors would leave
    half-used segments behind that the poisoned allocations of tests/gpu_checks.py do not expect"""
    import gc
    from unispeech_amd import ops
    saved = dict(ops._WS)
    yield
    torch.cuda.synchronize()
    ops._WS.clear()
    ops._WS.update(saved)
    for cached in (K.inexact, K.case, K.lm_of):
        cached.cache_clear()
    gc.collect()
    torch.cuda.empty_cache()


def _put(x, dtype=torch.float32, batch_first=True):
    x = x.to(dtype)
    if batch_first:
        return x.transpose(0, 1).contiguous().cuda().transpose(0, 1)     # the T x B x C view of batch-first storage: the model's
    return x.contiguous().cuda()                                         # T x B x C storage


def _device(name, dtype=torch.float32, batch_first=True, samples=None, x=None):
    from unispeech_amd.ctc import beam_decode
    x0, il, d, lm, opts = K.case(name)
    x = x0 if x is None else x
    if samples is not None:
        x, il = x[:, samples], [il[b] for b in samples]
    return beam_decode(_put(x, dtype, batch_first), il, d, lm, normalized=True, **opts)


# -------------------------------------------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("name", K.ALL)
def test_device_equals_the_reference(name):
    want = K.reference(name)
    got = _device(name)
    assert [len(h) for h in got] == [len(h) for h in want]                 # n_hyp
    for b, (g, w) in enumerate(zip(got, want)):
        assert [h[0] for h in g] == [h[0] for h in w], (name, b)           # tokens (and so the counts)
        assert [h[1] for h in g] == [h[1] for h in w], (name, b)           # scores, ==
    x, il, _, _, opts = K.case(name)
    assert all(len(h) >= 1 for h in got) and all(len(h) <= opts["nbest"] for h in got)
    if name == K.FLAT:
        assert [len(h) for h in got] == [3]
    if name == "lengths":                                                  # input length 0: one empty hypothesis, the end score
        assert got[0] == want[0] and len(got[0]) == 1 and got[0][0][0] == [] and got[4] == got[0]


def test_frames_behind_the_input_length_are_not_seen():
    """the same batch with other values behind each sample's length decodes alike"""
    x, il, _, _, _ = K.case("lengths")
    y = x.clone()
    for b, n in enumerate(il):
        y[n:, b] = torch.flip(y[n:, b], dims=[-1]) - 3.0
    assert not torch.equal(x, y)
    assert _device("lengths", x=y) == K.reference("lengths")


@pytest.mark.parametrize("beam", [1, 2, 5, 64])
def test_without_an_lm_the_one_best_is_the_greedy_decode(beam):
    from unispeech_amd.ctc import beam_decode, greedy_decode
    import ctc_score_cases as S
    for name in ("small", "words"):
        logits, il, _, decodes = S.batch(name)
        x = _put(logits)
        got = beam_decode(x, il, S.dictionary(), None, beam=beam, beam_size_token=7, beam_threshold=25.0)
        assert [h[0][0] for h in got] == greedy_decode(x, il, S.BLANK) == decodes


@pytest.mark.parametrize("name", ["beam63", "beam2_T257", "nolm"])
def test_bf16_logits_and_both_layouts(name):
    want = K.reference(name)
    for batch_first in (True, False):
        assert _device(name, torch.float32, batch_first) == want, batch_first
    xb = K.bf16_emissions(name)                                            # multiples of 2^-3 in [-8, 0]: exact in bf16
    assert torch.equal(xb.to(torch.bfloat16).float(), xb)
    want = K.reference(name, bf16=True)
    for batch_first in (True, False):
        assert _device(name, torch.bfloat16, batch_first, x=xb) == want, batch_first


def test_a_sample_alone_and_in_a_permuted_batch_and_twice():
    for name in ("lengths", "cut", "beam64"):
        a = _device(name)
        assert _device(name) == a
        B = len(a)
        for s in range(B):
            assert _device(name, samples=[s]) == [a[s]]
        perm = list(reversed(range(B)))
        assert _device(name, samples=perm) == [a[i] for i in perm]


def test_raw_logits_against_the_float64_reference():
    """normalized=False: the kernel subtracts each frame's log-sum-exp in fp32.  ctc_beam_cases.inexact() has asserted that every
    decision of the reference was taken by at least 64 x tol, tol = (T + 8) * 2^-23 * abs_sum (the forward error bound of an
    fp32 running sum plus the log-sum-exp's rounding per frame): the tokens are equal, the scores within tol."""
    from unispeech_amd.ctc import beam_decode
    logits, il, d, lm, ref, tol = K.inexact()
    for batch_first in (True, False):
        got = beam_decode(_put(logits, torch.float32, batch_first), il, d, lm, normalized=False, **K.INEXACT_OPTS)
        for b, (g, w) in enumerate(zip(got, ref)):
            assert [h[0] for h in g] == [h[0] for h in w], b
            err = [abs(x[1] - y[1]) for x, y in zip(g, w)]
            print("sample %d: score error %s, tol %.3g" % (b, err, tol[b]))
            assert max(err) <= tol[b], (b, err, tol[b])


def test_ops_returns_device_tensors_and_refuses_by_name():
    from unispeech_amd import ops
    x, il, d, lm, opts = K.case("beam63")
    xd = _put(x).transpose(0, 1)
    ild = torch.tensor(il, dtype=torch.int32).cuda()
    tokens, counts, scores, n_hyp = ops.ctc_beam(xd, ild, K.BLANK, K.BAR, lm, 63, 11, K.INF, 1.0, 0.0, 3, True)
    B, T = x.shape[1], x.shape[0]
    assert tokens.is_cuda and tokens.shape == (B, 3, T) and tokens.dtype == torch.int32 and counts.shape == (B, 3)
    assert scores.dtype == torch.float32 and n_hyp.cpu().tolist() == [3] * B
    tok, cnt = tokens.cpu(), counts.cpu()
    for b, hyps in enumerate(K.reference("beam63")):
        for h, (seq, sc) in enumerate(hyps):
            assert tok[b, h, :cnt[b, h]].tolist() == seq and (tok[b, h, cnt[b, h]:] == -1).all() and float(scores[b, h]) == sc
    with pytest.raises(NotImplementedError, match="beam = 513"):
        ops.ctc_beam(xd, ild, K.BLANK, K.BAR, lm, 513, 11, K.INF, 1.0, 0.0, 3, True)
    with pytest.raises(NotImplementedError, match="beam_size_token = 33"):
        ops.ctc_beam(torch.zeros(1, 2, 64, device="cuda"), ild[:1], K.BLANK, -1, None, 512, 33, K.INF, 1.0, 0.0, 1, True)
    with pytest.raises(ValueError, match="nbest"):
        ops.ctc_beam(xd, ild, K.BLANK, K.BAR, lm, 2, 11, K.INF, 1.0, 0.0, 3, True)
    with pytest.raises(ValueError, match="input_lengths"):
        ops.ctc_beam(xd, ild.long(), K.BLANK, K.BAR, lm, 2, 11, K.INF, 1.0, 0.0, 1, True)


# -------------------------------------------------------------------------------------------------------------- end to end
def test_decode_and_score_commands_with_an_lm(tmp_path, capsys):
    """two synthetic wavs, a dictionary, a trigram written here: `decode --lm` and `score --lm` print what beam_decode of the
    model's own logits gives, and without --lm both print what they print today (the greedy decode)"""
    import wave
    from test_ctc_gpu import NCLS, _tiny_ctc
    from conftest import TINY
    from unispeech_amd import ctc, ctc_lm
    from unispeech_amd.kmeans import read_wav
    model, _, sample = _tiny_ctc()
    syms = ["|"] + [chr(ord("A") + i) for i in range(NCLS - 5)]
    (tmp_path / "dict.ltr.txt").write_text("".join("%s 1\n" % c for c in syms))
    torch.save({"cfg": dict(TINY), "model": model.state_dict(), "arch": "wavlm", "normalize": False}, str(tmp_path / "ck.pt"))
    arpa = str(tmp_path / "lm.arpa")
    ctc_lm.write_arpa(arpa, 3, K.random_entries(3, syms[:-1], 3))          # the last symbol is not in the LM
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
    lm = ctc_lm.NgramLM.load(arpa, d)
    loaded, _ = ctc.load_ctc_checkpoint(str(tmp_path / "ck.pt"), len(d))
    kw = {"beam": 20, "beam_size_token": 6, "beam_threshold": 30.0, "lm_weight": 1.5, "sil_weight": -0.5}
    flags = ["--lm", arpa, "--beam", "20", "--beam-size-token", "6", "--beam-threshold", "30", "--lm-weight", "1.5",
             "--sil-weight", "-0.5"]

    def logits_of(path):
        x = torch.as_tensor(read_wav(path)[0], dtype=torch.float32).cuda()
        with torch.no_grad():
            return loaded(source=x.view(1, -1), padding_mask=None)["encoder_out"]
    # decode
    head = ["decode", str(tmp_path / "ck.pt"), str(tmp_path / "dict.ltr.txt")] + wavs
    assert ctc.main(head) == 0
    plain = capsys.readouterr().out
    assert plain == "".join(ctc.post_process(d.string(ctc.greedy_decode(logits_of(p), None, d.bos())[0]), "letter") + "\n"
                            for p in wavs)
    assert ctc.main(head + flags + ["--nbest", "2"]) == 0
    out = capsys.readouterr().out.splitlines()
    want = []
    for p in wavs:
        hyps = ctc.beam_decode(logits_of(p), None, d, lm, nbest=2, **kw)[0]
        assert len(hyps) == 2 and hyps[0][1] >= hyps[1][1]
        want += ["%.4f\t%s" % (sc, ctc.post_process(d.string(toks), "letter")) for toks, sc in hyps]
    assert out == want
    # score: the same padded batch by hand, shortest first
    argv = ["score", str(tmp_path / "ck.pt"), str(tmp_path / "dict.ltr.txt"), str(tmp_path / "t.tsv"), str(tmp_path / "t.ltr")]
    assert ctc.main(argv) == 0
    plain = capsys.readouterr().out
    src, pm = torch.zeros(2, 8000), torch.ones(2, 8000, dtype=torch.bool)
    for r, i in enumerate((1, 0)):
        w = torch.as_tensor(read_wav(wavs[i])[0], dtype=torch.float32)
        src[r, :w.numel()] = w
        pm[r, :w.numel()] = False
    with torch.no_grad():
        o = loaded(source=src.cuda(), padding_mask=pm.cuda())
    il = (~o["padding_mask"]).sum(-1)
    labels = [[d.index(s) for s in "B | D".split()], [d.index(s) for s in "A B | C A B |".split()]]
    target = torch.full((2, 7), d.pad(), dtype=torch.long)
    for r, row in enumerate(labels):
        target[r, :len(row)] = torch.tensor(row)
    g = ctc.error_counts(o["encoder_out"], il, target, d)
    assert plain.strip().splitlines()[-1].split()[4:] == ["c_errors", str(g["c_errors"]), "c_total", "10", "w_errors",
                                                          str(g["w_errors"]), "w_total", "4"]
    res = tmp_path / "res"
    assert ctc.main(argv + flags + ["--results", str(res)]) == 0
    line = capsys.readouterr().out.strip().splitlines()[-1].split()
    hyps = [h[0][0] for h in ctc.beam_decode(o["encoder_out"], il, d, lm, **kw)]
    c_err = sum(ctc.edit_distance(h, t) for h, t in zip(hyps, labels))
    w_err = sum(ctc.edit_distance(ctc.post_process(d.string(h), "letter").split(), ctc.post_process(d.string(t), "letter").split())
                for h, t in zip(hyps, labels))
    assert line[4:] == ["c_errors", str(c_err), "c_total", "10", "w_errors", str(w_err), "w_total", "4"]
    assert (res / "hypo.units").read_text().splitlines() == ["%s (None-%d)" % (d.string(hyps[1 - i]), i) for i in (0, 1)]
