"""csrc/ctc_score.hip on the device: wavlm_ctc_score's [B, 4] counts against the host path of the same call (greedy_decode + the
pure-Python edit_distance, which tests/test_ctc_score.py pins to a full-matrix Levenshtein), per sample, integer for integer --
there is no tolerance anywhere in this file.  The batches, and which boundary of the kernel each one stands on, are in
tests/ctc_score_cases.py; the host counts are computed once per process there.  Then EncoderCtc + CtcCriterion, Unispeech +
UnispeechCriterion and the `score` command end to end on the tiny configurations of tests/test_ctc_gpu.py and
tests/test_unispeech_gpu.py."""
import os

import numpy as np
import pytest
import torch

import ctc_score_cases as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def leave_no_device_memory_behind():
    """ops' grow-only workspaces are cached for the life of the process.  Put them back as they were when this module is done
    (the ones it grew and the ones its models were the first to ask for) and release the cache, so that later modules meet the
    caching allocator as they did before this one existed: the poisoned allocations of tests/gpu_checks.py count on that"""
    import gc
    from unispeech_amd import ops
    saved = dict(ops._WS)
    yield
    torch.cuda.synchronize()
    ops._WS.clear()
    ops._WS.update(saved)
    gc.collect()
    torch.cuda.empty_cache()


def _device(name, post_process, dtype=torch.float32, batch_first=True, samples=None):
    """sample_error_counts of the batch on the device: ([B, 4], decodes)"""
    from unispeech_amd.ctc import sample_error_counts
    logits, il, targets, _ = K.batch(name)
    if samples is not None:
        logits, il, targets = logits[:, samples], [il[b] for b in samples], targets[samples]
    x = logits.to(dtype)
    if batch_first:
        x = x.transpose(0, 1).contiguous().cuda().transpose(0, 1)        # the T x B x C view of batch-first storage: the model's
    else:
        x = x.contiguous().cuda()                                        # T x B x C storage
    return sample_error_counts(x, il, targets.cuda(), K.dictionary(), post_process)


# -------------------------------------------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("post_process", ["letter", None])
@pytest.mark.parametrize("name", K.ALL)
def test_counts_equal_the_host_path(name, post_process, monkeypatch):
    want, decoded = K.host_counts(name, post_process)
    got, dev_decoded = _device(name, post_process)
    assert dev_decoded == decoded
    assert got.tolist() == want.tolist()                                  # the [B, 4] array, not its sums
    # and the host path of the very same call: device logits, the switch set
    monkeypatch.setenv("WAVLM_CTC_SCORE_HOST", "1")
    host, host_decoded = _device(name, post_process)
    assert host.tolist() == want.tolist() and host_decoded == decoded


@pytest.mark.parametrize("name", ["small", "words", "per4_65", "per16_300"])
def test_bf16_logits_and_both_layouts(name):
    want, decoded = K.host_counts(name, "letter")
    for dtype in (torch.float32, torch.bfloat16):
        for batch_first in (True, False):
            got, dec = _device(name, "letter", dtype, batch_first)
            assert got.tolist() == want.tolist() and dec == decoded, (dtype, batch_first)


def test_a_sample_alone_and_in_the_batch_and_twice():
    for name in ("words", "per16_65"):
        a, a_dec = _device(name, "letter")
        b, b_dec = _device(name, "letter")
        assert np.array_equal(a, b) and a_dec == b_dec
        for s in (0, 4, 7):
            one, one_dec = _device(name, "letter", samples=[s])
            assert one.tolist() == [a[s].tolist()] and one_dec == [a_dec[s]]
        perm = [5, 2, 7, 0, 1, 6, 3, 4]
        p, p_dec = _device(name, "letter", samples=perm)
        assert p.tolist() == a[perm].tolist() and p_dec == [a_dec[i] for i in perm]


def _raw_args(name, post_process):
    from unispeech_amd import ctc
    logits, il, targets, _ = K.batch(name)
    x = logits.transpose(0, 1).contiguous().cuda()
    il = torch.tensor(il, dtype=torch.int32).cuda()
    t = targets.to(torch.int32).cuda().contiguous()
    cls = torch.from_numpy(ctc.word_classes(K.dictionary(), K.C, post_process)).cuda()
    return x, il, t, cls


def test_tokens_are_the_greedy_decodes_and_ops_returns_device_tensors():
    from unispeech_amd import ops
    for name in ("small", "per4_300"):
        x, il, t, cls = _raw_args(name, "letter")
        counts, tokens, token_counts = ops.ctc_score(x, il, t, K.PAD, K.EOS, K.BLANK, cls, False)
        g_tokens, g_counts = ops.ctc_greedy(x, il, K.BLANK)
        assert counts.is_cuda and counts.dtype == torch.int32 and counts.shape == (x.shape[0], 4)
        assert torch.equal(tokens, g_tokens) and torch.equal(token_counts, g_counts)
        assert counts.cpu().tolist() == K.host_counts(name, "letter")[0].tolist()
    x, il, t, cls = _raw_args("small", "letter")
    with pytest.raises(ValueError, match="cls"):
        ops.ctc_score(x, il, t, K.PAD, K.EOS, K.BLANK, cls[:5], False)
    with pytest.raises(ValueError, match="targets"):
        ops.ctc_score(x, il, t.long(), K.PAD, K.EOS, K.BLANK, cls, False)
    with pytest.raises(NotImplementedError, match="Lt = 1025"):
        ops.ctc_score(x, il, torch.ones(8, 1025, dtype=torch.int32, device="cuda"), K.PAD, K.EOS, K.BLANK, cls, False)


@pytest.mark.parametrize("name", ["words", "per16_64"])
def test_guard_bands_stay_intact_and_bad_arguments_are_refused(name):
    """tokens, counts, the [B, 4] output and the workspace sit inside larger buffers filled with a sentinel"""
    from unispeech_amd import _lib, ops
    L = _lib.lib()
    x, il, t, cls = _raw_args(name, "letter")
    B, T, C = x.shape
    Lt = t.shape[1]
    G, S = 64, -7777
    need = L.wavlm_ctc_score_workspace_bytes(B, T, Lt)
    tokens = torch.full((G + B * T + G,), S, dtype=torch.int32, device="cuda")
    counts = torch.full((G + B + G,), S, dtype=torch.int32, device="cuda")
    out = torch.full((G + 4 * B + G,), S, dtype=torch.int32, device="cuda")
    ws = torch.full((G + need // 4 + G,), S, dtype=torch.int32, device="cuda")

    def call(**over):
        a = dict(x=ops.ptr(x), dt=ops.dt(x), sb=x.stride(0), st=x.stride(1), B=B, T=T, C=C, il=ops.ptr(il), blank=K.BLANK,
                 t=ops.ptr(t), Lt=Lt, pad=K.PAD, eos=K.EOS, cls=ops.ptr(cls), each=0, tokens=ops.ptr(tokens, G),
                 counts=ops.ptr(counts, G), out=ops.ptr(out, G), ws=ops.ptr(ws, G), need=need)
        a.update(over)
        return L.wavlm_ctc_score(a["x"], a["dt"], a["sb"], a["st"], a["B"], a["T"], a["C"], a["il"], a["blank"], a["t"], a["Lt"],
                                 a["pad"], a["eos"], a["cls"], a["each"], a["tokens"], a["counts"], a["out"], a["ws"], a["need"],
                                 ops.stream())
    # refused before anything is launched: the library's invalid-argument code
    assert call(T=0) == -1 and call(Lt=1025) == -1 and call(Lt=-1) == -1 and call(need=need - 1) == -1
    assert call(cls=None) == -1 and call(out=None) == -1 and call(ws=None) == -1 and call(blank=C) == -1 and call(dt=7) == -1
    assert call(st=C - 1) == -1
    torch.cuda.synchronize()
    for buf in (tokens, counts, out, ws):
        assert (buf == S).all()
    assert call() == 0
    torch.cuda.synchronize()
    for buf, n in ((tokens, B * T), (counts, B), (out, 4 * B), (ws, need // 4)):
        assert (buf[:G] == S).all() and (buf[G + n:] == S).all()
    want, decoded = K.host_counts(name, "letter")
    assert out[G:G + 4 * B].view(B, 4).cpu().tolist() == want.tolist()
    assert counts[G:G + B].cpu().tolist() == [len(d) for d in decoded]
    tok = tokens[G:G + B * T].view(B, T).cpu()
    for b, d in enumerate(decoded):
        assert tok[b, :len(d)].tolist() == d and (tok[b, len(d):] == -1).all()


# -------------------------------------------------------------------------------------------------------------- end to end
def _no_host_dp(monkeypatch):
    from unispeech_amd import ctc

    def refuse(a, b):
        raise AssertionError("the host edit distance ran")
    monkeypatch.setattr(ctc, "edit_distance", refuse)


@pytest.mark.parametrize("kind", ["indices", "letters"])
def test_e2e_criterion_device_path_equals_the_host_path(kind, monkeypatch):
    from test_ctc_gpu import NCLS, _tiny_ctc
    from unispeech_amd import ctc
    model, crit, sample = _tiny_ctc()
    if kind == "letters":                                   # 4 specials + 8 symbols = NCLS classes, post_process = "letter"
        crit = ctc.CtcCriterion(ctc.LetterDictionary(["|"] + [chr(ord("A") + i) for i in range(NCLS - 5)]), zero_infinity=True)
    model.eval()
    with torch.no_grad():
        monkeypatch.setenv("WAVLM_CTC_SCORE_HOST", "1")
        _, _, host = crit(model, sample)
        monkeypatch.delenv("WAVLM_CTC_SCORE_HOST")
        _, _, dev = crit(model, sample)
        assert dev == host and dev["c_total"] == 8 and dev["wv_errors"] == dev["w_errors"]
        assert crit._classes(NCLS, sample["target"].device) is not None
        _no_host_dp(monkeypatch)
        _, _, again = crit(model, sample)                   # the host DP is off the path
        assert again == host
        monkeypatch.setenv("WAVLM_CTC_SCORE_HOST", "1")
        with pytest.raises(AssertionError, match="host edit distance"):
            crit(model, sample)


def test_e2e_unispeech_criterion_takes_the_device_path(monkeypatch):
    from unispeech_cases import build, sample_of
    m, crit, z = build("tiny_unispeech.npz", "cuda")
    assert crit.mtlalpha > 0
    m.eval()
    sample = sample_of(z, "cuda")

    def seed():                                             # the replace draw of the model: the same for both passes
        from unispeech_amd import functional as F
        np.random.seed(77)
        torch.manual_seed(31)
        F._SEED_CTR[0] = 0
    with torch.no_grad():
        monkeypatch.setenv("WAVLM_CTC_SCORE_HOST", "1")
        seed()
        _, _, host = crit(m, sample)
        monkeypatch.delenv("WAVLM_CTC_SCORE_HOST")
        _no_host_dp(monkeypatch)
        seed()
        _, _, dev = crit(m, sample)
    for k in ("c_errors", "c_total", "w_errors", "wv_errors", "w_total"):
        assert dev["ctc"][k] == host["ctc"][k], k
    for k in ("c_errors", "c_total", "w_errors", "w_total"):                        # and the reference's own counts
        assert dev["ctc"][k] == int(z["eval/" + k]), k


def test_score_command(tmp_path, capsys):
    """two synthetic wavs, a manifest and a label file written here: the printed totals are error_counts of the same padded batch
    through the loaded model, and the four result files hold what the same launch decoded"""
    import wave
    from test_ctc_gpu import NCLS, _tiny_ctc
    from conftest import TINY
    from unispeech_amd import ctc
    from unispeech_amd.kmeans import read_wav
    model, _, sample = _tiny_ctc()
    syms = ["|"] + [chr(ord("A") + i) for i in range(NCLS - 5)]
    (tmp_path / "dict.ltr.txt").write_text("".join("%s 1\n" % c for c in syms))
    torch.save({"cfg": dict(TINY), "model": model.state_dict(), "arch": "wavlm", "normalize": False}, str(tmp_path / "ck.pt"))
    lines = ["%s" % tmp_path]
    for i, n in enumerate((8000, 5000)):
        pcm = (sample["net_input"]["source"][i, :n].float().cpu().clamp(-1, 1) * 3000).to(torch.int16).numpy()
        with wave.open(str(tmp_path / ("u%d.wav" % i)), "wb") as w:
            w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000); w.writeframes(pcm.tobytes())
        lines.append("u%d.wav\t%d" % (i, n))
    (tmp_path / "t.tsv").write_text("\n".join(lines) + "\n")
    (tmp_path / "t.ltr").write_text("A B | C A B |\nB | D\n")
    res = tmp_path / "res"
    argv = ["score", str(tmp_path / "ck.pt"), str(tmp_path / "dict.ltr.txt"), str(tmp_path / "t.tsv"), str(tmp_path / "t.ltr")]
    assert ctc.main(argv + ["--results", str(res)]) == 0
    line = capsys.readouterr().out.strip().splitlines()[-1].split()
    assert line[0] == "UER" and line[2] == "WER"
    got = {line[i]: int(line[i + 1]) for i in range(4, len(line), 2)}
    # the same batch by hand: shortest first, padded to the longest, the padding masked
    d = ctc.LetterDictionary.load(str(tmp_path / "dict.ltr.txt"))
    loaded, _ = ctc.load_ctc_checkpoint(str(tmp_path / "ck.pt"), len(d))
    wavs = [torch.as_tensor(read_wav(str(tmp_path / ("u%d.wav" % i)))[0], dtype=torch.float32) for i in (1, 0)]
    src, pm = torch.zeros(2, 8000), torch.ones(2, 8000, dtype=torch.bool)
    for r, w in enumerate(wavs):
        src[r, :w.numel()] = w
        pm[r, :w.numel()] = False
    target = torch.tensor([[d.index("B"), d.index("|"), d.index("D"), d.pad(), d.pad(), d.pad(), d.pad()],
                           [d.index(s) for s in "A B | C A B |".split()]])
    with torch.no_grad():
        out = loaded(source=src.cuda(), padding_mask=pm.cuda())
    il = (~out["padding_mask"]).sum(-1)
    want = ctc.error_counts(out["encoder_out"], il, target, d)
    assert got == {k: want[k] for k in ("c_errors", "c_total", "w_errors", "w_total")} and got["c_total"] == 10
    uer, wer = float(line[1].rstrip("%")), float(line[3].rstrip("%"))
    assert abs(uer - want["c_errors"] * 100.0 / 10) < 1e-3 and abs(wer - want["w_errors"] * 100.0 / 4) < 1e-3
    hyps = ctc.greedy_decode(out["encoder_out"], il.tolist(), d.bos())
    files = {n: (res / n).read_text().splitlines() for n in ("hypo.units", "hypo.word", "ref.units", "ref.word")}
    assert files["ref.units"] == ["A B | C A B | (None-0)", "B | D (None-1)"]
    assert files["ref.word"] == ["AB CAB (None-0)", "B D (None-1)"]
    assert files["hypo.units"] == ["%s (None-%d)" % (d.string(hyps[1 - i]), i) for i in (0, 1)]
    assert files["hypo.word"] == ["%s (None-%d)" % (ctc.post_process(d.string(hyps[1 - i]), "letter"), i) for i in (0, 1)]
    # without --results nothing is written, and the totals are the same
    assert ctc.main(argv) == 0
    assert capsys.readouterr().out.strip().splitlines()[-1].split() == line
    assert sorted(os.listdir(str(res))) == ["hypo.units", "hypo.word", "ref.units", "ref.word"]
