"""csrc/ctc_align.hip on the device against the float64 reference of the same call (ctc_align.forced_align_reference): frames and
spans are compared with ==, score and token_scores within |d| <= 2^-22 max(1, |ref|) (ctc_align_cases.BOUND: one fp32 rounding
plus the float64 log-sum-exp's error, with a 4x margin).  The cases are in tests/ctc_align_cases.py."""
import numpy as np
import pytest
import torch

import ctc_align_cases as A

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def leave_no_device_memory_behind():
    """as in tests/test_ctc_score_gpu.py: ops' grow-only workspaces are put back as they were, what a caught exception's frames
    still hold is collected and the cache is released, so that later modules meet the caching allocator as they did before this
    one existed (the poisoned allocations of tests/gpu_checks.py count on that)"""
    import gc
    from unispeech_amd import ops
    saved = dict(ops._WS)
    yield
    torch.cuda.synchronize()
    ops._WS.clear()
    ops._WS.update(saved)
    for cached in (A.size_case, A.block_case, A.special_case, A.tie_case, A.bf16_case, A.reference):
        cached.cache_clear()
    gc.collect()
    torch.cuda.empty_cache()


# -------------------------------------------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("kind", ["tight", "loose"])
@pytest.mark.parametrize("L", A.SIZES)
def test_every_per_boundary_and_the_cap(L, kind):
    x, labels, il = A.size_case(L, kind)
    want = A.reference("size_case", L, kind)
    assert np.all(np.isfinite(want.score))
    if kind == "tight" and L > 0:                                       # a single path: label j on its own frame(s)
        assert all(int(want.spans[b, L - 1, 1]) == il[b] and int(want.spans[b, 0, 0]) == 0 for b in range(len(il)))
    A.assert_equal_to_reference(A.device(x, labels, il), want, (L, kind))


def test_input_lengths_around_the_staging_block():
    from unispeech_amd.ctc_align import ALIGN_BLOCK
    x, labels, il = A.block_case(ALIGN_BLOCK)
    assert il == [ALIGN_BLOCK - 1, ALIGN_BLOCK, ALIGN_BLOCK + 1, 2 * ALIGN_BLOCK + 1]
    want = A.reference("block_case", ALIGN_BLOCK)
    assert np.all(np.isfinite(want.score))                              # the NaN behind each length was not read
    A.assert_equal_to_reference(A.device(x, labels, il), want)


def test_special_cases():
    x, labels, il = A.special_case()
    want = A.reference("special_case")
    inf = float("inf")
    assert np.isfinite(want.score[0]) and want.frames[0, :11].tolist() == [0, -1, 1, -1, 2, -1, 3, -1, 4, -1, 5]
    assert want.score[1] == -inf and want.score[2] == 0.0 and want.score[3] == -inf and np.isfinite(want.score[4])
    assert np.isnan(want.score[5]) and np.isnan(want.score[6])
    got = A.device(x, labels, il)
    A.assert_equal_to_reference(got, want)
    for b in (1, 2, 3, 5, 6):
        assert np.all(got[0][b] == -2) and np.all(got[1][b] == -1) and np.all(got[2][b] == 0)


@pytest.mark.parametrize("name", ["zeros", "small", "wide"])
def test_the_tie_rule_on_integer_logits(name):
    x, labels, il = A.tie_case(name)
    assert torch.equal(x, x.round())
    want = A.reference("tie_case", name)
    if name == "zeros":                                                 # every path ties: the trailing blank is held from the end
        assert want.frames[0].tolist() == [0, 1, 2, 3, 4] + [-1] * 15
    A.assert_equal_to_reference(A.device(x, labels, il), want, name)


def test_bf16_logits_and_both_layouts():
    x, labels, il = A.size_case(127, "loose")
    want = A.reference("size_case", 127, "loose")
    for batch_first in (True, False):
        A.assert_equal_to_reference(A.device(x, labels, il, torch.float32, batch_first), want, batch_first)
    xb, labels, il = A.bf16_case()
    assert torch.equal(xb.to(torch.bfloat16).float(), xb) and not torch.equal(xb, x)
    want = A.reference("bf16_case")
    for batch_first in (True, False):
        A.assert_equal_to_reference(A.device(xb, labels, il, torch.bfloat16, batch_first), want, batch_first)


def test_a_sample_alone_equals_the_sample_in_a_batch_and_runs_repeat():
    x, labels, il = A.block_case(32)
    whole = A.device(x, labels, il)
    again = A.device(x, labels, il)
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(whole, again))
    Lmax = max(len(lab) for lab in labels)
    for b in (0, 3):
        alone = A.device(x[:il[b], b:b + 1], [labels[b]], [il[b]])
        n = len(labels[b])
        assert np.array_equal(alone[0][0], whole[0][b, :il[b]]) and np.all(whole[0][b, il[b]:] == -2)
        assert np.array_equal(alone[1][0], whole[1][b, :n]) and np.all(whole[1][b, n:] == -1) and n <= Lmax
        assert alone[2][0].tobytes() == whole[2][b, :n].tobytes() and alone[3].tobytes() == whole[3][b:b + 1].tobytes()


def test_aligning_the_greedy_decode_gives_the_argmax_path():
    """without ties the best path over ALL transcripts is the per-frame argmax, so the alignment of its collapse is that path and
    its score the sum of the per-frame maxima of the log-probabilities: a check that needs no reference"""
    from unispeech_amd.ctc import greedy_decode
    rng = np.random.RandomState(21)
    T, B = 90, 3
    il = [90, 61, 33]
    x = torch.from_numpy(rng.randn(T, B, A.C).astype(np.float32))
    xd = A.put(x)
    hyps = greedy_decode(xd, il, 0)
    frames, spans, tok, score = A.device(x, hyps, il)
    lp = torch.log_softmax(x.double(), -1).numpy()
    for b in range(B):
        arg = x[:il[b], b].argmax(-1).tolist()
        want = [hyps[b][j] if j >= 0 else 0 for j in frames[b, :il[b]]]
        assert want == arg
        ref = lp[:il[b], b].max(-1).sum()
        assert abs(float(score[b]) - ref) <= A.BOUND * max(1.0, abs(ref))
        assert abs(float(tok[b, :len(hyps[b])].astype(np.float64).sum()) - sum(lp[t, b, c] for t, c in enumerate(arg) if c != 0)) \
            <= len(hyps[b]) * A.BOUND * max(1.0, abs(ref))
    from unispeech_amd.ctc_align import get_timesteps, timesteps
    assert timesteps(xd, il, hyps, 0) == [get_timesteps(x[:il[b], b].argmax(-1).tolist(), 0) for b in range(B)]


def test_command_line_end_to_end(tmp_path, capsys):
    """`python -m unispeech_amd.ctc_align` on a tiny checkpoint written here, one utterance per batch: its CTM lines are those of
    the float64 reference on the host copy of the loaded model's logits (times ==, confidence to the printed digits), and the
    utterance whose transcript does not fit its frames is reported and skipped"""
    import wave
    from test_ctc_gpu import NCLS, TINY, _tiny_ctc
    from unispeech_amd import ctc, ctc_align
    from unispeech_amd.kmeans import read_wav
    model, _, sample = _tiny_ctc()
    d = ["|"] + [chr(ord("A") + i) for i in range(NCLS - 5)]
    (tmp_path / "dict.ltr.txt").write_text("".join("%s 1\n" % c for c in d))
    torch.save({"cfg": dict(TINY), "model": model.eval().state_dict(), "arch": "wavlm", "normalize": False}, str(tmp_path / "ck.pt"))
    sizes = (8000, 5000, 3200)
    for i, n in enumerate(sizes):
        pcm = (sample["net_input"]["source"][i % 2, :n].float().cpu().clamp(-1, 1) * 3000).to(torch.int16).numpy()
        with wave.open(str(tmp_path / ("u%d.wav" % i)), "wb") as w:
            w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000); w.writeframes(pcm.tobytes())
    (tmp_path / "m.tsv").write_text(str(tmp_path) + "\n" + "".join("u%d.wav\t%d\n" % (i, n) for i, n in enumerate(sizes)))
    text = ["A B | C A", "| D D | E", "A B C D E F G A B C D E"]
    (tmp_path / "l.ltr").write_text("".join(t + "\n" for t in text))
    args = [str(tmp_path / n) for n in ("ck.pt", "dict.ltr.txt", "m.tsv", "l.ltr")]
    assert ctc_align.main(args + ["--out", str(tmp_path / "o.ctm"), "--max-samples", "1"]) == 0
    err = capsys.readouterr().err
    assert "u2: no alignment" in err and err.count("no alignment") == 1
    got = (tmp_path / "o.ctm").read_text().splitlines()
    assert ctc_align.main(args + ["--tokens", "--max-samples", "1"]) == 0
    got_tokens = capsys.readouterr().out.splitlines()

    dic = ctc.LetterDictionary.load(args[1])
    loaded, _ = ctc.load_ctc_checkpoint(args[0], len(dic))
    stride = ctc_align.frame_stride(TINY["conv_feature_layers"])
    assert stride == 320
    want, want_tokens = [], []
    for i in range(2):
        x = torch.as_tensor(read_wav(str(tmp_path / ("u%d.wav" % i)))[0], dtype=torch.float32).cuda().view(1, -1)
        with torch.no_grad():
            logits = loaded(source=x, padding_mask=None)["encoder_out"].float().cpu()
        lab = [dic.index(s) for s in text[i].split()]
        a = ctc_align.forced_align_reference(logits, lab, None, [len(lab)], 0)
        assert np.isfinite(a.score[0])
        for each, out in ((False, want), (True, want_tokens)):
            out += ctc_align.ctm_lines("u%d" % i, ctc_align.word_segments(lab, a.spans[0], a.token_scores[0], dic, stride,
                                                                          each_token=each))
    assert [w.split()[4] for w in want] == ["AB", "CA", "DD", "E"] and len(want_tokens) == 5 + 5
    for g, w in ((got, want), (got_tokens, want_tokens)):
        assert [v.split()[:5] for v in g] == [v.split()[:5] for v in w]
        assert all(abs(float(a.split()[5]) - float(b.split()[5])) <= 1.5e-4 for a, b in zip(g, w))


def test_refusals():
    from unispeech_amd import _lib, ops
    from unispeech_amd.ctc_align import forced_align
    x = torch.zeros(1, 4, A.C, device="cuda")                           # [B, T, C]
    tg = torch.tensor([1, 2], dtype=torch.int32, device="cuda")
    off = torch.tensor([0, 2], dtype=torch.int32, device="cuda")
    il = torch.tensor([4], dtype=torch.int32, device="cuda")
    need = _lib.lib().wavlm_ctc_align_workspace_bytes(1, 4, 2)
    ops.ctc_align(x, tg, off, 2, 2, il, 0, ws=torch.empty(need, dtype=torch.uint8, device="cuda"))
    with pytest.raises(_lib.WavlmHipError, match="invalid argument"):
        ops.ctc_align(x, tg, off, 2, 2, il, 0, ws=torch.empty(need - 1, dtype=torch.uint8, device="cuda"))
    with pytest.raises(NotImplementedError, match=r"L = 1024\b"):
        forced_align(torch.zeros(2100, 1, 4, device="cuda"), [1] * 1024, None, [1024])
    torch.cuda.synchronize()
