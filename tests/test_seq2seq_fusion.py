"""Shallow fusion and the n-gram blocker of the seq2seq search on the CPU: the float64 specification (beam_step_reference's
lm_logits / history / no_repeat_ngram_size, generate_reference's lm_model) against a brute-force restatement of the ban rule,
hand-made steps and tests/golden/seq2seq_fusion.npz (tools/gen_seq2seq_fusion_golden.py: the reference's SequenceGenerator with
lm_model and no_repeat_ngram_size); the builder of the kernel cases; the new symbols; SequenceGenerator's surface.  Nothing here
needs a GPU."""
import math
import os
import re

import numpy as np
import pytest
import torch

import seq2seq_cases as C
import seq2seq_fusion_cases as F
from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPTS = dict(beam=2, max_len=20, min_len=1, pad=C.PAD, unk=C.UNK, eos=C.EOS)


@pytest.fixture(scope="module")
def golden():
    return load_golden(F.GOLDEN)


@pytest.fixture(scope="module")
def plain():
    return load_golden("seq2seq.npz")


@pytest.fixture(scope="module")
def models():
    return {name: (C.build(name), F.build_lm(name)) for name in C.MODELS}


# ------------------------------------------------------------------------------------------------------------ the ban rule
def brute_force_banned(h, step, n):
    """_no_repeat_ngram with its dictionaries: every n-gram of the row under the key of its first n - 1 tokens; the banned tokens
    are the entries under the key of the last n - 1 tokens (none before step + 2 - n >= 0)"""
    grams = {}
    for i in range(len(h) - n + 1):
        g = h[i:i + n]
        grams.setdefault(",".join(str(x) for x in g[:-1]), []).append(g[-1])
    if step + 2 - n < 0:
        return set()
    return set(grams.get(",".join(str(x) for x in h[step + 2 - n:step + 1]), []))


@pytest.mark.parametrize("n", (1, 2, 3, 4))
def test_ban_rule_against_brute_force(n):
    from unispeech_amd.seq2seq import beam_step_reference, ngram_banned
    V = 8
    seen = 0
    for step in sorted({s for s in (0, n - 2, n - 1, 11) if s >= 0}):
        for seed in range(20):
            g = torch.Generator().manual_seed(100 * n + 10 * step + seed)
            hist = torch.tensor(F.ALPHABET)[torch.randint(0, 3, (3, step + 1), generator=g)]
            hist[:, 0] = C.EOS
            hist = hist.tolist()
            logits = torch.randn(3, V, generator=g)
            r = beam_step_reference(logits, [0.0, -1.0, -2.0], step, 0, history=hist, no_repeat_ngram_size=n, **OPTS)
            want = [brute_force_banned(h, step, n) for h in hist]
            assert r["banned"] == want == [ngram_banned(h, step, n) for h in hist], (n, step, seed)
            seen += sum(len(w) for w in want)
            for s, i in r["candidates"]:                              # a banned token is -inf: it is no candidate above -inf
                assert not (s > -math.inf and i % V in want[i // V])
    assert seen > 0
    assert ngram_banned([C.EOS, 4, 5], 2, 1) == {C.EOS, 4, 5}                        # n = 1: the whole history, eos included
    assert ngram_banned([C.EOS, 4, 5, 4], 3, 2) == {5} and ngram_banned([C.EOS, 4], 1, 3) == set()
    with pytest.raises(ValueError, match="history"):
        beam_step_reference(torch.zeros(1, V), [0.0], 1, 0, no_repeat_ngram_size=2, **OPTS)


def test_the_ban_comes_after_the_log_softmax():
    from unispeech_amd.seq2seq import beam_step_reference
    x = torch.tensor([[0.0, 0.0, 0.0, 0.0, 5.0, 1.0, 0.0, 0.0]])
    free = beam_step_reference(x, [0.0], 2, 0, **OPTS)
    r = beam_step_reference(x, [0.0], 2, 0, history=[[C.EOS, 4, 4]], no_repeat_ngram_size=2, **OPTS)
    assert free["rows"][0][1] == 4 and r["banned"] == [{4}]
    assert r["rows"][0][1] == 5                                                        # 4 4 would repeat: 5 wins
    assert r["rows"][0][2] == pytest.approx(float(torch.log_softmax(x.double(), -1)[0, 5]))   # 4 still counts in the normaliser


def test_the_lm_flips_the_winner():
    from unispeech_amd.seq2seq import beam_step_reference
    x = torch.tensor([[0.0, 0.0, 0.0, 0.0, 2.0, 1.5, 0.0, 0.0]])
    y = torch.tensor([[0.0, 0.0, 0.0, 0.0, 0.0, 3.0, 0.0, 0.0]])
    assert beam_step_reference(x, [0.0], 1, 0, **OPTS)["rows"][0][1] == 4
    r = beam_step_reference(x, [0.0], 1, 0, lm_logits=y, lm_weight=0.5, **OPTS)
    assert r["rows"][0][1] == 5
    want = torch.log_softmax(x.double(), -1)[0, 5] + 0.5 * torch.log_softmax(y.double(), -1)[0, 5]
    assert r["rows"][0][2] == pytest.approx(float(want), abs=1e-12)
    assert beam_step_reference(x, [0.0], 1, 0, lm_logits=y, lm_weight=0.0, **OPTS)["rows"][0][1] == 4
    # the LM takes no temperature
    hot = beam_step_reference(x, [0.0], 1, 0, lm_logits=y, lm_weight=0.5, temperature=2.0, **OPTS)
    want = torch.log_softmax(x.double() / 2, -1)[0, 5] + 0.5 * torch.log_softmax(y.double(), -1)[0, 5]
    assert hot["rows"][0][2] == pytest.approx(float(want), abs=1e-12)


def test_zero_weight_against_minus_infinity_is_literal():
    from unispeech_amd.seq2seq import beam_step_reference
    x = torch.tensor([[0.0, 0.0, 0.0, 0.0, 2.0, 1.5, 0.0, 0.0]])
    y = torch.zeros(1, 8)
    y[0, 4] = -math.inf
    r = beam_step_reference(x, [0.0], 1, 0, lm_logits=y, lm_weight=0.0, **OPTS)       # 0 * -inf = NaN -> -inf: 4 is gone
    assert r["rows"][0][1] == 5 and all(i % 8 != 4 or s == -math.inf for s, i in r["candidates"])
    y[0, 6] = math.nan                                                                 # a NaN kills the row
    r = beam_step_reference(x, [0.0], 1, 0, lm_logits=y, lm_weight=0.7, **OPTS)
    assert all(s == -math.inf for s, _ in r["candidates"])


# -------------------------------------------------------------------------------------------------------------- the golden
@pytest.mark.parametrize("name,sname,beam", F.runs())
def test_search_reference_reproduces_the_golden_hypotheses(golden, plain, models, name, sname, beam):
    from unispeech_amd import seq2seq as S
    model, lm = models[name]
    o = F.SETS[sname]
    enc = S.encoder_proj_reference(model, torch.from_numpy(plain["enc/x"]))
    pm = torch.from_numpy(plain["enc/padding_mask"])
    src, _ = C.batch()
    margins = []
    res = S.generate_reference(model, enc, pm, src.shape[1], beam=beam, max_len_b=C.MAX_LEN_B, margins=margins,
                               lm_model=lm if o["lm"] else None, lm_weight=o["lm_weight"],
                               no_repeat_ngram_size=o["no_repeat_ngram_size"])
    p = "%s/%s/beam%d/" % (name, sname, beam)
    lens = golden[p + "lens"]
    assert min(margins) == pytest.approx(float(golden[p + "margin"]), rel=1e-6) and min(margins) > 1e-3
    assert float(golden[p + "score_gap"]) > 1e-3
    for b in range(3):
        assert len(res[b]) == int((lens[b] > 0).sum())
        for j, h in enumerate(res[b]):
            n = int(lens[b, j])
            assert h["tokens"].tolist() == golden[p + "tokens"][b, j, :n].tolist()
            assert abs(float(h["score"]) - float(golden[p + "score"][b, j])) <= 1e-4
            assert np.abs(h["positional_scores"].numpy() - golden[p + "pos"][b, j, :n]).max() <= 1e-4
            if o["no_repeat_ngram_size"]:
                assert not F.repeats(h["tokens"].tolist(), o["no_repeat_ngram_size"])


def test_the_golden_is_sensitive(golden, plain):
    """F changes a 1-best of either model, the blocker changes every result, and the loops of seq2seq.npz are broken"""
    def firsts(g, p):
        return [g[p + "tokens"][b, 0, :g[p + "lens"][b, 0]].tolist() for b in range(3)]
    lens = []
    for name in C.MODELS:
        assert any(firsts(golden, "%s/F/beam%d/" % (name, k)) != firsts(plain, "%s/beam%d/" % (name, k)) for k in C.BEAMS)
        for k in C.BEAMS:
            assert firsts(golden, "%s/FN/beam%d/" % (name, k)) != firsts(golden, "%s/F/beam%d/" % (name, k))
            assert any(F.repeats(t, 3) for t in firsts(golden, "%s/F/beam%d/" % (name, k)))
            lens.append(golden["%s/FN/beam%d/lens" % (name, k)])
    for k in C.BEAMS:
        assert firsts(golden, "A/N/beam%d/" % k) != firsts(plain, "A/beam%d/" % k)
        assert any(F.repeats(t, 2) for t in firsts(plain, "A/beam%d/" % k))
    lens = np.concatenate([v.reshape(-1) for v in lens])
    assert (lens[lens > 0] < C.MAX_LEN_B + 1).any() and (lens == C.MAX_LEN_B + 1).any()
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", F.GOLDEN)) < 256 * 1024
    assert not any("weight" in k or "bias" in k for k in golden.keys() if not k.endswith("/keys"))


@pytest.mark.parametrize("name", list(C.MODELS))
def test_lm_reference_against_the_golden_lm_logits(golden, models, name):
    """transformer_lm._forward64 of the refilled LM gives the reference LM's teacher-forced log-probs"""
    from unispeech_amd.transformer_lm import _forward64
    lm = models[name][1]
    assert [k for k in golden[name + "/lm/keys"] if str(k) in lm.state_dict()] == sorted(lm.state_dict())
    p = "%s/F/beam1/" % name
    for b in range(3):
        n = int(golden[p + "lens"][b, 0])
        toks = golden[p + "tokens"][b, 0, :n].tolist()
        with torch.no_grad():
            got = _forward64(lm, toks[:-1]).numpy()
        want = torch.log_softmax(torch.from_numpy(golden[p + "lm_logits"][b, :n]).double(), -1).numpy()
        assert np.abs(got - want).max() <= 1e-5 * float(golden[name + "/lm/max"])


# --------------------------------------------------------------------------------------------------------- the case builder
@pytest.mark.parametrize("n,w,step", [(0, 0.7, 11), (1, None, 0), (1, 0.0, 2), (2, 0.7, 1), (3, 0.7, 11), (4, 2.0, 5), (3, 0.7, 300)])
def test_case_builder_properties(n, w, step):
    case = F.fused_case(2049, 5, n, w, step)
    V, beam = 2049, 5
    assert case["hist"].shape == (15, step + 1) and bool((case["hist"][:, 0] == C.EOS).all())
    assert set(case["hist"][:, 1:].reshape(-1).tolist()) <= set(F.ALPHABET)
    assert case["n_live"][1] == 0 and case["n_fin"][1] == beam                        # sentence 1 is finished
    assert (case["lm"] is None) == (w is None)
    assert case["sensitive"] == F.ban_possible(n, step)                                # a ban changes a row's best token
    exp = F.fused_expected(case)
    assert exp[1] is None
    banned = F.fused_banned(case)
    assert not banned[beam:2 * beam].any() and (banned.any() == (n > 0 and (step >= n or n == 1)))
    if step > 0:
        assert case["cum"][2 * beam + 1] == -math.inf
        assert math.isinf(float(case["logits"][0, 0])) and math.isinf(float(case["logits"][0, V - 1]))
        if w is not None:
            assert float(case["lm"][0, F.ALPHABET[1]]) == -math.inf and bool(torch.isnan(case["lm"][2 * beam + 2]).any())
            assert all(s == -math.inf for s, i in exp[2]["candidates"] if i // V == 2)    # the NaN row is dead
    for b in (0, 2):
        s = [v for v, _ in exp[b]["candidates"] if v > -math.inf]
        assert all(a - c > C.BEAM_GAP * (1 + abs(case["lm_weight"])) for a, c in zip(s[:-1], s[1:]))
    assert (2049, 5, 3, 0.7, F.LONG_STEP) in F.fused_cases() and F.LONG_STEP > 256
    cases = F.fused_cases()
    assert {c[0] for c in cases} == set(F.FUSED_V) and {c[1] for c in cases} == set(F.FUSED_WIDTHS)
    assert {c[2] for c in cases} == set(F.FUSED_N) and {c[3] for c in cases} == set(F.FUSED_WEIGHTS)
    for m in F.FUSED_N:
        assert {s for s in (0, m - 2, m - 1, 11) if s >= 0} <= {c[4] for c in cases if c[2] == m}


# ------------------------------------------------------------------------------------------------------------------- ABI
def test_new_symbols_declared_bound_and_exported():
    from unispeech_amd import _lib, ops
    src = open(os.path.join(ROOT, "include", "wavlm_hip.h")).read()
    assert int(re.search(r"#define WAVLM_HIP_ABI_VERSION (\d+)", src).group(1)) == 30 == _lib.ABI_VERSION
    L = _lib.lib()
    for name in ("wavlm_beam_step_fused_supported", "wavlm_beam_step_fused"):
        decl = re.search(r"\b%s\(([^;]*)\);" % name, src).group(1)
        assert name in _lib.SIGNATURES and len(decl.split(",")) == len(_lib.SIGNATURES[name][1]), name
        assert hasattr(L, name)
    assert len(_lib.SIGNATURES["wavlm_beam_step_fused"][1]) == len(_lib.SIGNATURES["wavlm_beam_step"][1]) + 5
    for fn in ("beam_step_fused", "beam_step_fused_supported"):
        assert hasattr(ops, fn)
    assert ops.beam_step_fused_supported(32, 65536, 65535, torch.bfloat16, torch.float32)
    assert ops.beam_step_fused_supported(1, 2, 1, torch.float32, torch.bfloat16)
    for beam, V, B in ((0, 32, 1), (33, 32, 1), (5, 1, 1), (5, 65537, 1), (5, 32, 0), (5, 32, 65536)):
        assert not ops.beam_step_fused_supported(beam, V, B, torch.float32)
    assert not L.wavlm_beam_step_fused_supported(5, 32, 1, 0, 2) and not L.wavlm_beam_step_fused_supported(5, 32, 1, 2, 0)
    assert "consumed" in ops.beam_step_fused.__doc__.lower() and "CONSUMED" in src
    with pytest.raises(_lib.WavlmHipError):
        ops.beam_step_fused(torch.zeros(2, 32), None, 32, max_len=3, min_len=1, pad=1, unk=3, eos=2)


# ------------------------------------------------------------------------------------------------------ the public surface
class _Dict:
    def __init__(self, n=C.VOCAB, pad=C.PAD, eos=C.EOS, unk=C.UNK):
        self.n, self._pad, self._eos, self._unk = n, pad, eos, unk

    def __len__(self):
        return self.n

    def pad(self):
        return self._pad

    def eos(self):
        return self._eos

    def unk(self):
        return self._unk


def test_sequence_generator_surface_and_refusals(models):
    import inspect
    from unispeech_amd.sequence_generator import SequenceGenerator
    m, lm = models["A"]
    names = list(inspect.signature(SequenceGenerator.__init__).parameters)[1:]
    assert names == ["models", "tgt_dict", "beam_size", "max_len_a", "max_len_b", "max_len", "min_len", "normalize_scores",
                     "len_penalty", "unk_penalty", "temperature", "match_source_len", "no_repeat_ngram_size", "search_strategy",
                     "eos", "symbols_to_strip_from_output", "lm_model", "lm_weight"]
    d = _Dict()
    g = SequenceGenerator([m], d)
    assert (g.beam_size, g.max_len_b, g.min_len, g.lm_model, g.lm_weight, g.no_repeat_ngram_size) == (1, 200, 1, None, 1.0, 0)
    assert g.max_len == m.max_decoder_positions() and SequenceGenerator([m], d, max_len=7).max_len == 7
    assert SequenceGenerator([m], d, beam_size=50).beam_size == C.VOCAB - 1            # never pad
    assert SequenceGenerator([m], d, symbols_to_strip_from_output={5}).symbols_to_strip_from_output == {5, C.EOS}
    with pytest.raises(NotImplementedError, match="models"):
        SequenceGenerator([m, m], d)
    with pytest.raises(NotImplementedError, match="match_source_len"):
        SequenceGenerator([m], d, match_source_len=True)
    with pytest.raises(NotImplementedError, match="search_strategy"):
        SequenceGenerator([m], d, search_strategy=object())
    with pytest.raises(ValueError, match="tgt_dict"):
        SequenceGenerator([m], _Dict(n=13))
    src, pm = C.batch()
    sample = {"net_input": {"source": src, "padding_mask": pm}}
    with pytest.raises(NotImplementedError, match="prefix_tokens"):
        g.generate([m], sample, prefix_tokens=torch.zeros(3, 1))
    with pytest.raises(NotImplementedError, match="constraints"):
        g(sample, constraints=[1])
    with pytest.raises(NotImplementedError, match="models"):
        g.generate([m, m], sample)
    with pytest.raises(ValueError, match="min_len"):
        SequenceGenerator([m], d, max_len_b=3, min_len=4).generate([m], sample)
    with pytest.raises(ValueError, match="min_len"):
        SequenceGenerator([m], d, max_len=3, min_len=3).generate([m], sample)       # max_len - 1 = 2 steps
    # the LM is checked before the encoder runs (the encoder would ask for a device)
    with pytest.raises(NotImplementedError, match="lm_model"):
        SequenceGenerator([m], d, lm_model=object()).generate([m], sample)
    from unispeech_amd.transformer_lm import TransformerLM
    import transformer_lm_cases as LC
    other = TransformerLM(dict(LC.MODELS["A"]), 13, pad=C.PAD, eos=C.EOS, unk=C.UNK)
    with pytest.raises(ValueError, match="dictionary"):
        SequenceGenerator([m], d, lm_model=other).generate([m], sample)
    short = TransformerLM(dict(LC.MODELS["B"], max_target_positions=8), C.VOCAB, pad=C.PAD, eos=C.EOS, unk=C.UNK)
    with pytest.raises(ValueError, match="max_target_positions"):
        SequenceGenerator([m], d, lm_model=short, max_len_b=12).generate([m], sample)
    with pytest.raises(ValueError, match="lm_model is on"):
        SequenceGenerator([m], d, lm_model=lm).generate([m], {"net_input": {"source": src.to("meta"), "padding_mask": pm}})
    with pytest.raises(ValueError, match="lm_weight"):
        SequenceGenerator([m], d, lm_model=lm, lm_weight=math.inf)
    with pytest.raises(ValueError, match="no_repeat_ngram_size"):
        SequenceGenerator([m], d, no_repeat_ngram_size=-1)


def test_generate_still_refuses_and_points_to_the_generator(models):
    m, lm = models["A"]
    src, pm = C.batch()
    for name, value in (("lm_model", lm), ("no_repeat_ngram_size", 3), ("lm_weight", 0.5)):
        with pytest.raises(NotImplementedError, match=name) as e:
            m.generate(src, pm, **{name: value})
        assert "SequenceGenerator" in str(e.value)
    import inspect
    from unispeech_amd.seq2seq import Wav2Vec2Seq2Seq
    for fn in (Wav2Vec2Seq2Seq.search, Wav2Vec2Seq2Seq._search):
        ps = inspect.signature(fn).parameters
        for k, default in (("lm_model", None), ("lm_weight", 1.0), ("no_repeat_ngram_size", 0)):
            assert ps[k].kind is inspect.Parameter.KEYWORD_ONLY and ps[k].default == default


def test_cli_arguments():
    from unispeech_amd import seq2seq
    a = seq2seq.parse_args(["decode", "ck.pt", "dict.txt", "a.wav"])
    assert (a.lm, a.lm_weight, a.no_repeat_ngram_size) == (None, 1.0, 0)
    a = seq2seq.parse_args(["decode", "ck.pt", "dict.txt", "a.wav", "--lm", "lm.pt", "--lm-weight", "0.7",
                            "--no-repeat-ngram-size", "3"])
    assert (a.lm, a.lm_weight, a.no_repeat_ngram_size, a.beam) == ("lm.pt", 0.7, 3, 5)
    a = seq2seq.parse_args(["score", "ck.pt", "dict.txt", "m.tsv", "l.ltr", "--no-repeat-ngram-size", "2"])
    assert (a.cmd, a.lm, a.no_repeat_ngram_size) == ("score", None, 2)
