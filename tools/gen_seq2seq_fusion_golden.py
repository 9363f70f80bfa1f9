"""Writes tests/golden/seq2seq_fusion.npz: the reference's SequenceGenerator on the CPU in fp32 over the two seq2seq models of
tests/seq2seq_cases.py with lm_model= / lm_weight= (a reference TransformerLanguageModel, built as
tools/gen_transformer_lm_golden.py builds it) and no_repeat_ngram_size= (NGramRepeatBlock on its Python path: the extension is
not built).  Needs the reference checkout (oracle/ref_shim.py); run where it is, never on a test machine.

No weights are stored (tests/seq2seq_fusion_cases.py refills either side from seeds).  Contents, M in A, B, S in F, FN, N
(seq2seq_fusion_cases.SETS), k in 1, 5:
  <M>/lm/keys                    the reference LM's state-dict names
  <M>/lm/max, <M>/lm/e_ref       teacher-forced LM logits on the F beam-1 hypotheses: max |fp32|, and the reference in bf16 on the CPU
                                 against fp32, max |difference| / max
  <M>/<S>/beam<k>/tokens, lens, score, pos    the hypotheses, in the layout of seq2seq.npz
  <M>/<S>/beam<k>/margin, score_gap           the float64 run's smallest deciding gap and the smallest gap between two scores of
                                 a sentence (both asserted > 1e-3)
  <M>/<S>/beam1/lm_logits        (sets with an LM) teacher-forced LM logits fp32 [3, 13, 12] of the 1-best, 0 beyond its length
Asserted (on failure: change the seed in seq2seq_fusion_cases.LM_SEEDS): the float64 search of this package returns the reference's
tokens with scores within 1e-4; per model F's 1-best differs from seq2seq.npz's in some sentence; every FN and N hypothesis is free
of repeated n-grams and every FN and N result differs from its unblocked counterpart in some sentence; some hypothesis ends by eos
before max_len and some sentence runs into max_len.

    python tools/gen_seq2seq_fusion_golden.py
"""
import argparse
import copy
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import seq2seq_cases as C  # noqa: E402
import seq2seq_fusion_cases as F  # noqa: E402
import transformer_lm_cases as LC  # noqa: E402
import gen_seq2seq_golden as G  # noqa: E402
import gen_transformer_lm_golden as GL  # noqa: E402
from oracle import ref_shim  # noqa: E402


def forced_lm(lm, toks):
    """teacher-forced logits [n, V] after [eos, t_1 .. t_{n-1}] of a hypothesis t that ends in eos"""
    with torch.no_grad():
        return lm(torch.tensor([[C.EOS] + [int(t) for t in toks[:-1]]]))[0][0].float()


def main():
    ref_shim.fairseq_wavlm()
    from fairseq.sequence_generator import SequenceGenerator
    from unispeech_amd import seq2seq as S
    from conftest import load_golden
    src, pm = C.batch()
    plain = load_golden("seq2seq.npz")
    enc_x, enc_pm = torch.from_numpy(plain["enc/x"]), torch.from_numpy(plain["enc/padding_mask"])
    out = {}
    early = full_length = 0
    Lm = C.MAX_LEN_B + 1
    for name in C.MODELS:
        model, d, _ = G.build_reference(name)
        cfgname = F.LM_CONFIG[name]
        lm, keys = GL.build_reference(cfgname, LC.MODELS, C.VOCAB, {cfgname: F.LM_SEEDS[name]})
        out[name + "/lm/keys"] = np.array(keys)
        mine, mine_lm = C.build(name), F.build_lm(name)
        assert sorted(k for k in mine_lm.state_dict()) == [k for k in keys if k in mine_lm.state_dict()]
        enc64 = S.encoder_proj_reference(mine, enc_x)
        first = {}
        for sname, o in F.SETS.items():
            if name not in o["models"]:
                continue
            for beam in C.BEAMS:
                gen = SequenceGenerator([model], d, beam_size=beam, max_len_a=0, max_len_b=C.MAX_LEN_B, min_len=1,
                                        normalize_scores=True, len_penalty=1.0, unk_penalty=0.0, temperature=1.0,
                                        no_repeat_ngram_size=o["no_repeat_ngram_size"], lm_model=lm if o["lm"] else None,
                                        lm_weight=o["lm_weight"])
                if gen.repeat_ngram_blocker is not None:
                    assert not gen.repeat_ngram_blocker.use_extension
                with torch.no_grad():
                    fin = gen.generate([model], {"net_input": {"source": src, "padding_mask": pm}})
                margins = []
                mref = S.generate_reference(mine, enc64, enc_pm, src.shape[1], beam=beam, max_len_b=C.MAX_LEN_B, margins=margins,
                                            lm_model=mine_lm if o["lm"] else None, lm_weight=o["lm_weight"],
                                            no_repeat_ngram_size=o["no_repeat_ngram_size"])
                toks = -np.ones((len(fin), beam, Lm), dtype=np.int64)
                lens = np.zeros((len(fin), beam), dtype=np.int64)
                score = np.zeros((len(fin), beam), dtype=np.float32)
                pos = np.zeros((len(fin), beam, Lm), dtype=np.float32)
                gap = np.inf
                for b, hyps in enumerate(fin):
                    assert len(hyps) == len(mref[b]), (name, sname, beam, b, len(hyps), len(mref[b]))
                    for j, h in enumerate(hyps):
                        n = h["tokens"].numel()
                        toks[b, j, :n], lens[b, j], score[b, j] = h["tokens"].numpy(), n, float(h["score"])
                        pos[b, j, :n] = h["positional_scores"].numpy()
                        assert h["tokens"].tolist() == mref[b][j]["tokens"].tolist(), (name, sname, beam, b, j, "change the seed")
                        assert abs(float(h["score"]) - float(mref[b][j]["score"])) < 1e-4
                        if o["no_repeat_ngram_size"]:
                            assert not F.repeats(h["tokens"].tolist(), o["no_repeat_ngram_size"]), (name, sname, beam, b, j)
                        early += int(n < Lm)
                        full_length += int(n == Lm)
                    s = sorted(float(h["score"]) for h in hyps)
                    gap = min([gap] + [y - x for x, y in zip(s[:-1], s[1:])])
                margin = min(margins)
                print("model %s set %s beam %d: lengths %s, margin %.4f, score gap %.4f, 1-bests %s"
                      % (name, sname, beam, lens.tolist(), margin, gap, [toks[b, 0, :lens[b, 0]].tolist() for b in range(len(fin))]))
                assert margin > 1e-3 and gap > 1e-3, "change the seed: fp32 against float64 may pick differently"
                p = "%s/%s/beam%d/" % (name, sname, beam)
                out[p + "tokens"], out[p + "lens"], out[p + "score"], out[p + "pos"] = toks, lens, score, pos
                out[p + "margin"], out[p + "score_gap"] = np.float64(margin), np.float64(gap)
                first[sname, beam] = [toks[b, 0, :lens[b, 0]].tolist() for b in range(len(fin))]
                if o["lm"] and beam == 1:
                    ll = np.zeros((len(fin), Lm, C.VOCAB), dtype=np.float32)
                    for b in range(len(fin)):
                        ll[b, :lens[b, 0]] = forced_lm(lm, toks[b, 0, :lens[b, 0]]).numpy()
                    out[p + "lm_logits"] = ll
                    if sname == "F":
                        lb = copy.deepcopy(lm).to(torch.bfloat16)
                        mx = float(np.abs(ll).max())
                        err = max(float((forced_lm(lb, toks[b, 0, :lens[b, 0]]) - torch.from_numpy(ll[b, :lens[b, 0]])).abs().max())
                                  for b in range(len(fin)))
                        out[name + "/lm/max"], out[name + "/lm/e_ref"] = np.float64(mx), np.float64(err / mx)
                        print("   LM of model %s: max |logit| %.3f, bf16 reference on the CPU e_ref %.3e" % (name, mx, err / mx))
        changed = False
        for beam in C.BEAMS:
            unfused = [plain["%s/beam%d/tokens" % (name, beam)][b, 0, :plain["%s/beam%d/lens" % (name, beam)][b, 0]].tolist()
                       for b in range(src.shape[0])]
            changed = changed or first["F", beam] != unfused
            assert first["FN", beam] != first["F", beam], (name, beam, "the blocker changes nothing under the LM")
            if ("N", beam) in first:
                assert first["N", beam] != unfused, (name, beam, "the blocker changes nothing")
        assert changed, (name, "the LM changes no 1-best at any beam: change the seed")
    assert early > 0, "no hypothesis ends by eos before max_len"
    assert full_length > 0, "no sentence runs into max_len"
    path = os.path.join(ROOT, "tests", "golden", F.GOLDEN)
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 256 * 1024


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--seed", action="append", default=[], metavar="M=SEED",
                    help="try another LM seed for model M (then put it into seq2seq_fusion_cases.LM_SEEDS)")
    for kv in ap.parse_args().seed:
        F.LM_SEEDS[kv.split("=")[0]] = int(kv.split("=")[1])
    main()
