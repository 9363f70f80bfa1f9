"""Writes tests/golden/seq2seq.npz: the reference's wav2vec_seq2seq (fairseq.models.wav2vec.wav2vec2_asr: Wav2VecEncoder +
TransformerDecoder) on the CPU in fp32, teacher-forced and decoded by its SequenceGenerator.  Needs the reference checkout
(oracle/ref_shim.py); run where it is, never on a test machine.

No weights are stored: the encoder's are those of tests/golden/tiny_w2v2.npz, the decoder's (and encoder.proj's) are refilled from a
seed by tests/seq2seq_cases.py fill_decoder on either side.  Three things of the reference are worked around in the harness, not
reproduced: Wav2VecEncoder.__init__ builds its inner model through a task and a checkpoint path (here the inner model is built
directly and handed over); Wav2VecEncoder.reorder_encoder_out leaves encoder_out["padding_mask"] -- the mask its decoder reads --
unordered, which fails for any padded batch with beam > 1 or a sentence that finishes early (here the mask follows the order); and
this checkout's MultiheadAttention returns a third value (the position bias) that TransformerDecoderLayer does not expect from its
encoder attention (transformer_layer.py:378; here the call returns the first two).
Contents, M in A, B (tests/seq2seq_cases.py MODELS):
  enc/x, enc/padding_mask    the encoder's features fp32 [3, Ts, 64] before proj and its frame mask, for the CPU tests
  <M>/keys                   the reference's state-dict names
  <M>/logits                 teacher-forced logits fp32 [3, 9, 12] on forced_tokens()
  <M>/inc_err                max |incremental - full| of the reference itself over the positions that hold no pad (asserted <= 1e-5)
  <M>/e_ref, <M>/max         the reference in bf16 on the CPU against fp32: max |difference| / max, and max |fp32 logits|
  <M>/beam<k>/tokens, lens, score, pos   SequenceGenerator's hypotheses at beam k in 1, 5 with max_len_b 12: int64 [3, k, 13] (-1
                             beyond a length), int64 [3, k] (0: no such hypothesis), fp32 [3, k], fp32 [3, k, 13]
  <M>/beam<k>/margin         the smallest gap in the float64 run (unispeech_amd.seq2seq.generate_reference) between a candidate that
                             was taken and the best one that was not (asserted > 1e-3: fp32 against float64 then picks the same)
  <M>/beam<k>/score_gap      the smallest gap between two hypotheses' scores of one sentence (asserted > 1e-3: the same order)
Asserted as well: the float64 restatement returns the reference's tokens; at least one hypothesis ends by eos before max_len and
at least one sentence runs into max_len.

    python tools/gen_seq2seq_golden.py
"""
import argparse
import contextlib
import copy
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import seq2seq_cases as C  # noqa: E402
from oracle import gen_golden, ref_shim  # noqa: E402


def build_reference(name):
    from fairseq.data import Dictionary
    from fairseq.models import FairseqEncoder
    from fairseq.models.wav2vec import wav2vec2 as w2
    from fairseq.models.wav2vec import wav2vec2_asr as asr
    from conftest import golden_state_dict, load_golden
    asr.open_dict = lambda cfg: contextlib.nullcontext()              # omegaconf's context manager around a plain Namespace
    wcfg = w2.Wav2Vec2Config()
    for k, v in gen_golden.TINY.items():
        if hasattr(wcfg, k):
            setattr(wcfg, k, v)
    wcfg.final_dim = 32
    wcfg.quantize_targets = True
    wcfg.latent_vars, wcfg.latent_groups, wcfg.latent_dim = 20, 2, 0
    wcfg.latent_temp = (2.0, 0.5, 0.999995)
    wcfg.num_negatives, wcfg.cross_sample_negatives = 7, 3
    wcfg.logit_temp = 0.1
    inner = w2.Wav2Vec2Model(wcfg)
    inner.load_state_dict(golden_state_dict(load_golden(C.ENCODER_GOLDEN)), strict=True)
    inner.remove_pretraining_modules()

    class Encoder(asr.Wav2VecEncoder):
        def __init__(self, model, D):
            FairseqEncoder.__init__(self, None)
            self.apply_mask, self.w2v_model = False, model
            self.final_dropout = torch.nn.Dropout(0.0)
            self.freeze_finetune_updates, self.num_updates = 0, 0
            d = wcfg.encoder_embed_dim
            self.proj = asr.Linear(d, D) if D != d else None

        def reorder_encoder_out(self, encoder_out, new_order):
            out = super().reorder_encoder_out(encoder_out, new_order)
            if out.get("padding_mask") is not None:
                out["padding_mask"] = out["padding_mask"].index_select(0, new_order)
            return out

    d = Dictionary()
    for s in C.SYMBOLS:
        d.add_symbol(s)
    assert len(d) == C.VOCAB and (d.pad(), d.eos(), d.unk()) == (C.PAD, C.EOS, C.UNK)
    opts = dict(C.MODELS[name])
    cfg = argparse.Namespace(decoder_layerdrop=0.0, decoder_dropout=0.0, decoder_attention_dropout=0.0,
                             decoder_activation_dropout=0.0, no_token_positional_embeddings=False, **opts)
    embed = asr.Embedding(len(d), cfg.decoder_embed_dim, d.pad())
    model = asr.Wav2Vec2Seq2SeqModel(Encoder(inner, cfg.decoder_embed_dim), asr.TransformerDecoder(cfg, d, embed))
    from fairseq.modules import MultiheadAttention

    class TwoValues(MultiheadAttention):
        def forward(self, *a, **k):
            return super().forward(*a, **k)[:2]

    for layer in model.decoder.layers:
        layer.encoder_attn.__class__ = TwoValues
    sd = model.state_dict()
    full = C.fill_decoder(sd, C.SEEDS[name])
    full.update({k: v.clone() for k, v in sd.items() if k.startswith("encoder.w2v_model.") or k.rsplit(".", 1)[-1] in C.NOT_WEIGHTS})
    model.load_state_dict(full, strict=True)
    return model.eval(), d, sorted(sd)


def forced(model, src, pm, tok):
    """(teacher-forced logits [B, T, V], max |incremental - full| where no pad is involved) the way SequenceGenerator runs the model:
    encoder.forward with its default tbc=True, then decoder.forward"""
    eo = model.encoder(source=src, padding_mask=pm)
    full = model.decoder(tok, encoder_out=eo)[0]
    inc, err = {}, 0.0
    for t in range(tok.shape[1]):
        step = model.decoder(tok[:, :t + 1], encoder_out=eo, incremental_state=inc)[0][:, -1]
        keep = tok[:, t] != C.PAD
        err = max(err, float((step[keep].float() - full[keep, t].float()).abs().max()))
    return full.float(), err, eo


def hypotheses(model, d, src, pm, beam):
    from fairseq.sequence_generator import SequenceGenerator
    gen = SequenceGenerator([model], d, beam_size=beam, max_len_a=0, max_len_b=C.MAX_LEN_B, min_len=1, normalize_scores=True,
                            len_penalty=1.0, unk_penalty=0.0, temperature=1.0)
    return gen.generate([model], {"net_input": {"source": src, "padding_mask": pm}})


def main():
    ref_shim.fairseq_wavlm()
    from unispeech_amd import seq2seq as S
    src, pm = C.batch()
    tok = C.forced_tokens()
    out = {}
    early = full_length = 0
    for name in C.MODELS:
        model, d, keys = build_reference(name)
        out[name + "/keys"] = np.array(keys)
        with torch.no_grad():
            logits, err, eo = forced(model, src, pm, tok)
            res = model.encoder.w2v_model.extract_features(source=src, padding_mask=pm, mask=False)
            lb = forced(copy.deepcopy(model).to(torch.bfloat16), src.to(torch.bfloat16), pm, tok)[0]
        assert err <= 1e-5, err
        mx = float(logits.abs().max())
        e_ref = float((lb - logits).abs().max()) / mx
        print("model %s: max |logit| %.3f, incremental - full %.2e, bf16 reference on the CPU e_ref %.3e" % (name, mx, err, e_ref))
        out[name + "/logits"] = logits.numpy()
        out[name + "/inc_err"], out[name + "/e_ref"], out[name + "/max"] = np.float64(err), np.float64(e_ref), np.float64(mx)
        if "enc/x" not in out:
            out["enc/x"] = res["x"].float().numpy()
            out["enc/padding_mask"] = res["padding_mask"].numpy()
        assert np.array_equal(out["enc/x"], res["x"].float().numpy())
        mine = C.build(name)
        assert sorted(mine.state_dict()) == keys, set(mine.state_dict()) ^ set(keys)
        enc64 = S.encoder_proj_reference(mine, torch.from_numpy(out["enc/x"]))
        fpm = torch.from_numpy(out["enc/padding_mask"])
        d64 = S.decoder_reference(mine, enc64, fpm, tok)
        print("   float64 restatement against the reference's logits: %.2e of max" % (float((d64 - logits.double()).abs().max()) / mx))
        for beam in C.BEAMS:
            with torch.no_grad():
                fin = hypotheses(model, d, src, pm, beam)
            margins = []
            mref = S.generate_reference(mine, enc64, fpm, src.shape[1], beam=beam, max_len_b=C.MAX_LEN_B, margins=margins)
            Lm = C.MAX_LEN_B + 1
            toks = -np.ones((len(fin), beam, Lm), dtype=np.int64)
            lens = np.zeros((len(fin), beam), dtype=np.int64)
            score = np.zeros((len(fin), beam), dtype=np.float32)
            pos = np.zeros((len(fin), beam, Lm), dtype=np.float32)
            gap = np.inf
            for b, hyps in enumerate(fin):
                assert len(hyps) == len(mref[b]), (name, beam, b, len(hyps), len(mref[b]))
                for j, h in enumerate(hyps):
                    n = h["tokens"].numel()
                    toks[b, j, :n], lens[b, j], score[b, j] = h["tokens"].numpy(), n, float(h["score"])
                    pos[b, j, :n] = h["positional_scores"].numpy()
                    assert h["tokens"].tolist() == mref[b][j]["tokens"].tolist(), (name, beam, b, j)
                    assert abs(float(h["score"]) - float(mref[b][j]["score"])) < 1e-4
                    early += int(n < Lm)
                    full_length += int(n == Lm)
                s = sorted(float(h["score"]) for h in hyps)
                gap = min([gap] + [y - x for x, y in zip(s[:-1], s[1:])])
            margin = min(margins)
            print("   beam %d: lengths %s, margin %.4f, score gap %.4f" % (beam, lens.tolist(), margin, gap))
            assert margin > 1e-3 and gap > 1e-3, "change the seed: fp32 against float64 may pick differently"
            p = "%s/beam%d/" % (name, beam)
            out[p + "tokens"], out[p + "lens"], out[p + "score"], out[p + "pos"] = toks, lens, score, pos
            out[p + "margin"], out[p + "score_gap"] = np.float64(margin), np.float64(gap)
    assert early > 0, "no hypothesis ends by eos before max_len"
    assert full_length > 0, "no sentence runs into max_len"
    path = os.path.join(ROOT, "tests", "golden", "seq2seq.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 256 * 1024


if __name__ == "__main__":
    argparse.ArgumentParser(description=__doc__.split("\n\n")[0]).parse_args()
    main()
