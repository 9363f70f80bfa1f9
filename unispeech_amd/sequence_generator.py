"""The reference's `SequenceGenerator` (src/fairseq/sequence_generator.py) as a class surface over the device search of
unispeech_amd.seq2seq: beam search of one Wav2Vec2Seq2Seq with, optionally, shallow fusion of a Transformer LM (lm_model=,
lm_weight=, lines 38-39 and 338-344) and the n-gram blocker (no_repeat_ngram_size=, lines 94-97 and 388-389,
ngram_repeat_block.py) -- both inside the step kernel wavlm_beam_step_fused (csrc/s2s.hip).

    gen = SequenceGenerator([model], tgt_dict, beam_size=5, max_len_b=200, lm_model=lm, lm_weight=0.7, no_repeat_ngram_size=3)
    hypos = gen.generate([model], {"net_input": {"source": wav, "padding_mask": mask}})
    hypos[b][j] -> {"tokens": long [n] ending in eos, "score": fp32 scalar, "positional_scores": fp32 [n]}, best first

  models           a list holding one Wav2Vec2Seq2Seq (an ensemble is refused by name)
  tgt_dict         an object with pad() / unk() / eos() and a length; they must be the model's
  beam_size        clamped to len(tgt_dict) - 1 (line 82: pad is never selected)
  max_len          0: the model's max_decoder_positions(); a step count is min(int(max_len_a * src_len + max_len_b), max_len - 1)
                   (lines 86, 240-250)
  lm_model         a unispeech_amd.transformer_lm.TransformerLM over the same dictionary, on the model's device.  It is scored by a
                   plain log-softmax -- TransformerLM.score's -inf for unk is FairseqLM's rule, not SequenceGenerator's.
  eos              overrides tgt_dict.eos(); symbols_to_strip_from_output is kept for callers (the hypotheses are not stripped, as
                   in the reference)
Refused by name (NotImplementedError): more than one model, match_source_len, a search_strategy, prefix_tokens, constraints, and a
bos_token other than eos.
Taken literally from the reference: lm_weight = 0 against an LM entry of -inf is NaN and hence -inf; no_repeat_ngram_size = 1 bans
every token of the history, eos included (the row begins with it), so such a search ends at max_len without a hypothesis.
"""
import math

import torch

__all__ = ["SequenceGenerator"]


class SequenceGenerator:
    def __init__(self, models, tgt_dict, beam_size=1, max_len_a=0, max_len_b=200, max_len=0, min_len=1, normalize_scores=True,
                 len_penalty=1.0, unk_penalty=0.0, temperature=1.0, match_source_len=False, no_repeat_ngram_size=0,
                 search_strategy=None, eos=None, symbols_to_strip_from_output=None, lm_model=None, lm_weight=1.0):
        from .seq2seq import Wav2Vec2Seq2Seq
        self.model = self._one_model(models)
        if not isinstance(self.model, Wav2Vec2Seq2Seq):
            raise NotImplementedError("models: a Wav2Vec2Seq2Seq is decoded, not %s" % type(self.model).__name__)
        if match_source_len:
            raise NotImplementedError("match_source_len is not built (see unispeech_amd/sequence_generator.py)")
        if search_strategy is not None:
            raise NotImplementedError("search_strategy is not built: the search is BeamSearch (see "
                                      "unispeech_amd/sequence_generator.py)")
        self.tgt_dict = tgt_dict
        self.pad, self.unk = int(tgt_dict.pad()), int(tgt_dict.unk())
        self.eos = int(tgt_dict.eos()) if eos is None else int(eos)
        self.symbols_to_strip_from_output = set(symbols_to_strip_from_output or ()) | {self.eos}
        self.vocab_size = len(tgt_dict)
        m = self.model
        if (self.vocab_size, self.pad, self.eos, self.unk) != (m.vocab, m.pad, m.eos, m.unk):
            raise ValueError("tgt_dict (size, pad, eos, unk) = %r differs from the model's %r"
                             % ((self.vocab_size, self.pad, self.eos, self.unk), (m.vocab, m.pad, m.eos, m.unk)))
        self.beam_size = min(int(beam_size), self.vocab_size - 1)                      # line 82
        if self.beam_size < 1:
            raise ValueError("beam_size must be at least 1")
        self.max_len_a, self.max_len_b, self.min_len = max_len_a, max_len_b, int(min_len)
        self.max_len = int(max_len) or m.max_decoder_positions()                      # line 86
        self.normalize_scores, self.len_penalty, self.unk_penalty = bool(normalize_scores), float(len_penalty), float(unk_penalty)
        if not temperature > 0:
            raise ValueError("--temperature must be greater than 0")
        self.temperature = float(temperature)
        self.no_repeat_ngram_size = int(no_repeat_ngram_size)
        self.lm_model, self.lm_weight = lm_model, float(lm_weight)
        self.step_logits = None                # tests: a list that receives every step's (logits, row lengths, LM logits | None)
        if self.no_repeat_ngram_size < 0:
            raise ValueError("no_repeat_ngram_size must be >= 0")
        if lm_model is not None and not math.isfinite(self.lm_weight):
            raise ValueError("lm_weight must be finite")

    @staticmethod
    def _one_model(models):
        models = list(models) if isinstance(models, (list, tuple)) else [models]
        if len(models) != 1:
            raise NotImplementedError("models: an ensemble of %d is not built; hand over a list of one model" % len(models))
        return models[0]

    def cuda(self):
        self.model.cuda()
        return self

    def __call__(self, sample, **kw):
        return self._generate(sample, **kw)

    forward = __call__

    def generate(self, models, sample, **kw):
        """models: the list the generator was made with (the reference ignores it as well); sample["net_input"] holds "source"
        [B, T] and "padding_mask" (bool [B, T] or None) -> per sentence its finished hypotheses, best first"""
        if models is not None and self._one_model(models) is not self.model:
            raise NotImplementedError("models: generate() decodes the model the generator was made with")
        return self._generate(sample, **kw)

    def _generate(self, sample, prefix_tokens=None, constraints=None, bos_token=None):
        if prefix_tokens is not None:
            raise NotImplementedError("prefix_tokens is not built (see unispeech_amd/sequence_generator.py)")
        if constraints is not None:
            raise NotImplementedError("constraints is not built (see unispeech_amd/sequence_generator.py)")
        if bos_token is not None and int(bos_token) != self.eos:
            raise NotImplementedError("bos_token other than eos is not built (see unispeech_amd/sequence_generator.py)")
        net = sample["net_input"]
        if "source" not in net:
            raise ValueError("expected `source` in net_input, got %s" % sorted(net))
        source, padding_mask = net["source"], net.get("padding_mask")
        m = self.model
        m._refuse_grad(source)
        B, src_len = source.shape[:2]
        max_len = min(int(self.max_len_a * src_len + self.max_len_b), self.max_len - 1,                # lines 240-250
                      m.max_decoder_positions() - 1)
        if not 0 <= self.min_len <= max_len:
            raise ValueError("min_len cannot be larger than max_len (%d, %d)" % (self.min_len, max_len))
        from . import ops
        if not ops.beam_step_fused_supported(self.beam_size, m.vocab, B, torch.float32):
            raise NotImplementedError("wavlm_beam_step_fused takes 1 <= beam <= 32, 2 <= V <= 65536, B <= 65535 (beam=%d V=%d "
                                      "B=%d)" % (self.beam_size, m.vocab, B))
        m._check_fusion(self.lm_model, self.lm_weight, self.no_repeat_ngram_size, max_len, source.device)   # before the encoder
        with torch.no_grad():
            enc = m._encode(source, padding_mask)
        return m._search(enc, max_len, self.beam_size, self.min_len, self.normalize_scores, self.len_penalty, self.unk_penalty,
                         self.temperature, None, self.step_logits, lm_model=self.lm_model,
                         lm_weight=self.lm_weight, no_repeat_ngram_size=self.no_repeat_ngram_size)
