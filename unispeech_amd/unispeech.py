"""UniSpeech multitask pre-training: the model that joins the wav2vec 2.0 contrastive head with a CTC head over the same encoder,
and its criterion -- src/fairseq/models/unispeech/unispeech.py (`Unispeech`, `Wav2VecEncoder`) and
src/fairseq/criterions/unispeech_criterion.py (`UnispeechCriterion`), the pair the recipe trains with
`--arch unispeech --criterion unispeech_criterion --transpose --negatives-from-everywhere --quantize-targets --mtlalpha 0.5
--replace-prob 0.5` (src/examples/unispeech/scripts).

The inner model is wav2vec2.Wav2Vec2Model (its `q` result: the quantised frames projected to the encoder width); the CTC branch
replaces a random subset of encoder rows by their quantised counterparts, applies final_dropout and the Linear to the dictionary.
The reference does that in five elementwise passes over [T, B, D] (two masked_fill, an add, the dropout, its mask); here it is
one launch each way (functional.ReplaceMixFn, csrc/rowops.hip wavlm_replace_mix), and the logits stay in batch-first storage: the
T x B x C tensor handed to the CTC kernel is a view it reads in place.

What differs from the reference, on purpose:
  * with mtlalpha == 0 the reference's criterion raises KeyError on ctc_logging_output['ntokens']; here ntokens / nsentences then
    come from the InfoNCE log
  * fine-tuning from a checkpoint of this model (ctc.EncoderCtc.build(arch="unispeech")) removes the quantiser modules of the
    inner model; the reference leaves them in place, unused
"""
import math
from dataclasses import dataclass

import torch
import torch.nn as nn

from . import functional as F
from .ctc import CtcCriterion, head_logits
from .wav2vec2 import Wav2Vec2Config, Wav2Vec2Model, Wav2vecCriterion


@dataclass
class UniSpeechConfig(Wav2Vec2Config):
    """UniSpeechConfig (models/unispeech/unispeech.py:27-34)"""
    replace_prob: float = 0.5
    final_dropout: float = 0.1


def draw_replace_mat(T, B, p):
    """the reference's draw (unispeech.py:107-108) on the torch CPU generator: bool [T, B]"""
    return torch.bernoulli(torch.empty(T, B).fill_(p)).bool()


class Wav2VecEncoder(nn.Module):
    """Wav2VecEncoder of unispeech.py:69-122: w2v_model, final_dropout, proj"""

    def __init__(self, cfg, num_classes):
        super().__init__()
        self.w2v_model = Wav2Vec2Model(cfg)
        m = self.w2v_model
        if m.quantizer is None:
            raise ValueError("Unispeech needs quantize_targets: the CTC branch mixes the quantised frames (results['q']) into "
                             "the encoder output")
        d = cfg.encoder_embed_dim
        q_width = d if m.transpose else m.quantizer.vars.shape[-1] * m.quantizer.groups
        if q_width != d:
            raise ValueError("Unispeech: q is %d wide, the encoder output %d (without transpose the codebook width latent_dim / "
                             "final_dim must equal encoder_embed_dim)" % (q_width, d))
        m.return_q = True
        self.final_dropout = nn.Dropout(cfg.final_dropout)
        self.num_updates = 0
        self.replace_prob = float(cfg.replace_prob)
        self.proj = None
        if num_classes is not None:
            self.proj = nn.Linear(d, int(num_classes))
            nn.init.xavier_uniform_(self.proj.weight)
            nn.init.constant_(self.proj.bias, 0.0)

    def set_num_updates(self, num_updates):
        self.num_updates = num_updates
        self.w2v_model.set_num_updates(num_updates)

    def forward(self, source, padding_mask=None, tbc=True, **kwargs):
        res = self.w2v_model(source=source, padding_mask=padding_mask, mask=self.training,
                             **{k: v for k, v in kwargs.items() if k in ("padding_mask_cpu", "padding_count", "mask_indices")})
        x, q, padding_mask = res["features"], res["q"], res["padding_mask"]         # [B, T, D] both
        B, T, D = x.shape
        replace_mat = draw_replace_mat(T, B, self.replace_prob)                    # host draw, [T, B] like the reference
        sel = F.h2d(replace_mat.t().contiguous().view(-1).to(torch.uint8), x.device)   # one decision per row of [B * T, D]
        x = F.replace_mix(x, q.to(x.dtype), sel, self.final_dropout.p, self.training)
        if self.proj is not None:
            x = head_logits(x, self.proj)                                           # [B, T, C], batch-first storage
        if tbc:
            x = x.transpose(0, 1)                                                   # T x B x C view: wavlm_ctc_loss reads it in place
        return {"contrastive_res": res, "encoder_out": x, "encoder_padding_mask": padding_mask, "padding_mask": padding_mask,
                "replace_mat": replace_mat}

    def max_positions(self):
        return None


class Unispeech(nn.Module):
    """Unispeech (unispeech.py:36-67).  State-dict keys are the reference's: w2v_encoder.w2v_model.*, w2v_encoder.proj.{weight, bias};
    parameters are created in its order (the inner model, then proj with xavier weight and zero bias), so a seeded construction
    gives the reference's initial values.  target_dictionary: an object with __len__ (fairseq's Dictionary, ctc.LetterDictionary),
    a task that has one as .target_dictionary, or the number of classes; None builds no head.

    forward(source, padding_mask, tbc=True) returns contrastive_res (the inner model's result), encoder_out (T x B x C: a view
    of batch-first storage), encoder_padding_mask, padding_mask, and replace_mat (the bool [T, B] decisions, on the host).
    The replace decisions are drawn on the host exactly as the reference draws them -- torch.bernoulli on the CPU generator,
    after the inner forward's draws -- and, like the reference, in eval mode as well: validation mixes quantised rows in too."""

    def __init__(self, cfg, target_dictionary=None):
        if not hasattr(self, "_modules"):   # (the fairseq plugin mixes this class in front of BaseFairseqModel)
            nn.Module.__init__(self)
        self.cfg = cfg
        d = getattr(target_dictionary, "target_dictionary", target_dictionary)
        self.w2v_encoder = Wav2VecEncoder(cfg, d if (d is None or isinstance(d, int)) else len(d))

    @classmethod
    def build_model(cls, cfg, task=None):
        return cls(cfg, task)

    def upgrade_state_dict_named(self, state_dict, name):
        return state_dict

    def max_positions(self):
        return None

    def set_num_updates(self, num_updates):
        """reaches the quantiser's temperature schedule (the reference's generic set_num_updates walks the modules)"""
        self.w2v_encoder.set_num_updates(num_updates)

    def get_normalized_probs(self, net_output, log_probs, sample=None):
        logits = net_output["encoder_out"].float()
        return torch.log_softmax(logits, dim=-1) if log_probs else torch.softmax(logits, dim=-1)

    def forward(self, source=None, padding_mask=None, **kwargs):
        return self.w2v_encoder(source=source, padding_mask=padding_mask, **kwargs)

    def remove_pretraining_modules(self):
        self.w2v_encoder.proj = None


def _val(v):
    return float(v.item()) if torch.is_tensor(v) else float(v)


class UnispeechCriterion(nn.Module):
    """UnispeechCriterion (criterions/unispeech_criterion.py): one forward of the model, the CTC loss on encoder_out (when
    mtlalpha > 0) and the InfoNCE loss on contrastive_res, loss = mtlalpha * ctc + (1 - mtlalpha) * infonce, sample_size the
    InfoNCE one, and the nested logging dict {loss, ntokens, nsentences, ctc: {...}, infonce: {...}}.  target_dictionary and
    blank_idx / pad_idx / eos_idx as for ctc.CtcCriterion."""

    def __init__(self, target_dictionary=None, mtlalpha=0.5, infonce=False, loss_weights=None, log_keys=None, zero_infinity=False,
                 sentence_avg=False, post_process="letter", *, blank_idx=None, pad_idx=None, eos_idx=None, task=None):
        if not hasattr(self, "_modules"):
            nn.Module.__init__(self)
        self.mtlalpha = float(mtlalpha)
        self.w2v_criterion = Wav2vecCriterion(task, infonce, loss_weights, log_keys)
        if self.mtlalpha > 0:
            self.ctc_criterion = CtcCriterion(target_dictionary, zero_infinity, sentence_avg, post_process, blank_idx=blank_idx,
                                              pad_idx=pad_idx, eos_idx=eos_idx)

    def forward(self, model, sample, reduce=True):
        net_output = model(**sample["net_input"])
        if self.mtlalpha > 0.0:
            ctc_loss, _, ctc_log = self.ctc_criterion.get_loss(model, sample, net_output, reduce)
        else:
            ctc_loss, ctc_log = 0.0, {}
        nce_loss, sample_size, nce_log = self.w2v_criterion.get_loss(model.w2v_encoder.w2v_model, sample,
                                                                     net_output["contrastive_res"], reduce)
        loss = self.mtlalpha * ctc_loss + (1.0 - self.mtlalpha) * nce_loss
        counts = ctc_log if ctc_log else nce_log     # (mtlalpha == 0: the reference raises KeyError here)
        log = {"loss": float(loss.detach()), "ntokens": counts["ntokens"], "nsentences": counts["nsentences"], "ctc": ctc_log,
               "infonce": nce_log}
        return loss, sample_size, log

    @staticmethod
    def logging_outputs_can_be_summed() -> bool:
        return False

    @staticmethod
    def reduce_metrics(logging_outputs, log_scalar=None, log_derived=None):
        """unispeech_criterion.py:57-142; returns the aggregated values and logs them through the two callbacks when given
        (fairseq's metrics.log_scalar / log_derived).  ctc_loss / nll_loss are left out when no CTC sample was logged
        (mtlalpha == 0), where the reference divides by zero."""
        ln2 = math.log(2)
        ctc = [log.get("ctc", {}) for log in logging_outputs]
        nce = [log.get("infonce", {}) for log in logging_outputs]

        def tot(logs, k):
            return sum(_val(l.get(k, 0)) for l in logs)

        loss_sum = tot(logging_outputs, "loss")
        c_loss, c_ss, c_ntok = tot(ctc, "loss"), tot(ctc, "sample_size"), tot(ctc, "ntokens")
        n_loss, n_ss, n_nsent = tot(nce, "loss"), tot(nce, "sample_size"), tot(nce, "nsentences")
        err = {k: tot(ctc, k) for k in ("c_errors", "c_total", "w_errors", "wv_errors", "w_total")}
        correct, total = tot(nce, "correct"), tot(nce, "count")
        out = {"loss": loss_sum}
        scal = [("loss", loss_sum, 1, 3)]                                            # (key, value, weight, round)
        if c_ss > 0:
            out["ctc_loss"] = c_loss / c_ss / ln2
            scal.append(("ctc_loss", out["ctc_loss"], c_ss, 3))
        out["contrastive_loss"] = n_loss / n_ss / ln2
        scal.append(("contrastive_loss", out["contrastive_loss"], n_ss, 3))
        if c_ss != c_ntok and c_ntok > 0:
            out["nll_loss"] = c_loss / c_ntok / ln2
            scal.append(("nll_loss", out["nll_loss"], c_ntok, 3))
        for k, v in err.items():
            out["_" + k] = v
            scal.append(("_" + k, v, 1, None))
        if err["c_total"] > 0:
            out["uer"] = err["c_errors"] * 100.0 / err["c_total"]
        if err["w_total"] > 0:
            out["wer"] = err["w_errors"] * 100.0 / err["w_total"]
            out["raw_wer"] = err["wv_errors"] * 100.0 / err["w_total"]
        out.update(nsentences=n_nsent, ctc_sample_size=c_ss, contrastive_sample_size=n_ss, _correct=correct, _total=total)
        scal += [("nsentences", n_nsent, 1, None), ("ctc_sample_size", c_ss, 1, None), ("contrastive_sample_size", n_ss, 1, None),
                 ("_correct", correct, 1, None), ("_total", total, 1, None)]
        if total > 0:
            out["accuracy"] = correct / total
        builtin = {"loss", "ntokens", "nsentences", "sample_size", "correct", "count"}
        for k in nce[0]:
            if k not in builtin:
                v = tot(nce, k) / len(logging_outputs)
                if k.startswith("loss"):
                    out[k] = v / n_ss / ln2
                    scal.append((k, out[k], n_ss, None))
                else:
                    out[k] = v
                    scal.append((k, v, 1, 3))
        if log_scalar is not None:
            for k, v, w, r in scal:
                log_scalar(k, v, w, round=r)
        if log_derived is not None:
            def ratio(num, den, scale, digits):
                return lambda meters: (round(meters[num].sum * scale / meters[den].sum, digits) if meters[den].sum > 0
                                       else float("nan"))
            if err["c_total"] > 0:
                log_derived("uer", ratio("_c_errors", "_c_total", 100.0, 3))
            if err["w_total"] > 0:
                log_derived("wer", ratio("_w_errors", "_w_total", 100.0, 3))
                log_derived("raw_wer", ratio("_wv_errors", "_w_total", 100.0, 3))
            if total > 0:
                log_derived("accuracy", ratio("_correct", "_total", 1.0, 5))
        return out
