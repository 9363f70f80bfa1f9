"""CTC fine-tuning (csrc/ctc.hip, ABI 30): the loss, the criterion and the encoder + CTC head of the reference's ASR recipe --
src/fairseq/criterions/ctc.py, src/fairseq/models/hubert/hubert_asr.py (HubertCtc / HubertEncoder; wav2vec2_asr.py's Wav2VecCtc
is the same wrapper around the other encoder) and the greedy path of src/examples/speech_recognition/infer.py.

  ctc_reference   float64 numpy restatement of the recursion: the oracle of the tests and the documentation of the kernel
  ctc_loss        autograd Function over wavlm_ctc_loss (log-softmax fused, gradient with respect to the logits)
  greedy_decode   argmax / collapse repeats / drop blanks on the device (wavlm_ctc_greedy)
  CtcCriterion    criterions/ctc.py: sum-reduced loss, ntokens / nsentences / sample_size, error counts in eval
  EncoderCtc      hubert_asr.py:138-178, 237-340 around any pre-training model of this package
  error_counts    the validation counts (unit / word edit distances) of a batch: wavlm_ctc_score (csrc/ctc_score.hip), one launch
  beam_decode     lexicon-free beam search with an n-gram unit LM (ctc_lm.NgramLM, an ARPA file): wavlm_ctc_beam
                  (csrc/ctc_beam.hip) on the device, beam_search_reference -- float64, the specification -- on the host
  python -m unispeech_amd.ctc decode CKPT DICT a.wav ...      one greedy transcript per file
  python -m unispeech_amd.ctc score CKPT DICT MANIFEST.tsv LABELS.ltr      UER / WER over a manifest
  either with --lm FILE.arpa [--beam --beam-size-token --beam-threshold --lm-weight --sil-weight --nbest]: the beam search
The lexicon / word-LM decoder (w2l_decoder.py with --lexicon) is unispeech_amd.ctc_lexicon, with a command line of its own:
python -m unispeech_amd.ctc_lexicon {decode,score} ... --lexicon FILE [--lm FILE.arpa]; these two sub-commands take no lexicon.

Not built, refused by name: KenLM's binary format, the criterion's decoder options
(wer_kenlm_model, wer_lexicon, wer_args), reduce=False, and the seq2seq `decoder_*` options: EncoderCtc is the CTC model only.  (The
seq2seq model of wav2vec2_asr.py is unispeech_amd.seq2seq, inference only; training it is not built.  The UniSpeech multitask model
and criterion are unispeech_amd.unispeech; a checkpoint of theirs is fine-tuned through EncoderCtc.build(arch="unispeech").)

Tensors on the host take ctc_reference (loss) and numpy (decode): that path exists for the tests and for tiny inputs.  A device
tensor always takes the kernels, and a kernel that is missing or refuses its arguments is an error, never a detour.  The one
stated exception is error_counts: where word_classes() finds that token spans would not compare as the dictionary's strings do,
or the targets are wider than wavlm_ctc_score_supported allows, the counts come from the host loop -- the same integers.
"""
import argparse
import contextlib
import math
import os
import sys

import numpy as np
import torch
import torch.nn as nn


# ------------------------------------------------------------------------------------------------ float64 restatement
def _lae(*v):
    """log(sum(exp(v_i))) elementwise over float64 arrays; -inf where every term is -inf"""
    v = [np.asarray(x, dtype=np.float64) for x in v]
    m = v[0]
    for x in v[1:]:
        m = np.maximum(m, x)
    mf = np.where(np.isfinite(m), m, 0.0)
    with np.errstate(divide="ignore"):
        return mf + np.log(sum(np.exp(x - mf) for x in v))


def _flat_targets(targets, target_lengths):
    """1-D concatenated targets (2-D padded [B, Lmax] rows are cut to their lengths), as F.ctc_loss takes them"""
    tl = [int(v) for v in np.asarray(target_lengths).reshape(-1)]
    t = np.asarray(targets)
    if t.ndim == 2:
        return [[int(v) for v in t[b, :tl[b]]] for b in range(len(tl))]
    out, o = [], 0
    for n in tl:
        out.append([int(v) for v in t[o:o + n]])
        o += n
    return out


def ctc_reference(logits, targets, input_lengths, target_lengths, blank=0, zero_infinity=False):
    """F.ctc_loss(log_softmax(logits, -1), targets, input_lengths, target_lengths, blank, reduction="none", zero_infinity) and
    the gradient of the SUM of the per-sample losses with respect to the logits, in float64.
    logits [T, B, C]; targets flat or padded [B, Lmax]; returns (loss [B], grad [T, B, C]).

    l' = (blank, l_0, blank, ..., l_(L-1), blank), S = 2 L + 1, lp = log_softmax(logits):
        alpha_0(s)  = lp[0, l'_s] for s < 2, -inf beyond
        alpha_t(s)  = lae(alpha_(t-1)(s), alpha_(t-1)(s-1), alpha_(t-1)(s-2) if s is odd and l'_s != l'_(s-2)) + lp[t, l'_s]
        loss        = -lae(alpha_(Tb-1)(S-1), alpha_(Tb-1)(S-2))
        beta        the same from the last frame backwards (it includes lp[t, l'_s] too)
        grad[t, c]  = exp(lp[t, c]) - sum_{s: l'_s = c} exp(alpha_t(s) + beta_t(s) + loss - lp[t, c])      t < Tb, else 0
    A sample without an alignment has loss +inf and, as in torch, NaN in its rows of the gradient; with zero_infinity both are 0.
    An input length of 0 (which torch does not define) gives 0 for an empty target and +inf otherwise."""
    x = np.asarray(logits, dtype=np.float64)
    T, B, C = x.shape
    m = x.max(-1, keepdims=True)
    lp = x - (m + np.log(np.exp(x - m).sum(-1, keepdims=True)))
    labels = _flat_targets(targets, target_lengths)
    il = [min(max(int(v), 0), T) for v in np.asarray(input_lengths).reshape(-1)]
    loss = np.zeros(B)
    grad = np.zeros((T, B, C))
    NEG = -math.inf
    for b in range(B):
        ext = [blank]
        for v in labels[b]:
            ext += [v, blank]
        S, Tb = len(ext), il[b]
        if Tb == 0:
            loss[b] = 0.0 if S == 1 else math.inf
            if zero_infinity and S > 1:
                loss[b] = 0.0
            continue
        ext = np.array(ext)
        lpe = lp[:Tb, b][:, ext]                                              # lp[t, l'_s]
        skip = np.zeros(S, dtype=bool)
        skip[2:] = (np.arange(2, S) % 2 == 1) & (ext[2:] != ext[:-2])
        pad = np.full(2, NEG)
        alpha = np.full((Tb, S), NEG)
        alpha[0, :min(S, 2)] = lpe[0, :min(S, 2)]
        for t in range(1, Tb):
            a = np.concatenate([pad, alpha[t - 1]])                            # a[s + 2] = alpha_(t-1)(s)
            alpha[t] = _lae(a[2:], a[1:-1], np.where(skip, a[:-2], NEG)) + lpe[t]
        nll = -float(_lae(alpha[Tb - 1, S - 1], alpha[Tb - 1, S - 2] if S > 1 else NEG))
        loss[b] = nll
        if nll == math.inf:
            if zero_infinity:
                loss[b] = 0.0
            else:
                grad[:Tb, b, :] = math.nan
            continue
        skip_fwd = np.zeros(S, dtype=bool)                                     # from s to s + 2
        skip_fwd[:max(S - 2, 0)] = skip[2:]
        beta = np.full((Tb, S), NEG)
        beta[Tb - 1, max(S - 2, 0):] = lpe[Tb - 1, max(S - 2, 0):]
        for t in range(Tb - 2, -1, -1):
            a = np.concatenate([beta[t + 1], pad])
            beta[t] = _lae(a[:-2], a[1:-1], np.where(skip_fwd, a[2:], NEG)) + lpe[t]
        post = np.exp(alpha + beta + nll - lpe)                                # posterior of position s at frame t
        g = np.exp(lp[:Tb, b])
        for t in range(Tb):
            np.subtract.at(g[t], ext, post[t])
        grad[:Tb, b] = g
    return loss, grad


# ------------------------------------------------------------------------------------------------------------- the loss
def _host_ints(v, name):
    if torch.is_tensor(v):
        v = v.detach().cpu().tolist()
    out = [int(i) for i in (v if isinstance(v, (list, tuple)) else np.asarray(v).reshape(-1).tolist())]
    if any(i < 0 for i in out):
        raise ValueError("%s must not be negative" % name)
    return out


class _CtcFn(torch.autograd.Function):
    """nll [B] of a T x B x C logits tensor.  The gradient with respect to the logits is computed ONCE, in forward, by the same
    launch sequence that computes the loss (alpha is there already); backward only multiplies it by the incoming gradient."""

    @staticmethod
    def forward(ctx, logits, targets, offsets, n_targets, Lmax, input_lengths, blank, zero_infinity):
        from . import ops
        x = logits.transpose(0, 1)                                  # the [B, T, C]-indexed view the kernel reads in place
        if x.shape[2] > 1 and x.stride(2) != 1:
            x = x.contiguous()
        nll, dx = ops.ctc_loss_fwd_bwd(x, targets, offsets, n_targets, Lmax, input_lengths, blank, None, zero_infinity)
        ctx.save_for_backward(dx)
        return nll

    @staticmethod
    def backward(ctx, dnll):
        dx, = ctx.saved_tensors
        g = (dx.float() * dnll.to(torch.float32).view(-1, 1, 1)).to(dx.dtype)
        return g.transpose(0, 1), None, None, None, None, None, None, None


class _CtcHostFn(torch.autograd.Function):
    """the same on host tensors through ctc_reference (tests, tiny inputs)"""

    @staticmethod
    def forward(ctx, logits, targets, target_lengths, input_lengths, blank, zero_infinity):
        loss, grad = ctc_reference(logits.detach().to(torch.float64).numpy(), targets, input_lengths, target_lengths, blank,
                                   zero_infinity)
        ctx.save_for_backward(torch.from_numpy(grad))
        ctx.dtype = logits.dtype
        return torch.from_numpy(loss).to(torch.float32 if logits.dtype != torch.float64 else torch.float64)

    @staticmethod
    def backward(ctx, dnll):
        grad, = ctx.saved_tensors
        return (grad * dnll.to(torch.float64).view(1, -1, 1)).to(ctx.dtype), None, None, None, None, None


def ctc_loss(logits, targets, input_lengths, target_lengths, blank=0, reduction="sum", zero_infinity=False):
    """F.ctc_loss(F.log_softmax(logits.float(), -1), targets, input_lengths, target_lengths, blank, reduction, zero_infinity) for
    LOGITS [T, B, C] (fp32 or bf16; a T x B x C view of batch-first storage is read in place, no copy): the log-softmax is
    part of the kernel.  targets: flat [sum(target_lengths)] or padded [B, Lmax].  Returns a 0-dim fp32 tensor ("sum", "mean")
    or [B] ("none").

    The gradient is computed once, in forward, and kept (dlogits: the size of the logits); backward multiplies it by the
    incoming gradient.  Under torch.no_grad() the same launches run (the gradient stage is the one that writes the loss out).
    The target lengths are read on the host (one small copy if they live on the device): the kernel's variant and workspace
    depend on the longest target."""
    if reduction not in ("sum", "mean", "none"):
        raise ValueError("reduction=%r" % (reduction,))
    if logits.dim() != 3:
        raise ValueError("logits: expected [T, B, C]")
    T, B, C = logits.shape
    tl = _host_ints(target_lengths, "target_lengths")
    if len(tl) != B:
        raise ValueError("target_lengths: expected B = %d entries" % B)
    if not logits.is_cuda:
        nll = _CtcHostFn.apply(logits, targets.detach().cpu().numpy() if torch.is_tensor(targets) else targets, tl,
                               _host_ints(input_lengths, "input_lengths"), int(blank), bool(zero_infinity))
    else:
        from . import ops
        dev = logits.device
        Lmax, n = (max(tl) if tl else 0), sum(tl)
        ops.ctc_check_supported(C, Lmax)
        t = torch.as_tensor(targets)
        if t.dim() == 2:
            keep = torch.arange(t.shape[1]).view(1, -1) < torch.tensor(tl).view(-1, 1)
            t = t.to(dev)[keep.to(dev)]
        if t.numel() < n:
            raise ValueError("targets: %d labels, the target lengths sum to %d" % (t.numel(), n))
        t = t.to(device=dev, dtype=torch.int32).contiguous()
        if t.numel() == 0:
            t = torch.zeros(1, dtype=torch.int32, device=dev)
        off = torch.tensor(np.concatenate([[0], np.cumsum(tl)]).astype(np.int32)).to(dev)
        il = torch.as_tensor(input_lengths).to(device=dev, dtype=torch.int32).contiguous()
        if il.numel() != B:
            raise ValueError("input_lengths: expected B = %d entries" % B)
        nll = _CtcFn.apply(logits, t, off, n, Lmax, il, int(blank), bool(zero_infinity))
    if reduction == "none":
        return nll
    if reduction == "mean":     # torch: per-sample loss over its target length (at least 1), then the batch mean
        return (nll / torch.tensor(tl, dtype=nll.dtype, device=nll.device).clamp_min(1)).mean()
    return nll.sum()


# ------------------------------------------------------------------------------------------------------- greedy decode
def greedy_decode(logits, input_lengths=None, blank=0):
    """criterions/ctc.py:200-201 per sample: argmax per frame within the input length (the lowest class among equal maxima),
    unique_consecutive, blanks dropped.  logits [T, B, C]; returns a list of B token lists.  On the device one launch and a copy
    of [B, T] int32 tokens -- never of the [T, B, C] logits; host tensors are decoded with numpy."""
    T, B, C = logits.shape
    if input_lengths is None:
        il = [T] * B
    else:
        il = [min(max(int(v), 0), T) for v in _host_ints(input_lengths, "input_lengths")]
    if torch.is_tensor(logits) and logits.is_cuda:
        from . import ops
        x = logits.detach().transpose(0, 1)
        if x.shape[2] > 1 and x.stride(2) != 1:
            x = x.contiguous()
        tok, cnt = ops.ctc_greedy(x, torch.tensor(il, dtype=torch.int32).to(logits.device), blank)
        tok, cnt = tok.cpu().numpy(), cnt.cpu().numpy()
        return [[int(v) for v in tok[b, :cnt[b]]] for b in range(B)]
    x = logits.detach().float().numpy() if torch.is_tensor(logits) else np.asarray(logits)
    out = []
    for b in range(B):
        arg = x[:il[b], b].argmax(-1) if il[b] else np.zeros(0, dtype=np.int64)   # numpy: the first maximum
        seq, last = [], -1
        for a in arg.tolist():
            if a != last and a != blank:
                seq.append(int(a))
            last = a
        out.append(seq)
    return out


def edit_distance(a, b):
    """Levenshtein distance of two sequences (editdistance.eval of the reference, which is not a dependency here)"""
    a, b = list(a), list(b)
    if len(a) < len(b):
        a, b = b, a
    prev = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        cur = [i]
        for j, y in enumerate(b, 1):
            cur.append(min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (x != y)))
        prev = cur
    return prev[-1]


def post_process(sentence, symbol):
    """fairseq.data.data_utils.post_process for the two settings this path takes"""
    if symbol == "letter":
        return sentence.replace(" ", "").replace("|", " ").strip()
    if symbol is None or symbol == "none":
        return sentence
    raise NotImplementedError("post_process=%r is not implemented ('letter' or None)" % (symbol,))


_post_process = post_process      # for code whose own argument is called post_process


class LetterDictionary:
    """the part of fairseq's Dictionary this path uses: <s> = 0 (the CTC blank), <pad> = 1, </s> = 2, <unk> = 3, then the
    symbols of a `dict.ltr.txt` ("SYMBOL COUNT" per line) in file order"""

    def __init__(self, symbols=()):
        self.symbols = ["<s>", "<pad>", "</s>", "<unk>"] + list(symbols)

    @classmethod
    def load(cls, path):
        with open(path, encoding="utf-8") as f:
            return cls([line.rsplit(" ", 1)[0] for line in f.read().splitlines() if line.strip()])

    def __len__(self):
        return len(self.symbols)

    def bos(self):
        return 0

    def pad(self):
        return 1

    def eos(self):
        return 2

    def unk(self):
        return 3

    def string(self, tokens):
        return " ".join(self.symbols[int(t)] for t in tokens if int(t) not in (0, 1, 2))

    def index(self, symbol):
        """the symbol's id, <unk> for one the dictionary does not have (fairseq's Dictionary.index)"""
        n, ids = self.__dict__.get("_ids", (0, None))
        if n != len(self.symbols):                     # the first of equal symbols, as the file's order has it
            ids = {sym: i for i, sym in reversed(list(enumerate(self.symbols)))}
            self._ids = (len(self.symbols), ids)
        return ids.get(symbol, self.unk())


class _IndexDictionary:
    """stands in when the criterion is given three integers: a token's string is its index"""

    def __init__(self, blank, pad, eos):
        self._b, self._p, self._e = int(blank), int(pad), int(eos)

    def bos(self):
        return self._b

    def pad(self):
        return self._p

    def eos(self):
        return self._e

    def string(self, tokens):
        return " ".join(str(int(t)) for t in tokens)


# ---------------------------------------------------------------------------------------------------------- beam search
BEAM_DEFAULTS = {"beam": 50, "beam_size_token": 100, "beam_threshold": 25.0, "lm_weight": 0.2, "sil_weight": 0.0, "nbest": 1}


def silence_token(dictionary):
    """W2lDecoder.__init__: <sep> if the dictionary has one, else `|`, else eos"""
    syms = getattr(dictionary, "symbols", None)
    if syms is None:
        syms = list(getattr(dictionary, "indices", {}))
    for s in ("<sep>", "|"):
        if s in syms:
            return int(dictionary.index(s))
    return int(dictionary.eos())


def _beam_options(C, beam, beam_size_token, beam_threshold, lm_weight, sil_weight, nbest):
    beam, nbest = int(beam), int(nbest)
    ktok = min(int(beam_size_token), int(C))
    if beam < 1:
        raise ValueError("beam must be at least 1")
    if ktok < 1:
        raise ValueError("beam_size_token must be at least 1")
    if nbest < 1:
        raise ValueError("nbest must be at least 1")
    thr = float(beam_threshold)
    if not thr >= 0.0:
        raise ValueError("beam_threshold must not be negative")
    for name, v in (("lm_weight", lm_weight), ("sil_weight", sil_weight)):
        if not math.isfinite(float(v)):
            raise ValueError("%s must be finite" % name)
    return beam, ktok, thr, float(lm_weight), float(sil_weight), nbest


def beam_search_reference(logits, input_lengths=None, blank=0, sil=-1, lm=None, beam=50, beam_size_token=100, beam_threshold=25.0,
                          lm_weight=0.2, sil_weight=0.0, nbest=1, normalized=False):
    """The lexicon-free CTC beam search in float64: the specification of wavlm_ctc_beam (csrc/ctc_beam.hip) and the host path of
    beam_decode.  logits [T, B, C] (each frame's log-sum-exp is subtracted unless `normalized`); lm: a ctc_lm.NgramLM or None.

    A hypothesis is (score, lm state, last token, prev_blank, back-pointer); the start is (0, state of <s>, none, False).
    Frame t < input_length[b]: the min(beam_size_token, C) best classes by emission (ties to the lower class) are paired with
    every beam entry r in rank order: s = score_r + e[t, n] (+ sil_weight if n is `sil`).  n != blank and (n != last_r or
    prev_blank_r) is a new token: s += lm_weight * lm(state_r, n), the state advances, prev_blank = False.  n == blank keeps the
    state, prev_blank = True.  Otherwise a repeat: the state is kept, prev_blank = False.  Candidates with equal (state, n,
    prev_blank) merge; the best survives, and best everywhere is the total order (score descending, parent rank ascending,
    token ascending).  Everything below best_score - beam_threshold is dropped, the first `beam` in that order are kept, and
    that order is the next frame's rank.  At the end lm_weight * lm(state, </s>) is added, the survivors are re-ranked (ties keep
    their rank) and the first `nbest` are returned, each as the collapse of its frame tokens.  Input length 0: one empty
    hypothesis with the end score alone.

    Returns (hyps, margin, abs_sum): per sample the list of (tokens, score); the smallest score difference that decided a
    merge, a threshold cut, the beam boundary or the order of the returned n-best (inf if nothing was ever decided); and the
    sum of the absolute values of the terms of the 1-best's score."""
    x = logits.detach().to(torch.float64).cpu().numpy() if torch.is_tensor(logits) else np.asarray(logits, dtype=np.float64)
    T, B, C = x.shape
    beam, ktok, thr, lmw, silw, nbest = _beam_options(C, beam, beam_size_token, beam_threshold, lm_weight, sil_weight, nbest)
    il = [T] * B if input_lengths is None else [min(max(int(v), 0), T) for v in _host_ints(input_lengths, "input_lengths")]
    if not 0 <= int(blank) < C:
        raise ValueError("blank = %d is not a class" % blank)
    if lm is not None and len(lm.tok_word) < C:
        raise ValueError("the language model maps %d symbols, the logits have %d classes" % (len(lm.tok_word), C))
    blank, sil = int(blank), int(sil)
    out, margins, sums = [], [], []
    for b in range(B):
        e = x[:il[b], b]
        if not normalized and il[b]:
            m = e.max(-1, keepdims=True)
            e = e - (m + np.log(np.exp(e - m).sum(-1, keepdims=True)))
        if not np.isfinite(e).all():
            raise ValueError("sample %d: the emissions must be finite" % b)
        margin = math.inf
        # (score, state, token, prev_blank, back = (parent's back, token) chain, abs_sum)
        hyps = [(0.0, lm.start if lm is not None else 0, -1, False, None, 0.0)]
        for t in range(il[b]):
            et = e[t]
            toks = sorted(int(c) for c in np.lexsort((np.arange(C), -et))[:ktok])
            cands = {}
            for r, (sc, st, tok, pb, back, ab) in enumerate(hyps):
                for n in toks:
                    v = float(et[n])
                    s, a = sc + v, ab + abs(v)
                    if n == sil:
                        s, a = s + silw, a + abs(silw)
                    st2 = st
                    if n != blank and (n != tok or pb):
                        if lm is not None:
                            l, st2 = lm.score(st, n)
                            s, a = s + lmw * l, a + abs(lmw * l)
                    key = (st2, n)                                   # prev_blank is (n == blank)
                    rank = (-s, r, n)
                    old = cands.get(key)
                    if old is not None:
                        margin = min(margin, abs(old[0][0] - rank[0]))
                    if old is None or rank < old[0]:
                        cands[key] = (rank, (s, st2, n, n == blank, (back, n), a))
            best = -min(v[0][0] for v in cands.values())
            if thr != math.inf:
                margin = min([margin] + [abs(-v[0][0] - (best - thr)) for v in cands.values()])
            keep = sorted((v for v in cands.values() if -v[0][0] >= best - thr), key=lambda v: v[0])
            if len(keep) > beam:
                margin = min(margin, keep[beam - 1][1][0] - keep[beam][1][0])
            hyps = [v[1] for v in keep[:beam]]
        fin = []
        for r, h in enumerate(hyps):
            l = lmw * lm.score_eos(h[1]) if lm is not None else 0.0
            fin.append((-(h[0] + l), r, h, h[5] + abs(l)))
        fin.sort(key=lambda v: v[:2])
        for i in range(min(nbest, len(fin) - 1)):
            margin = min(margin, fin[i + 1][0] - fin[i][0])
        res = []
        for msc, _, h, _ in fin[:nbest]:
            path, back = [], h[4]
            while back is not None:
                path.append(back[1])
                back = back[0]
            seq, last = [], -1
            for a in reversed(path):
                if a != last and a != blank:
                    seq.append(int(a))
                last = a
            res.append((seq, -msc))
        out.append(res)
        margins.append(margin)
        sums.append(fin[0][3])
    return out, margins, sums


def beam_decode(logits, input_lengths, dictionary, lm=None, beam=50, beam_size_token=100, beam_threshold=25.0, lm_weight=0.2,
                sil_weight=0.0, nbest=1, normalized=False, blank=None):
    """Lexicon-free CTC beam search with an optional n-gram unit LM (examples/speech_recognition/w2l_decoder.py's
    W2lKenLMDecoder with --unit-lm and no lexicon; flashlight's LexiconFreeDecoder with log_add=False), by the rules of
    beam_search_reference.  logits [T, B, C], either storage order; lm: a ctc_lm.NgramLM loaded with this dictionary, or None
    (one state, every LM score 0: the 1-best is then the greedy decode).  Returns, per sample, a list of at most nbest
    (tokens, score), best first.

    Device logits take wavlm_ctc_beam (one workgroup per utterance; sizes beyond wavlm_ctc_beam_supported raise
    NotImplementedError naming the argument, before any launch); host logits take the float64 reference.
    Differences from flashlight, both deliberate: the search does not start from last_token = sil, and no final sil is appended
    to the path."""
    T, B, C = logits.shape
    if blank is None:
        blank = dictionary.bos()
    sil = silence_token(dictionary)
    if lm is not None and len(lm.tok_word) < C:
        raise ValueError("the language model maps %d symbols, the logits have %d classes" % (len(lm.tok_word), C))
    if not (torch.is_tensor(logits) and logits.is_cuda):
        return beam_search_reference(logits, input_lengths, blank, sil, lm, beam, beam_size_token, beam_threshold, lm_weight,
                                     sil_weight, nbest, normalized)[0]
    from . import ops
    beam, ktok, thr, lmw, silw, nbest = _beam_options(C, beam, beam_size_token, beam_threshold, lm_weight, sil_weight, nbest)
    nbest = min(nbest, beam)
    dev = logits.device
    x = logits.detach().transpose(0, 1)
    if x.shape[2] > 1 and x.stride(2) != 1:
        x = x.contiguous()
    if input_lengths is None:
        il = torch.full((B,), T, dtype=torch.int32, device=dev)
    else:
        il = torch.as_tensor(input_lengths).to(device=dev, dtype=torch.int32).contiguous()
    tokens, counts, scores, n_hyp = ops.ctc_beam(x, il, blank, sil, lm, beam, ktok, thr, lmw, silw, nbest, normalized)
    tokens, counts, scores, n_hyp = tokens.cpu().numpy(), counts.cpu().numpy(), scores.cpu().numpy(), n_hyp.cpu().numpy()
    return [[([int(v) for v in tokens[b, h, :counts[b, h]]], float(scores[b, h])) for h in range(int(n_hyp[b]))] for b in range(B)]


# --------------------------------------------------------------------------------------------------------- error counts
DROP, SEP, LETTER = 0, 1, 2           # the classes of wavlm_ctc_score's table (include/wavlm_hip.h)
_UNSET = object()


def _known_dictionary(d):
    t = type(d)
    return t in (LetterDictionary, _IndexDictionary) or (t.__name__ == "Dictionary" and t.__module__.startswith("fairseq."))


def word_classes(dictionary, C, post_process="letter"):
    """The uint8 table [C] from which wavlm_ctc_score builds its words -- DROP: dictionary.string() omits the token, SEP: the word
    boundary `|` (under "letter"), LETTER: anything else -- or None when comparing token spans on the device would not be
    exactly what post_process(dictionary.string(...)).split() compares on the host:
      * the dictionary is not a LetterDictionary, an _IndexDictionary or fairseq's Dictionary, or probing it raises;
      * a LETTER's string contains whitespace (or, under "letter", a `|`);
      * two LETTERs share a string; or, under "letter", one LETTER's string is a prefix of another's (words are concatenations
        there: "<" next to "<unk>", or the indices "1" and "12" of an _IndexDictionary, make two token spans one string).
    A dictionary longer than C is probed to its end: a target may name those symbols, and the kernel takes an id beyond C as a
    LETTER compared by value, so they must be LETTERs under the same rules."""
    letter = post_process == "letter"
    if not letter and post_process not in (None, "none"):
        return None
    if not _known_dictionary(dictionary):
        return None
    C = int(C)
    try:
        n = max(C, len(dictionary))
    except TypeError:
        n = C
    tab = np.empty(C, dtype=np.uint8)
    letters = []
    try:
        for i in range(n):
            s = dictionary.string([i])
            if not isinstance(s, str):
                return None
            if s == "":
                k = DROP
            elif letter and s == "|":
                k = SEP
            else:
                if any(ch.isspace() for ch in s) or (letter and "|" in s):
                    return None
                k = LETTER
                letters.append(s)
            if i < C:
                tab[i] = k
            elif k != LETTER:
                return None
    except Exception:
        return None
    letters.sort()
    for a, b in zip(letters, letters[1:]):
        if a == b or (letter and b.startswith(a)):
            return None
    return tab


def _host_counts(logits, input_lengths, targets, dictionary, symbol, blank):
    """the loop of criterions/ctc.py:200-226 on the host: per sample (c_err, c_len, w_err, w_len), and the decodes"""
    T, B = logits.shape[0], logits.shape[1]
    il = None if input_lengths is None else _host_ints(input_lengths, "input_lengths")
    with torch.no_grad():
        decoded = greedy_decode(logits, il, blank)
    labels = torch.as_tensor(targets).detach().cpu()
    pad, eos = dictionary.pad(), dictionary.eos()
    out = np.zeros((B, 4), dtype=np.int64)
    for b, (pred, t) in enumerate(zip(decoded, labels)):
        targ = t[(t != pad) & (t != eos)].tolist()
        targ_words = post_process(dictionary.string(targ), symbol).split()
        pred_words = post_process(dictionary.string(pred), symbol).split()
        out[b] = (edit_distance(pred, targ), len(targ), edit_distance(pred_words, targ_words), len(targ_words))
    return out, decoded


def sample_error_counts(logits, input_lengths, targets, dictionary, post_process="letter", blank=None, *, classes=_UNSET,
                        hypotheses=True):
    """Per sample what error_counts sums: (int64 numpy [B, 4] = c_err, c_len, w_err, w_len; the B greedy decodes as token lists, or
    None with hypotheses=False on the device path, which then copies nothing but the [B, 4] counts to the host).
    logits [T, B, C]; input_lengths [B] or None; targets [B, Lt] padded with the dictionary's pad() / eos().
    classes: word_classes(dictionary, C, post_process) if the caller has it already (as a numpy array or a device tensor)."""
    symbol = None if post_process in (None, "none") else post_process
    _post_process("", symbol)
    if blank is None:
        blank = dictionary.bos()
    T, B, C = logits.shape
    targets = torch.as_tensor(targets)
    if targets.dim() != 2 or targets.shape[0] != B:
        raise ValueError("targets: expected [B, Lt] with B = %d rows" % B)
    device = torch.is_tensor(logits) and logits.is_cuda and os.environ.get("WAVLM_CTC_SCORE_HOST", "") != "1"
    if device:
        from . import ops
        device = ops.ctc_score_supported(T, targets.shape[1])
    if device:
        if classes is _UNSET:
            classes = word_classes(dictionary, C, symbol)
        device = classes is not None
    if not device:
        return _host_counts(logits, input_lengths, targets, dictionary, symbol, blank)
    dev = logits.device
    x = logits.detach().transpose(0, 1)
    if x.shape[2] > 1 and x.stride(2) != 1:
        x = x.contiguous()
    if input_lengths is None:
        il = torch.full((B,), T, dtype=torch.int32, device=dev)
    else:
        il = torch.as_tensor(input_lengths).to(device=dev, dtype=torch.int32).contiguous()
    cls = torch.as_tensor(classes).to(device=dev, dtype=torch.uint8).contiguous()
    t = targets.detach().to(device=dev, dtype=torch.int32).contiguous()
    counts, tokens, token_counts = ops.ctc_score(x, il, t, dictionary.pad(), dictionary.eos(), blank, cls, symbol is None)
    decoded = None
    if hypotheses:
        tok, cnt = tokens.cpu().numpy(), token_counts.cpu().numpy()
        decoded = [[int(v) for v in tok[b, :cnt[b]]] for b in range(B)]
    return counts.cpu().numpy().astype(np.int64), decoded


def error_counts(logits, input_lengths, targets, dictionary, post_process="letter", blank=None, *, classes=_UNSET):
    """The validation counts of criterions/ctc.py:161-226 for one batch: {c_errors, c_total, w_errors, wv_errors, w_total} (unit
    and word edit distances of the greedy decode against the targets and their lengths; wv_errors = w_errors: the KenLM decoder
    is not built).  logits [T, B, C], input_lengths [B] or None, targets [B, Lt] padded; blank defaults to dictionary.bos().

    Device logits take wavlm_ctc_score -- decode, both distances and both lengths in one launch, [B, 4] integers copied back --
    when word_classes() has a table for this dictionary and wavlm_ctc_score_supported(T, Lt) says yes; otherwise, for host
    logits, and under WAVLM_CTC_SCORE_HOST=1, the host loop (greedy_decode + edit_distance per sample).  Both give the same
    integers (target ids are non-negative)."""
    n, _ = sample_error_counts(logits, input_lengths, targets, dictionary, post_process, blank, classes=classes, hypotheses=False)
    c_err, c_len, w_err, w_len = (int(v) for v in n.sum(0))
    return {"wv_errors": w_err, "w_errors": w_err, "w_total": w_len, "c_errors": c_err, "c_total": c_len}


# ------------------------------------------------------------------------------------------------------------ criterion
class CtcCriterion(nn.Module):
    """criterions/ctc.py CtcCriterion.  `target_dictionary`: an object with bos() / pad() / eos() / string() (fairseq's Dictionary,
    LetterDictionary) or a task that has one as .target_dictionary; or blank_idx / pad_idx / eos_idx as integers.  The blank is
    target_dictionary.bos(), as in the reference (index 0 of a fairseq dictionary)."""

    def __init__(self, target_dictionary=None, zero_infinity=False, sentence_avg=False, post_process="letter", *, blank_idx=None,
                 pad_idx=None, eos_idx=None, wer_kenlm_model=None, wer_lexicon=None, wer_args=None):
        # nn.Module.__init__ directly (not super()): in the fairseq plugin this class is mixed in front of FairseqCriterion,
        # whose __init__ takes `task` and is called by the plugin subclass itself
        if not hasattr(self, "_modules"):
            nn.Module.__init__(self)
        for name, v in (("wer_kenlm_model", wer_kenlm_model), ("wer_lexicon", wer_lexicon), ("wer_args", wer_args)):
            if v is not None:
                raise NotImplementedError("%s: the flashlight / KenLM decoder is not built; error counts come from the greedy "
                                          "decode (wv_errors = w_errors)" % name)
        d = getattr(target_dictionary, "target_dictionary", target_dictionary)
        if d is not None:
            if blank_idx is not None or pad_idx is not None or eos_idx is not None:
                raise ValueError("give a dictionary or the three indices, not both")
            self.dictionary = d
        else:
            if blank_idx is None or pad_idx is None or eos_idx is None:
                raise ValueError("CtcCriterion needs a target dictionary or blank_idx, pad_idx and eos_idx")
            self.dictionary = _IndexDictionary(blank_idx, pad_idx, eos_idx)
        self.blank_idx, self.pad_idx, self.eos_idx = self.dictionary.bos(), self.dictionary.pad(), self.dictionary.eos()
        _post_process("", post_process)                 # refuses the other settings by name
        self.post_process = post_process
        self.zero_infinity = bool(zero_infinity)
        self.sentence_avg = bool(sentence_avg)

    def get_net_output(self, model, sample):
        return model(**sample["net_input"])

    def forward(self, model, sample, reduce=True):
        net_output = self.get_net_output(model, sample)
        return self.get_loss(model, sample, net_output, reduce)

    def get_loss(self, model, sample, net_output, reduce=True):
        if not reduce:
            raise NotImplementedError("reduce=False: the criterion returns the sum-reduced loss only")
        logits = net_output["encoder_out"]                                  # T x B x C; the log-softmax is in the kernel
        T, B = logits.shape[0], logits.shape[1]
        if "src_lengths" in sample["net_input"]:
            input_lengths = sample["net_input"]["src_lengths"]
        elif net_output["padding_mask"] is not None:
            input_lengths = (~net_output["padding_mask"]).long().sum(-1)
        else:
            input_lengths = torch.full((B,), T, dtype=torch.long)
        target = sample["target"]
        pad_mask = (target != self.pad_idx) & (target != self.eos_idx)
        targets_flat = target.masked_select(pad_mask)
        target_lengths = sample["target_lengths"] if "target_lengths" in sample else pad_mask.sum(-1)
        tl = _host_ints(target_lengths, "target_lengths")
        loss = ctc_loss(logits, targets_flat, input_lengths, tl, blank=self.blank_idx, reduction="sum",
                        zero_infinity=self.zero_infinity)
        ntokens = sample["ntokens"] if "ntokens" in sample else sum(tl)
        sample_size = target.size(0) if self.sentence_avg else ntokens
        logging_output = {"loss": float(loss.detach()), "ntokens": ntokens, "nsentences": sample["id"].numel(),
                          "sample_size": sample_size}
        if not model.training:
            labels = sample["target_label"] if "target_label" in sample else target
            logging_output.update(error_counts(logits, input_lengths, labels, self.dictionary, self.post_process, self.blank_idx,
                                               classes=self._classes(logits.shape[2], logits.device) if logits.is_cuda else None))
        return loss, sample_size, logging_output

    def _classes(self, C, device):
        """word_classes of this criterion's dictionary for C classes, on `device`: built once (C probes of dictionary.string)"""
        cache = self.__dict__.setdefault("_cls_cache", {})
        key = (int(C), str(device))
        if key not in cache:
            tab = word_classes(self.dictionary, C, self.post_process)
            cache[key] = None if tab is None else torch.from_numpy(tab).to(device)
        return cache[key]

    @staticmethod
    def reduce_metrics(logging_outputs, log_scalar=None, log_derived=None):
        """criterions/ctc.py:236-295; returns the aggregated values, and logs them through the two callbacks when given
        (fairseq's metrics.log_scalar / log_derived)"""
        tot = {k: sum(log.get(k, 0) for log in logging_outputs)
               for k in ("loss", "ntokens", "nsentences", "sample_size", "c_errors", "c_total", "w_errors", "wv_errors", "w_total")}
        out = {"loss": tot["loss"] / max(tot["sample_size"], 1) / math.log(2), "ntokens": tot["ntokens"],
               "nsentences": tot["nsentences"]}
        if tot["sample_size"] != tot["ntokens"]:
            out["nll_loss"] = tot["loss"] / max(tot["ntokens"], 1) / math.log(2)
        if tot["c_total"] > 0:
            out["uer"] = tot["c_errors"] * 100.0 / tot["c_total"]
        if tot["w_total"] > 0:
            out["wer"] = tot["w_errors"] * 100.0 / tot["w_total"]
            out["raw_wer"] = tot["wv_errors"] * 100.0 / tot["w_total"]
        if log_scalar is not None:
            log_scalar("loss", out["loss"], tot["sample_size"], round=3)
            log_scalar("ntokens", tot["ntokens"])
            log_scalar("nsentences", tot["nsentences"])
            if "nll_loss" in out:
                log_scalar("nll_loss", out["nll_loss"], tot["ntokens"], round=3)
            for k in ("c_errors", "c_total", "w_errors", "wv_errors", "w_total"):
                log_scalar("_" + k, tot[k])
        if log_derived is not None:
            def ratio(num, den):
                return lambda meters: (round(meters[num].sum * 100.0 / meters[den].sum, 3) if meters[den].sum > 0
                                       else float("nan"))
            if tot["c_total"] > 0:
                log_derived("uer", ratio("_c_errors", "_c_total"))
            if tot["w_total"] > 0:
                log_derived("wer", ratio("_w_errors", "_w_total"))
                log_derived("raw_wer", ratio("_wv_errors", "_w_total"))
        return out

    @staticmethod
    def logging_outputs_can_be_summed() -> bool:
        return True


# ---------------------------------------------------------------------------------------------------- encoder + CTC head
# HubertAsrConfig (hubert_asr.py:22-130) field -> default.  OPTIONS are read by the wrapper, OVERRIDES are fields of the wrapped
# model's own config (EncoderCtc.build applies them before the model is built, as HubertEncoder's arg_overrides do), the
# rest is refused by name when it is given a value other than its default.
OPTIONS = {"apply_mask": False, "final_dropout": 0.0, "freeze_finetune_updates": 0, "feature_grad_mult": 0.0}
OVERRIDES = {"dropout_input": "dropout_input", "dropout": "dropout", "attention_dropout": "attention_dropout",
             "activation_dropout": "activation_dropout", "mask_length": "mask_length", "mask_prob": "mask_prob",
             "mask_selection": "mask_selection", "mask_other": "mask_other", "no_mask_overlap": "no_mask_overlap",
             "mask_channel_length": "mask_channel_length", "mask_channel_prob": "mask_channel_prob",
             "mask_channel_selection": "mask_channel_selection", "mask_channel_other": "mask_channel_other",
             "no_mask_channel_overlap": "no_mask_channel_overlap", "layerdrop": "encoder_layerdrop"}
REFUSED = {"no_pretrained_weights": False, "normalize": False, "data": None, "w2v_args": None, "w2v_path": None,
           # HubertSeq2SeqConfig / Wav2Vec2Seq2SeqConfig: not this wrapper's (unispeech_amd.seq2seq takes them)
           "decoder_embed_dim": 768, "decoder_ffn_embed_dim": 3072, "decoder_layers": 6, "decoder_layerdrop": 0.0,
           "decoder_attention_heads": 4, "decoder_learned_pos": False, "decoder_normalize_before": False,
           "no_token_positional_embeddings": False, "decoder_dropout": 0.0, "decoder_attention_dropout": 0.0,
           "decoder_activation_dropout": 0.0, "max_target_positions": 2048, "share_decoder_input_output_embed": False}


def _split_options(options, allow_overrides):
    opts, over = dict(OPTIONS), {}
    for k, v in options.items():
        if k in OPTIONS:
            opts[k] = v
        elif k in OVERRIDES:
            if not allow_overrides:
                raise ValueError("%s is a field of the wrapped model's own config: build the model with it, or let "
                                 "EncoderCtc.build apply it" % k)
            over[OVERRIDES[k]] = v
        elif k in REFUSED:
            if v is not None and v != REFUSED[k]:
                raise NotImplementedError("%s=%r is not implemented by EncoderCtc" % (k, v))
        else:
            raise TypeError("EncoderCtc: unknown option %r" % k)
    return opts, over


def head_logits(x, proj):
    """proj(x) through LinearFn for a head whose class count need not be a multiple of 8: the row kernels behind the Linear's
    backward take widths that are multiples of 8, so zero rows are appended to the head for the call and the logits are the
    first C columns of its output (a view; wavlm_ctc_loss reads it in place).  Used by _Encoder and unispeech.Unispeech."""
    from . import functional as F
    W, b = proj.weight, proj.bias
    C = W.shape[0]
    pad = -C % 8
    if pad:
        W = torch.cat([W, W.new_zeros(pad, W.shape[1])])
        b = torch.cat([b, b.new_zeros(pad)])
    x = F.LinearFn.apply(x, W, b)                                                   # [..., C (+ pad)]
    return x[..., :C] if pad else x


class _Encoder(nn.Module):
    """HubertEncoder (hubert_asr.py:237-340): w2v_model, final_dropout, proj"""

    def __init__(self, w2v_model, num_classes, opts):
        super().__init__()
        self.apply_mask = bool(opts["apply_mask"])
        self.w2v_model = w2v_model
        self.w2v_model.feature_grad_mult = float(opts["feature_grad_mult"])     # "reset feature grad mult ... to this"
        self.final_dropout = nn.Dropout(float(opts["final_dropout"]))
        self.freeze_finetune_updates = int(opts["freeze_finetune_updates"])
        self.num_updates = 0
        d = w2v_model.cfg.encoder_embed_dim
        self.proj = nn.Linear(d, int(num_classes))
        nn.init.xavier_uniform_(self.proj.weight)
        nn.init.constant_(self.proj.bias, 0.0)

    def set_num_updates(self, num_updates):
        self.num_updates = num_updates
        if hasattr(self.w2v_model, "set_num_updates"):
            self.w2v_model.set_num_updates(num_updates)

    def forward(self, source, padding_mask=None, tbc=True, **kwargs):
        from . import functional as F
        ft = self.freeze_finetune_updates <= self.num_updates
        # hubert_asr.py:324: no_grad while frozen, otherwise whatever the caller has set (validation stays under its no_grad)
        with contextlib.nullcontext() if ft else torch.no_grad():
            res = self.w2v_model.extract_features(source=source, padding_mask=padding_mask,
                                                  mask=self.apply_mask and self.training)
            x, padding_mask = (res["x"], res["padding_mask"]) if isinstance(res, dict) else res
        x = F.dropout(x, self.final_dropout.p, self.training)
        x = head_logits(x, self.proj)                                               # [B, T, C], batch-first storage
        if tbc:
            x = x.transpose(0, 1)                                                   # T x B x C view: wavlm_ctc_loss reads it in place
        return {"encoder_out": x, "encoder_padding_mask": padding_mask, "padding_mask": padding_mask}


class EncoderCtc(nn.Module):
    """HubertCtc (hubert_asr.py:138-178) == Wav2VecCtc: a pre-training model of this package (WavLMPretrainModel in any of its
    HuBERT / ILS / UniSpeech-SAT forms, Wav2Vec2Model) after remove_pretraining_modules(), final dropout and a Linear to the
    target dictionary.  State-dict keys are the reference's: w2v_encoder.w2v_model.*, w2v_encoder.proj.{weight, bias}.
    options: apply_mask, final_dropout, freeze_finetune_updates, feature_grad_mult (default 0.0 as in HubertAsrConfig: the
    feature extractor is frozen unless asked otherwise)."""

    def __init__(self, w2v_model, num_classes, **options):
        if not hasattr(self, "_modules"):   # (the fairseq plugin mixes this class in front of BaseFairseqModel)
            nn.Module.__init__(self)
        opts, _ = _split_options(options, allow_overrides=False)
        for name in ("final_proj", "label_embs_concat"):
            if getattr(w2v_model, name, None) is not None:
                raise ValueError("call remove_pretraining_modules() on the wrapped model first (%s is still there)" % name)
        self.w2v_encoder = _Encoder(w2v_model, num_classes, opts)

    @classmethod
    def build(cls, w2v_cfg, num_classes, *, arch="wavlm", task_cfg=None, state_dict=None, **options):
        """HubertEncoder.__init__: the pre-training config with the mask / dropout / layerdrop overrides applied, the model
        built from it, its pre-training weights loaded (strict=False: the heads are gone) and its pre-training modules removed.
        arch: "wavlm" (WavLMPretrainModel: wavlm, hubert, ils_hubert, unispeech_sat), "wav2vec2", or "unispeech": a checkpoint of
        the multitask model (unispeech.Unispeech) -- the inner Wav2Vec2Model is built from its config, the keys
        w2v_encoder.w2v_model.* are loaded with the prefix stripped and the pre-training CTC head w2v_encoder.proj.* is dropped
        (wav2vec2_asr.py:365-366, what the recipe's finetune.sh relies on).  The reference leaves the quantiser modules in
        place, unused; here they are removed like every other pre-training module."""
        import dataclasses
        opts, over = _split_options(options, allow_overrides=True)
        over["feature_grad_mult"] = opts["feature_grad_mult"]
        if arch in ("wav2vec2", "unispeech"):
            from .wav2vec2 import Wav2Vec2Config, Wav2Vec2Model
            if arch == "unispeech":
                prefix = "w2v_encoder.w2v_model."
                w2v_cfg = Wav2Vec2Config(**{k: getattr(w2v_cfg, k) for k in Wav2Vec2Config.__dataclass_fields__
                                            if hasattr(w2v_cfg, k)})
                if state_dict is not None:
                    state_dict = {k[len(prefix):]: v for k, v in state_dict.items() if k.startswith(prefix)}
            over = {k: v for k, v in over.items() if k in type(w2v_cfg).__dataclass_fields__}
            model = Wav2Vec2Model(dataclasses.replace(w2v_cfg, **over))
        elif arch == "wavlm":
            from .pretrain import WavLMPretrainModel
            model = WavLMPretrainModel(dataclasses.replace(w2v_cfg, **over), task_cfg, None)
        else:
            raise NotImplementedError("arch=%r (wavlm, wav2vec2 or unispeech)" % (arch,))
        model.remove_pretraining_modules()      # first: the heads' keys (whatever their shapes) are then simply not loaded
        if state_dict is not None:
            model.load_state_dict(state_dict, strict=False)
        return cls(model, num_classes, **opts)

    def set_num_updates(self, num_updates):
        self.w2v_encoder.set_num_updates(num_updates)

    def upgrade_state_dict_named(self, state_dict, name):
        return state_dict

    def max_positions(self):
        return None

    def forward(self, source=None, padding_mask=None, **kwargs):
        return self.w2v_encoder(source=source, padding_mask=padding_mask, **kwargs)

    def get_logits(self, net_output):
        """hubert_asr.py:164-172.  The reference's two assignments go through `logits[padding]`, a boolean-mask index, which
        yields a copy: the padded frames of the returned tensor are NOT changed, and neither are they here."""
        return net_output["encoder_out"]

    def get_normalized_probs(self, net_output, log_probs, sample=None):
        """hubert_asr.py:155-162, for callers other than CtcCriterion (whose kernel has the log-softmax fused)"""
        logits = net_output["encoder_out"].float()
        return torch.log_softmax(logits, dim=-1) if log_probs else torch.softmax(logits, dim=-1)


# ---------------------------------------------------------------------------------------------------------- command line
def load_ctc_checkpoint(path, num_classes):
    """{'cfg': the pre-training config's fields, 'model': EncoderCtc state dict, 'arch': 'wavlm' | 'wav2vec2' (default wavlm),
    'normalize': bool} -> (EncoderCtc on the device in eval mode, normalize)"""
    ck = torch.load(path, map_location="cpu", weights_only=False)
    if not (isinstance(ck, dict) and "cfg" in ck and "model" in ck):
        raise NotImplementedError("%s: only the standalone checkpoint dict {'cfg', 'model'} is loaded" % path)
    arch = ck.get("arch", "wavlm")
    if arch == "wav2vec2":
        from .wav2vec2 import Wav2Vec2Config as Cfg
    else:
        from .pretrain import WavLMPretrainConfig as Cfg
    cfg = Cfg(**{k: v for k, v in dict(ck["cfg"]).items() if k in Cfg.__dataclass_fields__})
    model = EncoderCtc.build(cfg, num_classes, arch=arch)
    model.load_state_dict(ck["model"])
    return model.cuda().eval(), bool(ck.get("normalize", getattr(cfg, "normalize", False)))


def base_parser(prog, description, decode_help="greedy CTC transcripts, one line per file",
                score_help="UER / WER of the greedy decode over a manifest (error_counts per batch)"):
    """(parser, its `decode` sub-parser, its `score` sub-parser) with the positionals and the options that do not concern a
    decoder; unispeech_amd.ctc_lexicon builds its command line on the same"""
    p = argparse.ArgumentParser(prog=prog, description=description)
    sub = p.add_subparsers(dest="cmd", required=True)
    d = sub.add_parser("decode", help=decode_help)
    d.add_argument("ckpt")
    d.add_argument("dict")
    d.add_argument("wavs", nargs="+")
    d.add_argument("--post-process", default="letter", choices=["letter", "none"])
    d.add_argument("--bf16", action="store_true")
    c = sub.add_parser("score", help=score_help)
    c.add_argument("ckpt")
    c.add_argument("dict")
    c.add_argument("manifest", help="fairseq manifest: the root directory, then `relpath<TAB>nsamples` per line")
    c.add_argument("labels", help="one line of space-separated symbols per utterance (.ltr)")
    c.add_argument("--batch-seconds", type=float, default=160.0, help="padded audio per batch, in seconds")
    c.add_argument("--post-process", default="letter", choices=["letter", "none"])
    c.add_argument("--bf16", action="store_true")
    c.add_argument("--results", default=None, metavar="DIR", help="write hypo.units, hypo.word, ref.units, ref.word there")
    return p, d, c


def add_beam_options(q, lm_help):
    q.add_argument("--lm", default=None, metavar="FILE.arpa", help=lm_help)
    q.add_argument("--beam", type=int, default=BEAM_DEFAULTS["beam"])
    q.add_argument("--beam-size-token", type=int, default=BEAM_DEFAULTS["beam_size_token"])
    q.add_argument("--beam-threshold", type=float, default=BEAM_DEFAULTS["beam_threshold"])
    q.add_argument("--lm-weight", type=float, default=BEAM_DEFAULTS["lm_weight"])
    q.add_argument("--sil-weight", type=float, default=BEAM_DEFAULTS["sil_weight"])
    q.add_argument("--nbest", type=int, default=BEAM_DEFAULTS["nbest"])


def refuse_binary_lm(a):
    if a.lm is not None and a.lm.endswith((".bin", ".binary", ".trie")):
        raise NotImplementedError("--lm %s: KenLM's binary format is not read; give the ARPA text file" % a.lm)
    return a


def parse_args(argv=None):
    p, d, c = base_parser("python -m unispeech_amd.ctc", __doc__.split("\n\n")[0])
    for q in (d, c):
        add_beam_options(q, "n-gram unit LM (ARPA text): decode with the beam search")
    return refuse_binary_lm(p.parse_args(argv))


def _beam_kwargs(a):
    return {"beam": a.beam, "beam_size_token": a.beam_size_token, "beam_threshold": a.beam_threshold, "lm_weight": a.lm_weight,
            "sil_weight": a.sil_weight, "nbest": a.nbest}


def read_manifest(path):
    """[(path of the audio file, its number of samples)] of a fairseq manifest"""
    with open(path, encoding="utf-8") as f:
        lines = f.read().splitlines()
    if not lines:
        raise ValueError("%s: empty manifest (line 1 is the root directory)" % path)
    root, out = lines[0].strip(), []
    for no, line in enumerate(lines[1:], 2):
        if not line.strip():
            continue
        parts = line.split("\t")
        if len(parts) < 2 or not parts[1].strip().isdigit():
            raise ValueError("%s:%d: expected `relpath<TAB>nsamples`" % (path, no))
        out.append((os.path.join(root, parts[0]), int(parts[1])))
    return out


def read_labels(path, dictionary, n_utterances=None):
    """one list of token ids per line of a label file (space-separated symbols, no eos appended: the fine-tuning task's
    LabelEncoder); a line count other than the manifest's is refused"""
    with open(path, encoding="utf-8") as f:
        lines = f.read().splitlines()
    if n_utterances is not None and len(lines) != n_utterances:
        raise ValueError("%s: %d label lines, but the manifest lists %d utterances" % (path, len(lines), n_utterances))
    return [[dictionary.index(sym) for sym in line.split()] for line in lines]


def length_batches(sizes, max_samples):
    """indices of the utterances, sorted by length (ties by index) and cut where the batch's padded size -- its longest
    utterance times its count -- would pass max_samples; an utterance longer than that is a batch of its own"""
    order = sorted(range(len(sizes)), key=lambda i: (sizes[i], i))
    out, cur = [], []
    for i in order:                                   # ascending: the newcomer is the batch's longest
        if cur and sizes[i] * (len(cur) + 1) > max_samples:
            out.append(cur)
            cur = []
        cur.append(i)
    if cur:
        out.append(cur)
    return out


def _load_lm(a, dictionary):
    if a.lm is None:
        return None
    from .ctc_lm import NgramLM
    return NgramLM.load(a.lm, dictionary)


def score(a, decoder=None):
    """`score`: the scoring half of examples/speech_recognition/infer.py and compute_WER.py with the greedy decode.
    decoder (the command line of unispeech_amd.ctc_lexicon): (logits, input lengths, dictionary) -> per sample (tokens, words or
    None), in place of the built-in decodes; words that are not None are the hypothesis's words as they stand (infer.py:123-124)"""
    from .kmeans import read_wav
    d = LetterDictionary.load(a.dict)
    symbol = None if a.post_process == "none" else "letter"
    entries = read_manifest(a.manifest)
    labels = read_labels(a.labels, d, len(entries))
    model, normalize = load_ctc_checkpoint(a.ckpt, len(d))
    if a.bf16:
        model = model.to(torch.bfloat16)
    dtype = next(model.parameters()).dtype
    classes = word_classes(d, len(d), symbol)
    lm = _load_lm(a, d) if decoder is None else None
    if lm is not None:
        def decoder(logits, il, d):
            return [(h[0][0] if h else [], None) for h in beam_decode(logits, il, d, lm, **_beam_kwargs(a))]
    total = np.zeros(4, dtype=np.int64)
    hyps, hyp_words = [None] * len(entries), [None] * len(entries)
    for batch in length_batches([n for _, n in entries], int(a.batch_seconds * 16000)):
        wavs = []
        for i in batch:
            wav, sr = read_wav(entries[i][0])
            if sr != 16000:
                raise NotImplementedError("%s: %d Hz; the models take 16 kHz audio (unispeech_amd.resample converts)"
                                          % (entries[i][0], sr))
            x = torch.as_tensor(wav, dtype=torch.float32)
            wavs.append(torch.nn.functional.layer_norm(x, x.shape) if normalize else x)
        n = max(w.numel() for w in wavs)
        src = torch.zeros(len(batch), n)
        pm = torch.ones(len(batch), n, dtype=torch.bool)
        for r, w in enumerate(wavs):
            src[r, :w.numel()] = w
            pm[r, :w.numel()] = False
        Lt = max(1, max(len(labels[i]) for i in batch))
        target = torch.full((len(batch), Lt), d.pad(), dtype=torch.long)
        for r, i in enumerate(batch):
            target[r, :len(labels[i])] = torch.tensor(labels[i], dtype=torch.long)
        with torch.no_grad():
            out = model(source=src.cuda().to(dtype), padding_mask=pm.cuda() if bool(pm.any()) else None)
        logits = out["encoder_out"]
        il = None if out["padding_mask"] is None else (~out["padding_mask"]).sum(-1)
        if decoder is not None:
            # the beam's 1-best through the host edit distance (fusing this into wavlm_ctc_score is not built)
            pairs = decoder(logits, il, d)
            decoded = [pred for pred, _ in pairs]
            counts = np.zeros((len(batch), 4), dtype=np.int64)
            for r, ((pred, words), i) in enumerate(zip(pairs, batch)):
                targ = [v for v in labels[i] if v not in (d.pad(), d.eos())]
                targ_words = post_process(d.string(targ), symbol).split()
                pred_words = post_process(d.string(pred), symbol).split() if words is None else list(words)
                counts[r] = (edit_distance(pred, targ), len(targ), edit_distance(pred_words, targ_words), len(targ_words))
                hyp_words[i] = None if words is None else " ".join(words)
        else:
            counts, decoded = sample_error_counts(logits, il, target, d, symbol, d.bos(), classes=classes,
                                                  hypotheses=a.results is not None)
        total += counts.sum(0)
        if decoded is not None:
            for i, toks in zip(batch, decoded):
                hyps[i] = toks
    c_err, c_len, w_err, w_len = (int(v) for v in total)
    print("UER %.3f%% WER %.3f%% c_errors %d c_total %d w_errors %d w_total %d"
          % (c_err * 100.0 / max(c_len, 1), w_err * 100.0 / max(w_len, 1), c_err, c_len, w_err, w_len))
    if a.results is not None:
        os.makedirs(a.results, exist_ok=True)
        files = {"hypo.units": [], "hypo.word": [], "ref.units": [], "ref.word": []}
        for i, (hyp, ref) in enumerate(zip(hyps, labels)):          # infer.py:120-148, speaker None, id = the utterance's index
            for kind, toks in (("hypo", hyp), ("ref", ref)):
                units = d.string(toks)
                word = hyp_words[i] if kind == "hypo" and hyp_words[i] is not None else post_process(units, symbol)
                files[kind + ".units"].append("%s (None-%d)" % (units, i))
                files[kind + ".word"].append("%s (None-%d)" % (word, i))
        for name, lines in files.items():
            with open(os.path.join(a.results, name), "w", encoding="utf-8") as f:
                f.write("".join(line + "\n" for line in lines))
    return 0


def decode(a, lines=None):
    """`decode`.  lines (the command line of unispeech_amd.ctc_lexicon): (logits of one file, dictionary) -> the lines to print
    for it, in place of the built-in decodes"""
    from .kmeans import read_wav
    d = LetterDictionary.load(a.dict)
    model, normalize = load_ctc_checkpoint(a.ckpt, len(d))
    if a.bf16:
        model = model.to(torch.bfloat16)
    dtype = next(model.parameters()).dtype
    lm = _load_lm(a, d) if lines is None else None
    symbol = None if a.post_process == "none" else "letter"
    for path in a.wavs:
        wav, sr = read_wav(path)
        if sr != 16000:
            raise NotImplementedError("%s: %d Hz; the models take 16 kHz audio (unispeech_amd.resample converts)" % (path, sr))
        x = torch.as_tensor(wav, dtype=torch.float32).cuda()
        if normalize:
            x = torch.nn.functional.layer_norm(x, x.shape)
        with torch.no_grad():
            out = model(source=x.view(1, -1).to(dtype), padding_mask=None)
        if lines is not None:
            for line in lines(out["encoder_out"], d):
                print(line)
            continue
        if lm is not None:                      # one line per hypothesis, best first; with --nbest above 1 the score in front
            for toks, sc in beam_decode(out["encoder_out"], None, d, lm, **_beam_kwargs(a))[0]:
                text = post_process(d.string(toks), symbol)
                print(text if a.nbest == 1 else "%.4f\t%s" % (sc, text))
            continue
        toks = greedy_decode(out["encoder_out"], None, d.bos())[0]
        print(post_process(d.string(toks), symbol))
    return 0


def main(argv=None):
    a = parse_args(argv)
    return score(a) if a.cmd == "score" else decode(a)


if __name__ == "__main__":
    sys.exit(main())
