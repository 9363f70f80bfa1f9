"""CTC forced alignment (csrc/ctc_align.hip, additive to ABI 30): which frames belong to which token and word of a transcript.

  forced_align_reference   float64 numpy: the specification of the kernel, itself checked against brute force by the tests
  forced_align             wavlm_ctc_align on the device: (frames, spans, token_scores, score); no CPU fallback
  timesteps                the `timesteps` of examples/speech_recognition/w2l_decoder.py:243-262 (get_timesteps) for the output of
                           any decoder -- greedy_decode, beam_decode, lexicon_beam_decode: the hypothesis is aligned and the first
                           frame of each of its tokens is returned
  word_segments            letter spans merged into words at the `|` separator (ctc.word_classes), in frames and in seconds
  python -m unispeech_amd.ctc_align CKPT DICT MANIFEST.tsv LABELS.ltr [--out FILE] [--tokens] [--max-samples N]
                           CTM lines `utt 1 start duration word confidence` for the transcripts of a manifest

The rules.  l' is the extended target (blank, l_0, blank, ..., l_(L-1), blank), S = 2 L + 1, x[t, c] the RAW logits of a sample, Tb
its input length, skip(s) = s odd and l'_s != l'_(s-2).  In float64:
    v_0(s) = x[0, l'_s] for s < 2, -inf otherwise
    v_t(s) = max(v_(t-1)(s), v_(t-1)(s-1), v_(t-1)(s-2) if skip(s)) + x[t, l'_s]
    end    = the better of v_(Tb-1)(S-1) and v_(Tb-1)(S-2)
The log-softmax is not needed to find the path: every path takes exactly one class per frame, so subtracting lse[t] shifts all of
them alike.  max is exact and each v is one float64 addition of the same two operands on the host and on the device, so the
kernel's path is this module's bit for bit, for fp32 and for bf16 logits.
Ties: among equal predecessors the one with the larger s wins (stay over s - 1 over s - 2) and at the end S - 1 wins over S - 2 --
of all best paths, the one whose state sequence read from the last frame to the first is lexicographically greatest.  torchaudio's
forced_align differs at the terminal tie only (it prefers S - 2 there).
Outputs per sample: frames[t] = the index j of the label frame t emits, -1 for a blank frame, -2 for t >= Tb; spans[j] = (first
frame, one past the last frame) of label j; token_scores[j] = the sum of lp[t, l_j] over the label's frames and score = the sum
of lp over all Tb frames of the path, both in ascending t in float64 (the device rounds them to fp32 once), lp = x - lse.
No alignment (Tb < L + the number of adjacent equal labels): score -inf, frames -2 throughout, spans -1, token_scores 0.  Tb = 0:
score 0 for L = 0, -inf otherwise.  A label outside [0, C): score NaN, the rest as without an alignment.  Rows at or beyond Tb
are never read.
"""
import argparse
import collections
import math
import os
import sys

import numpy as np
import torch

from . import ctc as _ctc

ALIGN_BLOCK = 32      # include/wavlm_hip.h WAVLM_CTC_ALIGN_BLOCK: frames of back-pointers the back-trace stages into LDS at a time

Alignment = collections.namedtuple("Alignment", ["frames", "spans", "token_scores", "score"])
WordSegment = collections.namedtuple("WordSegment", ["word", "start_frame", "end_frame", "score", "start", "end", "confidence"])


def _host_logits(logits):
    if torch.is_tensor(logits):
        return logits.detach().float().cpu().numpy()
    return np.asarray(logits)


def _input_lengths(input_lengths, T, B):
    if input_lengths is None:
        return [T] * B
    il = [min(max(int(v), 0), T) for v in _ctc._host_ints(input_lengths, "input_lengths")]
    if len(il) != B:
        raise ValueError("input_lengths: expected B = %d values" % B)
    return il


# ------------------------------------------------------------------------------------------------ float64 restatement
def forced_align_reference(logits, targets, input_lengths, target_lengths, blank=0):
    """The rules of this module's docstring on the host.  logits [T, B, C] (numpy or a host tensor; bf16 is widened exactly);
    targets flat or padded [B, Lmax] with target_lengths, as ctc_reference takes them.  Returns Alignment(frames int32 [B, T],
    spans int32 [B, Lmax, 2], token_scores float64 [B, Lmax], score float64 [B]) with Lmax the longest target."""
    x = _host_logits(logits).astype(np.float64)
    T, B, C = x.shape
    labels = _ctc._flat_targets(targets, target_lengths)
    il = _input_lengths(input_lengths, T, B)
    Lmax = max([len(v) for v in labels] + [0])
    frames = np.full((B, T), -2, dtype=np.int32)
    spans = np.full((B, Lmax, 2), -1, dtype=np.int32)
    token_scores = np.zeros((B, Lmax))
    score = np.full(B, -math.inf)
    NEG = -math.inf
    for b in range(B):
        lab = labels[b]
        L, Tb = len(lab), il[b]
        if any(v < 0 or v >= C for v in lab):
            score[b] = math.nan
            continue
        if Tb == 0:
            score[b] = 0.0 if L == 0 else NEG
            continue
        ext = [blank]
        for v in lab:
            ext += [v, blank]
        ext = np.array(ext)
        S = len(ext)
        xb = x[:Tb, b]
        xe = xb[:, ext]                                                        # x[t, l'_s]
        skip = np.zeros(S, dtype=bool)
        skip[2:] = (np.arange(2, S) % 2 == 1) & (ext[2:] != ext[:-2])
        v = np.full(S, NEG)
        v[:min(S, 2)] = xe[0, :min(S, 2)]
        back = np.zeros((Tb, S), dtype=np.int8)
        for t in range(1, Tb):
            a1 = np.concatenate([[NEG], v[:-1]])
            a2 = np.where(skip, np.concatenate([[NEG, NEG], v[:-2]])[:S], NEG)
            best, code = v.copy(), back[t]
            for k, a in ((1, a1), (2, a2)):                                    # strictly better only: the larger s wins a tie
                m = a > best
                best[m] = a[m]
                code[m] = k
            v = best + xe[t]
        s = S - 1
        if S > 1 and v[S - 2] > v[S - 1]:
            s = S - 2
        if not v[s] > NEG:
            continue                                                           # no alignment: -inf
        path = np.empty(Tb, dtype=np.int64)
        for t in range(Tb - 1, -1, -1):
            path[t] = s
            s -= int(back[t, s])
        m = xb.max(-1)
        lse = m + np.log(np.exp(xb - m[:, None]).sum(-1))
        total = 0.0
        for t in range(Tb):                                                    # ascending t, one addition each
            s = int(path[t])
            lp = float(xe[t, s]) - float(lse[t])
            total += lp
            if s & 1:
                j = s >> 1
                frames[b, t] = j
                if spans[b, j, 0] < 0:
                    spans[b, j, 0] = t
                spans[b, j, 1] = t + 1
                token_scores[b, j] += lp
            else:
                frames[b, t] = -1
        score[b] = total
    return Alignment(frames, spans, token_scores, score)


# ------------------------------------------------------------------------------------------------------------ the device
def forced_align(logits, targets, input_lengths, target_lengths, blank=0):
    """wavlm_ctc_align: logits [T, B, C] on the device, fp32 or bf16 -- the T x B x C view of batch-first storage (the model's
    encoder_out) and T x B x C storage are both read in place; targets, input_lengths (None: T) and target_lengths as
    forced_align_reference takes them, on the host or on the device.  Returns Alignment(frames int32 [B, T], spans int32
    [B, Lmax, 2], token_scores fp32 [B, Lmax], score fp32 [B]) on the device.  There is no CPU fallback: a host tensor, a missing
    library or a refusal of the kernel raises WavlmHipError, a target beyond the kernel's limit NotImplementedError."""
    from . import _lib, ops
    if not (torch.is_tensor(logits) and logits.is_cuda):
        raise _lib.WavlmHipError("forced_align needs a HIP device tensor (no CPU fallback; forced_align_reference is the host's)")
    T, B, C = logits.shape
    tl = _ctc._host_ints(target_lengths, "target_lengths")
    if len(tl) != B:
        raise ValueError("target_lengths: expected B = %d values" % B)
    t = targets.detach().cpu().numpy() if torch.is_tensor(targets) else targets
    labels = _ctc._flat_targets(t, tl)
    Lmax = max(tl + [0])
    ops.ctc_align_check_supported(Lmax)
    il = _input_lengths(input_lengths, T, B)
    dev = logits.device
    flat = [v for lab in labels for v in lab]
    offsets = np.concatenate([[0], np.cumsum(tl)]).astype(np.int32)
    x = logits.detach().transpose(0, 1)
    if x.shape[2] > 1 and x.stride(2) != 1:
        x = x.contiguous()
    out = ops.ctc_align(x, torch.tensor(flat if flat else [0], dtype=torch.int32).to(dev), torch.from_numpy(offsets).to(dev),
                        len(flat), Lmax, torch.tensor(il, dtype=torch.int32).to(dev), blank)
    return Alignment(*out)


# --------------------------------------------------------------------------------------------------------- time stamps
def get_timesteps(token_idxs, blank):
    """w2l_decoder.py:243-262 as it stands: the frame numbers of every non-blank token of a per-frame token path"""
    out = []
    for i, tok in enumerate(token_idxs):
        if tok == blank:
            continue
        if i == 0 or tok != token_idxs[i - 1]:
            out.append(i)
    return out


def frame_tokens(frames, labels, blank):
    """the per-frame classes of an aligned sample (what get_timesteps takes): frames is its row of Alignment.frames"""
    return [int(labels[f]) if f >= 0 else blank for f in (int(v) for v in frames) if f != -2]


def timesteps(logits, input_lengths, hypotheses, blank=0):
    """get_timesteps for hypotheses that come without a frame path: one list of token ids per sample (greedy_decode's output, or
    the tokens of a beam_decode / lexicon_beam_decode hypothesis) -> one list per sample of the first frame of each token on the
    hypothesis's best path through logits [T, B, C], or None where the hypothesis has no alignment (more tokens, counting
    adjacent repeats twice, than frames).  Device logits take the kernel, host logits forced_align_reference."""
    hyps = [[int(v) for v in h] for h in hypotheses]
    tl = [len(h) for h in hyps]
    flat = np.array([v for h in hyps for v in h], dtype=np.int64)
    if torch.is_tensor(logits) and logits.is_cuda:
        a = forced_align(logits, flat, input_lengths, tl, blank)
        spans, score = a.spans.cpu().numpy(), a.score.cpu().numpy()
    else:
        a = forced_align_reference(logits, flat, input_lengths, tl, blank)
        spans, score = a.spans, a.score
    return [[int(v) for v in spans[b, :n, 0]] if math.isfinite(score[b]) else None for b, n in enumerate(tl)]


def frame_stride(conv_feature_layers):
    """samples per frame of a conv feature extractor: the product of its layers' strides (320 for the shipped extractors)"""
    layers = eval(conv_feature_layers) if isinstance(conv_feature_layers, str) else conv_feature_layers
    n = 1
    for _, _, s in layers:
        n *= int(s)
    return n


def word_segments(tokens, spans, token_scores, dictionary, stride=320, sample_rate=16000, each_token=False):
    """Words of one aligned transcript (host).  tokens: its L label ids; spans [L, 2] and token_scores [L]: its rows of an
    Alignment.  Letters are merged into words at the separator `|` as ctc.word_classes(dictionary, ., "letter") classes them
    (tokens the dictionary's string() omits are dropped); each_token: every kept token, the separator included, is a segment of
    its own.  A word runs from its first letter's first frame to one past its last letter's last frame; its score is the sum of
    its letters' scores and its confidence exp(score / the number of frames its letters hold).  Seconds are frames x stride /
    sample_rate, with stride = frame_stride(the model's conv_feature_layers).  Returns a list of WordSegment."""
    tokens = [int(v) for v in tokens]
    n_sym = max([len(dictionary)] + [v + 1 for v in tokens])
    cls = _ctc.word_classes(dictionary, n_sym, "letter")
    if cls is None:
        raise NotImplementedError("word_segments: this dictionary's tokens do not spell its words (ctc.word_classes refuses it)")
    spans = np.asarray(spans).reshape(-1, 2)
    token_scores = np.asarray(token_scores, dtype=np.float64).reshape(-1)
    out, cur = [], None

    def close():
        if cur is not None:
            word, f0, f1, sc, nf = cur
            out.append(WordSegment(word, f0, f1, sc, f0 * stride / sample_rate, f1 * stride / sample_rate, math.exp(sc / nf)))

    for j, tok in enumerate(tokens):
        k = cls[tok]
        if k == _ctc.DROP:
            continue
        f0, f1, sc = int(spans[j, 0]), int(spans[j, 1]), float(token_scores[j])
        if f0 < 0:
            raise ValueError("word_segments: token %d has no span (the sample has no alignment)" % j)
        sym = dictionary.string([tok])
        if each_token:
            cur = (sym, f0, f1, sc, f1 - f0)
            close()
            cur = None
        elif k == _ctc.SEP:
            close()
            cur = None
        elif cur is None:
            cur = (sym, f0, f1, sc, f1 - f0)
        else:
            cur = (cur[0] + sym, cur[1], f1, cur[3] + sc, cur[4] + f1 - f0)
    close()
    return out


def ctm_lines(utt, segments):
    """`utt 1 start duration word confidence` per segment, times in seconds"""
    return ["%s 1 %.3f %.3f %s %.4f" % (utt, s.start, s.end - s.start, s.word, s.confidence) for s in segments]


# ---------------------------------------------------------------------------------------------------------- command line
def parse_args(argv=None):
    p = argparse.ArgumentParser(prog="python -m unispeech_amd.ctc_align", description=__doc__.split("\n\n")[0])
    p.add_argument("ckpt")
    p.add_argument("dict")
    p.add_argument("manifest", help="fairseq manifest: the root directory, then `relpath<TAB>nsamples` per line")
    p.add_argument("labels", help="one line of space-separated symbols per utterance (.ltr)")
    p.add_argument("--out", default=None, metavar="FILE", help="write the CTM there instead of standard output")
    p.add_argument("--tokens", action="store_true", help="one line per token instead of one per word")
    p.add_argument("--max-samples", type=int, default=160 * 16000, metavar="N", help="padded audio samples per batch")
    return p.parse_args(argv)


def align(a):
    from .kmeans import read_wav
    d = _ctc.LetterDictionary.load(a.dict)
    entries = _ctc.read_manifest(a.manifest)
    labels = _ctc.read_labels(a.labels, d, len(entries))
    model, normalize = _ctc.load_ctc_checkpoint(a.ckpt, len(d))
    dtype = next(model.parameters()).dtype
    stride = frame_stride(model.w2v_encoder.w2v_model.cfg.conv_feature_layers)
    lines = [None] * len(entries)
    for batch in _ctc.length_batches([n for _, n in entries], a.max_samples):
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
        with torch.no_grad():
            out = model(source=src.cuda().to(dtype), padding_mask=pm.cuda() if bool(pm.any()) else None)
        il = None if out["padding_mask"] is None else (~out["padding_mask"]).sum(-1)
        tl = [len(labels[i]) for i in batch]
        res = forced_align(out["encoder_out"], np.array([v for i in batch for v in labels[i]], dtype=np.int64), il, tl, d.bos())
        spans, tsc, score = res.spans.cpu().numpy(), res.token_scores.cpu().numpy(), res.score.cpu().numpy()
        for r, i in enumerate(batch):
            utt = os.path.splitext(os.path.basename(entries[i][0]))[0]
            if not math.isfinite(score[r]):
                print("%s: no alignment (score %s): skipped" % (utt, score[r]), file=sys.stderr)
                continue
            segs = word_segments(labels[i], spans[r, :tl[r]], tsc[r, :tl[r]], d, stride, 16000, each_token=a.tokens)
            lines[i] = ctm_lines(utt, segs)
    text = "".join(line + "\n" for ls in lines if ls is not None for line in ls)
    if a.out is None:
        sys.stdout.write(text)
    else:
        with open(a.out, "w", encoding="utf-8") as f:
            f.write(text)
    return 0


def main(argv=None):
    return align(parse_args(argv))


if __name__ == "__main__":
    sys.exit(main())
